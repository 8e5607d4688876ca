#!/usr/bin/env python3
"""Filtered search timed.  GPU box only.  Writes profiles/filter/filter_bench.json and prints the same JSON line.
Filters are random keep-bitmaps at --keep fractions (1 %, 50 %, 100 % of the documents), seeded.  --reps timed calls after a
warm-up; every value is listed.
  (1) the build: ns_segment_filter's passes (HIP events inside the call, summed by Engine::open_filter) and the whole open_filter
      (skip tables and the row table included) on cfg5's index (bench.py's: one generated segment of 1 M documents) and, with
      --mb > 0, on tools/ingest_bench.py's seeded corpus of that many MB indexed as ONE segment.  Bytes: 8 B (mark) + 12 B
      (scatter read) per posting + 12 B per kept posting (write), as a share of the 8 TB/s roofline.  The baseline is the
      one-thread host restatement of the same compaction (numpy: mask, prefix sum, gather of postings and norms, list ranks).
  (2) filtered search: search_filtered_batch of cfg5's 16 384 queries at each fraction against search_batch of the same queries,
      alternating in the same loop.  The keep-all filter is the control: the same postings without packed / impact streams.
  (3) latency: one search_filtered to JSON on an LRU hit and on a miss (the miss builds the filter).
--profile: the filter builds only, for a `rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROOFLINE_BPS = 8e12


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": list(xs)}


def random_bits(eng, frac, seed):
    rng = np.random.default_rng(seed)
    out = []
    for s in range(eng.num_segments):
        n = eng.segment_info(s)["n_docs"]
        keep = np.ones(n, bool) if frac >= 1.0 else rng.random(n) < frac
        out.append(np.packbits(np.concatenate([keep, np.zeros((-n) % 32, bool)]), bitorder="little").view(np.uint32).copy())
    return out


def host_compaction(post, pnorm, keep, starts, counts):
    """the compaction on one host thread: mask, prefix sum, gather, list ranks"""
    t0 = time.perf_counter()
    stays = keep[post[:, 0]]
    rank = np.concatenate([[0], np.cumsum(stays, dtype=np.int64)])
    out_p, out_n = post[stays], pnorm[stays]
    noff, ncnt = rank[starts] * 8, rank[starts + counts] - rank[starts]
    return time.perf_counter() - t0, len(out_p), int(noff[-1]) + int(ncnt[-1]) + len(out_n)


def build_section(eng, fracs, reps, what):
    n_post = sum(eng.segment_info(s)["n_postings"] for s in range(eng.num_segments))
    post = eng.segment_postings(0)
    n_docs = eng.segment_info(0)["n_docs"]
    pnorm = np.zeros(len(post), np.float32)
    starts = np.sort(np.random.default_rng(1).integers(0, max(len(post) - 64, 1), 50000)).astype(np.int64)
    counts = np.full(len(starts), 64, np.int64)
    rows = []
    for frac in fracs:
        bits = random_bits(eng, frac, 7)
        eng.close_filter(eng.open_filter(bits=bits))                      # warm-up: code objects
        dev, tot, st = [], [], None
        for _ in range(reps):
            h, st = eng.open_filter(bits=bits, stats=True)
            eng.close_filter(h)
            dev.append(st["device_ms"])
            tot.append(st["total_ms"])
        med = statistics.median(dev) * 1e-3
        nbytes = 20 * st["postings_total"] + 12 * st["postings_kept"]
        keep = np.unpackbits(bits[0].view(np.uint8), bitorder="little")[:n_docs].astype(bool)
        host_s, host_kept, _ = host_compaction(post, pnorm, keep, starts, counts)
        rows.append({"keep": frac, "docs_kept": st["docs_kept"], "postings_kept": st["postings_kept"], "postings_total": st["postings_total"],
                     "hbm_bytes": st["hbm_bytes"], "passes_device_ms": summary(dev), "open_filter_ms": summary(tot),
                     "algorithmic_bytes": nbytes, "bytes_per_s": nbytes / med, "fraction_of_8TBps": nbytes / med / ROOFLINE_BPS,
                     "host_one_thread_s_segment0": host_s, "host_kept_segment0": host_kept, "passes_over_host": host_s / med})
    return {"what": what, "segments": eng.num_segments, "docs": sum(eng.segment_info(s)["n_docs"] for s in range(eng.num_segments)),
            "postings": n_post, "reps": reps, "builds": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024, help="also time the build on the seeded text corpus of this many MB (0: skip)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keep", type=float, nargs="*", default=[0.01, 0.5, 1.0])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import nsbind
    import workloads
    gen, n_q, K, flags, (nseg, docs) = workloads.WORKLOADS["cfg5"]
    tmp = tempfile.mkdtemp(prefix="ns_filter_idx_")
    out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "reps": args.reps}
    try:
        index = os.path.join(tmp, "cfg5")
        nsbind.gen_index(index, nseg, docs, 65536, 1337, False)
        with open(os.path.join(index, "metadata.csv"), "w") as f:        # dates for the JSON call: a year per document
            f.write("cord_uid,publish_time\n" + "".join("u%08d,%d\n" % (i, 2000 + i % 20) for i in range(nseg * docs)))
        eng = nsbind.Engine(index, 0)
        out["cfg5_build"] = build_section(eng, args.keep, args.reps, "cfg5's index (generated, one segment)")
        if args.profile:
            eng.close()
            print(json.dumps({"profile": True, "builds": (args.reps + 1) * len(args.keep)}))
            return
        # ---- (2) filtered search against the unfiltered search of the same queries ----
        queries = gen()
        rows = []
        for frac in args.keep:
            h = eng.open_filter(bits=random_bits(eng, frac, 7))
            eng.search_filtered_batch(h, queries, K, flags)
            eng.search_batch(queries, K, flags)
            fl, un = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                eng.search_filtered_batch(h, queries, K, flags)
                fl.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                eng.search_batch(queries, K, flags)
                un.append(time.perf_counter() - t0)
            eng.close_filter(h)
            rows.append({"keep": frac, "filtered_s": summary(fl), "unfiltered_s": summary(un), "filtered_over_unfiltered": statistics.median(fl) / statistics.median(un)})
        out["search"] = {"what": "search_filtered_batch against search_batch, cfg5's queries, alternating; wall clock through the Python bindings",
                         "queries": len(queries), "k": K, "rows": rows}
        # ---- (3) latency of one search_filtered to JSON ----
        q = queries[0]
        hit, miss = [], []
        for i in range(args.reps + 1):
            t0 = time.perf_counter()
            eng.search_filtered_json(q, K, str(2000 + i), str(2001 + i))     # a filter not asked before: a miss
            m = time.perf_counter() - t0
            t0 = time.perf_counter()
            eng.search_filtered_json(q, K, str(2000 + i), str(2001 + i))     # the same again: a hit
            hh = time.perf_counter() - t0
            if i:
                miss.append(m * 1e3)
                hit.append(hh * 1e3)
        out["latency_ms"] = {"what": "one search_filtered to JSON; a miss builds the filter (2 of 20 years kept)", "hit": summary(hit), "miss": summary(miss)}
        eng.close()
        if args.mb > 0:
            from ingest_bench import corpus
            texts = corpus(args.mb << 20, 11)
            cidx = os.path.join(tmp, "corpus")
            os.makedirs(cidx)
            ceng = nsbind.Engine.create(cidx, 0)
            ceng.add_documents([(b"u%d" % j, b"t", b"p", d) for j, d in enumerate(texts)])
            del texts
            out["corpus_build"] = build_section(ceng, args.keep, args.reps, "the seeded text corpus of %d MB as one segment" % args.mb)
            ceng.close()
        os.makedirs(os.path.join(ROOT, "profiles", "filter"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "filter", "filter_bench.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
