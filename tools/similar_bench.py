#!/usr/bin/env python3
"""More like this timed on tools/ingest_bench.py's seeded corpus of about --mb MB as ONE segment (one
Engine::add_documents).  GPU box only.  Writes profiles/similar/similar_bench_<mb>mb.json and prints the same JSON line.
  (a) selection alone: ns_docterms_select over EVERY document of the segment, HIP events inside the call; documents/s,
      pairs/s and the fraction of the 8 TB/s roofline counting 8 B per pair read plus 8 B per gathered term entry (df + idf).
      The baseline is the same selection by the one-thread host restatement (nsh_similar_select_host).
  (b) Engine::similar_batch of --sources sources against Engine::search_batch (search_batch_flat behind it) of the same
      queries handed in as TEXT with K + 1: the capability the engine had before; the ratio is reported, and the selection's
      share of the call.
  (c) latency: one Engine::more_like_this to JSON, median over --latency-reps different uids.
--profile: the selection calls only, for a `rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import ctypes as C
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from ingest_bench import corpus  # noqa: E402
import invert_oracle  # noqa: E402

ROOFLINE_BPS = 8e12


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sources", type=int, default=16384)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--latency-reps", type=int, default=200)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import nsbind
    L = nsbind.hip_lib()
    t0 = time.perf_counter()
    docs = corpus(args.mb << 20, 11)
    text_mb = sum(len(d) for d in docs) / 1e6
    print(f"# generated {text_mb:.0f} MB in {len(docs)} documents, {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    tmp = tempfile.mkdtemp(prefix="ns_similar_idx_")
    try:
        index = os.path.join(tmp, "index")
        os.makedirs(index)
        eng = nsbind.Engine.create(index, 0)
        t0 = time.perf_counter()
        eng.add_documents([(b"u%d" % j, b"t", b"p", d) for j, d in enumerate(docs)])
        print(f"# indexed in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        del docs
        seg = os.path.join(index, "segments", eng.segment_name(0))
        counts, pairs = invert_oracle.read_forward(os.path.join(seg, "forward.bin"))
        part = {"counts": counts, "pairs": pairs}
        df, idf = eng.similar_term_stats(0)
        n_docs, n_pairs = len(counts), len(pairs)
        out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "text_mb": text_mb, "docs": n_docs, "terms": len(df), "pairs": n_pairs,
               "reps": args.reps, "max_pairs_of_a_document": int(counts.max()), "doc_cut": int(L.ns_docterms_doc_cut())}
        # ---- (a) selection alone, on a context of its own ----
        ctx = C.c_void_p()
        if L.ns_ctx_create(0, C.byref(ctx)) != 0:
            sys.exit("no device: " + L.ns_last_error(None).decode())
        t0 = time.perf_counter()
        dt = nsbind.DocTerms(ctx, part, df, idf)
        upload_s = time.perf_counter() - t0
        every = np.arange(n_docs, dtype=np.uint32)
        dt.select(every, 25)                                             # warm-up: code objects, pool block
        ms, call = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            term, w, cnt, m = dt.select(every, 25, garbage=False)
            call.append(time.perf_counter() - t0)
            ms.append(m)
        if args.profile:
            dt.close()
            L.ns_ctx_destroy(ctx)
            eng.close()
            print(json.dumps({"profile": True, "reps": args.reps + 1, "docs": n_docs, "pairs": n_pairs}))
            return
        med = statistics.median(ms) * 1e-3
        t0 = time.perf_counter()
        h_term, h_w, h_cnt = nsbind.similar_select_host(part, df, idf, every, 25)
        host_s = time.perf_counter() - t0
        same = bool(np.array_equal(term, h_term) and np.array_equal(w.view(np.uint32), h_w.view(np.uint32)) and np.array_equal(cnt, h_cnt))
        out["selection"] = {"what": "ns_docterms_select over every document, T = 25, default options; device ms = HIP events around the kernels",
                            "upload_s": upload_s, "device_ms": summary(ms), "call_s": summary(call), "docs_per_s": n_docs / med, "pairs_per_s": n_pairs / med,
                            "algorithmic_bytes": 16 * n_pairs, "fraction_of_8TBps": 16.0 * n_pairs / med / ROOFLINE_BPS,
                            "host_one_thread_s": host_s, "host_pairs_per_s": n_pairs / host_s, "device_over_host": host_s / med,
                            "call_over_host": host_s / statistics.median(call), "equals_host_restatement": same}
        dt.close()
        L.ns_ctx_destroy(ctx)
        # ---- (b) similar_batch against the text search of the same queries ----
        rng = np.random.default_rng(5)
        K = nsbind.similar_clamp_k(args.k)
        src = [(0, int(d)) for d in rng.integers(0, n_docs, args.sources)]
        terms = eng.similar_batch(src, K, terms=True)[4]                 # warm-up; builds the device copy
        queries = [b" ".join(t for t, _ in row).decode() for row in terms]
        eng.search_batch(queries, K + 1)
        ids = np.asarray([d for _, d in src], dtype=np.uint32)
        sim, txt, sel = [], [], []
        ctx2 = C.c_void_p()
        L.ns_ctx_create(0, C.byref(ctx2))
        dt2 = nsbind.DocTerms(ctx2, part, df, idf)
        dt2.select(ids, 25)
        for _ in range(args.reps):
            t0 = time.perf_counter()
            eng.similar_batch(src, K)
            sim.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            eng.search_batch(queries, K + 1)
            txt.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            m = dt2.select(ids, 25, garbage=False)[3]
            sel.append({"call_s": time.perf_counter() - t0, "device_ms": m})
        dt2.close()
        L.ns_ctx_destroy(ctx2)
        s_med, t_med = statistics.median(sim), statistics.median(txt)
        out["batch"] = {"what": "Engine::similar_batch of the sources against Engine::search_batch (K + 1) of the same queries as text; wall clock through the Python bindings",
                        "sources": len(src), "k": K, "terms_per_query": sum(len(r) for r in terms) / len(terms),
                        "similar_batch_s": summary(sim), "text_search_s": summary(txt), "similar_over_text": s_med / t_med,
                        "selection_call_s": summary([x["call_s"] for x in sel]), "selection_device_ms": summary([x["device_ms"] for x in sel]),
                        "selection_share_of_similar_batch": statistics.median([x["call_s"] for x in sel]) / s_med}
        # ---- (c) latency of one more_like_this ----
        lat = []
        for d in rng.integers(0, n_docs, args.latency_reps):
            t0 = time.perf_counter()
            eng.more_like_this_json(b"u%d" % int(d), K)
            lat.append(time.perf_counter() - t0)
        out["latency"] = {"what": "one Engine::more_like_this(uid, k) to JSON; the uid lookup walks every document's uid on the host",
                          "ms": {"median": statistics.median(lat) * 1e3, "min": min(lat) * 1e3, "max": max(lat) * 1e3, "n": len(lat)}}
        eng.close()
        os.makedirs(os.path.join(ROOT, "profiles", "similar"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "similar", "similar_bench_%dmb.json" % args.mb), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
