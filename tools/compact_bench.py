#!/usr/bin/env python3
"""Compaction timed on tools/ingest_bench.py's seeded corpus of about --mb MB cut into --parts batches.
GPU box only.  Legs, alternating, medians and every single figure reported:
  one_shot    the only way back to one segment without compaction: ns_forward_build over the whole text, fetch,
              ns_invert_forward
  compact     ns_forward_merge over the batches' forward indexes (as their segments hold them), fetch, ns_forward_invert;
              with the in-place document sort (ns_ctx_use_docsort 1) and with the four radix passes (0)
  host        the one-thread C++ restatement of the merge (tools/compact_host_baseline.cpp), no inversion
  search      (--search-mb > 0) an index fed with add_documents in --parts batches, and a copy of it compacted: the same query
              batch through search_batch on both, queries per second.  The answers differ legitimately (idf per segment).
--profile: warm-up and --reps merges of each kind only, for a `rocprofv3 --kernel-trace --stats` run of its own.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ingest_bench import corpus  # noqa: E402


def checksum(counts, pairs):
    doc = np.repeat(np.arange(1, len(counts) + 1, dtype=np.uint64), counts)
    return int((doc * np.uint64(1000003) + pairs[:, 0].astype(np.uint64) * np.uint64(7919) + pairs[:, 1].astype(np.uint64)).sum(dtype=np.uint64))


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--parts", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--search-mb", type=int, default=0)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import nsbind
    L = nsbind.hip_lib()
    t0 = time.perf_counter()
    docs = corpus(args.mb << 20, 11)
    per = (len(docs) + args.parts - 1) // args.parts
    batches = [docs[i:i + per] for i in range(0, len(docs), per)]
    print(f"# generated {sum(len(d) for d in docs) / 1e6:.0f} MB in {len(docs)} documents, {len(batches)} batches, {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    ctx = C.c_void_p()
    if L.ns_ctx_create(0, C.byref(ctx)) != 0:
        sys.exit("no device: " + L.ns_last_error(None).decode())
    parts = [nsbind.forward_build(ctx, b) for b in batches]
    arr, keep = nsbind.forward_sources(parts)
    blob = b"".join(docs)
    offs = np.zeros(len(docs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.fromiter((len(d) for d in docs), dtype=np.uint64, count=len(docs)))
    info = nsbind.NsForwardInfo(struct_size=C.sizeof(nsbind.NsForwardInfo))

    def fetch(h):
        L.ns_forward_get_info(h, C.byref(info))
        dl, cnt = (np.zeros(info.kept_docs, dtype=np.uint32) for _ in range(2))
        pairs = np.zeros((info.n_pairs, 2), dtype=np.uint32)
        tb, to = np.zeros(max(1, info.term_bytes), dtype=np.uint8), np.zeros(info.n_terms + 1, dtype=np.uint64)
        if L.ns_forward_fetch(h, None, dl.ctypes.data, cnt.ctypes.data, pairs.ctypes.data, tb.ctypes.data, to.ctypes.data) != 0:
            sys.exit("ns_forward_fetch: " + L.ns_last_error(ctx).decode())
        return cnt, pairs

    def one_shot():
        h, kept, ms = C.c_void_p(), C.c_uint64(), C.c_float()
        t = time.perf_counter()
        if L.ns_forward_build(ctx, blob, len(blob), offs.ctypes.data, len(offs) - 1, C.byref(h)) != 0:
            sys.exit("ns_forward_build: " + L.ns_last_error(ctx).decode())
        cnt, pairs = fetch(h)
        build_ms, n_terms = info.device_ms, info.n_terms
        L.ns_forward_destroy(h)
        df, post = np.zeros(n_terms, dtype=np.uint32), np.zeros((len(pairs), 2), dtype=np.uint32)
        if L.ns_invert_forward(ctx, cnt.ctypes.data, len(cnt), pairs.ctypes.data, len(pairs), n_terms, df.ctypes.data, post.ctypes.data, C.byref(kept), C.byref(ms)) != 0:
            sys.exit("ns_invert_forward: " + L.ns_last_error(ctx).decode())
        return {"call_s": time.perf_counter() - t, "build_ms": build_ms, "invert_ms": ms.value, "check": checksum(cnt, pairs),
                "post": int(post[:, 0].astype(np.uint64).sum()), "terms": n_terms, "pairs": len(pairs)}

    def compact(inplace, invert=True):
        h, kept, ms = C.c_void_p(), C.c_uint64(), C.c_float()
        L.ns_ctx_use_docsort(ctx, 1 if inplace else 0)
        t = time.perf_counter()
        if L.ns_forward_merge(ctx, arr, len(parts), C.byref(h)) != 0:
            sys.exit("ns_forward_merge: " + L.ns_last_error(ctx).decode())
        merge_s = time.perf_counter() - t
        cnt, pairs = fetch(h)
        merge_ms, n_terms, dev_bytes = info.device_ms, info.n_terms, info.device_bytes
        post = np.zeros((len(pairs), 2), dtype=np.uint32)
        if invert:
            df = np.zeros(n_terms, dtype=np.uint32)
            if L.ns_forward_invert(h, df.ctypes.data, post.ctypes.data, C.byref(kept), C.byref(ms)) != 0:
                sys.exit("ns_forward_invert: " + L.ns_last_error(ctx).decode())
        call_s = time.perf_counter() - t
        L.ns_forward_destroy(h)
        return {"call_s": call_s, "merge_call_s": merge_s, "merge_ms": merge_ms, "invert_ms": ms.value, "check": checksum(cnt, pairs),
                "post": int(post[:, 0].astype(np.uint64).sum()), "terms": n_terms, "pairs": len(pairs), "device_bytes": dev_bytes}

    compact(True)                                                      # warm-up: code objects, pool blocks
    compact(False)
    if args.profile:
        for _ in range(args.reps):
            compact(True, invert=False)
            compact(False, invert=False)
        print(json.dumps({"profile": True, "reps": args.reps, "pairs": int(sum(len(p["pairs"]) for p in parts))}))
        return
    one_shot()
    one, on, off = [], [], []
    for _ in range(args.reps):
        one.append(one_shot())
        on.append(compact(True))
        off.append(compact(False))
    host = []
    if args.host_reps:
        tmp = tempfile.mkdtemp(prefix="ns_compact_")
        exe, pf = os.path.join(tmp, "compact_host_baseline"), os.path.join(tmp, "parts.bin")
        subprocess.check_call(["g++", "-O3", "-std=c++17", os.path.join(ROOT, "tools", "compact_host_baseline.cpp"), "-o", exe])
        with open(pf, "wb") as f:
            f.write(struct.pack("<I", len(parts)))
            for p in parts:
                f.write(struct.pack("<IIQ", len(p["counts"]), len(p["terms"]), len(p["pairs"])))
                f.write(p["counts"].tobytes())
                f.write(np.ascontiguousarray(p["pairs"]).tobytes())
                f.write(b"".join(struct.pack("<I", len(t)) + t for t in p["terms"]))
        host = [json.loads(subprocess.check_output([exe, pf]).decode()) for _ in range(args.host_reps)]
        shutil.rmtree(tmp)
    L.ns_ctx_destroy(ctx)
    med = statistics.median
    pairs = on[0]["pairs"]
    out = {"text_mb": len(blob) / 1e6, "parts": len(parts), "docs": int(sum(len(p["counts"]) for p in parts)), "terms_in": int(sum(len(p["terms"]) for p in parts)),
           "terms": on[0]["terms"], "pairs": pairs, "merge_device_bytes_per_pair": on[0]["device_bytes"] / max(1, pairs),
           "one_shot": {"build_ms": summary([r["build_ms"] for r in one]), "invert_ms": summary([r["invert_ms"] for r in one]), "call_s": summary([r["call_s"] for r in one]),
                        "includes": "ns_forward_build over the whole text (upload, device part), fetch, ns_invert_forward (upload, device part, postings back)"},
           "compact_inplace": {"merge_ms": summary([r["merge_ms"] for r in on]), "invert_ms": summary([r["invert_ms"] for r in on]),
                               "merge_call_s": summary([r["merge_call_s"] for r in on]), "call_s": summary([r["call_s"] for r in on]),
                               "includes": "ns_forward_merge (upload, device part), fetch, ns_forward_invert (device part, postings back)"},
           "compact_radix": {"merge_ms": summary([r["merge_ms"] for r in off]), "invert_ms": summary([r["invert_ms"] for r in off]),
                             "merge_call_s": summary([r["merge_call_s"] for r in off]), "call_s": summary([r["call_s"] for r in off])},
           "same_result": len({(r["check"], r["post"], r["terms"], r["pairs"]) for r in one + on + off}) == 1}
    dev_one = med([r["build_ms"] + r["invert_ms"] for r in one])
    dev_on = med([r["merge_ms"] + r["invert_ms"] for r in on])
    out["device_part_one_shot_over_compact"] = dev_one / dev_on
    out["call_one_shot_over_compact"] = med([r["call_s"] for r in one]) / med([r["call_s"] for r in on])
    out["merge_ms_radix_over_inplace"] = med([r["merge_ms"] for r in off]) / med([r["merge_ms"] for r in on])
    if host:
        h_s = med([h["seconds"] for h in host])
        out["host_single_thread"] = {"s": h_s, "all_s": [h["seconds"] for h in host], "kind": "std::unordered_map term walk + remap + std::sort inside each document; no inversion"}
        out["same_result_as_host"] = host[0]["check"] == on[0]["check"] and host[0]["terms"] == on[0]["terms"] and host[0]["pairs"] == pairs
        out["merge_device_part_speedup_vs_host"] = h_s / (med([r["merge_ms"] for r in on]) * 1e-3)
        out["merge_call_speedup_vs_host"] = h_s / med([r["merge_call_s"] for r in on])
    if args.search_mb:
        out["search"] = search_leg(nsbind, args, parts[0]["terms"])
    print(json.dumps(out))


def search_leg(nsbind, args, terms):
    docs = corpus(args.search_mb << 20, 11)
    per = (len(docs) + args.parts - 1) // args.parts
    tmp = tempfile.mkdtemp(prefix="ns_compact_idx_")
    a, b = os.path.join(tmp, "segments16"), os.path.join(tmp, "compacted")
    os.makedirs(a)
    eng = nsbind.Engine.create(a, 0)
    for i in range(0, len(docs), per):
        eng.add_documents([(b"u%d" % j, b"t", b"p", docs[j]) for j in range(i, min(i + per, len(docs)))])
    shutil.copytree(a, b)
    eng_b = nsbind.Engine(b, 0)
    st = eng_b.compact()
    rng = np.random.default_rng(3)
    pool = [t.decode() for t in terms[:20000] if len(t) <= 16]
    queries = [" ".join(pool[int(min(len(pool) - 1, rng.zipf(1.2) - 1))] for _ in range(int(rng.integers(1, 4)))) for _ in range(args.queries)]
    rate = {"segments": [], "compacted": []}
    for e in (eng, eng_b):
        e.set_cache(False)
        e.search_batch(queries, 10, 0)
    for _ in range(5):
        for name, e in (("segments", eng), ("compacted", eng_b)):
            t = time.perf_counter()
            e.search_batch(queries, 10, 0)
            rate[name].append(len(queries) / (time.perf_counter() - t))
    n_seg = eng.num_segments
    eng.close()
    eng_b.close()
    shutil.rmtree(tmp)
    return {"text_mb": args.search_mb, "segments": n_seg, "queries": len(queries), "k": 10, "compact_stats": st,
            "queries_per_s_segments": summary(rate["segments"]), "queries_per_s_compacted": summary(rate["compacted"]),
            "compacted_over_segments": statistics.median(rate["compacted"]) / statistics.median(rate["segments"])}


if __name__ == "__main__":
    main()
