#!/usr/bin/env python3
"""Prefix terms timed on cfg5's index (bench.py's: one generated segment of 1 M documents).  GPU box only.  Writes
<--dir>/<--out>.json (default profiles/prefix/prefix_bench.json) and prints the same JSON line.
    union     ns_segment_union of ONE group of 2, 16, 128 and 1024 members, the most frequent terms of the index, on a context of
              its own: device ms of the call (every kernel of the round between two events), member postings per second (what
              k_un_add's global atomics sustain together with the table's clear, mark, scan and scatter), and the one-thread host
              restatement of the same union (numpy: concatenate, bincount with weights, nonzero), whose arrays the device's must equal
    rounds    16 groups of 16 members under the default scratch and under scratch of one table: what a round costs
    search    Engine::search_prefixed_after_batch over cfg5's 16 384 queries with the first term of each turned into a prefix (its
              last byte cut: ten generated terms), against Engine::search_boosted_after_batch of the same queries with that term
              replaced by the prefix's most frequent expansion; the two alternate in one loop; K = 10; wall ms and reported device ms
              (the prefixed call's includes its unions)
    latency   one Engine::search_prefixed to JSON, per query, over 100 queries
--only union: the union part alone (for a rocprofv3 --kernel-trace --stats run of its own).  No threshold is fixed in advance."""
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


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": list(xs)}


def host_union(flat, firsts, counts, n_docs):
    """one thread: the rule on the host -> (docIds, tfs)"""
    parts = [flat[a:a + c] for a, c in zip(firsts, counts)]
    every = np.concatenate(parts)
    every = every[every[:, 0] < n_docs]
    table = np.bincount(every[:, 0], weights=every[:, 1], minlength=n_docs).astype(np.uint32)
    docs = np.flatnonzero(table).astype(np.uint32)
    return docs, table[docs]


def union_part(nsbind, eng, rounds, out):
    L = nsbind.hip_lib()
    info = eng.segment_info(0)
    n_docs = info["n_docs"]
    flat = eng.segment_postings(0)
    doc_len = np.ascontiguousarray(eng.segment_doc_len(0), dtype=np.uint32)
    terms, scores, _ = eng.suggest_table()
    order = np.argsort(-scores.astype(np.int64), kind="stable")
    lists = []
    for i in order:
        lk = eng.lookup(0, terms[int(i)].decode())
        if lk and lk["df"]:
            lists.append((lk["byte_off"] // 8, lk["count"]))
        if len(lists) == 1024:
            break
    ctx, seg = C.c_void_p(), C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(ctx)) == 0
    payload = np.ascontiguousarray(flat, dtype=np.uint32)
    assert L.ns_segment_upload(ctx, 0, n_docs, C.c_float(info["avgdl"]), doc_len.ctypes.data, payload.ctypes.data, payload.nbytes, C.byref(seg)) == 0, L.ns_last_error(ctx)
    rows = []
    try:
        for m in (2, 16, 128, 1024):
            firsts, counts = [a for a, _ in lists[:m]], [c for _, c in lists[:m]]
            off, cnt, gb = np.array(firsts, np.uint64) * 8, np.array(counts, np.uint32), np.array([0, m], np.uint32)
            t0 = time.perf_counter()
            w_docs, w_tfs = host_union(flat, firsts, counts, n_docs)
            host_ms = (time.perf_counter() - t0) * 1e3
            h, noff, ncnt, written, n_rounds, _, got = nsbind.segment_union(ctx, seg, 1, off, cnt, gb, n_docs=n_docs)
            assert L.ns_segment_release(ctx, h) == 0
            assert written == len(w_docs) and np.array_equal(got[:, 0], w_docs) and np.array_equal(got[:, 1], w_tfs), m
            ms = []
            for _ in range(rounds):
                h, _, _, _, _, t, _ = nsbind.segment_union(ctx, seg, 1, off, cnt, gb)
                assert L.ns_segment_release(ctx, h) == 0
                ms.append(t)
            postings = int(cnt.sum(dtype=np.uint64))
            rows.append({"members": m, "member_postings": postings, "union_postings": int(written), "rounds": n_rounds, "device_ms": summary(ms),
                         "member_postings_per_s": postings / (statistics.median(ms) * 1e-3), "host_one_thread_ms": host_ms,
                         "host_over_device": host_ms / statistics.median(ms)})
        out["union"] = rows
        # what a round costs: 16 groups of 16 members, all tables at once and one table a round
        off = np.array([a for a, _ in lists[:256]], np.uint64) * 8
        cnt = np.array([c for _, c in lists[:256]], np.uint32)
        gb = np.arange(0, 257, 16, dtype=np.uint32)
        per = []
        for scratch in (0, 4 * n_docs):
            nsbind.ctx_union_scratch(ctx, scratch)
            ms, n_rounds = [], 0
            for _ in range(rounds + 1):
                h, _, _, _, n_rounds, t, _ = nsbind.segment_union(ctx, seg, 1, off, cnt, gb)
                assert L.ns_segment_release(ctx, h) == 0
                ms.append(t)
            per.append({"scratch_bytes": scratch or (64 << 20), "rounds": n_rounds, "member_postings": int(cnt.sum(dtype=np.uint64)), "device_ms": summary(ms[1:])})
        nsbind.ctx_union_scratch(ctx, 0)
        out["rounds_ab"] = per
    finally:
        L.ns_segment_release(ctx, seg)
        L.ns_ctx_destroy(ctx)


def search_part(nsbind, eng, queries, rounds, out):
    terms = [[w for w, _ in nsbind.parse_boolean(q)] for q in queries]
    best = {}

    def most_frequent(prefix):
        if prefix not in best:
            ex, _ = eng.expand_prefix(prefix)
            best[prefix] = (max(ex, key=lambda t: (eng.lookup(0, t) or {"df": 0})["df"]) if ex else prefix + "zz", len(ex))
        return best[prefix]

    pre, plain, n_exp = [], [], []
    for ws in terms:
        if not ws or len(ws[0]) < 3:
            pre.append(" ".join(ws)); plain.append(" ".join(ws))
            continue
        p = ws[0][:-1]
        word, n = most_frequent(p)
        n_exp.append(n)
        pre.append(" ".join([p + "*"] + ws[1:]))
        plain.append(" ".join([word] + ws[1:]))
    K = 10
    a = eng.search_prefixed_after_batch(pre, K, timing=True)                       # warm-up; the answers
    b = eng.search_boosted_after_batch(plain, K, timing=True)
    t = {k: [] for k in ("prefixed_wall", "prefixed_device", "boosted_wall", "boosted_device")}
    for _ in range(rounds):
        t0 = time.perf_counter()
        t["prefixed_device"].append(eng.search_prefixed_after_batch(pre, K, timing=True)[-1])
        t["prefixed_wall"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        t["boosted_device"].append(eng.search_boosted_after_batch(plain, K, timing=True)[-1])
        t["boosted_wall"].append((time.perf_counter() - t0) * 1e3)
    out["search"] = {"queries": len(queries), "k": K, "distinct_prefixes": len(best), "expansions_per_prefix": summary(n_exp)["median"],
                     "found_prefixed": int(np.sum(a[2], dtype=np.uint64)), "found_boosted": int(np.sum(b[2], dtype=np.uint64)),
                     **{k + "_ms": summary(v) for k, v in t.items()},
                     "prefixed_over_boosted_wall": statistics.median(t["prefixed_wall"]) / statistics.median(t["boosted_wall"])}
    lat = []
    for q in pre[:100]:
        t0 = time.perf_counter()
        eng.search_prefixed_json(q, 10)
        lat.append((time.perf_counter() - t0) * 1e3)
    out["latency_one_search_prefixed_ms"] = summary(lat)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--dir", default=os.path.join(ROOT, "profiles", "prefix"))
    ap.add_argument("--out", default="prefix_bench")
    args = ap.parse_args()
    assert args.rounds >= 3
    import nsbind
    import workloads
    gen, n_q, _, _, (nseg, docs) = workloads.WORKLOADS["cfg5"]
    tmp = tempfile.mkdtemp(prefix="ns_prefix_idx_")
    out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "rounds": args.rounds}
    try:
        index = os.path.join(tmp, "cfg5")
        nsbind.gen_index(index, nseg, docs, 65536, 1337, False)
        eng = nsbind.Engine(index, 0)
        eng.set_cache(False)
        out["n_docs"] = eng.segment_info(0)["n_docs"]
        out["n_postings"] = eng.segment_info(0)["n_postings"]
        union_part(nsbind, eng, args.rounds, out)
        if args.only != "union":
            queries = gen()
            assert len(queries) == n_q
            search_part(nsbind, eng, queries, args.rounds, out)
        eng.close()
        os.makedirs(args.dir, exist_ok=True)
        with open(os.path.join(args.dir, args.out + ".json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
