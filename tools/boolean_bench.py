#!/usr/bin/env python3
"""Boolean queries timed.  GPU box only.  Writes profiles/boolean/<--out>.json and prints the same JSON line.
On cfg5's index and batch (bench.py's: one generated segment of 1 M documents, 16 384 queries of 1 - 8 terms), --reps timed
calls after a warm-up; every value is listed.  Four role mixes of the same batch at K = 10 and K = 100:
  (a) every term SHOULD                      yardstick: the scoring launch under NS_FLAG_OR  (identical answers, asserted)
  (b) every term MUST                        yardstick: the scoring launch under NS_FLAG_AND (identical answers, asserted)
  (c) the first term MUST, the rest SHOULD   yardstick: ns_search_sorted on the OR batch, which cuts and marks the same lists
  (d) as (a), the last term turned into NOT  yardstick: as (c)
Per mix: the kernels' HIP-event time split into k_bq_select and k_bq_join (summed over the sub-batches), the whole call through
the Python binding (query preparation included), the yardstick's kernel time in the same loop, alternating, and the ratios.
Then one search_boolean call against one search call (cache off), both to JSON.
The window of k_bq_select is the loaded library's: the product's kBqWinDocs, or NS_BOOL_WIN_DOCS in the variants build
(NS_HIP_LIB=.../libnextsearch_hip_variants.so NS_BOOL_WIN_DOCS=16384 tools/boolean_bench.py --out boolean_bench_win16384)."""
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


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": list(xs)}


def same_answers(a, b):
    """(hits, nhits, found, has) twice -> the number of queries whose answers differ in any bit"""
    bad = 0
    for q in range(len(a[1])):
        n = int(a[1][q])
        ok = bool(a[3][q]) == bool(b[3][q]) and n == int(b[1][q]) and (not a[3][q] or int(a[2][q]) == int(b[2][q]))
        ok = ok and np.array_equal(a[0][q, :n].view(np.uint8), b[0][q, :n].view(np.uint8))
        bad += not ok
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--out", default="boolean_bench")
    args = ap.parse_args()
    import nsbind
    import workloads
    gen, n_q, _, _, (nseg, docs) = workloads.WORKLOADS["cfg5"]
    tmp = tempfile.mkdtemp(prefix="ns_boolean_idx_")
    out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "reps": args.reps, "tile_docs": nsbind.facet_tile_docs(),
           "NS_BOOL_WIN_DOCS": os.environ.get("NS_BOOL_WIN_DOCS", "")}
    mismatches = {}
    try:
        index = os.path.join(tmp, "cfg5")
        nsbind.gen_index(index, nseg, docs, 65536, 1337, False)
        with open(os.path.join(index, "metadata.csv"), "w") as f:        # tools/sorted_bench.py's dates: the sorted yardstick is the one measured there
            f.write("cord_uid,publish_time\n" + "".join(
                "u%08d,%s\n" % (i, "" if i % 16 == 5 else "%04d-%02d-%02d" % (1975 + (i * 7919) % 49, 1 + (i * 31) % 12, 1 + (i * 17) % 28))
                for i in range(nseg * docs)))
        eng = nsbind.Engine(index, 0)
        queries = gen()
        assert len(queries) == n_q
        words = [q.split() for q in queries]
        mixes = {
            "a_all_should": queries,
            "b_all_must": [" ".join("+" + w for w in ws) for ws in words],
            "c_first_must": [" ".join(("+" if i == 0 else "") + w for i, w in enumerate(ws)) for ws in words],
            "d_last_not": [" ".join(("-" if i == len(ws) - 1 and len(ws) > 1 else "") + w for i, w in enumerate(ws)) for ws in words],
        }
        _, refs, _ = eng.build_refs(queries)
        out["postings"] = int(refs["count"].sum(dtype=np.uint64))
        rows = []
        for K in [int(x) for x in args.ks.split(",")]:
            b_or, b_and = eng.prepare(queries, K, 0), eng.prepare(queries, K, nsbind.NS_FLAG_AND)
            try:
                eng.search_sorted_batch(queries, K, "newest")                                   # warm-up: builds the key tables
                for name, qs in mixes.items():
                    yard = {"a_all_should": "scoring_or", "b_all_must": "scoring_and"}.get(name, "sorted_or")
                    got = eng.search_boolean_batch(qs, K)                                       # warm-up
                    if yard == "scoring_or":
                        mismatches[(name, K)] = same_answers(got, eng.search_batch(queries, K, 0))
                    elif yard == "scoring_and":
                        mismatches[(name, K)] = same_answers(got, eng.search_batch(queries, K, nsbind.NS_FLAG_AND))
                    nsbind.boolean_kernel_ms(reset=True)
                    dev, split, whole, other = [], [], [], []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        r = eng.search_boolean_batch(qs, K, timing=True)
                        whole.append((time.perf_counter() - t0) * 1e3)
                        dev.append(r[-1])
                        split.append(nsbind.boolean_kernel_ms(reset=True))
                        if yard == "sorted_or":
                            other.append(eng.search_sorted_batch(queries, K, "newest", timing=True)[-1])
                        else:
                            b = b_or if yard == "scoring_or" else b_and
                            b.run(timed=True)
                            b.sync()
                            other.append(float(b.info().last_score_kernel_ms))
                    rows.append({"k": K, "mix": name, "usable_queries": int(got[3].sum()), "matched_documents": int(got[2].sum()),
                                 "hits_returned": int(got[1].sum()), "boolean_kernels_ms": summary(dev),
                                 "k_bq_select_ms": summary([s[0] for s in split]), "k_bq_join_ms": summary([s[1] for s in split]),
                                 "search_boolean_batch_python_ms": summary(whole), "yardstick": yard, "yardstick_kernels_ms": summary(other),
                                 "boolean_kernels_over_yardstick": statistics.median(dev) / statistics.median(other),
                                 "queries_that_differ_from_the_yardstick": mismatches.get((name, K))})
            finally:
                b_or.close()
                b_and.close()
        out["batch"] = {"what": "cfg5's 16 384 queries on cfg5's index; boolean search and its yardstick alternating", "queries": n_q, "rows": rows}
        eng.set_cache(False)
        K = 10
        eng.search_boolean_json(mixes["c_first_must"][0], K)
        eng.search_json(queries[0], K)
        sb, se = [], []
        for i in range(args.reps):
            t0 = time.perf_counter()
            eng.search_boolean_json(mixes["c_first_must"][1 + i], K)
            sb.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            eng.search_json(queries[1 + i], K)
            se.append((time.perf_counter() - t0) * 1e3)
        out["latency_ms"] = {"what": "one search_boolean (first term required, K = 10) against one search of the same words, to JSON, cache off",
                             "search_boolean": summary(sb), "search": summary(se)}
        eng.close()
        os.makedirs(os.path.join(ROOT, "profiles", "boolean"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "boolean", args.out + ".json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
        assert not any(mismatches.values()), {"queries that differ from the scoring launch": {str(k): v for k, v in mismatches.items()}}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
