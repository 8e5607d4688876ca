#!/usr/bin/env python3
"""Search sorted by date timed.  GPU box only.  Writes profiles/sorted/sorted_bench.json and prints the same
JSON line.  On cfg5's index and batch (bench.py's: one generated segment of 1 M documents, 16 384 queries of 1 - 8 terms),
--reps timed calls after a warm-up; every value is listed.
  (1) search_sorted_batch (newest first) at K = 10 and K = 100, OR and AND: the kernels' HIP-event time, split into
      k_sd_select, k_sd_join and k_sd_score (summed over the sub-batches), and the whole call through the Python binding
      (query preparation included).
  (2) the two yardsticks on the same batch in the same loop, alternating with (1): ns_facet_count at 50 buckets (identical
      cut and mark: the difference is selection against histogram) and the scoring launch (ns_batch_run's kernel time of a
      prepared batch at the same K).
  (3) one search_sorted call against one search call (cache off), both to JSON."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import nsbind
    import workloads
    gen, n_q, _, _, (nseg, docs) = workloads.WORKLOADS["cfg5"]
    tmp = tempfile.mkdtemp(prefix="ns_sorted_idx_")
    out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "reps": args.reps, "tile_docs": nsbind.facet_tile_docs()}
    try:
        index = os.path.join(tmp, "cfg5")
        nsbind.gen_index(index, nseg, docs, 65536, 1337, False)
        with open(os.path.join(index, "metadata.csv"), "w") as f:        # a day per document over 49 years, one in 16 undated
            f.write("cord_uid,publish_time\n" + "".join(
                "u%08d,%s\n" % (i, "" if i % 16 == 5 else "%04d-%02d-%02d" % (1975 + (i * 7919) % 49, 1 + (i * 31) % 12, 1 + (i * 17) % 28))
                for i in range(nseg * docs)))
        eng = nsbind.Engine(index, 0)
        queries = gen()
        assert len(queries) == n_q
        labels = eng.facet_buckets("year")[1]
        out["facet_buckets"] = len(labels)
        _, refs, _ = eng.build_refs(queries)
        out["postings"] = int(refs["count"].sum(dtype=np.uint64))
        rows = []
        for K in (10, 100):
            for flags, mode in ((0, "or"), (nsbind.NS_FLAG_AND, "and")):
                b = eng.prepare(queries, K, flags)
                try:
                    b.run(timed=True)
                    b.sync()
                    hits, keys, nhits, found, has = eng.search_sorted_batch(queries, K, "newest", flags=flags)      # warm-up: builds the key tables
                    _, _, s_found, s_has = eng.search_batch(queries, K, flags)
                    assert np.array_equal(found, np.where(s_has, s_found, 0)), "found differs from the search's"
                    eng.facet_batch(queries, len(labels), "year", flags=flags)
                    nsbind.sorted_kernel_ms(reset=True)
                    dev, split, whole, facet, score = [], [], [], [], []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        r = eng.search_sorted_batch(queries, K, "newest", flags=flags, timing=True)
                        whole.append((time.perf_counter() - t0) * 1e3)
                        dev.append(r[-1])
                        split.append(nsbind.sorted_kernel_ms(reset=True))
                        facet.append(eng.facet_batch(queries, len(labels), "year", flags=flags, timing=True)[3])
                        b.run(timed=True)
                        b.sync()
                        score.append(float(b.info().last_score_kernel_ms))
                finally:
                    b.close()
                rows.append({"k": K, "mode": mode, "matched_documents": int(found.sum()), "hits_returned": int(nhits.sum()),
                             "sorted_kernels_ms": summary(dev),
                             "k_sd_select_ms": summary([s[0] for s in split]), "k_sd_join_ms": summary([s[1] for s in split]),
                             "k_sd_score_ms": summary([s[2] for s in split]),
                             "search_sorted_batch_python_ms": summary(whole), "facet_kernels_ms_50_buckets": summary(facet),
                             "scoring_kernel_ms": summary(score),
                             "sorted_kernels_over_facet_kernels": statistics.median(dev) / statistics.median(facet),
                             "k_sd_select_over_facet_kernels": statistics.median([s[0] for s in split]) / statistics.median(facet),
                             "sorted_kernels_over_scoring_kernel": statistics.median(dev) / statistics.median(score)})
        out["batch"] = {"what": "cfg5's 16 384 queries on cfg5's index, newest first; sorted search, facet pass and scoring launch alternating",
                        "queries": n_q, "rows": rows}
        eng.set_cache(False)
        K = 10
        q = queries[0]
        eng.search_sorted_json(q, K, "newest")
        eng.search_json(q, K)
        so, se = [], []
        for i in range(args.reps):
            q = queries[1 + i]
            t0 = time.perf_counter()
            eng.search_sorted_json(q, K, "newest")
            so.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            eng.search_json(q, K)
            se.append((time.perf_counter() - t0) * 1e3)
        out["latency_ms"] = {"what": "one search_sorted (newest, K = 10) against one search of the same query, to JSON, cache off",
                             "search_sorted": summary(so), "search": summary(se)}
        eng.close()
        os.makedirs(os.path.join(ROOT, "profiles", "sorted"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "sorted", "sorted_bench.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
