#!/usr/bin/env python3
"""Facet counts timed.  GPU box only.  Writes profiles/facet/facet_bench.json and prints the same JSON line.
On cfg5's index and batch (bench.py's: one generated segment of 1 M documents, 16 384 queries of 1 - 8 terms), --reps timed
calls after a warm-up; every value is listed.
  (1) ns_facet_count for a year-like table (50 buckets, a year per document) and for 1024 buckets, OR and AND: the kernels'
      HIP-event time and the host-to-host time of the calls (planning, uploads, the kernels, the counts' way back), both as
      Engine::facet_batch_flat sums them over its sub-batches, and the whole facet_batch call through the Python binding
      (query preparation included).  posting_bytes_per_s = 8 B x the postings of the batch's lists / the kernels' time (an AND
      item that ends early reads fewer).
  (2) the scoring launch of the same batch in the same process: ns_batch_run's kernel time of a prepared batch, alternating
      with (1) in the same loop.
  (3) one search_faceted call against one search call (cache off), both to JSON."""
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
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import nsbind
    import workloads
    gen, n_q, K, _, (nseg, docs) = workloads.WORKLOADS["cfg5"]
    tmp = tempfile.mkdtemp(prefix="ns_facet_idx_")
    out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "reps": args.reps, "tile_docs": nsbind.facet_tile_docs()}
    try:
        index = os.path.join(tmp, "cfg5")
        nsbind.gen_index(index, nseg, docs, 65536, 1337, False)
        with open(os.path.join(index, "metadata.csv"), "w") as f:        # a year per document, 49 years: 50 buckets with "undated"
            f.write("cord_uid,publish_time\n" + "".join("u%08d,%d\n" % (i, 1975 + (i * 7919) % 49) for i in range(nseg * docs)))
        eng = nsbind.Engine(index, 0)
        queries = gen()
        assert len(queries) == n_q
        labels = eng.facet_buckets("year")[1]
        _, refs, _ = eng.build_refs(queries)
        postings = int(refs["count"].sum(dtype=np.uint64))                  # what one pass over the batch's lists reads, at 8 B each
        out["postings"] = postings
        wide = [((np.arange(eng.segment_info(s)["n_docs"], dtype=np.int64) * 7919) % 1024).astype(np.uint16) for s in range(eng.num_segments)]
        wide_labels = ["b%04d" % i for i in range(1024)]
        specs = {"year_50": dict(kind="year", n_buckets=len(labels)), "custom_1024": dict(kind="custom", n_buckets=1024, custom=wide, labels=wide_labels)}
        out["buckets"] = {"year_50": len(labels), "custom_1024": 1024}
        rows = []
        for name, sp in specs.items():
            for flags, mode in ((0, "or"), (nsbind.NS_FLAG_AND, "and")):
                b = eng.prepare(queries, K, flags)
                try:
                    b.run(timed=True)
                    b.sync()
                    fl = int(b.info().flags)                                     # what the scoring launch of this batch reads
                    out.setdefault("scoring_batch", {})[mode] = {"shared_term_scores": bool(fl & nsbind.NS_INFO_SHARED), "packed_stream": bool(fl & nsbind.NS_INFO_PACKED),
                                                                 "impact_stream": bool(fl & nsbind.NS_INFO_IMPACTS), "shared_postings": int(b.info().shared_postings)}
                    counts, found, _, _, _ = eng.facet_batch(queries, sp["n_buckets"], sp["kind"], flags=flags, custom=sp.get("custom"),
                                                             labels=sp.get("labels"), timing=True)
                    _, _, s_found, s_has = eng.search_batch(queries, K, flags)
                    assert np.array_equal(found, np.where(s_has, s_found, 0)), "found differs from the search's"
                    dev, call, whole, score = [], [], [], []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        _, _, _, d_ms, c_ms = eng.facet_batch(queries, sp["n_buckets"], sp["kind"], flags=flags, custom=sp.get("custom"),
                                                              labels=sp.get("labels"), timing=True)
                        whole.append((time.perf_counter() - t0) * 1e3)
                        dev.append(d_ms)
                        call.append(c_ms)
                        b.run(timed=True)
                        b.sync()
                        score.append(float(b.info().last_score_kernel_ms))
                finally:
                    b.close()
                rows.append({"table": name, "mode": mode, "matched_documents": int(found.sum()), "facet_kernels_ms": summary(dev),
                             "ns_facet_count_host_to_host_ms": summary(call), "facet_batch_python_ms": summary(whole),
                             "scoring_kernel_ms": summary(score), "facet_kernels_over_scoring_kernel": statistics.median(dev) / statistics.median(score),
                             "posting_bytes_per_s": 8.0 * postings / (statistics.median(dev) * 1e-3)})
        out["batch"] = {"what": "cfg5's 16 384 queries on cfg5's index; facet pass and scoring launch alternating", "queries": n_q, "k": K, "rows": rows}
        eng.set_cache(False)
        q = queries[0]
        eng.search_faceted_json(q, K, "year")
        eng.search_json(q, K)
        fa, se = [], []
        for i in range(args.reps):
            q = queries[1 + i]
            t0 = time.perf_counter()
            eng.search_faceted_json(q, K, "year")
            fa.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            eng.search_json(q, K)
            se.append((time.perf_counter() - t0) * 1e3)
        out["latency_ms"] = {"what": "one search_faceted (year) against one search of the same query, to JSON, cache off", "search_faceted": summary(fa), "search": summary(se)}
        eng.close()
        os.makedirs(os.path.join(ROOT, "profiles", "facet"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "facet", "facet_bench.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
