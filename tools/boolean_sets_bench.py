#!/usr/bin/env python3
"""Facet counts and date order for boolean queries timed.  GPU box only.  Writes <--dir>/<--out>.json (default
profiles/boolean_sets/boolean_sets_bench.json) and prints the same JSON line.
On cfg5's index and batch (bench.py's: one generated segment of 1 M documents, 16 384 queries of 1 - 8 terms), --reps timed
calls after a warm-up; every value is listed.  Four role mixes of the same batch:
  (a) every term SHOULD                      yardstick: ns_facet_count / ns_search_sorted under NS_FLAG_OR  (identical answers, asserted)
  (b) every term MUST                        yardstick: the same under NS_FLAG_AND                          (identical answers, asserted)
  (c) the first term MUST, the rest SHOULD   yardstick: the OR calls, which cut and mark the same lists
  (d) as (a), the last term turned into NOT  yardstick: as (c)
Counts at 50 (year) and 1024 (custom) buckets, date order (newest first) at K = 10 and K = 100.  Per row: the kernels' HIP-event
time (for the date order split into k_bs_select, k_sd_join and k_bs_score, summed over the sub-batches), the whole call
through the Python binding (query preparation included), the yardstick's kernel time in the same loop, alternating, the ratio
to it, and the ratio to ns_search_boolean's kernels (k_bq_select + k_bq_join) on the same mix and K, measured in that loop too
(for the counts: at K = 10)."""
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
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--dir", default=os.path.join(ROOT, "profiles", "boolean_sets"))
    ap.add_argument("--out", default="boolean_sets_bench")
    args = ap.parse_args()
    import nsbind
    import workloads
    gen, n_q, _, _, (nseg, docs) = workloads.WORKLOADS["cfg5"]
    tmp = tempfile.mkdtemp(prefix="ns_boolean_sets_idx_")
    out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "reps": args.reps, "tile_docs": nsbind.facet_tile_docs()}
    differ = {}
    try:
        index = os.path.join(tmp, "cfg5")
        nsbind.gen_index(index, nseg, docs, 65536, 1337, False)
        with open(os.path.join(index, "metadata.csv"), "w") as f:        # tools/sorted_bench.py's dates: 49 years and "undated" are 50 year buckets
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
        yard_flags = {"a_all_should": 0, "b_all_must": nsbind.NS_FLAG_AND, "c_first_must": 0, "d_last_not": 0}
        _, refs, _ = eng.build_refs(queries)
        out["postings"] = int(refs["count"].sum(dtype=np.uint64))
        labels = eng.facet_buckets("year")[1]
        wide = [((np.arange(eng.segment_info(s)["n_docs"], dtype=np.int64) * 7919) % 1024).astype(np.uint16) for s in range(eng.num_segments)]
        wide_labels = ["b%04d" % i for i in range(1024)]
        specs = {"year_50": dict(kind="year", n_buckets=len(labels)), "custom_1024": dict(kind="custom", n_buckets=1024, custom=wide, labels=wide_labels)}
        out["buckets"] = {"year_50": len(labels), "custom_1024": 1024}
        count_rows = []
        for sname, sp in specs.items():
            kw = dict(kind=sp["kind"], custom=sp.get("custom"), labels=sp.get("labels"))
            for name, qs in mixes.items():
                flags = yard_flags[name]
                counts, found, has = eng.facet_boolean_batch(qs, sp["n_buckets"], **kw)          # warm-up: builds the bucket tables
                y_counts, y_found, y_has = eng.facet_batch(queries, sp["n_buckets"], flags=flags, **kw)
                if name in ("a_all_should", "b_all_must"):
                    differ[(sname, name)] = int(np.sum(np.any(counts != y_counts, axis=1) | (found != y_found) | (has != y_has)))
                eng.search_boolean_batch(qs, 10)
                dev, whole, other, boolean = [], [], [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    r = eng.facet_boolean_batch(qs, sp["n_buckets"], timing=True, **kw)
                    whole.append((time.perf_counter() - t0) * 1e3)
                    dev.append(r[-1])
                    other.append(eng.facet_batch(queries, sp["n_buckets"], flags=flags, timing=True, **kw)[3])
                    boolean.append(eng.search_boolean_batch(qs, 10, timing=True)[-1])
                count_rows.append({"buckets": sname, "mix": name, "usable_queries": int(has.sum()), "matched_documents": int(found.sum()),
                                   "k_bs_count_ms": summary(dev), "facet_boolean_batch_python_ms": summary(whole),
                                   "yardstick": "ns_facet_count " + ("AND" if flags else "OR"), "yardstick_kernel_ms": summary(other),
                                   "over_yardstick": statistics.median(dev) / statistics.median(other),
                                   "ns_search_boolean_k10_kernels_ms": summary(boolean), "over_ns_search_boolean": statistics.median(dev) / statistics.median(boolean),
                                   "queries_that_differ_from_the_yardstick": differ.get((sname, name))})
        out["counts"] = {"what": "cfg5's 16 384 queries on cfg5's index; the boolean count, its yardstick and the boolean search alternating", "rows": count_rows}
        order_rows = []
        for K in [int(x) for x in args.ks.split(",")]:
            for name, qs in mixes.items():
                flags = yard_flags[name]
                got = eng.search_boolean_sorted_batch(qs, K, order="newest")                       # warm-up: builds the key tables
                want = eng.search_sorted_batch(queries, K, "newest", flags=flags)
                if name in ("a_all_should", "b_all_must"):
                    bad = 0
                    for q in range(n_q):
                        n = int(got[2][q])
                        same = bool(got[5][q]) == bool(want[4][q]) and n == int(want[2][q]) and int(got[3][q]) == int(want[3][q])
                        same = same and np.array_equal(got[0][q, :n].view(np.uint8), want[0][q, :n].view(np.uint8)) and np.array_equal(got[1][q, :n], want[1][q, :n])
                        bad += not same
                    differ[("order", name, K)] = bad
                eng.search_boolean_batch(qs, K)
                nsbind.boolean_sets_kernel_ms(reset=True)
                dev, split, whole, other, boolean = [], [], [], [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    r = eng.search_boolean_sorted_batch(qs, K, order="newest", timing=True)
                    whole.append((time.perf_counter() - t0) * 1e3)
                    dev.append(r[-1])
                    split.append(nsbind.boolean_sets_kernel_ms(reset=True))
                    other.append(eng.search_sorted_batch(queries, K, "newest", flags=flags, timing=True)[-1])
                    boolean.append(eng.search_boolean_batch(qs, K, timing=True)[-1])
                order_rows.append({"k": K, "mix": name, "usable_queries": int(got[5].sum()), "matched_documents": int(got[3].sum()), "hits_returned": int(got[2].sum()),
                                   "kernels_ms": summary(dev), "k_bs_select_ms": summary([s[1] for s in split]), "k_sd_join_ms": summary([s[2] for s in split]),
                                   "k_bs_score_ms": summary([s[3] for s in split]), "search_boolean_sorted_batch_python_ms": summary(whole),
                                   "yardstick": "ns_search_sorted " + ("AND" if flags else "OR"), "yardstick_kernels_ms": summary(other),
                                   "over_yardstick": statistics.median(dev) / statistics.median(other),
                                   "ns_search_boolean_kernels_ms": summary(boolean), "over_ns_search_boolean": statistics.median(dev) / statistics.median(boolean),
                                   "queries_that_differ_from_the_yardstick": differ.get(("order", name, K))})
        out["date_order"] = {"what": "the same batch, newest first; the boolean date order, its yardstick and the boolean search alternating", "rows": order_rows}
        eng.close()
        os.makedirs(args.dir, exist_ok=True)
        with open(os.path.join(args.dir, args.out + ".json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
        assert not any(differ.values()), {"queries that differ from the calls without roles": {str(k): v for k, v in differ.items()}}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
