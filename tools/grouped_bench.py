#!/usr/bin/env python3
"""Any-of groups in boolean queries timed against their boolean siblings.  GPU box only.  Writes
<--dir>/<--out>.json (default profiles/grouped/grouped_bench.json) and prints the same JSON line.
On cfg5's index and batch (bench.py's: one generated segment of 1 M documents, 16 384 queries of 1 - 8 terms), --rounds rounds
after a warm-up, within a round the grouped call and its sibling alternating; every value is listed.  Two forms of the batch:
  distinct   every term required: `+a +b +c` through the boolean call (the yardstick) and through the grouped call, where every
             term is a clause of its own.  The same marks and barriers, the same answers (asserted, byte for byte).
  synonyms   the first two terms one clause, the rest required: `+(a b) +c`; no sibling says this, `found` is listed next to it.
Ranked search at K = 10 and K = 100, facet counts at 50 year buckets, date order (newest first) at K = 10 and K = 100.  Times
are the kernels' HIP-event sums the calls report."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd"))


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": list(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--dir", default=os.path.join(ROOT, "profiles", "grouped"))
    ap.add_argument("--out", default="grouped_bench")
    args = ap.parse_args()
    assert args.rounds >= 3
    import nsbind
    import workloads
    gen, n_q, _, _, (nseg, docs) = workloads.WORKLOADS["cfg5"]
    tmp = tempfile.mkdtemp(prefix="ns_grouped_idx_")
    out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "rounds": args.rounds, "tile_docs": nsbind.facet_tile_docs()}
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
        must = [" ".join("+" + w for w in ws) for ws in words]
        synonyms = [("+(" + " ".join(ws[:2]) + ") " + " ".join("+" + w for w in ws[2:])).strip() for ws in words]
        out["queries"] = n_q
        labels = eng.facet_buckets("year")[1]
        B = len(labels)
        rows = []

        def same(a, b):
            return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))

        calls = [("search k=%d" % K, lambda qs, K=K: eng.search_grouped_after_batch(qs, K, timing=True), lambda qs, K=K: eng.search_boolean_after_batch(qs, K, timing=True), 2)
                 for K in [int(x) for x in args.ks.split(",")]]
        calls.append(("facets B=%d" % B, lambda qs: eng.facet_grouped_batch(qs, B, timing=True), lambda qs: eng.facet_boolean_batch(qs, B, timing=True), 1))
        calls += [("date order k=%d" % K, lambda qs, K=K: eng.search_grouped_sorted_batch(qs, K, order="newest", timing=True),
                   lambda qs, K=K: eng.search_boolean_sorted_batch(qs, K, order="newest", timing=True), 3) for K in [int(x) for x in args.ks.split(",")]]
        for name, grouped, sibling, found_at in calls:
            g, s, y = grouped(must), sibling(must), grouped(synonyms)                    # warm-up: builds the tables; the answers
            assert same(g[:-1], s[:-1]), name + ": the grouped call and its sibling differ"
            t_g, t_s, t_y = [], [], []
            for _ in range(args.rounds):
                t_g.append(grouped(must)[-1])
                t_s.append(sibling(must)[-1])
                t_y.append(grouped(synonyms)[-1])
            rows.append({"call": name, "grouped_distinct_ms": summary(t_g), "boolean_sibling_ms": summary(t_s),
                         "grouped_over_sibling": statistics.median(t_g) / statistics.median(t_s),
                         "grouped_median_inside_the_siblings_range": bool(min(t_s) <= statistics.median(t_g) <= max(t_s)),
                         "found_distinct": int(np.sum(g[found_at], dtype=np.uint64)), "grouped_synonyms_ms": summary(t_y),
                         "found_synonyms": int(np.sum(y[found_at], dtype=np.uint64))})
        out["rows"] = rows
        eng.close()
        os.makedirs(args.dir, exist_ok=True)
        with open(os.path.join(args.dir, args.out + ".json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
