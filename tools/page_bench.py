#!/usr/bin/env python3
"""Pages past the first K timed.  GPU box only.  Writes profiles/page/<--out>.json and prints the same JSON line.
On cfg5's index and batch (bench.py's: one generated segment of 1 M documents, 16 384 queries of 1 - 8 terms), --reps timed
calls after a warm-up; every value is listed.  Three modes at K = 10 and K = 100:
  or        Engine.search_after_batch, NS_FLAG_OR     (ns_search_boolean_after, roles == NULL)
  all_must  Engine.search_after_batch, NS_FLAG_AND    (ns_search_boolean_after, every role MUST)
  newest    Engine.search_sorted_after_batch          (ns_search_sorted_after, newest first)
Per mode and K: the call without cursors (the AFTER = false kernels: what the entry points without cursors run), then page 2 and
page 11 of the whole batch, reached by handing every query's last hit back, and at K = 100 page 101 on a slice of --slice
queries whose found allows it (found >= 100 K + 1), next to the slice's own call without cursors.  Times are the kernels'
HIP-event times as ns_boolean_kernel_ms / ns_sorted_kernel_ms sum them (select, join, and score for newest), per call.
The yardstick of the call without cursors is the parent commit's tools/boolean_bench.py (mixes a, b) and tools/sorted_bench.py
run in the same session; this tool fixes no ratio."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--slice", type=int, default=512)
    ap.add_argument("--out", default="page_bench")
    args = ap.parse_args()
    import nsbind
    import workloads
    gen, n_q, _, _, (nseg, docs) = workloads.WORKLOADS["cfg5"]
    tmp = tempfile.mkdtemp(prefix="ns_page_idx_")
    out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "reps": args.reps, "tile_docs": nsbind.facet_tile_docs()}
    try:
        index = os.path.join(tmp, "cfg5")
        nsbind.gen_index(index, nseg, docs, 65536, 1337, False)
        with open(os.path.join(index, "metadata.csv"), "w") as f:        # tools/sorted_bench.py's dates
            f.write("cord_uid,publish_time\n" + "".join(
                "u%08d,%s\n" % (i, "" if i % 16 == 5 else "%04d-%02d-%02d" % (1975 + (i * 7919) % 49, 1 + (i * 31) % 12, 1 + (i * 17) % 28))
                for i in range(nseg * docs)))
        eng = nsbind.Engine(index, 0)
        queries = gen()
        assert len(queries) == n_q

        def call(mode, qs, K, cursors):
            """-> (rank of every hit Q x K as uint32, hits, nhits, found, rest)"""
            if mode == "newest":
                hits, keys, nhits, found, rest, _ = eng.search_sorted_after_batch(qs, K, after=cursors, order="newest")
                return keys, hits, nhits, found, rest
            hits, nhits, found, rest, _ = eng.search_after_batch(qs, K, after=cursors, flags=nsbind.NS_FLAG_AND if mode == "all_must" else 0)
            return hits["score"].view(np.uint32), hits, nhits, found, rest

        def kernel_ms(mode):
            return nsbind.sorted_kernel_ms(reset=True) if mode == "newest" else nsbind.boolean_kernel_ms(reset=True)

        def step(mode, qs, K, cursors):
            """one page on: every query's last hit becomes its cursor; a query without a hit keeps what it had"""
            rank, hits, nhits, _, _ = call(mode, qs, K, cursors)
            nxt = [None] * len(qs) if cursors is None else list(cursors)
            for q in np.flatnonzero(nhits):
                n = int(nhits[q])
                nxt[q] = (int(rank[q, n - 1]), int(hits[q, n - 1]["seg"]), int(hits[q, n - 1]["doc"]))
            return nxt

        def timed(mode, qs, K, cursors):
            call(mode, qs, K, cursors)                                    # warm-up
            kernel_ms(mode)
            parts, got = [], None
            for _ in range(args.reps):
                got = call(mode, qs, K, cursors)
                parts.append(kernel_ms(mode))
            _, _, nhits, found, rest = got
            return {"kernels_ms": summary([sum(p) for p in parts]), "select_ms": summary([p[0] for p in parts]), "join_ms": summary([p[1] for p in parts]),
                    "queries_with_a_cursor": 0 if cursors is None else sum(c is not None for c in cursors), "hits_returned": int(nhits.sum()),
                    "matched_documents": int(found.sum()), "documents_after_the_cursors": int(rest.sum())}

        rows = []
        for K in [int(x) for x in args.ks.split(",")]:
            for mode in ("or", "all_must", "newest"):
                base = timed(mode, queries, K, None)
                rows.append(dict(k=K, mode=mode, page=1, queries=n_q, **base))
                cursors = None
                for page in range(2, 12):
                    cursors = step(mode, queries, K, cursors)
                    if page in (2, 11):
                        r = timed(mode, queries, K, cursors)
                        r["kernels_over_page_1"] = r["kernels_ms"]["median"] / base["kernels_ms"]["median"]
                        rows.append(dict(k=K, mode=mode, page=page, queries=n_q, **r))
                if K != 100:
                    continue
                _, _, _, found, _ = call(mode, queries, K, None)
                deep = [q for q in range(n_q) if int(found[q]) >= 100 * K + 1][:args.slice]
                if not deep:
                    continue
                qs = [queries[q] for q in deep]
                sbase = timed(mode, qs, K, None)
                rows.append(dict(k=K, mode=mode, page=1, queries=len(qs), slice=True, **sbase))
                cursors = None
                for page in range(2, 102):
                    cursors = step(mode, qs, K, cursors)
                r = timed(mode, qs, K, cursors)
                r["kernels_over_page_1"] = r["kernels_ms"]["median"] / sbase["kernels_ms"]["median"]
                assert r["hits_returned"] == len(qs) * K, r
                rows.append(dict(k=K, mode=mode, page=101, queries=len(qs), slice=True, **r))
        out["batch"] = {"what": "cfg5's 16 384 queries on cfg5's index; page n is reached by handing every query's last hit back", "rows": rows}
        eng.close()
        os.makedirs(os.path.join(ROOT, "profiles", "page"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "page", args.out + ".json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
