#!/usr/bin/env python3
"""At-least-m-of-n clauses in boolean queries timed against their siblings.  GPU box only.  Writes
<--dir>/<--out>.json (default profiles/quorum/quorum_bench.json) and prints the same JSON line.
On cfg5's index and batch (bench.py's: one generated segment of 1 M documents, 16 384 queries of 1 - 8 terms), --rounds rounds
after a warm-up, within a round the calls alternating; every value is listed.  Times are the kernels' HIP-event sums the calls
report.  Ranked search at K = 10 and K = 100, facet counts at 50 year buckets, date order (newest first) at K = 10 and K = 100.
  --part siblings (the default)
    ones      `+(a b) +c ...` through the grouped call (the yardstick) and through the quorum call, whose needs are all 1: the
              same clauses, the same answers (asserted, byte for byte); is the quorum median inside the sibling's own range?
    quorum    every term of a query ONE clause, with need min(2, n) and with need n (n: the query's distinct terms; more than
              seven are split into clauses of at most seven, each with need = its distinct terms), next to all-optional (`a b c`)
              and all-required (`+a +b +c`) through the boolean calls, with `found` for each.  Need n returns all-required's
              bytes (asserted).
  --part planes  (a process that loaded the variants or the counting build: they read NS_QUORUM_PLANES)
    the need-min(2, n) batch under the two counter planes it asks for and under three forced ones: the price of the planes' LDS,
    one workgroup per CU instead of two in the tile kernels.  Written to <--out>_planes.json."""
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


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def clause_texts(terms):
    """-> (need min(2, n), need n) of one query's terms as ONE required clause (n > 7: clauses of at most seven distinct terms)"""
    if not terms:
        return "", ""
    distinct = len(set(terms))
    two = "+(" + " ".join(terms) + ")~%d" % min(2, distinct)
    chunks, cur = [], []
    for t in terms:
        if t not in cur and len(set(cur)) == 7:
            chunks.append(cur)
            cur = []
        cur.append(t)
    chunks.append(cur)
    return two if distinct <= 7 else " ".join("+(" + " ".join(c) + ")~%d" % min(2, len(set(c))) for c in chunks), \
        " ".join("+(" + " ".join(c) + ")~%d" % len(set(c)) for c in chunks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--part", default="siblings", choices=["siblings", "planes"])
    ap.add_argument("--dir", default=os.path.join(ROOT, "profiles", "quorum"))
    ap.add_argument("--out", default="quorum_bench")
    args = ap.parse_args()
    assert args.rounds >= 3
    import nsbind
    import workloads
    gen, n_q, _, _, (nseg, docs) = workloads.WORKLOADS["cfg5"]
    tmp = tempfile.mkdtemp(prefix="ns_quorum_idx_")
    out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "rounds": args.rounds, "tile_docs": nsbind.facet_tile_docs(), "part": args.part}
    ks = [int(x) for x in args.ks.split(",")]
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
        terms = [[w for w, _ in nsbind.parse_boolean(q)] for q in queries]     # what the tokenizer keeps
        optional = [" ".join(ws) for ws in terms]
        required = [" ".join("+" + w for w in ws) for ws in terms]
        synonyms = [("+(" + " ".join(ws[:2]) + ") " + " ".join("+" + w for w in ws[2:])).strip() if ws else "" for ws in terms]
        need_two, need_all = (list(x) for x in zip(*[clause_texts(ws) for ws in terms]))
        out["queries"] = n_q
        out["queries_of_more_than_seven_distinct_terms"] = sum(len(set(ws)) > 7 for ws in terms)
        B = len(eng.facet_buckets("year")[1])
        calls = [("search k=%d" % K, lambda qs, K=K: eng.search_quorum_after_batch(qs, K, timing=True), lambda qs, K=K: eng.search_grouped_after_batch(qs, K, timing=True),
                  lambda qs, K=K: eng.search_boolean_after_batch(qs, K, timing=True), 2) for K in ks]
        calls.append(("facets B=%d" % B, lambda qs: eng.facet_quorum_batch(qs, B, timing=True), lambda qs: eng.facet_grouped_batch(qs, B, timing=True),
                      lambda qs: eng.facet_boolean_batch(qs, B, timing=True), 1))
        calls += [("date order k=%d" % K, lambda qs, K=K: eng.search_quorum_sorted_batch(qs, K, order="newest", timing=True),
                   lambda qs, K=K: eng.search_grouped_sorted_batch(qs, K, order="newest", timing=True),
                   lambda qs, K=K: eng.search_boolean_sorted_batch(qs, K, order="newest", timing=True), 3) for K in ks]
        rows = []
        if args.part == "planes":
            assert out["library"] != "libnextsearch_hip.so", "the product library does not read NS_QUORUM_PLANES: load the variants build (NS_HIP_LIB)"
            for name, quorum, _, _, found_at in calls:
                os.environ.pop("NS_QUORUM_PLANES", None)
                two = quorum(need_two)
                os.environ["NS_QUORUM_PLANES"] = "3"
                assert same(quorum(need_two)[:-1], two[:-1]), name + ": three planes change the answers"
                t2, t3 = [], []
                for _ in range(args.rounds):
                    os.environ.pop("NS_QUORUM_PLANES", None)
                    t2.append(quorum(need_two)[-1])
                    os.environ["NS_QUORUM_PLANES"] = "3"
                    t3.append(quorum(need_two)[-1])
                os.environ.pop("NS_QUORUM_PLANES", None)
                rows.append({"call": name, "two_planes_ms": summary(t2), "three_planes_forced_ms": summary(t3),
                             "three_over_two": statistics.median(t3) / statistics.median(t2), "found": int(np.sum(two[found_at], dtype=np.uint64))})
        else:
            for name, quorum, grouped, boolean, found_at in calls:
                q1, g1 = quorum(synonyms), grouped(synonyms)                                   # warm-up: builds the tables; the answers
                assert same(q1[:-1], g1[:-1]), name + ": needs of 1 and the grouped sibling differ"
                two, every, opt, req = quorum(need_two), quorum(need_all), boolean(optional), boolean(required)
                assert same(every[:-1], req[:-1]), name + ": need n and all-required differ"
                t = {k: [] for k in ("ones", "sibling", "two", "all", "optional", "required")}
                for _ in range(args.rounds):
                    t["ones"].append(quorum(synonyms)[-1])
                    t["sibling"].append(grouped(synonyms)[-1])
                    t["two"].append(quorum(need_two)[-1])
                    t["all"].append(quorum(need_all)[-1])
                    t["optional"].append(boolean(optional)[-1])
                    t["required"].append(boolean(required)[-1])
                total = lambda r: int(np.sum(r[found_at], dtype=np.uint64))      # noqa: E731
                rows.append({"call": name, "quorum_all_ones_ms": summary(t["ones"]), "grouped_sibling_ms": summary(t["sibling"]),
                             "ones_over_sibling": statistics.median(t["ones"]) / statistics.median(t["sibling"]),
                             "ones_median_inside_the_siblings_range": bool(min(t["sibling"]) <= statistics.median(t["ones"]) <= max(t["sibling"])),
                             "found_synonyms": total(q1),
                             "need_two_ms": summary(t["two"]), "need_all_ms": summary(t["all"]), "all_optional_ms": summary(t["optional"]),
                             "all_required_ms": summary(t["required"]), "found_need_two": total(two), "found_need_all": total(every),
                             "found_all_optional": total(opt), "found_all_required": total(req)})
        out["rows"] = rows
        eng.close()
        os.makedirs(args.dir, exist_ok=True)
        with open(os.path.join(args.dir, args.out + ("_planes" if args.part == "planes" else "") + ".json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
