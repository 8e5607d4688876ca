#!/usr/bin/env python3
"""Per-document boost factors in ranked search timed against the unboosted sibling.  GPU box only.  Writes
<--dir>/<--out>.json (default profiles/boost/boost_bench.json) and prints the same JSON line.
On cfg5's index and batch (bench.py's: one generated segment of 1 M documents, 16 384 queries of 1 - 8 terms, here as all-optional
texts and as `+(a b) +c ...`), --rounds rounds after a warm-up, within a round the calls alternating; every value is listed.  Times
are the kernels' HIP-event sums the calls report (k_bq_select + k_bq_join).  Ranked search at K = 10 and K = 100.
    sibling      Engine::search_quorum_after_batch: ns_search_quorum_after, the yardstick
    ones         Engine::search_boosted_after_batch under a custom table of 1.0f: the same answers (asserted, byte for byte)
                 through the boosted kernels: the price of the gather and the multiply
    exponential  under an exponential decay (half-life 5 years from the newest document, undated documents at 0.25): the price
                 when the ranking really changes and the kept set sees another insertion pattern; how many first hits changed
No ratio is fixed in advance: is the median of `ones` inside the sibling's own run-to-run range?"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--dir", default=os.path.join(ROOT, "profiles", "boost"))
    ap.add_argument("--out", default="boost_bench")
    args = ap.parse_args()
    assert args.rounds >= 3
    import nsbind
    import workloads
    gen, n_q, _, _, (nseg, docs) = workloads.WORKLOADS["cfg5"]
    tmp = tempfile.mkdtemp(prefix="ns_boost_idx_")
    out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "rounds": args.rounds, "tile_docs": nsbind.facet_tile_docs()}
    ks = [int(x) for x in args.ks.split(",")]
    try:
        index = os.path.join(tmp, "cfg5")
        nsbind.gen_index(index, nseg, docs, 65536, 1337, False)
        with open(os.path.join(index, "metadata.csv"), "w") as f:        # tools/sorted_bench.py's dates: 49 years, one document in 16 undated
            f.write("cord_uid,publish_time\n" + "".join(
                "u%08d,%s\n" % (i, "" if i % 16 == 5 else "%04d-%02d-%02d" % (1975 + (i * 7919) % 49, 1 + (i * 31) % 12, 1 + (i * 17) % 28))
                for i in range(nseg * docs)))
        eng = nsbind.Engine(index, 0)
        queries = gen()
        assert len(queries) == n_q
        terms = [[w for w, _ in nsbind.parse_boolean(q)] for q in queries]     # what the tokenizer keeps
        forms = {"all optional": [" ".join(ws) for ws in terms],
                 "synonyms": [("+(" + " ".join(ws[:2]) + ") " + " ".join("+" + w for w in ws[2:])).strip() if ws else "" for ws in terms]}
        ones = dict(kind="custom", custom=[np.ones(eng.segment_info(s)["n_docs"], np.float32) for s in range(eng.num_segments)])
        decay = dict(kind="exponential", weight=1.0, origin="", scale_days=5 * 365.25, undated=0.25)
        out["queries"] = n_q
        out["decay"] = {k: v for k, v in decay.items()}
        rows = []
        for form, qs in forms.items():
            for K in ks:
                sib = eng.search_quorum_after_batch(qs, K, timing=True)                      # warm-up; the answers
                one = eng.search_boosted_after_batch(qs, K, boost=ones, timing=True)
                assert same(one[:-1], sib[:-1]), "%s k=%d: a table of 1.0f and the sibling differ" % (form, K)
                exp = eng.search_boosted_after_batch(qs, K, boost=decay, timing=True)
                assert exp[2].tobytes() == sib[2].tobytes(), "a factor changes no matched set"
                t = {k: [] for k in ("sibling", "ones", "exponential")}
                for _ in range(args.rounds):                                                   # (the engine keeps one table set: each switch uploads 4 MB, outside the timed kernels)
                    t["sibling"].append(eng.search_quorum_after_batch(qs, K, timing=True)[-1])
                    t["ones"].append(eng.search_boosted_after_batch(qs, K, boost=ones, timing=True)[-1])
                    t["exponential"].append(eng.search_boosted_after_batch(qs, K, boost=decay, timing=True)[-1])
                has = sib[4].astype(bool) & (sib[1] > 0)
                first_changed = int(np.sum((exp[0][:, 0]["doc"] != sib[0][:, 0]["doc"]) & has))
                rows.append({"queries": form, "k": K, "sibling_ms": summary(t["sibling"]), "ones_ms": summary(t["ones"]), "exponential_ms": summary(t["exponential"]),
                             "ones_over_sibling": statistics.median(t["ones"]) / statistics.median(t["sibling"]),
                             "exponential_over_sibling": statistics.median(t["exponential"]) / statistics.median(t["sibling"]),
                             "ones_median_inside_the_siblings_range": bool(min(t["sibling"]) <= statistics.median(t["ones"]) <= max(t["sibling"])),
                             "found": int(np.sum(sib[2], dtype=np.uint64)), "queries_with_hits": int(np.sum(has)), "first_hits_changed_by_the_decay": first_changed})
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
