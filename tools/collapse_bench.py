#!/usr/bin/env python3
"""Collapsed ranked search timed against ns_search_boosted_after on the same tree.  GPU box only.  Writes
<--dir>/<--out>.json (default profiles/collapse/collapse_bench.json) and prints the same JSON line.
On cfg5's index and batch (bench.py's: one generated segment of 1 M documents, 16 384 queries of 1 - 8 terms, as all-optional
texts), --rounds rounds after a warm-up, within a round the calls alternating; every value is listed.  Times are the kernels'
HIP-event sums the calls report.  Ranked search at K = 10 and K = 100, three key laws, each with and without the count pass:
    sibling      Engine::search_boosted_after_batch without a spec: the yardstick, whose kernels the collapsed call leaves alone
    distinct     every document a key of its own: the sibling's answers (asserted, byte for byte) through the collapsing kernels:
                 pure overhead, the gather plus the membership test
    duplicates   about 30 % of the documents in groups of 2 - 5, the rest with keys of their own
    thousand     1000 groups over all documents: heavy collapsing, most candidates are dropped or replace an entry
No ratio is fixed in advance: the select kernel is expected to stay dominated by the score-table pass."""
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


def key_laws(sizes):
    """name -> one uint32 key array per segment"""
    total = sum(sizes)
    rng = np.random.default_rng(20261021)
    distinct = np.arange(1, total + 1, dtype=np.uint32)
    dup = distinct.copy()
    perm = rng.permutation(total)[: int(total * 0.3)]
    at = 0
    while at < len(perm):
        size = int(rng.integers(2, 6))
        dup[perm[at:at + size]] = dup[perm[at]]
        at += size
    thousand = (1 + rng.integers(0, 1000, total)).astype(np.uint32)

    def cut(a):
        out, off = [], 0
        for n in sizes:
            out.append(np.ascontiguousarray(a[off:off + n]))
            off += n
        return out

    return {"distinct": cut(distinct), "duplicates": cut(dup), "thousand": cut(thousand)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--dir", default=os.path.join(ROOT, "profiles", "collapse"))
    ap.add_argument("--out", default="collapse_bench")
    args = ap.parse_args()
    assert args.rounds >= 3
    import nsbind
    import workloads
    gen, n_q, _, _, (nseg, docs) = workloads.WORKLOADS["cfg5"]
    tmp = tempfile.mkdtemp(prefix="ns_collapse_idx_")
    out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "rounds": args.rounds, "tile_docs": nsbind.facet_tile_docs()}
    ks = [int(x) for x in args.ks.split(",")]
    try:
        index = os.path.join(tmp, "cfg5")
        nsbind.gen_index(index, nseg, docs, 65536, 1337, False)
        eng = nsbind.Engine(index, 0)
        queries = gen()
        assert len(queries) == n_q
        qs = [" ".join(w for w, _ in nsbind.parse_boolean(q)) for q in queries]     # what the tokenizer keeps, all optional
        laws = key_laws([eng.segment_info(s)["n_docs"] for s in range(eng.num_segments)])
        out["queries"] = n_q
        rows = []
        for K in ks:
            sib = eng.search_boosted_after_batch(qs, K, timing=True)                          # warm-up; the answers
            got = eng.search_collapsed_batch(qs, K, collapse=laws["distinct"], timing=True)
            assert got[0].tobytes() == sib[0].tobytes() and got[3].tobytes() == sib[1].tobytes() and got[4].tobytes() == sib[2].tobytes(), \
                "k=%d: keys that are all distinct and the sibling differ" % K
            assert not np.any(got[2])
            names = ["sibling"] + [law + tail for law in laws for tail in ("", " + count")]
            t = {n: [] for n in names}
            hits_of = {}
            for law in laws:                                                                    # warm-up of each law; what it collapses
                r = eng.search_collapsed_batch(qs, K, collapse=laws[law], timing=True)
                hits_of[law] = {"nhits": int(np.sum(r[3], dtype=np.uint64)), "others": int(np.sum(r[2], dtype=np.uint64))}
            for _ in range(args.rounds):                                                       # (the engine keeps one key set: each switch uploads 4 MB, outside the timed kernels)
                t["sibling"].append(eng.search_boosted_after_batch(qs, K, timing=True)[-1])
                for law in laws:
                    t[law].append(eng.search_collapsed_batch(qs, K, collapse=laws[law], others=False, timing=True)[-1])
                    t[law + " + count"].append(eng.search_collapsed_batch(qs, K, collapse=laws[law], others=True, timing=True)[-1])
            med = statistics.median(t["sibling"])
            row = {"k": K, "found": int(np.sum(sib[2], dtype=np.uint64)), "sibling_nhits": int(np.sum(sib[1], dtype=np.uint64)), "collapsed": hits_of}
            for n in names:
                row[n + "_ms"] = summary(t[n])
                if n != "sibling":
                    row[n + "_over_sibling"] = statistics.median(t[n]) / med
            rows.append(row)
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
