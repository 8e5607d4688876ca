#!/usr/bin/env python3
"""Diagnostic: CPU model of the driver-stream body's super-batches (no GPU).  Restates what dscore_body plans per super-batch
— rem, nact, Rf, the foreign windows (ns_internal.h foreign_slack / foreign_window), hi as the minimum of the windows' last
docIds, consumption up to hi, driver rounds of 256 — and prints the counters it models in the lines of tools/dbg/count_run.py,
so that a counted run and a simulated one can be laid side by side:

    python3 tools/dbg/window_sim.py --law cfg5_gen --sample 250 --seed 1 --c 3
    python3 tools/dbg/window_sim.py --law cfg5_thin --sample 120 --c 1,2,3 [--fb 64]

The lists are uniform random docIds with the generator's df law (0.6 N / rank); the class of a query is
tests/body_shapes.plan_rule; every sampled query is ONE item over the whole doc range (the product cuts long items into doc
ranges, which adds a partial super-batch per cut).  simulate_item() takes explicit lists: tests/foreign_reach.py compares the
counting build's window utilisation with it on its own shapes."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "nextsearch-api_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FB_OF = {"thin": 64, "general": 192}
ROUND = 256
MAXSPAN = (1 << (8 + 15)) - 1     # NB = 256 buckets: docs per super-batch - 1
f32 = np.float32


def windows(rem, c, fb):
    """the kernel's plan over the lists' remaining postings (an int array; 0 = nothing left) -> (windows, slack in effect)"""
    rem = np.asarray(rem, dtype=np.int64)
    nact, rf = int((rem > 0).sum()), int(min(rem.sum(), 0xFFFFFFFF))
    ce = c
    if rf <= fb - nact or 2 * c * nact > fb:     # (a) everything fits: whole lists; (b) the slack would take over half the budget
        ce = 1
    scale = f32(f32(fb - ce * nact) * (f32(1.0) / f32(max(rf, 1))))
    w = ce + (rem.astype(np.float32) * scale).astype(np.int64)
    return np.where(rem > 0, np.minimum(w, rem), 0), ce


def simulate_item(lists, n_docs, c, fb, doc_lo=0):
    """lists: sorted docId arrays of one term group -> the counters of count_run.py this model covers, by their index"""
    lists = [np.asarray(x, dtype=np.int64) for x in lists]
    lens = np.array([len(x) for x in lists], dtype=np.int64)
    dl = int(np.argmax(lens))                    # the first of the longest lists, as the kernel's ballot + ctz
    drv = lists[dl]
    cur = np.array([int(np.searchsorted(x, doc_lo)) for x in lists], dtype=np.int64)
    d_cur = int(cur[dl])
    cur[dl] = lens[dl]
    out = {i: 0 for i in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11)}
    out[0], out[10] = 1, len(lists)
    lo, last = doc_lo, n_docs - 1
    while True:
        out[1] += 1
        rem = lens - cur
        w, _ = windows(rem, c, fb)
        ends = [int(lists[t][cur[t] + w[t] - 1]) for t in range(len(lists)) if 0 < w[t] < rem[t]]
        hi = min(ends + [min(last, lo + MAXSPAN)])
        total = int(w.sum())
        if total:
            new = np.array([int(np.searchsorted(lists[t], hi, side="right")) if rem[t] > 0 else cur[t] for t in range(len(lists))])
            assert ((new - cur) <= w).all(), "every foreign posting with docId <= hi is inside its window"
            out[2] += 1
            out[3] += total
            out[4] += int((new - cur).sum())
            out[5] += (total + 63) // 64
            out[11] += int((w > 0).sum())
            cur = new
        left = int(np.searchsorted(drv, hi, side="right")) - d_cur      # driver postings of this super-batch
        out[9] += left
        while d_cur < len(drv):
            n = min(ROUND, len(drv) - d_cur)
            out[8] += 1
            cnt = min(n, left)
            d_cur += cnt
            left -= cnt
            if cnt < n:
                break
        if hi >= last or (int((lens - cur).sum()) == 0 and d_cur >= len(drv)):
            return out
        lo = hi + 1


NAMES = {0: "items (driver-stream body)", 1: "super-batches", 2: "super-batches with foreign postings", 3: "foreign postings LOADED (windows)",
         4: "foreign postings consumed", 5: "foreign chunks", 8: "driver rounds (256 loaded each)", 9: "driver postings consumed",
         10: "terms (sum over items)", 11: "active foreign terms (sum over sb)"}


def report(label, out):
    sb = max(out[1], 1)
    print(label)
    for i in sorted(out):
        print(f"    {NAMES[i]:>40}: {out[i]:>12}  ({out[i] / sb:8.2f} per super-batch)")
    print(f"    foreign window utilisation {out[4] / max(out[3], 1):.3f}; lanes used in foreign chunks {out[4] / max(out[5] * 64, 1):.3f}; "
          f"driver round utilisation {out[9] / max(out[8] * 256, 1):.3f}; "
          f"foreign share of consumed postings {out[4] / max(out[4] + out[9], 1):.3f}; "
          f"postings per super-batch {(out[4] + out[9]) / sb:.1f}")


def law_queries(law):
    """-> (rank lists of the law's queries that take the driver-stream body, their class)"""
    import body_shapes
    import workloads
    base, _, cls = law.partition("_")
    qs = {"cfg5": workloads.cfg5_queries, "cfg3": workloads.cfg3_queries}[base]()

    def rank_of(t):
        return workloads.WORDS.index(t) + 1 if t in workloads.WORDS else int(t[1:])
    want = {"gen": "general", "thin": "thin", "": None}[cls]
    picked = []
    for q in qs:
        ranks = [rank_of(t) for t in q.split()]
        if len(ranks) < 2:
            continue
        k = body_shapes.plan_rule([int(600000.0 / r) for r in ranks], 1_000_000)
        if k in ("thin", "general") and (want is None or k == want):
            picked.append((ranks, k))
    return picked


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--law", default="cfg5_gen", help="cfg5_gen, cfg5_thin, cfg5, cfg3, cfg3_gen, cfg3_thin")
    ap.add_argument("--sample", type=int, default=250)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--c", default="1", help="slack constants, comma separated")
    ap.add_argument("--fb", type=int, default=0, help="foreign budget; 0: the class's (thin 64, general 192)")
    ap.add_argument("--docs", type=int, default=1_000_000)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    qs = law_queries(args.law)
    pick = rng.permutation(len(qs))[:args.sample]
    cache = {}

    def plist(rank):
        if rank not in cache:
            cache[rank] = np.sort(rng.choice(args.docs, max(1, int(0.6 * args.docs / rank)), replace=False))
        return cache[rank]
    items = [([plist(r) for r in qs[i][0]], qs[i][1]) for i in pick]
    for c in (int(x) for x in args.c.split(",")):
        tot = {}
        for lists, k in items:
            o = simulate_item(lists, args.docs, c, args.fb or FB_OF[k])
            for i, v in o.items():
                tot[i] = tot.get(i, 0) + v
        report(f"{args.law}: {len(items)} sampled queries, seed {args.seed}, c = {c}, FB = {args.fb or 'per class'}", tot)


if __name__ == "__main__":
    main()
