#!/usr/bin/env python3
"""Cost of a (query, segment) group under the doc-tile body and under the driver-stream body, measured in the mix
(diagnostic tool, GPU box only; DESIGN.md §4 "Choosing the body by modelled cost").

    python tools/class_fit.py [--law cfg5] [--reps 9] [--min-groups 24] [--out profiles/class_model/fit_cfg5.json]

The general-class groups of three or more terms of the law are binned by foreign share rest / cost (tenths) and by postings
per 64 docs (2-4, 4-8, 8-12, 12-16).  Per bin the whole batch is prepared twice under the density rule (ns_ctx_class_model 0),
once with the bin's groups forced to the doc-tile body (ns_ctx_class_force) and once as it is, and the two batches run
alternately, timed in the kernel leg as tools/law_bench.py times them.  No timing is printed unless both batches give
byte-identical hits, nhits and found and nhits == min(found, K).  From the differences the tool fits

    tile cost    = a * tiles + v * (term, tile) visits + p * postings
    general cost = g * (cmax + f * rest) + s * terms

and prints the constants in units of g (one streamed driver posting), next to the planner's.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import nsbind  # noqa: E402
import law_bench  # noqa: E402

DENS = ((2, 4), (4, 8), (8, 12), (12, 16))
TILE_DOCS = 1024


def group_table(eng, queries, n_docs):
    """per (query, segment) group of a one-segment index: terms, cost, cmax, and the model's tile visits"""
    qd, refs = eng.build_refs(queries)[:2]
    tiles = -(-n_docs // TILE_DOCS)
    rows = []
    for q in range(len(qd)):
        c = refs["count"][int(qd[q]["term_begin"]): int(qd[q]["term_begin"]) + int(qd[q]["term_count"])].astype(np.int64)
        if len(c) == 0:
            continue
        visits = float(np.sum(tiles * (1.0 - np.exp(-c / tiles))))
        rows.append((len(c), int(c.sum()), int(c.max()), visits))
    g = np.array(rows, dtype=[("terms", "i8"), ("cost", "i8"), ("cmax", "i8"), ("visits", "f8")])
    return g, tiles


def same_results(a, b, k):
    ha, na, fa = a
    hb, nb, fb = b
    if not (np.array_equal(na, nb) and np.array_equal(fa, fb) and ha.tobytes() == hb.tobytes()):
        return False
    return bool(np.array_equal(na, np.minimum(fa, k)))


def timed(batches, reps):
    """alternate the batches `reps` times; per batch the kernel-leg times of its runs, in ms"""
    out = [[] for _ in batches]
    for b in batches:
        b.run(False)
        b.sync()
    for _ in range(reps):
        for i, b in enumerate(batches):
            b.run(True)
            b.sync()
            out[i].append(float(b.info().last_score_kernel_ms))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--law", default="cfg5")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--min-groups", type=int, default=24, help="bins with fewer groups are listed without a timing")
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    tmp = tempfile.TemporaryDirectory(prefix="ns_fit_")
    idx = os.path.join(tmp.name, "index")
    nsbind.gen_index(idx, 1, args.docs, 65536, 1337, False)
    eng = nsbind.Engine(idx, 0)
    queries, k = law_bench.laws()[args.law]
    g, tiles = group_table(eng, queries, args.docs)
    rest = g["cost"] - g["cmax"]
    general = (rest * 32 > g["cmax"]) & ~((g["terms"] >= 2) & (g["cost"] * 64 >= args.docs * 16)) & (g["terms"] >= 3)
    share10 = rest * 10 // np.maximum(g["cost"], 1)
    d64 = g["cost"] * 64 // args.docs

    eng.class_model(0)
    eng.class_force(0)
    base = eng.prepare(queries, k)
    base_stats = base.class_stats()
    base.run(False)
    base.sync()
    base_res = base.fetch()[:3]
    bins = []
    print(f"law={args.law} K={k} queries={len(queries)} tiles={tiles} groups by class (general, thin, tile, promoted)={base_stats}")
    print(f"{'share':>7} {'dens64':>7} {'groups':>7} {'tiles':>9} {'visits':>10} {'postings':>11} {'cmax':>11} {'rest':>11} {'terms':>7} {'gen_ms':>8} {'tile_ms':>8} {'delta_us':>9}")
    for s in range(10):
        for lo, hi in DENS:
            m = general & (share10 == s) & (d64 >= lo) & (d64 < hi)
            n = int(m.sum())
            row = dict(share10=s, dens64=[lo, hi], groups=n, tiles=n * tiles, visits=float(g["visits"][m].sum()), postings=int(g["cost"][m].sum()),
                       cmax=int(g["cmax"][m].sum()), rest=int(rest[m].sum()), terms=int(g["terms"][m].sum()))
            if n >= args.min_groups:
                eng.class_force(1, s, lo, hi)
                forced = eng.prepare(queries, k)
                eng.class_force(0)
                moved = forced.class_stats()[3]
                if moved != n:
                    raise SystemExit(f"bin {s} {lo}-{hi}: the planner moved {moved} groups, the restated rule {n}")
                t_gen, t_tile = timed([base, forced], args.reps)
                if not same_results(forced.fetch()[:3], base_res, k) or not same_results(base.fetch()[:3], base_res, k):
                    raise SystemExit(f"bin {s} {lo}-{hi}: results differ between the bodies or nhits != min(found, K); no timing printed")
                forced.close()
                row.update(gen_ms=t_gen, tile_ms=t_tile, gen_med=float(np.median(t_gen)), tile_med=float(np.median(t_tile)))
                row["delta_us"] = 1000.0 * float(np.median(np.array(t_tile) - np.array(t_gen)))
                print(f"{s / 10:>7.1f} {lo:>3}-{hi:<3} {n:>7} {row['tiles']:>9} {row['visits']:>10.0f} {row['postings']:>11} {row['cmax']:>11} {row['rest']:>11} {row['terms']:>7} "
                      f"{row['gen_med']:>8.3f} {row['tile_med']:>8.3f} {row['delta_us']:>9.1f}", flush=True)
            elif n:
                print(f"{s / 10:>7.1f} {lo:>3}-{hi:<3} {n:>7}   (fewer than {args.min_groups} groups: not timed)")
            bins.append(row)
    # the fit: delta = a T + v V + p P - g Cmax - gf Rest - s Terms over the timed bins (ms); reported in units of g
    tb = [b for b in bins if "delta_us" in b]
    fit = None
    if len(tb) >= 8:
        A = np.array([[b["tiles"], b["visits"], b["postings"], -b["cmax"], -b["rest"], -b["terms"]] for b in tb], float)
        y = np.array([b["delta_us"] * 1e-3 for b in tb])
        scale = np.abs(A).max(axis=0)
        x, *_ = np.linalg.lstsq(A / scale, y, rcond=None)
        x = x / scale
        res = y - A @ x
        a, v, p, gg, gf, sterm = (float(t) for t in x)
        fit = dict(a_ms=a, v_ms=v, p_ms=p, g_ms=gg, gf_ms=gf, s_ms=sterm, residual_rms_us=1000.0 * float(np.sqrt(np.mean(res ** 2))),
                   delta_rms_us=1000.0 * float(np.sqrt(np.mean(y ** 2))))
        if gg > 0:
            fit.update(a_units=a / gg, v_units=v / gg, p_units=p / gg, f=gf / gg, s_units=sterm / gg)
        print("fit:", json.dumps(fit))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(law=args.law, k=k, queries=len(queries), tiles=tiles, class_stats=base_stats, reps=args.reps, bins=bins, fit=fit), f, indent=1)
    base.close()
    eng.close()


if __name__ == "__main__":
    main()
