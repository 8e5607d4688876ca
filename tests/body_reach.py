"""Runs the directed families of tests/body_shapes.py through the raw C-ABI against the numpy restatement (tests/rawseg.py).

Imported by tests/test_body_shapes_gpu.py for the product library (run_family: every mode), and run as a program in a child
process that loaded the counting build (NS_HIP_LIB=libnextsearch_hip_count.so):

    python tests/body_reach.py OUT.json

There every family resets the event counters, runs, is checked against the restatement as well, and must have reached the
events it names; the generator-based inputs (the mid1 golden queries, the reduced cfg5 workload) run once for comparison.
The join families of tests/join_shapes.py and one synthetic rank-row case run there too (tests/join_run.py reach()): the
report's "join" key holds their counters and the per-path query counts their declarations predict.
OUT.json receives every counter of every input."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "nextsearch-api_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import nsbind  # noqa: E402
import body_shapes  # noqa: E402
import join_run  # noqa: E402
from rawseg import RawSegment, check_results, descriptors, reference  # noqa: E402

AND = nsbind.NS_FLAG_AND
WHOLE = (0, 1, 1 << 30)   # ns_set_tuning: one work item per (query, segment) group, so that a family's super-batches are the ones it planned


def run_family(fn, full=True):
    """full: every mode of the product-library test; otherwise the modes the reach check counts (in place, AND, the split variant)"""
    n, doc_len, lists, queries, idfs, weights = fn()
    seg = RawSegment(n, doc_len, lists)
    try:
        L, ctx = seg.L, seg.ctx
        ref = reference(lists, queries, idfs, weights, seg.doc_len, seg.avgdl)
        qd, refs = descriptors(queries, lists, seg.offs, idfs, weights)

        def go(label, k=10, flags=0, want=0):
            hits, nhits, found, info = seg.run(qd, refs, k, flags)
            assert info & want == want, (fn.__name__, label, "batch info flags", hex(info), "want", hex(want))
            check_results(ref, hits, nhits, found, k, and_mode=bool(flags & AND), label=(fn.__name__, label))

        def tuning(t):
            assert L.ns_set_tuning(ctx, *t) == 0, seg.err()

        def split_variant(label):
            for s in (fn.split or {}).values():
                tuning((0, 1, s))
                go(label + f" split {s}")
                go(label + f" split {s} k=100", k=100)
                go(label + f" split {s} AND", flags=AND)
            tuning(WHOLE)

        assert L.ns_ctx_share_scores(ctx, 0) == 0 and L.ns_ctx_use_merge(ctx, int(fn.merge)) == 0
        tuning(WHOLE)
        go("in place")
        go("in place AND", flags=AND)
        split_variant("no skip tables")
        if not full:
            return
        assert L.ns_ctx_use_merge(ctx, int(not fn.merge)) == 0
        go("merge body " + ("on" if not fn.merge else "off"))
        go("merge body " + ("on" if not fn.merge else "off") + " AND", flags=AND)
        assert L.ns_ctx_use_merge(ctx, int(fn.merge)) == 0
        tuning((0, 0, 0))
        go("default cut")
        go("default cut k=100", k=100)
        tuning(WHOLE)
        if fn.ks:
            for k in sorted(set(body_shapes.K_SET)):
                go(f"k={k}", k=k)
            go("k=65 AND", k=65, flags=AND)
        seg.build_skips()
        for on in (1, 0):
            assert L.ns_ctx_use_skips(ctx, on) == 0
            go(f"skip tables registered, use {on}")
            go(f"skip tables registered, use {on} AND", flags=AND)
            split_variant(f"skip tables use {on}")
        assert L.ns_ctx_use_skips(ctx, 1) == 0
        assert L.ns_ctx_share_scores(ctx, 2) == 0
        go("shared term scores", want=nsbind.NS_INFO_SHARED)
        go("shared term scores AND", flags=AND, want=nsbind.NS_INFO_SHARED)
        assert L.ns_ctx_share_scores(ctx, 0) == 0
        seg.build_packed()
        for mode in (1, 2):
            assert L.ns_ctx_use_packed(ctx, mode) == 0
            go(f"packed mode {mode}", want=nsbind.NS_INFO_PACKED)
            go(f"packed mode {mode} AND", flags=AND, want=nsbind.NS_INFO_PACKED)
        assert L.ns_ctx_use_packed(ctx, 0) == 0
        seg.build_impacts(idfs)
        go("impact stream", want=nsbind.NS_INFO_IMPACTS)
        go("impact stream AND", flags=AND, want=nsbind.NS_INFO_IMPACTS)
        go("impact stream k=100", k=100, want=nsbind.NS_INFO_IMPACTS)
    finally:
        seg.release()


def _named(counters):
    return {name: counters[getter][i] for name, (getter, i) in body_shapes.EVENTS.items()}


def _generator_inputs(tmp):
    """the generator-based inputs the suite leans on: (label, engine, queries, k, flags)"""
    import workloads
    with open(os.path.join(HERE, "golden", "mid1.json")) as f:
        g = json.load(f)
    p = g["params"]
    d = os.path.join(tmp, "mid1")
    nsbind.gen_index(d, p["n_segments"], p["docs_per_segment"], p["vocab"], p["seed"], p["legacy"])
    eng = nsbind.Engine(d, 0)
    try:
        for case in g["cases"]:
            yield "mid1 golden queries k=%d" % case["k"], eng, g["queries"], case["k"], 0
    finally:
        eng.close()
    gen, _, k, flags, (nseg, _) = workloads.WORKLOADS["cfg5"]
    d = os.path.join(tmp, "cfg5")
    nsbind.gen_index(d, nseg, 60_000, 65536, 1337, False)
    eng = nsbind.Engine(d, 0)
    try:
        yield "cfg5-shaped reduced workload (256 queries, 60000 docs)", eng, gen(256), k, flags
    finally:
        eng.close()


def main(out_path):
    import tempfile
    assert nsbind.debug_counters(), "this library exports no event counters: set NS_HIP_LIB to the counting build"
    t0 = time.time()
    report = {"directed": {}, "generator": {}, "missed": {}}
    for name, fn in body_shapes.FAMILIES.items():
        nsbind.debug_counters(reset=True)
        run_family(fn, full=False)
        c = nsbind.debug_counters(reset=True)
        ev = _named(c)
        report["directed"][name] = {"events": ev, "raw": c, "asserted": list(fn.events)}
        missed = [e for e in fn.events if ev[e] == 0]
        if missed:
            report["missed"][name] = missed
        print(name, {e: ev[e] for e in fn.events}, flush=True)
    with tempfile.TemporaryDirectory(prefix="ns_reach_") as tmp:
        for label, eng, queries, k, flags in _generator_inputs(tmp):
            nsbind.debug_counters(reset=True)
            eng.search_batch(queries, k, flags)
            c = nsbind.debug_counters(reset=True)
            report["generator"][label] = {"events": _named(c), "raw": c}
            print(label, "done", flush=True)
    t1 = time.time()
    report["join"] = join_run.reach()
    report["join"]["seconds"] = round(time.time() - t1, 1)
    for name, missed in report["join"].pop("missed").items():
        report["missed"]["join " + name] = missed
    report["seconds"] = round(time.time() - t0, 1)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    assert not report["missed"], ("families that did not reach the events they name", report["missed"])
    print("reach OK in %.1f s" % report["seconds"])


if __name__ == "__main__":
    main(sys.argv[1])
