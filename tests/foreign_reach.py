"""Runs the shapes of tests/window_shapes.py through the raw C-ABI against the numpy restatement (tests/rawseg.py).

Imported by tests/test_foreign_windows_gpu.py for the product library (run_shape: every mode), and run as a program in a
child process that loaded the counting build (NS_HIP_LIB=libnextsearch_hip_count.so):

    python tests/foreign_reach.py OUT.json

There the first general and the first thin shape (window_shapes.COUNTED) run once, one work item per query, and their
foreign-window counters are set against the lists themselves and against the CPU model of tools/dbg/window_sim.py on the
very same lists:
  consumed     foreign postings consumed == the postings of the foreign lists, exactly (nothing skipped, nothing taken twice)
  budget       foreign postings loaded <= FB * super-batches
  utilisation  consumed / loaded >= the model's - 0.02 (the margin: the device's v_rcp_f32 against the model's division in
               the truncated window sizes)
OUT.json receives the counted and the simulated values."""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "nextsearch-api_amd"), HERE, os.path.join(ROOT, "tools", "dbg")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nsbind  # noqa: E402
import window_shapes  # noqa: E402
from rawseg import PAD_ID, PAD_SCORE_BITS, RawSegment, check_results, descriptors, reference  # noqa: E402

AND = nsbind.NS_FLAG_AND
WHOLE = (0, 1, 1 << 30)   # one work item per (query, segment) group
KS = (1, 10, 33, 100)
UTIL_MARGIN = 0.02


def run_shape(fn, modes=("in place", "shared", "impacts")):
    """every hit, nhits, found and the padding of every query against the restatement: OR and AND, K in KS, whole groups
    and the forced split, scoring in place, with shared term scores and over the impact stream"""
    n, doc_len, lists, queries, idfs, weights = fn()
    seg = RawSegment(n, doc_len, lists)
    try:
        L, ctx = seg.L, seg.ctx
        ref = reference(lists, queries, idfs, weights, seg.doc_len, seg.avgdl)
        qd, refs = descriptors(queries, lists, seg.offs, idfs, weights)

        def go(label, want=0, cut=False):
            for k in KS:
                for flags in (0, AND):
                    b = nsbind.prepare_raw(ctx, qd, refs, k, flags)
                    try:
                        inf = b.info()
                        assert int(inf.flags) & want == want, (fn.__name__, label, hex(int(inf.flags)))
                        assert (int(inf.n_items) > len(queries)) == cut, (fn.__name__, label, "work items", int(inf.n_items))
                        b.run()
                        hits, nhits, found = b.fetch()
                    finally:
                        b.close()
                    check_results(ref, hits, nhits, found, k, and_mode=bool(flags), label=(fn.__name__, label))
                    for qi in range(len(queries)):
                        tail = hits[qi, int(nhits[qi]):k]
                        assert np.all(tail["score"].view(np.uint32) == PAD_SCORE_BITS) and np.all(tail["seg"] == PAD_ID) and \
                            np.all(tail["doc"] == PAD_ID), (fn.__name__, label, k, flags, qi, "padding")

        def both(label, want=0):
            assert L.ns_set_tuning(ctx, *WHOLE) == 0, seg.err()
            go(label + ", whole", want)
            assert L.ns_set_tuning(ctx, 0, 1, window_shapes.SPLIT) == 0, seg.err()
            go(label + ", split", want, cut=True)

        assert L.ns_ctx_share_scores(ctx, 0) == 0
        if "in place" in modes:
            both("in place")
        if "shared" in modes:
            assert L.ns_ctx_share_scores(ctx, 2) == 0
            both("shared term scores", nsbind.NS_INFO_SHARED)
            assert L.ns_ctx_share_scores(ctx, 0) == 0
        if "impacts" in modes:
            seg.build_impacts(idfs)
            both("impact stream", nsbind.NS_INFO_IMPACTS)
    finally:
        seg.release()


def slack_constants():
    with open(os.path.join(ROOT, "nextsearch-api_amd", "csrc", "ns_internal.h")) as f:
        text = f.read()
    return {"thin": int(re.search(r"#define NS_WIN_SLACK_THIN (\d+)", text).group(1)),
            "general": int(re.search(r"#define NS_WIN_SLACK_GEN (\d+)", text).group(1))}


def count_shape(fn):
    import window_sim
    n, doc_len, lists, queries, idfs, weights = fn()
    fb, c = window_shapes.FB[fn.cls], slack_constants()[fn.cls]
    seg = RawSegment(n, doc_len, lists)
    try:
        assert seg.L.ns_ctx_share_scores(seg.ctx, 0) == 0 and seg.L.ns_set_tuning(seg.ctx, *WHOLE) == 0
        ref = reference(lists, queries, idfs, weights, seg.doc_len, seg.avgdl)
        qd, refs = descriptors(queries, lists, seg.offs, idfs, weights)
        nsbind.debug_counters(reset=True)
        hits, nhits, found, _ = seg.run(qd, refs, 10, 0)
        cnt = nsbind.debug_counters(reset=True)["ns_debug_counters"]
        check_results(ref, hits, nhits, found, 10, label=(fn.__name__, "counting build"))
    finally:
        seg.release()
    sim = {}
    for q in queries:
        for i, v in window_sim.simulate_item([lists[li][0] for li in q], n, c, fb).items():
            sim[i] = sim.get(i, 0) + v
    foreign = sum(len(lists[li][0]) for q in queries for li in q if li != 0)
    rep = {"class": fn.cls, "FB": fb, "c": c, "foreign postings of the lists": foreign,
           "counted": {"items": cnt[0], "super_batches": cnt[1], "loaded": cnt[3], "consumed": cnt[4], "chunks": cnt[5],
                       "claim_iterations": cnt[6], "driver_rounds": cnt[8], "utilisation": cnt[4] / max(cnt[3], 1)},
           "simulated": {"items": sim[0], "super_batches": sim[1], "loaded": sim[3], "consumed": sim[4], "chunks": sim[5],
                         "driver_rounds": sim[8], "utilisation": sim[4] / max(sim[3], 1)}}
    print(fn.__name__, json.dumps(rep), flush=True)
    assert cnt[0] == len(queries), (fn.__name__, "one driver-stream item per query", cnt[0])
    assert cnt[4] == foreign == sim[4], (fn.__name__, "foreign postings consumed", cnt[4], foreign, sim[4])
    assert cnt[3] <= fb * cnt[1], (fn.__name__, "loaded", cnt[3], "super-batches", cnt[1])
    assert rep["counted"]["utilisation"] >= rep["simulated"]["utilisation"] - UTIL_MARGIN, (fn.__name__, rep)
    return rep


def main(out_path):
    assert nsbind.debug_counters(), "this library exports no event counters: set NS_HIP_LIB to the counting build"
    report = {name: count_shape(window_shapes.SHAPES[name]) for name in window_shapes.COUNTED}
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print("windows OK")


if __name__ == "__main__":
    main(sys.argv[1])
