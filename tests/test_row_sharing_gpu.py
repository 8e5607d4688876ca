"""Shared top rows on the GPU (ns_ctx_share_rows; k_rscore, ns_row_kernel.hip): every case of tests/row_shapes.py scored
with rows on and off — hits, score bits, nhits and found byte for byte — and against the numpy restatement; the fallback
of an item whose row cannot prove its top-K; two batches on the ctx's two streams; and ONE child process on the counting
build that asserts that the consumer's look-ups, look-up hits, row probes and row hits were reached."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nsbind
import rawseg
import row_shapes
from conftest import PKG

pytestmark = pytest.mark.gpu

COUNT_LIB = os.path.join(PKG, "libnextsearch_hip_count.so")
REACH_TIMEOUT_S = 30


@pytest.mark.parametrize("name", list(row_shapes.CASES))
def test_case_equals_rows_off_and_the_restatement(name):
    row_shapes.run_case(dict(row_shapes.CASES[name](), name=name))


def test_mode_2_waives_the_user_rule():
    """three users of H: no rows under mode 1 (no_eligible_group asserts it), rows under mode 2"""
    c = row_shapes.CASES["no_eligible_group"]()
    stats = row_shapes.run_case(dict(c, consumers=3 * 4), rows=2)
    assert stats[0] == 4


def test_fallback_when_the_row_cannot_prove_the_result():
    """A tail made of the 60 best docs of H in the first cell — taken from a rows-off run over that cell's part of H as a
    list of its own — at K = 10: 60 of the row's 64 entries hit the table, more than 64 - K, and the row does not hold the
    cell: the item is scored by the streaming body.  Same bytes, and fallbacks are counted."""
    rng, dl, H = row_shapes._base(21)
    in0 = H[0] < 1024
    first = row_shapes._mk(dl, [H, (H[0][in0], H[1][in0])], [[1]], idfs=[1.5, 1.5], weights=[0.75, 0.75])
    r = row_shapes.Runner(first)
    try:
        hits, nhits, _, _ = r.batch(0, k=60)
    finally:
        r.release()
    assert int(nhits[0]) == 60
    best60 = hits[0, :60]["doc"].astype(np.int64)
    assert np.all(best60 < 1024) and np.all(np.isin(best60, H[0]))
    tail = row_shapes._tail(rng, best60)
    c = row_shapes._mk(dl, [H, tail, row_shapes._tail(rng, row_shapes._pick(rng, 5))], [[0, 1], [1, 0], [0, 1, 2], [0, 2], [0], [2, 0, 1], [0, 1], [0, 2]],
                       consumers=32, fallbacks="some", row_hits="some")
    stats = row_shapes.run_case(c)
    assert stats[2] == 5 and stats[3] >= 5 * 60   # the five queries that name the tail, in the first cell each


def test_two_batches_on_the_two_streams():
    """the ctx's two streams (ns_ctx_set_overlap): two batches with rows prepared, run and then fetched; each equals its
    rows-off run"""
    ca, cb = row_shapes.CASES["tail_placement"](), row_shapes.CASES["tail_doc_in_the_row"]()
    # one segment holds both cases' lists: b's follow a's
    na = len(ca["lists"])
    lists = ca["lists"] + cb["lists"]
    qa, qb = ca["queries"], [[li + na for li in q] for q in cb["queries"]]
    c = row_shapes._mk(cb["doc_len"], lists, qa, idfs=ca["idfs"] + cb["idfs"], weights=ca["weights"] + cb["weights"])
    r = row_shapes.Runner(c)
    try:
        L, ctx = r.seg.L, r.seg.ctx
        qd_a, refs_a = r.qd, r.refs
        qd_b, refs_b = rawseg.descriptors(qb, lists, r.seg.offs, c["idfs"], c["weights"])
        want = {}
        for tag, (qd, refs) in (("a", (qd_a, refs_a)), ("b", (qd_b, refs_b))):
            r.qd, r.refs = qd, refs
            want[tag] = r.batch(0)
        assert L.ns_ctx_set_overlap(ctx, 1) == 0
        assert L.ns_ctx_share_rows(ctx, 1) == 0
        ba = nsbind.prepare_raw(ctx, qd_a, refs_a, 10)
        bb = nsbind.prepare_raw(ctx, qd_b, refs_b, 10)
        try:
            assert ba.stream != bb.stream
            ba.run()
            bb.run()
            got_b = bb.fetch()
            got_a = ba.fetch()
            assert ba.row_stats()[1] == 32 and bb.row_stats()[1] == 32 and bb.row_stats()[3] > 0
        finally:
            ba.close()
            bb.close()
        row_shapes.same_bytes(want["a"], got_a, "a")
        row_shapes.same_bytes(want["b"], got_b, "b")
    finally:
        r.release()


def test_counting_build_reaches_the_consumer_paths(tmp_path):
    """One fresh child process loads libnextsearch_hip_count.so and runs the cases that name events again: consumer items,
    look-ups of an owner's doc in the hot list, look-ups that found it, row entries that probed the table and row entries
    that hit it are each above zero for the cases that declare them."""
    if "count" in os.path.basename(os.environ.get("NS_HIP_LIB", "")):
        pytest.skip("this IS a counting-build process")
    assert os.path.exists(COUNT_LIB), "libnextsearch_hip_count.so is missing: make -C nextsearch-api_amd all"
    out = str(tmp_path / "rows_reach.json")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "row_shapes.py"), out],
                       env=dict(os.environ, NS_HIP_LIB=COUNT_LIB), capture_output=True, text=True, timeout=REACH_TIMEOUT_S)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "rows reach OK" in r.stdout, tail
    with open(out) as f:
        rep = json.load(f)
    declared = {name: fn().get("events") for name, fn in row_shapes.CASES.items()}
    assert set(rep) == {n for n, e in declared.items() if e}
    for name, got in rep.items():
        for e in declared[name]:
            assert got["events"][e] > 0, (name, e, got)
    assert {e for ev in declared.values() if ev for e in ev} == set(row_shapes.EVENTS)
