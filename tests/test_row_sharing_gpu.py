"""Shared top rows on the GPU (ns_ctx_share_rows; k_rscore, ns_row_kernel.hip): every case of tests/row_shapes.py scored
with rows on and off — hits, score bits, nhits and found byte for byte — and against the numpy restatement; the fallback
of an item whose row cannot prove its top-K; two batches on the ctx's two streams; and ONE child process on the counting
build that asserts that the consumer's look-ups, look-up hits, row probes and row hits were reached.

The second half leaves the one-segment, four-cell frame of the first cases: the library's own cell size, several segments,
pruning, impact and packed streams, AND batches, a filtered copy, a ctx without the side stream, a batch run three times,
caller-bound outputs, a plan in several slices, and a text search through nsbind.Engine (a child process of its own).  Every
one of them compares rows on with rows off byte for byte, checks the numpy restatement, and asserts the producer and consumer
counts exactly — a case that ran with rows silently off fails."""
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


def test_default_cell_size_k_10_and_32():
    """NS_ROW_CELL unset: 200 000 postings in 4 cells of the library's own size.  Every query against rows off; the
    restatement, which loops per posting, on two of them."""
    c = dict(row_shapes.default_cell_size(10), ref_queries=[1, 4])
    ref = row_shapes.restatement(c)
    for k in (10, 32):
        ck = dict(row_shapes.default_cell_size(k), ref_queries=[1, 4]) if k != 10 else c
        assert row_shapes.run_case(ck, ref=ref)[:2] == (4, 32)


@pytest.mark.parametrize("rows,prod,cons", [(2, 8, 28), (1, 4, 16)])
def test_three_segments(rows, prod, cons):
    """k_merge over consumer rows of two byte-identical segments (every score ties across them) and streamed rows of a third;
    under mode 1 segment 0's key has four users and segment 2's three"""
    c = row_shapes.three_segments(rows)
    ref = row_shapes.restatement(c)
    for keyed, _ in ref[:3]:   # the tie is in the input: one doc of segments 0 and 2 with one score, next to each other in the top 10
        assert any(a[0] == b[0] and (a[1], b[1]) == (0, 2) and a[2] == b[2] for a, b in zip(keyed[:10], keyed[1:10]))
    assert row_shapes.run_case(c, rows=rows, ref=ref)[:2] == (prod, cons)


def test_pruning_changes_the_user_count():
    """ns_ctx_use_pruning(1) takes the single-term group out of the candidates: three users under mode 1 are no rows, four
    with pruning off are; under mode 2 the two-term groups are consumers and the single-term one is pruned.  Same bytes."""
    c = row_shapes.pruning_input()
    ref = row_shapes.restatement(c)
    r = row_shapes.Runner(c)
    try:
        L, ctx = r.seg.L, r.seg.ctx
        r.seg.build_blockmax(c["idfs"], [0])
        base = r.batch(0)
        assert base[3] == (0, 0, 0, 0) and not int(r.info.flags) & nsbind.NS_INFO_PRUNED
        row_shapes.check_restatement(c, ref, base, 10)
        for rows, prune, want in ((0, 1, (0, 0)), (1, 1, (0, 0)), (1, 0, (4, 16)), (2, 1, (4, 12))):
            assert L.ns_ctx_use_pruning(ctx, prune) == 0
            got = r.batch(rows)
            row_shapes.same_bytes(base, got, (rows, prune))
            assert bool(int(r.info.flags) & nsbind.NS_INFO_PRUNED) == bool(prune), (rows, prune)
            plan = row_shapes.plan_rows(c, rows, pruning=bool(prune))
            assert got[3][:2] == want and got[3] == row_shapes.expected_stats(c, plan), (rows, prune, got[3])
    finally:
        r.release()


@pytest.mark.parametrize("stream", ["packed 1", "packed 2", "impacts", "impacts but one tail"])
def test_other_posting_streams(stream):
    """A batch that reads packed blocks or registered impact streams does not share its term scores, and rows need a sharing
    batch (ns_ctx_share_rows): no rows, the same bytes.  With one tail missing from the impact streams the batch scores every
    posting in place (ns_ctx_share_scores) and takes no rows either."""
    c = row_shapes.CASES["tail_placement"]()
    r = row_shapes.Runner(c)
    try:
        L, ctx = r.seg.L, r.seg.ctx
        base = r.batch(0)
        row_shapes.check_restatement(c, row_shapes.restatement(c), base, 10)
        want_flag = 0
        if stream.startswith("packed"):
            r.seg.build_packed()
            assert L.ns_ctx_use_packed(ctx, int(stream[-1])) == 0
            want_flag = nsbind.NS_INFO_PACKED
        else:
            assert L.ns_ctx_use_packed(ctx, 0) == 0
            r.seg.build_impacts(c["idfs"], leave_out=[3] if stream.endswith("tail") else [])
            want_flag = 0 if stream.endswith("tail") else nsbind.NS_INFO_IMPACTS
        off = r.batch(0, shared=None)
        on = r.batch(1, shared=None)
        flags = int(r.info.flags)
        assert flags & want_flag == want_flag
        row_shapes.same_bytes(base, off, stream)
        row_shapes.same_bytes(base, on, stream)
        assert not flags & nsbind.NS_INFO_SHARED and on[3] == (0, 0, 0, 0)
    finally:
        r.release()


def test_and_batch_takes_no_rows():
    c = row_shapes.CASES["tail_placement"]()
    r = row_shapes.Runner(c)
    try:
        off = r.batch(0, flags=nsbind.NS_FLAG_AND, shared=None)
        on = r.batch(1, flags=nsbind.NS_FLAG_AND, shared=None)
    finally:
        r.release()
    row_shapes.same_bytes(off, on)
    assert on[3] == (0, 0, 0, 0) == row_shapes.expected_stats(c, row_shapes.plan_rows(c, and_mode=True))
    row_shapes.check_restatement(c, row_shapes.restatement(c), on, 10, and_mode=True)
    assert any(int(n) for n in on[1])   # the AND side is not empty


def test_filtered_copy_takes_rows_once_it_has_skip_tables():
    """ns_segment_filter's copy of tails_1_3_70_200's segment without every third doc: no rows before ns_segment_build_skips
    on the copy, rows after; both times the restatement over the kept docs"""
    import filter_ref
    c = row_shapes.CASES["tails_1_3_70_200"]()
    keep = np.arange(c["n_docs"]) % 3 != 2
    masked = filter_ref.mask_lists(c["lists"], keep)
    queries = filter_ref.filtered_queries(c["queries"], masked, False)   # a list without a kept posting is not named
    cm = dict(c, lists=masked, queries=queries, consumers=None, events=None)
    plan = row_shapes.plan_rows(cm)
    assert len(plan["cells"]) == 1 and len(plan["consumers"]) == 7   # the 200-posting tail's group is still not thin
    dl = np.ascontiguousarray(c["doc_len"], np.uint32)
    ref = filter_ref.reference(c["lists"], queries, c["idfs"], c["weights"], dl, rawseg.avgdl_of(dl), keep)
    r = row_shapes.Runner(c)
    try:
        L, ctx = r.seg.L, r.seg.ctx
        h, noff, ncnt, kept, _, _ = nsbind.segment_filter(ctx, r.seg.seg, 1, filter_ref.bits_of(keep), r.seg.offs, r.seg.counts)
        try:
            assert ncnt.tolist() == [len(d) for d, _ in masked] and kept == int(ncnt.sum())
            r.qd, r.refs = rawseg.descriptors(queries, masked, noff, c["idfs"], c["weights"], seg_id=1)
            off = r.batch(0)
            on = r.batch(1)
            row_shapes.same_bytes(off, on, "before the skip tables")
            assert on[3] == (0, 0, 0, 0) == row_shapes.expected_stats(cm, row_shapes.plan_rows(cm, skips=False))
            rawseg.check_results(ref, on[0], on[1], on[2], 10)
            which = np.flatnonzero(ncnt >= 64)
            bo, cn = np.ascontiguousarray(noff[which]), np.ascontiguousarray(ncnt[which])
            assert L.ns_segment_build_skips(ctx, h, bo.ctypes.data, cn.ctypes.data, len(which)) == 0, r.seg.err()
            on = r.batch(1)
            row_shapes.same_bytes(off, on, "after the skip tables")
            want = row_shapes.expected_stats(cm, plan)
            assert on[3] == want and want[1] == 7 * len(next(iter(plan["cells"].values()))), (on[3], want)
            assert np.all(on[0]["seg"][on[0]["doc"] != 0xFFFFFFFF] == 1)
        finally:
            nsbind.close_batches_of(ctx)
            assert L.ns_segment_release(ctx, h) == 0
    finally:
        r.release()


def _mechanics_inputs():
    return {"tails_1_3_70_200": row_shapes.CASES["tails_1_3_70_200"](), "tail_doc_in_the_row": row_shapes.CASES["tail_doc_in_the_row"](),
            "one_cell_direct": row_shapes.CASES["one_cell_direct"](), "fallback": row_shapes.fallback_input()}


@pytest.mark.parametrize("name", ["tails_1_3_70_200", "tail_doc_in_the_row", "one_cell_direct", "fallback"])
def test_without_the_side_stream(name):
    """NS_ROW_FORK=0: producers, scoring launch and consumers on the batch's one stream — the same bytes and stats as forked"""
    c = dict(_mechanics_inputs()[name], name=name)
    forked, plain = {}, {}
    s_fork = row_shapes.run_case(c, keep=forked)
    s_plain = row_shapes.run_case(c, fork=False, keep=plain)
    assert s_fork == s_plain and s_plain[1] > 0
    row_shapes.same_bytes(forked["on"], plain["on"], name)
    if name == "fallback":
        assert s_plain[2] == 5


def test_one_prepared_batch_run_three_times():
    """the fork and join events are reused, the results are the same bytes after every run, and ns_batch_row_stats sums
    fallbacks and row hits over the runs; the second run is a timed one"""
    c = row_shapes.fallback_input()
    once = row_shapes.expected_stats(c, row_shapes.plan_rows(c))
    r = row_shapes.Runner(c)
    try:
        off = r.batch(0)
        b = r.prepare(1)
        try:
            for run in range(3):
                b.run(timed=run == 1)
                got = b.fetch()
                row_shapes.same_bytes(off, got, run)
                assert b.row_stats() == (once[0], once[1], (run + 1) * once[2], (run + 1) * once[3]), (run, b.row_stats(), once)
            assert once[2] == 5 and once[3] > 0
            info = b.info()
            assert info.timed_runs == 1 and info.last_total_ms > 0
        finally:
            b.close()
    finally:
        r.release()


def test_direct_batch_into_bound_torch_outputs():
    """one_cell_direct with caller-bound outputs: k_rscore writes the final rows straight into the torch tensors"""
    torch = pytest.importorskip("torch")
    c = row_shapes.CASES["one_cell_direct"]()
    Q, K = len(c["queries"]), 10
    r = row_shapes.Runner(c)
    try:
        off = r.batch(0)
        b = r.prepare(1)
        try:
            d_hits = torch.zeros((Q, K, 3), dtype=torch.int32, device="cuda")
            d_nhits = torch.zeros(Q, dtype=torch.int32, device="cuda")
            d_found = torch.zeros(Q, dtype=torch.int64, device="cuda")
            b.bind_outputs(d_hits.data_ptr(), d_nhits.data_ptr(), d_found.data_ptr())
            torch.cuda.synchronize()   # the ctx runs on its own non-blocking stream: finish torch's fills first
            b.run()
            b.sync()
            assert b.row_stats()[:2] == (1, Q) and int(b.info().n_items) == 1 + Q
            got = (d_hits.cpu().numpy().view(np.uint32).reshape(Q, K, 3), d_nhits.cpu().numpy().view(np.uint32), d_found.cpu().numpy().view(np.uint64))
            assert got[0].tobytes() == off[0].tobytes() and got[1].tobytes() == off[1].tobytes() and got[2].tobytes() == off[2].tobytes()
        finally:
            b.close()
    finally:
        r.release()


def test_plan_in_several_slices():
    """4096 queries prepared by one host thread and by eight (several slices): the same bytes as rows off, the same consumer
    count; the restatement on every 64th query"""
    c = dict(row_shapes.many_queries(4096), ref_queries=list(range(0, 4096, 64)))
    want = row_shapes.expected_stats(c, row_shapes.plan_rows(c))
    r = row_shapes.Runner(c)
    try:
        off = r.batch(0)
        got = {}
        for threads in (1, 8):
            assert r.seg.L.ns_ctx_set_host_threads(r.seg.ctx, threads) == 0
            got[threads] = r.batch(1)
            row_shapes.same_bytes(off, got[threads], threads)
            assert got[threads][3] == want, (threads, got[threads][3], want)
    finally:
        r.release()
    assert got[1][3][1] == got[8][3][1] == c["consumers"]
    row_shapes.check_restatement(c, row_shapes.restatement(c), got[8], 10)


def test_engine_text_search_takes_rows(tmp_path):
    """One child process on the counting build: a cfg5-law batch through nsbind.Engine.search_batch equals the C oracle, and
    the consumer's counters say that rows were taken (tests/row_engine.py)"""
    if "count" in os.path.basename(os.environ.get("NS_HIP_LIB", "")):
        pytest.skip("this IS a counting-build process")
    assert os.path.exists(COUNT_LIB), "libnextsearch_hip_count.so is missing: make -C nextsearch-api_amd all"
    out = str(tmp_path / "rows_engine.json")
    env = dict(os.environ, NS_HIP_LIB=COUNT_LIB, NS_SHARE="2", NS_SHARE_ROWS="2", NS_ROW_MIN_USERS="1")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "row_engine.py"), out, str(tmp_path / "index")],
                       env=env, capture_output=True, text=True, timeout=REACH_TIMEOUT_S)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "rows engine OK" in r.stdout, tail
    with open(out) as f:
        rep = json.load(f)
    assert rep["consumer_items"] > 0 and rep["lookups"] > 0, rep


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
        if "lookups" in got:   # the exact cases: look-ups and look-up hits are what the input says (row_shapes.expected_lookups)
            assert [got["events"]["lookups"], got["events"]["lookup_hits"]] == got["lookups"], (name, got)
            assert got["events"]["consumer_items"] == got["stats"][1], (name, got)
    assert {"one_cell_direct", "capped_cells", "lookup_cell_populations"} <= {n for n, g in rep.items() if "lookups" in g}
    assert {e for ev in declared.values() if ev for e in ev} == set(row_shapes.EVENTS)
