"""Derived segments on the device (csrc/ns_union.hip behind ns_segment_union).  The oracle is
tests/union_ref.py: the rule restated in numpy, and tests/rawseg.py's and tests/boolean_ref.py's fp32 restatements of the
scoring run over the restated lists.  Integers, bytes and fp32 bit patterns: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import boolean_ref
import nsbind
import rawseg
import union_ref

pytestmark = pytest.mark.gpu
NS_E_INVAL = -1
AND = nsbind.NS_FLAG_AND
DEFAULT_SCRATCH = 64 << 20


# ---- 1: the raw ABI, array for array ------------------------------------------------------------------------------------
N_DOCS = [1, 63, 64, 65, 300, 4099]
SPANS = [1, 63, 64, 65, 129]


def make_source(n_docs, seed):
    """-> (lists of the stream, {name: (first posting, count)}).  Named lists: `even` / `odd` (disjoint), `even2` (even's
    documents, other tf), `full` (every document), `oob` (its last docId is n_docs + 5), `none` (empty); then lists of 1
    to 3 postings.  Document 0 and document n_docs - 1 are named by `full`, and by `even` / the
    larger of the two.  400 small lists follow, so that the stream holds the spans at any n_docs."""
    rng = np.random.default_rng(seed)
    d = np.arange(n_docs, dtype=np.uint32)
    tf = lambda m: rng.integers(1, 9, m).astype(np.uint32)
    even, odd = d[d % 2 == 0], d[d % 2 == 1]
    inside = np.sort(rng.choice(n_docs, min(n_docs, 18), replace=False)).astype(np.uint32)
    named = [("even", even, tf(len(even))), ("odd", odd, tf(len(odd))), ("even2", even, tf(len(even)) + 9), ("full", d, tf(n_docs)),
             ("oob", np.concatenate([inside, [n_docs + 5]]).astype(np.uint32), tf(len(inside) + 1)), ("none", d[:0], tf(0))]
    lists, where, at = [], {}, 0
    for name, docs, tfs in named:
        where[name] = (at, len(docs))
        lists.append((docs, tfs))
        at += len(docs)
    first_small = at
    for _ in range(400):
        m = int(min(n_docs, rng.integers(1, 4)))
        lists.append((np.sort(rng.choice(n_docs, m, replace=False)).astype(np.uint32), tf(m)))
        at += m
    where["small"] = (first_small, at - first_small)
    where["small_lists"] = [(first_small + int(o), len(l[0])) for o, l in zip(np.cumsum([0] + [len(l[0]) for l in lists[6:-1]]), lists[6:])]
    return lists, where, at


def make_groups(where, n):
    """the group shapes of the issue -> (member_off, member_cnt, group_begin, {name: group number})"""
    assert n >= 200 + 129
    W = lambda name: where[name]
    groups = [
        ("empty", []),
        ("one empty member", [W("none")]),
        ("two empty members", [W("none"), (n, 0)]),
        ("single with a docId out of range", [W("oob")]),
        ("disjoint", [W("even"), W("odd")]),
        ("same documents", [W("even"), W("even2")]),
        ("twice", [W("even"), W("even")]),
        ("spans", [(7 + 3 * i, m) for i, m in enumerate(SPANS)]),
        ("200 small members", where["small_lists"][:200]),
        ("overlap in the stream", [(n - 120, 100), (n - 90, 90)]),
        ("multi with a docId out of range", [W("oob"), W("odd")]),
        ("every document", [W("full"), W("even")]),
        ("single across chunks", [(n - 129, 129)]),
        ("single whole stream", [(0, n)]),
        ("single again", [W("oob")]),
    ]
    assert len(where["small_lists"]) == 400
    off = np.array([a * 8 for _, ms in groups for a, _ in ms], dtype=np.uint64)
    cnt = np.array([c for _, ms in groups for _, c in ms], dtype=np.uint32)
    gb = np.cumsum([0] + [len(ms) for _, ms in groups]).astype(np.uint32)
    return off, cnt, gb, {name: g for g, (name, _) in enumerate(groups)}


@pytest.fixture(scope="module")
def sources():
    rng = np.random.default_rng(5)
    made = [make_source(n, 40 + i) for i, n in enumerate(N_DOCS)]
    segs = rawseg.RawSegments([(n, rng.integers(1, 400, n).astype(np.uint32), lists) for n, (lists, _, _) in zip(N_DOCS, made)])
    yield segs, made
    segs.release()


def compare(label, got, flat, off, cnt, gb, n_docs, scratch):
    """one call's outputs against the restatement -> the restated lists"""
    h, noff, ncnt, written, rounds, ms, payload = got
    want = union_ref.union(flat, off, cnt, gb, n_docs)
    assert [int(c) for c in ncnt] == [len(d) for d, _ in want], label
    assert written == int(ncnt.sum()) == len(payload) and written <= union_ref.bound(cnt, gb, n_docs), label
    union_ref.check_layout(noff, ncnt, written)
    for g, ((docs, tfs), (w_docs, w_tfs)) in enumerate(zip(union_ref.lists_of(payload, noff, ncnt), want)):
        np.testing.assert_array_equal(docs, w_docs, err_msg=str((label, "group", g)))
        np.testing.assert_array_equal(tfs, w_tfs, err_msg=str((label, "group", g)))
    assert rounds == union_ref.rounds(cnt, gb, n_docs, scratch), label
    assert ms >= 0.0
    return want


@pytest.mark.parametrize("si", range(len(N_DOCS)), ids=[str(n) for n in N_DOCS])
def test_union_equals_the_restatement(sources, si):
    segs, made = sources
    n_docs, (lists, where, n) = N_DOCS[si], made[si]
    flat = segs._keep[si].reshape(-1, 2)
    assert len(flat) == n
    off, cnt, gb, G = make_groups(where, n)
    got = nsbind.segment_union(segs.ctx, segs.segs[si], 100, off, cnt, gb, n_docs=n_docs)
    try:
        want = compare(n_docs, got, flat, off, cnt, gb, n_docs, DEFAULT_SCRATCH)
        count = lambda name: len(want[G[name]][0])
        # what the groups mean, stated without the restatement
        assert count("empty") == count("one empty member") == count("two empty members") == 0
        a, m = where["oob"]
        for name in ("single with a docId out of range", "single again"):
            assert np.array_equal(want[G[name]][0], flat[a:a + m, 0]) and np.array_equal(want[G[name]][1], flat[a:a + m, 1])
        assert int(want[G["single again"]][0][-1]) == n_docs + 5                      # kept as it stands
        assert count("disjoint") == where["even"][1] + where["odd"][1] == n_docs
        assert count("same documents") == where["even"][1]
        e0, em = where["even"]
        assert np.array_equal(want[G["twice"]][1], 2 * flat[e0:e0 + em, 1])
        assert count("multi with a docId out of range") and int(want[G["multi with a docId out of range"]][0].max()) < n_docs
        assert np.array_equal(want[G["every document"]][0], np.arange(n_docs))
        assert count("single whole stream") == n and count("single across chunks") == 129
        named = np.concatenate([w[0] for g, w in enumerate(want) if gb[g + 1] - gb[g] >= 2 and len(w[0])])
        assert 0 in named and n_docs - 1 in named
    finally:
        assert segs.L.ns_segment_release(segs.ctx, got[0]) == 0


@pytest.mark.parametrize("si", [0, 3, 5], ids=["1", "65", "4099"])
def test_rounds_do_not_change_the_outputs(sources, si):
    segs, made = sources
    n_docs, (lists, where, n) = N_DOCS[si], made[si]
    flat = segs._keep[si].reshape(-1, 2)
    off, cnt, gb, G = make_groups(where, n)
    # three multi groups (and a single between them): under two tables the last round is partial
    W = lambda name: where[name]
    three = [[W("even"), W("odd")], [W("oob")], [W("full"), W("even2")], [(n - 120, 100), (n - 90, 90)]]
    off3 = np.array([a * 8 for ms in three for a, _ in ms], dtype=np.uint64)
    cnt3 = np.array([c for ms in three for _, c in ms], dtype=np.uint32)
    gb3 = np.cumsum([0] + [len(ms) for ms in three]).astype(np.uint32)
    try:
        for o, c, b, multi in ((off, cnt, gb, 8), (off3, cnt3, gb3, 3)):
            base = nsbind.segment_union(segs.ctx, segs.segs[si], 100, o, c, b, n_docs=n_docs)
            assert segs.L.ns_segment_release(segs.ctx, base[0]) == 0
            assert base[4] == 1
            for scratch, want_rounds in ((4 * n_docs, multi), (8 * n_docs, (multi + 1) // 2), (1, multi), (4 * n_docs - 1, multi), (12 * n_docs, (multi + 2) // 3)):
                nsbind.ctx_union_scratch(segs.ctx, scratch)
                got = nsbind.segment_union(segs.ctx, segs.segs[si], 100, o, c, b, n_docs=n_docs)
                assert segs.L.ns_segment_release(segs.ctx, got[0]) == 0
                label = (n_docs, "scratch", scratch)
                compare(label, got, flat, o, c, b, n_docs, scratch)
                assert got[4] == want_rounds, label
                assert got[3] == base[3] and got[6].tobytes() == base[6].tobytes(), label
                assert got[1].tobytes() == base[1].tobytes() and got[2].tobytes() == base[2].tobytes(), label
    finally:
        nsbind.ctx_union_scratch(segs.ctx, 0)


def test_refusals(sources):
    segs, made = sources
    L, ctx, src = segs.L, segs.ctx, segs.segs[4]
    n = made[4][2]
    off, cnt, gb = np.array([0, 80], np.uint64), np.array([10, 5], np.uint32), np.array([0, 2], np.uint32)
    noff, ncnt = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    written, h = C.c_uint64(), C.c_void_p()
    buf = np.zeros((64, 2), np.uint32)

    def call(ctx=ctx, src=src, new_id=100, off_p=off.ctypes.data, cnt_p=cnt.ctypes.data, gb_p=gb.ctypes.data, n_groups=1,
             noff_p=noff.ctypes.data, ncnt_p=ncnt.ctypes.data, post_p=None, written_p=C.byref(written), out=C.byref(h)):
        return L.ns_segment_union(ctx, src, new_id, off_p, cnt_p, gb_p, n_groups, noff_p, ncnt_p, post_p, written_p, None, None, out)

    assert call(ctx=None) == NS_E_INVAL
    assert call(src=None) == NS_E_INVAL and b"src is NULL" in segs.err()
    assert call(out=None) == NS_E_INVAL
    assert call(gb_p=None) == NS_E_INVAL and b"group_begin is NULL" in segs.err()
    for null in ("off_p", "cnt_p", "noff_p", "ncnt_p"):
        assert call(**{null: None}) == NS_E_INVAL and b"null list arrays" in segs.err()
    assert call(new_id=3) == NS_E_INVAL and b"already uploaded" in segs.err()              # an id in use
    assert call(new_id=1 << 20) == NS_E_INVAL and b"too large" in segs.err()
    for bad_off, bad_cnt in ((0, n + 1), (n * 8, 1), (8, n), (4, 1)):                       # a member outside the source / misaligned
        o, c = np.array([bad_off, 0], np.uint64), np.array([bad_cnt, 1], np.uint32)
        assert call(off_p=o.ctypes.data, cnt_p=c.ctypes.data) == NS_E_INVAL
    for bad in ([1, 2], [0, 2, 1]):                                                        # not non-decreasing from 0
        g = np.array(bad, np.uint32)
        assert call(gb_p=g.ctypes.data, n_groups=len(bad) - 1) == NS_E_INVAL and b"group_begin" in segs.err()
    assert call(post_p=buf.ctypes.data, written_p=None) == NS_E_INVAL and b"postings_out without n_postings_out" in segs.err()
    assert L.ns_ctx_union_scratch(ctx, (16 << 30) + 1) == NS_E_INVAL and b"ns_ctx_union_scratch" in segs.err()
    assert L.ns_ctx_union_scratch(None, 0) == NS_E_INVAL
    # a pending source
    pend = C.c_void_p()
    dl = np.ones(4, np.uint32)
    assert L.ns_segment_upload_begin(ctx, 50, 4, C.c_float(1.0), dl.ctypes.data, 16, C.byref(pend)) == 0
    assert call(src=pend, n_groups=0) == NS_E_INVAL and b"has not ended" in segs.err()
    assert call(new_id=50) == NS_E_INVAL and b"being uploaded" in segs.err()
    assert L.ns_segment_release(ctx, pend) == 0
    assert not h.value
    # nothing was published by a refused call: the id is free; n_postings_out may be NULL without postings_out
    assert call(written_p=None) == 0 and noff[0] % 8 == 0
    h2 = C.c_void_p()
    assert call(new_id=100, out=C.byref(h2)) == NS_E_INVAL and b"already uploaded" in segs.err() and not h2.value
    assert L.ns_segment_release(ctx, h) == 0
    # no group at all: an empty segment
    h3 = C.c_void_p()
    zero = np.zeros(1, np.uint32)
    assert L.ns_segment_union(ctx, src, 100, None, None, zero.ctypes.data, 0, None, None, None, C.byref(written), None, None, C.byref(h3)) == 0, segs.err()
    assert written.value == 0 and L.ns_segment_release(ctx, h3) == 0


# ---- 2: queries over a derived segment -----------------------------------------------------------------------------------
Q_N_DOCS = 3001
Q_SIZES = [1500, 1200, 900, 500, 300, 150, 64, 7]
# derived lists: a mix of copied lists and unions (list numbers of the source)
Q_GROUPS = [[0], [1, 2], [3], [4, 5, 6], [0, 7], [5], [2, 3], [7], [6, 7, 5, 4, 3, 2, 1, 0]]
Q_QUERIES = [[0], [1], [7], [0, 1], [2, 6], [4, 7], [0, 1, 2], [3, 5, 7], [1, 3, 4, 6], [0, 1, 2, 3, 4], [8, 2, 5, 1, 7, 3], list(range(8))]
Q_IDFS = [0.4, 0.7, 1.1, 1.9, 2.6, 3.3, 4.1, 5.5, 0.3]
Q_WEIGHTS = [1.0, 1.0, 2.0, 1.0, 0.5, 1.0, 1.0, 3.0, 1.0]
S, M, X = boolean_ref.SHOULD, boolean_ref.MUST, boolean_ref.NOT
ROLE_CYCLE = [S, M, X, S, S, M, S, X]
PLAIN, SKIPS, SINGLES = 1, 2, 3                                              # ids of the derived segments


def derive(seg, new_id, groups):
    off = np.array([int(seg.offs[li]) for g in groups for li in g], dtype=np.uint64)
    cnt = np.array([int(seg.counts[li]) for g in groups for li in g], dtype=np.uint32)
    gb = np.cumsum([0] + [len(g) for g in groups]).astype(np.uint32)
    h, noff, ncnt, written, _, _, _ = nsbind.segment_union(seg.ctx, seg.seg, new_id, off, cnt, gb)
    return h, noff, ncnt, (off, cnt, gb)


@pytest.fixture(scope="module")
def derived():
    rng = np.random.default_rng(22)
    lists = []
    for m in Q_SIZES:
        docs = np.sort(rng.choice(Q_N_DOCS, m, replace=False)).astype(np.uint32)
        lists.append((docs, rng.integers(1, 12, m).astype(np.uint32)))
    seg = rawseg.RawSegment(Q_N_DOCS, rng.integers(1, 500, Q_N_DOCS), lists)
    h1, noff, ncnt, (off, cnt, gb) = derive(seg, PLAIN, Q_GROUPS)
    h2, noff2, ncnt2, _ = derive(seg, SKIPS, Q_GROUPS)
    assert noff.tobytes() == noff2.tobytes() and ncnt.tobytes() == ncnt2.tobytes()
    which = np.flatnonzero(ncnt >= 64)
    bo, cn = np.ascontiguousarray(noff[which]), np.ascontiguousarray(ncnt[which])
    assert len(which) >= 7
    assert seg.L.ns_segment_build_skips(seg.ctx, h2, bo.ctypes.data, cn.ctypes.data, len(which)) == 0, seg.err()
    ulists = union_ref.union(seg.flat.reshape(-1, 2), off, cnt, gb, Q_N_DOCS)
    assert [int(c) for c in ncnt] == [len(d) for d, _ in ulists] and int(ncnt[1]) > max(Q_SIZES[1], Q_SIZES[2])
    ref = rawseg.reference(ulists, Q_QUERIES, Q_IDFS, Q_WEIGHTS, seg.doc_len, seg.avgdl)      # once, shared, never changed
    bqueries = [[(0, li, ROLE_CYCLE[(qi + j) % 8]) for j, li in enumerate(q)] for qi, q in enumerate(Q_QUERIES)]
    yield {"seg": seg, "h": {PLAIN: h1, SKIPS: h2}, "noff": noff, "ncnt": ncnt, "ulists": ulists, "ref": ref, "bqueries": bqueries, "bcache": {}}
    for h in (h1, h2):
        seg.L.ns_segment_release(seg.ctx, h)
    seg.release()


def configurations(seg):
    """(label, derived id) three times: as made, with skip tables, with skip tables and shared scores forced"""
    yield "as made", PLAIN
    yield "skips", SKIPS
    assert seg.L.ns_ctx_share_scores(seg.ctx, 2) == 0
    try:
        yield "shared scores", SKIPS
    finally:
        assert seg.L.ns_ctx_share_scores(seg.ctx, 1) == 0


@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("and_mode", [False, True], ids=["or", "and"])
def test_ranked_queries_over_the_derived_segment(derived, k, and_mode):
    dv = derived
    for label, sid in configurations(dv["seg"]):
        qd, refs = rawseg.descriptors(Q_QUERIES, dv["ulists"], dv["noff"], Q_IDFS, Q_WEIGHTS, seg_id=sid)
        hits, nhits, found, _ = dv["seg"].run(qd, refs, k, AND if and_mode else nsbind.NS_FLAG_OR)
        rawseg.check_results(dv["ref"], hits, nhits, found, k, and_mode, label)
        assert np.all(hits["seg"][hits["doc"] != rawseg.PAD_ID] == sid)


@pytest.mark.parametrize("k", [1, 10, 100])
def test_boolean_queries_over_the_derived_segment(derived, k):
    dv = derived
    seg = dv["seg"]
    assert {r for q in dv["bqueries"] for _, _, r in q} == {S, M, X}
    segments = [(Q_N_DOCS, seg.doc_len, dv["ulists"])]
    want = boolean_ref.boolean_hits(segments, dv["bqueries"], k, None, [Q_IDFS], [Q_WEIGHTS], dv["bcache"])
    assert sum(1 for f, _ in want if f) >= 8
    roles = np.array([r for q in dv["bqueries"] for _, _, r in q], dtype=np.uint8)
    for label, sid in configurations(seg):
        qd, refs = rawseg.descriptors(Q_QUERIES, dv["ulists"], dv["noff"], Q_IDFS, Q_WEIGHTS, seg_id=sid)
        rc, hits, nhits, found, _ = nsbind.search_boolean_raw(seg.ctx, qd, refs, roles, k, [sid], [dv["h"][sid]])
        assert rc == 0, seg.err()
        boolean_ref.check(want, hits, nhits, found, k, label=label, ids=[sid])


def test_single_groups_alone_give_the_sources_hits(derived):
    seg = derived["seg"]
    h, noff, ncnt, _ = derive(seg, SINGLES, [[li] for li in reversed(range(len(Q_SIZES)))])
    try:
        assert [int(c) for c in ncnt] == Q_SIZES[::-1]
        queries = [q for q in Q_QUERIES if max(q) < 8]
        for k in (10, 100):
            for flags in (nsbind.NS_FLAG_OR, AND):
                qd, refs = rawseg.descriptors(queries, seg.lists, seg.offs, Q_IDFS, Q_WEIGHTS, seg_id=0)
                w_hits, w_nhits, w_found, _ = seg.run(qd, refs, k, flags)
                qd, refs = rawseg.descriptors(queries, seg.lists, noff[::-1], Q_IDFS, Q_WEIGHTS, seg_id=SINGLES)
                hits, nhits, found, _ = seg.run(qd, refs, k, flags)
                assert np.array_equal(nhits, w_nhits) and np.array_equal(found, w_found) and int(found.sum()) > 0
                assert np.array_equal(hits["doc"], w_hits["doc"])
                assert np.array_equal(hits["score"].view(np.uint32), w_hits["score"].view(np.uint32))
    finally:
        assert seg.L.ns_segment_release(seg.ctx, h) == 0


def test_source_and_derived_segment_are_released_in_either_order():
    rng = np.random.default_rng(4)
    lists = [(np.arange(0, 200, 2, dtype=np.uint32), np.ones(100, np.uint32)), (np.arange(100, dtype=np.uint32), np.full(100, 3, np.uint32))]
    for source_first in (True, False):
        seg = rawseg.RawSegment(200, rng.integers(1, 50, 200), lists)
        try:
            h, noff, ncnt, (off, cnt, gb) = derive(seg, 1, [[0, 1], [1]])
            ulists = union_ref.union(seg.flat.reshape(-1, 2), off, cnt, gb, 200)
            assert int(ncnt[0]) == 150
            if source_first:
                assert seg.L.ns_segment_release(seg.ctx, seg.seg) == 0
                seg.seg = None
            qd, refs = rawseg.descriptors([[0, 1]], ulists, noff, [1.5, 0.5], [1.0, 1.0], seg_id=1)
            hits, nhits, found, _ = seg.run(qd, refs, 10)
            rawseg.check_results(rawseg.reference(ulists, [[0, 1]], [1.5, 0.5], [1.0, 1.0], seg.doc_len, seg.avgdl), hits, nhits, found, 10)
            assert seg.L.ns_segment_release(seg.ctx, h) == 0
            if not source_first:                                                          # the id is free again, the source still serves
                h, _, ncnt, _ = derive(seg, 1, [[0, 1]])
                assert int(ncnt[0]) == 150 and seg.L.ns_segment_release(seg.ctx, h) == 0
        finally:
            seg.release()
