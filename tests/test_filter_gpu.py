"""Filtered search on the device (csrc/ns_filter.hip behind ns_segment_filter, Engine::open_filter / search_filtered*;
DESIGN.md §5o).  The oracle is tests/filter_ref.py: the compaction restated in numpy, and tests/rawseg.py's fp32 restatement
of the scoring over lists masked the same way.  Integers, bytes and fp32 bit patterns: every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_ref
import nsbind
import rawseg
from test_compact_gpu import new_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NS_E_INVAL = -1
AND = nsbind.NS_FLAG_AND


# ---- 1: the raw ABI, array for array ------------------------------------------------------------------------------------
N_DOCS = 300                                                             # 9 whole bitmap words and 12 bits of a tenth
LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4099]


def make_stream(n, seed):
    """docId-ascending lists of 1..120 postings, n postings in all.  Document 0 is named by the first posting of the stream
    alone and document N_DOCS - 1 by the last one alone."""
    rng = np.random.default_rng(seed)
    lists, left = [], n
    while left:
        m = int(min(left, rng.integers(1, 121)))
        docs = np.sort(rng.choice(np.arange(1, N_DOCS - 1), m, replace=False)).astype(np.uint32)
        lists.append((docs, rng.integers(1, 9, m).astype(np.uint32)))
        left -= m
    if n:
        lists[0][0][0] = 0
        if n > 1:
            lists[-1][0][-1] = N_DOCS - 1
    return lists


@pytest.fixture(scope="module")
def streams():
    rng = np.random.default_rng(3)
    doc_len = rng.integers(1, 400, N_DOCS).astype(np.uint32)
    segs = rawseg.RawSegments([(N_DOCS, doc_len, make_stream(n, 100 + i)) for i, n in enumerate(LENGTHS)])
    yield segs
    segs.release()


def probe_lists(n, offs, counts):
    """the segment's own lists, then lists that overlap them: the whole stream, empty lists at both ends, and spans that
    start and end inside a chunk"""
    off, cnt = [int(o) for o in offs], [int(c) for c in counts]
    extra = [(0, n), (0, 0), (n, 0)]
    if n >= 130:
        extra += [(70, 60), (65, 1), (63, 2), (1, n - 2)]
    return np.array(off + [a * 8 for a, _ in extra], dtype=np.uint64), np.array(cnt + [c for _, c in extra], dtype=np.uint32)


@pytest.mark.parametrize("si", range(len(LENGTHS)), ids=[str(n) for n in LENGTHS])
def test_compaction_equals_the_restatement(streams, si):
    n, lists = LENGTHS[si], streams.lists[si]
    flat = streams._keep[si].reshape(-1, 2)
    assert len(flat) == n
    counts = np.array([len(d) for d, _ in lists], dtype=np.uint32)
    off, cnt = probe_lists(n, streams.offs[si], counts)
    docs = np.arange(N_DOCS)
    last_doc = int(flat[-1, 0]) if n else 0
    keeps = {"all": np.ones(N_DOCS, bool), "none": np.zeros(N_DOCS, bool), "alternating": docs % 2 == 0, "first": docs == 0, "last": docs == last_doc}
    for name, keep in keeps.items():
        bits = filter_ref.bits_of(keep, fill_tail=(name in ("all", "alternating")))   # the unused bits of the last word must not matter
        h, noff, ncnt, kept, ms, payload = nsbind.segment_filter(streams.ctx, streams.segs[si], 100, bits, off, cnt, payload_cap=n)
        try:
            w_payload, w_off, w_cnt, w_kept = filter_ref.compact(flat, off, cnt, keep)
            what = (n, name)
            assert kept == w_kept, what
            np.testing.assert_array_equal(payload, w_payload, err_msg=str(what))
            np.testing.assert_array_equal(ncnt, w_cnt, err_msg=str(what))
            np.testing.assert_array_equal(noff, w_off, err_msg=str(what))
            assert ms >= 0.0
            # what the bitmaps mean, stated without the restatement
            if name == "all":
                assert kept == n and np.array_equal(payload, flat)
            if name == "none":
                assert kept == 0 and not ncnt.any()
            if name == "first" and n:
                assert kept == 1 and np.array_equal(payload, flat[:1])
            if name == "last" and n:
                assert kept == 1 and np.array_equal(payload, flat[-1:])
        finally:
            assert streams.L.ns_segment_release(streams.ctx, h) == 0


def test_list_shapes_and_documents_out_of_range():
    """A list that starts and ends mid-chunk, a list of one posting, a list dropped entirely between two kept ones, two
    lists sharing one 64-posting chunk; n_docs no multiple of 32 with the unused bits set; a docId >= n_docs in the stream."""
    n_docs = 203
    rng = np.random.default_rng(9)
    low, high = np.arange(0, 150), np.arange(150, 200)
    pick = lambda pool, m: np.sort(rng.choice(pool, m, replace=False)).astype(np.uint32)
    a, b, c, d = pick(low, 40), pick(low, 50), pick(low, 1), pick(high, 30)          # [0, 40) [40, 90) [90, 91) [91, 121)
    e = np.concatenate([pick(low, 18), [n_docs + 5]]).astype(np.uint32)               # [121, 140): its last docId is out of range
    lists = [(x, rng.integers(1, 5, len(x)).astype(np.uint32)) for x in (a, b, c, d, e)]
    seg = rawseg.RawSegment(n_docs, rng.integers(1, 90, n_docs), lists)
    try:
        flat = seg.flat.reshape(-1, 2)
        for keep in (np.arange(n_docs) < 150, np.ones(n_docs, bool)):
            bits = filter_ref.bits_of(keep, fill_tail=True)
            h, noff, ncnt, kept, _, payload = nsbind.segment_filter(seg.ctx, seg.seg, 7, bits, seg.offs, seg.counts, payload_cap=len(flat))
            w_payload, w_off, w_cnt, w_kept = filter_ref.compact(flat, seg.offs, seg.counts, keep)
            assert kept == w_kept
            np.testing.assert_array_equal(payload, w_payload)
            np.testing.assert_array_equal(noff, w_off)
            np.testing.assert_array_equal(ncnt, w_cnt)
            assert ncnt[2] == 1 and ncnt[4] == 18                                      # the docId >= n_docs is dropped, set bits or not
            if not keep.all():
                assert list(ncnt) == [40, 50, 1, 0, 18] and noff[3] == noff[4] == 91 * 8
            else:
                assert kept == len(flat) - 1
            assert seg.L.ns_segment_release(seg.ctx, h) == 0
    finally:
        seg.release()


def test_refusals(streams):
    L, ctx, src = streams.L, streams.ctx, streams.segs[5]
    n = LENGTHS[5]
    bits = filter_ref.bits_of(np.ones(N_DOCS, bool))
    off, cnt = np.array([0], np.uint64), np.array([n], np.uint32)
    noff, ncnt = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    kept, h = C.c_uint64(), C.c_void_p()

    def call(ctx=ctx, src=src, new_id=100, bits_p=bits.ctypes.data, off_p=off.ctypes.data, cnt_p=cnt.ctypes.data, n_lists=1,
             noff_p=noff.ctypes.data, ncnt_p=ncnt.ctypes.data, out=C.byref(h)):
        return L.ns_segment_filter(ctx, src, new_id, bits_p, off_p, cnt_p, n_lists, noff_p, ncnt_p, None, C.byref(kept), None, out)

    assert call(ctx=None) == NS_E_INVAL
    assert call(src=None) == NS_E_INVAL and b"src is NULL" in streams.err()
    assert call(out=None) == NS_E_INVAL
    assert call(bits_p=None) == NS_E_INVAL and b"keep_bits" in streams.err()
    for null in ("off_p", "cnt_p", "noff_p", "ncnt_p"):
        assert call(**{null: None}) == NS_E_INVAL and b"null list arrays" in streams.err()
    assert call(new_id=3) == NS_E_INVAL and b"already uploaded" in streams.err()              # an id in use
    assert call(new_id=1 << 20) == NS_E_INVAL and b"too large" in streams.err()
    for bad_off, bad_cnt in ((0, n + 1), (n * 8, 1), (8, n), (4, 1)):                          # a list outside the source / misaligned
        o, c = np.array([bad_off], np.uint64), np.array([bad_cnt], np.uint32)
        assert call(off_p=o.ctypes.data, cnt_p=c.ctypes.data) == NS_E_INVAL
    # a pending source
    pend = C.c_void_p()
    dl = np.ones(4, np.uint32)
    assert L.ns_segment_upload_begin(ctx, 50, 4, C.c_float(1.0), dl.ctypes.data, 16, C.byref(pend)) == 0
    small = np.array([0xF], np.uint32)
    assert call(src=pend, bits_p=small.ctypes.data, n_lists=0) == NS_E_INVAL and b"has not ended" in streams.err()
    assert call(new_id=50) == NS_E_INVAL and b"being uploaded" in streams.err()
    assert L.ns_segment_release(ctx, pend) == 0
    assert not h.value
    # nothing was published by a refused call: the id is free
    assert call() == 0 and kept.value == n and ncnt[0] == n and noff[0] == 0
    h2 = C.c_void_p()
    assert call(new_id=100, out=C.byref(h2)) == NS_E_INVAL and b"already uploaded" in streams.err() and not h2.value
    assert L.ns_segment_release(ctx, h) == 0


# ---- 2: queries over a filtered segment ----------------------------------------------------------------------------------
Q_N_DOCS = 5003
Q_SIZES = [3000, 2500, 1800, 900, 400, 150, 64, 7, 300]                    # the last list: documents that are all dropped
Q_QUERIES = [[0], [5], [7], [0, 1], [2, 6], [4, 7], [0, 1, 2], [3, 5, 7], list(range(8)), [8], [1, 8], [0, 3, 8]]
Q_IDFS = [0.4, 0.7, 1.1, 1.9, 2.6, 3.3, 4.1, 5.5, 2.2]


@pytest.fixture(scope="module")
def filtered_segment():
    rng = np.random.default_rng(21)
    keep = rng.random(Q_N_DOCS) < 0.5
    dropped = np.flatnonzero(~keep)
    lists = []
    for i, m in enumerate(Q_SIZES):
        pool = dropped if i == 8 else np.arange(Q_N_DOCS)
        docs = np.sort(rng.choice(pool, m, replace=False)).astype(np.uint32)
        lists.append((docs, rng.integers(1, 12, m).astype(np.uint32)))
    seg = rawseg.RawSegment(Q_N_DOCS, rng.integers(1, 500, Q_N_DOCS), lists)
    h, noff, ncnt, kept, _, _ = nsbind.segment_filter(seg.ctx, seg.seg, 1, filter_ref.bits_of(keep), seg.offs, seg.counts)
    masked = filter_ref.mask_lists(lists, keep)
    assert [int(c) for c in ncnt] == [len(d) for d, _ in masked] and ncnt[8] == 0 and kept == int(ncnt.sum())
    weights = [1.0] * len(lists)
    ref = filter_ref.reference(lists, Q_QUERIES, Q_IDFS, weights, seg.doc_len, seg.avgdl, keep)   # once, shared, never changed
    yield {"seg": seg, "h": h, "noff": noff, "ncnt": ncnt, "masked": masked, "ref": ref, "weights": weights}
    seg.L.ns_segment_release(seg.ctx, h)
    seg.release()


def run_filtered(fs, k, and_mode):
    queries = filter_ref.filtered_queries(Q_QUERIES, fs["masked"], and_mode)
    qd, refs = rawseg.descriptors(queries, fs["masked"], fs["noff"], Q_IDFS, fs["weights"], seg_id=1)
    return fs["seg"].run(qd, refs, k, AND if and_mode else nsbind.NS_FLAG_OR)


@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("and_mode", [False, True], ids=["or", "and"])
def test_queries_over_the_filtered_segment(filtered_segment, k, and_mode):
    fs = filtered_segment
    hits, nhits, found, _ = run_filtered(fs, k, and_mode)
    rawseg.check_results(fs["ref"], hits, nhits, found, k, and_mode, "filtered")
    assert int(found[9]) == 0 and int(nhits[9]) == 0                                   # the one list lost every posting
    if and_mode:
        assert int(found[10]) == 0 and int(found[11]) == 0                               # and takes its AND groups with it


def test_queries_with_skip_tables_and_shared_scores(filtered_segment):
    fs = filtered_segment
    seg = fs["seg"]
    which = np.flatnonzero(fs["ncnt"] >= 64)
    bo, cn = np.ascontiguousarray(fs["noff"][which]), np.ascontiguousarray(fs["ncnt"][which])
    assert len(which) >= 5
    assert seg.L.ns_segment_build_skips(seg.ctx, fs["h"], bo.ctypes.data, cn.ctypes.data, len(which)) == 0, seg.err()
    for and_mode in (False, True):
        hits, nhits, found, _ = run_filtered(fs, 10, and_mode)
        rawseg.check_results(fs["ref"], hits, nhits, found, 10, and_mode, "filtered + skips")
    assert seg.L.ns_ctx_share_scores(seg.ctx, 2) == 0
    try:
        for and_mode in (False, True):
            hits, nhits, found, _ = run_filtered(fs, 10, and_mode)
            rawseg.check_results(fs["ref"], hits, nhits, found, 10, and_mode, "filtered + shared scores")
    finally:
        assert seg.L.ns_ctx_share_scores(seg.ctx, 1) == 0


def test_source_and_copy_are_released_in_either_order():
    rng = np.random.default_rng(4)
    lists = [(np.arange(0, 200, 2, dtype=np.uint32), np.ones(100, np.uint32)), (np.arange(100, dtype=np.uint32), np.full(100, 3, np.uint32))]
    seg = rawseg.RawSegment(200, rng.integers(1, 50, 200), lists)
    try:
        keep = np.arange(200) % 3 != 0
        h, noff, ncnt, _, _, _ = nsbind.segment_filter(seg.ctx, seg.seg, 1, filter_ref.bits_of(keep), seg.offs, seg.counts)
        assert seg.L.ns_segment_release(seg.ctx, seg.seg) == 0                           # the source goes first
        seg.seg = None
        masked = filter_ref.mask_lists(lists, keep)
        qd, refs = rawseg.descriptors([[0, 1]], masked, noff, [1.5, 0.5], [1.0, 1.0], seg_id=1)
        hits, nhits, found, _ = seg.run(qd, refs, 10)
        rawseg.check_results(filter_ref.reference(lists, [[0, 1]], [1.5, 0.5], [1.0, 1.0], seg.doc_len, seg.avgdl, keep), hits, nhits, found, 10)
        assert seg.L.ns_segment_release(seg.ctx, h) == 0
    finally:
        seg.release()


# ---- 3: the engine ------------------------------------------------------------------------------------------------------
WORDS = ["w%03d" % i for i in range(90)]
QUERIES = ["w000", "w001 w002", "w003 w010 w020", "w000 w001 w002 w005 w009 w015 w030 w060", "w080", "w089 w000", "zzzzqq w004",
           "zzzzqq", "the of", "", "w002 W002", "w007;w011"]


def make_docs(seg, n, seed):
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(len(WORDS)) + 2.0)
    p /= p.sum()
    docs = []
    for i in range(n):
        m = int(rng.integers(8, 40))
        text = " ".join(WORDS[j] for j in rng.choice(len(WORDS), m, p=p))
        docs.append((b"s%dd%04d" % (seg, i), b"Title %d" % i, b"pdf_json/%d_%d.json" % (seg, i), text.encode()))
    return docs


def make_index(tmp, name, n_docs):
    """Three add_documents segments; segments 0 and 1 hold the SAME texts (every score ties across them).  Dates: segment 0
    2018 .. 2019, segment 1 2020 by month, segment 2 2021, year only, undated or without a row; one document on 2021-12-25."""
    index = str(tmp / name)
    batches = [make_docs(0, n_docs, 1), make_docs(1, n_docs, 1), make_docs(2, n_docs - 30, 2)]
    eng = new_engine(index, batches)
    lines = ["cord_uid,title,publish_time,authors,url"]
    for s, b in enumerate(batches):
        for i, d in enumerate(b):
            if s == 0:
                t = "%04d-%02d-%02d" % (2018 + i % 2, 1 + i % 12, 1 + i % 28)
            elif s == 1:
                t = "2020-%02d" % (1 + i % 12) if i % 3 else "2020-%02d-%02d" % (1 + i % 12, 1 + i % 28)
            else:
                r = i % 5
                if r == 4:
                    continue                                                              # no row
                t = ["2021-%02d-%02d" % (1 + i % 11, 1 + i % 24), "2021", "", "2021-%02d" % (1 + i % 11)][r]
                if i == 17:
                    t = "2021-12-25"
            lines.append("%s,T,%s,A B,http://x" % (d[0].decode(), t))
    with open(os.path.join(index, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.reload()
    return index, eng


@pytest.fixture(scope="module")
def served(tmp_path_factory):
    index, eng = make_index(tmp_path_factory.mktemp("filter_gpu"), "index", 260)
    S = eng.num_segments
    assert S == 3
    info = [eng.segment_info(s) for s in range(S)]
    post = [eng.segment_postings(s) for s in range(S)]
    dl = [eng.segment_doc_len(s) for s in range(S)]
    # per segment: the lists of every word the lexicon holds, in WORDS order
    seg_lists, seg_idfs, where = [], [], []
    for s in range(S):
        lists, idfs, at = [], [], {}
        for w in WORDS:
            lk = eng.lookup(s, w)
            if lk is None or lk["df"] == 0:
                continue
            a = lk["byte_off"] // 8
            at[w] = len(lists)
            lists.append((post[s][a:a + lk["count"], 0].copy(), post[s][a:a + lk["count"], 1].copy()))
            idfs.append(np.float32(lk["idf"]))
        seg_lists.append(lists)
        seg_idfs.append(idfs)
        where.append(at)
    yield {"index": index, "eng": eng, "S": S, "info": info, "dl": dl, "post": post, "lists": seg_lists, "idfs": seg_idfs, "where": where}
    eng.close()


def terms_of(query):
    import re
    stop = {"the", "of", "and", "a"}
    return [t for t in re.findall(r"[a-z0-9]+", query.lower()) if len(t) >= 2 and t not in stop]


def expected(sv, queries, keeps):
    """filter_ref over the engine's own postings and lexicons: per query (OR ranking, AND ranking), and usable"""
    refq = [[(s, sv["where"][s][t]) for s in range(sv["S"]) for t in terms_of(q) if t in sv["where"][s]] for q in queries]
    segments = [(sv["info"][s]["n_docs"], sv["dl"][s], sv["lists"][s]) for s in range(sv["S"])]
    weights = [[1.0] * len(sv["lists"][s]) for s in range(sv["S"])]
    avgdls = [sv["info"][s]["avgdl"] for s in range(sv["S"])]                           # the engine's own (stats.bin)
    return filter_ref.reference_multi(segments, refq, sv["idfs"], weights, keeps, avgdls), [1 if terms_of(q) else 0 for q in queries]


def check_filter(sv, bits, handle, queries=QUERIES, ks=(1, 10, 100)):
    keeps = [filter_ref.keep_of(bits[s], sv["info"][s]["n_docs"]) for s in range(sv["S"])]
    ref, usable = expected(sv, queries, keeps)
    for and_mode in (False, True):
        for k in ks:
            hits, nhits, found, has = sv["eng"].search_filtered_batch(handle, queries, k, AND if and_mode else 0)
            assert list(has) == usable
            rawseg.check_results_multi(ref, hits, nhits, found, k, and_mode, "engine")
    return ref, keeps


def test_keep_all_equals_the_unfiltered_search_byte_for_byte(served):
    eng = served["eng"]
    h = eng.open_filter("", "", keep_undated=True)
    try:
        for flags in (0, AND):
            for k in (1, 10, 100):
                a, b = eng.search_filtered_batch(h, QUERIES, k, flags), eng.search_batch(QUERIES, k, flags)
                for x, y in zip(a, b):
                    assert x.tobytes() == y.tobytes(), (flags, k)
        assert int(a[2][0]) > 100                                                       # the queries do find documents
    finally:
        eng.close_filter(h)
    assert eng.open_filters() == 0


@pytest.mark.parametrize("name,date_from,date_to,undated", [("half", "2019-01", "2020-06", False), ("one segment", "2020", "2020", False),
                                                            ("one document", "2021-12-25", "2021-12-25", False), ("nothing", "2030", "", False),
                                                            ("undated too", "2021-06", "", True)])
def test_date_ranges(served, name, date_from, date_to, undated):
    sv, eng = served, served["eng"]
    bits = eng.filter_bits(date_from, date_to, undated)
    h, st = eng.open_filter(date_from, date_to, undated, stats=True)
    try:
        ref, keeps = check_filter(sv, bits, h)
        kept = [int(k.sum()) for k in keeps]
        total = sum(sv["info"][s]["n_docs"] for s in range(sv["S"]))
        assert st["docs_kept"] == sum(kept) and st["docs_total"] == total
        assert st["postings_total"] == sum(sv["info"][s]["n_postings"] for s in range(sv["S"]))
        want_postings = sum(int(keeps[s][sv["post"][s][:, 0].astype(np.int64)].sum()) for s in range(sv["S"]))   # the whole streams
        assert st["postings_kept"] == want_postings
        if name == "half":
            assert 0.3 * total < sum(kept) < 0.7 * total and kept[0] and kept[1] and not kept[2] and st["segments_on_device"] == 2
            r = ref[0][0][:100]                                                         # the tie rule after the id mapping: equal
            assert any(a[0] == b[0] and a[1] < b[1] for a, b in zip(r, r[1:]))          # scores, segment 0 in front of segment 1
        if name == "one segment":
            assert kept == [0, sv["info"][1]["n_docs"], 0] and st["segments_on_device"] == 1
        if name == "one document":
            assert kept == [0, 0, 1] and st["segments_on_device"] == 1
        if name == "nothing":
            assert sum(kept) == 0 and st["segments_on_device"] == 0 and st["hbm_bytes"] == 0
            hits, nhits, found, has = eng.search_filtered_batch(h, ["w000"], 10)
            assert int(has[0]) == 1 and int(found[0]) == 0 and int(nhits[0]) == 0         # usable, found = 0
        if name == "undated too":
            assert kept[0] == 0 and kept[1] == 0 and kept[2] > 100
    finally:
        eng.close_filter(h)


def test_and_mode_with_a_list_emptied_in_one_segment_only(served):
    """A caller's bitmaps: segment 0 loses every document that holds w003, segments 1 and 2 keep all.  Under AND the query
    "w003 w001" has no match in segment 0 (its kept documents that hold w001 do not hold w003) but keeps its matches elsewhere;
    under OR segment 0 still contributes the documents of w001."""
    sv, eng = served, served["eng"]
    bits = [filter_ref.bits_of(np.ones(sv["info"][s]["n_docs"], bool)) for s in range(sv["S"])]
    keep0 = np.ones(sv["info"][0]["n_docs"], bool)
    keep0[np.asarray(sv["lists"][0][sv["where"][0]["w003"]][0], np.int64)] = False
    assert 0 < keep0.sum() < len(keep0)
    bits[0] = filter_ref.bits_of(keep0, fill_tail=True)
    h = eng.open_filter(bits=bits)
    try:
        queries = ["w003 w001", "w001 w003 w000", "w003", "w001"]
        ref, _ = check_filter(sv, bits, h, queries)
        assert all(s != 0 for _, s, _ in ref[0][1]) and any(s == 1 for _, s, _ in ref[0][1])   # AND: none of segment 0
        assert any(s == 0 for _, s, _ in ref[0][0])                                               # OR: segment 0 is there
        assert all(s != 0 for _, s, _ in ref[2][0])
    finally:
        eng.close_filter(h)


def test_capacity_and_handles(served):
    eng = served["eng"]
    bits = eng.filter_bits("2020", "2020")
    hs = [eng.open_filter(bits=bits) for _ in range(8)]
    try:
        assert len(set(hs)) == 8 and eng.open_filters() == 8
        with pytest.raises(RuntimeError, match="8 filters are open"):
            eng.open_filter(bits=bits)
        with pytest.raises(RuntimeError, match="8 filters are open"):
            eng.search_filtered_json("w000", 5, "2019", "2019")
        eng.close_filter(hs[3])
        with pytest.raises(RuntimeError, match="stale"):
            eng.close_filter(hs[3])
        with pytest.raises(RuntimeError, match="stale"):
            eng.search_filtered_batch(hs[3], ["w000"], 5)
        hs[3] = eng.open_filter(bits=bits)                                              # close_filter freed a slot
        a = eng.search_filtered_batch(hs[3], QUERIES, 10)
        b = eng.search_filtered_batch(hs[0], QUERIES, 10)                               # the same filter in another slot: the same answers
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        with pytest.raises(RuntimeError, match="bitmaps|words"):
            eng.open_filter(bits=bits[:2])
    finally:
        for h in hs:
            eng.close_filter(h)
    assert eng.open_filters() == 0


def test_handles_are_stale_after_reload_delete_and_compact(tmp_path):
    index, eng = make_index(tmp_path, "small", 60)
    try:
        h = eng.open_filter("2020", "2020")
        eng.search_filtered_json("w000", 5, "2018", "2019")
        assert eng.open_filters() == 2
        eng.reload()
        assert eng.open_filters() == 0
        with pytest.raises(RuntimeError, match="stale"):
            eng.search_filtered_batch(h, ["w000"], 5)
        h = eng.open_filter("2020", "2020")
        eng.delete_documents(["s1d0003"])
        assert eng.open_filters() == 0
        with pytest.raises(RuntimeError, match="stale"):
            eng.search_filtered_batch(h, ["w000"], 5)
        h2 = eng.open_filter("2020", "2020")
        assert h2 != h
        eng.compact()
        assert eng.open_filters() == 0 and eng.num_segments == 1
        with pytest.raises(RuntimeError, match="stale"):
            eng.close_filter(h2)
        h3 = eng.open_filter("2020", "2020")                                            # and the engine goes on serving filters
        hits, nhits, found, has = eng.search_filtered_batch(h3, ["w000"], 5)
        assert int(has[0]) == 1 and 0 < int(found[0]) < 60
        eng.close_filter(h3)
    finally:
        eng.close()


def filter_json(date_from, date_to, documents, keep_undated):
    return ('  "filter": {\n    "date_from": "%s",\n    "date_to": "%s",\n    "documents": %d,\n    "keep_undated": %s\n  },\n'
            % (date_from, date_to, documents, "true" if keep_undated else "false"))


def test_json_is_the_search_body_plus_the_filter_object(served):
    sv, eng = served, served["eng"]
    try:
        for q, k, f, t, u in (("w001 w002", 5, "2019-01", "2020-06", False), ("w000", 200, " 2020 ", "2020", True), ("the of", 10, "", "2019", False),
                              ("zzzzqq", 10, "2020", "", False), ("w003", 3, "2030", "", False)):
            bits = eng.filter_bits(f, t, u)
            docs = sum(int(filter_ref.keep_of(bits[s], sv["info"][s]["n_docs"]).sum()) for s in range(sv["S"]))
            h = eng.open_filter(f, t, u)
            K = nsbind.clamp_k(k)
            hits, nhits, found, has = eng.search_filtered_batch(h, [q], k)
            eng.close_filter(h)
            body = eng.hits_to_json(q, K, bool(has[0]), int(found[0]), hits[0, :int(nhits[0])])   # search's own entries for these hits
            assert body.startswith("{\n")
            want = "{\n" + filter_json(f.strip(), t.strip(), docs, u) + body[2:]
            assert eng.search_filtered_json(q, k, f, t, u) == want, (q, k, f, t, u)
        assert '"publish_time": "2020' in eng.search_filtered_json("w000", 3, "2020", "2020")   # decorated like search's hits
    finally:
        eng.reload()                                                                    # closes the filters the JSON calls left open
    assert eng.open_filters() == 0


def opens_since(eng, bits, mark):
    """how many filters were opened since `mark` (a handle): handles are never reused, handle // 8 counts the opens"""
    h = eng.open_filter(bits=bits)
    eng.close_filter(h)
    return h // 8 - mark // 8 - 1, h


def test_lru_of_search_filtered(served):
    eng = served["eng"]
    assert eng.open_filters() == 0
    bits = eng.filter_bits("2020", "2020")
    years = {"A": ("2018", "2018"), "B": ("2019", "2019"), "C": ("2020", "2020"), "D": ("2021", "2021"), "E": ("2018", "2021")}
    ask = lambda name: eng.search_filtered_json("w000", 3, *years[name])
    try:
        _, mark = opens_since(eng, bits, 0)
        for i, name in enumerate("ABCD"):
            ask(name)
            assert eng.open_filters() == i + 1
        n, mark = opens_since(eng, bits, mark)
        assert n == 4
        ask("E")                                                                        # a fifth distinct filter: A, the oldest, goes
        assert eng.open_filters() == 4
        for name in "BCDE":
            ask(name)                                                                   # all four are hits
        n, mark = opens_since(eng, bits, mark)
        assert n == 1 and eng.open_filters() == 4
        ask("A")                                                                        # a miss: B is now the oldest and goes
        for name in "CDEA":
            ask(name)
        n, mark = opens_since(eng, bits, mark)
        assert n == 1 and eng.open_filters() == 4
        ask("B")
        n, mark = opens_since(eng, bits, mark)
        assert n == 1 and eng.open_filters() == 4
        assert ask("C") == ask("C")                                                     # a hit answers what the miss answered
        # the cache's filters count towards the 8: four more are all that fit
        hs = [eng.open_filter(bits=bits) for _ in range(4)]
        with pytest.raises(RuntimeError, match="8 filters are open"):
            eng.open_filter(bits=bits)
        ask("D")                                                                        # the cache still turns over inside its four
        assert eng.open_filters() == 8
        for h in hs:
            eng.close_filter(h)
    finally:
        eng.reload()
    assert eng.open_filters() == 0


def test_two_contexts_on_one_device_give_the_single_context_answers(served):
    eng = served["eng"]
    two = nsbind.Engine(served["index"], [0, 0])
    try:
        assert two.num_devices == 2
        h1, h2 = eng.open_filter("2019-01", "2020-06"), two.open_filter("2019-01", "2020-06")
        for flags in (0, AND):
            a, b = eng.search_filtered_batch(h1, QUERIES * 3, 10, flags), two.search_filtered_batch(h2, QUERIES * 3, 10, flags)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
        u = two.search_batch(QUERIES * 3, 10)                                           # the sharded unfiltered path is what it was
        v = eng.search_batch(QUERIES * 3, 10)
        for x, y in zip(u, v):
            assert x.tobytes() == y.tobytes()
        eng.close_filter(h1)
    finally:
        two.close()


def test_ns_tool_search_filtered(served):
    eng = served["eng"]
    tool = os.path.join(ROOT, "nextsearch-api_amd", "ns_tool")
    try:
        want = eng.search_filtered_json("w001 w002", 5, "2019-01", "2020-06")
        out = subprocess.run([tool, "search-filtered", served["index"], "2019-01", "2020-06", "5", "w001", "w002"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout == want + "\n"
        want = eng.search_filtered_json("w000", 3, "", "2019")
        out = subprocess.run([tool, "search-filtered", served["index"], "-", "2019", "3", "w000"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout == want + "\n"
        bad = subprocess.run([tool, "search-filtered", served["index"], "2019-13", "-", "3", "w000"], capture_output=True, text=True, timeout=120)
        assert bad.returncode == 1 and "is not YYYY, YYYY-MM or YYYY-MM-DD" in bad.stderr
    finally:
        eng.reload()
