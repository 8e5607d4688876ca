"""The radix sort and the scans of csrc/ns_invert.hip on the shapes of tests/radix_shapes.py: every case of the table through the
raw ns_invert_forward against oracle/invert_oracle.invert, one through ns_segment_upload_inverted, and the sorts of
ns_forward_build (ig_sort) at 11 bits and with three passes against tests/ingest_ref.py.  Integers and bytes only: every
comparison is exact.  What each case reaches is asserted without a device in tests/test_radix_shapes_cpu.py; here the library's
own ns_radix_plan must be the plan those flags were computed from."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import ingest_ref
import nsbind
import radix_shapes as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import invert_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5C3A5C3


@pytest.fixture(scope="module")
def L():
    return nsbind.hip_lib()


@pytest.fixture(scope="module")
def T(L):
    return int(L.ns_radix_tile())


@pytest.fixture(scope="module")
def ctx(L):
    h = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(h)) == 0
    yield h
    L.ns_ctx_destroy(h)


def device_plan(L, key_range):
    pb = (C.c_uint32 * 3)()
    passes = L.ns_radix_plan(key_range, pb)
    return list(pb)[:passes]


def assert_case(L, ctx, case):
    """ns_invert_forward on one case: kept, df and postings[:kept] are the oracle's, the bytes past kept keep the sentinel"""
    assert device_plan(L, case.n_terms) == rs.plan(case.n_terms)[1], case.name       # the reach flags describe this build
    counts, pairs = np.ascontiguousarray(case.counts), np.ascontiguousarray(case.pairs)
    n = len(pairs)
    want_df, want = invert_oracle.invert(counts, pairs, case.n_terms)
    df = np.full(case.n_terms, SENTINEL, dtype=np.uint32)
    out = np.full((n, 2), SENTINEL, dtype=np.uint32)
    kept = C.c_uint64(SENTINEL)
    rc = L.ns_invert_forward(ctx, counts.ctypes.data, len(counts), pairs.ctypes.data, n, case.n_terms, df.ctypes.data, out.ctypes.data, C.byref(kept), None)
    assert rc == 0, (case.name, L.ns_last_error(ctx))
    assert kept.value == len(want), case.name
    assert np.array_equal(df, want_df), case.name
    if not np.array_equal(out[:len(want)], want):
        bad = np.flatnonzero((out[:len(want)] != want).any(axis=1))
        raise AssertionError("%s: %d of %d postings differ, the first at %d: %s, not %s" % (case.name, len(bad), len(want), bad[0], out[bad[0]], want[bad[0]]))
    assert (out[len(want):] == SENTINEL).all(), case.name
    return len(want)


@pytest.mark.parametrize("group", ["inst", "docs", "digit", "drop"])
def test_the_case_table_through_ns_invert_forward(L, T, ctx, group):
    cases = [c for c in rs.small_cases(T) if c.group == group]
    assert len(cases) >= 3
    kept = {c.name: assert_case(L, ctx, c) for c in cases}
    if group == "drop":
        assert kept["all_dropped"] == 0 and kept["one_kept"] == 1 and kept["kept_2T_of_4T"] == 2 * T


def test_three_passes_over_2_to_the_24_terms(L, T, ctx):
    (case,) = rs.huge_cases(T)
    assert device_plan(L, case.n_terms) == [9, 8, 8]
    assert assert_case(L, ctx, case) == 3 * T + 17


@pytest.mark.parametrize("name", ["scan_one_round_full", "scan_two_rounds"])
def test_the_scan_of_2_to_the_20_counters_and_of_more(L, T, ctx, name):
    (case,) = [c for c in rs.scan_cases(T) if c.name == name]
    blocks = (2048 * -(-len(case.pairs) // T) + 1023) // 1024                        # the block sums k_iv_scan_top scans, 1024 per round
    assert device_plan(L, case.n_terms) == [11] and blocks == (1024 if name == "scan_one_round_full" else 1028)
    assert_case(L, ctx, case)


def test_an_upload_whose_first_and_last_tile_are_dropped(L, T, ctx):
    """ns_segment_upload_inverted announces 4 T postings and keeps 2 T: the padding moves in front of a much shorter stream.  The
    segment serves what a segment uploaded from the oracle's lists serves."""
    case = rs.upload_case(T)
    counts, pairs, n_terms = np.ascontiguousarray(case.counts), np.ascontiguousarray(case.pairs), case.n_terms
    n_docs, n_pairs = len(counts), len(pairs)
    assert device_plan(L, n_terms) == rs.plan(n_terms)[1]
    df, postings = invert_oracle.invert(counts, pairs, n_terms)
    postings = np.ascontiguousarray(postings, dtype=np.uint32)
    assert len(postings) == 2 * T
    doc_len = np.maximum(1, np.bincount(np.repeat(np.arange(n_docs), counts), weights=pairs[:, 1], minlength=n_docs)).astype(np.uint32)
    avgdl = float(np.float32(doc_len.astype(np.float64).mean()))
    s_ref, s_dev = C.c_void_p(), C.c_void_p()
    assert L.ns_segment_upload(ctx, 0, n_docs, C.c_float(avgdl), doc_len.ctypes.data, postings.ctypes.data, postings.nbytes, C.byref(s_ref)) == 0
    try:
        assert L.ns_segment_upload_begin(ctx, 1, n_docs, C.c_float(avgdl), doc_len.ctypes.data, n_pairs * 8, C.byref(s_dev)) == 0
        try:
            df_out = np.full(n_terms, SENTINEL, dtype=np.uint32)
            host_copy = np.full((n_pairs, 2), SENTINEL, dtype=np.uint32)
            kept = C.c_uint64()
            assert L.ns_segment_upload_inverted(ctx, s_dev, counts.ctypes.data, pairs.ctypes.data, n_pairs, n_terms, df_out.ctypes.data,
                                                host_copy.ctypes.data, C.byref(kept), None) == 0, L.ns_last_error(ctx)
            assert kept.value == len(postings) and np.array_equal(df_out, df)
            assert np.array_equal(host_copy[:kept.value], postings) and (host_copy[kept.value:] == SENTINEL).all()
            assert L.ns_segment_upload_end(ctx, s_dev) == 0, L.ns_last_error(ctx)
            starts = np.concatenate([[0], np.cumsum(df, dtype=np.int64)])
            order = np.argsort(-df.astype(np.int64), kind="stable")
            rng = np.random.default_rng(3)
            queries = [[int(order[0]), int(order[1])], [int(order[2])], [int(order[np.count_nonzero(df) - 1])]]      # the last: the shortest list
            queries += [[int(t) for t in rng.choice(np.flatnonzero(df), size=rng.integers(1, 6), replace=False)] for _ in range(20)]
            res = []
            for sid in (0, 1):
                qd = np.zeros(len(queries), dtype=nsbind.QDESC_DTYPE)
                refs = []
                for qi, q in enumerate(queries):
                    qd[qi] = (len(refs), len(q))
                    for t in q:
                        refs.append((sid, int(df[t]), int(starts[t]) * 8, 1.0 + (t % 7) * 0.25, 1.0))
                rc, hits, nhits, found = nsbind.search_batch_raw(ctx, qd, np.array(refs, dtype=nsbind.TERM_DTYPE), 10)
                assert rc == 0, L.ns_last_error(ctx)
                res.append((hits, nhits, found))
            (h0, n0, f0), (h1, n1, f1) = res
            assert n0.tobytes() == n1.tobytes() and f0.tobytes() == f1.tobytes() and int(f0.sum()) > 0
            for q in range(len(queries)):
                k = int(n0[q])
                assert h0[q, :k]["doc"].tobytes() == h1[q, :k]["doc"].tobytes() and h0[q, :k]["score"].tobytes() == h1[q, :k]["score"].tobytes(), q
        finally:
            L.ns_segment_release(ctx, s_dev)
    finally:
        L.ns_segment_release(ctx, s_ref)


def assert_forward(got, want, want_kept_docs):
    assert np.array_equal(got["kept_docs"], want_kept_docs)
    for k in ("doc_len", "counts", "pairs"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert got["terms"] == want["terms"]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_the_sorts_of_ns_forward_build_at_11_bits(L, ctx, which):
    name, texts, by_term, by_doc = rs.ingest_corpora()[which]
    want = ingest_ref.build(texts)
    got = nsbind.forward_build(ctx, texts)
    assert_forward(got, want, want["kept_docs"])
    info = got["info"]
    assert info["n_docs"] == len(texts) and info["n_terms"] == len(want["terms"])
    assert device_plan(L, info["n_terms"]) == by_term and device_plan(L, info["n_docs"]) == by_doc, name
    assert 11 in by_term + by_doc


def test_the_sort_by_document_in_three_passes(L, ctx):
    """ns_forward_build over 2^22 + 1 documents of which about 2000 hold text: the sort by document takes three passes of 8 bits
    and the scan over the documents several rounds of k_iv_scan_top.  Against ingest_ref.build over the non-empty documents, the
    kept documents mapped back through their indices (the CPU file shows that this is build over all of them)."""
    n_docs = (1 << 22) + 1
    assert device_plan(L, n_docs) == [8, 8, 8]
    ids, texts = rs.sparse_corpus(n_docs)
    want = ingest_ref.build(texts)
    got = nsbind.forward_build_raw(ctx, b"".join(texts), rs.sparse_offsets(n_docs, ids, texts))
    assert got["info"]["n_docs"] == n_docs and got["info"]["kept_docs"] == len(ids)
    assert_forward(got, want, ids[want["kept_docs"]].astype(np.uint32))
    assert got["kept_docs"][0] == 0 and got["kept_docs"][-1] == n_docs - 1
