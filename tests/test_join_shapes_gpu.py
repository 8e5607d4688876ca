"""The top-K row join on the GPU: every directed family of tests/join_shapes.py on the product library against the numpy
restatement (found, nhits, segs, docs, score bits and the padding of the tail; OR, AND and shared term scores, under the
family's own tuning), and k_merge_ranks on synthetic rank rows against the numpy join.  That the families take the join
paths they declare is asserted on the CPU (tests/test_join_shapes_cpu.py) and, by counters, in the counting-build child of
tests/test_body_shapes_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import join_run
import join_shapes
import nsbind

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(join_shapes.FAMILIES))
def test_join_family_equals_numpy_restatement(name):
    ran = join_run.run_family(name)
    fam = join_shapes.FAMILIES[name]()
    assert sorted(set(ran)) == sorted(fam.ks) and len(ran) == 2 * len(fam.ks) + 2


@pytest.mark.parametrize("with_seg_map", [True, False], ids=["seg_map_reversed", "seg_map_null"])
@pytest.mark.parametrize("n_ranks", join_shapes.RANK_COUNTS)
def test_rank_join_on_synthetic_rows_equals_numpy_join(n_ranks, with_seg_map):
    """ns_merge_rank_rows on rows built in numpy: 1 to 64 ranks, K = 1 / 10 / 100, empty ranks and a query empty in every rank,
    nhits above K in the input, heavy ties across ranks under a seg_map that reverses the rank order (and without one),
    `found` sums past 2^32, 7 queries."""
    L = nsbind.hip_lib()
    ctx = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(ctx)) == 0
    try:
        for k in join_shapes.RANK_KS:
            join_run.run_rank_case(n_ranks, k, with_seg_map=with_seg_map, ctx=ctx)
    finally:
        L.ns_ctx_destroy(ctx)


def test_rank_join_refusals():
    """0 and 65 ranks, K = 0 and 101 are refused before anything is launched; no queries is not an error"""
    L = nsbind.hip_lib()
    ctx = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(ctx)) == 0
    dev = None
    try:
        hits, nhits, found, seg_map = join_shapes.rank_rows(2, 10)
        Q = join_shapes.RANK_QUERIES
        dev = join_run.DeviceArrays(hits, nhits, found, seg_map, np.full((Q, 10, 3), 7, np.int32), np.full(Q, 7, np.int32), np.full(Q, 7, np.int64))
        for n_ranks, k in ((0, 10), (65, 10), (2, 0), (2, nsbind.NS_MAX_K + 1)):
            assert join_run.merge_rank_rows(ctx, dev, n_ranks, Q, k, seg_map.shape[1]) != nsbind.NS_OK, (n_ranks, k)
            assert L.ns_last_error(ctx)
        assert join_run.merge_rank_rows(ctx, dev, 2, 0, 10, seg_map.shape[1]) == nsbind.NS_OK
        assert all(bool((dev.fetch(i) == 7).all()) for i in (4, 5, 6)), "a refused or empty call writes nothing"
    finally:
        if dev:
            dev.free()
        L.ns_ctx_destroy(ctx)
