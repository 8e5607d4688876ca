"""Doc-tile body, terms on the skip grid: full rounds and the straight-line partial rounds of 1..4 chunks (pytest -m gpu).

Raw C-ABI on the fixture of tests/test_tile_exact_rounds_cpu.py (per-cell posting counts 0, 1, 63, 64, 65, ... 513, 1024 for
three dense lists, a short list, a last cell cut short by n_docs).  Tables are registered explicitly through
ns_segment_build_skips, so every list can be a grid term or a cursor term.  docIds, order, nhits, found and fp32 score BITS
must equal the reference's.  The reference here is the numpy fp32 restatement of src/api_engine.cpp:477-480 that the other
raw-ABI cases use (test_equal_scores_in_doc_tiles_and_skip_tables): the CPU oracle of tests/orc.py opens index directories and
takes neither raw lists nor caller-chosen idfs and query weights; test_gpu_parity.py holds that restatement to the oracle's
bits on generated indexes.
"""
import ctypes as C
import os

import numpy as np
import pytest
from conftest import VARIANTS_BUILD, VARIANTS_LIB, need_variants

import nsbind
from test_tile_exact_rounds_cpu import expected, make_fixture

pytestmark = pytest.mark.gpu

IDF = [1.7, 0.9, 2.3, 4.1]
# (list indices in accumulation order, idfs or None for IDF, weights or None for 1.0)
QUERIES = [
    ([0, 1, 2], None, None),
    ([2, 1, 0], None, None),                        # the same docs, another fp32 accumulation order
    ([0, 1], None, None),
    ([1, 2, 3], None, None),                        # the short list: a cursor term in the same tiles
    ([3, 0, 2, 1], None, None),
    ([2, 0], None, None),
    ([0, 0, 1], None, None),                        # one list named twice
    ([1, 0, 2], None, [1.0, 0.37, 1.0]),            # a non-unit query weight
]
# a batch of its own (a batch that names one list with two idfs never shares term scores, and the main batch must share)
ODD_QUERIES = [
    ([0, 1, 3], [3.0e9, 0.9, 4.1], None),           # an idf outside [2^-30, 2^30]: the full division
    ([2, 0], [2.3, 3.0e9], [1.0, 2.5]),
    ([1, 2], [0.9, 2.3], None),
]


def _upload(L, ctx, fx):
    payload = [np.stack([d, t], axis=1).astype(np.uint32).ravel() for d, t in fx["lists"]]
    flat = np.concatenate(payload)
    offs = np.cumsum([0] + [len(p) * 4 for p in payload])[:-1]
    seg = C.c_void_p()
    rc = L.ns_segment_upload(ctx, 0, fx["n_docs"], C.c_float(fx["avgdl"]), fx["doc_len"].ctypes.data, flat.ctypes.data, flat.nbytes, C.byref(seg))
    assert rc == 0, L.ns_last_error(ctx)
    return seg, offs


def _descs(fx, offs, queries):
    qd = np.zeros(len(queries), dtype=nsbind.QDESC_DTYPE)
    refs = []
    for qi, (q, idfs, wts) in enumerate(queries):
        qd[qi] = (len(refs), len(q))
        for j, li in enumerate(q):
            refs.append((0, len(fx["lists"][li][0]), int(offs[li]), idfs[j] if idfs else IDF[li], wts[j] if wts else 1.0))
    return qd, np.array(refs, dtype=nsbind.TERM_DTYPE)


def _check(fx, queries, hits, nhits, found, k, conj, label):
    for qi, (q, idfs, wts) in enumerate(queries):
        docs, bits, n_found = expected(fx, q, idfs or [IDF[li] for li in q], wts or [1.0] * len(q), k, conj)
        n = int(nhits[qi])
        print(f"{label} q{qi} k={k} and={conj}: found {int(found[qi])} / {n_found}, nhits {n} / {len(docs)}")
        assert int(found[qi]) == n_found, (label, qi, k, conj)
        assert n == len(docs), (label, qi, k, conj)
        assert [int(d) for d in hits[qi, :n]["doc"]] == docs.tolist(), (label, qi, k, conj)
        np.testing.assert_array_equal(hits[qi, :n]["score"].view(np.uint32), bits, err_msg=f"{label} q{qi} k={k} and={conj}")


# tables: 2 = for all four lists, 1 = for lists 0 and 2 (1 and 3 keep their cursors inside the same grid tiles), 0 = none
# split: 0 = the planner's own ranges, else a posting budget that forces several doc ranges (they start and end on the grid)
# share: shared term scores forced off (0: BM25 in place) or on (2: scores in the stream) — the two forms of the body
@pytest.mark.parametrize("variant,split,tables,share", [
    (0, 0, 2, 0), (0, 0, 2, 2), (0, 0, 1, 0), (0, 0, 1, 2), (0, 0, 0, 0), (0, 0, 0, 2),
    (0, 3000, 2, 0), (0, 3000, 2, 2), (0, 3000, 1, 2), (0, 900, 2, 0), (0, 900, 1, 0),
    (19, 0, 0, 0), (18, 300, 0, 0), (12, 0, 0, 0)])
def test_every_round_shape_on_the_skip_grid(variant, split, tables, share):
    need_variants(variant)
    fx = make_fixture()
    L = nsbind.hip_lib()
    ctx = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(ctx)) == 0
    try:
        seg, offs = _upload(L, ctx, fx)
        if tables:
            which = [0, 1, 2, 3] if tables == 2 else [0, 2]
            bo = np.array([offs[i] for i in which], dtype=np.uint64)
            cn = np.array([len(fx["lists"][i][0]) for i in which], dtype=np.uint32)
            assert L.ns_segment_build_skips(ctx, seg, bo.ctypes.data, cn.ctypes.data, len(which)) == 0, L.ns_last_error(ctx)
        assert L.ns_set_tuning(ctx, variant, 1 if split else 0, split) == 0
        assert L.ns_ctx_share_scores(ctx, share) == 0
        for queries in (QUERIES, ODD_QUERIES):
            qd, refs = _descs(fx, offs, queries)
            label = f"v{variant} split={split} tables={tables} share={share} {'main' if queries is QUERIES else 'odd idfs'}"
            for flags in (nsbind.NS_FLAG_OR, nsbind.NS_FLAG_AND):
                for k in (1, 10, 100):
                    b = nsbind.prepare_raw(ctx, qd, refs, k, flags)
                    b.run(timed=False)
                    b.sync()
                    hits, nhits, found = b.fetch()
                    inf = b.info()
                    b.close()
                    if variant == 0 and queries is QUERIES:   # the batch took the form of the body the case names
                        assert bool(inf.flags & nsbind.NS_INFO_SHARED) == (share == 2), label
                        if split:
                            assert inf.n_items > len(queries), (label, inf.n_items)
                    _check(fx, queries, hits, nhits, found, k, flags == nsbind.NS_FLAG_AND, label)
        assert L.ns_segment_release(ctx, seg) == 0
    finally:
        L.ns_ctx_destroy(ctx)


def test_forced_tile_variants_of_this_file_in_the_variants_build():
    """The cases above with a forced kernel variant (the doc-tile body as a kernel of its own, 512 / 1024 / 2048-doc tiles) need
    libnextsearch_hip_variants.so: ONE child process that loads that build runs them."""
    import subprocess
    import sys
    if VARIANTS_BUILD:
        pytest.skip("this IS the variants process")
    assert os.path.exists(VARIANTS_LIB), "libnextsearch_hip_variants.so is missing: make -C nextsearch-api_amd variants"
    env = dict(os.environ, NS_HIP_LIB=VARIANTS_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "every_round_shape"], env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], tail
