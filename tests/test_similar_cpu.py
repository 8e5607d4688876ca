"""The "more like this" selection rule without a device: the one-thread host restatement
(host/similar.hpp behind nsh_similar_select_host) against the numpy restatement (tests/similar_ref.py) on seeded corpora and
on the directed shapes, the clamps and the boost weights, the df / idf builder of a host-only engine, and the failures a
call makes without a device or without forward files.  Integers and fp32 bit patterns: every comparison is exact."""
import os
import sys

import numpy as np
import pytest

import ingest_ref
import nsbind
import similar_ref
import similar_shapes
from similar_shapes import assert_rows_equal
from test_delete_cpu import make_index, three_batches
from test_ingest_gpu import gen_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import invert_oracle  # noqa: E402

CUT = 2048          # any cut serves the host restatement; the GPU tests take the library's


@pytest.mark.parametrize("seed,n_docs,words,vocab", [(1, 300, 40, 400), (2, 120, 400, 3000), (3, 40, 3000, 20000)])
def test_host_restatement_equals_the_numpy_one_on_seeded_corpora(seed, n_docs, words, vocab):
    fwd = ingest_ref.build(gen_corpus(seed, n_docs, words, vocab=vocab, long_tokens=()))
    n = len(fwd["counts"])
    df, _ = invert_oracle.invert(fwd["counts"], fwd["pairs"], len(fwd["terms"]))
    idf = similar_shapes.idf_of(n, df)
    assert n > 30 and int(df.min()) >= 1 and float(idf.min()) > 0
    docs = np.arange(n, dtype=np.uint32)
    some = 0
    for T in similar_shapes.T_VALUES + (0, 1000):
        for opts in [(1, 1, 0xFFFFFFFF), (2, 2, n // 2), (1, 3, 0xFFFFFFFF)]:
            want = similar_ref.select_rows(fwd["counts"], fwd["pairs"], df, idf, docs, T, *opts)
            got = nsbind.similar_select_host(fwd, df, idf, docs, T, *opts)
            assert_rows_equal(got, want, (seed, T, opts))
            assert got[0].shape[1] == similar_ref.clamp_terms(T)
            some += int(want[2].sum())
    assert some > 10 * n                                               # the comparison is not vacuous


@pytest.fixture(scope="module")
def shapes():
    return similar_shapes.directed(CUT)


def test_host_restatement_on_the_directed_shapes(shapes):
    part, df, idf, docs = shapes
    ids = np.asarray(sorted(docs.values()) + [docs["n65"], docs["n65"]], dtype=np.uint32)
    for T in similar_shapes.T_VALUES:
        for opts in similar_shapes.OPTION_SETS:
            want = similar_ref.select_rows(part["counts"], part["pairs"], df, idf, ids, T, *opts)
            assert_rows_equal(nsbind.similar_select_host(part, df, idf, ids, T, *opts), want, (T, opts))
    # what the shapes are there for, read off the oracle
    sel = lambda name, T=25, **kw: similar_ref.select(part["counts"], part["pairs"], df, idf, docs[name], T, **kw)  # noqa: E731
    assert len(sel("n0")[0]) == 0 and len(sel("none")[0]) == 0 and len(sel("few", 32)[0]) == 7 and len(sel("few", 25)[0]) == 7
    t, w = sel("tf1_equal_df", 32)
    assert len(set(w.view(np.uint32).tolist())) == 1 and list(t) == sorted(t) and t[0] == 2000
    for name in ("ties_short", "ties_long"):
        for T in similar_shapes.T_VALUES:
            t, w = similar_ref.rank(part["counts"], part["pairs"], df, idf, docs[name])
            assert w[T - 1] == w[T] and t[T - 1] < t[T]                # the tie straddles the cut; the smaller termId is in
            assert list(sel(name, T)[0]) == list(t[:T])
    for name in ("last_lane_wave", "last_lane_block"):
        off = similar_ref.doc_offsets(part["counts"])
        assert sel(name, 1)[0][0] == part["pairs"][off[docs[name] + 1] - 1, 0] and int(part["counts"][docs[name]]) % 64 == 37
    assert len(sel("options", 32, min_tf=6)[0]) == 0 and len(sel("options", 32, min_tf=5)[0]) == 15
    assert len(sel("options", 32, min_df=10, max_df=10)[0]) == 20 and len(sel("options", 32, min_df=11, max_df=9)[0]) == 0
    assert len(sel("options", 32, min_tf=0)[0]) == len(sel("options", 32, min_tf=1)[0]) == 32


def test_refused_inputs_of_the_host_restatement(shapes):
    part, df, idf, docs = shapes
    with pytest.raises(ValueError):
        nsbind.similar_select_host(part, df, idf, [len(part["counts"])])
    with pytest.raises(ValueError):
        nsbind.similar_select_host(part, df[:10], idf[:10], [docs["n64"]])
    short = {"counts": part["counts"][:-1], "pairs": part["pairs"]}
    with pytest.raises(ValueError):
        nsbind.similar_select_host(short, df, idf, [0])
    t, w, c = nsbind.similar_select_host(part, df, idf, [])
    assert t.shape == (0, 25) and len(c) == 0


def test_clamps_defaults_and_boost_weights():
    assert nsbind.similar_defaults() == similar_ref.DEFAULTS
    for m in (0, 1, 2, 25, 31, 32, 33, 1 << 31, 0xFFFFFFFF):
        assert nsbind.similar_clamp_terms(m) == similar_ref.clamp_terms(m)
    for k in (-5, 0, 1, 10, 98, 99, 100, 101, 10**6):
        assert nsbind.similar_clamp_k(k) == similar_ref.clamp_k(k)
    H = nsbind.host_lib()
    rng = np.random.default_rng(9)
    w = np.sort((rng.random(200, dtype=np.float32) * np.float32(40.0) + np.float32(1e-3)))[::-1].copy()
    want = similar_ref.weights(w, True)
    got = np.asarray([H.nsh_similar_qweight(float(x), float(w[0]), 1) for x in w], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and got[0] == 1.0 and len(set(got.tolist())) > 100
    assert all(H.nsh_similar_qweight(float(x), float(w[0]), 0) == 1.0 for x in w)
    assert np.array_equal(similar_ref.weights(w, False), np.ones(len(w), dtype=np.float32)) and len(similar_ref.weights([], True)) == 0


def test_term_stats_and_failures_of_a_host_only_engine(tmp_path):
    batches, dup = three_batches()
    index = make_index(tmp_path, batches)
    eng = nsbind.Engine(index, -1)
    try:
        for s, docs in enumerate(batches):
            seg = os.path.join(index, "segments", "seg_%06u" % s)
            counts, pairs = invert_oracle.read_forward(os.path.join(seg, "forward.bin"))
            terms = invert_oracle.read_terms(os.path.join(seg, "terms.bin"))
            df, _ = invert_oracle.invert(counts, pairs, len(terms))
            got_df, got_idf = eng.similar_term_stats(s)
            assert np.array_equal(got_df, df) and len(df) == len(terms) > 50
            assert np.array_equal(got_idf.view(np.uint32), similar_shapes.idf_of(len(docs), df).view(np.uint32))
        with pytest.raises(RuntimeError, match="not in the index"):
            eng.similar_term_stats(3)
        # the uid-to-source rule: the first (manifest position, docId) that carries the uid
        assert eng.find_documents([dup])[0] == (0, 7)
        with pytest.raises(RuntimeError, match="no document with cord_uid"):
            eng.more_like_this_json(b"no such uid")
        with pytest.raises(RuntimeError, match="no device context"):
            eng.more_like_this_json(dup)
        with pytest.raises(RuntimeError, match="no device context"):
            eng.similar_batch([(1, 0)], 10)
        with pytest.raises(RuntimeError, match=r"\(segment 3, document 0\) is not in the index"):
            eng.similar_batch([(1, 0), (3, 0)], 10)
        with pytest.raises(RuntimeError, match=r"\(segment 2, document %d\) is not in the index" % len(batches[2])):
            eng.similar_batch([(2, len(batches[2]))], 10)
        assert eng.similar_segments_on_device() == 0
    finally:
        eng.close()


def test_a_generated_index_has_no_forward_files_and_the_message_names_the_segment(index_factory):
    index, _ = index_factory(2, 300, 2000)
    eng = nsbind.Engine(index, -1)
    try:
        assert eng.find_documents([b"u00000301"]) == [(1, 1)]
        names = [eng.segment_name(s) for s in range(2)]
        assert len(set(names)) == 2
        with pytest.raises(RuntimeError, match=r"segment %s carries no forward index.*%s.forward\.bin" % (names[1], names[1])):
            eng.more_like_this_json(b"u00000301")
        with pytest.raises(RuntimeError, match=r"segment %s carries no forward index" % names[0]):
            eng.similar_term_stats(0)
    finally:
        eng.close()
