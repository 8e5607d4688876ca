"""Related terms on the device (csrc/ns_terms.hip behind ns_docterms_aggregate, Engine::terms_batch, Engine::related_terms;
DESIGN.md §5aa).  The oracles are tests/related_ref.py (the rule and the engine's merge in numpy) and nsh_related_aggregate_host (the
rule on one host thread).  Integers, bytes and fp32 bit patterns: every comparison is exact."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nsbind
import related_ref
import related_shapes as shapes
from related_shapes import assert_rows_equal
from test_compact_gpu import new_engine
from test_similar_gpu import index_oracle, three_segment_corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_LIB = os.path.join(ROOT, "nextsearch-api_amd", "libnextsearch_hip_count.so")
CHILD_TIMEOUT_S = 120
NS_E_INVAL, NS_E_STATE = -1, -5


# ---- 1: the raw ABI against both oracles, array for array ----------------------------------------------------------------
@pytest.fixture(scope="module")
def raw():
    L = nsbind.hip_lib()
    W, cut = int(L.ns_docterms_window()), int(L.ns_docterms_doc_cut())
    assert W in (1 << 15, 1 << 16) and L.ns_docterms_max_row_docs() == 255
    part, df, idf, docs, rows, n_terms = shapes.directed(W, cut)
    ctx = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(ctx)) == 0
    dt = nsbind.DocTerms(ctx, part, df, idf)
    yield {"L": L, "ctx": ctx, "dt": dt, "part": part, "df": df, "idf": idf, "docs": docs, "rows": rows, "W": W}
    dt.close()
    L.ns_ctx_destroy(ctx)


def both(raw, rows, T, o=shapes.OPTION_SETS[0]):
    """the restatement's answer, after checking that the host rule gives the same"""
    want = related_ref.aggregate_rows(raw["part"]["counts"], raw["part"]["pairs"], raw["df"], raw["idf"], rows, T, *o)
    assert_rows_equal(nsbind.related_aggregate_host(raw["part"], raw["df"], raw["idf"], rows, T, *o), want, ("host", T, o))
    return want


@pytest.mark.parametrize("T", shapes.T_VALUES)
def test_every_shape_alone_and_in_one_mixed_batch(raw, T):
    batch = list(raw["rows"].values())
    want = both(raw, batch, T)
    got = raw["dt"].aggregate(batch, T)
    assert_rows_equal(got[:5], want, ("batch", T))
    assert got[5] > 0.0                                                  # the kernel's time
    for i, (name, r) in enumerate(raw["rows"].items()):                  # n_rows = 1: every row alone
        assert_rows_equal(raw["dt"].aggregate([r], T)[:5], tuple(a[i:i + 1] for a in want), (name, T))
    assert int(want[3].max()) == T and int(want[3].min()) == 0


@pytest.mark.parametrize("o", shapes.OPTION_SETS[1:])
def test_min_tf_min_docs_min_df_max_df_at_and_next_to_the_values_present(raw, o):
    batch = list(raw["rows"].values())
    assert_rows_equal(raw["dt"].aggregate(batch, 64, *o)[:5], both(raw, batch, 64, o), o)


def test_max_terms_is_clamped_and_an_empty_batch_is_ok(raw):
    rows = [raw["rows"]["ties"], raw["rows"]["mixed"]]
    for m, T in ((0, 1), (65, 64), (1000, 64), (0xFFFFFFFF, 64)):
        got = raw["dt"].aggregate(rows, m)
        assert got[0].shape == (2, T)
        assert_rows_equal(got[:5], both(raw, rows, T), m)
    L, ms = raw["L"], C.c_float(7.0)
    assert L.ns_docterms_aggregate(raw["dt"].h, None, None, 0, 10, 1, 2, 1, 0xFFFFFFFF, None, None, None, None, None, C.byref(ms)) == 0 and ms.value == 0.0


def test_a_random_batch(raw):
    rng = np.random.default_rng(5)
    n_docs = 2000
    vocab = 3 * raw["W"] // 2 + 11
    hot = rng.choice(vocab, 400, replace=False)                           # shared vocabulary: terms do repeat across documents
    counts, chunks = [], []
    for d in range(n_docs):
        n = int(rng.integers(0, 120))
        t = np.unique(np.concatenate([rng.choice(hot, n // 2), rng.choice(vocab, n - n // 2)]))
        counts.append(len(t))
        chunks.append(np.stack([t, rng.integers(1, 4, len(t))], axis=1))
    part = {"counts": np.asarray(counts, np.uint32), "pairs": np.concatenate(chunks).astype(np.uint32)}
    df = rng.integers(0, 3000, vocab).astype(np.uint32)
    idf = shapes.idf_of(shapes.N_DOCS_FOR_IDF, df)
    rows = [rng.integers(0, n_docs, int(rng.integers(0, 256))).tolist() for _ in range(300)]
    assert max(len(set(r)) for r in rows) > 200 and any(len(set(r)) < len(r) for r in rows)
    dt = nsbind.DocTerms(raw["ctx"], part, df, idf)
    try:
        for T, o in ((10, (1, 2, 1, 0xFFFFFFFF)), (64, (2, 3, 5, 2500))):
            want = related_ref.aggregate_rows(part["counts"], part["pairs"], df, idf, rows, T, *o)
            assert_rows_equal(nsbind.related_aggregate_host(part, df, idf, rows, T, *o), want, ("host", T))
            assert_rows_equal(dt.aggregate(rows, T, *o)[:5], want, ("device", T))
            assert int(want[3].sum()) > 100 * T // 2
    finally:
        dt.close()


def test_refusals_their_messages_and_handle_lifetime(raw):
    L, ctx, dt, docs = raw["L"], raw["ctx"], raw["dt"], raw["docs"]
    n_docs = len(raw["part"]["counts"])
    for rows, match in (([[1], docs["full"] + [docs["extra"]]], "row 1 names 256 distinct documents; a row holds at most 255"),
                        ([[0, n_docs, 1]], r"doc_ids\[1\] = %d \(row 0\), the handle holds %d documents" % (n_docs, n_docs))):
        with pytest.raises(RuntimeError, match=match) as ei:
            dt.aggregate(rows)
        assert ei.value.args[1] == NS_E_INVAL
    # row_off that does not start at 0, or descends; NULL arguments; the outputs untouched
    ids = np.asarray([0, 1, 2], np.uint32)
    out = [np.full(20, 7, np.uint32) for _ in range(5)]
    args = lambda h, i, o, n, outs: (h, i, o, n, 10, 1, 2, 1, 0xFFFFFFFF) + tuple(a.ctypes.data if a is not None else None for a in outs) + (None,)  # noqa: E731
    for off, match in (([1, 2, 3], b"row_off[0] = 1, not 0"), ([0, 3, 2], b"row_off[2] = 2 is below row_off[1] = 3")):
        off = np.asarray(off, np.uint64)
        assert L.ns_docterms_aggregate(*args(dt.h, ids.ctypes.data, off.ctypes.data, 2, out)) == NS_E_INVAL and match in L.ns_last_error(ctx)
    off = np.asarray([0, 2, 3], np.uint64)
    assert L.ns_docterms_aggregate(*args(None, ids.ctypes.data, off.ctypes.data, 2, out)) == NS_E_INVAL
    assert L.ns_docterms_aggregate(*args(dt.h, None, off.ctypes.data, 2, out)) == NS_E_INVAL
    assert L.ns_docterms_aggregate(*args(dt.h, ids.ctypes.data, None, 2, out)) == NS_E_INVAL
    for k in range(5):
        assert L.ns_docterms_aggregate(*args(dt.h, ids.ctypes.data, off.ctypes.data, 2, out[:k] + [None] + out[k + 1:])) == NS_E_INVAL
        assert b"null argument" in L.ns_last_error(ctx)
    assert all((a == 7).all() for a in out)
    # 300 ids with 255 distinct documents are one row of 255
    t, g, w, c, n, _ = dt.aggregate([docs["full"] + docs["full"][:45]])
    assert n[0] == 255 and g[0, 0] == 255
    # a source with one descending pair of ids: select answers, the aggregate refuses the handle, every time
    part, df, idf = shapes.descending_source()
    bad = nsbind.DocTerms(ctx, part, df, idf)
    assert bad.select([1], 25)[2][0] == 3
    for _ in range(2):
        with pytest.raises(RuntimeError, match="strictly ascending order") as ei:
            bad.aggregate([[0, 2]])
        assert ei.value.args[1] == NS_E_INVAL
    assert bad.select([1], 25)[2][0] == 3
    bad.close()
    # an empty source and a source of empty documents are valid
    for counts in ([], [0, 0, 0]):
        e = nsbind.DocTerms(ctx, {"counts": np.asarray(counts, np.uint32), "pairs": np.zeros((0, 2), np.uint32)}, df[:0], idf[:0])
        t, g, w, c, n, _ = e.aggregate([[2, 0, 2]] if counts else [[]], 64)
        assert (t == 0xFFFFFFFF).all() and (g == 0).all() and (w.view(np.uint32) == 0).all() and c[0] == 0 and n[0] == (2 if counts else 0)
        e.close()
    # the ctx goes first: the handle is orphaned, answers NS_E_STATE and is freed without the ctx
    ctx2 = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(ctx2)) == 0
    part, df, idf = raw["part"], raw["df"], raw["idf"]
    a = nsbind.DocTerms(ctx2, part, df, idf)
    assert a.aggregate([raw["rows"]["ties"]], 64)[3][0] == 64
    L.ns_ctx_destroy(ctx2)
    with pytest.raises(RuntimeError, match="ctx has been destroyed") as ei:
        a.aggregate([raw["rows"]["ties"]])
    assert ei.value.args[1] == NS_E_STATE
    a.close()
    assert_rows_equal(dt.aggregate([raw["rows"]["skip"]], 10)[:5], both(raw, [raw["rows"]["skip"]], 10), "the module's handle still answers")


def test_the_counting_build_reaches_every_path(tmp_path):
    """a child process on libnextsearch_hip_count.so runs the directed shapes (tests/related_shapes.py main): every counter moves, and
    the windows skipped are the number the restatement derives"""
    assert os.path.exists(COUNT_LIB), "libnextsearch_hip_count.so is missing: make -C nextsearch-api_amd all"
    out = str(tmp_path / "related.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "related_shapes.py"), out], env=dict(os.environ, NS_HIP_LIB=COUNT_LIB), capture_output=True,
                       text=True, timeout=CHILD_TIMEOUT_S)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and "related shapes OK" in r.stdout, tail
    with open(out) as f:
        rep = json.load(f)
    assert rep["counting"] and rep["refused"] == 1
    cnt = dict(zip(shapes.COUNTER_NAMES, rep["counters"]))
    assert all(v > 0 for v in cnt.values()), cnt
    assert cnt["windows skipped"] == rep["want_skipped"] > 0 and cnt["rows refused"] == 1 and cnt["rows"] == rep["rows"], (cnt, rep)


# ---- 2: the engine -------------------------------------------------------------------------------------------------------
def merge_oracle(eng, index):
    orc = index_oracle(eng, index)
    lex = {}
    for o in orc:
        for t, d in zip(o["terms"], o["df"].tolist()):
            lex[t] = lex.get(t, 0) + d
    H = nsbind.host_lib()
    return orc, sum(len(o["counts"]) for o in orc), lambda N, d: H.nsh_bm25_idf(int(N), int(d)), lambda t: lex.get(t, 0)


def assert_terms_batch(eng, index, rows, what, **opt):
    orc, N, idf_of, lex_df = merge_oracle(eng, index)
    want, want_n = related_ref.merge(orc, N, idf_of, lex_df, rows, opt)
    got, got_n, ms = eng.terms_batch(rows, **opt)
    To = related_ref.clamp_out(opt.get("max_terms", 10))
    assert got_n.tolist() == want_n, what
    total = 0
    for q, (g, w) in enumerate(zip(got, want)):
        w = w[:To]
        assert [(t, d, f) for t, d, f, _ in g] == [(t, d, f) for t, d, f, _ in w], (what, q)
        assert [np.float32(x).view(np.uint32) for _, _, _, x in g] == [np.float32(x).view(np.uint32) for _, _, _, x in w], (what, q, "w bits")
        total += len(g)
    return total, want


@pytest.fixture(scope="module")
def served(tmp_path_factory):
    index = str(tmp_path_factory.mktemp("related") / "index")
    batches = three_segment_corpus()
    eng = new_engine(index, batches)
    assert eng.num_segments == 3
    yield {"eng": eng, "index": index, "batches": batches}
    eng.close()


def a_query(eng, index):
    """two words of middling df from the index's own dictionary"""
    o = index_oracle(eng, index)[0]
    mid = [t for t, d in zip(o["terms"], o["df"].tolist()) if 25 <= d <= 60]
    return (mid[3] + b" " + mid[11]).decode()


def test_terms_batch_over_three_segments_equals_the_merge_rule(served):
    eng, index, batches = served["eng"], served["index"], served["batches"]
    rng = np.random.default_rng(8)
    rows = []
    for n in (0, 1, 2, 7, 40, 100, 100, 250, 30, 30):
        rows.append([(s, int(rng.integers(0, len(batches[s])))) for s in rng.integers(0, 3, n).tolist()])
    rows.append([(1, int(d)) for d in rng.choice(len(batches[1]), 255, replace=False)])          # one segment's part at the cap
    rows.append(rows[4] + rows[4])                                                              # repeats count once
    total, _ = assert_terms_batch(eng, index, rows, "defaults")
    assert total > 60
    assert assert_terms_batch(eng, index, rows, "options", max_terms=32, min_tf=1, min_docs=3, min_df=4, max_df=200)[0] > 100
    assert assert_terms_batch(eng, index, rows[:6], "clamped", max_terms=1000)[0] > 60
    assert eng.terms_batch([])[0] == []
    with pytest.raises(RuntimeError, match=r"\(segment 3, document 0\) is not in the index"):
        eng.terms_batch([[(0, 0), (3, 0)]])
    with pytest.raises(RuntimeError, match="256 distinct documents"):
        eng.terms_batch([[(2, d) for d in range(256)]])


def expected_related(eng, index, query, **opt):
    o = dict(related_ref.DEFAULTS, **opt)
    K = max(1, min(o["sample"], 100))
    h, n, f, u = eng.search_batch([query], K)
    row = [(int(x["seg"]), int(x["doc"])) for x in h[0, :int(n[0])]]
    orc, N, idf_of, lex_df = merge_oracle(eng, index)
    want, _ = related_ref.merge(orc, N, idf_of, lex_df, [row], opt)
    own = [t.encode() for t in nsbind.base_terms(query)]
    keep = [c for c in want[0] if c[0] not in own][:related_ref.clamp_out(o["max_terms"])]
    return keep, len(row), int(f[0]), own


def test_related_terms_json_and_that_search_answers_as_before(served):
    eng, index = served["eng"], served["index"]
    query = a_query(eng, index)
    uid = served["batches"][1][100][0]
    eng.set_cache(False)                                                 # (a cached body says "from_cache")
    before = (eng.search_json(query, 10), eng.more_like_this_json(uid, 10))
    body = eng.related_terms_json(query).decode()
    js = json.loads(body)
    keep, sample, found, own = expected_related(eng, index, query)
    assert list(js) == ["found", "query", "sample", "segments", "terms"] and js["query"] == query and js["segments"] == 3
    assert js["found"] == found and js["sample"] == sample > 20 and len(js["terms"]) == 10 == len(keep)
    assert [(t["term"].encode(), t["docs"], t["df"]) for t in js["terms"]] == [(t, d, f) for t, d, f, _ in keep]
    assert [np.float32(t["weight"]).view(np.uint32) for t in js["terms"]] == [np.float32(w).view(np.uint32) for _, _, _, w in keep]
    assert not {t["term"].encode() for t in js["terms"]} & set(own) and len(own) == 2
    assert all(list(t) == ["df", "docs", "term", "weight"] and t["docs"] >= 2 for t in js["terms"])
    # the query's own words would have been among the first: they are dropped before the cut, not after
    orc, N, idf_of, lex_df = merge_oracle(eng, index)
    h, n, _, _ = eng.search_batch([query], 100)
    uncut = related_ref.merge(orc, N, idf_of, lex_df, [[(int(x["seg"]), int(x["doc"])) for x in h[0, :int(n[0])]]], {})[0][0]
    assert set(own) & {c[0] for c in uncut[:12]}
    js32 = json.loads(eng.related_terms_json(query, max_terms=1000, sample=30, min_docs=3).decode())
    keep32, sample32, _, _ = expected_related(eng, index, query, max_terms=1000, sample=30, min_docs=3)
    assert js32["sample"] == sample32 == 30 and [(t["term"].encode(), t["docs"]) for t in js32["terms"]] == [(t, d) for t, d, _, _ in keep32] and 10 < len(keep32) <= 32
    # no hits: an empty list, not an error; under a filter the sample is the filtered search's
    none = json.loads(eng.related_terms_json("zzzzqqqq").decode())
    assert none["terms"] == [] and none["sample"] == 0 and none["found"] == 0
    fl = json.loads(eng.related_terms_json(query, date_filter=("1900", "2100", True)).decode())
    assert fl["terms"] == js["terms"] and fl["sample"] == js["sample"]
    assert (eng.search_json(query, 10), eng.more_like_this_json(uid, 10)) == before
    eng.set_cache(True)


def test_after_compact_the_one_segment_answer_is_the_exact_aggregate(tmp_path):
    batches = three_segment_corpus()
    index = str(tmp_path / "index")
    eng = new_engine(index, [b[:150] for b in batches])
    try:
        rng = np.random.default_rng(9)
        eng.terms_batch([[(0, 1), (1, 2), (2, 3)]])
        assert eng.similar_segments_on_device() == 3
        eng.compact()
        assert eng.num_segments == 1 and eng.similar_segments_on_device() == 0
        o = index_oracle(eng, index)[0]
        rows = [rng.integers(0, 450, n).tolist() for n in (0, 1, 5, 60, 100, 255)]
        for opt in ({}, {"max_terms": 32, "min_tf": 2, "min_docs": 3, "min_df": 3, "max_df": 150}):
            oo = dict(related_ref.DEFAULTS, **opt)
            got, ndocs, _ = eng.terms_batch([[(0, d) for d in r] for r in rows], **opt)
            for q, r in enumerate(rows):                               # exact: EVERY qualifying term ranked from the forward files, then cut
                t, g, w, nd = related_ref.rank(o["counts"], o["pairs"], o["df"], o["idf"], r, oo["min_tf"], oo["min_docs"], oo["min_df"], oo["max_df"])
                m = min(len(t), related_ref.clamp_out(oo["max_terms"]))
                assert ndocs[q] == nd and [x[0] for x in got[q]] == [o["terms"][int(i)] for i in t[:m]], (opt, q)
                assert [x[1] for x in got[q]] == g[:m].tolist() and [x[2] for x in got[q]] == o["df"][t[:m]].tolist(), (opt, q)
                assert [np.float32(x[3]).view(np.uint32) for x in got[q]] == w[:m].view(np.uint32).tolist(), (opt, q)
            assert all(len(x) > 0 for x in got[3:]) and len(got[0]) == 0          # the larger rows do name terms; an empty row names none
    finally:
        eng.close()
