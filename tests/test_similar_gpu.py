"""More like this on the device (csrc/ns_similar.hip behind ns_docterms_upload / ns_docterms_select, Engine::similar_batch,
Engine::more_like_this).  The oracle is tests/similar_ref.py for the selection and the engine's own text
search for the scoring: similar_batch without boost must equal, row for row, search_batch with K + 1 over the selected terms
joined by spaces, minus the source.  Integers, bytes and fp32 bit patterns: every comparison is exact."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import ingest_ref
import nsbind
import similar_ref
import similar_shapes
from similar_shapes import assert_rows_equal
from test_compact_gpu import new_engine
from test_ingest_gpu import as_docs, gen_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import invert_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
NS_E_INVAL, NS_E_STATE = -1, -5


# ---- 1: the raw ABI against the oracle, array for array ------------------------------------------------
@pytest.fixture(scope="module")
def raw():
    L = nsbind.hip_lib()
    cut = int(L.ns_docterms_doc_cut())
    assert 129 < cut < 100_000
    part, df, idf, docs = similar_shapes.directed(cut)
    ctx = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(ctx)) == 0
    dt = nsbind.DocTerms(ctx, part, df, idf)
    yield {"L": L, "ctx": ctx, "dt": dt, "part": part, "df": df, "idf": idf, "docs": docs, "cut": cut}
    dt.close()
    L.ns_ctx_destroy(ctx)


def want_rows(raw, ids, T, opts=(1, 1, 0xFFFFFFFF)):
    return similar_ref.select_rows(raw["part"]["counts"], raw["part"]["pairs"], raw["df"], raw["idf"], ids, T, *opts)


@pytest.mark.parametrize("T", similar_shapes.T_VALUES)
def test_every_shape_alone_and_in_one_mixed_batch(raw, T):
    docs, counts = raw["docs"], raw["part"]["counts"]
    sizes = sorted(int(counts[d]) for d in docs.values())
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, raw["cut"] - 1, raw["cut"], raw["cut"] + 1, 100_003):
        assert n in sizes
    mixed = np.asarray(list(docs.values()) + [docs["cut_plus_1"], docs["n1"], docs["cut_plus_1"]], dtype=np.uint32)   # one document three times
    want = want_rows(raw, mixed, T)
    got = raw["dt"].select(mixed, T)
    assert_rows_equal(got[:3], want, ("mixed", T))
    assert got[3] > 0.0                                                  # the kernels' time
    for i, d in enumerate(mixed):                                        # n = 1: every document alone
        one = raw["dt"].select([d], T)[:3]
        assert_rows_equal(one, tuple(a[i:i + 1] for a in want), ("alone", T, int(d)))
    cnt = {name: int(want[2][i]) for i, name in enumerate(docs)}
    assert cnt["n0"] == 0 and cnt["none"] == 0 and cnt["few"] == min(T, 7) and cnt["n100003"] == T


@pytest.mark.parametrize("opts", similar_shapes.OPTION_SETS[1:])
def test_min_tf_min_df_max_df_at_and_next_to_the_values_present(raw, opts):
    ids = np.asarray(sorted(raw["docs"].values()), dtype=np.uint32)
    for T in (25, 32):
        assert_rows_equal(raw["dt"].select(ids, T, *opts)[:3], want_rows(raw, ids, T, opts), (T, opts))


def test_max_terms_is_clamped_and_an_empty_batch_is_ok(raw):
    ids = [raw["docs"]["n129"], raw["docs"]["cut"]]
    for m, T in ((0, 1), (33, 32), (0xFFFFFFFF, 32)):
        got = raw["dt"].select(ids, m)
        assert got[0].shape == (2, T)
        assert_rows_equal(got[:3], want_rows(raw, ids, T), m)
    L, ms = raw["L"], C.c_float(7.0)
    assert L.ns_docterms_select(raw["dt"].h, None, 0, 25, 1, 1, 0xFFFFFFFF, None, None, None, C.byref(ms)) == 0 and ms.value == 0.0


def test_refusals_and_handle_lifetime(raw):
    L, ctx, part, df, idf = raw["L"], raw["ctx"], raw["part"], raw["df"], raw["idf"]
    n_docs = len(part["counts"])
    # a doc id out of range: refused on the host, the outputs untouched
    ids = np.asarray([0, n_docs, 1], dtype=np.uint32)
    term, w, cnt = np.full((3, 25), 7, np.uint32), np.full((3, 25), 7, np.float32), np.full(3, 7, np.uint32)
    rc = L.ns_docterms_select(raw["dt"].h, ids.ctypes.data, 3, 25, 1, 1, 0xFFFFFFFF, term.ctypes.data, w.ctypes.data, cnt.ctypes.data, None)
    assert rc == NS_E_INVAL and b"doc_ids[1]" in L.ns_last_error(ctx)
    assert (term == 7).all() and (w == 7).all() and (cnt == 7).all()
    assert L.ns_docterms_select(None, ids.ctypes.data, 1, 25, 1, 1, 0xFFFFFFFF, term.ctypes.data, w.ctypes.data, cnt.ctypes.data, None) == NS_E_INVAL
    assert L.ns_docterms_select(raw["dt"].h, None, 1, 25, 1, 1, 0xFFFFFFFF, term.ctypes.data, w.ctypes.data, cnt.ctypes.data, None) == NS_E_INVAL
    # a termId out of range is found at upload time, by the kernel's flag word
    small = {"counts": np.asarray([3, 0, 2], np.uint32), "pairs": np.asarray([[0, 1], [4, 2], [2, 1], [1, 1], [3, 9]], np.uint32)}
    ok = nsbind.docterms_upload(ctx, small, df[:5], idf[:5])
    one_shot = nsbind.docterms_select(ctx, small, df[:5], idf[:5], [2, 1, 0])
    assert_rows_equal(ok.select([2, 1, 0])[:3], one_shot[:3], "upload + select + destroy in one helper")
    assert_rows_equal(one_shot[:3], similar_ref.select_rows(small["counts"], small["pairs"], df[:5], idf[:5], [2, 1, 0], 25), "small")
    ok.close()
    with pytest.raises(RuntimeError, match="termId >= n_terms = 4") as ei:
        nsbind.DocTerms(ctx, small, df[:4], idf[:4])
    assert ei.value.args[1] == NS_E_INVAL
    with pytest.raises(RuntimeError, match="termId >= n_terms = 0"):
        nsbind.DocTerms(ctx, small, df[:0], idf[:0])
    # counts that do not sum to n_pairs, in both directions
    for n_pairs in (4, 6):
        with pytest.raises(RuntimeError, match="do not sum to n_pairs") as ei:
            nsbind.DocTerms(ctx, small, df[:5], idf[:5], n_pairs=n_pairs)
        assert ei.value.args[1] == NS_E_INVAL
    h = C.c_void_p()
    assert L.ns_docterms_upload(ctx, None, None, None, C.byref(h)) == NS_E_INVAL and L.ns_docterms_upload(None, None, None, None, C.byref(h)) == NS_E_INVAL
    # an empty source and a source of empty documents are valid
    for counts in ([], [0, 0, 0]):
        e = nsbind.DocTerms(ctx, {"counts": np.asarray(counts, np.uint32), "pairs": np.zeros((0, 2), np.uint32)}, df[:0], idf[:0])
        if counts:
            t, w_, c, _ = e.select([2, 0], 32)
            assert (t == 0xFFFFFFFF).all() and (w_.view(np.uint32) == 0).all() and (c == 0).all()
        e.close()
    # the ctx goes first: the handle is orphaned, answers NS_E_STATE and is freed without the ctx
    ctx2 = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(ctx2)) == 0
    a, b = nsbind.DocTerms(ctx2, small, df[:5], idf[:5]), nsbind.DocTerms(ctx2, small, df[:5], idf[:5])
    assert a.select([0], 25)[2][0] == int((df[[0, 4, 2]] > 0).sum())
    b.close()                                                            # one released before its ctx, one after
    L.ns_ctx_destroy(ctx2)
    with pytest.raises(RuntimeError, match="ctx has been destroyed") as ei:
        a.select([0], 25)
    assert ei.value.args[1] == NS_E_STATE
    a.close()
    L.ns_docterms_destroy(None)
    assert_rows_equal(raw["dt"].select([2], 25)[:3], want_rows(raw, [2], 25), "the module's handle still answers")


# ---- 2: end to end ------------------------------------------------------------------------------------------
def segment_oracle(index, name):
    """counts, pairs, terms, df, idf of one segment directory, from its files alone"""
    seg = os.path.join(index, "segments", name)
    counts, pairs = invert_oracle.read_forward(os.path.join(seg, "forward.bin"))
    terms = invert_oracle.read_terms(os.path.join(seg, "terms.bin"))
    df, _ = invert_oracle.invert(counts, pairs, len(terms))
    return {"counts": counts, "pairs": pairs, "terms": terms, "df": df, "idf": similar_shapes.idf_of(len(counts), df)}


def index_oracle(eng, index):
    return [segment_oracle(index, eng.segment_name(s)) for s in range(eng.num_segments)]


def oracle_terms(orc, seg, doc, opt=None):
    o = orc[seg]
    opt = opt or {}
    t, w = similar_ref.select(o["counts"], o["pairs"], o["df"], o["idf"], doc, opt.get("max_terms", 25), opt.get("min_tf", 1),
                              opt.get("min_df", 1), opt.get("max_df", 0xFFFFFFFF))
    return [o["terms"][int(i)] for i in t], w


def drop_source(hits, nhits, found, sources, K):
    """the stated rule over rows of K + 1: the source's own hit goes if it is there, otherwise the last hit"""
    out, n_out = np.zeros((len(sources), K), dtype=nsbind.HIT_DTYPE), np.zeros(len(sources), dtype=np.uint32)
    among = 0
    for q, (s, d) in enumerate(sources):
        row = [h for h in hits[q, :int(nhits[q])] if not (int(h["seg"]) == s and int(h["doc"]) == d)]
        among += len(row) < int(nhits[q])
        row = row[:K]
        n_out[q] = len(row)
        for i, h in enumerate(row):
            out[q, i] = h
    return out, n_out, found - 1, among


def assert_rows(got, want, what):
    (gh, gn, gf), (wh, wn, wf) = got, want
    assert np.array_equal(gn, wn) and np.array_equal(gf, wf), what
    live = np.arange(gh.shape[1])[None, :] < gn[:, None]
    for f in ("doc", "seg"):
        assert np.array_equal(gh[f][live], wh[f][live]), (what, f)
    assert np.array_equal(gh["score"].view(np.uint32)[live], wh["score"].view(np.uint32)[live]), (what, "score bits")
    assert (gh["doc"][~live] == 0xFFFFFFFF).all() and (gh["seg"][~live] == 0xFFFFFFFF).all() and np.isneginf(gh["score"][~live]).all(), (what, "padding")
    return int(live.sum())


def assert_similar_equals_text_search(eng, index, sources, k, what, opt=None):
    """similar_batch without boost == search_batch(K + 1) over the oracle's terms joined by spaces, minus the source"""
    K = similar_ref.clamp_k(k)
    orc = index_oracle(eng, index)
    sel = [oracle_terms(orc, s, d, opt) for s, d in sources]
    queries = [b" ".join(t).decode() for t, _ in sel]
    some = np.asarray([bool(q) for q in queries])                      # an empty selection: not usable, no hits, no found
    th, tn, tf, tu = eng.search_batch(queries, K + 1)
    assert np.array_equal(tu.astype(bool), some)
    wh, wn, wf, among = drop_source(th, tn, np.where(some, tf, 1), sources, K)
    gh, gn, gf, gu, gterms = eng.similar_batch(sources, k, terms=True, **(opt or {}))
    assert np.array_equal(gu.astype(bool), some)
    live = assert_rows((gh, gn, gf), (wh, wn, wf), what)
    for q, (t, w) in enumerate(sel):
        assert [x for x, _ in gterms[q]] == t, (what, q)
        assert np.array_equal(np.asarray([y for _, y in gterms[q]], np.float32).view(np.uint32), w.view(np.uint32)), (what, q)
    return live, among, sel


def three_segment_corpus():
    texts = [t for t in gen_corpus(501, 900, 60, vocab=2500, long_tokens=()) if ingest_ref.kept_tokens(t)]
    docs = as_docs(texts)
    return [docs[:250], docs[250:600], docs[600:]]


@pytest.fixture(scope="module")
def served(tmp_path_factory):
    index = str(tmp_path_factory.mktemp("similar") / "index")
    batches = three_segment_corpus()
    eng = new_engine(index, batches)
    assert eng.num_segments == 3
    rng = np.random.default_rng(3)
    sources = [(s, int(d)) for s, b in enumerate(batches) for d in rng.choice(len(b), 67, replace=False)]
    yield {"eng": eng, "index": index, "batches": batches, "sources": sources}
    eng.close()


def test_similar_batch_equals_the_text_search_over_the_selected_terms(served):
    eng, sources = served["eng"], served["sources"]
    assert len(sources) == 201
    live, among, _ = assert_similar_equals_text_search(eng, served["index"], sources, 10, "k10")
    assert live > 1500 and among > 150                                   # the rows are full and the source usually sits in them
    assert_similar_equals_text_search(eng, served["index"], sources[::9], 1000, "k clamps to 99")
    live, _, sel = assert_similar_equals_text_search(eng, served["index"], sources[::7], 5, "options", {"max_terms": 7, "min_tf": 1, "min_df": 2, "max_df": 40})
    assert live > 100 and max(len(t) for t, _ in sel) == 7
    _, _, sel = assert_similar_equals_text_search(eng, served["index"], sources[::2], 5, "min_tf 2", {"max_terms": 32, "min_tf": 2})
    assert 0 < sum(len(t) for t, _ in sel) < 25 * len(sel)               # min_tf does cut the selections
    # every document of the index, twice: enough sources for the term lookup to be cut over several host threads
    every = [(s, d) for s, b in enumerate(served["batches"]) for d in range(len(b))] * 2
    assert len(every) > 1536
    assert assert_similar_equals_text_search(eng, served["index"], every, 3, "every document")[0] > 4000
    # a selection nothing qualifies for: usable 0, no hits, no found
    h, n, f, u = eng.similar_batch(sources[:3], 10, min_df=10**6)
    assert not u.any() and not n.any() and not f.any() and (h["doc"] == 0xFFFFFFFF).all()
    with pytest.raises(RuntimeError, match=r"\(segment 3, document 0\) is not in the index"):
        eng.similar_batch([sources[0], (3, 0)], 10)
    assert eng.similar_batch([], 10)[0].shape == (0, 10)


def test_boost_equals_the_raw_abi_over_refs_the_test_builds(served):
    eng, sources = served["eng"], served["sources"][::3]
    K = 10
    orc = index_oracle(eng, served["index"])
    memo = {}

    def lookup(seg, term):
        if (seg, term) not in memo:
            memo[(seg, term)] = eng.lookup(seg, term.decode())
        return memo[(seg, term)]

    qd, refs = np.zeros(len(sources), dtype=nsbind.QDESC_DTYPE), []
    for q, (s, d) in enumerate(sources):
        terms, w = oracle_terms(orc, s, d)
        qw = similar_ref.weights(w, True)
        assert qw[0] == 1.0 and (qw[1:] <= 1.0).all() and (qw < 1.0).any()
        qd[q]["term_begin"] = len(refs)
        for seg in range(eng.num_segments):                              # every segment, selection order: the fp32 accumulation order
            for t, x in zip(terms, qw):
                e = lookup(seg, t)
                if e is not None and e["df"]:
                    refs.append((seg, e["count"], e["byte_off"], e["idf"], x))
        qd[q]["term_count"] = len(refs) - int(qd[q]["term_begin"])
    rc, th, tn, tf = nsbind.search_batch_raw(eng.ctx, qd, np.asarray(refs, dtype=nsbind.TERM_DTYPE), K + 1)
    assert rc == 0
    wh, wn, wf, among = drop_source(th, tn, tf, sources, K)
    gh, gn, gf, gu = eng.similar_batch(sources, K, boost=True)
    assert gu.all() and assert_rows((gh, gn, gf), (wh, wn, wf), "boost") > 500
    ph = eng.similar_batch(sources, K)[0]
    assert not np.array_equal(ph["score"].view(np.uint32), gh["score"].view(np.uint32))   # boost does change the scores


def test_a_source_that_is_not_among_the_k_plus_1_best(tmp_path):
    K = 10
    rare = [b"rare%03d" % i for i in range(40)]
    common = [b"common%03d" % i for i in range(360)]
    texts = [b" ".join(rare + common)]                                   # the source: very long, tf = 1 everywhere
    texts += [b" ".join(rare * 3) + b" short%d" % j for j in range(K + 3)]   # hold its selected terms with tf = 3
    texts += [b" ".join(common) + b" filler%d" % j for j in range(30)]   # make the other 360 words frequent
    eng = new_engine(str(tmp_path / "index"), [as_docs(texts)])
    try:
        live, among, sel = assert_similar_equals_text_search(eng, str(tmp_path / "index"), [(0, 0)], K, "absent source")
        assert among == 0 and live == K and sel[0][0] == rare[:25]
        h, n, f, u = eng.similar_batch([(0, 0)], K)
        assert int(n[0]) == K and int(f[0]) == K + 3 and 0 not in h["doc"][0].tolist()
        th, tn, _, _ = eng.search_batch([b" ".join(rare[:25]).decode()], K + 1)
        assert int(tn[0]) == K + 1 and np.array_equal(th["doc"][0, :K], h["doc"][0])      # the last hit is dropped, nothing else changes
    finally:
        eng.close()


# ---- 3: lifetime, and the JSON ------------------------------------------------------------------------------
def expected_json(eng, orc, uid, k):
    """the body assembled from search's own result entries (hits_to_json) and the oracle's query_terms"""
    K = similar_ref.clamp_k(k)
    s, d = eng.find_documents([uid])[0]
    terms, w = oracle_terms(orc, s, d)
    h, n, f, u = eng.similar_batch([(s, d)], k)
    body = eng.hits_to_json("", K, True, int(f[0]), h[0, :int(n[0])])
    results = body[body.index('  "results": ['):body.index('  "segments": ')]
    qt = ",\n".join('    {\n      "term": %s,\n      "weight": %s\n    }' % (json.dumps(t.decode()), repr(float(x))) for t, x in zip(terms, w))
    return ('{\n  "found": %d,\n  "k": %d,\n  "query_terms": [\n%s\n  ],\n%s  "segments": %d,\n  "source": {\n    "cord_uid": %s,\n'
            '    "docId": %d,\n    "segment": %s\n  }\n}') % (int(f[0]), K, qt, results, eng.num_segments, json.dumps(uid.decode()), d,
                                                                 json.dumps(eng.segment_name(s)))


def test_more_like_this_json_delete_compact_and_lazy_device_copies(tmp_path):
    batches = three_segment_corpus()
    index = str(tmp_path / "index")
    eng = new_engine(index, batches)
    try:
        # reload() alone builds no device copy; a call builds the ones it names; release_similar and reload free them
        eng.reload()
        assert eng.similar_segments_on_device() == 0
        eng.similar_batch([(1, 5)], 10)
        assert eng.similar_segments_on_device() == 1
        eng.similar_batch([(0, 5), (2, 5), (1, 6)], 10)
        assert eng.similar_segments_on_device() == 3
        eng.release_similar()
        assert eng.similar_segments_on_device() == 0
        eng.similar_batch([(2, 1)], 10)
        eng.reload()
        assert eng.similar_segments_on_device() == 0
        # the JSON body
        uid = batches[1][100][0]
        assert eng.find_documents([uid]) == [(1, 100)]
        body = eng.more_like_this_json(uid, 10).decode()
        assert body == expected_json(eng, index_oracle(eng, index), uid, 10)
        js = json.loads(body)
        assert list(js) == ["found", "k", "query_terms", "results", "segments", "source"] and js["k"] == 10 and len(js["results"]) == 10
        assert len(js["query_terms"]) == 25 and js["source"] == {"cord_uid": uid.decode(), "docId": 100, "segment": eng.segment_name(1)}
        assert uid.decode() not in [r["cord_uid"] for r in js["results"]]
        assert json.loads(eng.more_like_this_json(uid, 1000).decode())["k"] == 99
        with pytest.raises(RuntimeError, match="no document with cord_uid"):
            eng.more_like_this_json(b"nobody")
        # delete three of the results and a document in front of the source: the uid answers from the new index
        victims = [r["cord_uid"].encode() for r in js["results"][:3]] + [batches[1][3][0]]
        new_doc = 100 - sum(1 for s, d in set(eng.find_documents(victims)) if s == 1 and d < 100)
        assert new_doc < 100
        eng.delete_documents(victims)
        assert eng.similar_segments_on_device() == 0
        assert eng.find_documents([uid]) == [(1, new_doc)]
        body2 = eng.more_like_this_json(uid, 10).decode()
        assert body2 == expected_json(eng, index_oracle(eng, index), uid, 10)
        js2 = json.loads(body2)
        assert js2["source"]["docId"] == new_doc and not {v.decode() for v in victims} & {r["cord_uid"] for r in js2["results"]}
        sources = [(s, d) for s in range(3) for d in range(0, 200, 13)]
        assert_similar_equals_text_search(eng, index, sources, 10, "after the delete")
        # after compact the one segment's df is the index's
        eng.compact()
        assert eng.num_segments == 1 and eng.similar_segments_on_device() == 0
        assert eng.find_documents([uid])[0][0] == 0
        body3 = eng.more_like_this_json(uid, 10).decode()
        assert body3 == expected_json(eng, index_oracle(eng, index), uid, 10)
        merged = [(0, d) for d in range(0, 800, 11)]
        assert_similar_equals_text_search(eng, index, merged, 10, "after compact")
        assert json.loads(body3)["query_terms"] != js2["query_terms"]    # the merged segment's df weighs the words differently
    finally:
        eng.close()


def test_ns_tool_similar_prints_the_same_body(tmp_path):
    import subprocess
    batches = three_segment_corpus()
    index = str(tmp_path / "index")
    eng = new_engine(index, [batches[0][:120]])
    try:
        uid = batches[0][17][0]
        want = eng.more_like_this_json(uid, 5).decode()
    finally:
        eng.close()
    tool = os.path.join(ROOT, "nextsearch-api_amd", "ns_tool")
    out = subprocess.run([tool, "similar", index, uid.decode(), "5"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout == want + "\n"
    bad = subprocess.run([tool, "similar", index, "nobody"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "no document with cord_uid" in bad.stderr
