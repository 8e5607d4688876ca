"""Spelling correction on the device (csrc/ns_fuzzy.hip): raw ns_ac_fuzzy on hand-made tables, the
generated index of the suggest fixtures (65 536 equal-length terms: hundreds of candidates within distance 2 of a query, ranked
by score), a table made so that the keep buffer must overflow, and did_you_mean end to end on an indexed word-like
dictionary.  Every answer is compared with the restatement of tests/correct_ref.py, exact in index, distance and count."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import correct_ref
import nsbind
import suggest_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "suggest")


def _ctx():
    h = C.c_void_p()
    assert nsbind.hip_lib().ns_ctx_create(0, C.byref(h)) == 0
    return h


def _check(tab, queries, edits, prefix_len, L, idx, dist, cnt):
    W = suggest_ref.clamp_limit(L)
    assert idx.shape == (len(queries), W) and dist.shape == (len(queries), W)
    for q, t in enumerate(queries):
        want = tab.fuzzy(t, int(edits[q]), prefix_len, W)
        got = [(int(idx[q, r]), int(dist[q, r])) for r in range(int(cnt[q]))]
        assert got == want, (t, int(edits[q]), prefix_len, L)
        assert all(v == 0xFFFFFFFF for v in idx[q, cnt[q]:]) and all(v == 0xFF for v in dist[q, cnt[q]:])


def _hand_made(n, rng):
    """n sorted terms: mostly one length (every slice boundary falls among ties), with repeated strings, terms past 8
    and past 66 bytes and bytes outside [0-9a-z] among them once the table is large enough"""
    extra = []
    if n >= 63:
        extra = [b"a00001", b"a00001", b"a00001", b"b1", b"", b"a", b"A-b_9", b"a0\xc3\xa9t\xc3\xa9", b"a000 1", b"b00002abcdefgh",
                 b"b00002abcdefhg", b"b00002abcdefghijklmnopqrstuvwxyz0123456789", b"a" * 63, b"a" * 64, b"a" * 65, b"a" * 66, b"a" * 67,
                 b"a" * 80, b"b" * 64 + b"c", b"b" * 64 + b"c", b"a0000", b"a000001"]
    base = set()
    while len(base) < n - len(extra):
        base.add(b"%c%05d" % (rng.choice(b"ab"), rng.randrange(100000 if n > 100 else 300)))
    return sorted(list(base) + extra)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_raw_fuzzy_on_hand_made_tables(n):
    ctx = _ctx()
    try:
        rng = random.Random(100 + n)
        terms = _hand_made(n, rng)
        assert len(terms) == n
        queries = [correct_ref.random_edits(rng, rng.choice(terms), rng.randint(0, 3), b"ab019-") for _ in range(120)] if n else []
        queries += [b"", b"a", b"b1", b"a00001", b"a0001", b"a" * 64, b"a" * 65, b"a" * 62 + b"ba", b"b" * 64, b"A-b9_", b"ca", b"abc",
                    b"a0\xc3\xa9t", b"b00002abcdefgh", b"b00002abdcefhg", b"b00002abcdefghijklmnopqrstuvwxyz0123456798", b"zzzzzzzz"]
        edits = np.array([rng.randrange(3) for _ in queries], dtype=np.uint8)   # 0 / 1 / 2 mixed in one batch
        for scores in ([7] * n, [rng.choice([0, 1, 2, 3, 3, 1 << 31, 0xFFFFFFFF]) for _ in range(n)]):
            tab = correct_ref.Table(terms, scores)
            ac = nsbind.AcTable(ctx, terms, scores)
            assert ac.rc == 0
            with pytest.raises(RuntimeError, match="rc=-5"):       # NS_E_STATE before ns_ac_build_fuzzy
                ac.fuzzy(queries, edits, 0, 5)
            assert ac.build_fuzzy()[0] == 0
            assert ac.build_fuzzy() == (0, 0.0)                    # idempotent
            for prefix_len in (0, 1, 3, 100):
                for L in (1, 5, 10, 11):
                    idx, dist, cnt, _ = ac.fuzzy(queries, edits, prefix_len, L)
                    _check(tab, queries, edits, prefix_len, L, idx, dist, cnt)
            with pytest.raises(RuntimeError, match="rc=-1"):       # max_edits 3: NS_E_INVAL
                ac.fuzzy(queries, [3] * len(queries), 0, 5)
            ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


def test_directed_distances():
    ctx = _ctx()
    try:
        terms = sorted([b"abc", b"ab", b"ba", b"abcdef", b"bacdef", b"abcdfe"])
        ac = nsbind.AcTable(ctx, terms, [1] * len(terms))
        assert ac.build_fuzzy()[0] == 0
        idx, dist, cnt, _ = ac.fuzzy([b"ca", b"ab", b"abcdef"], 2, 0, 10)
        got = [[(terms[int(idx[q, r])], int(dist[q, r])) for r in range(int(cnt[q]))] for q in range(3)]
        assert (b"abc", 2) not in got[0] and (b"abc", 3) not in got[0]            # d("ca", "abc") = 3: outside two edits
        assert got[0] == [(b"ba", 1), (b"ab", 2)]
        for q, t in enumerate([b"ca", b"ab", b"abcdef"]):
            assert got[q] == [(terms[i], d) for i, d in correct_ref.fuzzy_plain(terms, [1] * len(terms), t, 2, 0, 10)]
        assert got[1] == [(b"ab", 0), (b"abc", 1), (b"ba", 1)]                    # one transposition
        assert got[2] == [(b"abcdef", 0), (b"abcdfe", 1), (b"bacdef", 1)]         # transpositions at both ends
        ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


def test_keep_buffer_overflows_and_is_reduced():
    """Directed input for the reduction of a full keep buffer (128 keys per wave).  One query, so a slice is 1024
    consecutive slots and a wave verifies 256 of them, in slot order = index order (all terms have one length).  Every
    term is within two edits of the query and the scores ascend with the index, so each key beats all earlier ones and is
    kept: the third batch of 64 finds 128 keys in the buffer and must reduce it, and the answer is the LAST terms."""
    ctx = _ctx()
    try:
        abc = b"0123456789abcdefghijklmnopqrstuvwxyz"
        terms = sorted(b"aaaa" + bytes([x, y]) for x in abc for y in abc)      # 1296 terms, one length
        scores = list(range(1, len(terms) + 1))
        tab = correct_ref.Table(terms, scores)
        assert len(tab.within(b"aaaa--", 2, 0)[0]) == len(terms)              # all survive the DP (and the signature: 1 + 2 <= 4)
        ac = nsbind.AcTable(ctx, terms, scores)
        assert ac.build_fuzzy()[0] == 0
        for L in (1, 5, 10):
            idx, dist, cnt, _ = ac.fuzzy([b"aaaa--"], 2, 0, L)
            _check(tab, [b"aaaa--"], [2], 0, L, idx, dist, cnt)
            assert list(idx[0]) == list(range(len(terms) - 1, len(terms) - 1 - L, -1))
        # the same with the order of arrival reversed (descending scores: after the first reduction nothing beats the L-th)
        ac2 = nsbind.AcTable(ctx, terms, scores[::-1])
        assert ac2.build_fuzzy()[0] == 0
        idx, dist, cnt, _ = ac2.fuzzy([b"aaaa--", b"aaaazz", b"aaaa"], 2, 0, 10)
        _check(correct_ref.Table(terms, scores[::-1]), [b"aaaa--", b"aaaazz", b"aaaa"], [2, 2, 2], 0, 10, idx, dist, cnt)
        ac2.close()
        ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


@pytest.fixture(scope="module")
def barrel3(index_factory):
    with open(os.path.join(GOLDEN, "barrel3.json")) as f:
        p = json.load(f)["params"]
    return index_factory(p["n_segments"], p["docs_per_segment"], p["vocab"], p["seed"], p["legacy"])[0]


@pytest.fixture(scope="module")
def barrel3_queries(barrel3):
    eng = nsbind.Engine(barrel3, -1)
    terms, scores, _ = eng.suggest_table()
    eng.close()
    rng = random.Random(23)
    queries = [correct_ref.random_edits(rng, terms[rng.randrange(len(terms))], rng.randint(0, 3), b"t0123456789") for _ in range(1100)]
    return terms, [int(s) for s in scores], correct_ref.Table(terms, scores), queries


def test_generated_index_over_a_thousand_candidates_per_query(barrel3, barrel3_queries):
    terms, scores, tab, queries = barrel3_queries
    assert len(terms) >= 65536
    assert len(set(scores)) > 8                       # the ranking among equal distances is decided by the scores
    # The vocabulary is t000000 .. t065535, not every six-digit number, so two substituted digits do not give C(6,2) * 81
    # neighbours.  What holds for a query t0dxxxx with d <= 5: every change of one or two of its LAST FOUR digits names an
    # existing term (below 60 000): 1 + 4 * 9 + C(4,2) * 81 = 523 terms within two edits, far more than the L = 10 asked
    # for and than one keep buffer (128 keys): the best are decided by score among hundreds of equal distances.
    for t in (b"t012345", b"t031234"):
        n_within = len(tab.within(t, 2, 0)[0])
        print("candidates within two edits of", t, ":", n_within)
        assert n_within >= 523
    eng = nsbind.Engine(barrel3, 0)
    assert eng.correct_build_ms() == 0.0              # reload() did not build the corrector
    sent = queries + [b"t012345", b"t065535", b"t031234"]
    for prefix_len, L in ((0, 5), (1, 10)):
        idx, dist, cnt, _ = eng.correct_batch_raw(sent, L, -1, prefix_len)
        _check(tab, sent, [correct_ref.auto_edits(len(t)) for t in sent], prefix_len, L, idx, dist, cnt)
    assert eng.correct_build_ms() > 0.0
    # explicit edits, a longer prefix
    idx, dist, cnt, _ = eng.correct_batch_raw(sent[:200], 10, 1, 3)
    _check(tab, sent[:200], [1] * 200, 3, 10, idx, dist, cnt)
    with pytest.raises(RuntimeError, match="max_edits"):
        eng.correct_batch_raw(sent[:2], 5, 3, 0)
    eng.close()


def test_batch_sizes_and_a_second_identical_call(barrel3, barrel3_queries):
    terms, scores, tab, queries = barrel3_queries
    eng = nsbind.Engine(barrel3, 0)
    big = [queries[q % len(queries)] for q in range(16384)]
    for Q in (1, 63, 64, 65, 16384):
        idx, dist, cnt, _ = eng.correct_batch_raw(big[:Q], 5, -1, 0)
        _check(tab, big[:Q], [correct_ref.auto_edits(len(t)) for t in big[:Q]], 0, 5, idx, dist, cnt)
        again = eng.correct_batch_raw(big[:Q], 5, -1, 0)
        assert idx.tobytes() == again[0].tobytes() and dist.tobytes() == again[1].tobytes() and cnt.tobytes() == again[2].tobytes()
    # raw terms are normalised like the table's
    idx, dist, cnt, _ = eng.correct_batch_raw([b"T0-123 45!", b"", b"!!", b"x" * 65], 5, -1, 0)
    _check(tab, [b"t012345", b"", b"", b"x" * 65], [2, 0, 0, 2], 0, 5, idx, dist, cnt)
    eng.close()


def test_two_context_engine_answers_the_same(barrel3, barrel3_queries):
    queries = barrel3_queries[3][:300]
    one = nsbind.Engine(barrel3, 0)
    two = nsbind.Engine(barrel3, [0, 0])
    a, b = one.correct_batch_raw(queries, 10, -1, 0), two.correct_batch_raw(queries, 10, -1, 0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))
    for t in (b"t01234 covd vacine", b"Pandemc of t000100"):
        assert one.did_you_mean_json(t, 5) == two.did_you_mean_json(t, 5)
    two.close()
    one.close()


@pytest.mark.parametrize("name", ["tiny1", "barrel3"])
def test_suggest_answers_identically_before_and_after_the_build(name, barrel3, tmp_path):
    import base64
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        fx = json.load(f)
    if name == "barrel3":
        d = barrel3
    else:
        d = str(tmp_path / "index")
        suggest_ref.write_tiny_index(d, [[(base64.b64decode(t), df) for t, df in seg] for seg in fx["params"]["segments_b64"]])
    eng = nsbind.Engine(d, -1)
    terms, scores, _ = eng.suggest_table()
    eng.close()
    cases = [(base64.b64decode(c["input_b64"]), c["limit"], [base64.b64decode(s) for s in c["suggestions_b64"]]) for c in fx["cases"]]
    ctx = _ctx()
    try:
        ac = nsbind.AcTable(ctx, terms, scores)
        assert ac.rc == 0

        def answers():
            out = []
            for L in sorted({suggest_ref.clamp_limit(c[1]) for c in cases}):
                ins = [c for c in cases if suggest_ref.clamp_limit(c[1]) == L]
                idx, cnt, _ = ac.suggest([suggest_ref.split(c[0])[1] for c in ins], L)
                for c, row, k in zip(ins, idx, cnt):
                    base, prefix = suggest_ref.split(c[0])
                    if prefix:   # an empty prefix never reaches the device (the engine answers it with nothing)
                        assert [base + terms[int(i)] for i in row[:k]] == c[2], c[0]
                out.append((idx.tobytes(), cnt.tobytes()))
            return out

        before = answers()
        assert ac.build_fuzzy()[0] == 0
        assert answers() == before
        ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


# ---- a word-like dictionary, end to end --------------------------------------------------------------------------------

_SYL = [b"ka", b"to", b"mi", b"ren", b"sol", b"va", b"qu", b"el", b"dor", b"bi", b"nu", b"sha", b"pe", b"lim", b"ox", b"ra", b"zen", b"fu", b"gi", b"9", b"2x"]


def _pseudo_words(rng, n):
    out = set()
    while len(out) < n:
        w = b"".join(rng.choice(_SYL) for _ in range(rng.randint(1, 6)))
        if 3 <= len(w) <= 14 and w not in correct_ref.STOPWORDS:
            out.add(w)
    return sorted(out)


def _lexicon_terms(index_dir):
    known = set()
    for name in suggest_ref.read_manifest(index_dir):
        known.update(t for t, df in suggest_ref.read_lexicons(os.path.join(index_dir, "segments", name)).items() if df)   # the term dictionary skips df 0
    return known


def test_did_you_mean_on_an_indexed_word_like_dictionary(tmp_path):
    rng = random.Random(77)
    words = _pseudo_words(rng, 3000)
    docs = []
    for i in range(240):   # Zipf-like use: the early words appear in many documents, so scores differ
        body = b" ".join(words[min(int(rng.paretovariate(0.6)) - 1 + rng.randrange(40), len(words) - 1)] for _ in range(150))
        body += b" " + b" ".join(words[(i * 13 + j) % len(words)] for j in range(13))
        docs.append((b"uid%04d" % i, b"title %d" % i, b"doc/%d.json" % i, body))
    d = str(tmp_path / "index")
    os.makedirs(d)
    eng = nsbind.Engine.create(d, 0)
    eng.add_documents(docs)

    def restate():
        terms, scores, _ = eng.suggest_table()
        return correct_ref.Table(terms, [int(s) for s in scores]), _lexicon_terms(d)

    tab, known = restate()
    assert len(tab.terms) > 2500
    queries = []
    for _ in range(150):
        toks = []
        for _ in range(rng.randint(1, 4)):
            w = rng.choice(tab.terms)
            r = rng.random()
            toks.append(w if r < 0.3 else correct_ref.random_edits(rng, w, rng.randint(1, 3), b"aeioknrst"))
        queries.append(b" ".join(toks))
    queries += [b"", b"   ", b"the of and", b"a b c 7", b"The " + tab.terms[5].upper() + b", x!",          # stop words, one-byte tokens
                b"qqqqqqqqqqzzzzzzzz " + tab.terms[9],                                                  # a token with no candidate
                b"  (" + correct_ref.random_edits(rng, tab.terms[40], 1, b"e").upper() + b")--" + correct_ref.random_edits(rng, tab.terms[41], 1, b"e") + b"?!  ",
                b"Caf\xc3\xa9 " + correct_ref.random_edits(rng, tab.terms[100], 1, b"o") + b"\xc3\xa9" + tab.terms[7] + b"\t\"quoted\\\" \x01",
                b"x" * 70 + b" " + tab.terms[3][:-1]]
    n_changed = n_unchanged = 0
    for q in queries:
        for limit in (1, 5):
            got = eng.did_you_mean_json(q, limit)
            assert got == correct_ref.did_you_mean(tab, known, q, limit), (q, limit)
        doc = json.loads(got.decode("latin-1"))
        n_changed += doc["changed"]
        n_unchanged += not doc["changed"]
    assert n_changed > 50 and n_unchanged > 5
    doc = json.loads(eng.did_you_mean_json(b"The " + tab.terms[5].upper() + b", x!", 5))
    assert doc["changed"] is False and doc["corrected"] == "The " + tab.terms[5].upper().decode() + ", x!"
    assert [t["token"] for t in doc["terms"]] == [tab.terms[5].decode()] and doc["terms"][0]["known"] is True
    # correct_batch on the same table, every edit bound and a prefix
    terms_in = [correct_ref.random_edits(rng, rng.choice(tab.terms), rng.randint(0, 3), b"aeioknrst") for _ in range(400)]
    for e in (0, 1, 2):
        idx, dist, cnt, _ = eng.correct_batch_raw(terms_in, 10, e, 2)
        _check(tab, terms_in, [e] * len(terms_in), 2, 10, idx, dist, cnt)
    # a term that arrives with add_documents is a candidate afterwards (the corrector is rebuilt lazily after the reload)
    new = b"zyxwvutsr"
    assert new not in tab.terms
    before = json.loads(eng.did_you_mean_json(b"zyxwvutr", 5))
    assert before["changed"] is False and before["terms"][0]["suggestions"] == []
    eng.add_documents([(b"uidnew", b"t", b"doc/new.json", new + b" " + tab.terms[0])])
    assert eng.correct_build_ms() == 0.0
    tab2, known2 = restate()
    assert new in tab2.terms
    got = eng.did_you_mean_json(b"zyxwvutr", 5)
    assert got == correct_ref.did_you_mean(tab2, known2, b"zyxwvutr", 5)
    assert json.loads(got)["corrected"] == new.decode() and eng.correct_build_ms() > 0.0
    eng.close()
