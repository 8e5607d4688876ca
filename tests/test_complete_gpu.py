"""Typo-tolerant completion on the device (csrc/ns_fuzzy.hip k_fp_*): raw ns_ac_fuzzy_prefix on hand-made
tables, directed prefix distances (both band edges, the bytes past a term's end, candidates past 66 and past 255 bytes,
queries no longer than the edit bound), its equality with ns_ac_suggest at 0 edits, the generated index of the suggest
fixtures, the neighbours' answers before and after, and Engine.complete end to end on an indexed word-like dictionary.
Every answer is compared with the restatement of tests/complete_ref.py, exact in index, distance and count."""
import base64
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import complete_ref
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
        want = tab.complete(t, int(edits[q]), prefix_len, W)
        got = [(int(idx[q, r]), int(dist[q, r])) for r in range(int(cnt[q]))]
        assert got == want, (t, int(edits[q]), prefix_len, L)
        assert all(v == 0xFFFFFFFF for v in idx[q, cnt[q]:]) and all(v == 0xFF for v in dist[q, cnt[q]:])


def _on_the_signature_bound(tab, queries, edits, prefix_len):
    """the (query, answer) pairs with e >= 1 whose popcount(sig_q & ~sig_c) is exactly e: a filter with a tighter bound
    would lose these answers"""
    out = []
    for t, e in zip(queries, edits):
        if e >= 1:
            out += [(t, i) for i, _ in tab.complete(t, int(e), prefix_len, 10) if complete_ref.sig_missing(t, tab.terms[i]) == e]
    return out


def _hand_made(n, rng):
    """n sorted terms: mostly one length (every slice boundary falls among ties), with repeated strings, terms past 8,
    past 66 and past 255 bytes and bytes outside [0-9a-z] among them once the table is large enough"""
    extra = []
    if n >= 63:
        extra = [b"a00001", b"a00001", b"a00001", b"b1", b"", b"a", b"A-b_9", b"a0\xc3\xa9t\xc3\xa9", b"a000 1", b"b00002abcdefgh",
                 b"b00002abcdefhg", b"b00002abcdefghijklmnopqrstuvwxyz0123456789", b"a" * 63, b"a" * 64, b"a" * 65, b"a" * 66, b"a" * 67,
                 b"a" * 80, b"a" * 300, b"b" * 64 + b"c", b"b" * 64 + b"c", b"b" * 70 + b"xyz", b"a0000", b"a000001"]
    base = set()
    while len(base) < n - len(extra):
        base.add(b"%c%05d" % (rng.choice(b"ab"), rng.randrange(100000 if n > 100 else 300)))
    return sorted(list(base) + extra)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_raw_fuzzy_prefix_on_hand_made_tables(n):
    ctx = _ctx()
    try:
        rng = random.Random(200 + n)
        terms = _hand_made(n, rng)
        assert len(terms) == n
        queries = []
        for _ in range(100 if n else 0):
            w = rng.choice(terms)
            queries.append(correct_ref.random_edits(rng, w[:rng.randint(1, max(1, min(len(w), 64)))], rng.randint(0, 3), b"ab019-"))
        queries += [b"", b"a", b"b", b"b1", b"a0", b"a00001", b"a0001", b"a" * 64, b"a" * 65, b"a" * 62 + b"ba", b"b" * 64, b"b" * 62 + b"cb",
                    b"A-b9_", b"ca", b"abc", b"a0\xc3\xa9t", b"b00002abcdefgh", b"b00002abdcefhg", b"b00002abcdefghijklmnopqrstuvwxyz0123456798",
                    b"zzzzzzzz", b"zz", b"-"]
        edits = [rng.randrange(3) for _ in queries]                                   # 0 / 1 / 2 mixed in one batch
        # answers on the bound of the signature filter: one and two bytes of the query that the answer has no byte class for
        queries += [b"a0x", b"a0xy0", b"b0-z", b"a000x1"]
        edits += [1, 2, 2, 1]
        edits = np.array(edits, dtype=np.uint8)
        for scores in ([7] * n, [rng.choice([0, 1, 2, 3, 3, 1 << 31, 0xFFFFFFFF]) for _ in range(n)]):
            tab = complete_ref.Table(terms, scores)
            ac = nsbind.AcTable(ctx, terms, scores)
            assert ac.rc == 0
            with pytest.raises(RuntimeError, match="rc=-5"):       # NS_E_STATE before ns_ac_build_fuzzy
                ac.fuzzy_prefix(queries, edits, 0, 5)
            assert ac.build_fuzzy()[0] == 0
            for prefix_len in (0, 1, 3, 100):
                for L in (1, 5, 10, 11):
                    idx, dist, cnt, _ = ac.fuzzy_prefix(queries, edits, prefix_len, L)
                    _check(tab, queries, edits, prefix_len, L, idx, dist, cnt)
            with pytest.raises(RuntimeError, match="rc=-1"):       # max_edits 3: NS_E_INVAL
                ac.fuzzy_prefix(queries, [3] * len(queries), 0, 5)
            if n >= 63 and scores[0] == 7:   # (equal scores: every distinct string is a candidate)
                bound = _on_the_signature_bound(tab, queries, edits, 0)
                assert {e for e in (1, 2) if any(complete_ref.sig_missing(t, terms[i]) == e for t, i in bound)} == {1, 2}
            if n == 4097 and scores[0] == 7:   # more candidates than one 1024-slot slice, and the best are ties that straddle the slices
                assert len(tab.within(b"a0", 0, 0)[0]) > 100 and len(tab.within(b"zz", 2, 0)[0]) > 3000
            ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


# (q, c, prefix distance): DESIGN.md §5m's table
HAND = [(b"ca", b"abc", 1), (b"abcd", b"axxbcdzz", 2), (b"abxxcd", b"abcd", 2), (b"abdc", b"abcdef", 1), (b"ab", b"bazz", 1), (b"abcd", b"ab", 2),
        (b"abcd", b"abc", 1), (b"a", b"zzzz", 1), (b"virsu", b"viruses", 1), (b"cornoa", b"coronavirus", 1), (b"abcd", b"abcd" + b"x" * 300, 0),
        (b"abcde", b"cdxxx", 3)]


def test_directed_distances():
    """each hand-computed pair, alone in its table (so the answer is that pair's and nothing else's) and in the table of
    all the candidates; (abcd, axxbcdzz) ends at column n + 2 and (abxxcd, abcd) at n - 2, each the only cut within two edits"""
    ctx = _ctx()
    try:
        for q, c, d in HAND:
            assert complete_ref.pd(q, c) == d
            ac = nsbind.AcTable(ctx, [c], [1])
            assert ac.build_fuzzy()[0] == 0
            idx, dist, cnt, _ = ac.fuzzy_prefix([q, q, q], [0, 1, 2], 0, 10)
            for e in (0, 1, 2):
                got = [(int(idx[e, r]), int(dist[e, r])) for r in range(int(cnt[e]))]
                assert got == ([(0, d)] if d <= e else []), (q, c, e)
            ac.close()
        for q, c, j in ((b"abcd", b"axxbcdzz", 6), (b"abxxcd", b"abcd", 4)):
            assert [k for k in range(len(c) + 1) if correct_ref.osa(q, c[:k]) <= 2] == [j] and abs(j - len(q)) == 2
        terms = sorted({c for _, c, _ in HAND})
        scores = [9 if t == b"zzzz" else 1 for t in terms]
        tab = complete_ref.Table(terms, scores)
        ac = nsbind.AcTable(ctx, terms, scores)
        assert ac.build_fuzzy()[0] == 0
        qs = sorted({q for q, _, _ in HAND})
        for e in (0, 1, 2):
            for prefix_len in (0, 1):
                idx, dist, cnt, _ = ac.fuzzy_prefix(qs, e, prefix_len, 10)
                _check(tab, qs, [e] * len(qs), prefix_len, 10, idx, dist, cnt)
                for q, c, d in HAND:
                    got = [(terms[int(i)], int(x)) for i, x in zip(idx[qs.index(q)], dist[qs.index(q)]) if i != 0xFFFFFFFF]
                    assert ((c, d) in got) == (d <= e and (prefix_len == 0 or c[:1] == q[:1])), (q, c, e, prefix_len)
        ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


def test_bytes_past_the_end_of_a_term_are_not_matched():
    """In the pool "ab" is followed by "cd": a DP that reads on past the term would see "abcd" and report distance 0."""
    ctx = _ctx()
    try:
        terms = [b"ab", b"cd"]
        ac = nsbind.AcTable(ctx, terms, [1, 1])
        assert ac.build_fuzzy()[0] == 0
        idx, dist, cnt, _ = ac.fuzzy_prefix([b"abcd", b"abcd", b"abcd"], [2, 1, 0], 0, 10)
        assert [(int(idx[0, r]), int(dist[0, r])) for r in range(int(cnt[0]))] == [(0, 2), (1, 2)]
        assert list(cnt) == [2, 0, 0]
        ac.close()
        # the same past 8 bytes, where a term's bytes come from the pool and no longer from its packed head
        terms = [b"0123456789ab", b"cdef"]
        ac = nsbind.AcTable(ctx, terms, [1, 1])
        assert ac.build_fuzzy()[0] == 0
        tab = complete_ref.Table(terms, [1, 1])
        qs = [b"0123456789abcd", b"0123456789abcdef", b"0123456789abc", b"0123456789ab"]
        for e in (0, 1, 2):
            idx, dist, cnt, _ = ac.fuzzy_prefix(qs, e, 0, 10)
            _check(tab, qs, [e] * len(qs), 0, 10, idx, dist, cnt)
        assert tab.complete(qs[0], 2, 0, 10) == [(0, 2)] and tab.complete(qs[1], 2, 0, 10) == [] and tab.complete(qs[2], 1, 0, 10) == [(0, 1)]
        ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


def test_candidates_past_66_and_past_255_bytes_are_found():
    ctx = _ctx()
    try:
        rng = random.Random(31)
        stems = [b"alpha7", b"bravo", b"charlie42", b"delta", b"echo9x"]
        longs = [(s * 60)[:m] for s, m in zip(stems, (67, 70, 80, 128, 300))]
        assert [len(t) for t in longs] == [67, 70, 80, 128, 300]
        # shorter neighbours with a signature, which the filter does test
        terms = sorted(longs + [t[:k] for t in longs for k in (3, 10, 66)] + [b"alpha", b"alphq7alpha7", b"bravq"])
        scores = [rng.randint(1, 5) for _ in terms]
        tab = complete_ref.Table(terms, scores)
        ac = nsbind.AcTable(ctx, terms, scores)
        assert ac.build_fuzzy()[0] == 0
        queries, edits = [], []
        for t in longs:
            for k in (4, 9, 33, 63, 64):
                for e in (0, 1, 2):
                    queries.append(t[:1] + correct_ref.random_edits(rng, t[1:k], e, b"xyz-"))   # the first byte stays: prefix_len 1
                    edits.append(e)
        queries += [b"alphx7a", b"brxyo", b"alpha7alph-7"]          # answers on the signature bound
        edits += [1, 2, 1]
        keep = [k for k, q in enumerate(queries) if len(q) <= 64]
        queries, edits = [queries[k] for k in keep], [edits[k] for k in keep]
        for prefix_len in (0, 1):
            for L in (10, 3):
                idx, dist, cnt, _ = ac.fuzzy_prefix(queries, edits, prefix_len, L)
                _check(tab, queries, edits, prefix_len, L, idx, dist, cnt)
            idx, dist, cnt, _ = ac.fuzzy_prefix(queries, edits, prefix_len, 10)
            made = [t for t in longs for _ in range(15)]              # found: the term each query was made from
            for r, row in enumerate(keep):
                if row < len(made):
                    assert terms.index(made[row]) in [int(i) for i in idx[r, :int(cnt[r])]], (queries[r], edits[r], prefix_len)
        bound = _on_the_signature_bound(tab, queries, edits, 0)
        assert any(len(terms[i]) <= 66 for _, i in bound)
        ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


def test_queries_no_longer_than_the_edit_bound_get_the_best_by_score():
    """§5l's table of 1296 equal-length terms.  A query of one or two bytes with two edits matches every candidate (the
    whole query can be deleted).  With ascending scores each key beats all earlier ones, so a wave's 128-key keep buffer
    fills and is reduced; the answer is the table's best L by score: the LAST terms."""
    ctx = _ctx()
    try:
        abc = b"0123456789abcdefghijklmnopqrstuvwxyz"
        terms = sorted(b"aaaa" + bytes([x, y]) for x in abc for y in abc)
        n = len(terms)
        for scores, best in ((list(range(1, n + 1)), list(range(n - 1, -1, -1))), (list(range(n, 0, -1)), list(range(n)))):
            tab = complete_ref.Table(terms, scores)
            ac = nsbind.AcTable(ctx, terms, scores)
            assert ac.build_fuzzy()[0] == 0
            qs = [b"z", b"zz", b"a", b"aa", b"za", b"-"]
            for L in (1, 5, 10):
                idx, dist, cnt, _ = ac.fuzzy_prefix(qs, 2, 0, L)
                _check(tab, qs, [2] * len(qs), 0, L, idx, dist, cnt)
                for q, t in enumerate(qs):
                    assert list(idx[q]) == best[:L] and int(cnt[q]) == L
                assert list(dist[0]) == [1] * L and list(dist[1]) == [2] * L and list(dist[2]) == [0] * L and list(dist[3]) == [0] * L
            ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


def test_zero_edits_is_ns_ac_suggest():
    ctx = _ctx()
    try:
        rng = random.Random(41)
        terms = sorted({bytes(rng.choice(b"abc01") for _ in range(rng.randint(2, 12))) for _ in range(3000)} | {b"ab" * 40, b"abc" * 100})
        scores = [rng.randint(1, 50) for _ in terms]                 # no score 0, no repeated string: every entry is a candidate
        ac = nsbind.AcTable(ctx, terms, scores)
        assert ac.build_fuzzy()[0] == 0
        prefixes = [rng.choice(terms)[:rng.randint(1, 6)] for _ in range(300)] + [b"a", b"zz", b"ab" * 32, b"abc" * 21, b"abcabcabd", terms[0], terms[-1]]
        for L in (1, 5, 10):
            want_idx, want_cnt, _ = ac.suggest(prefixes, L)
            for prefix_len in (0, 1, 100):
                idx, dist, cnt, _ = ac.fuzzy_prefix(prefixes, 0, prefix_len, L)
                assert idx.tobytes() == want_idx.tobytes() and cnt.tobytes() == want_cnt.tobytes()
                assert all(int(d) == 0 for q in range(len(prefixes)) for d in dist[q, :int(cnt[q])])
        assert int(want_cnt.max()) == 10 and int(want_cnt.min()) == 0
        ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


@pytest.fixture(scope="module")
def barrel3(index_factory):
    with open(os.path.join(GOLDEN, "barrel3.json")) as f:
        p = json.load(f)["params"]
    return index_factory(p["n_segments"], p["docs_per_segment"], p["vocab"], p["seed"], p["legacy"])[0]


@pytest.fixture(scope="module")
def barrel3_prefixes(barrel3):
    eng = nsbind.Engine(barrel3, -1)
    terms, scores, _ = eng.suggest_table()
    eng.close()
    rng = random.Random(29)
    prefixes = []
    for _ in range(1100):   # true terms cut after 3..7 bytes, with 0..2 random edits
        w = terms[rng.randrange(len(terms))]
        prefixes.append(correct_ref.random_edits(rng, w[:rng.randint(3, 7)], rng.randint(0, 2), b"t0123456789"))
    return terms, [int(s) for s in scores], complete_ref.Table(terms, scores), prefixes


def test_generated_index(barrel3, barrel3_prefixes):
    terms, scores, tab, prefixes = barrel3_prefixes
    assert len(terms) >= 65536
    eng = nsbind.Engine(barrel3, 0)
    assert eng.correct_build_ms() == 0.0              # reload() did not build the side structures
    auto = [correct_ref.auto_edits(len(t)) for t in prefixes]
    for prefix_len, L in ((1, 5), (0, 10)):
        idx, dist, cnt, base, _ = eng.complete_batch_raw(prefixes, L, -1, prefix_len)
        _check(tab, prefixes, auto, prefix_len, L, idx, dist, cnt)
        assert not base.any()
    assert eng.correct_build_ms() > 0.0
    n_many = sum(len(tab.within(t, e, 0)[0]) > 1024 for t, e in zip(prefixes[:100], auto[:100]))
    print("of the first 100 prefixes,", n_many, "have more than 1024 candidates within their bound")
    assert n_many >= 10                               # the best 10 are chosen among thousands, by score
    # explicit edits, a longer fixed prefix
    idx, dist, cnt, _, _ = eng.complete_batch_raw(prefixes[:200], 10, 1, 3)
    _check(tab, prefixes[:200], [1] * 200, 3, 10, idx, dist, cnt)
    with pytest.raises(RuntimeError, match="max_edits"):
        eng.complete_batch_raw(prefixes[:2], 5, 3, 0)
    eng.close()


def test_batch_sizes_and_a_second_identical_call(barrel3, barrel3_prefixes):
    terms, scores, tab, prefixes = barrel3_prefixes
    eng = nsbind.Engine(barrel3, 0)
    big = [prefixes[q % len(prefixes)] for q in range(16384)]
    for Q in (1, 63, 64, 65, 16384):
        idx, dist, cnt, base, _ = eng.complete_batch_raw(big[:Q], 5, -1, 1)
        _check(tab, big[:Q], [correct_ref.auto_edits(len(t)) for t in big[:Q]], 1, 5, idx, dist, cnt)
        again = eng.complete_batch_raw(big[:Q], 5, -1, 1)
        assert idx.tobytes() == again[0].tobytes() and dist.tobytes() == again[1].tobytes() and cnt.tobytes() == again[2].tobytes()
    # raw inputs are split and normalised like suggest's
    ins = [b"see T0-123", b"", b"!!", b"x" * 65, b"covid T012?! "]
    idx, dist, cnt, base, _ = eng.complete_batch_raw(ins, 5, -1, 1)
    assert list(base) == [7, 0, 0, 0, 6]                # the bytes before the last alnum run; no run: 0
    _check(tab, [b"123", b"", b"", b"x" * 65, b"t012"], [1, 0, 0, 2, 1], 1, 5, idx, dist, cnt)
    eng.close()


def test_neighbours_answer_identically_before_and_after(barrel3, barrel3_prefixes):
    terms, scores, tab, prefixes = barrel3_prefixes
    with open(os.path.join(GOLDEN, "barrel3.json")) as f:
        fx = json.load(f)
    cases = [(base64.b64decode(c["input_b64"]), c["limit"], [base64.b64decode(s) for s in c["suggestions_b64"]]) for c in fx["cases"]]
    ctx = _ctx()
    try:
        ac = nsbind.AcTable(ctx, terms, scores)
        assert ac.rc == 0 and ac.build_fuzzy()[0] == 0
        rng = random.Random(3)
        hand = _hand_made(4097, rng)
        hand_scores = [rng.choice([0, 1, 2, 3]) for _ in hand]
        ac2 = nsbind.AcTable(ctx, hand, hand_scores)
        assert ac2.build_fuzzy()[0] == 0
        words = [correct_ref.random_edits(rng, rng.choice(hand), rng.randint(0, 3), b"ab019-") for _ in range(100)]
        ctab = correct_ref.Table(hand, hand_scores)

        def neighbours():
            out = []
            for L in sorted({suggest_ref.clamp_limit(c[1]) for c in cases}):
                ins = [c for c in cases if suggest_ref.clamp_limit(c[1]) == L]
                idx, cnt, _ = ac.suggest([suggest_ref.split(c[0])[1] for c in ins], L)
                for c, row, k in zip(ins, idx, cnt):
                    base, prefix = suggest_ref.split(c[0])
                    if prefix:
                        assert [base + terms[int(i)] for i in row[:k]] == c[2], c[0]
                out.append((idx.tobytes(), cnt.tobytes()))
            idx, dist, cnt, _ = ac2.fuzzy(words, 2, 0, 10)
            for q, t in enumerate(words):
                assert [(int(idx[q, r]), int(dist[q, r])) for r in range(int(cnt[q]))] == ctab.fuzzy(t, 2, 0, 10)
            out.append((idx.tobytes(), dist.tobytes(), cnt.tobytes()))
            return out

        before = neighbours()
        for prefix_len in (0, 1):
            ac.fuzzy_prefix(prefixes[:64], 1, prefix_len, 10)
            ac2.fuzzy_prefix(words, 2, prefix_len, 10)
        assert neighbours() == before
        ac2.close()
        ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


# ---- a word-like dictionary, end to end --------------------------------------------------------------------------------

_SYL = [b"ka", b"to", b"mi", b"ren", b"sol", b"va", b"qu", b"el", b"dor", b"bi", b"nu", b"sha", b"pe", b"lim", b"ox", b"ra", b"zen", b"fu", b"gi", b"9", b"2x"]


def _pseudo_words(rng, n):
    out = {b"covid", b"vaccine", b"vaccination", b"coronavirus"}
    while len(out) < n:
        w = b"".join(rng.choice(_SYL) for _ in range(rng.randint(1, 6)))
        if 3 <= len(w) <= 14 and w not in correct_ref.STOPWORDS:
            out.add(w)
    return sorted(out)


def test_complete_on_an_indexed_word_like_dictionary(tmp_path):
    rng = random.Random(78)
    words = _pseudo_words(rng, 1500)
    docs = []
    for i in range(120):   # Zipf-like use: the early words appear in many documents, so scores differ
        body = b" ".join(words[min(int(rng.paretovariate(0.6)) - 1 + rng.randrange(40), len(words) - 1)] for _ in range(150))
        body += b" " + b" ".join(words[(i * 13 + j) % len(words)] for j in range(13))
        docs.append((b"uid%04d" % i, b"title %d" % i, b"doc/%d.json" % i, body))
    d = str(tmp_path / "index")
    os.makedirs(d)
    eng = nsbind.Engine.create(d, 0)
    eng.add_documents(docs)

    def restate():
        terms, scores, _ = eng.suggest_table()
        return complete_ref.Table(terms, [int(s) for s in scores])

    tab = restate()
    assert len(tab.terms) > 1200
    inputs = []
    for _ in range(120):
        w = rng.choice(tab.terms)
        typed = correct_ref.random_edits(rng, w[:rng.randint(1, len(w))], rng.randint(0, 2), b"aeioknrst")
        inputs.append(b" ".join([rng.choice(tab.terms) for _ in range(rng.randint(0, 2))] + [typed]))
    inputs += [b"", b"   ", b"covid vacc", b"covid vacc?! ", b"Covid VACC", b"cornoav", b"the cornoav...", b"caf\xc3\xa9 vacicn", b"x" * 70,
               b"\"quoted\\\" \x01 vaccni", b"qqqqqqqqzzzz", b"co", b"c"]
    n_some = n_fuzzy = 0
    for s in inputs:
        for limit in (1, 5):
            got = eng.complete_json(s, limit)
            assert got == complete_ref.complete_json(tab, s, limit), (s, limit)
        doc = json.loads(got.decode("latin-1"))
        n_some += bool(doc["suggestions"])
        n_fuzzy += any(x["distance"] > 0 for x in doc["suggestions"])
    assert n_some > 60 and n_fuzzy > 30
    doc = json.loads(eng.complete_json(b"covid vacc?! ", 5))
    assert [x["suggestion"] for x in doc["suggestions"]][:2] == ["covid vaccination", "covid vaccine"] or \
        {x["suggestion"] for x in doc["suggestions"]} >= {"covid vaccination", "covid vaccine"}
    assert all(x["suggestion"] == "covid " + x["term"] for x in doc["suggestions"]) and doc["query"] == "covid vacc?! "
    assert "coronavirus" in [x["term"] for x in json.loads(eng.complete_json(b"cornoav", 5))["suggestions"]]
    assert eng.suggest_json(b"cornoav", 5) == b'{\n  "limit": 5,\n  "query": "cornoav",\n  "suggestions": []\n}'   # suggest itself: unchanged
    # complete_batch on the same table, every edit bound, with and without the fixed prefix
    typed = [suggest_ref.split(s)[1] for s in inputs]
    for e in (0, 1, 2):
        for prefix_len in (0, 2):
            idx, dist, cnt, base, _ = eng.complete_batch_raw(inputs, 10, e, prefix_len)
            _check(tab, typed, [e] * len(typed), prefix_len, 10, idx, dist, cnt)
            assert [int(b) for b in base] == [len(suggest_ref.split(s)[0]) for s in inputs]
    pairs = eng.complete_batch([b"covid vacc"], 5, -1, 1, table=tab.terms)
    assert pairs[0] and all(s.startswith(b"covid ") for s, _ in pairs[0])
    # a two-context engine answers from its primary context, like a one-context one
    two = nsbind.Engine(d, [0, 0])
    for s in inputs[:40] + inputs[-13:]:
        assert two.complete_json(s, 5) == eng.complete_json(s, 5)
    a, b = eng.complete_batch_raw(inputs, 10, -1, 1), two.complete_batch_raw(inputs, 10, -1, 1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4]))
    two.close()
    # a term that arrives with add_documents completes afterwards (the side structures are rebuilt lazily after the reload)
    new = b"zyxwvutsr"
    assert new not in tab.terms
    assert json.loads(eng.complete_json(b"zyxvw", 5))["suggestions"] == []
    eng.add_documents([(b"uidnew", b"t", b"doc/new.json", new + b" " + tab.terms[0])])
    assert eng.correct_build_ms() == 0.0
    tab2 = restate()
    assert new in tab2.terms
    got = eng.complete_json(b"zyxvw", 5)
    assert got == complete_ref.complete_json(tab2, b"zyxvw", 5)
    assert [x["term"] for x in json.loads(got)["suggestions"]] == [new.decode()] and eng.correct_build_ms() > 0.0
    eng.close()
