"""Typo-tolerant completion without a device: the two restatements of tests/complete_ref.py against
hand-computed prefix distances and against each other, the limits on a query's length, the bucket of terms past 66 bytes,
the auto rule and the request split of the host library, the JSON layout of the restatement on the tiny fixture table, and
the failure of a host-only engine."""
import json
import random

import pytest

import complete_ref
import correct_ref
import nsbind
import suggest_ref

# (q, c, prefix distance): DESIGN.md §5m's table
HAND = [
    (b"ca", b"abc", 1),                      # osa of the whole strings: 3
    (b"abcd", b"axxbcdzz", 2),               # ends at j = n + 2
    (b"abxxcd", b"abcd", 2),                 # ends at j = n - 2
    (b"abdc", b"abcdef", 1),                 # a transposition at the cut
    (b"ab", b"bazz", 1),
    (b"abcd", b"ab", 2),
    (b"abcd", b"abc", 1),
    (b"a", b"zzzz", 1),
    (b"virsu", b"viruses", 1),
    (b"cornoa", b"coronavirus", 1),
    (b"abcd", b"abcd" + b"x" * 300, 0),
    (b"abcde", b"cdxxx", 3),                 # outside two edits
]


@pytest.mark.parametrize("q,c,d", HAND)
def test_hand_computed_prefix_distances(q, c, d):
    assert complete_ref.pd(q, c) == d
    assert min(correct_ref.osa(q, c[:j]) for j in range(len(c) + 1)) == d        # the definition, every j
    tab = complete_ref.Table([c], [1])
    for e in (0, 1, 2):
        want = [(0, d)] if d <= e else []
        assert tab.complete(q, e, 0, 10) == want
        assert complete_ref.complete_plain([c], [1], q, e, 0, 10) == want


def test_band_edges_are_the_unique_best_end():
    """the pairs that end at j = n + 2 and at j = n - 2: every other cut of the candidate is further away"""
    for q, c, j_best in ((b"abcd", b"axxbcdzz", 6), (b"abxxcd", b"abcd", 4)):
        ds = [correct_ref.osa(q, c[:j]) for j in range(len(c) + 1)]
        assert ds[j_best] == 2 and all(d > 2 for j, d in enumerate(ds) if j != j_best)
        assert j_best == len(q) + 2 or j_best == len(q) - 2


def test_full_distance_of_ca_abc():
    assert correct_ref.osa(b"ca", b"abc") == 3 and complete_ref.pd(b"ca", b"abc") == 1


def _words(rng, n, alphabet, lo, hi):
    return sorted({bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(n)})


def test_numpy_restatement_equals_the_plain_one():
    rng = random.Random(6)
    terms = _words(rng, 300, b"abc", 0, 9) + [b"zz", b"zz", b"zz"]
    terms += [b"q" * 63, b"q" * 64, b"q" * 65, b"q" * 66, b"q" * 67, b"q" * 90, b"qqab" + b"q" * 300]
    terms.sort()
    scores = [rng.choice([0, 1, 1, 2, 7]) for _ in terms]
    tab = complete_ref.Table(terms, scores)
    queries = []
    for _ in range(60):
        w = rng.choice(terms)
        queries.append(correct_ref.random_edits(rng, w[:rng.randint(0, len(w))], rng.randint(0, 3), b"abcd"))
    queries += [b"", b"a", b"z", b"zz", b"q" * 64, b"q" * 65, b"q" * 62 + b"rq", b"qqba", b"qaqb"]
    for q in queries:
        for e in (0, 1, 2):
            for p in (0, 1, 3, 100):
                want = complete_ref.complete_plain(terms, scores, q, e, p, 10)
                assert tab.complete(q, e, p, 10) == want, (q, e, p)
                for L in (1, 5):
                    assert tab.complete(q, e, p, L) == want[:L]


def test_lengths_0_1_64_and_65():
    terms = sorted([b"a", b"ab", b"b", b"q" * 62, b"q" * 64, b"q" * 65, b"q" * 66, b"q" * 67, b"q" * 300])
    scores = [3] * len(terms)
    tab = complete_ref.Table(terms, scores)
    assert tab.complete(b"", 2, 0, 10) == []                                      # empty query: nothing
    assert tab.complete(b"q" * 65, 2, 0, 10) == []                                # longer than NS_FUZZY_MAX_LEN: nothing
    assert complete_ref.complete_plain(terms, scores, b"", 2, 0, 10) == [] == complete_ref.complete_plain(terms, scores, b"q" * 65, 2, 0, 10)
    # one byte, one edit: every candidate matches (the byte can be deleted), the exact starts first
    got = tab.complete(b"b", 1, 0, 10)
    assert [(terms[i], d) for i, d in got][0] == (b"b", 0) and len(got) == len(terms) and all(d == 1 for _, d in got[1:])
    assert [(terms[i], d) for i, d in tab.complete(b"b", 0, 0, 10)] == [(b"b", 0)]
    # 64 bytes: everything from 62 bytes on, however long
    got = tab.complete(b"q" * 64, 2, 0, 10)
    assert [(terms[i], d) for i, d in got] == [(b"q" * m, 0) for m in (64, 65, 66, 67, 300)] + [(b"q" * 62, 2)]
    assert got == complete_ref.complete_plain(terms, scores, b"q" * 64, 2, 0, 10)


def test_the_bucket_past_66_bytes_is_reached():
    terms = sorted([b"long" + b"x" * 63, b"long" + b"y" * 76, b"lone" + b"z" * 296, b"lo"])
    scores = [1, 2, 3, 4][:len(terms)]
    assert sorted(len(t) for t in terms) == [2, 67, 80, 300]
    tab = complete_ref.Table(terms, scores)
    for q, e in ((b"long", 0), (b"lonx", 1), (b"olng", 1), (b"lxnx", 2), (b"long" + b"x" * 60, 0), (b"lone" + b"z" * 59 + b"a", 1)):
        want = complete_ref.complete_plain(terms, scores, q, e, 0, 10)
        assert tab.complete(q, e, 0, 10) == want and want, (q, e)
        assert all(len(terms[i]) >= 67 for i, _ in want if terms[i] != b"lo")
    assert {terms[i] for i, _ in tab.complete(b"lonx", 1, 1, 10)} == {t for t in terms if len(t) >= 67}


def test_edits_0_is_the_prefix_match_ranked_by_score():
    rng = random.Random(9)
    terms = _words(rng, 500, b"abc", 1, 8)
    scores = [rng.randint(1, 9) for _ in terms]
    tab = complete_ref.Table(terms, scores)
    for q in [rng.choice(terms)[:rng.randint(1, 4)] for _ in range(60)] + [b"zz"]:
        want = sorted((i for i, t in enumerate(terms) if t.startswith(q)), key=lambda i: (-scores[i], i))[:10]
        assert [i for i, _ in tab.complete(q, 0, 0, 10)] == want
        assert [terms[i] for i in want] == suggest_ref.suggest(terms, scores, q, 10)


def test_a_query_of_at_most_e_bytes_gets_the_best_by_score():
    rng = random.Random(10)
    terms = _words(rng, 300, b"abc", 0, 8)
    scores = [rng.choice([0, 1, 2, 3, 9]) for _ in terms]
    tab = complete_ref.Table(terms, scores)
    cand = correct_ref.candidates(terms, scores)
    for q in (b"z", b"zz", b"zy"):
        got = tab.complete(q, 2, 0, 10)
        assert len(got) == 10 and all(d == len(q) for _, d in got)
        assert [i for i, _ in got] == sorted((i for i in range(len(terms)) if cand[i]), key=lambda i: (-scores[i], i))[:10]


def test_auto_rule_and_split_of_the_host_library():
    f = nsbind.host_lib().nsh_correct_auto_edits
    assert [f(n) for n in (0, 1, 2, 3, 5, 6, 64)] == [correct_ref.auto_edits(n) for n in (0, 1, 2, 3, 5, 6, 64)] == [0, 0, 0, 1, 1, 2, 2]
    for s in (b"covid vacc", b"covid vacc?! ", b"Cornoav", b"", b"  ", b"a-b"):
        assert nsbind.suggest_split(s) == suggest_ref.split(s)


def test_json_layout_on_the_tiny_table_and_a_host_only_engine_fails_with_a_message(tmp_path):
    d = str(tmp_path / "index")
    suggest_ref.write_tiny_index(d, suggest_ref.TINY_SEGMENTS)
    eng = nsbind.Engine(d, -1)
    terms, scores, _ = eng.suggest_table()
    tab = complete_ref.Table(terms, [int(s) for s in scores])
    # the restated answer over the host library's table, in the layout the engine prints: dump(2), keys in alphabetical order
    got = complete_ref.complete_json(tab, b"see Covd, ", 5)
    doc = json.loads(got.decode("latin-1"))
    assert list(doc) == ["limit", "query", "suggestions"] and doc["limit"] == 5 and doc["query"] == "see Covd, "
    assert doc["suggestions"] == [{"distance": 1, "score": 6, "suggestion": "see covid", "term": "covid"}]   # of three "covid" the first
    assert got.startswith(b'{\n  "limit": 5,\n  "query": "see Covd, ",\n  "suggestions": [\n    {\n      "distance": 1,\n      "score": 6,\n')
    assert complete_ref.complete_json(tab, b"qqqq", 5) == b'{\n  "limit": 5,\n  "query": "qqqq",\n  "suggestions": []\n}'
    doc = json.loads(complete_ref.complete_json(tab, b"cta", 11))
    assert doc["limit"] == 10 and doc["suggestions"][0]["term"] == "cab"                # "cta" -> "ca": one deletion; the best score first
    assert sorted(s["term"] for s in doc["suggestions"]) == ["cab", "caf", "car", "cat"]   # of two "car" one; "covid" is two edits away
    assert [(s["term"], s["distance"]) for s in json.loads(complete_ref.complete_json(tab, b"zz", 5))["suggestions"]] == []   # score 0: no candidate
    # up to here no device was needed; the engine's own answer needs one
    with pytest.raises(RuntimeError, match="no CPU completion path"):
        eng.complete_json("covd", 5)
    with pytest.raises(RuntimeError, match="no CPU completion path"):
        eng.complete_batch_raw(["covd", "vacc"], 5)
    # suggest's failure is what it was
    with pytest.raises(RuntimeError, match="no CPU autocomplete path"):
        eng.suggest_json("co", 5)
    eng.close()
