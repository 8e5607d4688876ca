"""Spelling correction without a device: the two restatements of tests/correct_ref.py against each other
and against hand-computed distances, the auto rule of the host library, the candidate rules on the tiny fixture table,
and the failure of a host-only engine."""
import random

import pytest

import correct_ref
import nsbind
import suggest_ref


@pytest.mark.parametrize("a,b,d", [
    (b"", b"", 0), (b"a", b"", 1), (b"", b"abc", 3), (b"a", b"a", 0), (b"a", b"b", 1),
    (b"ab", b"ba", 1),                 # one transposition
    (b"ca", b"abc", 3),                # not 2: no substring is edited twice
    (b"abcdef", b"bacdef", 1),         # transposition at the front
    (b"abcdef", b"abcdfe", 1),         # transposition at the end
    (b"abcdef", b"badcfe", 3),
    (b"kitten", b"sitting", 3), (b"vaccine", b"vacine", 1), (b"coronavirus", b"coronavirs", 1),
    (b"abc", b"acb", 1), (b"abc", b"cab", 2), (b"abcd", b"acbd", 1), (b"a" * 64, b"a" * 63 + b"b", 1),
    (b"x" * 64, b"x" * 65, 1), (b"x" * 65, b"x" * 64, 1), (b"ab" * 32, b"ba" * 32, 2),   # a shift: one deletion, one insertion
])
def test_hand_computed_distances(a, b, d):
    assert correct_ref.osa(a, b) == d
    assert correct_ref.osa(b, a) == d


def _words(rng, n, alphabet, lo, hi):
    return sorted({bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(n)})


def test_numpy_restatement_equals_the_plain_one():
    rng = random.Random(5)
    terms = _words(rng, 600, b"abc", 0, 9) + [b"zz", b"zz", b"zz"]
    terms += [b"q" * 63, b"q" * 64, b"q" * 65, b"q" * 66, b"q" * 67, b"q" * 90]
    terms.sort()
    scores = [rng.choice([0, 1, 1, 2, 7]) for _ in terms]
    tab = correct_ref.Table(terms, scores)
    queries = [correct_ref.random_edits(rng, rng.choice(terms), rng.randint(0, 3), b"abcd") for _ in range(300)]
    queries += [b"", b"a", b"q" * 64, b"q" * 65, b"q" * 63 + b"r", b"zz", b"z"]
    for q in queries:
        for e in (0, 1, 2):
            for p in (0, 1, 3, 100):
                for L in (1, 5, 10):
                    assert tab.fuzzy(q, e, p, L) == correct_ref.fuzzy_plain(terms, scores, q, e, p, L), (q, e, p, L)


def test_lengths_0_1_64_and_65():
    terms = sorted([b"a", b"ab", b"q" * 62, b"q" * 64, b"q" * 65, b"q" * 66, b"q" * 67])
    scores = [3] * len(terms)
    tab = correct_ref.Table(terms, scores)
    assert tab.fuzzy(b"", 2, 0, 10) == []                                          # empty query: nothing
    assert tab.fuzzy(b"q" * 65, 2, 0, 10) == []                                    # longer than NS_FUZZY_MAX_LEN: nothing
    assert [terms[i] for i, _ in tab.fuzzy(b"b", 1, 0, 10)] == [b"a", b"ab"]       # one byte: a substitution and an insertion
    got = tab.fuzzy(b"q" * 64, 2, 0, 10)
    assert [(terms[i], d) for i, d in got] == [(b"q" * 64, 0), (b"q" * 65, 1), (b"q" * 62, 2), (b"q" * 66, 2)]
    assert got == correct_ref.fuzzy_plain(terms, scores, b"q" * 64, 2, 0, 10)


def test_ranking_is_distance_then_score_then_index():
    terms = [b"cab", b"car", b"cat", b"cot", b"cut"]
    scores = [5, 9, 9, 1, 9]
    tab = correct_ref.Table(terms, scores)
    assert tab.fuzzy(b"cat", 1, 0, 10) == [(2, 0), (1, 1), (4, 1), (0, 1), (3, 1)]
    assert tab.fuzzy(b"cat", 1, 2, 10) == [(2, 0), (1, 1), (0, 1)]                 # prefix "ca"
    assert tab.fuzzy(b"cat", 1, 7, 10) == [(2, 0)]                                 # prefix longer than the query: the query itself


def test_auto_rule_of_the_host_library():
    f = nsbind.host_lib().nsh_correct_auto_edits
    assert [f(n) for n in (0, 1, 2, 3, 4, 5, 6, 7, 64, 1000)] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2]
    assert [correct_ref.auto_edits(n) for n in (0, 1, 2, 3, 4, 5, 6, 7, 64, 1000)] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2]


def test_candidate_rules_on_the_tiny_table(tmp_path):
    d = str(tmp_path / "index")
    suggest_ref.write_tiny_index(d, suggest_ref.TINY_SEGMENTS)
    eng = nsbind.Engine(d, -1)
    terms, scores, _ = eng.suggest_table()
    eng.close()
    scores = [int(s) for s in scores]
    cand = correct_ref.candidates(terms, scores)
    by = {}
    for t, s, c in zip(terms, scores, cand):
        by.setdefault(t, []).append((s, c))
    assert by[b"covid"] == [(6, True), (3, False), (2, False)]      # of equal strings only the first, the run's best
    assert by[b"ab"] == [(1, True), (0, False)]
    assert by[b"zz"] == [(0, False), (0, False)]                    # score 0: no document carries it
    assert by[b"car"] == [(3, True), (1, False)]
    tab = correct_ref.Table(terms, scores)
    assert [terms[i] for i, _ in tab.fuzzy(b"zz", 0, 0, 10)] == []  # an exact match that is no candidate
    assert [(terms[i], d) for i, d in tab.fuzzy(b"covd", 1, 0, 10)] == [(b"covid", 1)]
    assert [(terms[i], d) for i, d in tab.fuzzy(b"cta", 1, 0, 10)] == [(b"cat", 1)]


def test_a_host_only_engine_fails_with_a_message(tmp_path):
    d = str(tmp_path / "index")
    suggest_ref.write_tiny_index(d, suggest_ref.TINY_SEGMENTS)
    eng = nsbind.Engine(d, -1)
    with pytest.raises(RuntimeError, match="no CPU spelling correction path"):
        eng.did_you_mean_json("covd vacine", 5)
    with pytest.raises(RuntimeError, match="no CPU spelling correction path"):
        eng.correct_batch_raw(["covd", "vacine"], 5)
    eng.close()
