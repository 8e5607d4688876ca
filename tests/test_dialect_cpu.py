"""The one scanner of the query box against tests/dialect_ref.py, the grammars restated in Python: every short string over an
alphabet of the grammar's own bytes, seeded random longer ones and the directed texts of the three parser tests.  No device."""
import itertools
import random

import pytest

import dialect_ref
import nsbind

ALPHABET = "+-()~ a12"
KINDS = ("two or more clauses", "group with need >= 2", "promoted term next to a group", "unclosed group", ")~ with no digit", "-( )~m", "empty body",
         "~m with nothing to promote")
# the texts test_parse_boolean, test_parse_grouped and test_parse_quorum spell out
DIRECTED = ["+alpha beta -gamma", "covid-19", "+covid-19", "-covid-19 +sars/cov2", "- alpha", "+", "-", "+ -", "--alpha", "-+alpha", "+-alpha", "++alpha",
            "alpha+beta alpha-beta", "+the +of -and vaccine +a -x +y2", "+COVID -Mouse VacCine", "", "   \t\n ", "-alpha -beta", "alpha alpha +alpha -alpha",
            "+(coronavirus covid sars) +(vaccine vaccination) -mouse safety", "+alpha +(beta gamma) +delta", "(a1 b1)", "-(a1 b1)", "(a1) -(b1 c1)",
            "+(covid-19 sars/cov2)", "+(alpha beta gamma", "alpha +(beta", "+(", "-(", "(", "+()", "+() +alpha", "+(the of) +(alpha beta) +( ) +gamma",
            "+(alpha beta)gamma", "+(alpha beta)+gamma", "+(alpha)-(beta)(gamma)", "+(alpha\nbeta\r\n\tgamma)\ndelta", "+(alpha +beta -gamma (delta)", "alpha) beta",
            ") +alpha)", "+(alpha beta) gamma)", "al(pha bx)ta", "+alpha(beta gamma)", "+ (alpha beta)", "++(alpha)", "+(alpha alpha) +(alpha)",
            "+(a1 b1 c1)~2", "(a1 b1 c1)~2", "-(a1 b1)~2", "a1 b1 c1 ~2", "a1 b1 ~2 c1 ~0", "a1 ~0 b1 ~3", "+(a1 b1)~", "+(a1 b1)~xy", "+(a1 b1) ~2", "~12", "~12 a1",
            "+(a1 b1)~12", "~99999999999999999999 a1", "+(a1 b1)~0", "(a1 b1)~0", "+(a1 b1)~2c1 +d1", "+d1 a1 (b1 c1)~2 -e1 ~1", "(a1 b1) c1 ~2", "+(a1 a1 b1)~2", "a~2",
            "+~2", "~2x", "+()~2 +(the of)~2 a1", "+(a1 b1)~99999999999999999999"]


def _corpus():
    texts = ["".join(t) for n in range(6) for t in itertools.product(ALPHABET, repeat=n)]
    assert len(texts) == 66430
    rng = random.Random(20260)
    texts += ["".join(rng.choice(ALPHABET) for _ in range(rng.randint(6, 24))) for _ in range(12000)]
    return texts + DIRECTED


@pytest.fixture(scope="module")
def corpus():
    return _corpus()


def test_the_scanner_parses_every_text_as_the_restated_grammars_do(corpus):
    seen = set()
    for text in corpus:
        b, _, _ = dialect_ref.parse(text, dialect_ref.BOOLEAN)
        assert nsbind.parse_boolean(text) == [(w, r) for w, r, _, _, _ in b], text
        g, _, _ = dialect_ref.parse(text, dialect_ref.GROUPED)
        assert nsbind.parse_grouped(text) == [(w, r, c) for w, r, c, _, _ in g], text
        q, m, kinds = dialect_ref.parse(text, dialect_ref.QUORUM)
        assert nsbind.parse_quorum(text) == (q, m), text
        seen |= kinds
    # reach, from the reference's own account of what each text made the grammar do
    assert [k for k in KINDS if k not in seen] == []


def test_the_dialects_are_nested(corpus):
    n_plain = n_grouped = 0
    for text in corpus:
        g = nsbind.parse_grouped(text)
        if "(" not in text:   # without '(' the grouped dialect is the boolean one
            assert [(w, r) for w, r, _ in g] == nsbind.parse_boolean(text), text
            n_plain += 1
        if "~" not in text:   # with neither quorum form (both need a '~') the quorum dialect is the grouped one
            got, gm = nsbind.parse_quorum(text)
            assert gm == 0 and [(w, r, c) for w, r, c, _, _ in got] == g and not any(p for *_, p in got), text
            n_grouped += 1
    assert n_plain > 1000 and n_grouped > 1000
