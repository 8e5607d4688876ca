"""Prefix terms without a GPU: the parser of `vaccin*` (host/prefix.hpp parse_prefixed), Engine::expand_prefix of a
host-only engine against a sorted-list restatement, the numpy restatement of ns_segment_union's rule (tests/union_ref.py) on its
own, and tests/union_plan_harness.cpp and tests/prefix_host_check.cpp built with the host sanitizers and run as programs."""
import bisect
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nsbind
import suggest_ref
import union_ref
from boolean_ref import MUST, NOT, SHOULD
from test_boost_cpu import QUORUM_TEXTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
HOST = os.path.join(ROOT, "nextsearch-api_amd", "host")
S, M, X = SHOULD, MUST, NOT

# every text of the boost suite's parser tests (tests/test_boost_cpu.py) that holds no '*'
BOOST_TEXTS = ["vaccine^2.5", "+vaccine^2.5 covid", "+(covid sars)^0.5", "(a1 b1 c1)~2^3", "(a1 b1)^3 c1", "covid-19^2", "a1^b1^4", "-mouse^4 -(rat hamster)^2 a1",
               "a1^.5 b1^5. c1^0.1 d1^1000000 e1^007", "a1^2 b1 ~2", "+(a1 b1)~2^1.5 c1^2", "ab^", "ab^0", "ab^0.0", "ab^-1", "ab^1e3", "ab^1.2.3", "ab^1000001",
               "ab^1000000.5", "ab^.", "ab^+2", "ab^2x", "ab^ 2", "^", "^^", "ab^99999999999999999999", "+(ab cd)^0 ef", "+(ab cd)^1e3", "+(ab cd)^1.2.3", "(ab cd)~2^",
               "(ab cd)~2^-1 ef", "+(ab cd)^2x", "+(ab cd) ^2", "-(ab cd)^0", "ab^0.000000000000000000000000000000000000000000000001"]


def parse_prefixed(text):
    """nsx::parse_prefixed (host only): ([(term, role, clause, need, promoted, weight, is_prefix)], min_should)"""
    b = text.encode() if isinstance(text, str) else text
    cap = len(b) + 1
    buf = C.create_string_buffer(cap)
    roles, clauses, needs, promoted = np.zeros(cap, np.uint8), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
    weights, prefix = np.zeros(cap, np.float32), np.zeros(cap, np.uint8)
    m = C.c_uint32()
    n = int(nsbind.host_lib().nsh_parse_prefixed(b, buf, cap, roles.ctypes.data, clauses.ctypes.data, needs.ctypes.data, promoted.ctypes.data, weights.ctypes.data,
                                                 prefix.ctypes.data, cap, C.addressof(m)))
    terms = buf.value.decode().split(" ") if n else []
    assert len(terms) == n
    return [(terms[i], int(roles[i]), int(clauses[i]), int(needs[i]), bool(promoted[i]), float(weights[i]), bool(prefix[i])) for i in range(n)], int(m.value)


# ---- the parser ---------------------------------------------------------------------------------------------------------
def test_parse_prefixed_reads_the_star_case_by_case():
    P = parse_prefixed
    assert P("vaccin*") == ([("vaccin", S, 0, 0, False, 1.0, True)], 0)
    assert P("+vaccin*") == ([("vaccin", M, 0, 1, False, 1.0, True)], 0)
    assert P("-mouse*") == ([("mouse", X, 0, 0, False, 1.0, True)], 0)
    assert P("+(vaccin* immun*)~1") == ([("vaccin", M, 0, 1, False, 1.0, True), ("immun", M, 0, 1, False, 1.0, True)], 0)
    assert P("vir*^2.5") == ([("vir", S, 0, 0, False, 2.5, True)], 0)
    assert P("vac*cine") == ([("vac", S, 0, 0, False, 1.0, False), ("cine", S, 0, 0, False, 1.0, False)], 0)   # an alphanumeric byte behind it: a separator
    assert P("a*") == ([], 0)                                                                                    # shorter than 2 bytes
    assert P("the*") == ([("the", S, 0, 0, False, 1.0, True)], 0) and P("the") == ([], 0)                        # no stop-word test
    assert P("covid-19*") == ([("covid", S, 0, 0, False, 1.0, False), ("19", S, 0, 0, False, 1.0, True)], 0)
    assert P("**") == ([], 0) and P("x *") == ([], 0) and P("*") == ([], 0)
    assert P("ab *") == ([("ab", S, 0, 0, False, 1.0, False)], 0)                                                # not directly behind the token
    assert P("VacCin*") == ([("vaccin", S, 0, 0, False, 1.0, True)], 0)                                          # lower-cased
    assert P("vaccin*, Immun*.") == ([("vaccin", S, 0, 0, False, 1.0, True), ("immun", S, 0, 0, False, 1.0, True)], 0)
    assert P("vir*^0.5 vir*") == ([("vir", S, 0, 0, False, 0.5, True), ("vir", S, 0, 0, False, 1.0, True)], 0)
    assert P("+(vir* covid)^3 -(mouse* rat)^2 sars* ~1") == ([("vir", M, 0, 1, False, 3.0, True), ("covid", M, 0, 1, False, 3.0, False), ("mouse", X, 0, 0, False, 1.0, True),
                                                              ("rat", X, 0, 0, False, 1.0, False), ("sars", M, 1, 1, True, 1.0, True)], 1)


def test_a_text_without_a_star_parses_as_parse_boosted_parses_it():
    texts = BOOST_TEXTS + QUORUM_TEXTS
    assert len(texts) > 80
    for text in texts:
        assert "*" not in text
        got, m = parse_prefixed(text)
        want, wm = nsbind.parse_boosted(text)
        assert m == wm and [t[:6] for t in got] == want and not any(t[6] for t in got), text


# ---- the restatement of the union, on its own ---------------------------------------------------------------------------
def test_the_restatement_states_the_rule():
    flat = np.array([[0, 2], [3, 1], [9, 4],            # list a
                     [3, 5], [4, 1],                    # list b
                     [1, 0xFFFFFFFF], [1, 2]],          # a span that names document 1 twice: the sum wraps to 1
                    dtype=np.uint32)
    gb = [0, 1, 3, 5, 5, 6, 8]                          # [a] [b a] [the span, an empty member] [] [a] [a b]
    off = np.array([0, 24, 0, 40, 0, 0, 0, 24], np.uint64)
    cnt = np.array([3, 2, 3, 2, 0, 3, 3, 2], np.uint32)
    got = union_ref.union(flat, off, cnt, gb, 5)
    assert [d.tolist() for d, _ in got] == [[0, 3, 9], [0, 3, 4], [1], [], [0, 3, 9], [0, 3, 4]]
    assert [t.tolist() for _, t in got] == [[2, 1, 4], [2, 6, 1], [1], [], [2, 1, 4], [2, 6, 1]]   # document 9 >= n_docs: kept by a copy, dropped by a union
    assert union_ref.bound(cnt, gb, 5) == 3 + 5 + 2 + 0 + 3 + 5
    assert union_ref.rounds(cnt, gb, 5, 20) == 3 and union_ref.rounds(cnt, gb, 5, 40) == 2 and union_ref.rounds(cnt, gb, 5, 1) == 3
    assert union_ref.rounds(cnt, gb, 5, 64 << 20) == 1


# ---- expand_prefix on a host-only engine ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_only(tmp_path_factory):
    index = str(tmp_path_factory.mktemp("prefix_cpu") / "index")
    nsbind.gen_index(index, 3, 150, 2048, 31, False)
    eng = nsbind.Engine(index, -1)
    terms, scores, _ = eng.suggest_table()
    assert terms == sorted(terms) and len(terms) > 200
    yield eng, [t.decode() for t in terms], [int(s) for s in scores]
    eng.close()


def under(terms, prefix):
    """the rows of the sorted list that begin with the prefix (lower-case alnum bytes, all below 0x7f)"""
    rows = range(bisect.bisect_left(terms, prefix), bisect.bisect_left(terms, prefix + "\x7f"))
    assert all(terms[i].startswith(prefix) for i in rows)
    return list(rows)


def restated(terms, scores, prefix, limit, held=None):
    """the sorted-list restatement: the terms under the prefix; above the limit the best by (score descending, bytes ascending: the
    row, in a list sorted by bytes), in byte order again; then a term the lexicons do not hold as it stands (`held`: the raw terms)
    goes, and a term the list holds twice comes once"""
    rows = under(terms, prefix)
    kept = sorted(sorted(rows, key=lambda i: (-scores[i], i))[:limit])
    out = []
    for i in kept:
        if (held is None or terms[i] in held) and (not out or out[-1] != terms[i]):
            out.append(terms[i])
    return out, len(rows) > limit


# Raw terms per segment with their df.  Summed: vaccine 8, then a tie of three at 4 (vaccination < vaccines < vaccinology by bytes),
# "vaccinia" 3 from a raw term that is not those bytes (the dictionary does not hold it), vaccinated 2, "vaccine" a second time from
# VACCINE 2, vaccin 1; virus 8, viral = virology 7, virion 1.
TINY = [
    [(b"vaccine", 6), (b"vaccines", 4), (b"vaccination", 4), (b"vaccinated", 2), (b"vaccin", 1), (b"vac-cinia", 3), (b"VACCINE", 2), (b"virus", 7), (b"viral", 7),
     (b"virology", 7), (b"virion", 1), (b"immune", 5), (b"zebra", 1)],
    [(b"vaccine", 2), (b"vaccinology", 4), (b"virus", 1), (b"immunity", 5)],
]


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    index = str(tmp_path_factory.mktemp("prefix_tiny") / "index")
    suggest_ref.write_tiny_index(index, TINY)
    eng = nsbind.Engine(index, -1)
    terms, scores = suggest_ref.table(index)
    got_terms, got_scores, _ = eng.suggest_table()
    assert list(got_terms) == terms and [int(x) for x in got_scores] == scores
    terms = [t.decode() for t in terms]
    yield eng, terms, scores, {t.decode("latin-1") for seg in TINY for t, _ in seg}
    eng.close()


def test_expand_prefix_equals_the_sorted_list(tiny):
    eng, terms, scores, held = tiny
    E = eng.expand_prefix
    assert E("vaccin") == (["vaccin", "vaccinated", "vaccination", "vaccine", "vaccines", "vaccinology"], False)   # equal to a whole term, which is included
    assert E("vaccine") == (["vaccine", "vaccines"], False)
    assert E("zeb") == (["zebra"], False) and E("zebra") == (["zebra"], False)                                        # one match
    assert E("qq") == ([], False) and E("vaccinez") == ([], False) and E("zz") == ([], False)                        # none
    assert E("VacCin*")[0] == E("vaccin")[0]                                                                          # normalised like a table term
    assert E("vaccini") == ([], False)                                                                                # "vaccinia" is no term of a lexicon as it stands
    # truncation at 1, at 2 and at exactly the number of matches; the tie at 4 and the tie at 7 are broken by bytes
    assert len(under(terms, "vaccin")) == 8 and len(under(terms, "vir")) == 4
    assert E("vaccin", 1) == (["vaccine"], True) and E("vaccin", 2) == (["vaccination", "vaccine"], True)
    assert E("vaccin", 3) == (["vaccination", "vaccine", "vaccines"], True)
    assert E("vaccin", 5) == (["vaccination", "vaccine", "vaccines", "vaccinology"], True)                            # the fifth is "vaccinia"
    assert E("vaccin", 7) == (["vaccinated", "vaccination", "vaccine", "vaccines", "vaccinology"], True)              # ... and the seventh "vaccine" again
    assert E("vaccin", 8) == (["vaccin", "vaccinated", "vaccination", "vaccine", "vaccines", "vaccinology"], False)
    assert E("vir", 1) == (["virus"], True) and E("vir", 2) == (["viral", "virus"], True) and E("vir", 3) == (["viral", "virology", "virus"], True)
    assert E("vir", 4) == (["viral", "virion", "virology", "virus"], False) == E("vir", 5)
    for prefix in ("vaccin", "vaccine", "vir", "v", "va", "im", "immun", "", "zebra", "qq"):
        for limit in (1, 2, 3, 4, 5, 6, 7, 8, 9, 1024, 65535):
            assert E(prefix, limit) == restated(terms, scores, prefix, limit, held), (prefix, limit)


def test_expand_prefix_truncates_in_suggests_order(host_only):
    eng, terms, scores = host_only
    # a prefix whose matches hold a score tie that a cut at 1 or at 2 falls into: bytes break it
    tied = None
    for prefix in sorted({t[:n] for t in terms for n in (1, 2, 3, 4)}):
        rows = sorted(under(terms, prefix), key=lambda i: (-scores[i], terms[i]))
        if len(rows) >= 4 and (scores[rows[0]] == scores[rows[1]] or scores[rows[1]] == scores[rows[2]]):
            tied = prefix
            break
    assert tied is not None
    assert len(set(terms)) == len(terms)                                     # (this index holds no two raw terms that normalise alike)
    for prefix in (tied, "t", "t0"):
        n = len(under(terms, prefix))
        assert n >= 3, prefix
        for limit in (1, 2, n - 1, n, n + 1, 65535):
            want = restated(terms, scores, prefix, limit)
            assert want[1] == (limit < n) and len(want[0]) == min(limit, n)
            assert eng.expand_prefix(prefix, limit) == want, (prefix, limit)
    for bad in (65536, 1 << 20):
        with pytest.raises(RuntimeError, match="max_expansions"):
            eng.expand_prefix("t0", bad)


def test_a_host_only_engine_answers_no_prefixed_query_and_says_so(host_only):
    eng = host_only[0]
    with pytest.raises(RuntimeError, match="no device context"):
        eng.search_prefixed_after_batch(["t0*"], 10)
    body = eng.search_prefixed_json("t0*", 10, check=False)
    assert '"error"' in body and "no device context" in body
    assert '"error"' in eng.search_prefixed_page_json("t0*", 10, check=False)


# ---- the stand-alone programs under the sanitizers ------------------------------------------------------------------------
@pytest.mark.parametrize("name, ok", [("union_plan_harness", "union plan check OK"), ("prefix_host_check", "prefix host check OK")])
def test_the_plan_and_the_parser_under_the_sanitizers(tmp_path, name, ok):
    """tests/union_plan_harness.cpp and tests/prefix_host_check.cpp, programs of their own, built with -fsanitize=address,undefined and
    run here"""
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + CSRC, "-I" + HOST, "-o", exe, os.path.join(ROOT, "tests", name + ".cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and ok in out.stdout, (out.stdout + out.stderr)[-3000:]
