"""Collapsed hits without a GPU: the restatement's own properties on the directed inputs (tests/collapse_shapes.py
check_properties over tests/collapse_ref.py), Engine::collapse_table of a host-only engine against the numpy rule, the refusal of
a `*` prefix term, and tests/collapse_host_check.cpp built with the host sanitizers and run as a program."""
import os
import subprocess

import numpy as np
import pytest

import boost_ref
import boost_shapes
import collapse_ref
import collapse_shapes as shapes
import nsbind
import quorum_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
HOST = os.path.join(ROOT, "nextsearch-api_amd", "host")
N_SEG, N_PER_SEG = 3, 120


# ---- the restatement on the directed inputs -----------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[1, 2, 3])
def family(request):
    n_segs = request.param
    segments, queries, idfs, weights, order = shapes.directed_inputs(n_segs)
    order = list(range(n_segs)) if order is None else order
    everything = quorum_ref.quorum_all(segments, queries, order, idfs, weights)
    tables = shapes.with_lift(boost_shapes.tables_for(segments, everything, order), n_segs)
    return n_segs, everything, tables, order


def test_the_directed_cases_are_what_their_names_say(family):
    """each law's named property holds in the reference itself; the identities of nhits and others hold; the collapsed list is a
    subsequence of the uncollapsed one (all asserted inside check_properties)"""
    n_segs, everything, tables, order = family
    whole = shapes.check_properties(everything, tables, order)
    assert len(whole) == len(shapes.LAWS) * 4 and len(everything) == len(shapes.NAMES) == 14


def test_the_cut_at_k_and_the_identities_of_nhits_and_others(family):
    n_segs, everything, tables, order = family
    laws = shapes.laws_for(n_segs)
    rows = boost_ref.boosted_rows(everything, tables["rough"], order)
    for law in shapes.LAWS:
        full = collapse_ref.collapsed(rows, laws[law], 100)
        for k in (0, 1, 10, 64, 65, 100, 1000):
            K = min(max(k, 1), 100)
            got = collapse_ref.collapsed(rows, laws[law], k)
            for q, (hits, groups, others, n, found) in enumerate(got):
                total = collapse_ref.distinct_total(rows[q], laws[law])
                assert n == min(K, total) == len(hits) == len(groups) == len(others) and found == len(rows[q])
                assert hits == full[q][0][:K] and groups == full[q][1][:K] and others == full[q][2][:K]      # a smaller K is a prefix
                assert all((g == 0) <= (o == 0) for g, o in zip(groups, others))
                nz = [g for g in groups if g]
                assert len(nz) == len(set(nz))
                if total <= K:
                    assert sum(o + 1 for o in others) == found
                # the hits in the uncollapsed order, each the first of its group there
                pos = [[(r[3], r[2], r[4]) for r in rows[q]].index(h) for h in hits]
                assert pos == sorted(pos)
                for h, g, p in zip(hits, groups, pos):
                    assert not g or all(int(laws[law][r[3]][r[2]]) != g for r in rows[q][:p])


def test_the_two_wave_family_puts_a_groups_members_into_different_waves():
    segments, queries, idfs, weights, tables, laws, everything = shapes.wave_inputs()
    coll = shapes.check_wave_properties(everything, tables, laws)
    assert len(coll) == shapes.WAVE_DOCS - shapes.WAVE_PAIRS


# ---- collapse_table through a host-only engine ------------------------------------------------------------------------------
def title_of(i):
    r = i % 9
    if r == 0:
        return ""                                            # no title: stands alone
    if r == 1:
        return "  ?! "                                       # nothing alphanumeric: stands alone
    if r < 5:
        return ["A Study of Things", "a study, of THINGS.", "A  study of things"][r - 2] + (" %d" % (i % 4))     # three spellings of four titles
    return "Unique paper number %d" % i


def author_of(i):
    """the `authors` column: "Surname, Given" authors, ';'-separated"""
    return ["Smith, J; Doe, A", "SMITH, John", "", "Lee, K", "Author%d, X" % i][i % 5]


def author_field(authors):
    """what MetaFields holds of it: the first author's surname and " et al.", or nothing"""
    return authors.split(";")[0].split(",")[0].strip() + " et al." if authors.strip() else ""


@pytest.fixture(scope="module")
def titled(tmp_path_factory):
    index = str(tmp_path_factory.mktemp("collapse_cpu") / "index")
    nsbind.gen_index(index, N_SEG, N_PER_SEG, 512, 91, False)
    lines = ["cord_uid,title,publish_time,authors,url"]
    rows = {}
    for i in range(N_SEG * N_PER_SEG):
        if i % 13 == 12:
            continue                                         # no metadata row at all: stands alone
        rows[i] = (title_of(i), author_field(author_of(i)))
        lines.append('u%08d,"%s","2020-01-%02d","%s",http://x/%d' % (i, title_of(i), 1 + i % 28, author_of(i), i))
    with open(os.path.join(index, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    eng = nsbind.Engine(index, -1)                                             # host only
    yield eng, rows
    eng.close()


@pytest.mark.parametrize("field", ["title", "author"])
def test_collapse_table_is_the_dense_id_rule(titled, field):
    eng, rows = titled
    which = 0 if field == "title" else 1
    fields = [[rows.get(s * N_PER_SEG + d, ("", ""))[which] for d in range(N_PER_SEG)] for s in range(N_SEG)]
    want = collapse_ref.dense_keys(fields)
    got = eng.collapse_table(field)
    assert [t.dtype for t in got] == [np.uint32] * N_SEG and [list(map(int, t)) for t in got] == want
    flat = [k for t in want for k in t]
    groups = sorted(set(flat) - {0})
    assert groups == list(range(1, len(groups) + 1)) and flat.count(0) >= N_SEG * N_PER_SEG // 13       # dense from 1; the keyless stand alone
    first = [flat.index(g) for g in groups]
    assert first == sorted(first)                                                                   # by first appearance in manifest order
    if field == "title":
        assert collapse_ref.normalise("a study, of THINGS. 2") == "a study of things 2"
        spellings = {flat[i] for i in range(len(flat)) if i in rows and 2 <= i % 9 < 5 and i % 4 == 2}
        assert len(spellings) == 1 and max(flat.count(g) for g in groups) >= 20                      # three spellings, one group


def test_custom_keys_come_back_as_given_and_are_checked(titled):
    eng, _ = titled
    keys = [((np.arange(N_PER_SEG) * 7 + s) % 11).astype(np.uint32) for s in range(N_SEG)]
    keys[1][5] = 0xFFFFFFFE
    assert all(a.tobytes() == b.tobytes() for a, b in zip(eng.collapse_table(keys), keys))
    bad = [k.copy() for k in keys]
    bad[2][7] = 0xFFFFFFFF
    with pytest.raises(RuntimeError, match="collapse custom: segment 2 holds the reserved key 0xFFFFFFFF"):
        eng.collapse_table(bad)
    with pytest.raises(RuntimeError, match="collapse custom: 2 key arrays for 3 segments"):
        eng.collapse_table(keys[:2])
    with pytest.raises(RuntimeError, match="collapse custom: 2 key arrays for 3 segments"):                 # (the flat C form: whole arrays as far as the keys reach)
        eng.collapse_table([keys[0], keys[1], keys[2][:-1]])
    with pytest.raises(RuntimeError, match="collapse custom: 4 key arrays for 3 segments"):
        eng.collapse_table(keys + [np.ones(3, np.uint32)])
    assert len(eng.collapse_table("title")) == N_SEG                                                # and the engine still answers


def test_a_prefix_term_is_refused_and_a_host_only_engine_says_so(titled):
    eng, _ = titled
    with pytest.raises(RuntimeError, match=r"search_collapsed_batch_flat: query 1 holds the prefix term t0000\*: prefix terms are not collapsed"):
        eng.search_collapsed_batch(["t000001", "+(t000002 t0000*)~1"], 10)
    body = eng.search_collapsed_json("vaccin* t000001", 10, check=False)
    assert body.startswith('{\n  "error": "') and "search_collapsed: the query holds the prefix term vaccin*" in body
    with pytest.raises(RuntimeError, match="search_collapsed_batch_flat: no device context"):
        eng.search_collapsed_batch(["t000001 vac*cine"], 10, collapse="author")                     # (that '*' is a separator)
    body = eng.search_collapsed_json("t000001^2", 10, check=False)
    assert body.startswith('{\n  "error": "') and "search_collapsed: no device context" in body
    assert eng.collapse_tables_on_device() == 0


# ---- the stand-alone program under the host sanitizers --------------------------------------------------------------------
def test_the_table_builder_and_the_plan_under_the_sanitizers(tmp_path):
    """tests/collapse_host_check.cpp, a program of its own, built with -fsanitize=address,undefined and run here"""
    exe = str(tmp_path / "collapse_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + CSRC, "-I" + HOST, "-o", exe, os.path.join(ROOT, "tests", "collapse_host_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "collapse host check OK" in out.stdout, (out.stdout + out.stderr)[-3000:]
