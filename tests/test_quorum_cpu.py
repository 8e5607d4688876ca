"""At-least-m-of-n clauses in boolean queries, host side (csrc/ns_boolean_plan.hpp bq_plan_quorum, host/quorum.hpp):
the restatement tests/quorum_ref.py pinned to a brute-force loop, to tests/grouped_ref.py under all-ones needs and to
tests/boolean_ref.py under need = clause size; the planner through tests/quorum_plan_harness.cpp; the parser; a stand-alone host
program under the address and undefined-behaviour sanitizers; and the properties the directed cases of tests/quorum_shapes.py
are named after, and the floors its equivalence checks assert, through the restatement.  No device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import boolean_ref
import grouped_ref
import nsbind
import quorum_ref
import test_grouped_cpu as grouped_cpu
from boolean_ref import MUST, NOT, SHOULD
from rawseg import avgdl_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
HOST = os.path.join(ROOT, "nextsearch-api_amd", "host")
NS_E_INVAL = -1
S, M, X = SHOULD, MUST, NOT


# ---- the restatement ----------------------------------------------------------------------------------------------------
def brute(segments, queries, order, idfs, weights):
    """nested loops over documents, no numpy set operation, no code shared with the restatements"""
    f32 = np.float32
    out = []
    for q in queries:
        cand = []
        for pos, s in enumerate(order):
            n_docs, doc_len, lists = segments[s]
            named = [(li, r, c, max(m, 1)) for ss, li, r, c, m in q if ss == s]
            if not named:
                continue
            has = [set(int(x) for x in lists[li][0].tolist()) for li, _, _, _ in named]
            avgdl = f32(avgdl_of(np.asarray(doc_len, np.uint32)))
            values = []
            for _, r, c, _ in named:
                if r == MUST and c not in values:
                    values.append(c)
            for d in range(n_docs):
                if any(r == NOT and d in h for (_, r, _, _), h in zip(named, has)):
                    continue
                if values:
                    ok = True
                    for v in values:
                        holding, need = set(), 0
                        for (li, r, c, m), h in zip(named, has):
                            if r == MUST and c == v:
                                need = m
                                if d in h:
                                    holding.add(li)
                        if len(holding) < need:
                            ok = False
                else:
                    ok = any(d in h for (_, r, _, _), h in zip(named, has) if r == SHOULD)
                if not ok:
                    continue
                acc = f32(0.0)
                for li, r, _, _ in named:
                    if r == NOT:
                        continue
                    for dd, tf in zip(lists[li][0].tolist(), lists[li][1].tolist()):
                        if dd == d:
                            norm = f32(1.2) * ((f32(1.0) - f32(0.75)) + f32(0.75) * (f32(doc_len[d]) / avgdl))
                            tf = f32(tf)
                            acc = f32(acc + f32(f32(weights[s][li]) * f32(f32(f32(idfs[s][li]) * f32(tf * f32(f32(1.2) + f32(1.0)))) / f32(tf + norm))))
                cand.append((-float(acc), pos, d, s, acc))
        cand.sort(key=lambda c: c[:3])
        out.append([(acc, s, d) for _, _, d, s, acc in cand])
    return out


# over grouped_cpu.random_segments: four random lists, an empty one (4) and one with a posting >= n_docs (5)
QUERIES = [[], [(0, 0, M, 0, 1)], [(0, 0, M, 0, 2)], [(0, 0, M, 0, 2), (0, 0, M, 0, 2)],
           [(0, 0, M, 0, 2), (0, 1, M, 0, 2)], [(0, 0, M, 0, 2), (0, 1, M, 0, 2), (0, 2, M, 0, 2)], [(0, 0, M, 0, 3), (0, 1, M, 0, 3), (0, 2, M, 0, 3)],
           [(0, 0, M, 0, 2), (0, 0, M, 0, 2), (0, 1, M, 0, 2)], [(0, 0, M, 3, 2), (0, 4, M, 3, 2), (0, 1, M, 3, 2)], [(0, 0, M, 3, 2), (0, 4, M, 3, 2)],
           [(0, 0, M, 0, 2), (0, 1, M, 0, 2), (0, 2, M, 0, 2), (0, 3, X, 0, 0)], [(0, 0, M, 0, 2), (0, 1, M, 0, 2), (0, 2, M, 1, 0), (0, 3, M, 1, 0), (0, 5, S, 0, 0)],
           [(0, 0, M, 7, 2), (0, 1, M, 7, 2), (0, 2, M, 7, 2), (0, 1, M, 2, 2), (0, 2, M, 2, 2), (0, 3, M, 2, 2)], [(0, 5, M, 0, 2), (0, 0, M, 0, 2), (0, 1, M, 0, 2)],
           [(1, 0, M, 3, 2), (1, 1, M, 3, 2), (1, 2, X, 3, 0), (1, 3, M, 3, 2), (1, 5, S, 1, 9)],
           [(0, 0, M, 9, 2), (1, 1, M, 9, 2), (2, 2, X, 0, 0), (2, 3, M, 9, 1), (1, 0, M, 9, 2), (0, 5, M, 9, 2), (2, 0, M, 9, 1), (0, 1, S, 9, 0), (1, 4, M, 9, 2)],
           [(2, 0, M, 0, 4), (2, 1, M, 0, 4), (2, 2, M, 0, 4), (2, 3, M, 0, 4), (2, 5, M, 0, 4)], [(2, 0, M, 0, 5), (2, 1, M, 0, 5), (2, 2, M, 0, 5), (2, 3, M, 0, 5), (2, 4, M, 0, 5)],
           [(2, li, M, 0, 7) for li in (0, 1, 2, 3, 5, 0, 1, 2)]]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_restatement_equals_a_brute_force_loop(seed):
    segments, idfs, weights = grouped_cpu.random_segments(seed)
    for order in ([0, 1, 2], [2, 0, 1]):
        got = quorum_ref.quorum_all(segments, QUERIES, order, idfs, weights)
        want = brute(segments, QUERIES, order, idfs, weights)
        for qi, (g, w) in enumerate(zip(got, want)):
            assert [(s, d) for _, s, d in g] == [(s, d) for _, s, d in w], (order, qi)
            assert [np.float32(x).view(np.uint32) for x, _, _ in g] == [np.float32(x).view(np.uint32) for x, _, _ in w], (order, qi)
        docs = [set(int(x) for x in d.tolist() if x < segments[0][0]) for d, _ in segments[0][2]]
        assert got[2] == [] and got[3] == [] and got[9] == [] and got[18] == []       # fewer distinct live lists than the need: a dead group
        assert sorted(d for _, _, d in got[4]) == sorted(docs[0] & docs[1]) == sorted(d for _, _, d in got[7]) == sorted(d for _, _, d in got[8])
        assert sorted(d for _, _, d in got[6]) == sorted(docs[0] & docs[1] & docs[2])
        assert sum(len(g) >= 2 for g in got) >= 6
        for k in (1, 5, 100):
            for (found, hits), rows in zip(quorum_ref.hits(got, k), got):
                assert found == len(rows) and hits == rows[:k]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_all_ones_needs_are_the_grouped_restatement(seed):
    segments, idfs, weights = grouped_cpu.random_segments(seed)
    for need in (1, 0):
        queries = [[(s, li, r, c, need) for s, li, r, c in q] for q in grouped_cpu.QUERIES]
        for order in ([0, 1, 2], [2, 0, 1]):
            got = quorum_ref.quorum_all(segments, queries, order, idfs, weights)
            want = grouped_ref.grouped_all(segments, grouped_cpu.QUERIES, order, idfs, weights)
            bits = lambda rows: [[(np.float32(v).view(np.uint32), s, d) for v, s, d in r] for r in rows]      # noqa: E731
            assert bits(got) == bits(want)
            assert sum(len(g) >= 2 for g in got) >= 8


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_need_equal_to_the_clause_size_is_the_boolean_restatement(seed):
    segments, idfs, weights = grouped_cpu.random_segments(seed)
    lists_of = [[0, 1], [0, 1, 2], [1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3, 5], [2, 2, 3], [0, 4], [5]]
    quorum, plain = [], []
    for s in range(3):
        for ls in lists_of:
            live = len({li for li in ls if len(segments[s][2][li][0])})
            quorum.append([(s, li, M, 77, max(live, 1)) for li in ls] + [(s, 3, X, 0, 0)] * (len(ls) == 2) + [(s, 1, S, 0, 0)])
            # boolean_ref: an empty MUST list kills the group, as a clause short of live members does
            plain.append([(s, li, M) for li in ls] + [(s, 3, X)] * (len(ls) == 2) + [(s, 1, S)])
    got = quorum_ref.quorum_all(segments, quorum, [2, 0, 1], idfs, weights)
    want = boolean_ref.boolean_all(segments, plain, [2, 0, 1], idfs, weights)
    bits = lambda rows: [[(np.float32(v).view(np.uint32), s, d) for v, s, d in r] for r in rows]      # noqa: E731
    for qi, (g, w, q) in enumerate(zip(bits(got), bits(want), quorum)):
        if any(len(segments[s][2][li][0]) == 0 for s, li, r, _, _ in q if r == M):
            continue            # [0, 4]: the clause is its one live list with need 1, while every-ref-MUST dies on the empty list
        assert g == w, qi
    assert sum(len(g) >= 2 for g in got) >= 4


# ---- the directed cases of the GPU suite have the properties their names claim ---------------------------------------------
def test_the_directed_cases_are_what_their_names_say():
    import quorum_shapes as shapes
    lists = shapes.lists()
    n, tile, win = shapes.N_DOCS, shapes.SMALL_TILE, shapes.SMALL_WIN
    docs = [set(int(x) for x in d.tolist() if x < n) for d, _ in lists]
    A, B, Cc = docs[shapes.A], docs[shapes.B], docs[shapes.C]

    def matched(name):
        return quorum_ref.group_matched(lists, shapes.CASES[name], n).tolist()

    def held(d, members):
        return sum(d in docs[li] for li in members)

    # two of three: documents holding exactly 0, 1, 2 and 3 of the members exist, and exactly those with 2 or 3 match
    counts = {d: held(d, (shapes.A, shapes.B, shapes.C)) for d in range(n)}
    assert set(counts.values()) == {0, 1, 2, 3}
    assert matched("two of three") == sorted(d for d, c in counts.items() if c >= 2) == [10, 40, 41, 42, 200]
    assert matched("three of three") == sorted(A & B & Cc) == [10, 200]
    # saturation: document 77 lies in all nine / ten lists: two planes (which count to 3) wrap at the fourth and again at the eighth
    # addition unless they saturate; three planes (to 7) wrap at the eighth
    assert held(77, shapes.SAT[:9]) == 9 and held(77, shapes.SAT) == 10
    assert matched("saturation: two of nine") == sorted(d for d in range(n) if held(d, shapes.SAT[:9]) >= 2) == [10, 77, 200, 211, 212, 213, 214]
    assert matched("saturation: three of nine") == [10, 77, 200, 212, 213, 214]
    assert matched("saturation: seven of ten") == [77, 200, 213] and held(214, shapes.SAT) == 6 and matched("six of ten") == [10, 77, 200, 213, 214]
    # per-window exit: window 1 holds a posting of one member alone, window 2 of both, in the same tile
    w1, w2 = range(win, 2 * win), range(2 * win, 3 * win)
    assert any(d in docs[shapes.W1] for d in w1) and not any(d in docs[shapes.W2] for d in w1)
    assert any(d in docs[shapes.W1] for d in w2) and any(d in docs[shapes.W2] for d in w2) and 3 * win <= tile
    assert matched("per-window exit") == [70]
    # a duplicate counts once: a document with only A is out; the score carries A twice
    assert matched("duplicate member") == sorted(A & B) and 3 in A and 3 not in B and 3 not in matched("duplicate member")
    assert matched("a duplicate alone cannot make two") == []
    idf, w = shapes.small_weights(len(lists))
    seg = (n, (5 + np.arange(n) % 41).astype(np.uint32), lists)
    twice = boolean_ref.group_scores(seg, [(shapes.A, M), (shapes.A, M), (shapes.B, M)], idf, w)
    once = boolean_ref.group_scores(seg, [(shapes.A, M), (shapes.B, M)], idf, w)
    a_alone = boolean_ref.group_scores(seg, [(shapes.A, M)], idf, w)
    assert np.float32(twice[10]) != np.float32(once[10]) and np.float32(twice[10]) == np.float32(np.float32(np.float32(a_alone[10]) + np.float32(a_alone[10])) +
                                                                                                 np.float32(np.float32(once[10]) - np.float32(a_alone[10])))
    # planes cleared: 40, 41 and 42 reach the need in the first clause and need - 1 in the second
    second = (shapes.P1, shapes.P2, shapes.P3)
    assert all(counts[d] == 2 and held(d, second) == 1 for d in (40, 41, 42)) and matched("planes cleared") == [10, 200]
    anyof = docs[shapes.P1] | docs[shapes.P2]
    assert matched("a counted clause before an any-of clause") == sorted(set(matched("two of three")) & anyof) == matched("an any-of clause before a counted clause")
    assert len(matched("a counted clause before an any-of clause")) == 4
    # word tail: document 299 is the last bit of the partial last word of the bitmap
    assert n - 1 == 299 and n % 32 != 0 and matched("word tail") == [299]
    # out-of-range postings: 305 lies in both members, and is no document
    assert 305 in lists[shapes.T2][0].tolist() and 305 in lists[shapes.T3][0].tolist() and matched("out-of-range postings") == []
    assert matched("out-of-range postings, three members") == [299]
    assert matched("tile edges") == [127, 128, 255, 256] and tile == 128
    assert matched("NOT after count") == [40, 42, 200] and {10, 41} <= docs[shapes.NOTL]
    for name in ("a long item: seven of ten, each named six times", "a long item: the counted clause behind"):
        assert len(shapes.CASES[name]) > 64
    assert matched("a long item: seven of ten, each named six times") == [200] and matched("a long item: the counted clause behind") == [10, 200]
    assert matched("an empty member is dropped") == sorted(A & B)
    assert matched("single ref, need 1") == sorted(A) and matched("single ref, need 2") == [] and matched("one survivor, need 1") == sorted(A)
    assert len(matched("more than a hundred")) > 100 and len(matched("more than a hundred, with optional terms")) > 100
    assert matched("needs on SHOULD and NOT refs are not read") == sorted((docs[shapes.R1] | docs[shapes.R3]) - docs[shapes.R2])
    needs = {m for q in shapes.CASES.values() for _, r, _, m in q if r == M}
    assert {2, 7} <= needs and {3, 6} <= needs                                     # mixed needs in one launch, two planes and three
    # too few members: with three segments the clause is short of a live member in segment 1 alone
    segments, queries, idfs, weights, order = shapes.directed_inputs(3)
    few = queries[shapes.NAMES.index("too few members")]
    assert [s for _, s, d in quorum_ref.matched(segments, few, order) if len(d)] == [2, 0]
    founds = [sum(len(d) for _, _, d in quorum_ref.matched(segments, q, order)) for q in queries]
    assert 0 in founds and max(founds) > 100 and len(set(founds)) >= 8


def test_the_gpu_suites_equivalence_inputs_clear_their_floors():
    """tests/test_quorum_gpu.py compares whole answers with the siblings and asserts how many queries had found >= 2: the chosen
    inputs have that many, by the restatements"""
    import grouped_shapes
    import quorum_shapes as shapes
    covered = 0
    for n_segs in (1, 3):
        segments, queries, idfs, weights, order = grouped_shapes.directed_inputs(n_segs)
        ones = [[(s, li, r, c, 1) for s, li, r, c in q] for q in queries]
        got = quorum_ref.quorum_all(segments, ones, order, idfs, weights)
        want = grouped_ref.grouped_all(segments, queries, order, idfs, weights)
        assert [[(s, d) for _, s, d in rows] for rows in got] == [[(s, d) for _, s, d in rows] for rows in want]
        covered += sum(len(rows) >= 2 for rows in got)
    assert covered >= shapes.FLOOR_ONES, covered
    segments, quorum, plain, idfs, weights = shapes.full_need_inputs()
    assert len(quorum) >= 5 and max(m for q in quorum for _, _, _, _, m in q) >= 3
    got = quorum_ref.quorum_all(segments, quorum, [2, 0, 1], idfs, weights)
    want = boolean_ref.boolean_all(segments, plain, [2, 0, 1], idfs, weights)
    assert [[(np.float32(v).view(np.uint32), s, d) for v, s, d in rows] for rows in got] == [[(np.float32(v).view(np.uint32), s, d) for v, s, d in rows] for rows in want]
    assert sum(len(rows) >= 2 for rows in got) >= shapes.FLOOR_FULL
    # the product-tile family: members on either side of a tile edge
    tile = 1 << 17
    segments, queries, idfs, weights, docs = shapes.product_inputs(tile)
    founds = [sum(len(d) for _, _, d in quorum_ref.matched(segments, q)) for q in queries]
    assert founds[0] >= 40 and founds[1] >= 9 and founds[2] == 0 and founds[4] == 0 and founds[5] >= 1 and founds[6] >= 1, founds
    edge = set(quorum_ref.matched(segments, queries[0])[0][2].tolist())
    assert {tile - 1, tile} <= edge


# ---- the planner --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("quorum_plan") / "quorum_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "quorum_plan_harness.cpp")], check=True)
    lib = C.CDLL(so)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.quorum_plan.argtypes = [C.c_int, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, u32, u32, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64), vp, C.POINTER(u32),
                                C.c_char_p, u32]
    lib.quorum_ref_bytes.restype = u32
    lib.quorum_max_need.restype = u32
    return lib


def plan(harness, queries, segs, tile=128, which=0, clauses_null=False, needs_null=False):
    """queries: per query [(seg_id, count, byte_off, role, clause, need)] (idf = 1 + ref index, qweight 0.5); segs: [(seg_id, n_docs,
    n_postings)]; which: 0 bq_plan_quorum, 1 bq_plan_grouped, 2 bq_plan -> (rc, items as rows of 6, planned refs as rows of (first,
    count, role, clause index, need as stored, duplicate flag, idf), raw ref bytes, largest need, message)"""
    flat = [r for q in queries for r in q]
    refs = np.array([(s, c, o, 1.0 + i, 0.5) for i, (s, c, o, _, _, _) in enumerate(flat)], dtype=nsbind.TERM_DTYPE) if flat else np.zeros(0, nsbind.TERM_DTYPE)
    roles = np.array([r[3] for r in flat] + [0], dtype=np.uint8)
    clauses = np.array([r[4] for r in flat] + [0], dtype=np.uint16)
    needs = np.array([r[5] for r in flat] + [0], dtype=np.uint8)
    qd, at = [], 0
    for q in queries:
        qd += [at, len(q)]
        at += len(q)
    qd = np.array(qd + [0, 0], dtype=np.uint32)
    ids, docs, posts = (np.array([s[i] for s in segs] + [0], dtype=t) for i, t in ((0, np.uint32), (1, np.uint32), (2, np.uint64)))
    cap_i, cap_r = 4096, len(flat) + 1
    items, pref = np.zeros((cap_i, 6), np.uint32), np.zeros((cap_r, 7), np.uint64)
    raw = np.zeros(cap_r * harness.quorum_ref_bytes(), np.uint8)
    ni, nr, mx = C.c_uint64(), C.c_uint64(), C.c_uint32()
    err = C.create_string_buffer(256)
    rc = harness.quorum_plan(which, qd.ctypes.data, len(queries), refs.ctypes.data if len(refs) else None, roles.ctypes.data,
                             None if clauses_null else clauses.ctypes.data, None if needs_null else needs.ctypes.data, len(flat), ids.ctypes.data, docs.ctypes.data,
                             posts.ctypes.data, len(segs), tile, items.ctypes.data, cap_i, C.byref(ni), pref.ctypes.data, cap_r, C.byref(nr), raw.ctypes.data, C.byref(mx),
                             err, len(err))
    assert ni.value <= cap_i and nr.value <= cap_r
    planned = [(int(f), int(c), int(r), int(cl), int(ne), int(du), float(np.array([w], np.uint32).view(np.float32)[0])) for f, c, r, cl, ne, du, w in pref[: nr.value].tolist()]
    return rc, items[: ni.value].tolist(), planned, raw[: nr.value * harness.quorum_ref_bytes()].tobytes(), int(mx.value), err.value.decode()


SEGS = [(7, 100, 1000), (3, 50, 1000), (9, 10, 1000)]            # positions 0, 1, 2 carry the ids 7, 3, 9
Q0 = [(3, 5, 80, M, 1, 2), (7, 6, 0, S, 2, 0), (9, 2, 160, X, 3, 0), (3, 4, 240, S, 4, 0), (7, 1, 400, X, 5, 0), (9, 3, 480, S, 6, 0), (7, 6, 0, M, 7, 3), (3, 2, 0, M, 1, 2)]
Q1 = [(7, 0, 0, M, 1, 1), (7, 3, 0, S, 1, 0), (3, 3, 0, M, 9, 1)]


def test_without_needs_the_plan_is_bq_plan_groupeds_byte_for_byte(harness):
    assert harness.quorum_ref_bytes() == 32 and harness.quorum_max_need() == 7 == quorum_ref.MAX_NEED
    want = plan(harness, [Q0, Q1], SEGS, tile=32, which=1)
    got = plan(harness, [Q0, Q1], SEGS, tile=32, needs_null=True)
    assert want[0] == 0 and got == want and len(want[3]) == 32 * len(want[2]) > 0 and got[4] == 0
    assert all(r[4] == 0 and r[5] == 0 for r in got[2])                              # no need and no flag where the call had none
    # bq_plan_grouped is bq_plan_quorum without needs, so the comparison above cannot fail by itself: what pins the bytes is the record
    # of what bq_plan_grouped gave for these inputs before it became that wrapper (items, (first, count, role, clause, idf), sha256 of the raw refs)
    assert got[1] == [[0, 0, 0, 3, 0, 32], [0, 0, 0, 3, 32, 64], [0, 0, 0, 3, 64, 96], [0, 0, 0, 3, 96, 100], [0, 1, 3, 3, 0, 32], [0, 1, 3, 3, 32, 50],
                      [0, 2, 6, 2, 0, 10], [1, 1, 8, 1, 0, 32], [1, 1, 8, 1, 32, 50]]
    assert [r[:4] + r[6:] for r in got[2]] == [(0, 6, 0, 0, 2.0), (50, 1, 2, 0, 5.0), (0, 6, 1, 0, 7.0), (10, 5, 1, 0, 1.0), (30, 4, 0, 0, 4.0), (0, 2, 1, 0, 8.0),
                                               (20, 2, 2, 0, 3.0), (60, 3, 0, 0, 6.0), (0, 3, 1, 0, 11.0)]
    import hashlib
    assert hashlib.sha256(got[3]).hexdigest() == "aa873990b27f44ee97c7d175583b5c2399cd5fb0c804e9d0951d84cf8927dce8"
    # ... and without clauses either it is bq_plan's
    assert plan(harness, [Q0, Q1], SEGS, tile=32, clauses_null=True, needs_null=True) == plan(harness, [Q0, Q1], SEGS, tile=32, which=2)
    # all needs 1: the same items and refs but for the need stored next to the clause index
    ones = [[r[:5] + (1,) for r in q] for q in (Q0, Q1)]
    a = plan(harness, ones, SEGS, tile=32)
    assert a[0] == 0 and a[1] == want[1] and [r[:4] + r[6:] for r in a[2]] == [r[:4] + r[6:] for r in want[2]] and a[4] == 1
    assert all(r[4] == (1 if r[2] == M else 0) and r[5] == 0 for r in a[2])


def test_the_need_and_the_duplicate_flag_live_in_spare_bits_of_the_clause_word(harness):
    # clause 900 (need 2): list at 0 named twice and list at 320; clause 17 (need 0 = 1): its first ref is empty; a NOT and a SHOULD ref
    q = [(7, 5, 0, M, 900, 2), (7, 0, 80, M, 17, 0), (7, 6, 160, S, 17, 9), (7, 4, 240, M, 17, 0), (7, 5, 0, M, 900, 2), (7, 3, 320, M, 900, 2), (7, 2, 400, X, 5, 200),
         (7, 5, 0, M, 17, 0), (7, 5, 8, M, 900, 2), (7, 4, 0, M, 900, 2)]
    rc, items, refs, raw, largest, msg = plan(harness, [q], SEGS)
    assert rc == 0, msg
    assert items == [[0, 0, 0, 9, 0, 100]] and largest == 2
    # (first posting, count, role, clause index, need, duplicate): query order, the empty member gone; the same offset with another
    # count, and another offset with the same count, are other lists; the same list in ANOTHER clause counts there
    assert [r[:6] for r in refs] == [(0, 5, M, 0, 2, 0), (20, 6, S, 0, 0, 0), (30, 4, M, 1, 1, 0), (0, 5, M, 0, 2, 1), (40, 3, M, 0, 2, 0), (50, 2, X, 0, 0, 0),
                                     (0, 5, M, 1, 1, 0), (1, 5, M, 0, 2, 0), (0, 4, M, 0, 2, 0)]
    words = np.frombuffer(raw, np.uint32).reshape(-1, 8)[:, 7]
    assert words.tolist() == [0 | 2 << 16, 0, 1 | 1 << 16, 0 | 2 << 16 | 1 << 19, 0 | 2 << 16, 0, 1 | 1 << 16, 0 | 2 << 16, 0 | 2 << 16]


def test_a_clause_short_of_distinct_live_members_kills_the_group_in_its_segment_only(harness):
    # segment 7: clause 4 has two refs of ONE list and an empty ref: one distinct live list < 2; segment 3: two lists
    q = [(7, 5, 0, M, 4, 2), (3, 5, 0, M, 4, 2), (7, 5, 0, M, 4, 2), (3, 4, 80, M, 4, 2), (7, 0, 80, M, 4, 2), (7, 9, 160, S, 0, 0), (3, 9, 160, S, 0, 0), (9, 2, 0, S, 0, 0)]
    rc, items, refs, _, largest, msg = plan(harness, [q], SEGS, tile=32)
    assert rc == 0, msg
    assert items == [[0, 1, 0, 3, 0, 32], [0, 1, 0, 3, 32, 50], [0, 2, 3, 1, 0, 10]] and largest == 2
    assert [(r[1], r[2], r[3], r[4], r[5]) for r in refs] == [(5, M, 0, 2, 0), (4, M, 0, 2, 0), (9, S, 0, 0, 0), (2, S, 0, 0, 0)]
    # one surviving ref: need 1 is the single-list item, need 2 a dead group; need = members lives, need = members + 1 dies
    rc, items, refs, _, largest, _ = plan(harness, [[(7, 0, 0, M, 1, 1), (7, 6, 80, M, 1, 1)], [(7, 0, 0, M, 1, 2), (7, 6, 80, M, 1, 2)],
                                                     [(7, 6, 80, M, 1, 3), (7, 5, 0, M, 1, 3), (7, 4, 160, M, 1, 3)], [(7, 6, 80, M, 1, 4), (7, 5, 0, M, 1, 4), (7, 4, 160, M, 1, 4)]], SEGS)
    assert rc == 0 and [(it[0], it[3]) for it in items] == [(0, 1), (2, 3)] and largest == 3
    # the largest need is that of the refs that were emitted: a dead group's 7 does not count
    rc, items, _, _, largest, _ = plan(harness, [[(7, 6, 80, M, 1, 7)], [(7, 6, 80, M, 1, 2), (7, 5, 0, M, 1, 2)]], SEGS)
    assert rc == 0 and len(items) == 1 and largest == 2
    rc, items, _, _, largest, _ = plan(harness, [[(7, 6, 80, M, 1, 7)]], SEGS)
    assert rc == 0 and items == [] and largest == 0
    for need, planes in ((4, 3), (7, 3)):
        rc, items, _, _, largest, _ = plan(harness, [[(7, 6, 80 + 8 * i, M, 1, need) for i in range(8)]], SEGS)
        assert rc == 0 and len(items) == 1 and largest == need


def test_the_refusals(harness):
    ok = [(7, 5, 0, M, 1, 2), (7, 4, 80, M, 1, 2), (3, 2, 8, X, 1, 0)]
    for queries, kw, match in (([ok[:1] + [(7, 4, 80, M, 1, 8)]], {}, "ref 1: a need of 8 (query 0); at most 7"),
                               ([ok, ok[:1] + [(7, 4, 80, M, 1, 3)]], {}, "query 1: the refs of clause 1 carry the needs 2 and 3"),
                               ([ok[:1] + [(7, 4, 80, M, 1, 0)]], {}, "query 0: the refs of clause 1 carry the needs 2 and 1"),
                               ([ok], {"clauses_null": True}, "needs without clauses"),
                               ([[(7, 5, 0, 3, 1, 1)]], {}, "ref 0: role 3 is none of NS_ROLE_SHOULD, NS_ROLE_MUST, NS_ROLE_NOT"),
                               ([[(7, 5, 4, M, 1, 1)]], {}, "ref 0: byte offset 4 is not a multiple of 8"),
                               ([ok], {"tile": 48}, "facet tile of 48 documents: not a power of two")):
        rc, items, refs, _, largest, msg = plan(harness, queries, SEGS, **kw)
        assert rc == NS_E_INVAL and items == [] and refs == [] and largest == 0 and match in msg, (msg, match)
    # the same clause value in two segments may carry two needs: a clause belongs to a (query, segment) group
    rc, items, _, _, largest, msg = plan(harness, [[(7, 5, 0, M, 1, 2), (7, 4, 80, M, 1, 2), (3, 5, 0, M, 1, 1)]], SEGS)
    assert rc == 0 and len(items) == 2 and largest == 2, msg
    # needs on SHOULD and NOT refs are never read
    rc, items, _, _, largest, msg = plan(harness, [[(7, 5, 0, S, 1, 255), (7, 4, 80, X, 1, 99)]], SEGS)
    assert rc == 0 and len(items) == 1 and largest == 0, msg


# ---- the parser ---------------------------------------------------------------------------------------------------------
def test_parse_quorum():
    P = nsbind.parse_quorum
    group = [("a1", M, 0, 2, False), ("b1", M, 0, 2, False), ("c1", M, 0, 2, False)]
    assert P("+(a1 b1 c1)~2") == (group, 0) == P("(a1 b1 c1)~2")
    assert P("-(a1 b1)~2") == ([("a1", X, 0, 0, False), ("b1", X, 0, 0, False)], 0)
    assert P("a1 b1 c1 ~2") == ([("a1", M, 0, 2, True), ("b1", M, 0, 2, True), ("c1", M, 0, 2, True)], 2)
    assert P("a1 b1 ~2 c1 ~0") == ([("a1", S, 0, 0, False), ("b1", S, 0, 0, False), ("c1", S, 0, 0, False)], 0)      # the last piece wins; ~0 is none
    assert P("a1 ~0 b1 ~3") == ([("a1", M, 0, 3, True), ("b1", M, 0, 3, True)], 3)
    # no digits: no need, and the rest is scanned as before
    assert P("+(a1 b1)~") == ([("a1", M, 0, 1, False), ("b1", M, 0, 1, False)], 0)
    assert P("+(a1 b1)~xy") == ([("a1", M, 0, 1, False), ("b1", M, 0, 1, False), ("xy", S, 0, 0, False)], 0)
    assert P("+(a1 b1) ~2") == ([("a1", M, 0, 1, False), ("b1", M, 0, 1, False)], 2)                                  # a piece of its own: nothing optional to promote
    # the parser is total: a need above the limit is the engine's to refuse
    assert P("~12") == ([], 12) and P("~12 a1") == ([("a1", M, 0, 12, True)], 12) and P("+(a1 b1)~12")[0][0] == ("a1", M, 0, 12, False)
    assert P("~99999999999999999999 a1")[1] == 1000000
    # a need of 0 says nothing; scanning resumes behind the digits
    assert P("+(a1 b1)~0") == ([("a1", M, 0, 1, False), ("b1", M, 0, 1, False)], 0) and P("(a1 b1)~0") == ([("a1", S, 0, 0, False), ("b1", S, 0, 0, False)], 0)
    assert P("+(a1 b1)~2c1 +d1") == ([("a1", M, 0, 2, False), ("b1", M, 0, 2, False), ("c1", S, 0, 0, False), ("d1", M, 1, 1, False)], 0)
    # the promoted clause is the query's last; groups keep their ids; excluded terms are never promoted
    assert P("+d1 a1 (b1 c1)~2 -e1 ~1") == ([("d1", M, 0, 1, False), ("a1", M, 2, 1, True), ("b1", M, 1, 2, False), ("c1", M, 1, 2, False), ("e1", X, 0, 0, False)], 1)
    assert P("(a1 b1) c1 ~2") == ([("a1", M, 0, 2, True), ("b1", M, 0, 2, True), ("c1", M, 0, 2, True)], 2)          # `(a b)` is `a b`
    assert P("+(a1 a1 b1)~2")[0] == [("a1", M, 0, 2, False), ("a1", M, 0, 2, False), ("b1", M, 0, 2, False)]          # duplicates stay
    assert P("a~2") == ([], 0) and P("+~2") == ([], 0) and P("~2x") == ([("2x", S, 0, 0, False)], 0)                  # no whole `~m` piece
    assert P("+()~2 +(the of)~2 a1") == ([("a1", S, 0, 0, False)], 0)                                                # an empty body uses no id
    # a text with neither form parses as parse_grouped parses it
    for text in ("+(coronavirus covid sars) +(vaccine vaccination) -mouse safety", "+alpha +(beta gamma) +delta", "(a1 b1)", "-(a1 b1)", "+covid-19",
                 "+(covid-19 sars/cov2)", "+(alpha beta gamma", "+(", "(", "+() +alpha", "+(alpha beta)gamma", "+(alpha)-(beta)(gamma)", "alpha) beta",
                 "al(pha bx)ta", "+ (alpha beta)", "++(alpha)", "+(alpha alpha) +(alpha)", "+alpha beta -gamma", "--alpha", "", "   \t\n ", "alpha alpha +alpha -alpha"):
        got, m = P(text)
        assert m == 0 and [(w, r, c) for w, r, c, _, _ in got] == nsbind.parse_grouped(text), text
        assert all(n == (1 if r == M else 0) and not p for _, r, _, n, p in got), text


def test_the_planner_and_the_parser_under_the_sanitizers(tmp_path):
    """tests/quorum_host_check.cpp, a program of its own, built with -fsanitize=address,undefined and run here"""
    exe = str(tmp_path / "quorum_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + CSRC, "-I" + HOST, "-o", exe, os.path.join(ROOT, "tests", "quorum_host_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "quorum host check OK" in out.stdout, (out.stdout + out.stderr)[-3000:]


def test_a_host_only_engine_answers_no_quorum_query_and_says_so(tmp_path):
    index = str(tmp_path / "index")
    nsbind.gen_index(index, 2, 45, 512, 77, False)
    eng = nsbind.Engine(index, -1)
    try:
        with pytest.raises(RuntimeError, match="search_quorum_after_batch_flat: no device context"):
            eng.search_quorum_after_batch(["+(t000001 t000002)~2 t000003"], 10)
        with pytest.raises(RuntimeError, match="facet_quorum_batch_flat: no device context"):
            eng.facet_quorum_batch(["t000001 t000002 ~2"], 8)
        with pytest.raises(RuntimeError, match="search_quorum_sorted_batch_flat: no device context"):
            eng.search_quorum_sorted_batch(["+(t000001 t000002)~2"], 10, order="oldest")
        for name, call in (("search_quorum", eng.search_quorum_json), ("search_quorum_faceted", eng.search_quorum_faceted_json),
                           ("search_quorum_sorted", eng.search_quorum_sorted_json)):
            with pytest.raises(RuntimeError, match=name + ": no device context"):
                call("+(t000001 t000002)~2 -t000003", 10)
            body = call("+(t000001 t000002)~2", 10, check=False)
            assert body.startswith('{\n  "error": "') and "no device context" in body
        assert nsbind.PAGE_MODES["quorum"] == 7 and nsbind.PAGE_MODES["quorum_sorted"] == 8
        for mode in ("quorum", "quorum_sorted"):
            with pytest.raises(RuntimeError, match="search_page: no device context"):
                eng.search_page_json("+(t000001 t000002)~2", 10, mode=mode)
    finally:
        eng.close()
