"""Any-of groups in boolean queries, host side (csrc/ns_boolean_plan.hpp bq_plan_grouped): the restatement
tests/grouped_ref.py pinned to a brute-force loop, to tests/boolean_ref.py where every clause is a singleton and to the
distributive law; the planner through tests/grouped_plan_harness.cpp; and the properties the directed cases of
tests/grouped_shapes.py are named after, and the floors its equivalence checks assert, through the restatement.  No device is
touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import boolean_ref
import facet_shapes
import grouped_ref
import nsbind
from boolean_ref import MUST, NOT, SHOULD
from rawseg import avgdl_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
NS_E_INVAL = -1
S, M, X = SHOULD, MUST, NOT


# ---- the restatement ----------------------------------------------------------------------------------------------------
def brute(segments, queries, order, idfs, weights):
    """nested loops over documents, no numpy set operation, no code shared with grouped_ref or boolean_ref"""
    f32 = np.float32
    out = []
    for q in queries:
        cand = []
        for pos, s in enumerate(order):
            n_docs, doc_len, lists = segments[s]
            named = [(li, r, c) for ss, li, r, c in q if ss == s]
            if not named:
                continue
            has = [set(int(x) for x in lists[li][0].tolist()) for li, _, _ in named]
            avgdl = f32(avgdl_of(np.asarray(doc_len, np.uint32)))
            values = []
            for _, r, c in named:
                if r == MUST and c not in values:
                    values.append(c)
            for d in range(n_docs):
                if any(r == NOT and d in h for (_, r, _), h in zip(named, has)):
                    continue
                if values:
                    ok = True
                    for v in values:
                        if not any(d in h for (_, r, c), h in zip(named, has) if r == MUST and c == v):
                            ok = False
                else:
                    ok = any(d in h for (_, r, _), h in zip(named, has) if r == SHOULD)
                if not ok:
                    continue
                acc = f32(0.0)
                for li, r, _ in named:
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


def random_segments(seed):
    """the 23, 9 and 40 document scheme of test_boolean_cpu: four random lists, an empty one (4) and one with a posting >= n_docs (5)"""
    rng = np.random.default_rng(seed)
    segments, idfs, weights = [], [], []
    for n in (23, 9, 40):
        lists = []
        for m in list(rng.integers(1, n + 1, 4)) + [0]:
            d = np.sort(rng.choice(n, int(m), replace=False)).astype(np.uint32)
            lists.append((d, rng.integers(1, 4, len(d)).astype(np.uint32)))
        lists.append((np.array([1, n - 1, n + 3], np.uint32), np.array([2, 2, 2], np.uint32)))
        segments.append((n, np.full(n, 7, np.uint32) if n == 9 else rng.integers(3, 50, n).astype(np.uint32), lists))   # equal lengths: ties
        idfs.append([float(x) for x in rng.uniform(0.5, 4.0, 6)])
        weights.append([1.0, 0.5, 1.0, 0.25, 1.0, -0.5])
    return segments, idfs, weights


QUERIES = [[], [(0, 0, S, 0)], [(0, 0, M, 0)], [(0, 0, X, 0)],
           [(0, 1, M, 0), (0, 2, M, 0)], [(0, 1, M, 0), (0, 2, M, 1)], [(0, 1, M, 5), (0, 2, M, 5), (0, 3, M, 2)], [(0, 3, M, 2), (0, 1, M, 5), (0, 2, M, 5)],
           [(0, 0, M, 0), (0, 4, M, 0)], [(0, 4, M, 0), (0, 4, M, 0), (0, 1, S, 0)], [(0, 4, M, 1), (0, 0, M, 0)], [(0, 1, M, 0), (0, 1, M, 0)],
           [(0, 1, M, 0), (0, 2, M, 0), (0, 1, X, 0)], [(0, 1, M, 0), (0, 2, M, 0), (0, 1, S, 7)], [(0, 5, M, 0), (0, 4, M, 0)],
           [(1, 0, M, 3), (1, 1, M, 3), (1, 2, X, 3), (1, 3, M, 1), (1, 5, S, 1)],
           [(0, 0, M, 9), (1, 1, M, 9), (2, 2, X, 0), (2, 3, M, 9), (1, 0, M, 200), (0, 5, M, 200), (2, 0, M, 9), (0, 1, S, 9), (1, 4, M, 200)],
           [(2, 0, M, 0), (2, 1, M, 0), (2, 2, M, 1), (2, 3, M, 1), (2, 5, M, 2), (2, 0, M, 2), (2, 1, X, 0)],
           [(0, 3, M, 1), (2, 1, X, 0), (0, 0, S, 0), (2, 2, S, 0), (1, 5, M, 1), (1, 4, M, 2)], [(2, 4, M, 0), (2, 0, S, 0), (1, 0, S, 0)]]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_restatement_equals_a_brute_force_loop(seed):
    segments, idfs, weights = random_segments(seed)
    for order in ([0, 1, 2], [2, 0, 1]):
        got = grouped_ref.grouped_all(segments, QUERIES, order, idfs, weights)
        want = brute(segments, QUERIES, order, idfs, weights)
        for qi, (g, w) in enumerate(zip(got, want)):
            assert [(s, d) for _, s, d in g] == [(s, d) for _, s, d in w], (order, qi)
            assert [np.float32(x).view(np.uint32) for x, _, _ in g] == [np.float32(x).view(np.uint32) for x, _, _ in w], (order, qi)
        # an empty member is dropped: the clause is its other list; a clause of empty lists alone kills the group
        assert [(s, d) for _, s, d in got[8]] == [(s, d) for _, s, d in got[2]] and len(got[8]) > 0
        assert got[9] == [] and got[10] == [] and got[3] == []
        assert sorted(d for _, _, d in got[11]) == sorted(set(segments[0][2][1][0].tolist()))        # named twice: matched once
        assert len(got[14]) == 2                                                                       # the posting >= n_docs is ignored
        assert {s for _, s, _ in got[18]} == {0, 2} and {s for _, s, _ in got[19]} == {1}                 # a dead clause kills its segment only
        assert sum(len(g) >= 2 for g in got) >= 8
        for k in (1, 5, 100):
            for (found, hits), rows in zip(grouped_ref.hits(got, k), got):
                assert found == len(rows) and hits == rows[:k]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_singleton_clauses_are_the_boolean_restatement(seed):
    segments, idfs, weights = random_segments(seed)
    queries = [[(s, li, r, (40000 + 911 * i) % 65536) for i, (s, li, r, _) in enumerate(q)] for q in QUERIES]
    for order in ([0, 1, 2], [2, 0, 1]):
        got = grouped_ref.grouped_all(segments, queries, order, idfs, weights)
        want = boolean_ref.boolean_all(segments, grouped_ref.strip(queries), order, idfs, weights)
        assert [[(np.float32(v).view(np.uint32), s, d) for v, s, d in rows] for rows in got] == [[(np.float32(v).view(np.uint32), s, d) for v, s, d in rows] for rows in want]
        assert sum(len(g) >= 2 for g in got) >= 5


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_two_clauses_of_two_are_the_union_of_the_four_conjunctions(seed):
    segments, _, _ = random_segments(seed)
    seen = 0
    for s, (n, _, lists) in enumerate(segments):
        for a, b, c, d in ((0, 1, 2, 3), (0, 5, 1, 2), (3, 2, 5, 0), (0, 1, 1, 2)):
            whole = grouped_ref.group_matched(lists, [(a, M, 0), (b, M, 0), (c, M, 1), (d, M, 1)], n)
            parts = np.zeros(0, np.int64)
            for x in (a, b):
                for y in (c, d):
                    parts = np.union1d(parts, boolean_ref.group_matched(lists, [(x, M), (y, M)], n))
            assert whole.tolist() == parts.tolist(), (s, a, b, c, d)
            seen += len(whole) > 0
    assert seen >= 6


# ---- the directed cases of the GPU suite have the properties their names claim ---------------------------------------------
def test_the_directed_cases_are_what_their_names_say():
    import grouped_shapes as shapes
    lists = facet_shapes.small_lists()
    n, tile, win = shapes.N_DOCS, shapes.SMALL_TILE, shapes.SMALL_WIN
    docs = [set(int(x) for x in d.tolist() if x < n) for d, _ in lists]
    tiles = [range(lo, min(lo + tile, n)) for lo in range(0, n, tile)]

    def hits(li, span):
        return any(d in docs[li] for d in span)

    def matched(name):
        return grouped_ref.group_matched(lists, shapes.CASES[name], n).tolist()

    assert len(tiles) == 3 and all(hits(7, t) != hits(8, t) for t in tiles)
    assert matched("every tile is hit by one member and missed by the other") == sorted(docs[7] | docs[8]) and len(docs[7] | docs[8]) == 90
    both = sorted((docs[7] | docs[8]) & docs[5])
    assert matched("a two-list clause first") == both == matched("a two-list clause second") and len(both) >= 2
    assert not hits(7, tiles[2]) and not hits(1, tiles[2]) and hits(6, tiles[2])
    assert matched("clause 0 misses the last tile, clause 1 hits it") == sorted((docs[7] | docs[1]) & docs[6])
    # ... and with windows of 32 documents the clause hits tile 0 (document 0) but misses its other three windows, which list 6 hits
    assert hits(1, range(0, win)) and not any(hits(7, range(lo, lo + win)) or hits(1, range(lo, lo + win)) for lo in range(win, tile, win))
    assert all(hits(6, range(lo, lo + win)) for lo in range(win, tile, win))
    assert len(lists[0][0]) == 0 and matched("an empty member is dropped") == sorted(docs[5])
    assert matched("a dead clause") == []
    assert matched("sparse unordered ids, interleaved roles") == sorted(((docs[2] | docs[6]) & (docs[4] | docs[7])) - docs[5])
    three = ((docs[2] | docs[3]) & (docs[4] | docs[5]) & (docs[6] | docs[8]))
    assert matched("three clauses, then an exclusion") == sorted(three - docs[7]) and len(three & docs[7]) > 0 and len(three - docs[7]) >= 2
    assert matched("a list in two clauses") == sorted((docs[4] | docs[5]) & (docs[4] | docs[6])) and docs[4] <= set(matched("a list in two clauses"))
    assert matched("the member adds twice") == sorted(docs[4] | docs[5])
    assert matched("exclusion wins") == sorted(docs[5] - docs[4]) and len(docs[4] & docs[5]) > 0
    assert matched("one survivor: the single-list path") == sorted(docs[6]) and 305 in lists[6][0].tolist() and len(docs[6]) == 256
    assert matched("named twice in a clause: matched once, scored twice") == sorted(docs[6])
    assert matched("70 refs as one clause") == sorted(set().union(*docs[2:9]))
    pairs = [(2 + i % 7, 2 + (i + 1) % 7) for i in range(0, 70, 2)]
    every = set(range(n))
    for a, b in pairs:
        every &= docs[a] | docs[b]
    assert matched("70 refs as 35 clauses of two") == sorted(every) and len(every) >= 2
    garbage = shapes.CASES["garbage clause values on SHOULD and NOT refs"]
    assert matched("garbage clause values on SHOULD and NOT refs") == sorted((docs[2] | docs[5]) - docs[4] - docs[8])
    assert {c for _, r, c in garbage if r != M} >= {0xFFFF, 1, 0xABCD} and {c for _, r, c in garbage if r == M} == {1}
    # the scores: a member adds twice; named twice scores twice what it scores once
    idf, w = shapes.boolean_shapes.small_weights(len(lists))
    seg = (n, (5 + np.arange(n) % 41).astype(np.uint32), lists)
    once = boolean_ref.group_scores(seg, [(6, M)], idf, w)
    twice = boolean_ref.group_scores(seg, [(6, M), (6, M)], idf, w)
    d = sorted(docs[6])[3]
    assert np.float32(twice[d]) == np.float32(np.float32(once[d]) + np.float32(once[d])) != np.float32(once[d])
    # in the three-segment family the dead clause is dead in two segments only, and the single survivor has company in segment 1
    segments, queries, idfs, weights, order = shapes.directed_inputs(3)
    dead = queries[shapes.NAMES.index("a dead clause")]
    assert [s for _, s, docs_ in grouped_ref.matched(segments, dead, order) if len(docs_)] == [1]
    single = queries[shapes.NAMES.index("one survivor: the single-list path")]
    assert sorted((s, li) for s, li, _, _ in single) == [(0, 0), (0, 6), (1, 5), (1, 6), (2, 0), (2, 6)]


def test_the_gpu_suites_equivalence_inputs_clear_their_floors():
    """tests/test_grouped_gpu.py compares whole answers with the boolean siblings and asserts how many queries had found >= 2:
    the chosen inputs have that many, by the restatements"""
    import boolean_shapes
    import grouped_shapes as shapes
    covered = 0
    for segments, queries, idfs, weights, order in shapes.distinct_inputs():
        grouped = shapes.distinct_clauses(queries)
        for q in grouped:
            values = [c for _, _, _, c in q]
            assert len(set(values)) == len(values) and (len(values) < 3 or values != sorted(values))      # all distinct, not ordered
        got = grouped_ref.grouped_all(segments, grouped, order, idfs, weights)
        want = boolean_ref.boolean_all(segments, queries, order, idfs, weights)
        assert [[(s, d) for _, s, d in rows] for rows in got] == [[(s, d) for _, s, d in rows] for rows in want]
        covered += sum(len(rows) >= 2 for rows in got)
    assert covered >= shapes.FLOOR_DISTINCT, covered
    segments, queries, idfs, weights = boolean_shapes.same_role_inputs(M)
    one = grouped_ref.grouped_all(segments, [[(s, li, r, 4242) for s, li, r in q] for q in queries], [2, 0, 1], idfs, weights)
    plain = boolean_ref.boolean_all(segments, [[(s, li, S) for s, li, _ in q] for q in queries], [2, 0, 1], idfs, weights)
    assert [[(np.float32(v).view(np.uint32), s, d) for v, s, d in rows] for rows in one] == [[(np.float32(v).view(np.uint32), s, d) for v, s, d in rows] for rows in plain]
    assert sum(len(rows) >= 2 for rows in one) >= shapes.FLOOR_ONE_CLAUSE
    # the product-tile family: a clause's two lists on either side of a tile edge
    tile = 1 << 17
    segments, queries, idfs, weights, docs = shapes.product_inputs(tile)
    assert docs[0].max() == tile - 1 and docs[1].min() == tile and docs[2].max() == 2 * tile - 1 and docs[3].min() == 2 * tile
    founds = [sum(len(d) for _, _, d in grouped_ref.matched(segments, q)) for q in queries]
    assert founds[0] == 80 and founds[3] == 92 and founds[7] == 0 and founds[1] == founds[2] == 40, founds


# ---- the planner --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("grouped_plan") / "grouped_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "grouped_plan_harness.cpp")], check=True)
    lib = C.CDLL(so)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.grouped_plan.argtypes = [C.c_int, vp, u32, vp, vp, vp, u32, vp, vp, vp, u32, u32, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64), vp, C.c_char_p, u32]
    lib.grouped_ref_bytes.restype = u32
    return lib


def plan(harness, queries, segs, tile=128, roles_null=False, clauses_null=False, use_bq_plan=False, n_refs=None):
    """queries: per query [(seg_id, count, byte_off, role, clause)] (idf = 1 + ref index, qweight 0.5); segs: [(seg_id, n_docs,
    n_postings)] -> (rc, items as rows of 6, planned refs as rows of (first, count, role, clause, idf), raw ref bytes, message)"""
    flat = [r for q in queries for r in q]
    refs = np.array([(s, c, o, 1.0 + i, 0.5) for i, (s, c, o, _, _) in enumerate(flat)], dtype=nsbind.TERM_DTYPE) if flat else np.zeros(0, nsbind.TERM_DTYPE)
    roles = np.array([r for _, _, _, r, _ in flat] + [0], dtype=np.uint8)
    clauses = np.array([c for _, _, _, _, c in flat] + [0], dtype=np.uint16)
    qd, at = [], 0
    for q in queries:
        qd += [at, len(q)]
        at += len(q)
    qd = np.array(qd + [0, 0], dtype=np.uint32)
    ids, docs, posts = (np.array([s[i] for s in segs] + [0], dtype=t) for i, t in ((0, np.uint32), (1, np.uint32), (2, np.uint64)))
    cap_i, cap_r = 4096, len(flat) + 1
    items, pref = np.zeros((cap_i, 6), np.uint32), np.zeros((cap_r, 5), np.uint64)
    raw = np.zeros(cap_r * harness.grouped_ref_bytes(), np.uint8)
    ni, nr = C.c_uint64(), C.c_uint64()
    err = C.create_string_buffer(256)
    rc = harness.grouped_plan(int(use_bq_plan), qd.ctypes.data, len(queries), refs.ctypes.data if len(refs) else None, None if roles_null else roles.ctypes.data,
                              None if clauses_null else clauses.ctypes.data, len(flat) if n_refs is None else n_refs, ids.ctypes.data, docs.ctypes.data,
                              posts.ctypes.data, len(segs), tile, items.ctypes.data, cap_i, C.byref(ni), pref.ctypes.data, cap_r, C.byref(nr), raw.ctypes.data, err, len(err))
    assert ni.value <= cap_i and nr.value <= cap_r
    planned = [(int(f), int(c), int(r), int(cl), float(np.array([w & 0xFFFFFFFF], np.uint32).view(np.float32)[0])) for f, c, r, cl, w in pref[: nr.value].tolist()]
    return rc, items[: ni.value].tolist(), planned, raw[: nr.value * harness.grouped_ref_bytes()].tobytes(), err.value.decode()


SEGS = [(7, 100, 1000), (3, 50, 1000), (9, 10, 1000)]            # positions 0, 1, 2 carry the ids 7, 3, 9


def test_clauses_are_numbered_densely_by_first_appearance_among_the_survivors(harness):
    assert harness.grouped_ref_bytes() == 32
    q = [(7, 5, 0, M, 900), (7, 0, 80, M, 17), (7, 6, 160, S, 17), (7, 4, 240, M, 17), (7, 3, 320, M, 900), (7, 2, 400, X, 5), (7, 1, 480, M, 0), (7, 0, 560, M, 0)]
    rc, items, refs, _, msg = plan(harness, [q], SEGS)
    assert rc == 0, msg
    assert items == [[0, 0, 0, 6, 0, 100]]
    # (first posting, count, role, clause, idf = 1 + ref index): query order, the empty members gone; 900 -> 0, 17 -> 1 (its first
    # ref is empty: numbered where its first SURVIVOR stands), 0 -> 2; SHOULD and NOT refs carry 0
    assert refs == [(0, 5, M, 0, 1.0), (20, 6, S, 0, 3.0), (30, 4, M, 1, 4.0), (40, 3, M, 0, 5.0), (50, 2, X, 0, 6.0), (60, 1, M, 2, 7.0)]


def test_a_dead_clause_kills_the_group_in_its_segment_only(harness):
    q = [(7, 0, 0, M, 4), (3, 5, 0, M, 4), (7, 0, 80, M, 4), (3, 0, 80, M, 4), (7, 9, 160, S, 0), (3, 9, 160, S, 0), (9, 2, 0, S, 0)]
    rc, items, refs, _, msg = plan(harness, [q, q[:2]], SEGS, tile=32)
    assert rc == 0, msg
    # query 0: segment 7 dies (clause 4 has no posting there), segment 3 lives on one member in two tiles, segment 9 has no clause
    assert items == [[0, 1, 0, 2, 0, 32], [0, 1, 0, 2, 32, 50], [0, 2, 2, 1, 0, 10], [1, 1, 3, 1, 0, 32], [1, 1, 3, 1, 32, 50]]
    assert [(r[1], r[2], r[3]) for r in refs] == [(5, M, 0), (9, S, 0), (2, S, 0), (5, M, 0)]
    # one survivor and positive: ref_count == 1, the single-list path of the set kernels; two refs of one clause are not
    rc, items, refs, _, _ = plan(harness, [[(7, 0, 0, M, 1), (7, 6, 80, M, 1)], [(7, 6, 80, M, 1), (7, 6, 80, M, 1)]], SEGS)
    assert rc == 0 and [it[3] for it in items] == [1, 2] and [r[3] for r in refs] == [0, 0, 0]
    # a clause of empty refs next to live clauses, and NOT refs alone
    rc, items, _, _, _ = plan(harness, [[(7, 5, 0, M, 1), (7, 0, 80, M, 2)], [(7, 5, 0, X, 1)], [(7, 0, 0, M, 1), (7, 5, 80, S, 1)]], SEGS)
    assert rc == 0 and items == []


def test_without_clauses_the_plan_is_bq_plans_byte_for_byte(harness):
    q0 = [(3, 5, 80, M, 1), (7, 6, 0, S, 2), (9, 2, 160, X, 3), (3, 4, 240, S, 4), (7, 1, 400, X, 5), (9, 3, 480, S, 6), (7, 6, 0, M, 7), (3, 2, 0, M, 2)]
    q1 = [(7, 0, 0, M, 1), (7, 3, 0, S, 1), (3, 3, 0, M, 9)]
    want = plan(harness, [q0, q1], SEGS, tile=32, use_bq_plan=True)
    got = plan(harness, [q0, q1], SEGS, tile=32, clauses_null=True)
    assert want[0] == 0 and got == want and len(want[3]) == 32 * len(want[2]) and len(want[2]) == 9
    assert all(r[3] == 0 for r in want[2])                                       # clause stays 0, where pad was
    # with clause values: the same items and refs but for the clause field, as long as no clause has an empty member
    grouped = plan(harness, [q0, q1], SEGS, tile=32)
    assert grouped[1] == want[1] and [r[:3] + r[4:] for r in grouped[2]] == [r[:3] + r[4:] for r in want[2]]
    assert [r[3] for r in grouped[2]] == [0, 0, 0, 0, 0, 1, 0, 0, 0]             # segment 7: clause 7 -> 0; segment 3: 1 -> 0, 2 -> 1; q1's 9 -> 0
    # roles == NULL: every ref SHOULD, the clause values are never read
    a, b = plan(harness, [q0, q1], SEGS, roles_null=True), plan(harness, [q0, q1], SEGS, roles_null=True, clauses_null=True)
    assert a[0] == 0 and a == b and all(r[2] == S and r[3] == 0 for r in a[2])


def test_the_refusals_are_bq_plans(harness):
    ok = [(7, 5, 0, M, 1), (3, 2, 8, X, 1)]
    for queries, kw, match in (([[(7, 5, 0, 3, 1)]], {}, "ref 0: role 3 is none of NS_ROLE_SHOULD, NS_ROLE_MUST, NS_ROLE_NOT"),
                               ([ok + [(4, 1, 0, S, 0)]], {}, "ref 2 names segment 4, which the call does not list"),
                               ([[(7, 5, 4, M, 1)]], {}, "ref 0: byte offset 4 is not a multiple of 8"),
                               ([[(7, 5, 8 * 996, M, 1)]], {}, "ref 0 runs past the postings of segment 7"),
                               ([ok], {"n_refs": 1}, "query 0: refs [0, 2) run past the 1 given"),
                               ([ok], {"tile": 48}, "facet tile of 48 documents: not a power of two"),
                               ([ok], {"tile": 1 << 18}, "facet tile of 262144 documents: not a power of two")):
        for clauses_null in (False, True):
            rc, items, refs, _, msg = plan(harness, queries, SEGS, clauses_null=clauses_null, **kw)
            assert rc == NS_E_INVAL and items == [] and refs == [] and match in msg, (msg, match)
    rc, _, _, _, msg = plan(harness, [ok], SEGS + [(7, 5, 5)])
    assert rc == NS_E_INVAL and "seg_id 7 is listed twice" in msg


# ---- the parser ---------------------------------------------------------------------------------------------------------
def test_parse_grouped():
    P = nsbind.parse_grouped
    # a MUST group's tokens share one fresh clause id; ids count up in query order; SHOULD and NOT terms carry 0
    assert P("+(coronavirus covid sars) +(vaccine vaccination) -mouse safety") == [("coronavirus", M, 0), ("covid", M, 0), ("sars", M, 0), ("vaccine", M, 1),
                                                                                  ("vaccination", M, 1), ("mouse", X, 0), ("safety", S, 0)]
    assert P("+alpha +(beta gamma) +delta") == [("alpha", M, 0), ("beta", M, 1), ("gamma", M, 1), ("delta", M, 2)]
    assert P("(a1 b1)") == [("a1", S, 0), ("b1", S, 0)] == P("a1 b1")
    assert P("-(a1 b1)") == [("a1", X, 0), ("b1", X, 0)] == P("-a1 -b1")
    assert P("(a1) -(b1 c1)") == [("a1", S, 0), ("b1", X, 0), ("c1", X, 0)]
    # every other piece follows parse_boolean's rule, each MUST token a clause of its own
    assert P("+covid-19") == [("covid", M, 0), ("19", M, 1)]
    assert P("+(covid-19 sars/cov2)") == [("covid", M, 0), ("19", M, 0), ("sars", M, 0), ("cov2", M, 0)]
    # a missing ')': the body runs to the end of the query
    assert P("+(alpha beta gamma") == [("alpha", M, 0), ("beta", M, 0), ("gamma", M, 0)]
    assert P("alpha +(beta") == [("alpha", S, 0), ("beta", M, 0)] and P("+(") == [] and P("-(") == [] and P("(") == []
    # a body without a token emits nothing and uses no id
    assert P("+()") == [] and P("+() +alpha") == [("alpha", M, 0)]
    assert P("+(the of) +(alpha beta) +( ) +gamma") == [("alpha", M, 0), ("beta", M, 0), ("gamma", M, 1)]
    # scanning resumes right behind the ')'
    assert P("+(alpha beta)gamma") == [("alpha", M, 0), ("beta", M, 0), ("gamma", S, 0)]
    assert P("+(alpha beta)+gamma") == [("alpha", M, 0), ("beta", M, 0), ("gamma", M, 1)]
    assert P("+(alpha)-(beta)(gamma)") == [("alpha", M, 0), ("beta", X, 0), ("gamma", S, 0)]
    # a group across whitespace of every kind
    assert P("+(alpha\nbeta\r\n\tgamma)\ndelta") == [("alpha", M, 0), ("beta", M, 0), ("gamma", M, 0), ("delta", S, 0)]
    # inside a body '+', '-' and '(' are the tokenizer's business; so is a ')' without an open group
    assert P("+(alpha +beta -gamma (delta)") == [("alpha", M, 0), ("beta", M, 0), ("gamma", M, 0), ("delta", M, 0)]
    assert P("alpha) beta") == [("alpha", S, 0), ("beta", S, 0)] and P(") +alpha)") == [("alpha", M, 0)]
    assert P("+(alpha beta) gamma)") == [("alpha", M, 0), ("beta", M, 0), ("gamma", S, 0)]
    assert P("al(pha bx)ta") == [("al", S, 0), ("pha", S, 0), ("bx", S, 0), ("ta", S, 0)]      # '(' inside a piece opens nothing
    assert P("+alpha(beta gamma)") == [("alpha", M, 0), ("beta", M, 1), ("gamma", S, 0)]
    assert P("+ (alpha beta)") == [("alpha", S, 0), ("beta", S, 0)] and P("++(alpha)") == [("alpha", M, 0)]   # only ONE byte is a prefix
    assert P("+(COVID CoronaVirus)") == [("covid", M, 0), ("coronavirus", M, 0)]
    assert P("+(alpha alpha) +(alpha)") == [("alpha", M, 0), ("alpha", M, 0), ("alpha", M, 1)]   # duplicates stay
    # every case of test_parse_boolean: the same words and roles, and every MUST token a clause of its own
    for text in ("+alpha beta -gamma", "covid-19", "+covid-19", "-covid-19 +sars/cov2", "- alpha", "+", "-", "+ -", "--alpha", "-+alpha", "+-alpha", "++alpha",
                 "alpha+beta alpha-beta", "+the +of -and vaccine +a -x +y2", "+COVID -Mouse VacCine", "", "   \t\n ", "-alpha -beta", "alpha alpha +alpha -alpha",
                 "\t+alpha\n-beta\r\ngamma", "+caf\xe9s"):
        got = P(text)
        assert [(w, r) for w, r, _ in got] == nsbind.parse_boolean(text), text
        assert [c for _, r, c in got if r == M] == list(range(sum(r == M for _, r, _ in got))) and all(c == 0 for _, r, c in got if r != M), text


def test_a_host_only_engine_answers_no_grouped_query_and_says_so(tmp_path):
    index = str(tmp_path / "index")
    nsbind.gen_index(index, 2, 45, 512, 77, False)
    eng = nsbind.Engine(index, -1)
    try:
        with pytest.raises(RuntimeError, match="search_grouped_after_batch_flat: no device context"):
            eng.search_grouped_after_batch(["+(t000001 t000002) t000003"], 10)
        with pytest.raises(RuntimeError, match="facet_grouped_batch_flat: no device context"):
            eng.facet_grouped_batch(["+(t000001 t000002) -t000003"], 8)
        with pytest.raises(RuntimeError, match="search_grouped_sorted_batch_flat: no device context"):
            eng.search_grouped_sorted_batch(["+(t000001 t000002)"], 10, order="oldest")
        for name, call in (("search_grouped", eng.search_grouped_json), ("search_grouped_faceted", eng.search_grouped_faceted_json),
                           ("search_grouped_sorted", eng.search_grouped_sorted_json)):
            with pytest.raises(RuntimeError, match=name + ": no device context"):
                call("+(t000001 t000002) -t000003", 10)
            body = call("+(t000001 t000002)", 10, check=False)
            assert body.startswith('{\n  "error": "') and "no device context" in body
        assert nsbind.PAGE_MODES["grouped"] == 5 and nsbind.PAGE_MODES["grouped_sorted"] == 6
        for mode in ("grouped", "grouped_sorted"):
            with pytest.raises(RuntimeError, match="search_page: no device context"):
                eng.search_page_json("+(t000001 t000002)", 10, mode=mode)
    finally:
        eng.close()
