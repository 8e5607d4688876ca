"""Boolean queries, host side (host/boolean.hpp, csrc/ns_boolean_plan.hpp): the restatement
tests/boolean_ref.py pinned to rawseg.reference_multi and to a brute-force loop, the planner through
tests/boolean_plan_harness.cpp, nsx::parse_boolean through the host library, and a host-only engine that says no.  No device is
touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import boolean_ref
import facet_shapes
import nsbind
from boolean_ref import MUST, NOT, SHOULD
from rawseg import avgdl_of, reference_multi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
NS_E_INVAL = -1


# ---- the restatement ----------------------------------------------------------------------------------------------------
def multi_family():
    """facet_shapes' three segments (300, 77, 1000 documents, every list non-empty) plus queries that leave a segment without
    a match (sorted_shapes.multi_family's)"""
    segments, queries = facet_shapes.multi_family()
    return segments, queries + [[(0, 2), (2, 3)], [(1, 1), (1, 1), (0, 0)]]


def weights_of(segments):
    return ([[1.0 + 0.5 * i for i in range(len(s[2]))] for s in segments], [[1.0 if i % 2 else 0.75 for i in range(len(s[2]))] for s in segments])


@pytest.mark.parametrize("role, and_mode", [(SHOULD, False), (MUST, True)])
def test_one_role_for_every_ref_is_the_existing_restatement(role, and_mode):
    """all SHOULD == rawseg.reference_multi's OR answer, all MUST (every list non-empty) == its AND answer: triples, order, bits"""
    segments, queries = multi_family()
    assert all(len(d) for s in segments for d, _ in s[2])
    idfs, weights = weights_of(segments)
    want = reference_multi(segments, queries, idfs, weights)
    got = boolean_ref.boolean_all(segments, [[(s, li, role) for s, li in q] for q in queries], None, idfs, weights)
    sizes = set()
    for qi, (rows, both) in enumerate(zip(got, want)):
        exp = both[1] if and_mode else both[0]
        assert [(s, d) for _, s, d in rows] == [(s, d) for _, s, d in exp], qi
        assert [np.float32(v).view(np.uint32) for v, _, _ in rows] == [np.float32(v).view(np.uint32) for v, _, _ in exp], qi
        sizes.add(len(rows))
    assert 0 in sizes and max(sizes) > 100


def brute(segments, queries, order, idfs, weights):
    """nested loops over documents, no numpy set operation, no code shared with boolean_ref"""
    f32 = np.float32
    out = []
    for q in queries:
        cand = []
        for pos, s in enumerate(order):
            n_docs, doc_len, lists = segments[s]
            named = [(li, r) for ss, li, r in q if ss == s]
            if not named:
                continue
            has = [set(int(x) for x in lists[li][0].tolist()) for li, _ in named]
            avgdl = f32(avgdl_of(np.asarray(doc_len, np.uint32)))
            any_must = any(r == MUST for _, r in named)
            for d in range(n_docs):
                if any(r == NOT and d in h for (_, r), h in zip(named, has)):
                    continue
                if any_must:
                    ok = all(d in h for (_, r), h in zip(named, has) if r == MUST)
                else:
                    ok = any(d in h for (_, r), h in zip(named, has) if r == SHOULD)
                if not ok:
                    continue
                acc = f32(0.0)
                for li, r in named:
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


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_restatement_equals_a_brute_force_loop(seed):
    rng = np.random.default_rng(seed)
    segments, idfs, weights = [], [], []
    for n in (23, 9, 40):
        lists = []
        for m in list(rng.integers(1, n + 1, 4)) + [0]:
            d = np.sort(rng.choice(n, int(m), replace=False)).astype(np.uint32)
            lists.append((d, rng.integers(1, 4, len(d)).astype(np.uint32)))
        lists.append((np.array([1, n - 1, n + 3], np.uint32), np.array([2, 2, 2], np.uint32)))       # a posting >= n_docs
        segments.append((n, np.full(n, 7, np.uint32) if n == 9 else rng.integers(3, 50, n).astype(np.uint32), lists))   # equal lengths: ties
        idfs.append([float(x) for x in rng.uniform(0.5, 4.0, 6)])
        weights.append([1.0, 0.5, 1.0, 0.25, 1.0, -0.5])
    S, M, X = SHOULD, MUST, NOT
    queries = [[], [(0, 0, S)], [(0, 0, M)], [(0, 0, X)], [(0, 1, S), (0, 2, S)], [(0, 1, M), (0, 2, M)], [(0, 1, M), (0, 2, S)], [(0, 1, S), (0, 2, X)],
               [(0, 1, M), (0, 1, X)], [(0, 1, S), (0, 1, S)], [(0, 1, S), (0, 1, X)], [(0, 0, M), (0, 4, M)], [(0, 0, S), (0, 4, S)], [(0, 0, S), (0, 4, X)],
               [(1, 0, S), (1, 1, S), (1, 2, X), (1, 3, M)], [(0, 0, S), (1, 1, M), (2, 2, X), (2, 3, S), (1, 0, S), (0, 5, S)],
               [(2, 0, M), (2, 1, M), (2, 2, M), (2, 3, X), (2, 5, S)], [(1, 4, X), (1, 0, X)], [(0, 3, M), (2, 1, X), (0, 0, S), (2, 2, S), (1, 5, M)]]
    for order in ([0, 1, 2], [2, 0, 1]):
        got = boolean_ref.boolean_all(segments, queries, order, idfs, weights)
        want = brute(segments, queries, order, idfs, weights)
        for qi, (g, w) in enumerate(zip(got, want)):
            assert [(s, d) for _, s, d in g] == [(s, d) for _, s, d in w], (order, qi)
            assert [np.float32(x).view(np.uint32) for x, _, _ in g] == [np.float32(x).view(np.uint32) for x, _, _ in w], (order, qi)
        assert got[3] == [] and got[8] == [] and got[11] == [] and got[17] == []     # NOT alone, MUST == NOT, MUST of an empty list, NOTs alone
        for k in (1, 5, 100):
            for (found, hits), rows in zip(boolean_ref.boolean_hits(segments, queries, k, order, idfs, weights), got):
                assert found == len(rows) and hits == rows[:k]


def test_the_gpu_suites_equivalence_inputs_clear_their_floors():
    """tests/test_boolean_gpu.py compares whole answers with the scoring path and asserts how many queries had found >= 2: the
    chosen inputs have that many, by the restatement"""
    import boolean_shapes
    for role in (SHOULD, MUST):
        segments, queries, idfs, weights = boolean_shapes.same_role_inputs(role)
        founds = [len(rows) for rows in boolean_ref.boolean_all(segments, queries, None, idfs, weights)]
        assert sum(f >= 2 for f in founds) >= boolean_shapes.FLOOR_SAME_ROLE[role], (role, founds)
    segments, queries, idfs, weights = boolean_shapes.excluding_inputs()
    founds = [len(rows) for rows in boolean_ref.boolean_all(segments, queries, None, idfs, weights)]
    assert sum(f >= 2 for f in founds) >= boolean_shapes.FLOOR_EXCLUDED and 0 in founds, founds
    for k in (64, 65, 100):                                                   # found == K - 1, K, K + 1 through every role
        assert {k - 1, k, k + 1} <= set(boolean_shapes.COUNT_SIZES)


# ---- the planner --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("boolean_plan") / "boolean_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "boolean_plan_harness.cpp")], check=True)
    lib = C.CDLL(so)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.boolean_plan.argtypes = [vp, u32, vp, vp, u32, vp, vp, vp, u32, u32, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64), vp, C.c_char_p, u32]
    for name in ("boolean_win_docs", "boolean_max_win_docs", "boolean_tile_docs", "boolean_role"):
        getattr(lib, name).restype = u32
    lib.boolean_win_ok.argtypes = [u32]
    lib.boolean_role.argtypes = [C.c_int]
    return lib


def plan(harness, queries, segs, tile=32, roles_null=False, n_refs=None, qd=None):
    """queries: per query [(seg_id, count, byte_off, role)] (idf = 1 + ref index, qweight 0.5); segs: [(seg_id, n_docs,
    n_postings)] -> (rc, items as rows of 6, planned refs as rows of (first, count, role, idf, qweight), q_off, message)"""
    flat = [r for q in queries for r in q]
    refs = np.array([(s, c, o, 1.0 + i, 0.5) for i, (s, c, o, _) in enumerate(flat)], dtype=nsbind.TERM_DTYPE) if flat else np.zeros(0, nsbind.TERM_DTYPE)
    roles = np.array([r for _, _, _, r in flat] + [0], dtype=np.uint8)
    if qd is None:
        qd, at = [], 0
        for q in queries:
            qd += [at, len(q)]
            at += len(q)
    qd = np.array(qd + [0, 0], dtype=np.uint32)
    ids, docs, posts = (np.array([s[i] for s in segs] + [0], dtype=t) for i, t in ((0, np.uint32), (1, np.uint32), (2, np.uint64)))
    cap_i, cap_r = 4096, len(flat) + 1
    items, pref, q_off = np.zeros((cap_i, 6), np.uint32), np.zeros((cap_r, 4), np.uint64), np.zeros(len(queries) + 2, np.uint32)
    ni, nr = C.c_uint64(), C.c_uint64()
    err = C.create_string_buffer(256)
    rc = harness.boolean_plan(qd.ctypes.data, len(queries), refs.ctypes.data if len(refs) else None, None if roles_null else roles.ctypes.data,
                              len(flat) if n_refs is None else n_refs, ids.ctypes.data, docs.ctypes.data, posts.ctypes.data, len(segs), tile,
                              items.ctypes.data, cap_i, C.byref(ni), pref.ctypes.data, cap_r, C.byref(nr), q_off.ctypes.data, err, len(err))
    assert ni.value <= cap_i and nr.value <= cap_r
    planned = [(int(f), int(c), int(r), float(np.array([w & 0xFFFFFFFF], np.uint32).view(np.float32)[0]), float(np.array([w >> 32], np.uint32).view(np.float32)[0]))
               for f, c, r, w in pref[: nr.value].tolist()]
    return rc, items[: ni.value].tolist(), planned, q_off[: len(queries) + 1].tolist(), err.value.decode()


def test_the_constants(harness):
    assert [harness.boolean_role(i) for i in range(3)] == [nsbind.NS_ROLE_SHOULD, nsbind.NS_ROLE_MUST, nsbind.NS_ROLE_NOT] == [SHOULD, MUST, NOT] == [0, 1, 2]
    win, tile = harness.boolean_win_docs(), harness.boolean_tile_docs()
    assert tile == 1 << 17 and win in (1 << 13, 1 << 14) and tile % win == 0
    # the window's LDS: accumulators, three bitmaps, the row exchange; four workgroups fit a CU's 160 KiB at the product value
    assert 4 * (win * 4 + 3 * win // 8 + 4096 + 16) <= 160 << 10 or win == 1 << 14
    assert harness.boolean_max_win_docs() * 4 + 3 * harness.boolean_max_win_docs() // 8 + 4096 + 16 <= 160 << 10
    assert [harness.boolean_win_ok(w) for w in (0, 16, 32, 48, 64, 1 << 13, 1 << 15, 1 << 16)] == [0, 0, 1, 0, 1, 1, 1, 0]


def test_groups_by_segment_position_in_query_order_with_roles(harness):
    segs = [(7, 100, 1000), (3, 50, 1000), (9, 10, 1000)]            # positions 0, 1, 2 carry the ids 7, 3, 9
    q = [(3, 5, 80, MUST), (7, 6, 0, SHOULD), (9, 2, 160, NOT), (3, 4, 240, SHOULD), (7, 1, 400, NOT), (9, 3, 480, SHOULD), (7, 6, 0, SHOULD)]
    rc, items, refs, q_off, msg = plan(harness, [q], segs, tile=128)
    assert rc == 0, msg
    assert items == [[0, 0, 0, 3, 0, 100], [0, 1, 3, 2, 0, 50], [0, 2, 5, 2, 0, 10]]
    # (first posting, count, role, idf = 1 + ref index, qweight): query order inside every group, duplicates kept
    assert refs == [(0, 6, SHOULD, 2.0, 0.5), (50, 1, NOT, 5.0, 0.5), (0, 6, SHOULD, 7.0, 0.5),
                    (10, 5, MUST, 1.0, 0.5), (30, 4, SHOULD, 4.0, 0.5),
                    (20, 2, NOT, 3.0, 0.5), (60, 3, SHOULD, 6.0, 0.5)]
    assert q_off == [0, 3]
    rc, items2, refs2, _, _ = plan(harness, [q], segs, tile=128, roles_null=True)             # NULL: every ref SHOULD
    assert rc == 0 and items2 == items and [r[2] for r in refs2] == [SHOULD] * 7


def test_dead_groups_dropped_refs_and_groups_without_a_positive_ref(harness):
    segs = [(0, 40, 1000), (1, 40, 1000), (2, 40, 1000), (3, 0, 1000)]
    queries = [
        [(0, 3, 0, SHOULD), (0, 0, 0, MUST)],                        # a MUST ref without postings kills the group
        [(0, 0, 0, SHOULD), (0, 3, 0, SHOULD), (0, 0, 8, NOT)],       # empty SHOULD / NOT refs are dropped
        [(0, 3, 0, NOT), (0, 2, 24, NOT)],                           # NOT refs alone: no item
        [(0, 0, 0, SHOULD), (0, 3, 0, NOT)],                         # the only positive ref is empty: no item
        [(0, 3, 0, MUST), (1, 0, 0, MUST), (2, 3, 0, NOT), (1, 5, 0, SHOULD), (2, 1, 0, SHOULD)],   # segment 1 dead, 0 and 2 alive
        [],
        [(3, 3, 0, SHOULD)],                                         # a segment without documents
        [(0, 0, 0, MUST), (0, 0, 0, NOT)],
    ]
    rc, items, refs, q_off, msg = plan(harness, queries, segs, tile=64)
    assert rc == 0, msg
    assert items == [[1, 0, 0, 1, 0, 40], [4, 0, 1, 1, 0, 40], [4, 2, 2, 2, 0, 40]]
    assert [r[:3] for r in refs] == [(0, 3, SHOULD), (0, 3, MUST), (0, 3, NOT), (0, 1, SHOULD)]
    assert q_off == [0, 0, 1, 1, 1, 3, 3, 3, 3]                      # sd_query_items holds: contiguous, in query order


def test_tile_cuts(harness):
    tile = 64
    sizes = [1, tile - 1, tile, tile + 1, 2 * tile + 5]
    segs = [(i, n, 100) for i, n in enumerate(sizes)]
    queries = [[(i, 4, 0, MUST), (i, 2, 32, NOT)] for i in range(len(sizes))] + [[(i, 4, 0, SHOULD) for i in (4, 0, 3)]]
    rc, items, refs, q_off, msg = plan(harness, queries, segs, tile=tile)
    assert rc == 0, msg
    want = []
    for q, n in enumerate(sizes):
        want += [[q, q, 2 * q, 2, lo, min(lo + tile, n)] for lo in range(0, n, tile)]
    at = 2 * len(sizes)
    for pos in (0, 3, 4):                                            # by position, not in the order the query names them
        want += [[5, pos, at, 1, lo, min(lo + tile, sizes[pos])] for lo in range(0, sizes[pos], tile)]
        at += 1
    assert items == want
    assert [b - a for a, b in zip(q_off, q_off[1:])] == [1, 1, 1, 2, 3, 1 + 2 + 3]
    for q in range(len(queries)):
        assert all(it[0] == q for it in items[q_off[q]:q_off[q + 1]])


def test_every_refusal_has_its_message_and_leaves_nothing(harness):
    segs = [(0, 40, 10), (1, 40, 10)]
    ok = [[(0, 3, 0, MUST), (1, 2, 16, NOT)]]
    cases = [
        (dict(queries=[[(0, 3, 0, MUST), (1, 2, 16, 3)]], segs=segs), "ref 1: role 3 is none of NS_ROLE_SHOULD, NS_ROLE_MUST, NS_ROLE_NOT"),
        (dict(queries=[[(0, 3, 0, MUST), (5, 2, 16, NOT)]], segs=segs), "ref 1 names segment 5, which the call does not list"),
        (dict(queries=ok, segs=[(0, 40, 10), (0, 40, 10)]), "seg_id 0 is listed twice"),
        (dict(queries=[[(0, 3, 4, SHOULD)]], segs=segs), "ref 0: byte offset 4 is not a multiple of 8"),
        (dict(queries=[[(0, 3, 64, SHOULD)]], segs=segs), "ref 0 runs past the postings of segment 0"),
        (dict(queries=[[(0, 11, 0, NOT)]], segs=segs), "ref 0 runs past the postings of segment 0"),
        (dict(queries=ok, segs=segs, qd=[1, 2]), "query 0: refs [1, 3) run past the 2 given"),
        (dict(queries=ok, segs=segs, tile=48), "facet tile of 48 documents: not a power of two in [32, 131072]"),
    ]
    for kw, text in cases:
        rc, items, refs, _, msg = plan(harness, **kw)
        assert rc == NS_E_INVAL and msg == text and items == [] and refs == [], (text, msg)
    assert plan(harness, ok, segs)[0] == 0


def test_a_scoring_ref_must_have_finite_numbers(harness):
    """a NaN or infinite idf / qweight of a MUST or SHOULD ref is refused; under NOT it is never read; negative values and -0.0
    are taken"""
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    ids, docs, posts = np.array([0], np.uint32), np.array([40], np.uint32), np.array([10], np.uint64)
    qd = np.array([0, 1], np.uint32)
    out = dict(items=np.zeros((8, 6), np.uint32), refs=np.zeros((8, 4), np.uint64), q_off=np.zeros(4, np.uint32))

    def one(idf, qw, role):
        refs = np.array([(0, 3, 0, idf, qw)], dtype=nsbind.TERM_DTYPE)
        roles = np.array([role], np.uint8)
        ni, nr, err = u64(), u64(), C.create_string_buffer(256)
        rc = harness.boolean_plan(qd.ctypes.data, 1, refs.ctypes.data, roles.ctypes.data, 1, ids.ctypes.data, docs.ctypes.data, posts.ctypes.data, 1, 32,
                                  out["items"].ctypes.data, 8, C.byref(ni), out["refs"].ctypes.data, 8, C.byref(nr), out["q_off"].ctypes.data, err, 256)
        return rc, err.value.decode(), ni.value

    for role in (SHOULD, MUST):
        for idf, qw in ((np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, -np.inf)):
            assert one(idf, qw, role) == (NS_E_INVAL, "ref 0: idf or qweight is not finite", 0)
        for idf, qw in ((-1.5, 1.0), (1.0, -0.0), (-0.0, -0.0), (3.0e38, 3.0e38)):
            assert one(idf, qw, role)[0] == 0
    assert one(np.nan, np.inf, NOT) == (0, "", 0)                     # planned away: a NOT ref alone has no item


# ---- the parser ---------------------------------------------------------------------------------------------------------
def test_parse_boolean():
    S, M, X = SHOULD, MUST, NOT
    P = nsbind.parse_boolean
    assert P("+alpha beta -gamma") == [("alpha", M), ("beta", S), ("gamma", X)]
    assert P("covid-19") == [("covid", S), ("19", S)]                 # a '-' inside a piece is the tokenizer's
    assert P("+covid-19") == [("covid", M), ("19", M)]                # the prefix holds for every token of the piece
    assert P("-covid-19 +sars/cov2") == [("covid", X), ("19", X), ("sars", M), ("cov2", M)]
    assert P("- alpha") == [("alpha", S)]                             # a lone prefix says nothing
    assert P("+") == [] and P("-") == [] and P("+ -") == []
    assert P("--alpha") == [("alpha", X)] and P("-+alpha") == [("alpha", X)] and P("+-alpha") == [("alpha", M)] and P("++alpha") == [("alpha", M)]
    assert P("alpha+beta alpha-beta") == [("alpha", S), ("beta", S), ("alpha", S), ("beta", S)]
    assert P("+the +of -and vaccine +a -x +y2") == [("vaccine", S), ("y2", M)]          # stop words and one-byte tokens go, under a prefix too
    assert P("+COVID -Mouse VacCine") == [("covid", M), ("mouse", X), ("vaccine", S)]
    assert P("") == [] and P("   \t\n ") == []
    assert P("-alpha -beta") == [("alpha", X), ("beta", X)]
    assert P("alpha alpha +alpha -alpha") == [("alpha", S), ("alpha", S), ("alpha", M), ("alpha", X)]   # duplicates stay
    assert P("\t+alpha\n-beta\r\ngamma") == [("alpha", M), ("beta", X), ("gamma", S)]
    assert P("+caf\xe9s") == [("caf", M)]                             # bytes >= 0x80 split tokens, as in search ("s" is one byte)
    for text in ("+alpha beta -gamma", "covid-19 the vaccine", "-alpha"):               # without prefixes it is search's tokenizer
        plain = text.replace("+", " ").replace("-", " ")
        L = nsbind.host_lib()
        buf = C.create_string_buffer(256)
        n = L.nsh_base_terms(plain.encode(), buf, 256)
        assert [w for w, _ in P(text)] == (buf.value.decode().split(" ") if n else [])


def test_a_host_only_engine_answers_no_boolean_query_and_says_so(tmp_path):
    index = str(tmp_path / "index")
    nsbind.gen_index(index, 2, 45, 512, 77, False)
    eng = nsbind.Engine(index, -1)
    try:
        with pytest.raises(RuntimeError, match="no device context"):
            eng.search_boolean_batch(["+t000001 t000002"], 10)
        with pytest.raises(RuntimeError, match="no device context"):
            eng.search_boolean_json("+t000001", 10)
        body = eng.search_boolean_json("t000001 -t000002", 10, check=False)
        assert body.startswith('{\n  "error": "') and "no device context" in body
    finally:
        eng.close()
