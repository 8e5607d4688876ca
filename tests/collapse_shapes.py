"""Directed inputs of ns_search_collapsed (the COLLAPSE instantiations of k_bq_select, k_bq_join_collapsed and k_cl_count;
DESIGN.md §5ac) and the code that runs them through the raw C-ABI against the restatement (tests/collapse_ref.py over
tests/boost_ref.py over tests/quorum_ref.py).  The segments, lists, queries and factor tables are tests/boost_shapes.py's (300
documents per raw segment, one segment, two, or three listed as 2, 0, 1); this file adds the key laws, one uint32 per document,
each built for the properties it is named after.  check_properties asserts those properties on the restatement's own answer, so a
law that lost its point fails before any kernel runs (tests/test_collapse_cpu.py calls it without a GPU).  All comparisons are
exact.

Imported by tests/test_collapse_gpu.py for the product library (one tile and one window hold a 300-document segment: its ten
bitmap words are ten lanes of ONE round of the sweep, so documents d and d + 32 meet in a round), and run as a program in a child
process that loaded the variants or the counting build with NS_FACET_TILE_DOCS=128 NS_BOOL_WIN_DOCS=32: there 300 documents are two
whole tiles and a part, four windows each, and the members of a group lie in different windows, tiles and segments (a window is
one bitmap word there, so a round of the sweep carries one candidate).  A second family of a few thousand documents (the
randomised one) is run at tiles and windows of 4096 documents as well, where two waves of a workgroup each sweep a part of a
window with all 64 lanes."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "nextsearch-api_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import boost_ref  # noqa: E402
import boost_shapes  # noqa: E402
import collapse_ref  # noqa: E402
import filter_ref  # noqa: E402
import nsbind  # noqa: E402
import quorum_ref  # noqa: E402
from boolean_ref import MUST, NOT, SHOULD  # noqa: E402

NS_E_INVAL = -1
SMALL_TILE, SMALL_WIN, N_DOCS = boost_shapes.SMALL_TILE, boost_shapes.SMALL_WIN, boost_shapes.N_DOCS
MID = 4096                                    # tile and window of the randomised family in the test builds
KS = [1, 10, 64, 65, 100]                     # 64 / 65: the boundary between the kept set's two registers
S, M, X = SHOULD, MUST, NOT
EVENTS = nsbind.COLLAPSE_EVENTS               # ns_debug_collapse_counters, in order (counting build)
ALL, EDGE, NEG, P1, P2, A, B, C, NOTL, INV = range(10)

# boost_shapes' queries, and the "boolean" one without its exclusion: what the NOT ref takes away shows against it
CASES = dict(boost_shapes.CASES)
CASES["boolean, no exclusion"] = [r for r in CASES["boolean"] if r[1] != X]
DIRECTED = [[]] + list(CASES.values())
NAMES = ["no ref"] + list(CASES)
TABLES = ["ones", "zeros", "rough"]           # factor tables of boost_shapes.tables_for that the laws run under ("lift" is added here)
LIFT_A, LIFT_B = 7, 255                       # "lift": the pair of the law "pair"; 255 = 7 * 32 + 31 is swept late and boosted to the top


def directed_inputs(n_segs):
    segments, queries, idfs, weights, order = boost_shapes.directed_inputs(n_segs, cases=DIRECTED)
    if n_segs == 2:
        order = [1, 0]
    return segments, queries, idfs, weights, order


def laws_for(n_segs):
    """name -> one uint32 key per document and segment (indexed by segment number)"""
    d = np.arange(N_DOCS, dtype=np.uint32)
    u = np.uint32
    out = {
        "zeros": [np.zeros(N_DOCS, u) for _ in range(n_segs)],
        "distinct": [(1 + s * N_DOCS + d).astype(u) for s in range(n_segs)],
        "one": [np.full(N_DOCS, 7, u) for _ in range(n_segs)],
        # 7 groups over every window, tile and segment: fewer groups than K although found > K
        "mod7": [(1 + d % 7).astype(u) for _ in range(n_segs)],
        # d, d + 32, d + 64, ...: at product size all members of a group meet in ONE round of the sweep
        "mod32": [(1 + d % 32).astype(u) for _ in range(n_segs)],
        # 150 groups of 2 per segment, more than K: a group pushed out comes back with a better member
        "mod150": [(1 + (d * 7) % 150).astype(u) for _ in range(n_segs)],
        # two documents in three stand alone; the rest form 9 groups
        "sparse": [np.where(d % 3 != 0, 0, 1 + (d // 3) % 9).astype(u) for _ in range(n_segs)],
        # the smallest and the largest legal key, and no key
        "extremes": [np.where(d % 5 == 0, 0, np.where(d % 2 == 0, 1, 0xFFFFFFFE)).astype(u) for _ in range(n_segs)],
        # groups that do not span segments
        "per segment": [(1 + 1000 * s + d % 5).astype(u) for s in range(n_segs)],
        # every document a key of its own but one pair
        "pair": [(1 + s * N_DOCS + d).astype(u) for s in range(n_segs)],
    }
    for s in range(n_segs):
        out["pair"][s][LIFT_B] = out["pair"][s][LIFT_A]
    return out


LAWS = ["zeros", "distinct", "one", "mod7", "mod32", "mod150", "sparse", "extremes", "per segment", "pair"]


def with_lift(tables, n_segs):
    """boost_shapes' factor tables + "lift": 1.0f but for LIFT_B, which a factor of 64 puts in front of everything"""
    tables = dict(tables)
    tables["lift"] = [np.ones(N_DOCS, np.float32) for _ in range(n_segs)]
    for t in tables["lift"]:
        t[LIFT_B] = 64.0
    return tables


def windows_of(doc):
    return doc // SMALL_WIN, doc // SMALL_TILE


def check_properties(everything, tables, order):
    """what each law exists for, asserted on the restatement's own answer -> {(law, table): per query collapse_rows}"""
    order = list(order)
    n_segs = len(order)
    laws = laws_for(n_segs)
    q_of = NAMES.index
    rows_of = {t: boost_ref.boosted_rows(everything, tables[t], order) for t in TABLES + ["lift"]}
    whole = {(law, t): [collapse_ref.collapse_rows(rows, laws[law]) for rows in rows_of[t]] for law in LAWS for t in TABLES + ["lift"]}
    dense = q_of("dense")

    def members(law, t, q):
        """group -> its matched documents as rows, in the uncollapsed order"""
        out = {}
        for r in rows_of[t][q]:
            g = int(laws[law][r[3]][r[2]])
            if g:
                out.setdefault(g, []).append(r)
        return out

    for (law, t), per_query in whole.items():
        for q, coll in enumerate(per_query):
            rows = rows_of[t][q]
            kept = [r for r, _, _ in coll]
            # a subsequence of the uncollapsed ranking, every group once, its first member; the identities of nhits and others
            it = iter(rows)
            assert all(any(r is x for x in it) for r in kept), (law, t, q)
            gs = [g for _, g, _ in coll if g]
            assert len(gs) == len(set(gs)) and len(coll) == collapse_ref.distinct_total(rows, laws[law])
            assert sum(o + 1 for _, _, o in coll) == len(rows)
            mem = members(law, t, q)
            assert all(mem[g][0] is r and o == len(mem[g]) - 1 for r, g, o in coll if g) and all(o == 0 for _, g, o in coll if not g)
    for t in TABLES:
        for q in range(len(NAMES)):
            # all zero and all distinct: the uncollapsed ranking; one key: its first row alone, others = found - 1
            for law in ("zeros", "distinct"):
                assert [r for r, _, _ in whole[(law, t)][q]] == rows_of[t][q] and all(o == 0 for _, _, o in whole[(law, t)][q])
            one = whole[("one", t)][q]
            assert len(one) == min(1, len(rows_of[t][q])) and all(r is rows_of[t][q][0] and o == len(rows_of[t][q]) - 1 for r, _, o in one)
    # replacement and drop: a group whose best member lies in a LATER window (tile) than a worse one, and one where it lies earlier
    for law in ("mod7", "mod32", "mod150"):
        mem = members(law, "rough", dense)
        later_w = sum(1 for ms in mem.values() if any(m[3] == ms[0][3] and windows_of(m[2])[0] < windows_of(ms[0][2])[0] for m in ms[1:]))
        earlier_w = sum(1 for ms in mem.values() if any(m[3] == ms[0][3] and windows_of(m[2])[0] > windows_of(ms[0][2])[0] for m in ms[1:]))
        later_t = sum(1 for ms in mem.values() if any(m[3] == ms[0][3] and windows_of(m[2])[1] < windows_of(ms[0][2])[1] for m in ms[1:]))
        assert later_w >= 3 and earlier_w >= 3 and later_t >= 2, (law, later_w, earlier_w, later_t)
    # two and three members of one group in one round of 64 lanes at product size: documents d and d + 32 (and d + 64) of a segment
    mem = members("mod32", "rough", dense)
    assert all(len({m[2] % 32 for m in ms}) == 1 and sum(1 for m in ms if m[3] == order[0]) >= 3 for ms in mem.values()) and len(mem) == 32
    mem = members("mod7", "rough", dense)
    assert any(sum(1 for m in ms if m[3] == order[0] and m[2] % 32 == ms[0][2] % 32) == 2 for ms in mem.values())
    # members in different tiles of a segment, and in two and three segments
    assert all(len({windows_of(m[2])[1] for m in ms if m[3] == order[0]}) == 3 for ms in mem.values())
    assert all(len({m[3] for m in ms}) == n_segs for ms in mem.values())
    assert all(len({m[3] for m in ms}) == 1 for ms in members("per segment", "rough", dense).values()) and len(members("per segment", "rough", dense)) == 5 * n_segs
    if n_segs > 1:   # a group's representative is not always in the first listed segment
        assert len({r[3] for r, g, _ in whole[("mod7", "rough")][dense]}) > 1
    # more groups than K: the hits are cut at K, and a hit group's member of the lowest docId is often not the one that represents it
    coll = whole[("mod150", "rough")][dense]
    assert len(coll) == 150 and sum(1 for r, g, _ in coll[:100] if min(m[2] for m in members("mod150", "rough", dense)[g] if m[3] == r[3]) != r[2]) >= 20
    # fewer groups than K although found > K: nhits < K and a padded tail
    assert len(whole[("mod7", "rough")][dense]) == 7 and len(rows_of["rough"][dense]) > 100
    # many key-0 documents that do not collapse, among groups
    coll = whole[("sparse", "rough")][dense]
    assert sum(1 for _, g, _ in coll if not g) == n_segs * 200 and sum(1 for _, g, _ in coll if g) == 9 and sum(1 for _, g, _ in coll[:100] if not g) >= 50
    # keys 1 and 0xFFFFFFFE
    coll = whole[("extremes", "rough")][dense]
    assert {g for _, g, _ in coll} == {0, 1, 0xFFFFFFFE} and {g for _, g, _ in coll[:10]} >= {1, 0xFFFFFFFE}
    # equal score bits within a group and between groups: under factors of 0.0f every product is +0.0f, and the representative is the
    # member of the lowest (segment position, docId)
    coll = whole[("mod7", "zeros")][dense]
    assert {r[4] for r in rows_of["zeros"][dense]} == {0} and [(r[1], r[2]) for r, _, _ in coll] == [(0, i) for i in range(7)]
    assert [o for _, _, o in coll] == [len(members("mod7", "zeros", dense)[1 + i]) - 1 for i in range(7)]
    # a factor table that changes which member represents a group, and (at K = 100, product size, one segment) lifts the group's
    # entry from a slot >= 64 to the front: without the factor LIFT_A represents the pair from a rank in [64, 100)
    for s in order:
        plain = [r for r, _, _ in whole[("pair", "ones")][dense] if r[3] == s]
        assert LIFT_A in [r[2] for r in plain] and LIFT_B not in [r[2] for r in plain]
        lifted = whole[("pair", "lift")][dense]
        assert LIFT_B in [r[2] for r, _, _ in lifted[:n_segs] if r[3] == s] and all(not (r[3] == s and r[2] == LIFT_A) for r, _, _ in lifted)
    if n_segs == 1:
        without_b = [r for r in rows_of["lift"][dense] if r[2] != LIFT_B]
        assert 64 <= [r[2] for r in without_b].index(LIFT_A) < 100 and LIFT_B % 32 == 31 and LIFT_A % 32 < 31
    # a NOT ref removes a group's best member: the next member represents it, and others drops by one
    law, seen = "mod7", 0
    with_x, without_x = whole[(law, "rough")][q_of("boolean")], whole[(law, "rough")][q_of("boolean, no exclusion")]
    for r, g, o in without_x:
        here = [(r2, o2) for r2, g2, o2 in with_x if g2 == g]
        gone = (r[3], r[2]) not in {(x[3], x[2]) for x in rows_of["rough"][q_of("boolean")]}
        if gone and here and here[0][0][2] != r[2]:
            seen += 1
            lost = sum(1 for m in members(law, "rough", q_of("boolean, no exclusion"))[g] if (m[3], m[2]) not in {(x[3], x[2]) for x in rows_of["rough"][q_of("boolean")]})
            assert here[0][1] == o - lost and lost >= 1
    assert seen >= 1, "no group lost its representative to the exclusion"
    # every dialect form matches something that collapses; a query whose hits are all key 0; a hit group with no other member
    for name in ("dense", "all optional", "required edges of the dense list", "grouped", "quorum: two of three"):
        coll = whole[("mod32" if name.startswith("quorum") else "mod7", "rough")][q_of(name)]
        assert any(o > 0 for _, _, o in coll) and len(coll) < len(rows_of["rough"][q_of(name)]), name
    assert all(g == 0 for _, g, _ in whole[("zeros", "rough")][dense])
    assert any(g and o == 0 for _, g, o in whole[("pair", "ones")][dense]) and any(o == 1 for _, g, o in whole[("pair", "ones")][dense])
    assert not whole[("mod7", "rough")][q_of("nothing matches")] and not whole[("mod7", "rough")][q_of("no ref")]
    return whole


class Family(boost_shapes.Family):
    """boost_shapes.Family + the key laws, uploaded as ns_dockeys tables when a call first asks for them"""

    def __init__(self, segments, queries, idfs, weights, seg_order=None, tables=None, laws=None):
        super().__init__(segments, queries, idfs, weights, seg_order, tables=tables)
        n_segs = len(segments)
        if tables is None:
            self.tables = with_lift(self.tables, n_segs)
        self.laws = laws_for(n_segs) if laws is None else laws
        self._groups = {}

    def groups(self, law):
        """the ns_dockeys handles of a law, in the call's segment order"""
        if law not in self._groups:
            hs = []
            for s in self.order:
                rc, h = nsbind.dockeys_upload(self.segs.ctx, self.laws[law][s])
                assert rc == 0, self.segs.err()
                hs.append(h)
            self._groups[law] = hs
        return self._groups[law]

    def collapsed(self, law, table, k, others=True, roles="own", clauses="own", needs="own", queries=None, groups="own"):
        """ns_search_collapsed under a law and a factor table (None: boosts == NULL) -> nsbind.search_collapsed_raw's tuple"""
        qd = self.qd if queries is None else self.qd[list(queries)]
        return nsbind.search_collapsed_raw(self.segs.ctx, qd, self.refs, self.roles if isinstance(roles, str) else roles,
                                           self.clauses if isinstance(clauses, str) else clauses, self.needs if isinstance(needs, str) else needs, k, self.order,
                                           self.handles, None if table is None else self.boosts(table), self.groups(law) if isinstance(groups, str) else groups,
                                           others=others)

    def want(self, law, table, k, queries=None):
        rows = self.rows("ones" if table is None else table)
        return collapse_ref.collapsed(rows if queries is None else [rows[q] for q in queries], self.laws[law], k)

    def check(self, label, law, table, k, **kw):
        out = self.collapsed(law, table, k, **kw)
        assert out[0] == 0, (label, self.segs.err())
        collapse_ref.check((label, law, table), self.want(law, table, k, kw.get("queries")), *out[1:6], k)
        return out

    def sibling(self, table, k, roles="own", clauses="own", needs="own", queries=None):
        qd = self.qd if queries is None else self.qd[list(queries)]
        return nsbind.search_boosted_after_raw(self.segs.ctx, qd, self.refs, self.roles if isinstance(roles, str) else roles,
                                               self.clauses if isinstance(clauses, str) else clauses, self.needs if isinstance(needs, str) else needs, k, None,
                                               self.order, self.handles, None if table is None else self.boosts(table))

    def release(self):
        if self.segs.ctx:
            for hs in self._groups.values():
                for h in hs:
                    assert nsbind.dockeys_release(self.segs.ctx, h) == 0
            self._groups = {}
        super().release()


def directed_family(n_segs):
    segments, queries, idfs, weights, order = directed_inputs(n_segs)
    return Family(segments, queries, idfs, weights, seg_order=order)


# (law, factor table or None for boosts == NULL) pairs of the directed runs
PAIRS = [("mod7", "rough"), ("mod7", "zeros"), ("mod32", "rough"), ("mod150", "rough"), ("sparse", "rough"), ("extremes", None), ("per segment", "ones"),
         ("pair", "lift"), ("pair", None), ("mod150", None)]


def run_directed(n_segs, tile_expected=None, ks=KS, pairs=PAIRS):
    """every directed query under the (law, table) pairs at K = 1, 10, 64, 65 and 100, against the restatement; K = 10 once more
    without the count pass"""
    tile = nsbind.facet_tile_docs()
    if tile_expected is not None:
        assert tile == tile_expected, (tile, tile_expected)
    fam = directed_family(n_segs)
    try:
        check_properties(fam.everything, fam.tables, fam.order)
        for law, table in pairs:
            for k in ks:
                fam.check(("collapse directed", n_segs), law, table, k)
            out = fam.check(("collapse directed, no others", n_segs), law, table, 10, others=False)
            assert out[3] is None
    finally:
        fam.release()
    return tile


def same_as_sibling(label, got, want):
    """hits, nhits and found of a collapsed call against ns_search_boosted_after(after = NULL)'s, byte for byte"""
    assert got[0] == 0 and want[0] == 0, label
    assert got[1].tobytes() == want[1].tobytes(), (label, "hits")
    assert got[4].tobytes() == want[2].tobytes(), (label, "nhits")
    assert got[5].tobytes() == want[3].tobytes(), (label, "found")


def run_sibling_identities(n_segs=3):
    """all-zero tables and all-distinct tables give the sibling's bytes through the collapsing kernels (others all 0); one key on
    every document gives one hit per query, the sibling's first, with others = found - 1; for every dialect form, without and with
    factor tables"""
    fam = directed_family(n_segs)
    try:
        forms = [("own", "own", "own", None)] + [(ro, cl, ne, [NAMES.index(n) for n in names]) for names, (ro, cl, ne) in boost_shapes.NULL_FORMS.values()]
        checked = 0
        for ro, cl, ne, qs in forms:
            kw = dict(roles=ro, clauses=cl, needs=ne, queries=qs)
            for table in (None, "rough", "zeros"):
                for k in (7, 64, 65, 100):
                    want = fam.sibling(table, k, **kw)
                    nsbind.collapsed_kernel_ms(reset=True)
                    for law in ("zeros", "distinct"):
                        got = fam.collapsed(law, table, k, **kw)
                        same_as_sibling((law, table, k), got, want)
                        assert not np.any(got[3]), (law, "others")
                        n = want[2]
                        for q in range(len(n)):
                            assert not np.any(got[2][q, int(n[q]):]) and (law == "zeros" or np.all(got[2][q, :int(n[q])])) and (law != "zeros" or not np.any(got[2][q]))
                    assert all(v > 0.0 for v in nsbind.collapsed_kernel_ms())       # the collapsing kernels ran, the count pass too
                    got = fam.collapsed("one", table, k, **kw)
                    assert got[0] == 0
                    for q in range(len(want[2])):
                        n = min(int(want[2][q]), 1)
                        assert int(got[4][q]) == n and int(got[5][q]) == int(want[3][q])
                        assert got[1][q, :n].tobytes() == want[1][q, :n].tobytes()
                        tail = got[1][q, n:]
                        assert np.all(tail["score"].view(np.uint32) == 0xFF800000) and np.all(tail["seg"] == 0xFFFFFFFF) and np.all(tail["doc"] == 0xFFFFFFFF)
                        assert not np.any(got[2][q, n:]) and not np.any(got[3][q, n:])
                        if n:
                            assert int(got[2][q, 0]) == 7 and int(got[3][q, 0]) == int(want[3][q]) - 1
                        checked += n
        return checked
    finally:
        fam.release()


def run_dialects(n_segs=3):
    """each dialect form under a law: the arrays a call may leave NULL, left NULL; and MUST refs under clauses == NULL"""
    fam = directed_family(n_segs)
    try:
        for form, (names, (roles, clauses, needs)) in boost_shapes.NULL_FORMS.items():
            qs = [NAMES.index(n) for n in names]
            for law, table in (("mod7", "rough"), ("mod150", None)):
                for k in (3, 100):
                    fam.check(("collapse dialect", form), law, table, k, roles=roles, clauses=clauses, needs=needs, queries=qs)
        segments, _, idfs, weights, order = directed_inputs(n_segs)
        one = [[(ALL, M, 0, 1), (EDGE, M, 1, 1), (A, S, 0, 0), (NOTL, X, 0, 0)], [(A, M, 0, 1), (B, M, 1, 1)], [(NEG, M, 0, 1), (ALL, S, 0, 0)]]
        queries = [[(s, li, r, c, m) for li, r, c, m in q for s in range(n_segs)] for q in one]
        bfam = Family(segments, queries, idfs, weights, seg_order=order, tables={"rough": fam.tables["rough"]})
        try:
            assert min(bfam.founds) >= 1
            bfam.check(("collapse dialect", "boolean"), "mod7", "rough", 100, clauses=None, needs=None)
        finally:
            bfam.release()
    finally:
        fam.release()


def run_filter():
    """under a filter's copy of a segment: the copy keeps the docIds, so the source's group table serves it unchanged, and a
    document the filter removed is neither a representative nor counted"""
    segments, queries, idfs, weights, _ = directed_inputs(1)
    fam = Family(segments, queries, idfs, weights)
    copy = None
    try:
        n_docs, dl, ls = segments[0]
        keep = (np.arange(n_docs) % 3 != 1)
        keep[[31, 32, 127, 128, 299]] = True
        kept_lists = [(d[keep[d]], t[keep[d]]) for d, t in ls]
        want_all = quorum_ref.quorum_all([(n_docs, dl, kept_lists)], queries, [0], idfs, weights)
        counts = np.array([len(d) for d, _ in ls], dtype=np.uint32)
        copy, noff, ncnt, _, _, _ = nsbind.segment_filter(fam.segs.ctx, fam.segs.segs[0], 7, filter_ref.bits_of(keep), fam.segs.offs[0], counts)
        refs = fam.refs.copy()
        li_of = [li for q in queries for _, li, _, _, _ in q]
        for r, li in enumerate(li_of):
            refs[r] = (7, int(ncnt[li]), int(noff[li]), idfs[0][li], weights[0][li])
        unfiltered = collapse_ref.collapsed(fam.rows("rough"), fam.laws["mod7"], 100)
        for law in ("mod7", "mod150"):
            rows = boost_ref.boosted_rows([[(v, 7, d) for v, _, d in r] for r in want_all], {7: fam.tables["rough"][0]}, [7])
            for k in (1, 100):
                out = nsbind.search_collapsed_raw(fam.segs.ctx, fam.qd, refs, fam.roles, fam.clauses, fam.needs, k, [7], [copy], fam.boosts("rough"), fam.groups(law))
                assert out[0] == 0, fam.segs.err()
                want = collapse_ref.collapsed(rows, {7: fam.laws[law][0]}, k)
                collapse_ref.check(("collapse filter", law), want, *out[1:6], k)
                if law == "mod7" and k == 100:
                    q = NAMES.index("dense")
                    assert want[q][2] != unfiltered[q][2] and sum(want[q][2]) + want[q][3] == want[q][4] < unfiltered[q][4]
    finally:
        if copy is not None:
            fam.segs.L.ns_segment_release(fam.segs.ctx, copy)
        fam.release()


# ---- the randomised family --------------------------------------------------------------------------------------------
RANDOM_SEED = 20261021
RANDOM_DOCS = [4500, 2300, 700]


def random_inputs():
    """three segments of a few thousand documents, four lists, keys drawn so that the group sizes range from 1 to 50 (groups span
    the segments), a sixth of the documents without a key; the seed is fixed"""
    rng = np.random.default_rng(RANDOM_SEED)
    total = sum(RANDOM_DOCS)
    keys, g = np.zeros(total, np.uint32), 1
    perm = rng.permutation(total)
    at = 0
    while at < total:
        size = int(rng.integers(1, 51))
        keys[perm[at:at + size]] = 0 if g % 6 == 0 else g * 2654435761 % 0xFFFFFFFE + 1
        at += size
        g += 1
    segments, laws, off = [], {"random": []}, 0
    for n in RANDOM_DOCS:
        ls = []
        for density in (0.6, 0.2, 0.05, 0.02):
            ids = np.flatnonzero(rng.random(n) < density).astype(np.uint32)
            ls.append((ids, rng.integers(1, 6, len(ids)).astype(np.uint32)))
        segments.append((n, rng.integers(5, 60, n).astype(np.uint32), ls))
        laws["random"].append(keys[off:off + n].copy())
        off += n
    one = [[(0, S, 0, 0)], [(0, S, 0, 0), (1, S, 0, 0), (2, S, 0, 0)], [(0, M, 0, 1), (1, M, 1, 1), (3, X, 0, 0)], [(1, M, 0, 2), (2, M, 0, 2), (0, M, 0, 2), (3, S, 0, 0)],
           [(2, M, 0, 1), (3, M, 0, 1), (0, S, 0, 0)]]
    queries = [[(s, li, r, c, m) for li, r, c, m in q for s in range(3)] for q in one]
    tables = {"rough": [np.float32(0.5) + (((np.arange(n) * 37 + 11 * s) % 101) / 101.0).astype(np.float32) for s, n in enumerate(RANDOM_DOCS)],
              "ones": [np.ones(n, np.float32) for n in RANDOM_DOCS]}
    idf, w = [1.3, 1.7, 2.1, 1.0], [1.0, 0.75, 1.25, 1.0]
    return segments, queries, [idf] * 3, [w] * 3, [1, 2, 0], tables, laws


def run_random(ks=(10, 100)):
    segments, queries, idfs, weights, order, tables, laws = random_inputs()
    fam = Family(segments, queries, idfs, weights, seg_order=order, tables=tables, laws=laws)
    try:
        sizes = np.unique(np.concatenate(laws["random"]), return_counts=True)[1][1:]
        assert sizes.min() == 1 and sizes.max() >= 40 and min(fam.founds) > 100
        for k in ks:
            for table in ("rough", None):
                out = fam.check(("collapse random",), "random", table, k)
                assert int(out[3].max()) >= 5
    finally:
        fam.release()
    return [int(f) for f in fam.founds]


# ---- members in different waves of one workgroup ----------------------------------------------------------------------
WAVE_DOCS = 4200          # one segment; a window that holds 4096 of them is 128 bitmap words: wave 0 sweeps words 0 .. 63, wave 1 words 64 .. 127
WAVE_SPAN = 2048          # documents per wave: 64 words of 32
WAVE_PAIRS = 40           # groups with one member in each wave, both among their wave's best K = 100


def wave_inputs():
    """one segment of 4200 documents under one dense list (and a sparse one).  Law "waves": the i-th best document of [0, 2048) by
    the dense query and the (39 - i)-th best of [2048, 4096) share key 1 + i, everything else stands alone: at a window of 4096
    documents (and at the product's) the two members of a group are kept by DIFFERENT waves of the workgroup and meet when wave 0
    merges the four sets, the better one in wave 0 for some groups (the other is dropped) and in wave 1 for others (it replaces).
    Law "mod32": documents d, d + 32, ... share a key: neighbouring words, so neighbouring lanes of one round of the sweep."""
    d = np.arange(WAVE_DOCS, dtype=np.uint32)
    sparse = d[(d * 13) % 17 == 3]
    ls = [(d, (1 + (d * 7) % 5).astype(np.uint32)), (sparse, (1 + sparse % 3).astype(np.uint32))]
    segments = [(WAVE_DOCS, (5 + (d * 11) % 53).astype(np.uint32), ls)]
    queries = [[(0, 0, S, 0, 0)], [(0, 0, M, 0, 1), (0, 1, S, 0, 0)], [(0, 1, S, 0, 0)]]
    idfs, weights = [[1.3, 2.1]], [[1.0, 0.75]]
    everything = quorum_ref.quorum_all(segments, queries, [0], idfs, weights)
    tables = {"ones": [np.ones(WAVE_DOCS, np.float32)]}
    ranked = [r[2] for r in boost_ref.boosted_rows(everything, tables["ones"], [0])[0]]
    lower = [x for x in ranked if x < WAVE_SPAN][:WAVE_PAIRS]
    upper = [x for x in ranked if WAVE_SPAN <= x < 2 * WAVE_SPAN][:WAVE_PAIRS]
    keys = np.zeros(WAVE_DOCS, np.uint32)
    for i in range(WAVE_PAIRS):
        keys[lower[i]] = keys[upper[WAVE_PAIRS - 1 - i]] = 1 + i
    laws = {"waves": [keys], "mod32": [(1 + d % 32).astype(np.uint32)]}
    return segments, queries, idfs, weights, tables, laws, everything


def check_wave_properties(everything, tables, laws):
    """the property the family is named after, on the restatement's own answer"""
    rows = boost_ref.boosted_rows(everything, tables["ones"], [0])[0]
    keys = laws["waves"][0]
    rank_in_wave = {}
    for w in (0, 1):
        for i, r in enumerate([r for r in rows if r[2] // WAVE_SPAN == w]):
            rank_in_wave[r[2]] = i
    coll = collapse_ref.collapse_rows(rows, laws["waves"])
    rep_wave = {g: r[2] // WAVE_SPAN for r, g, _ in coll if g}
    assert len(rep_wave) == WAVE_PAIRS and all(o == 1 for _, g, o in coll if g)
    for g in range(1, WAVE_PAIRS + 1):
        docs = [int(x) for x in np.flatnonzero(keys == g)]
        assert len(docs) == 2 and sorted(x // WAVE_SPAN for x in docs) == [0, 1]                      # one member per wave
        assert all(x // 32 // 64 == x // WAVE_SPAN and rank_in_wave[x] < 100 for x in docs)          # words 0 .. 63 | 64 .. 127; both kept at K = 100
    assert sum(1 for w in rep_wave.values() if w == 0) >= 5 and sum(1 for w in rep_wave.values() if w == 1) >= 5   # drops and replacements at the merge
    assert WAVE_DOCS > 2 * WAVE_SPAN and len(rows) == WAVE_DOCS
    mod = collapse_ref.collapse_rows(rows, laws["mod32"])
    assert len(mod) == 32 and all(o >= WAVE_DOCS // 32 - 1 for _, _, o in mod)
    return coll


def run_waves(ks=(10, 64, 65, 100)):
    """the family against the restatement; needs a window of more than 2048 documents to be what it is named after (the product's
    8192, or 4096 in the test builds), and is exact at any"""
    segments, queries, idfs, weights, tables, laws, everything = wave_inputs()
    check_wave_properties(everything, tables, laws)
    fam = Family(segments, queries, idfs, weights, tables=tables, laws=laws)
    try:
        for law in ("waves", "mod32"):
            for k in ks:
                fam.check(("collapse waves",), law, None, k)
                fam.check(("collapse waves",), law, "ones", k, others=False)
    finally:
        fam.release()
    return WAVE_DOCS


# ---- refusals -----------------------------------------------------------------------------------------------------------
def run_refusals():
    """a NULL table entry, a table of another ctx, a table whose n_docs differs from its segment's (shorter AND longer), NULL arrays;
    the sibling's refusals under this call's name.  A refused call writes nothing."""
    import ctypes as Ct

    L = nsbind.hip_lib()
    fam = directed_family(3)
    ctx, order = fam.segs.ctx, fam.order
    other = Ct.c_void_p()
    extra = []
    try:
        def call(match, groups="own", boosts="rough", roles=fam.roles, clauses=fam.clauses, needs=fam.needs):
            rc, *outs = fam.collapsed("mod7", boosts, 10, roles=roles, clauses=clauses, needs=needs, groups=groups)
            if match is None:
                assert rc == 0, L.ns_last_error(ctx).decode()
                return
            msg = L.ns_last_error(ctx).decode()
            assert rc == NS_E_INVAL and "ns_search_collapsed: " in msg and match in msg, (rc, msg)
            for o in outs[:5]:
                fill = 0xAB if o.dtype == nsbind.HIT_DTYPE else 0xABABABAB
                assert np.all((o.view(np.uint8) if o.dtype == nsbind.HIT_DTYPE else o) == fill), "a refused call writes nothing"

        good = fam.groups("mod7")
        call(None)
        call("segment or group table 1 is NULL", groups=[good[0], None, good[2]])
        call("null group tables", groups=None)
        for n in (N_DOCS - 1, N_DOCS + 1, 0):
            rc, h = nsbind.dockeys_upload(ctx, np.ones(n, np.uint32))
            assert rc == 0
            extra.append(h)
            call("group table 2 keys %d documents, its segment has 300" % n, groups=[good[0], good[1], h])
        assert L.ns_ctx_create(0, Ct.byref(other)) == 0
        rc, foreign = nsbind.dockeys_upload(other, np.ones(N_DOCS, np.uint32))
        assert rc == 0
        call("group table 1 does not belong to this ctx", groups=[good[0], foreign, good[2]])
        assert L.ns_dockeys_release(other, foreign) == 0
        bad = np.ones(N_DOCS, np.uint32)
        bad[17] = 0xFFFFFFFF
        assert nsbind.dockeys_upload(ctx, bad)[0] == NS_E_INVAL                 # the upload still refuses the reserved key
        # the sibling's refusals, under this call's name
        q2 = NAMES.index("quorum: two of three")
        first = int(fam.qd[q2]["term_begin"])
        eight = fam.needs.copy()
        eight[first] = 8
        call("ref %d: a need of 8 (query %d); at most 7" % (first, q2), needs=eight)
        call("needs without clauses", clauses=None)
        roles = fam.roles.copy()
        roles[first] = 3
        call("ref %d: role 3 is none of" % first, roles=roles)
        gb = fam.boosts("rough")
        rc = nsbind.search_collapsed_raw(ctx, fam.qd, fam.refs, fam.roles, fam.clauses, fam.needs, 10, order, fam.handles, [gb[0], None, gb[2]], good)[0]
        assert rc == NS_E_INVAL and "segment or boost table 1 is NULL" in L.ns_last_error(ctx).decode()
        args = [None, 0, None, None, None, None, 0, 10, None, None, None, None, 0, None, None, None, None, None, None]
        assert L.ns_search_collapsed(ctx, *args) == 0 and L.ns_search_collapsed(None, *args) == NS_E_INVAL
        out3 = (Ct.c_float * 3)()
        assert L.ns_collapsed_kernel_ms(out3, 1) == 0 and all(v > 0.0 for v in out3) and L.ns_collapsed_kernel_ms(None, 0) == NS_E_INVAL
    finally:
        for h in extra:
            assert nsbind.dockeys_release(ctx, h) == 0
        if other:
            L.ns_ctx_destroy(other)
        fam.release()


def main(out_path):
    """child process at NS_FACET_TILE_DOCS = 128 and NS_BOOL_WIN_DOCS = 32.  Both builds run the directed families at one, two and
    three segments; the counting build then runs the two-wave family at tiles and windows of 4096 documents and reports the counters of
    all the directed inputs, of the all-distinct law alone and of the randomised family at 4096; the variants build runs the dialects,
    the filter, the identities, the randomised family and the two-wave family."""
    counting = "ns_debug_collapse_counters" in nsbind.debug_counters(reset=True)
    assert os.environ.get("NS_BOOL_WIN_DOCS") == str(SMALL_WIN)
    rep = {"tile": run_directed(1, tile_expected=SMALL_TILE), "counting": counting}
    run_directed(2, ks=[10, 100])
    run_directed(3, ks=[10, 100])
    if counting:
        def events():
            c = nsbind.debug_counters(reset=True)
            return dict(zip(EVENTS, c["ns_debug_collapse_counters"]), all_select_items=c["ns_debug_boolean_counters"][0])

        os.environ["NS_FACET_TILE_DOCS"] = os.environ["NS_BOOL_WIN_DOCS"] = str(MID)     # the directed family that needs two waves in one window
        assert nsbind.facet_tile_docs() == MID
        run_waves()
        rep["events_directed"] = events()
        os.environ["NS_FACET_TILE_DOCS"], os.environ["NS_BOOL_WIN_DOCS"] = str(SMALL_TILE), str(SMALL_WIN)
        assert nsbind.facet_tile_docs() == SMALL_TILE
        run_directed(3, ks=[10, 100], pairs=[("distinct", "rough"), ("distinct", None)])
        rep["events_distinct"] = events()
        os.environ["NS_FACET_TILE_DOCS"] = os.environ["NS_BOOL_WIN_DOCS"] = str(MID)
        assert nsbind.facet_tile_docs() == MID
        run_random()
        rep["events_random"] = events()
        print("collapse", rep["events_directed"], rep["events_distinct"], rep["events_random"], flush=True)
    else:
        run_dialects()
        run_filter()
        rep["identities"] = run_sibling_identities()
        rep["random_small"] = run_random(ks=(100,))
        os.environ["NS_FACET_TILE_DOCS"] = os.environ["NS_BOOL_WIN_DOCS"] = str(MID)
        assert nsbind.facet_tile_docs() == MID
        rep["random_mid"] = run_random()
        rep["waves"] = run_waves()
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print("collapse shapes OK")


if __name__ == "__main__":
    main(sys.argv[1])
