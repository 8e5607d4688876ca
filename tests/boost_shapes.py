"""Directed inputs of ns_search_boosted_after (k_bq_select<true, ., ., true> in csrc/ns_boolean.hip) and the code
that runs them through the raw C-ABI against the restatement (tests/boost_ref.py over tests/quorum_ref.py).  300 documents per
segment (not a multiple of 32), one segment and three listed as 2, 0, 1, a handful of lists and a handful of factor tables, each
built for the property a case is named after; check_properties asserts those properties on the restatement's own answer, so a
case that lost its point fails before any kernel runs (tests/test_boost_cpu.py calls it without a GPU).  All comparisons are
exact, product bits included.

Imported by tests/test_boost_gpu.py for the product library (one tile and one window hold a segment; a family of a product tile
+ 37 documents puts matched documents at 8191 | 8192 and 131071 | 131072), and run as a program in a child process that loaded
the variants or the counting build with NS_FACET_TILE_DOCS=128 NS_BOOL_WIN_DOCS=32: there 300 documents are two whole tiles and a
part, four windows each, matched documents lie on both sides of window and tile edges, every item of the dense list matches more
than K = 100 documents, and the counting build reports what the boosted sweep reached."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "nextsearch-api_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import after_ref  # noqa: E402
import after_shapes  # noqa: E402
import boolean_shapes  # noqa: E402
import boost_ref  # noqa: E402
import filter_ref  # noqa: E402
import grouped_shapes  # noqa: E402
import nsbind  # noqa: E402
import quorum_ref  # noqa: E402
import quorum_shapes  # noqa: E402
from boolean_ref import MUST, NOT, SHOULD  # noqa: E402

NS_E_INVAL = -1
SMALL_TILE, SMALL_WIN, N_DOCS = boolean_shapes.SMALL_TILE, boolean_shapes.SMALL_WIN, boolean_shapes.N_DOCS
KS = [1, 64, 65, 100]                         # 64 / 65: the boundary between the kept set's two registers
S, M, X = SHOULD, MUST, NOT
EVENTS = nsbind.BOOST_EVENTS                  # ns_debug_boolean_boost_counters, in order (counting build)
POS0, NEG0 = 0x00000000, 0x80000000           # the bits of +0.0f and -0.0f

# list numbers
ALL, EDGE, NEG, P1, P2, A, B, C, NOTL, INV = range(10)
INV_DOCS = [1, 30, 33, 62, 65, 90, 126, 129, 160, 190, 220, 254, 257, 270, 280, 290, 295, 297, 298, 299]
TIE_PAIRS = [(40, 41), (95, 96)]              # (document of P1, document of P2): equal length, equal tf; 95 | 96 share a window, 40 | 41 too
IDF = [1.3, 1.7, 1.1, 2.0, 2.0, 1.9, 2.3, 2.9, 1.0, 1.45]
QWEIGHT = [1.0, 0.75, -0.25, 1.0, 2.0, 1.0, 1.25, 0.5, 1.0, 1.0]      # NEG scores below zero; P2 scores exactly twice P1


def lists():
    """ALL: every document (each small tile matches more than K = 100).  EDGE: both sides of the window edges 32 and 64, of the
    tile edges 128 and 256, and the last two documents.  NEG: a list under a negative weight, on edges too.  P1, P2: the tie
    pairs.  A, B, C: documents in exactly 0, 1, 2 and 3 of them (quorum_shapes').  NOTL: an exclusion.  INV: twenty documents of
    twenty different scores, spread over every tile."""
    d = np.arange(N_DOCS, dtype=np.uint32)
    docs = {ALL: (d, 1 + d % 5), EDGE: ([0, 31, 32, 63, 64, 127, 128, 255, 256, 298, 299], 2), NEG: ([5, 31, 32, 100, 127, 128, 299], 3),
            P1: ([a for a, _ in TIE_PAIRS], 3), P2: ([b for _, b in TIE_PAIRS], 3), A: ([3, 10, 40, 41, 130, 200, 299], 1), B: ([10, 41, 42, 131, 200, 260], 2),
            C: ([10, 40, 42, 132, 200, 261], 1), NOTL: ([10, 41, 150], 1), INV: (INV_DOCS, 1 + np.arange(len(INV_DOCS)))}
    out = []
    for li in range(len(docs)):
        ids = np.asarray(docs[li][0], dtype=np.uint32)
        assert np.all(ids[1:] > ids[:-1])
        out.append((ids, np.broadcast_to(np.asarray(docs[li][1], dtype=np.uint32), ids.shape).copy()))
    return out


# (list, role, clause, need) per ref
CASES = {
    "dense": [(ALL, S, 0, 0)],
    "edges": [(EDGE, S, 0, 0)],
    "negative": [(NEG, S, 0, 0)],
    "inverted": [(INV, S, 0, 0)],
    "tie pairs": [(P1, S, 0, 0), (P2, S, 0, 0)],
    "all optional": [(A, S, 0, 0), (B, S, 0, 0), (C, S, 0, 0)],
    "boolean": [(A, M, 0, 1), (B, S, 0, 0), (ALL, M, 1, 1), (NOTL, X, 0, 0)],
    "grouped": [(A, M, 0, 1), (B, M, 0, 1), (C, S, 0, 0), (EDGE, M, 1, 1), (ALL, M, 1, 1), (NOTL, X, 0, 0)],
    "quorum: two of three": [(A, M, 0, 2), (B, M, 0, 2), (C, M, 0, 2)],
    "dense, with a negative list and the pairs": [(ALL, S, 0, 0), (NEG, S, 0, 0), (P2, S, 0, 0)],
    "required edges of the dense list": [(ALL, M, 0, 1), (EDGE, M, 1, 1), (NEG, S, 0, 0)],
    "nothing matches": [(A, M, 0, 1), (A, X, 0, 0)],
}
DIRECTED = [[]] + list(CASES.values())
NAMES = ["no ref"] + list(CASES)
# the dialect forms: what a call may leave NULL, and the queries that say the same with the arrays given
NULL_FORMS = {"roles NULL": (["dense", "edges", "negative", "tie pairs", "all optional"], (None, None, None)),
              "clauses NULL": (["dense", "negative"], ("own", None, None)),      # (MUST refs of singleton clauses are added below)
              "needs NULL": (["dense", "boolean", "grouped", "nothing matches"], ("own", "own", None))}


def doc_lens(s):
    dl = (5 + (np.arange(N_DOCS) * (1 + 2 * s)) % 41).astype(np.uint32)
    for a, b in TIE_PAIRS:
        dl[b] = dl[a]
    return dl


def directed_inputs(n_segs, cases=None):
    """DIRECTED over one or three segments -> (segments, queries, idfs, weights, seg_order): with three segments the refs of a
    query interleave the segments and the call lists them as 2, 0, 1"""
    ls = lists()
    segments = [(N_DOCS, doc_lens(s), ls) for s in range(n_segs)]
    queries = [[(s, li, role, clause, need) for li, role, clause, need in q for s in range(n_segs)] for q in (DIRECTED if cases is None else cases)]
    return segments, queries, [IDF] * n_segs, [QWEIGHT] * n_segs, ([2, 0, 1] if n_segs == 3 else None)


def tables_for(segments, everything, seg_order):
    """name -> one float32 table per segment (indexed by segment number), different from segment to segment where the name allows"""
    n_segs = len(segments)
    d = np.arange(N_DOCS)
    out = {"ones": [np.ones(N_DOCS, np.float32) for _ in range(n_segs)], "zeros": [np.zeros(N_DOCS, np.float32) for _ in range(n_segs)]}
    out["mixed"] = [(((d * 7 + 3 * s) % 13) / 4.0).astype(np.float32) for s in range(n_segs)]                     # 0 .. 3 in quarters, zeros among them
    out["rough"] = [np.float32(0.5) + (((d * 37 + 11 * s) % 101) / 101.0).astype(np.float32) for s in range(n_segs)]   # products that round
    out["ties"] = [np.ones(N_DOCS, np.float32) for _ in range(n_segs)]
    for t in out["ties"]:
        for _, b in TIE_PAIRS:
            t[b] = 0.5
    # powers of two that turn the ranking of "inverted" round, per segment: the i-th best score gets 2^(c * (i - n)), where 2^c is
    # above the ratio of the largest to the smallest score, so every product is exact and below the next one's
    out["invert"] = [np.ones(N_DOCS, np.float32) for _ in range(n_segs)]
    rows = everything[NAMES.index("inverted")]
    for s in range(n_segs):
        mine = [(float(v), int(doc)) for v, seg, doc in rows if seg == s]
        assert len(mine) == len(INV_DOCS) and len({v for v, _ in mine}) == len(mine) and min(v for v, _ in mine) > 0.0
        c = int(np.ceil(np.log2(max(v for v, _ in mine) / min(v for v, _ in mine)))) + 1
        assert c * len(mine) < 120
        for i, (_, doc) in enumerate(sorted(mine, reverse=True)):
            out["invert"][s][doc] = np.float32(2.0) ** (c * (i - len(mine)))
    return out


TABLES = ["ones", "zeros", "mixed", "rough", "ties", "invert"]


def check_properties(everything, tables, seg_order):
    """what each case exists for, asserted on the restatement's own answer"""
    order = list(seg_order)
    n_segs = len(order)
    q_of = NAMES.index
    rows_of = {name: boost_ref.boosted_rows(everything, tables[name], order) for name in TABLES}
    plain = rows_of["ones"]
    # all-1.0f: the unboosted ranking, bits and all
    for q, rows in enumerate(everything):
        assert [(r[3], r[2], r[4]) for r in plain[q]] == [(s, int(d), int(np.float32(v).view(np.uint32))) for v, s, d in rows]
    # inverted ranking: per segment the boosted order of the twenty documents is the unboosted order backwards
    for s in order:
        before = [r[2] for r in plain[q_of("inverted")] if r[3] == s]
        after = [r[2] for r in rows_of["invert"][q_of("inverted")] if r[3] == s]
        assert len(before) == len(INV_DOCS) and after == before[::-1] and after != before
    # all-zero factors: every product of the positive scores is +0.0f and the order falls to (segment position, docId)
    rows = rows_of["zeros"][q_of("dense")]
    assert len(rows) == n_segs * N_DOCS and {r[4] for r in rows} == {POS0}
    assert [(r[1], r[2]) for r in rows] == sorted((r[1], r[2]) for r in rows) and [r[3] for r in rows[::N_DOCS]] == order
    # zero against negative: -0.0f, just below +0.0f
    rows = rows_of["zeros"][q_of("negative")]
    assert rows and {r[4] for r in rows} == {NEG0} and all(r[4] & 0x80000000 and r[4] != NEG0 for r in plain[q_of("negative")])
    rows = rows_of["zeros"][q_of("dense, with a negative list and the pairs")]
    assert {r[4] for r in rows} == {POS0}                                     # (the dense list outweighs the negative one)
    rows = rows_of["mixed"][q_of("negative")]
    bits = [r[4] for r in rows]
    assert NEG0 in bits and any(b & 0x80000000 and b != NEG0 for b in bits) and bits.index(NEG0) == 0     # -0.0f leads the negative products
    rows = rows_of["mixed"][q_of("required edges of the dense list")]
    assert POS0 in {r[4] for r in rows} and any(r[4] not in (POS0, NEG0) for r in rows)
    # product ties: different raw scores (exactly 2 : 1), equal products, so the docId decides where the raw score decided
    for s in order:
        raw = {r[2]: r[4] for r in plain[q_of("tie pairs")] if r[3] == s}
        tied = [r for r in rows_of["ties"][q_of("tie pairs")] if r[3] == s]
        for a, b in TIE_PAIRS:
            assert raw[a] != raw[b] and np.uint32(raw[b]).view(np.float32) == 2.0 * np.uint32(raw[a]).view(np.float32)
            ra, rb = [r for r in tied if r[2] == a][0], [r for r in tied if r[2] == b][0]
            assert ra[4] == rb[4] == raw[a] and tied.index(ra) + 1 == tied.index(rb)
        assert [r[2] for r in plain[q_of("tie pairs")] if r[3] == s][0] in [b for _, b in TIE_PAIRS]          # unboosted: a P2 document leads
    # segments with different tables: the join orders by product, so the segments interleave and the ranking really changes
    if n_segs > 1:
        for name in ("mixed", "rough"):
            assert all(tables[name][0].tobytes() != tables[name][s].tobytes() for s in order if s != 0)
            segs = [r[3] for r in rows_of[name][q_of("dense")][:100]]
            assert len(set(segs)) == n_segs and segs != sorted(segs, key=order.index)
            assert [(r[3], r[2]) for r in rows_of[name][q_of("dense")]] != [(r[3], r[2]) for r in plain[q_of("dense")]]
    # K and the kept set: more than K = 100 matched documents in every small tile of the dense list
    assert len(plain[q_of("dense")]) == n_segs * N_DOCS and SMALL_TILE > 100
    # edges: matched documents on both sides of window edges, of tile edges, and the last document of a partial word
    docs = {r[2] for r in plain[q_of("edges")]}
    assert {31, 32, 63, 64, 127, 128, 255, 256, 299} <= docs and N_DOCS % 32 != 0
    # rounding: under "rough" most products are not exact
    inexact = sum(float(np.uint32(boost_ref.product_bits(v, tables["rough"][seg][int(d)])).view(np.float32)) != float(v) * float(tables["rough"][seg][int(d)])
                  for v, seg, d in everything[q_of("dense")])
    assert inexact > N_DOCS // 4, inexact
    # the dialects match something, and differently
    founds = [len(r) for r in everything]
    for name in ("all optional", "boolean", "grouped", "quorum: two of three"):
        assert founds[q_of(name)] >= 2 * n_segs, (name, founds)
    assert founds[q_of("no ref")] == 0 and founds[q_of("nothing matches")] == 0
    return rows_of


class Family(quorum_shapes.Family):
    """quorum_shapes.Family + named factor tables, uploaded when a call first asks for them"""

    def __init__(self, segments, queries, idfs, weights, seg_order=None, tables=None):
        super().__init__(segments, queries, idfs, weights, seg_order)
        self.tables = tables_for(segments, self.everything, self.order) if tables is None else tables
        self._boosts, self._rows = {}, {}

    def boosts(self, name):
        """the ns_docboost handles of a table, in the call's segment order"""
        if name not in self._boosts:
            hs = []
            for s in self.order:
                rc, h = nsbind.docboost_upload(self.segs.ctx, self.tables[name][s])
                assert rc == 0, self.segs.err()
                hs.append(h)
            self._boosts[name] = hs
        return self._boosts[name]

    def rows(self, name):
        if name not in self._rows:
            self._rows[name] = boost_ref.boosted_rows(self.everything, self.tables[name], self.order)
        return self._rows[name]

    def release(self):
        if self.segs.ctx:
            for hs in self._boosts.values():
                for h in hs:
                    assert nsbind.docboost_release(self.segs.ctx, h) == 0
            self._boosts = {}
        super().release()


class Boosted(grouped_shapes.Ranked):
    """a Family under one table, in product order: what after_shapes.walk, check_call and run_cursor_rounds drive.  roles /
    clauses / needs: "own", or what the call gets instead (None: NULL); queries: the subset of the family's queries the call
    carries (None: all)"""

    def __init__(self, fam, table, roles="own", clauses="own", needs="own", queries=None):
        self.fam, self.table, self.roles, self.clauses, self.needs = fam, table, roles, clauses, needs
        self.queries = list(range(len(fam.qd))) if queries is None else list(queries)
        self.rows = [fam.rows(table)[q] for q in self.queries]
        self.qd = fam.qd[self.queries]

    def arrays(self):
        fam = self.fam
        return (fam.roles if isinstance(self.roles, str) else self.roles, fam.clauses if isinstance(self.clauses, str) else self.clauses,
                fam.needs if isinstance(self.needs, str) else self.needs)

    def raw(self, k, cursors, boosts="own"):
        fam = self.fam
        ro, cl, ne = self.arrays()
        return nsbind.search_boosted_after_raw(fam.segs.ctx, self.qd, fam.refs, ro, cl, ne, k, None if cursors is None else nsbind.cursors(cursors), fam.order,
                                               fam.handles, fam.boosts(self.table) if isinstance(boosts, str) else boosts)

    def sibling(self, k, cursors):
        fam = self.fam
        ro, cl, ne = self.arrays()
        return nsbind.search_quorum_after_raw(fam.segs.ctx, self.qd, fam.refs, ro, cl, ne, k, None if cursors is None else nsbind.cursors(cursors), fam.order,
                                              fam.handles)


def directed_family(n_segs):
    segments, queries, idfs, weights, order = directed_inputs(n_segs)
    return Family(segments, queries, idfs, weights, seg_order=order)


def run_directed(n_segs, tile_expected=None, tables=TABLES, ks=KS):
    """every directed case under every table at K = 1, 64, 65 and 100, against the restatement"""
    tile = nsbind.facet_tile_docs()
    if tile_expected is not None:
        assert tile == tile_expected, (tile, tile_expected)
    fam = directed_family(n_segs)
    try:
        check_properties(fam.everything, fam.tables, fam.order)
        for name in tables:
            side = Boosted(fam, name)
            for k in ks:
                side.check(("boost directed", n_segs, name), k)
    finally:
        fam.release()
    return tile


def run_dialects(n_segs=3):
    """each dialect form under one non-trivial table: the arrays a call may leave NULL, left NULL"""
    fam = directed_family(n_segs)
    try:
        for form, (names, (roles, clauses, needs)) in NULL_FORMS.items():
            qs = [NAMES.index(n) for n in names]
            if form == "clauses NULL":                                          # every MUST ref a clause of its own: the boolean call's reading
                assert all(len({c for _, _, r, c, _ in fam.quorum[q] if r == M}) <= 1 for q in qs)
            for table in ("mixed", "rough"):
                side = Boosted(fam, table, roles=roles, clauses=clauses, needs=needs, queries=qs)
                for k in (3, 100):
                    side.check(("boost dialect", form, table), k)
        # clauses NULL with MUST refs: a family whose MUST refs are singleton clauses
        segments, _, idfs, weights, order = directed_inputs(n_segs)
        one = [[(ALL, M, 0, 1), (EDGE, M, 1, 1), (A, S, 0, 0), (NOTL, X, 0, 0)], [(A, M, 0, 1), (B, M, 1, 1)], [(NEG, M, 0, 1), (ALL, S, 0, 0)]]
        queries = [[(s, li, r, c, m) for li, r, c, m in q for s in range(n_segs)] for q in one]
        bfam = Family(segments, queries, idfs, weights, seg_order=order, tables={"mixed": fam.tables["mixed"]})
        try:
            assert min(bfam.founds) >= 1
            Boosted(bfam, "mixed", clauses=None, needs=None).check(("boost dialect", "boolean"), 100)
        finally:
            bfam.release()
    finally:
        fam.release()


def run_walks():
    """pages of 3 to exhaustion under "mixed" (tie runs at +0.0f and at every quarter) on three segments: per query the pages
    concatenated are the full boosted ranking, rest counting down (after_shapes.walk asserts each); and K = 1 under "zeros", where
    (segment, docId) alone decides every page"""
    fam = directed_family(3)
    try:
        qs = [q for q in range(len(NAMES)) if NAMES[q] != "dense" and "dense," not in NAMES[q]]       # (the 900-document rankings walk at K = 100 below)
        pages = {"3": after_shapes.walk(("boost walk", 3), Boosted(fam, "mixed", queries=qs), 3),
                 "1": after_shapes.walk(("boost walk", 1), Boosted(fam, "zeros", queries=[NAMES.index("edges"), NAMES.index("negative")]), 1),
                 "100": after_shapes.walk(("boost walk", 100), Boosted(fam, "rough"), 100)}
        assert pages["3"] >= 20 and pages["1"] == 34 and pages["100"] == 10, pages
        return pages
    finally:
        fam.release()


def run_cursors():
    """arbitrary cursors against after_ref.page: on a product rank that no document has, on a tie run (before, inside and behind
    it), behind the last document, the special bit patterns; term weights, factors and a cursor together (the family's weights
    are not 1)"""
    fam = directed_family(3)
    try:
        order = fam.order
        for table, names in (("mixed", [n for n in NAMES if n not in ("required edges of the dense list", "dense, with a negative list and the pairs")]),
                             ("ties", ["tie pairs", "edges"])):
            side = Boosted(fam, table, queries=[NAMES.index(n) for n in names])

            def between(rows):
                have = {r[4] for r in rows}
                return [b for b in sorted({r[4] + 1 for r in rows} | {r[4] - 1 for r in rows if r[4]}) if b not in have][:4]

            per_query = after_shapes.arbitrary_cursors(side, lambda r: r[4], between)
            assert any(between(rows) for rows in side.rows)
            specials = [(n, (after_shapes.BITS[n], order[1], 128)) for n in ("+0", "-0", "+inf", "-inf")]
            specials += [("above everything", (after_shapes.BITS["top"], order[0], 0)), ("below everything", (after_shapes.BITS["bottom"], order[-1], 0xFFFFFFFF))]
            after_shapes.run_cursor_rounds(("boost cursors", table), side, per_query, specials, 10)
        # a cursor inside the tie run at +0.0f of "mixed": the rest of the run follows, in (segment, docId) order
        side = Boosted(fam, "mixed", queries=[NAMES.index("dense")])
        run = [r for r in side.rows[0] if r[4] == POS0]
        assert len(run) >= 9
        mid = run[len(run) // 2]
        hits, _, nhits, found, rest = side.check(("boost cursors", "inside the +0.0f run"), 100, [(POS0, mid[3], mid[2])])
        assert int(rest[0]) == len(run) - len(run) // 2 - 1 and int(nhits[0]) == int(rest[0]) and int(found[0]) == len(side.rows[0])
        # behind the last document: nothing left, found intact
        last = side.rows[0][-1]
        hits, _, nhits, found, rest = side.check(("boost cursors", "behind the last"), 100, [(last[4], last[3], last[2])])
        assert int(nhits[0]) == 0 and int(rest[0]) == 0 and int(found[0]) == 3 * N_DOCS
    finally:
        fam.release()


def same_bytes(label, got, want):
    for i, (a, b) in enumerate(zip(got[1:5], want[1:5])):                       # hits, nhits, found, rest
        assert a.tobytes() == b.tobytes(), (label, "output", i)
    assert got[0] == want[0] == 0, label


def run_null_and_ones_are_the_sibling():
    """boosts == NULL IS ns_search_quorum_after (its kernels: the boosted kernels' times stay 0); an all-1.0f table gives its bytes
    through the boosted kernels: hits, nhits, found and rest, for all four dialect forms, without and with cursors"""
    fam = directed_family(3)
    try:
        forms = [("own", "own", "own", None)] + [(ro, cl, ne, [NAMES.index(n) for n in names]) for names, (ro, cl, ne) in NULL_FORMS.values()]
        for ro, cl, ne, qs in forms:
            side = Boosted(fam, "ones", roles=ro, clauses=cl, needs=ne, queries=qs)
            for k in (7, 64, 100):
                first = side.sibling(k, None)
                assert first[0] == 0, fam.segs.err()
                cursors = [None if not first[2][q] else side.next_cursor(first[1], None, q, int(first[2][q])) for q in range(len(side.rows))]
                for cu in (None, cursors):
                    want = side.sibling(k, cu)
                    nsbind.boosted_kernel_ms(reset=True)
                    same_bytes(("boosts NULL", k, cu is not None), side.raw(k, cu, boosts=None), want)
                    assert all(v == 0.0 for v in nsbind.boosted_kernel_ms())
                    same_bytes(("all ones", k, cu is not None), side.raw(k, cu), want)
                    assert all(v > 0.0 for v in nsbind.boosted_kernel_ms())
        return sum(f >= 2 for f in fam.founds)
    finally:
        fam.release()


def run_filter():
    """under a filter's copy of a segment (ns_segment_filter with a caller's bitmap): the copy keeps the docIds, so the source's
    table serves it unchanged"""
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
        assert [len(r) for r in want_all] != fam.founds and max(len(r) for r in want_all) > 100
        for table in ("mixed", "rough"):
            rows = boost_ref.boosted_rows([[(v, 7, d) for v, _, d in r] for r in want_all], {7: fam.tables[table][0]}, [7])
            for k in (1, 100):
                rc, hits, nhits, found, rest, _ = nsbind.search_boosted_after_raw(fam.segs.ctx, fam.qd, refs, fam.roles, fam.clauses, fam.needs, k, None, [7], [copy],
                                                                                  fam.boosts(table))
                assert rc == 0, fam.segs.err()
                for q in range(len(rows)):
                    after_shapes.check_page(("boost filter", table, k, q), rows[q], None, k, hits[q], nhits[q], found[q], rest[q], [7])
    finally:
        if copy is not None:
            fam.segs.L.ns_segment_release(fam.segs.ctx, copy)
        fam.release()


def product_inputs(tile):
    """one segment of a product tile + 37 documents: matched documents on both sides of the product's window edge (8191 | 8192) and
    of its tile edge (131071 | 131072), the last document, and a list over every 613th document"""
    n = tile + 37
    win = min(1 << 13, tile)
    edge = np.array([0, win - 1, win, 2 * win - 1, 2 * win, tile - 1, tile, n - 1], dtype=np.uint32)
    wide = np.union1d(np.arange(0, n, 613), edge).astype(np.uint32)
    ls = [(edge, np.full(len(edge), 2, np.uint32)), (wide, (1 + wide % 4).astype(np.uint32)), (np.array([win, tile], np.uint32), np.array([1, 1], np.uint32))]
    segments = [(n, (7 + np.arange(n) % 23).astype(np.uint32), ls)]
    one = [[(0, S, 0, 0)], [(1, S, 0, 0)], [(0, M, 0, 1), (1, M, 1, 1)], [(0, M, 0, 2), (1, M, 0, 2), (2, M, 0, 2)], [(1, S, 0, 0), (2, X, 0, 0)]]
    d = np.arange(n)
    tables = {"mixed": [(((d * 7) % 13) / 4.0).astype(np.float32)], "rough": [np.float32(0.5) + (((d * 37) % 101) / 101.0).astype(np.float32)],
              "edges first": [np.where(np.isin(d, edge), np.float32(4.0), np.float32(0.25)).astype(np.float32)]}
    return segments, [[(0, li, r, c, m) for li, r, c, m in q] for q in one], [[1.5, 1.1, 2.0]], [[1.0, 0.75, 1.0]], tables, edge


def run_product_tile():
    """the product build's window and tile: docIds 8191 | 8192 and 131071 | 131072"""
    tile = nsbind.facet_tile_docs()
    segments, queries, idfs, weights, tables, edge = product_inputs(tile)
    fam = Family(segments, queries, idfs, weights, tables=tables)
    try:
        assert fam.founds[0] == len(edge) and fam.founds[1] > 200 and fam.founds[2] == len(edge) and fam.founds[3] == len(edge) and fam.founds[4] == fam.founds[1] - 2
        assert {int(r[2]) for r in fam.rows("edges first")[1][:len(edge)]} == set(edge.tolist())      # the factors lift the edge documents to the top
        for name in tables:
            for k in (1, 65, 100):
                Boosted(fam, name).check(("boost product tile", tile, name), k)
        side = Boosted(fam, "mixed", queries=[1])
        assert after_shapes.walk(("boost product walk",), side, 100) == -(-fam.founds[1] // 100) + 1
    finally:
        fam.release()
    return tile, int(segments[0][0])


# ---- refusals -----------------------------------------------------------------------------------------------------------
def run_refusals():
    """at upload: NaN, +inf, -inf, a negative factor and -0.0f are refused and nothing is left; 0.0f, the smallest denormal and the
    largest finite value are legal.  At the call: a NULL entry, a short table, a table of another ctx; the sibling's refusals
    unchanged and first.  A refused call writes nothing."""
    import ctypes as Ct

    L = nsbind.hip_lib()
    fam = directed_family(3)
    ctx, order = fam.segs.ctx, fam.order
    other = Ct.c_void_p()
    extra = []
    try:
        for bad in (np.nan, np.inf, -np.inf, -1.0, -0.0, -1e-45):
            for at in (0, 31, 255, 256, N_DOCS - 1):
                t = np.ones(N_DOCS, np.float32)
                t[at] = bad
                rc, h = nsbind.docboost_upload(ctx, t)
                msg = L.ns_last_error(ctx).decode()
                assert rc == NS_E_INVAL and h.value is None and "ns_docboost_upload: a document has a factor that is not finite or has its sign bit set" in msg, (bad, at, rc, msg)
        t = np.ones(N_DOCS, np.float32)
        t.view(np.uint32)[7] = 0x7FC00001                                        # a NaN with a payload
        assert nsbind.docboost_upload(ctx, t)[0] == NS_E_INVAL
        legal = np.array([0.0, 1e-45, np.finfo(np.float32).max, 1.0], np.float32)
        rc, h = nsbind.docboost_upload(ctx, legal)
        assert rc == 0, L.ns_last_error(ctx).decode()
        extra.append(h)
        rc, h = nsbind.docboost_upload(ctx, np.zeros(0, np.float32))              # an empty table is a table
        assert rc == 0
        extra.append(h)
        assert L.ns_docboost_upload(ctx, 5, None, Ct.byref(Ct.c_void_p())) == NS_E_INVAL and L.ns_docboost_upload(ctx, 0, None, None) == NS_E_INVAL
        assert L.ns_docboost_upload(None, 0, None, Ct.byref(Ct.c_void_p())) == NS_E_INVAL
        assert L.ns_docboost_release(ctx, None) == NS_E_INVAL

        side = Boosted(fam, "mixed")

        def refused(rc, outs, match):
            if match is None:
                assert rc == 0, L.ns_last_error(ctx).decode()
                return
            msg = L.ns_last_error(ctx).decode()
            assert rc == NS_E_INVAL and "ns_search_boosted_after: " in msg and match in msg, (rc, msg)
            for o in outs:
                fill = 0xAB if o.dtype == nsbind.HIT_DTYPE else 0xABABABAB
                assert np.all((o.view(np.uint8) if o.dtype == nsbind.HIT_DTYPE else o) == fill), "a refused call writes nothing"

        def call(match, boosts="own", roles=fam.roles, clauses=fam.clauses, needs=fam.needs, cursors=None):
            rc, *outs = nsbind.search_boosted_after_raw(ctx, fam.qd, fam.refs, roles, clauses, needs, 10, cursors, order, fam.handles,
                                                       fam.boosts("mixed") if isinstance(boosts, str) else boosts)
            refused(rc, outs[:4], match)

        good = fam.boosts("mixed")
        call(None)
        call("segment or boost table 1 is NULL", boosts=[good[0], None, good[2]])
        call("boost table 2 has 4 factors, its segment has 300 documents", boosts=[good[0], good[1], extra[0]])
        call("boost table 0 has 0 factors", boosts=[extra[1], good[1], good[2]])
        rc, long_table = nsbind.docboost_upload(ctx, np.ones(N_DOCS + 50, np.float32))    # longer than the segment: served
        assert rc == 0
        extra.append(long_table)
        call(None, boosts=[good[0], long_table, good[2]])
        assert L.ns_ctx_create(0, Ct.byref(other)) == 0
        rc, foreign = nsbind.docboost_upload(other, np.ones(N_DOCS, np.float32))
        assert rc == 0
        call("boost table 1 does not belong to this ctx", boosts=[good[0], foreign, good[2]])
        assert L.ns_docboost_release(ctx, foreign) == NS_E_INVAL and L.ns_docboost_release(other, foreign) == 0
        # the sibling's refusals, under this call's name, with tables given
        q2 = NAMES.index("quorum: two of three")
        first = int(fam.qd[q2]["term_begin"])
        eight = fam.needs.copy()
        eight[first] = 8
        call("ref %d: a need of 8 (query %d); at most 7" % (first, q2), needs=eight)
        call("needs without clauses", clauses=None)
        bad = fam.roles.copy()
        bad[first] = 3
        call("ref %d: role 3 is none of" % first, roles=bad)
        cu = nsbind.cursors([(0, 9, 0)] + [None] * (len(fam.qd) - 1))
        call("query 0: cursor names segment 9, which the call does not list", cursors=cu)
        cu = nsbind.cursors([None] * len(fam.qd))
        cu["set"][1] = 2
        call("query 1: cursor with set = 2", cursors=cu)
        assert L.ns_search_boosted_after(ctx, None, 0, None, None, None, None, 0, 10, None, None, None, None, 0, None, None, None, None, None) == 0
        assert L.ns_search_boosted_after(None, None, 0, None, None, None, None, 0, 10, None, None, None, None, 0, None, None, None, None, None) == NS_E_INVAL
        out2 = (Ct.c_float * 2)()
        assert L.ns_boosted_kernel_ms(out2, 1) == 0 and out2[0] > 0.0 and out2[1] > 0.0 and L.ns_boosted_kernel_ms(None, 0) == NS_E_INVAL
        del side
    finally:
        for h in extra:
            assert nsbind.docboost_release(ctx, h) == 0
        if other:
            L.ns_ctx_destroy(other)
        fam.release()


def main(out_path):
    """child process at NS_FACET_TILE_DOCS = 128 and NS_BOOL_WIN_DOCS = 32.  Both builds run the directed families; the counting
    build reports the counters of those and of one cursor call; the variants build runs the walks, the cursors, the dialects, the
    filter and the equivalences."""
    counting = "ns_debug_boolean_boost_counters" in nsbind.debug_counters(reset=True)
    assert os.environ.get("NS_BOOL_WIN_DOCS") == str(SMALL_WIN)
    rep = {"tile": run_directed(1, tile_expected=SMALL_TILE), "counting": counting}
    run_directed(3)
    if counting:
        def events():
            c = nsbind.debug_counters(reset=True)
            return dict(zip(EVENTS, c["ns_debug_boolean_boost_counters"]), select_items=c["ns_debug_boolean_counters"][0])

        rep["events_directed"] = events()
        run_cursors()
        rep["events_cursors"] = events()
        run_dialects()
        rep["events_dialects"] = events()
        print("boost", rep["events_directed"], rep["events_cursors"], rep["events_dialects"], flush=True)
    else:
        rep["pages"] = run_walks()
        run_cursors()
        run_dialects()
        run_filter()
        rep["ones"] = run_null_and_ones_are_the_sibling()
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print("boost shapes OK")


if __name__ == "__main__":
    main(sys.argv[1])
