"""Directed inputs of ns_search_grouped_after, ns_facet_count_grouped and ns_search_sorted_grouped (the GROUPED instantiations in
csrc/ns_boolean.hip and csrc/ns_boolean_sets.hip) and the code that runs them through the raw C-ABI against the
restatement (tests/grouped_ref.py).  The shapes are the boolean suites': 300 documents per segment, one segment and three
listed as 2, 0, 1, facet_shapes.small_lists(), boolean_sets_shapes' bucket tables and key patterns.  All comparisons are exact,
score bits included.

Imported by tests/test_grouped_gpu.py for the product library (one tile and one window hold a 300-document segment; a family of
two product tiles + 5 documents puts a clause's two lists on either side of a tile edge), and run as a program in a child
process that loaded the variants or the counting build with NS_FACET_TILE_DOCS=128 NS_BOOL_WIN_DOCS=32: there 300 documents are
two whole tiles and a part, four windows each, a clause hits a tile but misses a window, and the counting build reports which
paths of the grouped required stage the inputs reached."""
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
import boolean_sets_ref  # noqa: E402
import boolean_sets_shapes as bss  # noqa: E402
import boolean_shapes  # noqa: E402
import facet_shapes  # noqa: E402
import grouped_ref  # noqa: E402
import nsbind  # noqa: E402
from boolean_ref import MUST, NOT, SHOULD  # noqa: E402

ASC = nsbind.NS_SORT_ASC
NS_E_INVAL = -1
SMALL_TILE, SMALL_WIN, N_DOCS = boolean_shapes.SMALL_TILE, boolean_shapes.SMALL_WIN, boolean_shapes.N_DOCS
KS = [1, 10, 63, 64, 65, 100]                 # 64 / 65: the boundary between the kept set's two registers
BUCKETS = [1, 50, 1024]
WALK_KS = [1, 10, 64]
S, M, X = SHOULD, MUST, NOT
EVENTS = nsbind.GROUPED_EVENTS                # ns_debug_boolean_groups_counters, in order (counting build)

# Over facet_shapes.small_lists(): 0 empty, 1 {0}, 2 .. 6 of 63, 64, 65, 128 and 257 postings (6 with docId 305 >= n_docs), 7 in
# the middle 128-document tile alone, 8 on the rim alone.  (list, role, clause) per ref; the names are the issue's: 7M0 = list 7,
# MUST, clause 0.  test_grouped_cpu asserts through the restatement that every case has the property its name claims.
CASES = {
    "every tile is hit by one member and missed by the other": [(7, M, 0), (8, M, 0)],
    "a two-list clause first": [(7, M, 0), (8, M, 0), (5, M, 1)],
    "a two-list clause second": [(5, M, 0), (7, M, 1), (8, M, 1)],
    "clause 0 misses the last tile, clause 1 hits it": [(7, M, 0), (1, M, 0), (6, M, 1)],
    "an empty member is dropped": [(0, M, 0), (5, M, 0), (6, S, 0)],
    "a dead clause": [(0, M, 0), (0, M, 0), (5, S, 0)],
    "sparse unordered ids, interleaved roles": [(2, M, 9), (3, S, 0), (4, M, 200), (5, X, 0), (6, M, 9), (7, M, 200)],
    "three clauses, then an exclusion": [(2, M, 0), (3, M, 0), (4, M, 1), (5, M, 1), (6, M, 2), (8, M, 2), (7, X, 0)],
    "a list in two clauses": [(4, M, 0), (5, M, 0), (4, M, 1), (6, M, 1)],
    "the member adds twice": [(4, M, 0), (5, M, 0), (4, S, 0)],
    "exclusion wins": [(4, M, 0), (5, M, 0), (4, X, 0)],
    "one survivor: the single-list path": [(0, M, 0), (6, M, 0)],
    "named twice in a clause: matched once, scored twice": [(6, M, 0), (6, M, 0)],
    "70 refs as one clause": [(2 + i % 7, M, 0) for i in range(70)],
    "70 refs as 35 clauses of two": [(2 + i % 7, M, i // 2) for i in range(70)],
    "garbage clause values on SHOULD and NOT refs": [(2, M, 1), (3, S, 0xFFFF), (4, X, 1), (5, M, 1), (6, S, 1), (8, X, 0xABCD), (7, S, 40000)],
}
DIRECTED = [[]] + list(CASES.values())
NAMES = ["no ref"] + list(CASES)


class Family(boolean_shapes.Family):
    """uploaded segments + one call's descriptors, roles and clause values; the restatement's whole answer is computed once and
    kept.  queries: per query [(segment, list, role, clause)]"""

    def __init__(self, segments, queries, idfs, weights, seg_order=None, keys=None):
        super().__init__(segments, grouped_ref.strip(queries), idfs, weights, seg_order)
        self.grouped = queries
        self.clauses = np.array([c for q in queries for _, _, _, c in q], dtype=np.uint16)
        self.everything = grouped_ref.grouped_all(segments, queries, self.order, idfs, weights)
        self.founds = [len(r) for r in self.everything]
        self.handles = [self.segs.segs[s] for s in self.order]
        self.keys = bss.keys_for(segments, "pool5") if keys is None else keys
        self.key_tables, self._counts = None, {}

    def key_handles(self):
        if self.key_tables is None:
            self.key_tables = []
            for s in self.order:
                rc, h = nsbind.dockeys_upload(self.segs.ctx, self.keys[s])
                assert rc == 0, self.segs.err()
                self.key_tables.append(h)
        return self.key_tables

    def set_keys(self, keys):
        for h in self.key_tables or []:
            assert nsbind.dockeys_release(self.segs.ctx, h) == 0
        self.key_tables, self.keys = None, keys

    def count(self, tables, n_buckets, roles="own", clauses="own", sibling=False):
        """ns_facet_count_grouped (sibling: ns_facet_count_boolean) under freshly uploaded tables -> (rc, counts, found)"""
        ro = self.roles if isinstance(roles, str) else roles
        cl = self.clauses if isinstance(clauses, str) else clauses
        handles = []
        try:
            for s in self.order:
                rc, h = nsbind.facet_upload(self.segs.ctx, tables[s], n_buckets)
                assert rc == 0, self.segs.err()
                handles.append(h)
            if sibling:
                return nsbind.facet_count_boolean(self.segs.ctx, self.qd, self.refs, ro, self.order, self.handles, handles, n_buckets)[:3]
            return nsbind.facet_count_grouped(self.segs.ctx, self.qd, self.refs, ro, cl, self.order, self.handles, handles, n_buckets)[:3]
        finally:
            for h in handles:
                assert nsbind.facet_release(self.segs.ctx, h) == 0

    def check_counts(self, label, kind, n_buckets):
        tables = bss.tables_for(self.segments, kind, n_buckets)
        if (kind, n_buckets) not in self._counts:
            self._counts[(kind, n_buckets)] = grouped_ref.counts(self.segments, self.grouped, tables, n_buckets, self.order)
        rc, counts, found = self.count(tables, n_buckets)
        what = (label, kind, "B", n_buckets)
        assert rc == 0, what + (self.segs.err(),)
        np.testing.assert_array_equal(counts.astype(np.int64), self._counts[(kind, n_buckets)], err_msg=str(what))
        np.testing.assert_array_equal(found.astype(np.int64), self.founds, err_msg=str(what + ("found",)))

    def release(self):
        if self.segs.ctx:
            self.set_keys(self.keys)
        super().release()


class Ranked:
    """a Family in score order: what after_shapes.walk, check_call and run_cursor_rounds drive"""

    def __init__(self, fam, roles="own", clauses="own"):
        self.fam, self.roles, self.clauses = fam, roles, clauses
        self.rows = grouped_ref.score_rows(fam.everything, fam.order)

    def raw(self, k, cursors):
        fam = self.fam
        return nsbind.search_grouped_after_raw(fam.segs.ctx, fam.qd, fam.refs, fam.roles if isinstance(self.roles, str) else self.roles,
                                               fam.clauses if isinstance(self.clauses, str) else self.clauses, k,
                                               None if cursors is None else nsbind.cursors(cursors), fam.order, fam.handles)

    def call(self, k, cursors):
        """cursors: None, or per query None | (score bits, seg_id, doc)"""
        rc, hits, nhits, found, rest, _ = self.raw(k, cursors)
        assert rc == 0, self.fam.segs.err()
        return hits, None, nhits, found, rest

    def mapped(self, c):
        return None if c is None else (after_ref.ord32(c[0]), self.fam.order.index(c[1]), c[2])

    def next_cursor(self, hits, keys, q, n):
        h = hits[q, n - 1]
        return (int(h["score"].view(np.uint32)), int(h["seg"]), int(h["doc"]))

    def check(self, label, k, cursors=None):
        out = self.call(k, cursors)
        after_shapes.check_call(label, self, k, cursors, out)
        return out


class Dated:
    """a Family in date order under one direction"""

    def __init__(self, fam, flags, roles="own", clauses="own"):
        self.fam, self.flags, self.roles, self.clauses = fam, flags, roles, clauses
        self.rows = boolean_sets_ref.rows(fam.everything, fam.keys, bool(flags & ASC), fam.order)

    def raw(self, k, cursors):
        fam = self.fam
        return nsbind.search_sorted_grouped_raw(fam.segs.ctx, fam.qd, fam.refs, fam.roles if isinstance(self.roles, str) else self.roles,
                                                fam.clauses if isinstance(self.clauses, str) else self.clauses, k, self.flags,
                                                None if cursors is None else nsbind.cursors(cursors), fam.order, fam.handles, fam.key_handles())

    def call(self, k, cursors):
        """cursors: None, or per query None | (key as uploaded, seg_id, doc)"""
        rc, hits, keys, nhits, found, rest, _ = self.raw(k, cursors)
        assert rc == 0, self.fam.segs.err()
        return hits, keys, nhits, found, rest

    def mapped(self, c):
        return None if c is None else (after_ref.sort_rank(c[0], bool(self.flags & ASC)), self.fam.order.index(c[1]), c[2])

    def next_cursor(self, hits, keys, q, n):
        h = hits[q, n - 1]
        return (int(keys[q, n - 1]), int(h["seg"]), int(h["doc"]))

    def check(self, label, k, cursors=None):
        out = self.call(k, cursors)
        after_shapes.check_call((label, "flags", hex(self.flags)), self, k, cursors, out)
        return out


def directed_inputs(n_segs):
    """DIRECTED over one or three segments of 300 documents -> (segments, queries, idfs, weights, seg_order): with three segments
    the refs of a query interleave the segments, the call lists them as 2, 0, 1, and in segment 1 list 5 stands in for the empty
    list 0 as a MUST ref (boolean_sets_shapes.directed_inputs' substitution), so that the dead clause is dead in two segments only"""
    lists = facet_shapes.small_lists()
    segments = [(N_DOCS, (5 + (np.arange(N_DOCS) * (1 + 2 * s)) % 41).astype(np.uint32), lists) for s in range(n_segs)]
    queries = []
    for q in DIRECTED:
        refs = []
        for li, role, clause in q:
            for s in range(n_segs):
                refs.append((s, 5 if (s == 1 and li == 0 and role == M and len(q) > 1) else li, role, clause))
        queries.append(refs)
    idf, w = boolean_shapes.small_weights(len(lists))
    return segments, queries, [idf] * n_segs, [w] * n_segs, ([2, 0, 1] if n_segs == 3 else None)


def directed_family(n_segs, pattern="pool5"):
    segments, queries, idfs, weights, order = directed_inputs(n_segs)
    return Family(segments, queries, idfs, weights, seg_order=order, keys=bss.keys_for(segments, pattern))


def run_directed(n_segs, tile_expected=None):
    """every directed case at B = 1, 50, 1024, K = 1 .. 100 in score order and in both date directions, without and with skip
    tables"""
    tile = nsbind.facet_tile_docs()
    if tile_expected is not None:
        assert tile == tile_expected, (tile, tile_expected)
    fam = directed_family(n_segs)
    try:
        for with_skips in (False, True):
            if with_skips:
                for s in range(n_segs):
                    assert facet_shapes.build_skips(fam.segs, s) == 4
            label = ("grouped directed", n_segs, "skips", with_skips)
            for B in BUCKETS:
                for kind in ("modulo", "tile"):
                    fam.check_counts(label, kind, B)
            ranked = Ranked(fam)
            sides = [Dated(fam, 0), Dated(fam, ASC)]
            for k in KS:
                ranked.check(label, k)
                for side in sides:
                    side.check(label, k)
        assert 0 in fam.founds and max(fam.founds) > 100 and len(set(fam.founds)) >= 8, fam.founds
    finally:
        fam.release()
    return tile


def run_walks(ks=WALK_KS):
    """score order and date order paged to exhaustion: per query the pages concatenated are the full ranking, nothing twice, rest
    counting down to 0 (after_shapes.walk asserts each).  K = 1 on one segment (date order under equal keys: the docId decides
    every page), K = 10 and 64 on three segments, date order in both directions."""
    pages = {}
    for k in ks:
        fam = directed_family(1, "same") if k == 1 else directed_family(3)
        try:
            assert max(fam.founds) > 100 and min(fam.founds) == 0
            pages[("score", k)] = after_shapes.walk(("grouped walk", "score"), Ranked(fam), k)
            for flags in ((0,) if k == 1 else (0, ASC)):
                pages[("date", k, flags)] = after_shapes.walk(("grouped walk", "date", hex(flags)), Dated(fam, flags), k)
        finally:
            fam.release()
    return pages


def run_cursors():
    """cursors that are no document of the matched set, or no document at all, on the three-segment directed family: after_shapes'
    cursor rounds against the restatement, in score order and in both date directions (fifty even key values, some undated)"""
    segments, queries, idfs, weights, order = directed_inputs(3)
    keys = [np.where(np.arange(s[0]) % 9 == 4, 0, 20200101 + 2 * (np.arange(s[0]) % 50)).astype(np.uint32) for s in segments]
    fam = Family(segments, queries, idfs, weights, seg_order=order, keys=keys)
    try:
        side = Ranked(fam)

        def between(rows):
            have = {r[4] for r in rows}
            return [b for b in sorted({r[4] + 1 for r in rows} | {r[4] - 1 for r in rows if r[4]}) if b not in have][:4]

        bits = after_shapes.BITS
        specials = [(n, (bits[n], order[1], 128)) for n in ("+0", "-0", "+inf", "-inf")]
        specials += [("above everything", (bits["top"], order[0], 0)), ("below everything", (bits["bottom"], order[-1], 0xFFFFFFFF))]
        after_shapes.run_cursor_rounds("grouped cursors", side, after_shapes.arbitrary_cursors(side, lambda r: r[4], between), specials, 10)
        plain = side.call(100, None)
        for cursors in ([(bits["top"], order[0], 0)] * len(side.rows), [None] * len(side.rows)):
            for a, b in zip(plain, side.call(100, cursors)):
                assert a is b is None or a.tobytes() == b.tobytes(), "a cursor above everything, or every cursor unset"
        assert plain[4].tobytes() == plain[3].tobytes()                                # no cursor: rest = found
        _, _, nhits, found, rest = side.call(100, [(bits["bottom"], order[-1], 0xFFFFFFFF)] * len(side.rows))
        assert not np.any(nhits) and not np.any(rest) and list(found) == fam.founds
        for flags in (0, ASC):
            side = Dated(fam, flags)
            per_query = after_shapes.arbitrary_cursors(side, lambda r: r[4], lambda rows: sorted({r[4] + 1 for r in rows if r[4]})[:4])
            specials = [("undated", (0, order[1], 128)), ("key 1", (1, order[1], 128)), ("largest key", (0xFFFFFFFE, order[0], 0)),
                        ("below everything", (0, order[-1], 0xFFFFFFFF))]
            after_shapes.run_cursor_rounds(("grouped date cursors", hex(flags)), side, per_query, specials, 10)
            _, _, nhits, found, rest = side.call(100, [(0, order[-1], 0xFFFFFFFF)] * len(side.rows))
            assert not np.any(nhits) and not np.any(rest) and list(found) == fam.founds
    finally:
        fam.release()


def product_inputs(tile):
    """n_docs = two tiles + 5.  Lists 0 and 1 lie on either side of the first tile edge, 2 and 3 on either side of the second;
    list 4 is spread over everything with a posting at every edge, list 5 is every 997th document."""
    n = 2 * tile + 5
    rng = np.random.default_rng(37)
    edges = np.array([0, tile - 1, tile, 2 * tile - 1, 2 * tile, n - 1])
    docs = [np.arange(tile - 60, tile), np.arange(tile, tile + 20), np.arange(2 * tile - 7, 2 * tile), np.arange(2 * tile, n),
            np.union1d(rng.choice(n, 400, replace=False), np.concatenate([edges, np.arange(tile - 30, tile + 10), np.arange(2 * tile - 4, n - 2)])),
            np.arange(0, n, 997)]
    lists = [(x.astype(np.uint32), (1 + x % 3).astype(np.uint32)) for x in docs]
    segments = [(n, np.full(n, 11, np.uint32), lists)]
    one = [[(0, M, 0), (1, M, 0)], [(0, M, 0), (1, M, 0), (4, M, 1)], [(4, M, 0), (0, M, 1), (1, M, 1)], [(0, M, 3), (1, M, 3), (2, M, 3), (3, M, 3)],
           [(0, M, 0), (1, M, 0), (2, M, 0), (3, M, 0), (4, M, 1), (5, S, 0)], [(0, M, 0), (1, M, 0), (4, X, 0)], [(2, M, 0), (3, M, 0), (4, M, 1), (0, S, 0)],
           [(0, M, 0), (1, M, 1)], [(4, M, 0), (5, M, 0), (4, M, 1), (0, M, 1)]]
    queries = [[(0, li, r, c) for li, r, c in q] for q in one]
    idf, w = boolean_shapes.small_weights(len(lists))
    return segments, queries, [idf], [w], docs


def run_product_tile():
    """the product build's tile: a clause whose two lists lie on either side of a tile edge, in score order, in date order under
    equal keys (the docId decides across the edge) and in facet counts; a cursor at each edge"""
    tile = nsbind.facet_tile_docs()
    segments, queries, idfs, weights, docs = product_inputs(tile)
    n = int(segments[0][0])
    fam = Family(segments, queries, idfs, weights, keys=bss.keys_for(segments, "same"))
    try:
        assert fam.founds[0] == 80 and fam.founds[3] == 60 + 20 + 7 + 5 and fam.founds[7] == 0 and fam.founds[1] == 40 and fam.founds[2] == 40, fam.founds
        d = np.arange(n, dtype=np.int64)
        for with_skips in (False, True):
            if with_skips:
                assert facet_shapes.build_skips(fam.segs, 0) >= 1
            for B, table in ((50, ((d * 7919) % 50).astype(np.uint16)), (1024, (d // tile).astype(np.uint16))):
                rc, counts, found = fam.count([table], B)
                assert rc == 0, fam.segs.err()
                np.testing.assert_array_equal(counts.astype(np.int64), grouped_ref.counts(segments, queries, [table], B))
                np.testing.assert_array_equal(found.astype(np.int64), fam.founds)
            for k in (1, 64, 65, 100):
                Ranked(fam).check(("grouped product tile", tile, with_skips), k)
                Dated(fam, 0).check(("grouped product tile", tile, with_skips), k)
        side = Dated(fam, ASC)
        for at in (tile - 1, tile, 2 * tile - 1, 2 * tile, n - 1):
            side.check(("grouped product edges", at), 100, [(20200101, 0, at)] * len(queries))
    finally:
        fam.release()
    return tile, n


# ---- equivalences on the same raw inputs --------------------------------------------------------------------------------
FLOOR_DISTINCT = 40          # queries with found >= 2 that the all-distinct comparison must cover (test_grouped_cpu counts them)
FLOOR_ONE_CLAUSE = boolean_shapes.FLOOR_SAME_ROLE[S]


def distinct_inputs():
    """the three role-mix families of the boolean sets suite, each as (segments, boolean queries, idfs, weights, seg_order)"""
    return [bss.directed_inputs(1), bss.directed_inputs(3), bss.mixed_inputs()]


def distinct_clauses(queries):
    """a clause value per ref, different for every ref of a query, neither dense nor ordered"""
    return [[(s, li, r, (60000 - 777 * i) % 65536) for i, (s, li, r) in enumerate(q)] for q in queries]


def same_bytes(label, got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), (label, "output", i)


def compare_with_siblings(label, fam, roles, clauses, sib_roles):
    """the three grouped calls under (roles, clauses) against the three boolean siblings under sib_roles: every output array, byte
    for byte, with and without cursors"""
    ctx = fam.segs.ctx
    for B in (50, 1024):
        tables = bss.tables_for(fam.segments, "modulo", B)
        rc, counts, found = fam.count(tables, B, roles=roles, clauses=clauses)
        assert rc == 0, fam.segs.err()
        rc, w_counts, w_found = fam.count(tables, B, roles=sib_roles, sibling=True)
        assert rc == 0, fam.segs.err()
        same_bytes(label + ("facets", B), (counts, found), (w_counts, w_found))
    Q = len(fam.qd)
    for k in (7, 64, 100):
        for cursors in (None, "page 2"):
            cu = None
            if cursors:
                rc, hits, nhits, *_ = nsbind.search_boolean_after_raw(ctx, fam.qd, fam.refs, sib_roles, k, None, fam.order, fam.handles)
                assert rc == 0
                cu = nsbind.cursors([None if not nhits[q] else (int(hits[q, nhits[q] - 1]["score"].view(np.uint32)), int(hits[q, nhits[q] - 1]["seg"]),
                                                             int(hits[q, nhits[q] - 1]["doc"])) for q in range(Q)])
            rc, *want = nsbind.search_boolean_after_raw(ctx, fam.qd, fam.refs, sib_roles, k, cu, fam.order, fam.handles)
            assert rc == 0, fam.segs.err()
            rc, *got = nsbind.search_grouped_after_raw(ctx, fam.qd, fam.refs, roles, clauses, k, cu, fam.order, fam.handles)
            assert rc == 0, fam.segs.err()
            same_bytes(label + ("score", k, cursors), got[:4], want[:4])
            for flags in (0, ASC):
                cu = None
                if cursors:
                    rc, hits, keys, nhits, *_ = nsbind.search_sorted_boolean_raw(ctx, fam.qd, fam.refs, sib_roles, k, flags, None, fam.order, fam.handles, fam.key_handles())
                    assert rc == 0
                    cu = nsbind.cursors([None if not nhits[q] else (int(keys[q, nhits[q] - 1]), int(hits[q, nhits[q] - 1]["seg"]), int(hits[q, nhits[q] - 1]["doc"]))
                                         for q in range(Q)])
                rc, *want = nsbind.search_sorted_boolean_raw(ctx, fam.qd, fam.refs, sib_roles, k, flags, cu, fam.order, fam.handles, fam.key_handles())
                assert rc == 0, fam.segs.err()
                rc, *got = nsbind.search_sorted_grouped_raw(ctx, fam.qd, fam.refs, roles, clauses, k, flags, cu, fam.order, fam.handles, fam.key_handles())
                assert rc == 0, fam.segs.err()
                same_bytes(label + ("date", k, flags, cursors), got[:5], want[:5])


def run_distinct_clauses_equal_the_siblings():
    """every MUST ref a clause of its own == ns_search_boolean_after, ns_facet_count_boolean, ns_search_sorted_boolean"""
    covered = 0
    for i, (segments, queries, idfs, weights, order) in enumerate(distinct_inputs()):
        fam = Family(segments, distinct_clauses(queries), idfs, weights, seg_order=order)
        try:
            for with_skips in (False, True):
                if with_skips:
                    for s in range(len(segments)):
                        facet_shapes.build_skips(fam.segs, s)
                compare_with_siblings(("distinct", i, with_skips), fam, fam.roles, fam.clauses, fam.roles)
            covered += sum(f >= 2 for f in fam.founds)
        finally:
            fam.release()
    assert covered >= FLOOR_DISTINCT, covered
    return covered


def run_one_clause_equals_roles_null():
    """every ref MUST in ONE clause == the sibling under roles == NULL (every ref SHOULD): the union, scored over every ref"""
    segments, queries, idfs, weights = boolean_shapes.same_role_inputs(M)
    fam = Family(segments, [[(s, li, r, 4242) for s, li, r in q] for q in queries], idfs, weights, seg_order=[2, 0, 1])
    try:
        covered = sum(f >= 2 for f in fam.founds)
        assert covered >= FLOOR_ONE_CLAUSE, covered
        compare_with_siblings(("one clause",), fam, fam.roles, fam.clauses, None)
    finally:
        fam.release()
    return covered


def run_clauses_null_is_the_sibling():
    segments, queries, idfs, weights, order = bss.mixed_inputs()
    fam = Family(segments, distinct_clauses(queries), idfs, weights, seg_order=order)
    try:
        compare_with_siblings(("clauses NULL",), fam, fam.roles, None, fam.roles)
        # roles == NULL: no ref is MUST, the clause values are never read
        compare_with_siblings(("roles NULL",), fam, None, fam.clauses, None)
    finally:
        fam.release()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def run_refusals():
    """the siblings' refusals under the new names: NS_E_INVAL with the message, nothing launched, the outputs keep their fill"""
    import ctypes as C

    from rawseg import RawSegments

    L = nsbind.hip_lib()
    segments, queries, idfs, weights, order = bss.mixed_inputs()
    fam = Family(segments, distinct_clauses(queries), idfs, weights, seg_order=order)
    other = RawSegments(segments[:1])
    ctx, Q, B = fam.segs.ctx, len(fam.qd), 50
    tabs = [nsbind.facet_upload(ctx, t, B)[1] for t in [bss.tables_for(segments, "modulo", B)[s] for s in order]]
    try:
        def message(match):
            msg = L.ns_last_error(ctx).decode()
            assert match in msg, msg

        def refused(name, rc, outs, match):
            if match is None:
                assert rc == 0, L.ns_last_error(ctx).decode()
                return
            assert rc == NS_E_INVAL, rc
            message(name + ": ")
            message(match)
            for o in outs:
                fill = 0xAB if o.dtype == nsbind.HIT_DTYPE else 0xABABABAB                # nsbind's fill of the output arrays
                assert np.all((o.view(np.uint8) if o.dtype == nsbind.HIT_DTYPE else o) == fill), "a refused call writes nothing"

        def ranked(match, refs=fam.refs, roles=fam.roles, after=None, hs=None, flags=None):
            rc, *outs = nsbind.search_grouped_after_raw(ctx, fam.qd, refs, roles, fam.clauses, 10, after, order, fam.handles if hs is None else hs)
            refused("ns_search_grouped_after", rc, outs[:4], match)

        def count(match, refs=fam.refs, roles=fam.roles, after=None, hs=None, flags=None):
            rc, *outs = nsbind.facet_count_grouped(ctx, fam.qd, refs, roles, fam.clauses, order, fam.handles if hs is None else hs, tabs, B)
            refused("ns_facet_count_grouped", rc, outs[:2], match)

        def dated(match, refs=fam.refs, roles=fam.roles, after=None, hs=None, flags=0):
            rc, *outs = nsbind.search_sorted_grouped_raw(ctx, fam.qd, refs, roles, fam.clauses, 10, flags, after, order, fam.handles if hs is None else hs, fam.key_handles())
            refused("ns_search_sorted_grouped", rc, outs[:5], match)

        for call in (ranked, count, dated):
            call(None)
            bad = fam.roles.copy()
            bad[3] = 3
            call("ref 3: role 3 is none of NS_ROLE_SHOULD, NS_ROLE_MUST, NS_ROLE_NOT", roles=bad)
            past = fam.refs.copy()
            past["byte_off"][0] = 8 * 10 ** 6
            call("runs past the postings", refs=past)
            odd = fam.refs.copy()
            odd["byte_off"][0] += 4
            call("ref 0: byte offset", refs=odd)
            scoring = int(np.flatnonzero(fam.roles != X)[0])
            nan = fam.refs.copy()
            nan["idf"][scoring] = np.nan
            call("ref %d: idf or qweight is not finite" % scoring, refs=nan)
            excluded = int(np.flatnonzero(fam.roles == X)[0])
            nan = fam.refs.copy()
            nan["idf"][excluded] = np.nan
            call(None, refs=nan)                                                   # under NOT the numbers are never read
            alien = fam.refs.copy()
            alien["seg_id"][1] = 9
            call("ref 1 names segment 9, which the call does not list", refs=alien)
            call("segment 0 is not a published segment of this ctx", hs=[other.segs[0]] + fam.handles[1:])
        for flags in (nsbind.NS_FLAG_AND, 0x2000):
            dated("flags 0x%x: only NS_SORT_ASC is known" % flags, flags=flags)
        ok = nsbind.cursors([(20200101, 2, 5)] * Q)
        for call in (ranked, dated):
            call(None, after=ok)
            alien = ok.copy()
            alien["seg"][1] = 7
            call("query 1: cursor names segment 7, which the call does not list", after=alien)
            two = ok.copy()
            two["set"][3] = 2
            call("query 3: cursor with set = 2 (0 or 1)", after=two)
        # no queries: NS_OK, nothing touched, whatever else is passed; no ctx: refused
        assert L.ns_search_grouped_after(ctx, None, 0, None, None, None, 0, 10, None, None, None, 0, None, None, None, None, None) == 0
        assert L.ns_facet_count_grouped(ctx, None, 0, None, None, None, 0, None, None, None, 0, None, None, None) == 0
        assert L.ns_search_sorted_grouped(ctx, None, 0, None, None, None, 0, 10, 0, None, None, None, None, 0, None, None, None, None, None, None) == 0
        assert L.ns_search_grouped_after(None, None, 0, None, None, None, 0, 10, None, None, None, 0, None, None, None, None, None) == NS_E_INVAL
        assert L.ns_facet_count_grouped(None, None, 0, None, None, None, 0, None, None, None, 0, None, None, None) == NS_E_INVAL
        # the kernel times of the calls that were given clauses, apart from the siblings'
        out6, out2 = (C.c_float * 6)(), (C.c_float * 2)()
        assert L.ns_grouped_kernel_ms(out6, 1) == 0 and all(v > 0.0 for v in out6), list(out6)
        assert L.ns_boolean_kernel_ms(out2, 1) == 0
        ranked(None)
        assert L.ns_boolean_kernel_ms(out2, 1) == 0 and all(v == 0.0 for v in out2), list(out2)
        assert L.ns_grouped_kernel_ms(out6, 1) == 0 and out6[0] > 0.0 and out6[1] > 0.0 and all(v == 0.0 for v in out6[2:]), list(out6)
        assert L.ns_grouped_kernel_ms(out6, 0) == 0 and all(v == 0.0 for v in out6)
        assert L.ns_grouped_kernel_ms(None, 0) == NS_E_INVAL
    finally:
        for h in tabs:
            nsbind.facet_release(ctx, h)
        other.release()
        fam.release()


def main(out_path):
    """child process at NS_FACET_TILE_DOCS = 128 and NS_BOOL_WIN_DOCS = 32.  Both builds run the directed families; the counting
    build reports the counters of those; the variants build runs the walks, the cursor rounds and the equivalences."""
    counting = "ns_debug_boolean_groups_counters" in nsbind.debug_counters(reset=True)
    assert os.environ.get("NS_BOOL_WIN_DOCS") == str(SMALL_WIN)
    rep = {"tile": run_directed(1, tile_expected=SMALL_TILE), "counting": counting}
    run_directed(3)
    if counting:
        rep["events"] = nsbind.grouped_counters(reset=True)
        rep["missed"] = [e for e in EVENTS if rep["events"][e] == 0]
        print("grouped", rep["events"], flush=True)
    else:
        rep["pages"] = {str(k): v for k, v in run_walks().items()}
        run_cursors()
        rep["distinct"] = run_distinct_clauses_equal_the_siblings()
        rep["one_clause"] = run_one_clause_equals_roles_null()
        run_clauses_null_is_the_sibling()
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print("grouped shapes OK")


if __name__ == "__main__":
    main(sys.argv[1])
