"""Directed inputs of ns_facet_count_boolean and ns_search_sorted_boolean (csrc/ns_boolean_sets.hip) and the code
that runs them through the raw C-ABI against the restatement (tests/boolean_sets_ref.py).  The shapes are boolean_shapes'
directed families (300 documents per segment, one and three segments, lists of 0 .. 257 postings, queries of 0, 1, 2, 3, 4, 8
and 70 refs per segment) with a few role mixes added, facet_shapes' bucket tables and sorted_shapes' key patterns.  All
comparisons are exact, score bits included.

Imported by tests/test_boolean_sets_gpu.py for the product library (one tile holds a 300-document segment; a family of two
product tiles + 5 documents hits the product's tile edges), and run as a program in a child process that loaded the variants
or the counting build with NS_FACET_TILE_DOCS=128: there 300 documents are two whole tiles and a part, and the counting build
reports which paths of the three kernels the inputs reached."""
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
import boolean_ref  # noqa: E402
import boolean_sets_ref  # noqa: E402
import boolean_shapes  # noqa: E402
import facet_shapes  # noqa: E402
import nsbind  # noqa: E402
import sorted_shapes  # noqa: E402
from boolean_ref import MUST, NOT, SHOULD  # noqa: E402

AND, ASC = nsbind.NS_FLAG_AND, nsbind.NS_SORT_ASC
NS_E_INVAL = -1
SMALL_TILE, N_DOCS = boolean_shapes.SMALL_TILE, boolean_shapes.N_DOCS
KS = [1, 10, 63, 64, 65, 100]                 # 64 / 65: the boundary between the kept set's two registers
BUCKETS = [1, 50, 1024]
WALK_KS = [1, 10, 64]
CAND_BYTES = 64 << 20                          # kSdCandBytes
S, M, X = SHOULD, MUST, NOT
# name -> index of ns_debug_boolean_sets_counters (counting build)
EVENTS = {"items": 0, "single_list_items": 1, "must_intersections": 2, "must_early_outs": 3, "exclusions_that_cleared": 4,
          "empty_after_exclusion": 5, "flushed_entries": 6, "chunks_skipped": 7, "chunks_inserted": 8, "score_found": 9,
          "score_not_found": 10, "score_not_refs_skipped": 11}

# Over facet_shapes.small_lists() (see boolean_shapes.DIRECTED), what that list leaves out; (list, role) per ref.
EXTRA = [
    [(6, M), (5, M), (4, M), (3, X)],          # three MUST lists, then the exclusion: the scratch bitmap was cleared twice before
    [(7, S), (8, S), (7, X)],                  # the exclusion removes every matched document of the middle small tile alone
    [(6, M), (8, M)], [(8, M), (6, S)],        # a MUST list without a posting in the middle small tile
    [(6, S), (2, X)], [(6, M), (2, X)],        # one positive ref and an exclusion: not the single-list path
    [(5, S), (6, S), (5, X)],                  # a list named as SHOULD and as NOT, next to another SHOULD list
    [(4, M), (4, S), (3, X)],                  # a list named as MUST and as SHOULD, with an exclusion
]
ROLE_MIXES = boolean_shapes.DIRECTED + EXTRA
# where in ROLE_MIXES the cases stand that the suite promises (test_boolean_sets_cpu checks them against the restatement)
CASES = {
    "one MUST + NOT": [(2, M), (3, X)], "two MUST + NOT": [(6, M), (5, M), (4, X)], "three MUST + NOT": EXTRA[0], "SHOULD + NOT": [(2, S), (3, X)],
    "NOT empties one tile": EXTRA[1], "MUST list misses a tile": EXTRA[2], "MUST count == 0": [(0, M), (5, S)], "MUST and SHOULD": [(4, M), (4, S)],
    "MUST and NOT": [(5, M), (5, X)], "SHOULD and NOT": [(5, S), (5, X)], "docId >= n_docs": [(6, S)], "single positive": [(6, M)],
    "single positive + NOT": EXTRA[4], "NOT alone": [(5, X), (6, X)],
}


def directed_inputs(n_segs):
    """boolean_shapes.directed_family's segments under ROLE_MIXES -> (segments, queries, idfs, weights, seg_order): with three
    segments the refs of a query interleave the segments, the call lists them as 2, 0, 1, and in segment 1 list 5 stands in for
    the empty list 0 as the MUST ref of the `count == 0` queries, so that the group dies in the other two segments alone"""
    lists = facet_shapes.small_lists()
    segments = [(N_DOCS, (5 + (np.arange(N_DOCS) * (1 + 2 * s)) % 41).astype(np.uint32), lists) for s in range(n_segs)]
    queries = []
    for q in ROLE_MIXES:
        refs = []
        for li, role in q:
            for s in range(n_segs):
                refs.append((s, 5 if (s == 1 and li == 0 and role == M and len(q) > 1) else li, role))
        queries.append(refs)
    idf, w = boolean_shapes.small_weights(len(lists))
    return segments, queries, [idf] * n_segs, [w] * n_segs, ([2, 0, 1] if n_segs == 3 else None)


def mixed_inputs():
    """facet_shapes' three segments of 300, 77 and 1000 documents with a role per ref: MUST, SHOULD and NOT by turns"""
    segments, queries = boolean_shapes.multi_family()
    mixed = [[(s, li, (M, S, X, S)[(qi + i) % 4]) for i, (s, li) in enumerate(q)] for qi, q in enumerate(queries)]
    return (segments, mixed) + boolean_shapes.multi_weights(segments) + ([2, 0, 1],)


def keys_for(segments, pattern):
    return [sorted_shapes.keys_of(pattern, int(s[0]), seed=5 + i) for i, s in enumerate(segments)]


def tables_for(segments, kind, n_buckets, tile=SMALL_TILE):
    """a bucket table per segment, shifted by the segment's number so that equal docIds of two segments differ in bucket"""
    return [((facet_shapes.table_of(kind, int(s[0]), n_buckets, tile).astype(np.int64) + 3 * i) % n_buckets).astype(np.uint16) for i, s in enumerate(segments)]


class Sets:
    """a boolean_shapes.Family with a key table per segment; the restatement's whole answer is computed once and kept"""

    def __init__(self, fam, keys):
        self.fam, self.keys = fam, keys
        self.handles = [fam.segs.segs[s] for s in fam.order]
        self.key_tables, self._rows, self._counts = None, {}, {}
        fam.ref(1)
        self.everything = fam.cache["all"]                      # boolean_ref.boolean_all: per query (score, segment, doc)

    def set_keys(self, keys):
        self.drop_keys()
        self.keys, self._rows = keys, {}

    def drop_keys(self):
        for h in self.key_tables or []:
            assert nsbind.dockeys_release(self.fam.segs.ctx, h) == 0
        self.key_tables = None

    def key_handles(self):
        if self.key_tables is None:
            self.key_tables = []
            for s in self.fam.order:
                rc, h = nsbind.dockeys_upload(self.fam.segs.ctx, self.keys[s])
                assert rc == 0, self.fam.segs.err()
                self.key_tables.append(h)
        return self.key_tables

    def rows(self, ascending):
        if ascending not in self._rows:
            self._rows[ascending] = boolean_sets_ref.rows(self.everything, self.keys, ascending, self.fam.order)
        return self._rows[ascending]

    def roles_arg(self, roles):
        return self.fam.roles if isinstance(roles, str) else roles

    def count(self, tables, n_buckets, roles="own"):
        fam = self.fam
        handles = []
        try:
            for s in fam.order:
                rc, h = nsbind.facet_upload(fam.segs.ctx, tables[s], n_buckets)
                assert rc == 0, fam.segs.err()
                handles.append(h)
            return nsbind.facet_count_boolean(fam.segs.ctx, fam.qd, fam.refs, self.roles_arg(roles), fam.order, self.handles, handles, n_buckets)[:3]
        finally:
            for h in handles:
                assert nsbind.facet_release(fam.segs.ctx, h) == 0

    def check_counts(self, label, kind, n_buckets):
        fam = self.fam
        tables = tables_for(fam.segments, kind, n_buckets)
        if (kind, n_buckets) not in self._counts:
            self._counts[(kind, n_buckets)] = boolean_sets_ref.counts(fam.segments, fam.queries, tables, n_buckets, fam.order)
        want = self._counts[(kind, n_buckets)]
        rc, counts, found = self.count(tables, n_buckets)
        what = (label, kind, "B", n_buckets)
        assert rc == 0, what + (fam.segs.err(),)
        np.testing.assert_array_equal(counts.astype(np.int64), want, err_msg=str(what))
        np.testing.assert_array_equal(found.astype(np.int64), [len(r) for r in self.everything], err_msg=str(what + ("found",)))

    def release(self):
        if self.fam.segs.ctx:
            self.drop_keys()
        self.fam.release()


class Dated:
    """a Sets under one direction and its full order: what after_shapes.walk and after_shapes.check_call drive"""

    def __init__(self, sets, flags, roles="own"):
        self.sets, self.fam, self.flags, self.roles = sets, sets.fam, flags, roles
        self.rows = sets.rows(bool(flags & ASC))

    def raw(self, k, cursors):
        fam = self.fam
        return nsbind.search_sorted_boolean_raw(fam.segs.ctx, fam.qd, fam.refs, self.sets.roles_arg(self.roles), k, self.flags,
                                                None if cursors is None else nsbind.cursors(cursors), fam.order, self.sets.handles, self.sets.key_handles())

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


def undated_last(rows):
    for r in rows:
        ks = [x[4] for x in r]
        first0 = ks.index(0) if 0 in ks else len(ks)
        assert all(kk == 0 for kk in ks[first0:]), ks


def directed_sets(n_segs, pattern="pool5"):
    segments, queries, idfs, weights, order = directed_inputs(n_segs)
    return Sets(boolean_shapes.Family(segments, queries, idfs, weights, seg_order=order), keys_for(segments, pattern))


def run_directed(n_segs, tile_expected=None):
    """every role mix at B = 1, 50, 1024 and K = 1 .. 100 in both directions, without and with skip tables; then the key
    patterns that are all ties and half undated; then roles == NULL against the all-SHOULD restatement"""
    tile = nsbind.facet_tile_docs()
    if tile_expected is not None:
        assert tile == tile_expected, (tile, tile_expected)
    sets = directed_sets(n_segs)
    fam = sets.fam
    try:
        assert sorted({int(c) // n_segs for c in fam.qd["term_count"]}) == [0, 1, 2, 3, 4, 8, 70]
        for with_skips in (False, True):
            if with_skips:
                for s in range(n_segs):
                    assert facet_shapes.build_skips(fam.segs, s) == 4
            for B in BUCKETS:
                for kind in ("modulo", "tile"):
                    sets.check_counts(("directed", n_segs, "skips", with_skips), kind, B)
            for flags in (0, ASC):
                side = Dated(sets, flags)
                undated_last(side.rows)
                for k in KS:
                    side.check(("directed", n_segs, "skips", with_skips), k)
        for pattern in ("same", "half_undated"):                  # ties across every tile edge and across the segments; key 0 last
            sets.set_keys(keys_for(fam.segments, pattern))
            for flags in (0, ASC):
                side = Dated(sets, flags)
                undated_last(side.rows)
                for k in (10, 65):
                    side.check(("pattern", pattern, n_segs), k)
        founds = [len(r) for r in sets.everything]
        assert 0 in founds and max(founds) > 100 and len(set(founds)) > 10
        # roles == NULL: every ref SHOULD
        segments, queries, idfs, weights, order = directed_inputs(n_segs)
        plain = Sets(boolean_shapes.Family(segments, [[(s, li, S) for s, li, _ in q] for q in queries], idfs, weights, seg_order=order), keys_for(segments, "pool5"))
        try:
            tables = tables_for(segments, "modulo", 50)
            rc, counts, found = plain.count(tables, 50, roles=None)
            assert rc == 0, plain.fam.segs.err()
            np.testing.assert_array_equal(counts.astype(np.int64), boolean_sets_ref.counts(segments, plain.fam.queries, tables, 50, plain.fam.order))
            np.testing.assert_array_equal(found.astype(np.int64), [len(r) for r in plain.everything])
            for flags in (0, ASC):
                Dated(plain, flags, roles=None).check(("roles NULL", n_segs), 100)
        finally:
            plain.release()
    finally:
        sets.release()
    return tile


def run_counts():
    """found == K - 1, K, K + 1 and 0 around K = 64, 65 and 100 through every role (boolean_shapes.counts_family)"""
    fam, sizes = boolean_shapes.counts_family()
    sets = Sets(fam, keys_for(fam.segments, "pool5"))
    try:
        founds = [len(r) for r in sets.everything]
        for i, m in enumerate(sizes):
            assert founds[4 * i:4 * i + 4] == [m] * 4
        for k in (64, 65, 100):
            assert {-1, 0, 1} <= {f - k for f in founds} and 0 in founds, (k, founds)
            for flags in (0, ASC):
                hits, keys, nhits, found, rest = Dated(sets, flags).check("counts", k)
                assert [int(n) for n in nhits] == [min(k, f) for f in founds]
        sets.check_counts("counts", "modulo", 50)
    finally:
        sets.release()


def run_walks(ks=WALK_KS):
    """date order paged to exhaustion: per query the pages concatenated are the full order with the scores of the unpaged call,
    no document twice, rest counting down to 0 (after_shapes.walk asserts each).  K = 1 on one segment whose keys are all
    equal (every page is decided by the docId alone), K = 10 and 64 on three segments in both directions."""
    pages = {}
    for k in ks:
        sets = directed_sets(1, "same") if k == 1 else directed_sets(3, "pool5")
        try:
            for flags in ((0,) if k == 1 else (0, ASC)):
                side = Dated(sets, flags)
                assert max(len(r) for r in side.rows) > 100 and min(len(r) for r in side.rows) == 0
                pages[(k, flags)] = after_shapes.walk(("boolean sets walk", hex(flags)), side, k)
        finally:
            sets.release()
    return pages


def run_cursors():
    """cursors that are no document of the matched set, or no document at all, on the mixed-role family over three segments
    (fifty even key values, some documents undated): after_shapes' cursor rounds against the restatement"""
    segments, queries, idfs, weights, order = mixed_inputs()
    keys = [np.where(np.arange(s[0]) % 9 == 4, 0, 20200101 + 2 * (np.arange(s[0]) % 50)).astype(np.uint32) for s in segments]
    sets = Sets(boolean_shapes.Family(segments, queries, idfs, weights, seg_order=order), keys)
    try:
        for flags in (0, ASC):
            side = Dated(sets, flags)
            assert max(len(r) for r in side.rows) > 100
            per_query = after_shapes.arbitrary_cursors(side, lambda r: r[4], lambda rows: sorted({r[4] + 1 for r in rows if r[4]})[:4])
            specials = [("undated", (0, order[1], 128)), ("key 1", (1, order[1], 128)), ("largest key", (0xFFFFFFFE, order[0], 0)),
                        ("below everything", (0, order[-1], 0xFFFFFFFF))]
            for k in (10, 100):
                after_shapes.run_cursor_rounds(("boolean sets cursors", hex(flags)), side, per_query, specials, k)
            above = (1 if flags & ASC else 0xFFFFFFFE, order[0], 0)
            plain = side.call(100, None)
            for a, b in zip(plain, side.call(100, [above] * len(side.rows))):
                assert a.tobytes() == b.tobytes(), "a cursor above everything"
            for a, b in zip(plain, side.call(100, [None] * len(side.rows))):
                assert a.tobytes() == b.tobytes(), "every cursor unset"
            assert plain[4].tobytes() == plain[3].tobytes()                       # no cursor: rest = found
            _, _, nhits, found, rest = side.call(100, [(0, order[-1], 0xFFFFFFFF)] * len(side.rows))
            assert not np.any(nhits) and not np.any(rest) and list(found) == [len(r) for r in side.rows]
    finally:
        sets.release()


def product_inputs(tile):
    """boolean_shapes.run_product_tile's family: n_docs = two tiles + 5, lists whose documents straddle both tile edges and the end"""
    n = 2 * tile + 5
    win = min(1 << 13, tile)
    rng = np.random.default_rng(31)
    edges = np.array([0, win - 1, win, tile - 1, tile, tile + win - 1, tile + win, 2 * tile - 1, 2 * tile, n - 1])
    docs = [np.concatenate([np.arange(win - 40, win + 40), np.arange(tile - 100, tile + 100), np.arange(2 * tile - 50, n)]),
            np.union1d(rng.choice(n, 300, replace=False), edges),
            np.arange(0, n, 997),
            np.concatenate([np.arange(win - 3, win + 3), np.arange(tile - 3, tile + 3)]),
            np.arange(tile - 60, tile + 20)]
    lists = [(x.astype(np.uint32), np.full(len(x), 3, np.uint32)) for x in docs]
    segments = [(n, np.full(n, 11, np.uint32), lists)]
    one = [[(0, S)], [(1, S)], [(0, S), (1, S)], [(0, M), (1, S)], [(0, M), (4, X)], [(0, M), (4, M)], [(1, M), (2, M)], [(0, S), (1, S), (2, S), (3, X)],
           [(3, M), (0, M), (1, S)], [(2, S), (2, S)], [(3, X)], [(4, S), (0, X)], [(1, M), (1, X)], [(0, M), (0, S), (4, S), (3, X)], [(4, M), (0, M), (2, X)]]
    queries = [[(0, li, r) for li, r in q] for q in one]
    idf, w = boolean_shapes.small_weights(len(lists))
    return segments, queries, [idf], [w], docs


def run_product_tile():
    """the product build's tile: the order decided by the docId across both tile edges (all keys equal), by five key values, and a
    cursor at each edge"""
    tile = nsbind.facet_tile_docs()
    segments, queries, idfs, weights, docs = product_inputs(tile)
    n = int(segments[0][0])
    sets = Sets(boolean_shapes.Family(segments, queries, idfs, weights), keys_for(segments, "same"))
    try:
        founds = [len(r) for r in sets.everything]
        assert founds[0] == len(docs[0]) and founds[10] == 0 and founds[12] == 0 and founds[4] == len(docs[0]) - 80
        d = np.arange(n, dtype=np.int64)
        for with_skips in (False, True):
            if with_skips:
                assert facet_shapes.build_skips(sets.fam.segs, 0) == 4
            for B, table in ((50, ((d * 7919) % 50).astype(np.uint16)), (1024, (d // tile).astype(np.uint16))):
                rc, counts, found = sets.count([table], B)
                assert rc == 0, sets.fam.segs.err()
                np.testing.assert_array_equal(counts.astype(np.int64), boolean_sets_ref.counts(segments, queries, [table], B))
                np.testing.assert_array_equal(found.astype(np.int64), founds)
            for k in (1, 64, 65, 100):
                Dated(sets, 0).check(("product tile", tile, with_skips), k)
        side = Dated(sets, ASC)
        for at in (tile - 1, tile, 2 * tile - 1, 2 * tile, n - 1):
            side.check(("product edges", at), 100, [(20200101, 0, at)] * len(queries))
        sets.set_keys(keys_for(segments, "pool5"))
        for flags in (0, ASC):
            Dated(sets, flags).check(("product tile", "pool5"), 100)
    finally:
        sets.release()
    return tile, n


# ---- equivalences on the same raw inputs --------------------------------------------------------------------------------
FLOOR_SAME_ROLE = boolean_shapes.FLOOR_SAME_ROLE      # queries with found >= 2 under one role for every ref
FLOOR_SMALL_SETS = 12                                  # queries with 2 <= found <= 100 that the set comparison must cover


def run_same_role_equals_the_unroled_calls():
    """roles == NULL (and all SHOULD) == ns_facet_count / ns_search_sorted under NS_FLAG_OR, all MUST == under NS_FLAG_AND: the
    same arrays, byte for byte"""
    covered = {}
    for role, mode in ((S, 0), (M, AND)):
        segments, queries, idfs, weights = boolean_shapes.same_role_inputs(role)
        sets = Sets(boolean_shapes.Family(segments, queries, idfs, weights, seg_order=[2, 0, 1]), keys_for(segments, "pool5"))
        fam = sets.fam
        try:
            ctx = fam.segs.ctx
            covered[role] = sum(len(r) >= 2 for r in sets.everything)
            assert covered[role] >= FLOOR_SAME_ROLE[role], covered
            for with_skips in (False, True):
                if with_skips:
                    for s in range(3):
                        facet_shapes.build_skips(fam.segs, s)
                for roles in ((None, "own") if role == S else ("own",)):
                    for B in (50, 1024):
                        tables = tables_for(segments, "modulo", B)
                        handles = [nsbind.facet_upload(ctx, tables[s], B)[1] for s in fam.order]
                        try:
                            rc, want, want_found, _ = nsbind.facet_count(ctx, fam.qd, fam.refs, mode, fam.order, sets.handles, handles, B)
                            assert rc == 0, fam.segs.err()
                            rc, got, found, _ = nsbind.facet_count_boolean(ctx, fam.qd, fam.refs, sets.roles_arg(roles), fam.order, sets.handles, handles, B)
                            assert rc == 0, fam.segs.err()
                            assert got.tobytes() == want.tobytes() and found.tobytes() == want_found.tobytes(), (role, roles, B)
                            assert [int(f) for f in found] == [len(r) for r in sets.everything]
                        finally:
                            for h in handles:
                                nsbind.facet_release(ctx, h)
                    for k in (7, 64, 100):
                        for direction in (0, ASC):
                            rc, *want = nsbind.search_sorted_raw(ctx, fam.qd, fam.refs, k, mode | direction, fam.order, sets.handles, sets.key_handles())
                            assert rc == 0, fam.segs.err()
                            rc, hits, keys, nhits, found, rest, _ = Dated(sets, direction, roles).raw(k, None)
                            assert rc == 0, fam.segs.err()
                            for a, b in zip((hits, keys, nhits, found), want):
                                assert a.tobytes() == b.tobytes(), (role, roles, k, direction)
                            assert rest.tobytes() == found.tobytes()
        finally:
            sets.release()
    return covered


def small_sets(everything):
    return [q for q, rows in enumerate(everything) if 2 <= len(rows) <= 100]


def run_equals_the_boolean_search():
    """found == ns_search_boolean's; where found <= 100, the K = 100 answer holds the same (segment, doc, score bits) triples"""
    covered = 0
    for make in (lambda: directed_sets(1), lambda: directed_sets(3), lambda: Sets(boolean_shapes.Family(*mixed_inputs()[:4], seg_order=[2, 0, 1]), keys_for(mixed_inputs()[0], "pool5"))):
        sets = make()
        fam = sets.fam
        try:
            rc, b_hits, b_nhits, b_found = fam.call(100)
            assert rc == 0, fam.segs.err()
            for flags in (0, ASC):
                hits, keys, nhits, found, rest = Dated(sets, flags).call(100, None)
                np.testing.assert_array_equal(found, b_found)
                np.testing.assert_array_equal(nhits, b_nhits)
                for q in small_sets(sets.everything):
                    n = int(nhits[q])
                    triples = lambda h: sorted((int(x["seg"]), int(x["doc"]), int(x["score"].view(np.uint32))) for x in h[q, :n])  # noqa: E731
                    assert n == int(found[q]) and triples(hits) == triples(b_hits), (q, flags)
            covered += len(small_sets(sets.everything))
            rc, counts, c_found = sets.count(tables_for(fam.segments, "modulo", 50), 50)
            assert rc == 0
            np.testing.assert_array_equal(c_found, b_found)
        finally:
            sets.release()
    assert covered >= FLOOR_SMALL_SETS, covered
    return covered


# ---- refusals -----------------------------------------------------------------------------------------------------------
def run_refusals():
    """each NS_E_INVAL with its message, nothing launched: the output arrays keep their fill"""
    import ctypes as C

    from rawseg import RawSegments

    L = nsbind.hip_lib()
    segments, queries, idfs, weights, order = mixed_inputs()
    sets = Sets(boolean_shapes.Family(segments, queries, idfs, weights, seg_order=order), keys_for(segments, "pool5"))
    other = RawSegments(segments[:1])
    o_tab = o_keys = None
    fam = sets.fam
    ctx, Q = fam.segs.ctx, len(fam.qd)
    B = 50
    tabs = [nsbind.facet_upload(ctx, t, B)[1] for t in [tables_for(segments, "modulo", B)[s] for s in order]]
    try:
        rc, o_tab = nsbind.facet_upload(other.ctx, tables_for(segments, "modulo", B)[0], B)
        assert rc == 0
        rc, o_keys = nsbind.dockeys_upload(other.ctx, sets.keys[0])
        assert rc == 0

        def message(match):
            msg = L.ns_last_error(ctx).decode()
            assert match in msg, msg

        def count(match, qd=fam.qd, refs=fam.refs, roles=fam.roles, hs=None, ts=None):
            rc, counts, found, _ = nsbind.facet_count_boolean(ctx, qd, refs, roles, order, sets.handles if hs is None else hs, tabs if ts is None else ts, B)
            if match is None:
                assert rc == 0, L.ns_last_error(ctx).decode()
                return
            assert rc == NS_E_INVAL, rc
            message("ns_facet_count_boolean: ")
            message(match)
            assert np.all(counts == 0xABABABAB) and np.all(found == 0xABABABAB), "a refused call writes nothing"

        def dated(match, qd=fam.qd, refs=fam.refs, roles=fam.roles, flags=0, after=None, hs=None, ks=None):
            rc, hits, keys, nhits, found, rest, _ = nsbind.search_sorted_boolean_raw(ctx, qd, refs, roles, 10, flags, after, order,
                                                                                    sets.handles if hs is None else hs, sets.key_handles() if ks is None else ks)
            if match is None:
                assert rc == 0, L.ns_last_error(ctx).decode()
                return
            assert rc == NS_E_INVAL, rc
            message("ns_search_sorted_boolean: ")
            message(match)
            assert np.all(hits.view(np.uint8) == 0xAB) and np.all(keys == 0xABABABAB) and np.all(nhits == 0xABABABAB) and np.all(found == 0xABABABAB)
            assert np.all(rest == 0xABABABAB), "a refused call writes nothing"

        for call in (count, dated):
            call(None)
            bad = fam.roles.copy()
            bad[3] = 3
            call("ref 3: role 3 is none of NS_ROLE_SHOULD, NS_ROLE_MUST, NS_ROLE_NOT", roles=bad)
            past = fam.refs.copy()
            past["byte_off"][0] = 8 * 10 ** 6
            call("runs past the postings", refs=past)
            scoring = int(np.flatnonzero(fam.roles != X)[0])
            nan = fam.refs.copy()
            nan["idf"][scoring] = np.nan
            call("ref %d: idf or qweight is not finite" % scoring, refs=nan)
            inf = fam.refs.copy()
            inf["qweight"][scoring] = -np.inf
            call("ref %d: idf or qweight is not finite" % scoring, refs=inf)
            excluded = int(np.flatnonzero(fam.roles == X)[0])
            nan = fam.refs.copy()
            nan["idf"][excluded] = np.nan
            call(None, refs=nan)                                                   # under NOT the numbers are never read
            call("segment 0 is not a published segment of this ctx", hs=[other.segs[0]] + sets.handles[1:])
        count("table 1 does not belong to this ctx", ts=[tabs[0], o_tab, tabs[2]])
        dated("key table 2 does not belong to this ctx", ks=sets.key_handles()[:2] + [o_keys])
        for flags in (AND, AND | ASC, 0x2000, 1 << 31):
            dated("flags 0x%x: only NS_SORT_ASC is known" % flags, flags=flags)
        dated(None, flags=ASC)
        ok = nsbind.cursors([(20200101, 2, 5)] * Q)
        dated(None, after=ok)
        alien = ok.copy()
        alien["seg"][1] = 7
        dated("query 1: cursor names segment 7, which the call does not list", after=alien)
        alien["set"][1] = 0                                                        # an unset cursor's fields are ignored
        dated(None, after=alien)
        two = ok.copy()
        two["set"][3] = 2
        dated("query 3: cursor with set = 2 (0 or 1)", after=two)
        reserved = ok.copy()
        reserved["rank"][2] = 0xFFFFFFFF
        dated("query 2: cursor with the reserved key 0xFFFFFFFF", after=reserved)
        # no queries: NS_OK, nothing touched, whatever else is passed
        assert L.ns_facet_count_boolean(ctx, None, 0, None, None, 0, None, None, None, 0, None, None, None) == 0
        assert L.ns_search_sorted_boolean(ctx, None, 0, None, None, 0, 10, 0, None, None, None, None, 0, None, None, None, None, None, None) == 0
        assert L.ns_facet_count_boolean(None, None, 0, None, None, 0, None, None, None, 0, None, None, None) == NS_E_INVAL
        # the kernel times of both calls
        out4 = (C.c_float * 4)()
        assert L.ns_boolean_sets_kernel_ms(out4, 1) == 0 and all(v > 0.0 for v in out4), list(out4)
        assert L.ns_boolean_sets_kernel_ms(out4, 0) == 0 and all(v == 0.0 for v in out4)
        assert L.ns_boolean_sets_kernel_ms(None, 0) == NS_E_INVAL
    finally:
        for h in tabs:
            nsbind.facet_release(ctx, h)
        if o_tab:
            nsbind.facet_release(other.ctx, o_tab)
        if o_keys:
            nsbind.dockeys_release(other.ctx, o_keys)
        other.release()
        sets.release()


def run_refused_between_two_runs():
    """The five calls that share one call scaffold, each once; then calls that each of them refuses after it has
    bound its segments (the planner's refusal for the counts, a cursor that names an unlisted segment for the ranked calls,
    and an unknown flag for the dated ones); then the five again: every output byte is the first run's, and ns_last_error
    names the refused call.  The refusals are host-side: nothing is launched, and the blocks of the first runs are in the pool."""
    L = nsbind.hip_lib()
    segments, queries, idfs, weights, order = mixed_inputs()
    sets = Sets(boolean_shapes.Family(segments, queries, idfs, weights, seg_order=order), keys_for(segments, "pool5"))
    fam = sets.fam
    ctx, Q, B, K = fam.segs.ctx, len(fam.qd), 50, 10
    tabs = [nsbind.facet_upload(ctx, t, B)[1] for t in [tables_for(segments, "modulo", B)[s] for s in order]]
    try:
        hs, ks = sets.handles, sets.key_handles()
        alien = nsbind.cursors([(20200101, 7, 5)] * Q)                            # the call lists segments 2, 0, 1
        past = fam.refs.copy()
        past["byte_off"][0] = 8 * 10 ** 6
        calls = {
            "ns_facet_count": lambda refs=fam.refs: nsbind.facet_count(ctx, fam.qd, refs, 0, order, hs, tabs, B),
            "ns_search_sorted_after": lambda after=None, flags=ASC: nsbind.search_sorted_after_raw(ctx, fam.qd, fam.refs, K, flags, after, order, hs, ks),
            "ns_search_boolean_after": lambda after=None: nsbind.search_boolean_after_raw(ctx, fam.qd, fam.refs, fam.roles, K, after, order, hs),
            "ns_facet_count_boolean": lambda refs=fam.refs: nsbind.facet_count_boolean(ctx, fam.qd, refs, fam.roles, order, hs, tabs, B),
            "ns_search_sorted_boolean": lambda after=None, flags=ASC: nsbind.search_sorted_boolean_raw(ctx, fam.qd, fam.refs, fam.roles, K, flags, after, order, hs, ks),
        }
        unlisted = "query 0: cursor names segment 7, which the call does not list"
        refusals = [("ns_facet_count", dict(refs=past), "runs past the postings"), ("ns_facet_count_boolean", dict(refs=past), "runs past the postings"),
                    ("ns_search_sorted_after", dict(after=alien), unlisted), ("ns_search_boolean_after", dict(after=alien), unlisted),
                    ("ns_search_sorted_boolean", dict(after=alien), unlisted),
                    ("ns_search_sorted_after", dict(flags=0x2000), "flags 0x2000: only NS_FLAG_AND and NS_SORT_ASC are known"),
                    ("ns_search_sorted_boolean", dict(flags=AND), "flags 0x1: only NS_SORT_ASC is known")]

        def run_all():
            out = {}
            for name, call in calls.items():
                res = call()
                assert res[0] == 0, (name, L.ns_last_error(ctx).decode())
                out[name] = [a.tobytes() for a in res[1:-1]]                      # every output array; the last member is the time
                assert len(out[name]) >= 2 and all(out[name])
            return out

        first = run_all()
        assert int(np.frombuffer(first["ns_facet_count"][1], dtype=np.uint64).sum()) > 0      # found: the runs are about something
        for name, change, match in refusals:
            res = calls[name](**change)
            assert res[0] == NS_E_INVAL, (name, res[0])
            msg = L.ns_last_error(ctx).decode()
            assert msg.startswith(name + ": ") and match in msg, msg
            # (the binding fills hits with 0xAB bytes and the integer arrays with the value 0xABABABAB)
            assert all(np.all(a.view(np.uint8) == 0xAB if a.dtype.names else a == 0xABABABAB) for a in res[1:-1]), "a refused call writes nothing"
        assert run_all() == first
        for name, change, _ in refusals:                                           # and a refusal directly before its own call's rerun
            assert calls[name](**change)[0] == NS_E_INVAL
            assert [a.tobytes() for a in calls[name]()[1:-1]] == first[name], name
    finally:
        for h in tabs:
            nsbind.facet_release(ctx, h)
        sets.release()


def run_one_query_past_the_candidate_buffer():
    """a single query whose work items x K x 8 B exceed the 64 MiB of candidate rows is refused; with one item fewer it runs.
    Only a small tile makes that many items affordable: a segment of (rows + 1) x tile documents and one list of three postings."""
    tile = nsbind.facet_tile_docs()
    assert tile <= SMALL_TILE, tile
    K = 100
    rows = CAND_BYTES // (8 * K)
    n = (rows + 1) * tile
    d = np.array([0, tile * rows - 1, n - 1], np.uint32)
    lists = [(d, np.ones(3, np.uint32))]
    segments = [(n, np.full(n, 7, np.uint32), lists), (rows * tile, np.full(rows * tile, 7, np.uint32), [(d[:2], np.ones(2, np.uint32))])]
    queries = [[(1, 0, M)], [(0, 0, M)]]
    sets = Sets(boolean_shapes.Family(segments, queries, [[1.0]] * 2, [[1.0]] * 2), [np.full(int(s[0]), 20200101, np.uint32) for s in segments])
    try:
        fam = sets.fam
        side = Dated(sets, 0)
        rc, hits, keys, nhits, found, rest, _ = side.raw(K, None)
        assert rc == NS_E_INVAL
        msg = fam.segs.err().decode()
        assert "ns_search_sorted_boolean: query 1 alone has %d work items" % (rows + 1) in msg and "holds %d rows at K = 100" % rows in msg, msg
        assert np.all(hits.view(np.uint8) == 0xAB) and np.all(nhits == 0xABABABAB) and np.all(found == 0xABABABAB)
        qd = fam.qd[:1].copy()
        rc, hits, keys, nhits, found, rest, _ = nsbind.search_sorted_boolean_raw(fam.segs.ctx, qd, fam.refs[:1], fam.roles[:1], K, 0, None, fam.order, sets.handles,
                                                                                sets.key_handles())
        assert rc == 0 and int(found[0]) == 2 and [int(x) for x in hits[0, :2]["doc"]] == [0, tile * rows - 1], (rc, found)
        return rows + 1
    finally:
        sets.release()


def main(out_path):
    """child process at NS_FACET_TILE_DOCS = 128.  Both builds run the directed families; the counting build reports the
    counters of those and of one walk; the variants build runs the walks, the cursor rounds, the equivalences and the query
    past the candidate buffer."""
    counting = "ns_debug_boolean_sets_counters" in nsbind.debug_counters(reset=True)
    rep = {"tile": run_directed(1, tile_expected=SMALL_TILE), "counting": counting}
    run_directed(3)
    run_counts()
    if counting:
        run_walks(ks=[64])
        c = nsbind.debug_counters(reset=True)["ns_debug_boolean_sets_counters"]
        rep["events"] = {e: c[i] for e, i in EVENTS.items()}
        rep["missed"] = [e for e in EVENTS if rep["events"][e] == 0]
        print("boolean sets", rep["events"], flush=True)
    else:
        run_walks()
        run_cursors()
        run_same_role_equals_the_unroled_calls()
        run_equals_the_boolean_search()
        rep["past_the_buffer"] = run_one_query_past_the_candidate_buffer()
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print("boolean sets shapes OK")


if __name__ == "__main__":
    main(sys.argv[1])
