"""Directed inputs of ns_search_quorum_after, ns_facet_count_quorum and ns_search_sorted_quorum (the QUORUM instantiations in
csrc/ns_boolean.hip and csrc/ns_boolean_sets.hip) and the code that runs them through the raw C-ABI against the
restatement (tests/quorum_ref.py).  300 documents per segment, one segment and three listed as 2, 0, 1, lists of a few postings
built for the property each case is named after (tests/test_quorum_cpu.py asserts the properties through the restatement).  All
comparisons are exact, score bits included.

Imported by tests/test_quorum_gpu.py for the product library (one tile and one window hold a segment), and run as a program in a
child process that loaded the variants or the counting build with NS_FACET_TILE_DOCS=128 NS_BOOL_WIN_DOCS=32: there 300 documents
are two whole tiles and a part, four windows each, a counted clause ends one window and holds in the next, members straddle tile
edges, and the counting build reports which paths of the quorum required stage the inputs reached."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "nextsearch-api_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import after_shapes  # noqa: E402
import boolean_sets_shapes as bss  # noqa: E402
import boolean_shapes  # noqa: E402
import facet_shapes  # noqa: E402
import grouped_shapes  # noqa: E402
import nsbind  # noqa: E402
import quorum_ref  # noqa: E402
from boolean_ref import MUST, NOT, SHOULD  # noqa: E402

ASC = nsbind.NS_SORT_ASC
NS_E_INVAL = -1
SMALL_TILE, SMALL_WIN, N_DOCS = boolean_shapes.SMALL_TILE, boolean_shapes.SMALL_WIN, boolean_shapes.N_DOCS
KS = [1, 3, 64, 65, 100]                      # 64 / 65: the boundary between the kept set's two registers
BUCKETS = [1, 50]
S, M, X = SHOULD, MUST, NOT
EVENTS = nsbind.QUORUM_EVENTS                 # ns_debug_boolean_quorum_counters, in order (counting build)

# list numbers
EMPTY, A, B, C = 0, 1, 2, 3
SAT = list(range(4, 14))                      # ten lists that all hold document 77
W1, W2 = 14, 15
T1, T2, T3 = 16, 17, 18
E1, E2 = 19, 20
NOTL = 21
P1, P2, P3 = 22, 23, 24
R1, R2, R3 = 25, 26, 27


def lists():
    """A, B, C: documents in exactly 0, 1, 2 and 3 of them.  SAT[i]: document 77 in all ten, 150 + i in SAT[i] alone, 211 in two,
    212 in three, 214 and 10 in six, 213 and 200 in seven.  W1, W2: window [32, 64) holds a posting of W1 alone, window [64, 96)
    one of each and document 70 of both.  T1, T2, T3: document 299, the last bit of the partial last bitmap word; postings 305 and
    400 >= n_docs in T2, 305 in T3.  E1, E2: postings on both sides of the tile edges 128 and 256.  NOTL: an exclusion.  P1, P2,
    P3: a second counted clause in which documents 40, 41, 42 reach 1 where A, B, C gave them 2.  R1, R2, R3: 150 random documents
    each, more than 100 of them in two."""
    rng = np.random.default_rng(23)
    docs = {EMPTY: [], A: [3, 10, 40, 41, 130, 200, 299], B: [10, 41, 42, 131, 200, 260], C: [10, 40, 42, 132, 200, 261],
            W1: [33, 70], W2: [70, 71], T1: [6, 299], T2: [7, 299, 305, 400], T3: [8, 298, 305], E1: [126, 127, 128, 129, 255, 256],
            E2: [127, 128, 255, 256, 257], NOTL: [10, 41, 150], P1: [10, 40, 200], P2: [10, 41, 201], P3: [42, 200, 202]}
    for i, li in enumerate(SAT):
        docs[li] = sorted([77, 150 + i] + ([211] if i < 2 else []) + ([212] if i < 3 else []) + ([10, 214] if i < 6 else []) + ([200, 213] if i < 7 else []))
    for li in (R1, R2, R3):
        docs[li] = np.sort(rng.choice(N_DOCS, 150, replace=False)).tolist()
    out = []
    for li in range(len(docs)):
        d = np.array(docs[li], dtype=np.uint32)
        assert np.all(d[1:] > d[:-1])
        out.append((d, (1 + d % 3).astype(np.uint32)))
    return out


# (list, role, clause, need) per ref
CASES = {
    "two of three": [(A, M, 0, 2), (B, M, 0, 2), (C, M, 0, 2)],
    "three of three": [(A, M, 0, 3), (B, M, 0, 3), (C, M, 0, 3)],
    "saturation: two of nine": [(li, M, 0, 2) for li in SAT[:9]],
    "saturation: three of nine": [(li, M, 0, 3) for li in SAT[:9]],
    "saturation: seven of ten": [(li, M, 0, 7) for li in SAT],
    "six of ten": [(li, M, 0, 6) for li in SAT],
    "per-window exit": [(W1, M, 0, 2), (W2, M, 0, 2)],
    "duplicate member": [(A, M, 0, 2), (A, M, 0, 2), (B, M, 0, 2)],
    "a duplicate alone cannot make two": [(A, M, 0, 2), (A, M, 0, 2)],
    "planes cleared": [(A, M, 0, 2), (B, M, 0, 2), (C, M, 0, 2), (P1, M, 1, 2), (P2, M, 1, 2), (P3, M, 1, 2)],
    "a counted clause before an any-of clause": [(A, M, 0, 2), (B, M, 0, 2), (C, M, 0, 2), (P1, M, 1, 1), (P2, M, 1, 1)],
    "an any-of clause before a counted clause": [(P1, M, 5, 0), (P2, M, 5, 0), (A, M, 2, 2), (B, M, 2, 2), (C, M, 2, 2)],
    "word tail": [(T1, M, 0, 2), (T2, M, 0, 2)],
    "out-of-range postings": [(T2, M, 0, 2), (T3, M, 0, 2)],
    "out-of-range postings, three members": [(T1, M, 0, 2), (T2, M, 0, 2), (T3, M, 0, 2)],
    "tile edges": [(E1, M, 0, 2), (E2, M, 0, 2)],
    "NOT after count": [(A, M, 0, 2), (B, M, 0, 2), (C, M, 0, 2), (NOTL, X, 0, 0)],
    "a long item: seven of ten, each named six times": [(SAT[i % 10], M, 0, 7) for i in range(60)] + [(A, M, 1, 2), (B, M, 1, 2), (C, M, 1, 2)]
                                                       + [(W1 + i % 2, S, 0, 0) for i in range(7)],
    "a long item: the counted clause behind": [(A, M, 9, 2), (B, M, 9, 2), (C, M, 9, 2)] + [(SAT[i % 10], M, 3, 2) for i in range(62)],
    "too few members": [(A, M, 0, 2), (B, M, 0, 2)],                      # with three segments: B is EMPTY in segment 1
    "an empty member is dropped": [(A, M, 0, 2), (EMPTY, M, 0, 2), (B, M, 0, 2), (C, S, 0, 0)],
    "single ref, need 1": [(A, M, 0, 1)],
    "single ref, need 2": [(A, M, 0, 2)],
    "one survivor, need 1": [(EMPTY, M, 0, 1), (A, M, 0, 1)],
    "more than a hundred": [(R1, M, 0, 2), (R2, M, 0, 2), (R3, M, 0, 2)],
    "more than a hundred, with optional terms": [(R1, M, 7, 2), (A, S, 0, 0), (R2, M, 7, 2), (R3, M, 7, 2), (E1, S, 3, 5), (NOTL, X, 9, 9)],
    "needs on SHOULD and NOT refs are not read": [(R1, S, 1, 200), (R2, X, 1, 9), (R3, S, 2, 8)],
}
DIRECTED = [[]] + list(CASES.values())
NAMES = ["no ref"] + list(CASES)


def small_weights(n_lists):
    idf, w = boolean_shapes.small_weights(9)
    return [idf[i % 9] + 0.01 * i for i in range(n_lists)], [w[i % 9] for i in range(n_lists)]


def directed_inputs(n_segs, cases=None):
    """DIRECTED over one or three segments of 300 documents -> (segments, queries, idfs, weights, seg_order): with three segments
    the refs of a query interleave the segments, the call lists them as 2, 0, 1, and in segment 1 the EMPTY list stands in for B
    in "too few members", which so dies there alone"""
    ls = lists()
    segments = [(N_DOCS, (5 + (np.arange(N_DOCS) * (1 + 2 * s)) % 41).astype(np.uint32), ls) for s in range(n_segs)]
    few = CASES["too few members"]
    queries = []
    for q in (DIRECTED if cases is None else cases):
        refs = []
        for li, role, clause, need in q:
            for s in range(n_segs):
                refs.append((s, EMPTY if (s == 1 and li == B and q is few) else li, role, clause, need))
        queries.append(refs)
    idf, w = small_weights(len(ls))
    return segments, queries, [idf] * n_segs, [w] * n_segs, ([2, 0, 1] if n_segs == 3 else None)


class Family(boolean_shapes.Family):
    """uploaded segments + one call's descriptors, roles, clause values and needs; the restatement's whole answer is computed
    once and kept.  queries: per query [(segment, list, role, clause, need)]"""

    def __init__(self, segments, queries, idfs, weights, seg_order=None, keys=None):
        super().__init__(segments, [[(s, li, r) for s, li, r, _, _ in q] for q in queries], idfs, weights, seg_order)
        self.quorum = queries
        self.clauses = np.array([c for q in queries for _, _, _, c, _ in q], dtype=np.uint16)
        self.needs = np.array([m for q in queries for _, _, _, _, m in q], dtype=np.uint8)
        self.everything = quorum_ref.quorum_all(segments, queries, self.order, idfs, weights)
        self.founds = [len(r) for r in self.everything]
        self.handles = [self.segs.segs[s] for s in self.order]
        self.keys = bss.keys_for(segments, "pool5") if keys is None else keys
        self.key_tables, self._counts = None, {}

    key_handles = grouped_shapes.Family.key_handles
    set_keys = grouped_shapes.Family.set_keys

    def count(self, tables, n_buckets, roles="own", clauses="own", needs="own", call="quorum"):
        """ns_facet_count_quorum (call: "grouped" / "boolean" for the siblings) under freshly uploaded tables -> (rc, counts, found)"""
        ro = self.roles if isinstance(roles, str) else roles
        cl = self.clauses if isinstance(clauses, str) else clauses
        ne = self.needs if isinstance(needs, str) else needs
        handles = []
        try:
            for s in self.order:
                rc, h = nsbind.facet_upload(self.segs.ctx, tables[s], n_buckets)
                assert rc == 0, self.segs.err()
                handles.append(h)
            if call == "boolean":
                return nsbind.facet_count_boolean(self.segs.ctx, self.qd, self.refs, ro, self.order, self.handles, handles, n_buckets)[:3]
            if call == "grouped":
                return nsbind.facet_count_grouped(self.segs.ctx, self.qd, self.refs, ro, cl, self.order, self.handles, handles, n_buckets)[:3]
            return nsbind.facet_count_quorum(self.segs.ctx, self.qd, self.refs, ro, cl, ne, self.order, self.handles, handles, n_buckets)[:3]
        finally:
            for h in handles:
                assert nsbind.facet_release(self.segs.ctx, h) == 0

    def check_counts(self, label, kind, n_buckets):
        """the counts equal the restatement's, and they sum to found"""
        tables = bss.tables_for(self.segments, kind, n_buckets)
        if (kind, n_buckets) not in self._counts:
            self._counts[(kind, n_buckets)] = quorum_ref.counts(self.segments, self.quorum, tables, n_buckets, self.order)
        rc, counts, found = self.count(tables, n_buckets)
        what = (label, kind, "B", n_buckets)
        assert rc == 0, what + (self.segs.err(),)
        np.testing.assert_array_equal(counts.astype(np.int64), self._counts[(kind, n_buckets)], err_msg=str(what))
        np.testing.assert_array_equal(found.astype(np.int64), self.founds, err_msg=str(what + ("found",)))
        np.testing.assert_array_equal(counts.sum(axis=1, dtype=np.int64), self.founds, err_msg=str(what + ("sum",)))

    def release(self):
        if self.segs.ctx:
            self.set_keys(self.keys)
        super().release()


class Ranked(grouped_shapes.Ranked):
    """a Family in score order: what after_shapes.walk and check_call drive"""

    def raw(self, k, cursors):
        fam = self.fam
        return nsbind.search_quorum_after_raw(fam.segs.ctx, fam.qd, fam.refs, fam.roles, fam.clauses, fam.needs, k,
                                              None if cursors is None else nsbind.cursors(cursors), fam.order, fam.handles)


class Dated(grouped_shapes.Dated):
    """a Family in date order under one direction"""

    def raw(self, k, cursors):
        fam = self.fam
        return nsbind.search_sorted_quorum_raw(fam.segs.ctx, fam.qd, fam.refs, fam.roles, fam.clauses, fam.needs, k, self.flags,
                                               None if cursors is None else nsbind.cursors(cursors), fam.order, fam.handles, fam.key_handles())


def directed_family(n_segs, pattern="pool5"):
    segments, queries, idfs, weights, order = directed_inputs(n_segs)
    return Family(segments, queries, idfs, weights, seg_order=order, keys=bss.keys_for(segments, pattern))


def run_directed(n_segs, tile_expected=None):
    """every directed case in facet counts, in score order and in both date directions, without and with skip tables"""
    tile = nsbind.facet_tile_docs()
    if tile_expected is not None:
        assert tile == tile_expected, (tile, tile_expected)
    fam = directed_family(n_segs)
    try:
        for with_skips in (False, True):
            if with_skips:
                for s in range(n_segs):
                    assert facet_shapes.build_skips(fam.segs, s) >= 1
            label = ("quorum directed", n_segs, "skips", with_skips)
            for B in BUCKETS:
                fam.check_counts(label, "modulo", B)
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


def run_walks(ks=(1, 7)):
    """score order and date order paged to exhaustion: per query the pages concatenated are the full ranking, nothing twice, rest
    counting down to 0 (after_shapes.walk asserts each).  K = 1 on one segment under equal keys (the docId decides every page),
    K = 7 on three segments in both directions."""
    pages = {}
    for k in ks:
        fam = directed_family(1, "same") if k == 1 else directed_family(3)
        try:
            assert max(fam.founds) > 100 and min(fam.founds) == 0
            pages[("score", k)] = after_shapes.walk(("quorum walk", "score"), Ranked(fam), k)
            for flags in ((0,) if k == 1 else (0, ASC)):
                pages[("date", k, flags)] = after_shapes.walk(("quorum walk", "date", hex(flags)), Dated(fam, flags), k)
        finally:
            fam.release()
    return pages


def product_inputs(tile):
    """grouped_shapes.product_inputs' segment of two tiles + 5 documents (lists 0 | 1 on either side of the first tile edge, 2 | 3 of
    the second, list 4 over everything with a posting at every edge, list 5 every 997th document) under counted clauses"""
    segments, _, idfs, weights, docs = grouped_shapes.product_inputs(tile)
    one = [[(0, M, 0, 2), (1, M, 0, 2), (4, M, 0, 2)], [(2, M, 0, 2), (3, M, 0, 2), (4, M, 0, 2), (5, M, 0, 2)], [(li, M, 0, 2) for li in range(4)],
           [(li, M, 0, 3) for li in range(6)], [(li, M, 3, 7) for li in range(6)] + [(4, M, 3, 7), (4, M, 3, 7)],
           [(0, M, 0, 2), (1, M, 0, 2), (4, M, 0, 2), (2, M, 1, 1), (3, M, 1, 1), (4, M, 1, 1), (5, X, 0, 0)], [(4, M, 0, 2), (5, M, 0, 2), (0, S, 0, 0)]]
    return segments, [[(0, li, r, c, m) for li, r, c, m in q] for q in one], idfs, weights, docs


def run_product_tile():
    """the product build's tile and its planes of 16 KiB: members on either side of a tile edge, in facet counts, in score order and
    in date order under equal keys (the docId decides across the edge)"""
    tile = nsbind.facet_tile_docs()
    segments, queries, idfs, weights, docs = product_inputs(tile)
    n = int(segments[0][0])
    fam = Family(segments, queries, idfs, weights, keys=bss.keys_for(segments, "same"))
    try:
        in4 = set(docs[4].tolist())
        assert fam.founds[0] == len(in4 & (set(docs[0].tolist()) | set(docs[1].tolist()))) >= 40 and fam.founds[2] == 0 and fam.founds[4] == 0, fam.founds
        assert fam.founds[1] >= 9 and fam.founds[5] >= 1 and fam.founds[6] >= 1, fam.founds
        d = np.arange(n, dtype=np.int64)
        table = (d // tile).astype(np.uint16)
        for with_skips in (False, True):
            if with_skips:
                assert facet_shapes.build_skips(fam.segs, 0) >= 1
            rc, counts, found = fam.count([table], 8)
            assert rc == 0, fam.segs.err()
            np.testing.assert_array_equal(counts.astype(np.int64), quorum_ref.counts(segments, queries, [table], 8))
            np.testing.assert_array_equal(found.astype(np.int64), fam.founds)
            for k in (1, 65, 100):
                Ranked(fam).check(("quorum product tile", tile, with_skips), k)
                Dated(fam, 0).check(("quorum product tile", tile, with_skips), k)
    finally:
        fam.release()
    return tile, n


# ---- equivalences on the same raw inputs --------------------------------------------------------------------------------
def same_bytes(label, got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), (label, "output", i)


def three_calls(fam, call, roles, clauses, needs, k, flags, cursors):
    """the ranked, the dated and (no cursors) the counting call of one family under one set of per-ref arrays -> every output array"""
    ctx, cu = fam.segs.ctx, None

    def ranked(cu):
        if call == "quorum":
            return nsbind.search_quorum_after_raw(ctx, fam.qd, fam.refs, roles, clauses, needs, k, cu, fam.order, fam.handles)
        if call == "grouped":
            return nsbind.search_grouped_after_raw(ctx, fam.qd, fam.refs, roles, clauses, k, cu, fam.order, fam.handles)
        return nsbind.search_boolean_after_raw(ctx, fam.qd, fam.refs, roles, k, cu, fam.order, fam.handles)

    def dated(cu):
        if call == "quorum":
            return nsbind.search_sorted_quorum_raw(ctx, fam.qd, fam.refs, roles, clauses, needs, k, flags, cu, fam.order, fam.handles, fam.key_handles())
        if call == "grouped":
            return nsbind.search_sorted_grouped_raw(ctx, fam.qd, fam.refs, roles, clauses, k, flags, cu, fam.order, fam.handles, fam.key_handles())
        return nsbind.search_sorted_boolean_raw(ctx, fam.qd, fam.refs, roles, k, flags, cu, fam.order, fam.handles, fam.key_handles())

    Q, out = len(fam.qd), []
    rc, hits, nhits, found, rest, _ = ranked(None)
    assert rc == 0, fam.segs.err()
    if cursors:
        last = [None if not nhits[q] else (int(hits[q, nhits[q] - 1]["score"].view(np.uint32)), int(hits[q, nhits[q] - 1]["seg"]), int(hits[q, nhits[q] - 1]["doc"]))
                for q in range(Q)]
        rc, hits, nhits, found, rest, _ = ranked(nsbind.cursors(last))
        assert rc == 0, fam.segs.err()
    out += [hits, nhits, found, rest]
    rc, hits, keys, nhits, found, rest, _ = dated(None)
    assert rc == 0, fam.segs.err()
    if cursors:
        last = [None if not nhits[q] else (int(keys[q, nhits[q] - 1]), int(hits[q, nhits[q] - 1]["seg"]), int(hits[q, nhits[q] - 1]["doc"])) for q in range(Q)]
        rc, hits, keys, nhits, found, rest, _ = dated(nsbind.cursors(last))
        assert rc == 0, fam.segs.err()
    out += [hits, keys, nhits, found, rest]
    if not cursors:
        rc, counts, found = fam.count(bss.tables_for(fam.segments, "modulo", 50), 50, roles=roles, clauses=clauses, needs=needs, call=call)
        assert rc == 0, fam.segs.err()
        out += [counts, found]
    return out


def compare(label, fam, got, want):
    """got / want: (call, roles, clauses, needs); every output array of the three calls, byte for byte, with and without cursors"""
    for k in (7, 64, 100):
        for flags in (0, ASC):
            for cursors in (False, True):
                same_bytes(label + (k, flags, cursors), three_calls(fam, *got, k, flags, cursors), three_calls(fam, *want, k, flags, cursors))


def grouped_as_quorum(n_segs):
    """grouped_shapes' directed family (any-of clauses of every shape) as a quorum Family whose needs are all 1"""
    segments, queries, idfs, weights, order = grouped_shapes.directed_inputs(n_segs)
    return Family(segments, [[(s, li, r, c, 1) for s, li, r, c in q] for q in queries], idfs, weights, seg_order=order)


def run_needs_null_is_the_sibling():
    """needs == NULL IS the grouped call (and, without clauses, the boolean call): every byte, and the quorum kernels' times stay 0"""
    fam = grouped_as_quorum(3)
    try:
        nsbind.quorum_kernel_ms(reset=True)
        nsbind.grouped_kernel_ms(reset=True)
        compare(("needs NULL",), fam, ("quorum", fam.roles, fam.clauses, None), ("grouped", fam.roles, fam.clauses, None))
        compare(("needs and clauses NULL",), fam, ("quorum", fam.roles, None, None), ("boolean", fam.roles, None, None))
        compare(("roles NULL",), fam, ("quorum", None, fam.clauses, fam.needs), ("boolean", None, None, None))   # no MUST ref: nothing reads them
        assert all(v == 0.0 for v in nsbind.quorum_kernel_ms()) and all(v > 0.0 for v in nsbind.grouped_kernel_ms())
    finally:
        fam.release()


def run_all_ones_equal_the_sibling():
    """needs all 1 (or all 0, which reads as 1) give the grouped call's answers through the quorum kernels"""
    covered = 0
    for n_segs in (1, 3):
        fam = grouped_as_quorum(n_segs)
        try:
            nsbind.quorum_kernel_ms(reset=True)
            compare(("all ones", n_segs), fam, ("quorum", fam.roles, fam.clauses, fam.needs), ("grouped", fam.roles, fam.clauses, None))
            compare(("all zeros", n_segs), fam, ("quorum", fam.roles, fam.clauses, np.zeros_like(fam.needs)), ("grouped", fam.roles, fam.clauses, None))
            assert all(v > 0.0 for v in nsbind.quorum_kernel_ms())
            covered += sum(f >= 2 for f in fam.founds)
        finally:
            fam.release()
    assert covered >= FLOOR_ONES, covered
    return covered


FLOOR_ONES = 16              # queries with found >= 2 that the all-ones comparison must cover (test_quorum_cpu counts them)
FLOOR_FULL = 4               # ... and the need = members comparison


def full_need_inputs():
    """boolean_shapes' all-MUST family (every list non-empty, every docId in range): per (query, segment) ONE clause whose need is the
    number of its distinct lists; queries with more than seven lists in a segment are left out -> the quorum form and the boolean
    form of the same refs"""
    segments, queries, idfs, weights = boolean_shapes.same_role_inputs(M)
    quorum, plain = [], []
    for q in queries:
        per_seg = {}
        for s, li, _ in q:
            per_seg.setdefault(s, set()).add(li)
        if not q or max(len(v) for v in per_seg.values()) > quorum_ref.MAX_NEED:
            continue
        quorum.append([(s, li, M, 11, len(per_seg[s])) for s, li, _ in q])
        plain.append([(s, li, M) for s, li, _ in q])
    return segments, quorum, plain, idfs, weights


def run_need_equal_to_the_members_is_singleton_clauses():
    """a clause of n distinct lists with need n == n one-term clauses == every ref MUST in the boolean call; and "three of three"
    of the directed family against its singleton form"""
    segments, quorum, plain, idfs, weights = full_need_inputs()
    fam = Family(segments, quorum, idfs, weights, seg_order=[2, 0, 1])
    try:
        covered = sum(f >= 2 for f in fam.founds)
        assert covered >= FLOOR_FULL and int(fam.needs.max()) >= 3, (covered, fam.needs.max())
        singles = np.arange(len(fam.refs), dtype=np.uint16)
        compare(("need = members", "boolean"), fam, ("quorum", fam.roles, fam.clauses, fam.needs), ("boolean", fam.roles, None, None))
        compare(("need = members", "singletons"), fam, ("quorum", fam.roles, fam.clauses, fam.needs), ("quorum", fam.roles, singles, np.ones_like(fam.needs)))
    finally:
        fam.release()
    segments, queries, idfs, weights, order = directed_inputs(3, [CASES["three of three"], CASES["saturation: seven of ten"][:7]])
    fam = Family(segments, queries, idfs, weights, seg_order=order)
    try:
        assert min(fam.founds) >= 2
        compare(("need = members", "directed"), fam, ("quorum", fam.roles, fam.clauses, fam.needs), ("grouped", fam.roles, np.arange(len(fam.refs), dtype=np.uint16), None))
    finally:
        fam.release()
    return covered


# ---- refusals -----------------------------------------------------------------------------------------------------------
def run_refusals():
    """the three refusals of the needs under each call's name: NS_E_INVAL with the message, nothing launched, the outputs keep their
    fill; the siblings' refusals still come first"""
    import ctypes as Ct

    L = nsbind.hip_lib()
    segments, queries, idfs, weights, order = directed_inputs(3)
    fam = Family(segments, queries, idfs, weights, seg_order=order)
    ctx, B = fam.segs.ctx, 50
    tabs = [nsbind.facet_upload(ctx, t, B)[1] for t in [bss.tables_for(segments, "modulo", B)[s] for s in order]]
    try:
        def refused(name, rc, outs, match):
            if match is None:
                assert rc == 0, L.ns_last_error(ctx).decode()
                return
            msg = L.ns_last_error(ctx).decode()
            assert rc == NS_E_INVAL and (name + ": ") in msg and match in msg, (rc, msg)
            for o in outs:
                fill = 0xAB if o.dtype == nsbind.HIT_DTYPE else 0xABABABAB
                assert np.all((o.view(np.uint8) if o.dtype == nsbind.HIT_DTYPE else o) == fill), "a refused call writes nothing"

        def ranked(match, roles=fam.roles, clauses=fam.clauses, needs=fam.needs):
            rc, *outs = nsbind.search_quorum_after_raw(ctx, fam.qd, fam.refs, roles, clauses, needs, 10, None, order, fam.handles)
            refused("ns_search_quorum_after", rc, outs[:4], match)

        def count(match, roles=fam.roles, clauses=fam.clauses, needs=fam.needs):
            rc, *outs = nsbind.facet_count_quorum(ctx, fam.qd, fam.refs, roles, clauses, needs, order, fam.handles, tabs, B)
            refused("ns_facet_count_quorum", rc, outs[:2], match)

        def dated(match, roles=fam.roles, clauses=fam.clauses, needs=fam.needs):
            rc, *outs = nsbind.search_sorted_quorum_raw(ctx, fam.qd, fam.refs, roles, clauses, needs, 10, 0, None, order, fam.handles, fam.key_handles())
            refused("ns_search_sorted_quorum", rc, outs[:5], match)

        q2 = NAMES.index("two of three")
        first = int(fam.qd[q2]["term_begin"])
        for call in (ranked, count, dated):
            call(None)
            eight = fam.needs.copy()
            eight[first] = 8
            call("ref %d: a need of 8 (query %d); at most 7" % (first, q2), needs=eight)
            differ = fam.needs.copy()
            differ[first + 3] = 3                                          # the second ref of the clause in the first segment
            call("query %d: the refs of clause 0 carry the needs 2 and 3" % q2, needs=differ)
            call("needs without clauses", clauses=None)
            bad = fam.roles.copy()
            bad[first] = 3
            call("ref %d: role 3 is none of" % first, roles=bad)
            on_should = fam.needs.copy()
            on_should[fam.roles != M] = 255                                # never read
            call(None, needs=on_should)
        assert L.ns_search_quorum_after(ctx, None, 0, None, None, None, None, 0, 10, None, None, None, 0, None, None, None, None, None) == 0
        assert L.ns_facet_count_quorum(ctx, None, 0, None, None, None, None, 0, None, None, None, 0, None, None, None) == 0
        assert L.ns_search_sorted_quorum(ctx, None, 0, None, None, None, None, 0, 10, 0, None, None, None, None, 0, None, None, None, None, None, None) == 0
        assert L.ns_search_quorum_after(None, None, 0, None, None, None, None, 0, 10, None, None, None, 0, None, None, None, None, None) == NS_E_INVAL
        out6 = (Ct.c_float * 6)()
        assert L.ns_quorum_kernel_ms(out6, 1) == 0 and all(v > 0.0 for v in out6), list(out6)
        ranked(None)
        assert L.ns_quorum_kernel_ms(out6, 1) == 0 and out6[0] > 0.0 and out6[1] > 0.0 and all(v == 0.0 for v in out6[2:]), list(out6)
        assert L.ns_quorum_kernel_ms(None, 0) == NS_E_INVAL
    finally:
        for h in tabs:
            nsbind.facet_release(ctx, h)
        fam.release()


def main(out_path):
    """child process at NS_FACET_TILE_DOCS = 128 and NS_BOOL_WIN_DOCS = 32.  Both builds run the directed families; the counting
    build reports the counters of those; the variants build runs the walks and the equivalences."""
    counting = "ns_debug_boolean_quorum_counters" in nsbind.debug_counters(reset=True)
    assert os.environ.get("NS_BOOL_WIN_DOCS") == str(SMALL_WIN)
    rep = {"tile": run_directed(1, tile_expected=SMALL_TILE), "counting": counting}
    run_directed(3)
    if counting:
        rep["events"] = nsbind.quorum_counters(reset=True)
        rep["missed"] = [e for e in EVENTS if rep["events"][e] == 0]
        print("quorum", rep["events"], flush=True)
    else:
        rep["pages"] = {str(k): v for k, v in run_walks().items()}
        run_needs_null_is_the_sibling()
        rep["ones"] = run_all_ones_equal_the_sibling()
        rep["full"] = run_need_equal_to_the_members_is_singleton_clauses()
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print("quorum shapes OK")


if __name__ == "__main__":
    main(sys.argv[1])
