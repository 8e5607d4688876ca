"""Directed inputs of ns_search_boolean_after and ns_search_sorted_after (csrc/ns_after_plan.hpp, csrc/ns_after.hip; DESIGN.md
§5s) and the code that runs them through the raw C-ABI against the restatement (tests/after_ref.py).  The families are
boolean_shapes' and sorted_shapes'.  All comparisons are exact, score bits included.

Imported by tests/test_after_gpu.py for the product library (one tile and one window hold the 300-document families), and
run as a program in a child process that loaded the variants or the counting build with NS_FACET_TILE_DOCS=128
NS_BOOL_WIN_DOCS=32: there the 300 documents span two whole tiles and a part, so that a cursor falls before, inside and
behind tiles of its own segment; the variants child also crosses the candidate buffer (sub-batches), the counting child
reports ns_debug_after_counters."""
import bisect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "nextsearch-api_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import after_ref  # noqa: E402
import boolean_shapes  # noqa: E402
import facet_shapes  # noqa: E402
import nsbind  # noqa: E402
import sorted_shapes  # noqa: E402
from boolean_ref import MUST, NOT, SHOULD  # noqa: E402
from rawseg import _np_bm25, avgdl_of  # noqa: E402

AND, ASC = nsbind.NS_FLAG_AND, nsbind.NS_SORT_ASC
SMALL_TILE, SMALL_WIN, N_DOCS = boolean_shapes.SMALL_TILE, boolean_shapes.SMALL_WIN, boolean_shapes.N_DOCS
WALK_KS = [7, 64, 65, 100]
PAD_SCORE_BITS, PAD_ID = 0xFF800000, 0xFFFFFFFF
CAND_BYTES = 64 << 20                                    # kSdCandBytes
EDGE_DOCS = [31, 32, 127, 128, 255, 256, 299, 300, 0xFFFFFFFF]
BITS = {"+0": 0x00000000, "-0": 0x80000000, "+inf": 0x7F800000, "-inf": 0xFF800000, "top": 0x7FFFFFFF, "bottom": 0xFFFFFFFF}


# ---- one page against the restatement -----------------------------------------------------------------------------------
def check_page(label, rows, cursor, k, hits, nhits, found, rest, order, keys=None):
    """one query's outputs against after_ref.page: found, rest, nhits, (seg, doc), the reported rank bits and the padding.
    rows: the query's full order; cursor: None or (mapped rank, pos, doc); order: position -> seg_id."""
    K = min(max(int(k), 1), 100)
    want_rest, want = after_ref.page(rows, cursor, K)
    assert int(found) == len(rows), (label, "found", int(found), len(rows))
    assert int(rest) == want_rest, (label, "rest", int(rest), want_rest)
    n = int(nhits)
    assert n == len(want) == min(K, want_rest), (label, "nhits", n, len(want))
    got = [(int(s), int(d)) for s, d in zip(hits[:n]["seg"], hits[:n]["doc"])]
    exp = [(r[3], r[2]) for r in want]
    assert got == exp, (label, "(seg, doc)", got[:4], exp[:4])
    if keys is None:
        assert [int(b) for b in hits[:n]["score"].view(np.uint32)] == [r[4] for r in want], (label, "score bits")
    else:
        assert [int(x) for x in keys[:n]] == [r[4] for r in want], (label, "keys")
        assert [int(b) for b in hits[:n]["score"].view(np.uint32)] == [r[5] for r in want], (label, "score bits")
        assert np.all(keys[n:K] == 0), (label, "key padding")
    tail = hits[n:K]
    assert np.all(tail["score"].view(np.uint32) == PAD_SCORE_BITS) and np.all(tail["seg"] == PAD_ID) and np.all(tail["doc"] == PAD_ID), (label, "padding")


class Boolean:
    """a boolean_shapes.Family and its full order"""

    def __init__(self, fam):
        self.fam = fam
        self.rows = after_ref.boolean_rows(fam.segments, fam.queries, fam.order, fam.idfs, fam.weights)
        self.handles = [fam.segs.segs[s] for s in fam.order]

    def call(self, k, cursors, roles="own"):
        """cursors: None, or per query None | (score bits, seg_id, doc)"""
        fam = self.fam
        rc, hits, nhits, found, rest, _ = nsbind.search_boolean_after_raw(fam.segs.ctx, fam.qd, fam.refs, fam.roles if isinstance(roles, str) else roles, k,
                                                                          None if cursors is None else nsbind.cursors(cursors), fam.order, self.handles)
        assert rc == 0, fam.segs.err()
        return hits, None, nhits, found, rest

    def mapped(self, c):
        return None if c is None else (after_ref.ord32(c[0]), self.fam.order.index(c[1]), c[2])

    def next_cursor(self, hits, keys, q, n):
        h = hits[q, n - 1]
        return (int(h["score"].view(np.uint32)), int(h["seg"]), int(h["doc"]))

    def release(self):
        self.fam.release()


def sorted_rows_scored(fam, and_mode, ascending):
    """after_ref.sorted_rows with the score bits of every document as a sixth field"""
    rows = after_ref.sorted_rows(fam.segments, fam.queries, fam.keys, and_mode, ascending, fam.order)
    out = []
    for qi, (q, rr) in enumerate(zip(fam.queries, rows)):
        acc_of = fam.cache.setdefault(("after_acc", qi), {})
        scored = []
        for r in rr:
            s = r[3]
            if s not in acc_of:
                n_docs, doc_len, lists = fam.segments[s]
                numbers = [li for ss, li in q if ss == s]
                dl = np.ascontiguousarray(doc_len, dtype=np.uint32)
                inside = [(lists[li][0][lists[li][0] < n_docs], lists[li][1][lists[li][0] < n_docs]) for li in range(len(lists))]
                acc_of[s] = _np_bm25(inside, numbers, [fam.idfs[s][li] for li in numbers], [fam.weights[s][li] for li in numbers], dl, avgdl_of(dl))
            scored.append(r + (int(np.float32(acc_of[s][r[2]]).view(np.uint32)),))
        out.append(scored)
    return out


class Sorted:
    """a sorted_shapes.Family under one set of flags, and its full order"""

    def __init__(self, fam, flags):
        self.fam, self.flags = fam, flags
        self.rows = sorted_rows_scored(fam, bool(flags & AND), bool(flags & ASC))
        self.handles = [fam.segs.segs[s] for s in fam.order]

    def call(self, k, cursors):
        """cursors: None, or per query None | (key as uploaded, seg_id, doc)"""
        fam = self.fam
        rc, hits, keys, nhits, found, rest, _ = nsbind.search_sorted_after_raw(fam.segs.ctx, fam.qd, fam.refs, k, self.flags,
                                                                              None if cursors is None else nsbind.cursors(cursors), fam.order, self.handles,
                                                                              [fam.table(s) for s in fam.order])
        assert rc == 0, fam.segs.err()
        return hits, keys, nhits, found, rest

    def mapped(self, c):
        return None if c is None else (after_ref.sort_rank(c[0], bool(self.flags & ASC)), self.fam.order.index(c[1]), c[2])

    def next_cursor(self, hits, keys, q, n):
        h = hits[q, n - 1]
        return (int(keys[q, n - 1]), int(h["seg"]), int(h["doc"]))


def check_call(label, side, k, cursors, out):
    hits, keys, nhits, found, rest = out
    for q, rows in enumerate(side.rows):
        c = None if cursors is None else cursors[q]
        check_page((label, "k", k, "query", q, "cursor", c), rows, side.mapped(c), k, hits[q], nhits[q], found[q], rest[q], side.fam.order,
                   None if keys is None else keys[q])


def walk(label, side, k):
    """batch all queries; hand each query's last hit back (an exhausted query keeps its cursor) until every nhits is 0.  Per
    query the concatenation of the pages is the full order; on every page found is constant, rest falls by the previous
    nhits and the tail is padded.  Returns the number of pages."""
    Q, K = len(side.rows), min(max(int(k), 1), 100)
    cursors, seen, pages = None, [0] * Q, 0
    while True:
        hits, keys, nhits, found, rest = side.call(k, cursors)
        pages += 1
        nxt = [None] * Q if cursors is None else list(cursors)
        for q, rows in enumerate(side.rows):
            n = int(nhits[q])
            what = (label, "k", k, "page", pages, "query", q)
            assert int(found[q]) == len(rows), what + ("found", int(found[q]), len(rows))
            assert int(rest[q]) == len(rows) - seen[q], what + ("rest", int(rest[q]), len(rows) - seen[q])
            assert n == min(K, int(rest[q])), what + ("nhits", n)
            want = rows[seen[q]:seen[q] + n]
            got = [(int(s), int(d)) for s, d in zip(hits[q, :n]["seg"], hits[q, :n]["doc"])]
            assert got == [(r[3], r[2]) for r in want], what + ("(seg, doc)", got[:3], [(r[3], r[2]) for r in want[:3]])
            bits = [int(b) for b in hits[q, :n]["score"].view(np.uint32)]
            if keys is None:
                assert bits == [r[4] for r in want], what + ("score bits",)
            else:
                assert [int(x) for x in keys[q, :n]] == [r[4] for r in want], what + ("keys",)
                assert bits == [r[5] for r in want], what + ("score bits",)
                assert np.all(keys[q, n:K] == 0), what + ("key padding",)
            tail = hits[q, n:K]
            assert np.all(tail["score"].view(np.uint32) == PAD_SCORE_BITS) and np.all(tail["seg"] == PAD_ID) and np.all(tail["doc"] == PAD_ID), what + ("padding",)
            if n:
                nxt[q] = side.next_cursor(hits, keys, q, n)
                seen[q] += n
        if not np.any(nhits):
            break
        cursors = nxt
        assert pages <= 2 + max(len(r) for r in side.rows), label
    assert seen == [len(r) for r in side.rows], label                  # nothing skipped, nothing repeated: the whole ranking
    return pages


# ---- boolean ------------------------------------------------------------------------------------------------------------
def multi_boolean(role=SHOULD):
    return Boolean(boolean_shapes.Family(*boolean_shapes.same_role_inputs(role), seg_order=[2, 0, 1]))


def mixed_multi_boolean():
    """the multi family with a role per ref: MUST, SHOULD and NOT by turns"""
    segments, queries = boolean_shapes.multi_family()
    mixed = [[(s, li, (MUST, SHOULD, NOT, SHOULD)[(qi + i) % 4]) for i, (s, li) in enumerate(q)] for qi, q in enumerate(queries)]
    return Boolean(boolean_shapes.Family(segments, mixed, *boolean_shapes.multi_weights(segments), seg_order=[2, 0, 1]))


def run_boolean_walks(ks=WALK_KS):
    """every role mix of boolean_shapes.DIRECTED over one and three segments, the multi-segment family with one role and with
    mixed roles, K = 7, 64, 65, 100; the tied family at K = 1"""
    pages = {}
    for name, make in (("directed 1", lambda: Boolean(boolean_shapes.directed_family(1))), ("directed 3", lambda: Boolean(boolean_shapes.directed_family(3))),
                       ("multi should", lambda: multi_boolean(SHOULD)), ("multi must", lambda: multi_boolean(MUST)), ("multi mixed", mixed_multi_boolean)):
        side = make()
        try:
            assert max(len(r) for r in side.rows) > 100 and min(len(r) for r in side.rows) == 0, name
            for k in ks:
                pages[(name, k)] = walk(("boolean walk", name), side, k)
        finally:
            side.release()
    return pages


def run_tied_walk():
    """K = 1 through tie groups that straddle windows, tiles and segments: every page is decided by (segment, doc) alone"""
    side = Boolean(boolean_shapes.tied_family())
    try:
        n = walk(("boolean walk", "tied"), side, 1)
        assert n == 1 + max(len(r) for r in side.rows) == 901, n
        return n
    finally:
        side.release()


def arbitrary_cursors(side, rank_of_row, between):
    """per query a list of cursors (rank as the call takes it, seg_id, doc): a rank equal to a document's with (segment, doc)
    before all, between and after all of that rank's documents, at the edge docIds in the first, middle and last segment;
    ranks between two documents'; the special values"""
    order = side.fam.order
    out = []
    for rows in side.rows:
        cs = []
        if rows:
            for r in (rows[0], rows[len(rows) // 2], rows[-1]):
                for seg in (order[0], order[len(order) // 2], order[-1]):
                    cs += [(rank_of_row(r), seg, d) for d in EDGE_DOCS + [0]]
                cs.append((rank_of_row(r), r[3], r[2]))                                   # the document itself
                cs.append((rank_of_row(r), r[3], max(r[2] - 1, 0)))
            cs += [(x, order[len(order) // 2], 128) for x in between(rows)]
        out.append(cs)
    return out


def run_cursor_rounds(label, side, per_query, specials, k):
    """round i gives query q its i-th cursor (None once its list is used up: set and unset cursors mix), then every query the
    same special cursor"""
    rounds = max(len(c) for c in per_query)
    assert rounds >= 30, (label, rounds)
    for i in range(rounds):
        cursors = [c[i] if i < len(c) else None for c in per_query]
        check_call((label, "round", i), side, k, cursors, side.call(k, cursors))
    for name, c in specials:
        cursors = [c if q % 5 else None for q in range(len(side.rows))]              # every fifth query without a cursor
        check_call((label, name), side, k, cursors, side.call(k, cursors))
    return rounds


def run_boolean_cursors():
    """arbitrary cursors on the tied family (three segments listed as 1, 2, 0; large tie groups) against after_ref"""
    side = Boolean(boolean_shapes.tied_family())
    try:
        order = side.fam.order

        def between(rows):
            have = {r[4] for r in rows}
            return [b for b in sorted({r[4] + 1 for r in rows} | {r[4] - 1 for r in rows if r[4]}) if b not in have][:4]

        per_query = arbitrary_cursors(side, lambda r: r[4], between)
        specials = [(n, (BITS[n], order[1], 128)) for n in ("+0", "-0", "+inf", "-inf")]
        specials += [("above everything", (BITS["top"], order[0], 0)), ("below everything", (BITS["bottom"], order[-1], 0xFFFFFFFF))]
        for k in (10, 100):
            run_cursor_rounds("boolean cursors", side, per_query, specials, k)
        # above everything: the answer without a cursor; below everything: nothing left, found intact
        plain = side.call(100, None)
        top = side.call(100, [(BITS["top"], order[0], 0)] * len(side.rows))
        for a, b in zip(plain, top):
            assert a is b is None or (a.tobytes() == b.tobytes()), "a cursor above everything"
        _, _, nhits, found, rest = side.call(100, [(BITS["bottom"], order[-1], 0xFFFFFFFF)] * len(side.rows))
        assert not np.any(nhits) and not np.any(rest) and list(found) == [len(r) for r in side.rows] and max(found) > 100
        # all cursors unset: the entry point without cursors, byte for byte
        fam = side.fam
        rc, hits0, nhits0, found0, _ = nsbind.search_boolean_raw(fam.segs.ctx, fam.qd, fam.refs, fam.roles, 100, fam.order, side.handles)
        assert rc == 0
        for cursors in (None, [None] * len(side.rows)):
            hits, _, nhits, found, rest = side.call(100, cursors)
            assert hits.tobytes() == hits0.tobytes() and nhits.tobytes() == nhits0.tobytes() and found.tobytes() == found0.tobytes() and rest.tobytes() == found0.tobytes()
    finally:
        side.release()


# ---- sorted -------------------------------------------------------------------------------------------------------------
def small_sorted_family(pattern):
    lists = facet_shapes.small_lists()
    segments = [(N_DOCS, (5 + np.arange(N_DOCS) % 41).astype(np.uint32), lists)]
    queries = [[(0, li) for li in q] for q in facet_shapes.SMALL_QUERIES]
    idfs, weights = sorted_shapes.small_weights(len(lists))
    return sorted_shapes.Family(segments, queries, [sorted_shapes.keys_of(pattern, N_DOCS)], idfs, weights)


def multi_sorted_family(pattern):
    segments, queries = sorted_shapes.multi_family()
    idfs = [[1.0 + 0.5 * i for i in range(len(s[2]))] for s in segments]
    weights = [[1.0 if i % 2 else 0.75 for i in range(len(s[2]))] for s in segments]
    keys = [sorted_shapes.keys_of(pattern, s[0], seed=40 + i) for i, s in enumerate(segments)]
    return sorted_shapes.Family(segments, queries, keys, idfs, weights, seg_order=[2, 0, 1])


def run_sorted_walks(pattern, ks=WALK_KS):
    """OR / AND x newest / oldest on the 300-document family and on the three-segment family under one key pattern ("same" and
    "half_undated" are all ties: the segment and the docId decide)"""
    pages = {}
    for name, make in (("small", small_sorted_family), ("multi", multi_sorted_family)):
        fam = make(pattern)
        try:
            for flags in (0, ASC, AND, AND | ASC):
                side = Sorted(fam, flags)
                assert max(len(r) for r in side.rows) > (100 if not flags & AND else 7), (name, pattern, flags)
                for k in ks:
                    pages[(name, flags, k)] = walk(("sorted walk", name, pattern, hex(flags)), side, k)
        finally:
            fam.release()
    return pages


def run_sorted_cursors():
    """arbitrary cursors on the three-segment family (fifty key values, equal across the segments) against after_ref"""
    segments, queries = sorted_shapes.multi_family()
    idfs = [[1.0 + 0.5 * i for i in range(len(s[2]))] for s in segments]
    weights = [[1.0 if i % 2 else 0.75 for i in range(len(s[2]))] for s in segments]
    keys = [np.where(np.arange(s[0]) % 9 == 4, 0, 20200101 + 2 * (np.arange(s[0]) % 50)).astype(np.uint32) for s in segments]   # even values, some undated
    fam = sorted_shapes.Family(segments, queries, keys, idfs, weights, seg_order=[2, 0, 1])
    try:
        order = fam.order
        for flags in (0, ASC, AND | ASC):
            side = Sorted(fam, flags)
            per_query = arbitrary_cursors(side, lambda r: r[4], lambda rows: sorted({r[4] + 1 for r in rows if r[4]})[:4])
            specials = [("undated", (0, order[1], 128)), ("key 1", (1, order[1], 128)), ("largest key", (0xFFFFFFFE, order[0], 0)),
                        ("below everything", (0, order[-1], 0xFFFFFFFF))]
            for k in (10, 100):
                run_cursor_rounds(("sorted cursors", hex(flags)), side, per_query, specials, k)
            above = (1 if flags & ASC else 0xFFFFFFFE, order[0], 0)
            plain = side.call(100, None)
            top = side.call(100, [above] * len(side.rows))
            for a, b in zip(plain, top):
                assert a.tobytes() == b.tobytes(), "a cursor above everything"
            _, _, nhits, found, rest = side.call(100, [(0, order[-1], 0xFFFFFFFF)] * len(side.rows))
            assert not np.any(nhits) and not np.any(rest) and list(found) == [len(r) for r in side.rows] and max(found) > 100
            rc, hits0, keys0, nhits0, found0, _ = nsbind.search_sorted_raw(fam.segs.ctx, fam.qd, fam.refs, 100, flags, fam.order, side.handles,
                                                                           [fam.table(s) for s in fam.order])
            assert rc == 0
            for cursors in (None, [None] * len(side.rows)):
                hits, kk, nhits, found, rest = side.call(100, cursors)
                assert hits.tobytes() == hits0.tobytes() and kk.tobytes() == keys0.tobytes() and nhits.tobytes() == nhits0.tobytes()
                assert found.tobytes() == found0.tobytes() and rest.tobytes() == found0.tobytes()
    finally:
        fam.release()


# ---- sub-batches (variants build: tiles of 128 documents) ---------------------------------------------------------------
def run_sub_batches():
    """copies of the multi-family queries until work items x K x 8 B cross the candidate buffer at K = 100, every copy with a
    cursor of its own: last[] is indexed by the call's item number across the sub-batches of sd_cut"""
    tile = nsbind.facet_tile_docs()
    K = 100
    segments, queries = boolean_shapes.multi_family()
    base = Boolean(boolean_shapes.Family(*boolean_shapes.same_role_inputs(SHOULD), seg_order=[2, 0, 1]))
    try:
        # sd_cut's rule: a sub-batch takes queries while its items' rows fit cand_bytes / (8 K); an item per tile of every
        # segment a query has a non-empty ref in
        tiles = [(s[0] + tile - 1) // tile for s in segments]
        items_of = [sum(tiles[s] for s in {s for s, _ in q}) for q in queries]
        max_items = CAND_BYTES // (8 * K)
        copies = max_items // sum(items_of) + 2
        n_items = copies * sum(items_of)
        assert n_items > max_items and n_items * K * 8 > CAND_BYTES and max(items_of) <= max_items, (n_items, max_items)
        fam = base.fam
        Q0, R0 = len(fam.qd), len(fam.refs)
        qd = np.tile(fam.qd, copies)
        qd["term_begin"] += np.repeat(np.arange(copies, dtype=np.uint32) * R0, Q0)
        refs = np.tile(fam.refs, copies)
        # copy c, query q: the cursor is the document at rank (37 c + 11 q) mod found of that query's order; every seventh unset
        cursors, want = [], []
        for c in range(copies):
            for q, rows in enumerate(base.rows):
                if not rows or (c + q) % 7 == 0:
                    cursors.append(None)
                    want.append((len(rows), 0))
                    continue
                r = rows[(37 * c + 11 * q) % len(rows)]
                cursors.append((r[4], r[3], r[2]))
                want.append((len(rows), (37 * c + 11 * q) % len(rows) + 1))
        rc, hits, nhits, found, rest, _ = nsbind.search_boolean_after_raw(fam.segs.ctx, qd, refs, None, K, nsbind.cursors(cursors), fam.order, base.handles)
        assert rc == 0, fam.segs.err()
        places = [[after_ref.position(*r[:3]) for r in rows] for rows in base.rows]
        for i, (n_rows, at) in enumerate(want):
            rows, pos = base.rows[i % Q0], places[i % Q0]
            c = base.mapped(cursors[i])
            assert at == (0 if c is None else bisect.bisect_right(pos, after_ref.position(*c)))       # the plain comparison, on a sorted list
            n = int(nhits[i])
            assert int(found[i]) == n_rows and int(rest[i]) == n_rows - at and n == min(K, n_rows - at), ("sub-batches", i)
            exp = rows[at:at + n]
            assert [(int(s), int(d)) for s, d in zip(hits[i, :n]["seg"], hits[i, :n]["doc"])] == [(r[3], r[2]) for r in exp], ("sub-batches", i)
            assert [int(b) for b in hits[i, :n]["score"].view(np.uint32)] == [r[4] for r in exp], ("sub-batches", i)
            assert np.all(hits[i, n:]["doc"] == PAD_ID)
        return {"copies": copies, "items": n_items, "max_items": max_items}
    finally:
        base.release()


# ---- the product build's tile and window --------------------------------------------------------------------------------
def run_product_edges():
    """boolean_shapes.run_product_tile's family of two product tiles + 5 documents (equal scores in runs that straddle a window
    edge, both tile edges and the end); cursors at the documents 2^13 - 1, 2^13, 2^17 - 1, 2^17 and 262 148"""
    tile = nsbind.facet_tile_docs()
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
    S, M, X = SHOULD, MUST, NOT
    one = [[(0, S)], [(1, S)], [(0, S), (1, S)], [(0, M), (1, S)], [(0, M), (4, X)], [(0, M), (4, M)], [(1, M), (2, M)], [(0, S), (1, S), (2, S), (3, X)],
           [(3, M), (0, M), (1, S)], [(2, S), (2, S)], [(3, X)], [(4, S), (0, X)], [(1, M), (1, X)], [(0, M), (0, S), (4, S), (3, X)]]
    queries = [[(0, li, r) for li, r in q] for q in one]
    idf, w = boolean_shapes.small_weights(len(lists))
    side = Boolean(boolean_shapes.Family(segments, queries, [idf], [w]))
    try:
        assert len({r[4] for r in side.rows[0]}) == 1 and len(side.rows[0]) == len(docs[0])          # one tie group: the docId alone decides
        at = [(1 << 13) - 1, 1 << 13, (1 << 17) - 1, 1 << 17, 262148]
        for d in at:
            for k in (64, 100):
                # every query at the rank of its own best document (query 0: of all its documents), at document d
                cursors = [(rows[0][4], 0, d) if rows else (BITS["+0"], 0, d) for rows in side.rows]
                check_call(("product edges", d), side, k, cursors, side.call(k, cursors))
        return tile, n
    finally:
        side.release()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def run_refusals():
    """each NS_E_INVAL with its message, nothing launched: the output arrays keep their fill"""
    L = nsbind.hip_lib()
    side = multi_boolean(SHOULD)
    sfam = multi_sorted_family("pool5")
    try:
        fam = side.fam
        ctx, Q = fam.segs.ctx, len(fam.qd)

        def refused_b(after, match):
            rc, hits, nhits, found, rest, _ = nsbind.search_boolean_after_raw(ctx, fam.qd, fam.refs, None, 10, after, fam.order, side.handles)
            assert rc == -1, rc
            assert match in L.ns_last_error(ctx).decode(), L.ns_last_error(ctx).decode()
            assert np.all(hits.view(np.uint8) == 0xAB) and np.all(nhits == 0xABABABAB) and np.all(found == 0xABABABAB) and np.all(rest == 0xABABABAB), "a refused call writes nothing"

        def refused_s(after, match, flags=0):
            rc, hits, keys, nhits, found, rest, _ = nsbind.search_sorted_after_raw(sfam.segs.ctx, sfam.qd, sfam.refs, 10, flags, after, sfam.order,
                                                                                   [sfam.segs.segs[s] for s in sfam.order], [sfam.table(s) for s in sfam.order])
            assert rc == -1, rc
            msg = L.ns_last_error(sfam.segs.ctx).decode()
            assert match in msg, msg
            assert np.all(hits.view(np.uint8) == 0xAB) and np.all(keys == 0xABABABAB) and np.all(nhits == 0xABABABAB) and np.all(found == 0xABABABAB)
            assert np.all(rest == 0xABABABAB), "a refused call writes nothing"

        ok = nsbind.cursors([(0x3F800000, 2, 5)] * Q)
        two = ok.copy()
        two["set"][3] = 2
        refused_b(two, "query 3: cursor with set = 2 (0 or 1)")
        alien = ok.copy()
        alien["seg"][1] = 7
        refused_b(alien, "query 1: cursor names segment 7, which the call does not list")
        unset = alien.copy()
        unset["set"][1] = 0                                                            # an unset cursor's fields are ignored
        assert nsbind.search_boolean_after_raw(ctx, fam.qd, fam.refs, None, 10, unset, fam.order, side.handles)[0] == 0
        reserved = nsbind.cursors([(0xFFFFFFFF, 2, 5)] * Q)
        assert nsbind.search_boolean_after_raw(ctx, fam.qd, fam.refs, None, 10, reserved, fam.order, side.handles)[0] == 0   # NaN bits are a legal score cursor
        Qs = len(sfam.qd)
        oks = nsbind.cursors([(20200101, 0, 5)] * Qs)
        for flags in (0, ASC):
            bad = oks.copy()
            bad["rank"][2] = 0xFFFFFFFF
            refused_s(bad, "query 2: cursor with the reserved key 0xFFFFFFFF", flags)
        two = oks.copy()
        two["set"][0] = 0xFFFFFFFF
        refused_s(two, "query 0: cursor with set = 4294967295 (0 or 1)")
        alien = oks.copy()
        alien["seg"][Qs - 1] = 3
        refused_s(alien, "query %d: cursor names segment 3, which the call does not list" % (Qs - 1))
        # the kernel times sum the paged launches too
        nsbind.boolean_kernel_ms(reset=True)
        nsbind.sorted_kernel_ms(reset=True)
        assert nsbind.search_boolean_after_raw(ctx, fam.qd, fam.refs, None, 10, ok, fam.order, side.handles)[0] == 0
        assert nsbind.search_sorted_after_raw(sfam.segs.ctx, sfam.qd, sfam.refs, 10, 0, oks, sfam.order, [sfam.segs.segs[s] for s in sfam.order],
                                              [sfam.table(s) for s in sfam.order])[0] == 0
        assert all(v > 0.0 for v in nsbind.boolean_kernel_ms(reset=True)) and all(v > 0.0 for v in nsbind.sorted_kernel_ms(reset=True))
    finally:
        sfam.release()
        side.release()


# ---- a child process ----------------------------------------------------------------------------------------------------
def main(out_path):
    """child process at NS_FACET_TILE_DOCS = 128 and NS_BOOL_WIN_DOCS = 32.  The counting build: a batch of unset cursors leaves
    ns_debug_after_counters at 0, then the cursor families reach every one of them.  The variants build: the walks, the
    cursor families and the sub-batches."""
    counting = nsbind.after_counters(reset=True) is not None
    rep = {"tile": nsbind.facet_tile_docs(), "counting": counting}
    assert rep["tile"] == SMALL_TILE, rep
    if counting:
        side = multi_boolean(SHOULD)
        sfam = multi_sorted_family("pool5")
        try:
            for cursors in (None, [None] * len(side.rows)):
                side.call(100, cursors)
                Sorted(sfam, AND).call(100, cursors)
                Sorted(sfam, ASC).call(100, cursors)
            rep["unset"] = nsbind.after_counters(reset=True)
        finally:
            sfam.release()
            side.release()
        run_boolean_cursors()
        rep["boolean"] = nsbind.after_counters(reset=True)
        run_sorted_cursors()
        rep["sorted"] = nsbind.after_counters(reset=True)
        run_boolean_walks(ks=[65])
        print("after", rep["unset"], rep["boolean"], rep["sorted"], flush=True)
    else:
        run_boolean_walks()
        run_tied_walk()
        for pattern in sorted_shapes.PATTERNS:
            run_sorted_walks(pattern)
        run_boolean_cursors()
        run_sorted_cursors()
        rep["sub_batches"] = run_sub_batches()
        run_refusals()
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print("after shapes OK")


if __name__ == "__main__":
    main(sys.argv[1])
