"""Directed inputs of ns_search_boolean (csrc/ns_boolean.hip) and the code that runs them through the raw C-ABI
against the restatement (tests/boolean_ref.py).  All comparisons are exact, score bits included.

Imported by tests/test_boolean_gpu.py for the product library (tile of 2^17 documents, windows of kBqWinDocs), and run as a
program in a child process that loaded the variants or the counting build with NS_FACET_TILE_DOCS=128 NS_BOOL_WIN_DOCS=32:
there the 300 documents of the small families span two whole tiles and a part, four windows each, and the counting build
reports which paths of the two kernels the inputs reached."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "nextsearch-api_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import boolean_ref  # noqa: E402
import facet_shapes  # noqa: E402
import filter_ref  # noqa: E402
import nsbind  # noqa: E402
from boolean_ref import MUST, NOT, SHOULD  # noqa: E402
from rawseg import RawSegments, descriptors_multi  # noqa: E402

AND = nsbind.NS_FLAG_AND
SMALL_TILE, SMALL_WIN, N_DOCS = facet_shapes.SMALL_TILE, 32, facet_shapes.N_DOCS
KS = [1, 10, 63, 64, 65, 100]                 # 64 / 65: the boundary between the kept set's two registers
# name -> index of ns_debug_boolean_counters (counting build)
BOOLEAN_EVENTS = {"items": 0, "windows": 1, "windows_left_early": 2, "must_intersections": 3, "exclusions_that_cleared": 4, "chunks_skipped": 5,
                  "chunks_inserted": 6, "rows_joined": 7}
S, M, X = SHOULD, MUST, NOT

# Over facet_shapes.small_lists(): 0 empty, 1 {0}, 2 .. 6 of 63, 64, 65, 128 and 257 postings (6 with a posting >= n_docs), 7 in
# the middle small tile alone, 8 outside it.  (list, role) per ref.
DIRECTED = [
    [],
    [(6, S)], [(6, M)], [(6, X)],                                       # one ref of every role; NOT alone matches nothing
    [(1, S)], [(0, S)], [(0, M)], [(0, X)],
    [(2, S), (3, S)], [(2, M), (3, M)], [(2, M), (3, S)], [(2, S), (3, X)], [(2, M), (3, X)], [(3, S), (2, M)],
    [(7, M), (8, M)],                                                   # MUST ∩ = ∅: every window ends on an empty cut or an empty AND
    [(7, S), (8, S)], [(7, S), (8, X)], [(7, M), (8, S)],               # a SHOULD list that never meets the MUST list
    [(5, S), (5, X)], [(5, M), (5, X)],                                 # everything excluded: once SHOULD and once NOT; NOT == MUST
    [(4, S), (4, S)], [(4, M), (4, M)], [(4, M), (4, S)],               # a list named twice adds twice, matches once
    [(0, M), (5, S)], [(5, S), (0, M)],                                 # a MUST ref with count == 0 kills the group
    [(0, S), (5, S)], [(5, S), (0, X)], [(0, S), (5, X)],               # empty SHOULD / NOT refs are dropped
    [(5, X), (6, X)],
    [(6, S), (2, X), (3, X), (4, X)], [(6, M), (5, M), (4, X)], [(6, M), (5, M), (2, M), (3, S)],
    [(li, S) for li in range(1, 9)], [(li, M if li in (5, 6) else S) for li in range(1, 9)], [(li, X if li in (7, 2) else S) for li in range(1, 9)],
    [(li, (M, S, X, S, S, S, M, S)[li - 1]) for li in range(1, 9)],
    [(2 + i % 7, S) for i in range(70)], [(2 + i % 7, M if i % 7 == 4 else S) for i in range(70)], [(2 + i % 7, X if i % 7 in (5, 0) else S) for i in range(70)],
    [(2 + i % 7, (M if i % 7 == 4 else X if i % 7 == 5 else S)) for i in range(70)],
    [(6, M)] * 70,
]


def small_weights(n_lists):
    """distinct idfs and weights per list, so that a wrong list or a wrong order shows in the score bits; one negative weight"""
    return [1.0 + 0.37 * i for i in range(n_lists)], [1.0 if i % 2 == 0 else 0.6 + 0.05 * i for i in range(n_lists - 1)] + [-0.25]


class Family:
    """uploaded segments + one call's descriptors and roles; the restatement's answer is computed once and kept"""

    def __init__(self, segments, queries, idfs, weights, seg_order=None):
        self.segments, self.queries, self.idfs, self.weights = segments, queries, idfs, weights
        self.order = list(range(len(segments))) if seg_order is None else list(seg_order)
        self.segs = RawSegments(segments)
        self.cache = {}
        self.qd, self.refs = descriptors_multi([[(s, li) for s, li, _ in q] for q in queries], self.segs.lists, self.segs.offs, idfs, weights)
        self.roles = np.array([r for q in queries for _, _, r in q], dtype=np.uint8)

    def ref(self, k):
        return boolean_ref.boolean_hits(self.segments, self.queries, k, self.order, self.idfs, self.weights, self.cache)

    def call(self, k, roles="own"):
        rc, hits, nhits, found, _ = nsbind.search_boolean_raw(self.segs.ctx, self.qd, self.refs, self.roles if isinstance(roles, str) else roles, k, self.order,
                                                              [self.segs.segs[s] for s in self.order])
        return rc, hits, nhits, found

    def check(self, k, label):
        rc, hits, nhits, found = self.call(k)
        assert rc == 0, (label, self.segs.err())
        ref = self.ref(k)
        boolean_ref.check(ref, hits, nhits, found, k, label=label)
        return ref, hits, nhits, found

    def release(self):
        self.segs.release()


def directed_family(n_segs):
    """one or three segments of 300 documents over the small lists (different document lengths per segment); with three, the
    refs of a query interleave the segments, the call lists them as 2, 0, 1, and in segment 1 list 5 stands in for the empty
    list 0 as the MUST ref of the two-ref `count == 0` queries, so that the group dies in the other two segments alone"""
    lists = facet_shapes.small_lists()
    segments = [(N_DOCS, (5 + (np.arange(N_DOCS) * (1 + 2 * s)) % 41).astype(np.uint32), lists) for s in range(n_segs)]
    queries = []
    for q in DIRECTED:
        refs = []
        for li, role in q:
            for s in range(n_segs):
                refs.append((s, 5 if (s == 1 and li == 0 and role == M and len(q) > 1) else li, role))
        queries.append(refs)
    idf, w = small_weights(len(lists))
    return Family(segments, queries, [idf] * n_segs, [w] * n_segs, seg_order=[2, 0, 1] if n_segs == 3 else None)


def run_directed(n_segs, tile_expected=None):
    """every role mix of DIRECTED at K = 1 .. 100, without and with skip tables; roles == NULL is the all-SHOULD call"""
    tile = nsbind.facet_tile_docs()
    if tile_expected is not None:
        assert tile == tile_expected, (tile, tile_expected)
    fam = directed_family(n_segs)
    try:
        assert sorted({int(c) // n_segs for c in fam.qd["term_count"]}) == [0, 1, 2, 3, 4, 8, 70]
        for with_skips in (False, True):
            if with_skips:
                for s in range(n_segs):
                    assert facet_shapes.build_skips(fam.segs, s) == 4
            for k in KS:
                ref = fam.check(k, ("directed", n_segs, "skips", with_skips))[0]
        founds = [f for f, _ in ref]
        assert 0 in founds and max(founds) > 100 and len({f for f in founds}) > 10
        for qi in (3, 5, 6, 7, 14, 18, 19, 28):                                # NOT alone, empty lists, MUST ∩ = ∅, everything excluded
            assert founds[qi] == 0, (qi, founds[qi])
        assert founds[23] == (0 if n_segs == 1 else 128)                        # the dead group: in segment 1 list 5 stands in for the empty one
        # roles == NULL: every ref SHOULD
        plain = Family(fam.segments, [[(s, li, S) for s, li, _ in q] for q in fam.queries], fam.idfs, fam.weights, fam.order)
        try:
            for k in (10, 100):
                rc, hits, nhits, found = plain.call(k, roles=None)
                assert rc == 0, plain.segs.err()
                boolean_ref.check(plain.ref(k), hits, nhits, found, k, label=("roles NULL", n_segs))
        finally:
            plain.release()
    finally:
        fam.release()
    return tile


def tied_family():
    """equal tf and equal document length: every document of a list scores the same bits, in every segment.  List 0 holds
    every document, 1 every third, 2 the documents 100 .. 199, 3 a few around the edges.  Ties straddle the 32-document
    windows, the 128-document tiles and the segment boundaries; K = 1 .. 100 cuts through the tie groups."""
    d = np.arange(N_DOCS, dtype=np.uint32)
    docs = [d, d[d % 3 == 0], d[(d >= 100) & (d < 200)], np.array([0, 31, 32, 127, 128, 255, 256, 299], np.uint32)]
    lists = [(x, np.full(len(x), 2, np.uint32)) for x in docs]
    segments = [(N_DOCS, np.full(N_DOCS, 9, np.uint32), lists) for _ in range(3)]
    one = [(0, S)], [(0, M), (1, S)], [(0, S), (1, S), (2, S)], [(0, M), (2, X)], [(1, M), (2, M)], [(0, M), (3, S), (1, X)], [(3, S)], [(2, S), (3, S)], \
          [(0, S), (0, S), (1, X), (2, X)]
    queries = [[(s, li, r) for li, r in q for s in (1, 2, 0)] for q in one] + [[(0, li, r) for li, r in q] for q in one[:4]] + [[(2, 0, M), (1, 0, S), (1, 3, X)]]
    idf, w = [1.5, 0.75, 2.0, 1.25], [1.0, 1.0, 0.5, 1.0]
    return Family(segments, queries, [idf] * 3, [w] * 3, seg_order=[1, 2, 0])


def run_tied():
    fam = tied_family()
    try:
        for with_skips in (False, True):
            if with_skips:
                for s in range(3):
                    facet_shapes.build_skips(fam.segs, s)
            for k in KS:
                ref = fam.check(k, ("tied", "skips", with_skips))[0]
        # the precondition: K = 100 ends inside a tie group for most queries, and ties cross segments
        cut = 0
        for (found, hits), rows in zip(ref, fam.cache["all"]):
            cut += int(found > 100 and np.float32(rows[99][0]).view(np.uint32) == np.float32(rows[100][0]).view(np.uint32))
        assert cut >= 8, cut
        assert len({s for _, s, _ in ref[0][1]}) == 1 and ref[0][0] == 900     # 100 equal scores: all from the segment listed first
    finally:
        fam.release()


def run_product_tile():
    """the product build's tile and window: n_docs = two tiles + 5; lists of equal tf over documents of equal length whose ties
    straddle a window edge (2^13 at the product value), both tile edges and the end; K cuts through the tie groups"""
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
    one = [[(0, S)], [(1, S)], [(0, S), (1, S)], [(0, M), (1, S)], [(0, M), (4, X)], [(0, M), (4, M)], [(1, M), (2, M)], [(0, S), (1, S), (2, S), (3, X)],
           [(3, M), (0, M), (1, S)], [(2, S), (2, S)], [(3, X)], [(4, S), (0, X)], [(1, M), (1, X)], [(0, M), (0, S), (4, S), (3, X)]]
    queries = [[(0, li, r) for li, r in q] for q in one]
    idf, w = small_weights(len(lists))
    fam = Family(segments, queries, [idf], [w])
    try:
        for with_skips in (False, True):
            if with_skips:
                assert facet_shapes.build_skips(fam.segs, 0) == 4
            for k in (1, 64, 65, 100):
                ref = fam.check(k, ("product tile", tile, with_skips))[0]
        assert ref[0][0] == len(docs[0]) and ref[10][0] == 0 and ref[12][0] == 0 and ref[4][0] == len(docs[0]) - 80
        rows = fam.cache["all"][0]                                              # one tie group across a window edge, a tile edge and the end
        assert len({np.float32(v).view(np.uint32).item() for v, _, _ in rows}) == 1 and rows[0][2] == win - 40 and rows[99][2] == tile - 100 + 19
    finally:
        fam.release()
    return tile, n


# ---- equivalence with the scoring path, same raw inputs -----------------------------------------------------------------
def equal_rows(label, got, want, k, ids=None):
    """(hits, nhits, found) of the boolean call against those of the scoring path; returns the queries with found >= 2"""
    hits, nhits, found = got
    w_hits, w_nhits, w_found = want
    np.testing.assert_array_equal(found, w_found.astype(np.uint64), err_msg=str(label))
    np.testing.assert_array_equal(nhits, w_nhits, err_msg=str(label))
    for q in range(len(found)):
        n = int(nhits[q])
        np.testing.assert_array_equal(hits[q, :n]["score"].view(np.uint32), w_hits[q, :n]["score"].view(np.uint32), err_msg=str((label, q)))
        np.testing.assert_array_equal(hits[q, :n]["doc"], w_hits[q, :n]["doc"], err_msg=str((label, q)))
        want_seg = w_hits[q, :n]["seg"] if ids is None else np.array([ids[int(x)] for x in w_hits[q, :n]["seg"]], np.uint32)
        np.testing.assert_array_equal(hits[q, :n]["seg"], want_seg, err_msg=str((label, q)))
        tail = hits[q, n:]
        assert np.all(tail["score"].view(np.uint32) == boolean_ref.PAD_SCORE_BITS) and np.all(tail["seg"] == boolean_ref.PAD_ID) and np.all(tail["doc"] == boolean_ref.PAD_ID)
    return int(np.sum(found >= 2))


def multi_family():
    """facet_shapes' three segments (300, 77, 1000 documents; every list non-empty, every docId in range) and queries, two of
    which leave a segment without a match"""
    segments, queries = facet_shapes.multi_family()
    return segments, queries + [[(0, 2), (2, 3)], [(1, 1), (1, 1), (0, 0)]]


def multi_weights(segments):
    return [[1.0 + 0.5 * i for i in range(len(s[2]))] for s in segments], [[1.0 if i % 2 else 0.75 for i in range(len(s[2]))] for s in segments]


FLOOR_SAME_ROLE = {S: 8, M: 4}        # queries with found >= 2 that the two equivalence checks must cover (test_boolean_cpu counts them)
FLOOR_EXCLUDED = 5


def same_role_inputs(role):
    segments, queries = multi_family()
    return (segments, [[(s, li, role) for s, li in q] for q in queries]) + multi_weights(segments)


def excluding_inputs():
    segments, _ = multi_family()
    return (segments, [[(s, li, role) for li in pos] + [(s, li, X) for li in neg] for s, pos, role, neg in EXCLUDING]) + multi_weights(segments)


def run_same_role_equals_the_scoring_path():
    """all SHOULD == ns_search_batch under NS_FLAG_OR, all MUST (non-empty lists) == under NS_FLAG_AND"""
    covered = {}
    for role, flags in ((S, 0), (M, AND)):
        fam = Family(*same_role_inputs(role))
        try:
            for with_skips in (False, True):
                if with_skips:
                    for s in range(3):
                        facet_shapes.build_skips(fam.segs, s)
                for k in (7, 64, 100):
                    rc, w_hits, w_nhits, w_found = nsbind.search_batch_raw(fam.segs.ctx, fam.qd, fam.refs, k, flags)
                    assert rc == 0, fam.segs.err()
                    rc, hits, nhits, found = fam.call(k)
                    assert rc == 0, fam.segs.err()
                    covered[role] = equal_rows(("role", role, k, with_skips), (hits, nhits, found), (w_hits, w_nhits, w_found), k)
                    assert covered[role] >= FLOOR_SAME_ROLE[role], covered
        finally:
            fam.release()
    return covered


EXCLUDING = [   # (positive refs, their role, excluded lists) per query, all in ONE segment so that one filtered copy answers it
    (0, [0, 1], S, [2]), (0, [0, 1, 3], S, [2]), (0, [0, 3], M, [1]), (0, [3], S, [0, 1]), (2, [0, 1, 2], S, [3]), (2, [0, 2], M, [1]),
    (2, [2, 2], S, [0]), (1, [1], S, [0, 2]), (1, [0, 1], M, [2]), (2, [1], S, [1]),
]


def run_excluded_equals_the_search_over_filtered_copies():
    """with NOT refs: the search (OR for SHOULD refs, AND for MUST refs) over an ns_segment_filter copy of the segment whose
    keep-bitmap is the complement of the excluded lists' union"""
    segments, queries, idfs, weights = excluding_inputs()
    fam = Family(segments, queries, idfs, weights)
    copies, covered = [], 0
    try:
        ctx = fam.segs.ctx
        for k in (5, 100):
            rc, hits, nhits, found = fam.call(k)
            assert rc == 0, fam.segs.err()
            for qi, (s, pos, role, neg) in enumerate(EXCLUDING):
                n_docs, _, lists = segments[s]
                keep = np.ones(n_docs, bool)
                for li in neg:
                    keep[lists[li][0]] = False
                counts = np.array([len(d) for d, _ in lists], dtype=np.uint32)
                new_id = 3 + len(copies)
                h, noff, ncnt, _, _, _ = nsbind.segment_filter(ctx, fam.segs.segs[s], new_id, filter_ref.bits_of(keep), fam.segs.offs[s], counts)
                copies.append(h)
                qd = np.array([(0, len(pos))], dtype=nsbind.QDESC_DTYPE)
                refs = np.array([(new_id, int(ncnt[li]), int(noff[li]), idfs[s][li], weights[s][li]) for li in pos], dtype=nsbind.TERM_DTYPE)
                if role == M and any(int(ncnt[li]) == 0 for li in pos):
                    w = (np.zeros((1, k), nsbind.HIT_DTYPE), np.zeros(1, np.uint32), np.zeros(1, np.uint64))       # a required list lost every posting
                else:
                    rc, *w = nsbind.search_batch_raw(ctx, qd, refs, k, AND if role == M else 0)
                    assert rc == 0, fam.segs.err()
                covered += equal_rows(("excluded", qi, k), (hits[qi:qi + 1], nhits[qi:qi + 1], found[qi:qi + 1]), tuple(w), k, ids={new_id: s})
        assert covered >= 2 * FLOOR_EXCLUDED, covered
    finally:
        for h in copies:
            fam.segs.L.ns_segment_release(fam.segs.ctx, h)
        fam.release()
    return covered


COUNT_SIZES = [63, 64, 65, 66, 99, 100, 101]


def counts_family():
    """found == K - 1, K, K + 1 and 0 around K = 64, 65 and 100 through every role: list i has SIZES[i] postings inside one base
    list of 200; MUST base + MUST list, SHOULD list alone, and base minus a list of 200 - m"""
    rng = np.random.default_rng(3)
    base = np.sort(rng.choice(N_DOCS, 200, replace=False)).astype(np.uint32)
    sizes = COUNT_SIZES
    lists = [(base, (1 + base % 5).astype(np.uint32))]
    for m in sizes:
        d = np.sort(rng.choice(base, m, replace=False)).astype(np.uint32)
        lists.append((d, (1 + d % 4).astype(np.uint32)))
        rest = np.setdiff1d(base, d).astype(np.uint32)
        lists.append((rest, np.ones(len(rest), np.uint32)))
    lists.append((np.zeros(0, np.uint32), np.zeros(0, np.uint32)))
    segments = [(N_DOCS, rng.integers(5, 60, N_DOCS).astype(np.uint32), lists)]
    queries = []
    for i in range(len(sizes)):
        queries += [[(0, 1 + 2 * i, S)], [(0, 0, M), (0, 1 + 2 * i, M)], [(0, 0, S), (0, 2 + 2 * i, X)], [(0, 0, M), (0, 2 + 2 * i, X), (0, 1 + 2 * i, S)]]
    queries.append([(0, len(lists) - 1, S)])
    idf, w = small_weights(len(lists))
    return Family(segments, queries, [idf], [w]), sizes


def run_counts():
    fam, sizes = counts_family()
    try:
        for k in (64, 65, 100):
            ref = fam.check(k, "counts")[0]
            got = {f - k for f, _ in ref}
            assert {-1, 0, 1} <= got and 0 in {f for f, _ in ref}, (k, got)
            for i, m in enumerate(sizes):
                assert [f for f, _ in ref[4 * i:4 * i + 4]] == [m] * 4
    finally:
        fam.release()


def main(out_path):
    """child process: the directed and the tied families at NS_FACET_TILE_DOCS = 128 and NS_BOOL_WIN_DOCS = 32; with the
    counting build, the counters of those families"""
    counting = "ns_debug_boolean_counters" in nsbind.debug_counters(reset=True)
    rep = {"tile": run_directed(1, tile_expected=SMALL_TILE), "counting": counting}
    run_directed(3)
    run_tied()
    if counting:
        c = nsbind.debug_counters(reset=True)["ns_debug_boolean_counters"]
        rep["events"] = {e: c[i] for e, i in BOOLEAN_EVENTS.items()}
        rep["missed"] = [e for e in BOOLEAN_EVENTS if rep["events"][e] == 0]
        print("boolean", rep["events"], flush=True)
    run_counts()
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print("boolean shapes OK")


if __name__ == "__main__":
    main(sys.argv[1])
