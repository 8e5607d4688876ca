"""Directed inputs for the top-K row join (ns_kernels.hip: k_merge, k_merge_wide, k_merge_ranks).  Plain data and
constructors, no GPU use: tests/test_join_shapes_cpu.py plans every family under the family's own tuning and asserts which
join path each (query, K) takes; tests/test_join_shapes_gpu.py runs them against the numpy restatement and, on the counting
build, asserts that the paths and tie rules named here were reached, the per-path query counts exactly.

The join's paths, by the number of partial rows of a query (part_count, "pc") and K (path_rule restates them; the CPU test
pins the constants to the sources):
  sort64      pc * K <= 64                          one 64-key bitonic sort
  staged      pc <= 64 and pc * K <= kMergeStage    scores in LDS; on equal scores the LOWEST lane wins, which is the canonical
                                                    order only because a query's rows ascend in (segment, doc range)
  tournament  the rest that is not wide             merge_rows_wave, row heads in global memory
  wide        pc > 64 and pc >= K                   threshold from the row heads, gather into LDS, one sort; falls back to the
                                                    tournament when more than kMergeCap candidates tie

A family is a function returning a Family: segments (n_docs, doc_len, lists) with ids 0 .. n-1, queries as lists of
(segment, list) refs, idfs / weights per [segment][list], the ns_set_tuning triple it runs under, its K values, for every K the
path of every query, and the counters (JOIN_EVENTS) its run must move.

How the pc are pinned.  The product library plans with variant 0 only.  With ns_set_tuning(0, 1, S) a group of ONE list of c
postings is cut into ceil(c / 2S) doc ranges, rounded to the nearest power of two in ratio and, at K > 32, to at least 8 when
it is cut at all; a query's pc is the sum over its segments.  With ns_set_tuning(0, 128 * groups, big) every group is cut
into 128 ranges but never into more than the segment has docs: a segment of n <= 128 docs gives pc == n exactly, one doc per row.
Nothing here is trusted: the CPU test plans every family through tests/plan_harness.cpp.

Ties are the point.  In the flat segments every doc has length 100 (avgdl 100 in all of them) and tf 1, so that with one idf
all postings of all lists and segments score alike; a few docs carry tf 2, the second, higher level.  K is smaller than
the tie group, so WHICH of the tied docs leave is the join's decision: (segment asc, doc asc).  No score is -0.0f."""
import numpy as np

WAVE = 64
MERGE_STAGE = 2048     # kMergeStage
MERGE_CAP = 2048       # kMergeCap
MERGE_REG_ROWS = 32    # kMergeRegRows: a k_merge_wide thread keeps this many row heads in registers, 256 threads
MAX_K = 100            # NS_MAX_K
PATHS = ("sort64", "staged", "tournament", "wide")
# test_gpu_parity.py::test_lone_query_wide_merge_ties_and_thresholds: the fewest docs at which its lone one-list query (every
# second doc, default tuning and min_items = 20000) is still cut into enough rows to be wide at K = 1, 10, 64 and 100
LONE_WIDE_N = 100

# name -> index of ns_debug_join_counters (counting build)
JOIN_EVENTS = {"sort64": 0, "staged": 1, "tournament": 2, "wide": 3, "wide_theta0": 4, "wide_second_hist": 5, "wide_overflow": 6,
               "wide_unregistered_rows": 7, "staged_tie_rounds": 8, "tournament_tie_rounds": 9, "wide_threshold_ties": 10,
               "rank_join": 11, "rank_join_tie_rounds": 12, "empty_query": 13}
JOIN_GETTER = "ns_debug_join_counters"


def is_wide(pc, k):
    return pc > WAVE and pc >= k


def path_rule(pc, k):
    """the join path of a query with pc partial rows at this K"""
    if is_wide(pc, k):
        return "wide"
    if pc * k <= WAVE:
        return "sort64"
    if pc <= WAVE and pc * k <= MERGE_STAGE:
        return "staged"
    return "tournament"


class Family:
    def __init__(self, segments, queries, tuning, ks, paths, events, idf=1.75, shared_k=None):
        self.segments, self.queries, self.tuning, self.ks, self.paths = segments, queries, tuning, tuple(ks), paths
        self.events = tuple(dict.fromkeys(list(events) + [p for k in ks for p in paths[k]]))   # every declared path is a counter to move
        self.idfs = [[idf] * len(lists) for _, _, lists in segments]
        self.weights = [[1.0] * len(lists) for _, _, lists in segments]
        self.shared_k = self.ks[0] if shared_k is None else shared_k
        assert set(paths) == set(self.ks) and all(len(p) == len(queries) for p in paths.values())
        assert all(e in JOIN_EVENTS for e in self.events)


FAMILIES = {}


def family(fn):
    FAMILIES[fn.__name__] = fn
    return fn


def _flat(n_docs, lists):
    return n_docs, np.full(n_docs, 100, dtype=np.uint32), lists


def _lst(docs, high=()):
    d = np.unique(np.asarray(docs, dtype=np.int64)).astype(np.uint32)
    return d, np.where(np.isin(d, np.asarray(high, dtype=np.uint32)), 2, 1).astype(np.uint32)


def _per_range(width, counts):
    """docs of a list with counts[r] postings, evenly spaced, in the doc range [r * width, (r + 1) * width)"""
    out = []
    for r, c in enumerate(counts):
        if c:
            out.extend(r * width + (np.arange(c) * (width // c)))
    return np.array(out, dtype=np.int64)


S, G, T, W = "sort64", "staged", "tournament", "wide"


@family
def sort_stage_boundary():
    """pc * K around 64: (K=10, pc=6) and (K=32, pc=2) sort, (K=10, pc=7) stages, (K=1, pc=64) sorts, (K=32, pc=64) is exactly
    kMergeStage entries and stages, (K=100, pc=64) takes the tournament; a query without terms (pc = 0) at every K; the two-list query is cut into 32 rows.  List 0 of
    segment 0 has an empty range and a range of 3 postings between full ones; the high docs sit in its LAST rows and in segment 1."""
    a = _per_range(4096, [200, 0, 3, 250])
    seg0 = _flat(16384, [_lst(a, high=[a[201], a[-1]]), _lst(np.arange(0, 16384, 2), high=[16382, 9000]), _lst(np.arange(0, 16384, 64))])
    seg1 = _flat(4096, [_lst(np.arange(0, 4096, 16), high=[4080]), _lst(np.arange(5, 4096, 41))])
    seg2 = _flat(4096, [_lst(np.arange(3, 4096, 41))])
    queries = [[(0, 0), (1, 0)], [(0, 0), (1, 0), (2, 0)], [(0, 2)], [(0, 1)], [], [(1, 1), (2, 0)], [(0, 0), (0, 2)]]
    paths = {1: [S, S, S, S, S, S, S], 10: [S, G, S, G, S, S, G], 32: [G, G, S, G, S, S, G], 100: [G, G, G, T, S, G, T]}
    return Family([seg0, seg1, seg2], queries, (0, 1, 64), (1, 10, 32, 100), paths,
                  ("sort64", "staged", "tournament", "empty_query", "staged_tie_rounds", "tournament_tie_rounds"), shared_k=10)


@family
def stage_tournament_boundary():
    """pc * K around kMergeStage: (K=64, pc=32) is exactly 2048 entries and stages, (K=64, pc=33), (K=100, pc=21) and
    (K=100, pc=64) take the tournament, (K=100, pc=80) takes it with more than one row per lane, and the same 80 rows are wide
    at K = 64 and 10; the two-list query has 128 rows and is wide at every K.  Ties across rows and across six segments; list 1 of segment 0 has two empty ranges and a range of 5
    postings in the middle."""
    a32 = _per_range(512, [140] * 3 + [0, 0] + [140] * 2 + [5] + [140] * 24)
    seg0 = _flat(16384, [_lst(np.arange(1, 16384, 2), high=[16383, 8191, 1]), _lst(a32, high=[a32[-1], a32[425]]), _lst(np.arange(0, 16384, 8), high=[16376])])
    seg1 = _flat(8192, [_lst(np.arange(0, 8192, 4), high=[8188, 4]), _lst(np.arange(7, 8192, 83))])
    small = [_flat(1024, [_lst(np.arange(i, 1024, 11), high=[i + 11 * 50] if i % 2 else [])]) for i in range(4)]
    queries = [[(0, 1)], [(0, 1), (2, 0)], [(0, 2), (1, 1), (2, 0), (3, 0), (4, 0), (5, 0)], [(0, 0)], [(0, 0), (1, 0)], [], [(0, 0), (0, 2)]]
    paths = {10: [G, G, G, G, W, S, W], 64: [G, T, G, T, W, S, W], 100: [T, T, T, T, T, S, W]}
    return Family([seg0, seg1] + small, queries, (0, 1, 64), (10, 64, 100), paths,
                  ("staged", "tournament", "wide", "staged_tie_rounds", "tournament_tie_rounds", "empty_query"), shared_k=64)


@family
def wide_levels():
    """k_merge_wide over rows longer than one entry: two levels with the tie group AT the threshold (128 rows of 12: 1536
    candidates), every score equal with 4096 candidates (overflow: tournament fall-back), distinct scores (segment 1: random
    lengths and tfs), and two segments whose tied candidates number exactly kMergeCap (1536 + 512: no overflow)."""
    rng = np.random.default_rng(11)
    x = _per_range(32, [12] * 128)
    seg0 = _flat(4096, [_lst(x, high=[x[5], x[700], x[-1]]), _lst(np.arange(4096))])
    zd = np.sort(rng.choice(4096, size=2048, replace=False))
    seg1 = (4096, rng.integers(20, 5000, size=4096, dtype=np.uint32), [(zd.astype(np.uint32), rng.integers(1, 9, size=2048, dtype=np.uint32))])
    x2 = _per_range(128, [16] * 32)
    seg2 = _flat(4096, [_lst(x2, high=[x2[-1]])])
    queries = [[(0, 0)], [(0, 1)], [(1, 0)], [(0, 0), (2, 0)], [(2, 0)], [(0, 0), (0, 1)]]
    paths = {1: [W, W, W, W, S, W], 10: [W, W, W, W, G, W], 64: [W, W, W, W, G, W], 100: [W, W, W, W, T, W]}
    return Family([seg0, seg1, seg2], queries, (0, 1, 8), (1, 10, 64, 100), paths,
                  ("wide", "wide_second_hist", "wide_overflow", "wide_threshold_ties", "tournament_tie_rounds", "staged", "tournament"), shared_k=10)


@family
def wide_tiny_segments():
    """Segments of at most 128 docs, every group cut into one row per doc: pc == n_docs exactly.  Lists whose postings lie in
    fewer than K of 128 ranges (theta = 0), in exactly K of them for K = 1, 10, 64, 100, pc == K == 100, pc = 96 (wide up to
    K = 64, the tournament with two rows per lane at K = 100; a segment is cut into as many rows as it has docs only from 91
    docs on: below that the nearest power of two is 64), two segments joined (228 rows), a narrow query of 3 rows."""
    a = [_lst(np.arange(128), high=[127, 40]), _lst([3, 50, 51, 90, 127]), _lst([77]), _lst(np.arange(6, 126, 12)),
         _lst(np.arange(0, 128, 2), high=[126]), _lst(np.arange(28, 128), high=[127])]
    segs = [_flat(128, a), _flat(100, [_lst(np.arange(100), high=[99, 0])]), _flat(3, [_lst(np.arange(3))]), _flat(96, [_lst(np.arange(96), high=[95])])]
    queries = [[(0, 0)], [(0, 1)], [(0, 2)], [(0, 3)], [(0, 4)], [(0, 5)], [(1, 0)], [(0, 0), (1, 0)], [(2, 0)], [(3, 0)], [], [(0, 0), (0, 4)]]
    groups = sum(len({s for s, _ in q}) for q in queries)
    wides = [W] * 8
    paths = {1: wides + [S, W, S, W], 10: wides + [S, W, S, W], 64: wides + [G, W, S, W], 100: wides + [G, T, S, W]}
    return Family(segs, queries, (0, 128 * groups, 1 << 30), (1, 10, 64, 100), paths,
                  ("wide", "wide_theta0", "wide_second_hist", "wide_threshold_ties", "tournament", "tournament_tie_rounds", "empty_query"), shared_k=10)


@family
def wide_unregistered_rows():
    """Three segments of 8192 docs, each cut into 4096 ranges: 12288 rows, more than the 256 * kMergeRegRows = 8192 whose heads
    k_merge_wide keeps in registers.  Distinct scores (random lengths and tfs), so the best docs lie in all three segments,
    those of the third in re-read rows; one segment alone (4096 rows) and a narrow query run in the same batch."""
    rng = np.random.default_rng(12)
    segs = []
    for _ in range(3):
        few = np.sort(rng.choice(8192, size=8, replace=False)).astype(np.uint32)
        segs.append((8192, rng.integers(20, 5000, size=8192, dtype=np.uint32),
                     [(np.arange(8192, dtype=np.uint32), rng.integers(1, 9, size=8192, dtype=np.uint32)), (few, rng.integers(1, 9, size=8, dtype=np.uint32))]))
    queries = [[(0, 0), (1, 0), (2, 0)], [(0, 1)], [(1, 0)], [(2, 1), (2, 0)]]
    paths = {10: [W, S, W, W], 100: [W, G, W, W]}
    return Family(segs, queries, (0, 1, 1), (10, 100), paths, ("wide", "wide_unregistered_rows", "wide_second_hist", "sort64", "staged"), shared_k=10)


# ---- synthetic rows for k_merge_ranks (ns_merge_rank_rows): no index -----------------------------------------------------
RANK_COUNTS = (1, 2, 3, 63, 64)
RANK_KS = (1, 10, 100)
RANK_QUERIES = 7          # not a multiple of the 4 queries of a workgroup
RANK_LOCAL_SEGS = 2


def rank_rows(n_ranks, k, seed=0, with_seg_map=True):
    """-> (g_hits [W, Q, K, 3] int32 (score bits, local seg, doc), g_nhits [W, Q] int32, g_found [W, Q] int64, seg_map
    [W, RANK_LOCAL_SEGS] int32 or None).  Every row is sorted the canonical way, (global seg, doc) pairs are unique across
    ranks, scores come from four levels (heavy ties across ranks), and seg_map REVERSES the rank order: rank 0 holds the
    highest global ids, so that neither the lane number nor the local id breaks a tie correctly.  Without a seg_map the local
    ids are global already, and rank r's docs are r mod 64 apart so that pairs stay unique.
    Query 0: every rank empty.  Query 1: rank 0 (and every third) empty.  Query 2: rows reporting nhits = K + 7 (must be
    clamped to K) in every rank but the last; the rows of query 3 right behind them hold valid-looking, higher scores.
    Query 4: short rows.  `found` per row is near 2^32, so that sums pass it from two ranks on."""
    rng = np.random.default_rng(1000 * n_ranks + k + seed)
    Q, LS = RANK_QUERIES, RANK_LOCAL_SEGS
    levels = np.array([1.5, 1.25, 1.0, 0.75], dtype=np.float32)
    hits = np.zeros((n_ranks, Q, k, 3), dtype=np.int32)
    hits[..., 0] = np.array([-np.inf], dtype=np.float32).view(np.int32)[0]
    hits[..., 1:] = -1
    nhits = np.zeros((n_ranks, Q), dtype=np.int32)
    found = np.zeros((n_ranks, Q), dtype=np.int64)
    seg_map = np.array([[(n_ranks - 1 - r) * LS + s for s in range(LS)] for r in range(n_ranks)], dtype=np.int32) if with_seg_map else None
    for r in range(n_ranks):
        for q in range(Q):
            found[r, q] = (1 << 32) - 5 + r + q
            if q == 0 or (q == 1 and r % 3 == 0):
                found[r, q] = 0
                continue
            n = k if q in (2, 3) else int(rng.integers(1, k + 1)) if q != 4 else min(k, 1 + r % 3)
            seg = np.sort(rng.integers(0, LS, size=n))
            doc = rng.choice(4 * k + 8, size=n, replace=False) * (1 if with_seg_map else 64) + (0 if with_seg_map else r)
            score = levels[rng.integers(0, len(levels), size=n)] + (np.float32(2.0) if q == 3 else np.float32(0.0))
            order = np.lexsort((doc, seg, -score))
            hits[r, q, :n, 0] = score[order].view(np.int32)
            hits[r, q, :n, 1] = seg[order]
            hits[r, q, :n, 2] = doc[order]
            nhits[r, q] = n + 7 if (q == 2 and r != n_ranks - 1) else n
    return hits, nhits, found, seg_map


def brute_join(g_hits, g_nhits, g_found, seg_map, k):
    """the rank join by one lexsort over all entries (not the heap of join_ref.np_join): same output format"""
    n_ranks, Q = g_nhits.shape
    out = []
    for q in range(Q):
        rows = [g_hits[r, q, :min(int(g_nhits[r, q]), k)] for r in range(n_ranks)]
        gseg = [row[:, 1] if seg_map is None else seg_map[r][row[:, 1]] for r, row in enumerate(rows)]
        allr, gs = np.concatenate(rows), np.concatenate(gseg).astype(np.int64)
        score = np.ascontiguousarray(allr[:, 0]).view(np.float32)
        order = np.lexsort((allr[:, 2].astype(np.int64), gs, -score.astype(np.float64)))[:k]
        out.append(([(int(allr[i, 0]) & 0xFFFFFFFF, int(gs[i]), int(allr[i, 2])) for i in order], sum(int(x) for x in g_found[:, q])))
    return out
