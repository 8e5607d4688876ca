"""Directed inputs for the rare paths of the wave scoring bodies (ns_driver_kernel.hip, ns_merge_kernel.hip,
ns_tile_kernel.hip, WaveTopK).  Plain data and constructors, no GPU use: tests/test_body_shapes_cpu.py plans every family
and asserts which body each query takes; tests/test_body_shapes_gpu.py scores them against the numpy restatement and, on
the counting build, asserts that the paths named here were reached.

A family is a function returning (n_docs, doc_len, lists, queries, idfs, weights): lists of (docIds, tfs), queries as lists
of list numbers, one idf and one weight per list.  `@family(...)` attaches what the tests need to know about it:
  bodies   the body every query's group must take: "thin" | "general" | "merge" | "tile" (a list, or a function of the family)
  events   counters of the counting build that must be above zero after the family ran (see EVENTS)
  split    {class: split value} for the variant whose doc-range cut must fall inside `run` (first, last docId of a run)
  merge    False: the family is planned and run with the merge body off

The sizes follow from the constants of the bodies that k_uscore<512, 192, ...> instantiates (read from the sources by
test_body_shapes_cpu.py::test_constants_match_the_kernels, not guessed):
  NB = HK / 2 = 256 buckets of 4 entries in both driver-stream classes, FB = 64 foreign postings per super-batch in the
  thin class (one 64-lane chunk), FB = 192 in the general class (three chunks), a driver / merge round of 256 postings,
  doc tiles and skip-grid cells of kSkipDocs = 1024 docs, NS_MAX_K = 100, candidate buffer of 128 entries up to K = 32
  (ns_batch_run: `K <= 32`; the comment above it still speaks of 64, so K_SET holds both pairs) and of 256 above.

How a driver-stream family pins its super-batch: a wave plans windows over the foreign lists, at most FB postings less one
per active foreign term in total.  When ALL foreign postings of the item fit (sum <= FB - foreign terms), every window is
its whole list, nothing is probed, and the item is ONE super-batch [doc_lo, doc_hi - 1].  With n_docs = 2^17 the bucket
multiplier is exactly 2^24 / 2^17 = 128, so bucket(doc) = doc >> 9: 512 docs per bucket, docs 130560 .. 131071 in the last one.
Postings are laid out flat in query-term order, so a list's first posting sits at the sum of the windows in front of it.

The planner's classes, restated (plan_rule; ns_plan.hpp): thin when the other lists hold <= 1/32 of the largest, else
doc tiles when the group has >= 0.25 postings per doc, else general; a general group of two lists takes the merge body
when the shorter holds >= 1/8 of the longer."""
import numpy as np

NB = 256
FB = {"thin": 64, "general": 192}
ROUND = 256
SKIP_DOCS = 1024
MAX_K = 100
CB_SWITCH_K = 32
K_SET = (1, 32, 33, 63, 64, 65, 100, MAX_K)

# name -> (getter of the counting build, index)
EVENTS = {
    "full_lanes": ("ns_debug_counters", 20), "carry_chunks": ("ns_debug_counters", 21), "next_moves": ("ns_debug_counters", 22),
    "wrap_moves": ("ns_debug_counters", 23), "owner_found": ("ns_debug_counters", 24), "no_primary": ("ns_debug_counters", 25),
    "many_terms": ("ns_debug_counters", 26), "span_clamps": ("ns_debug_counters", 27), "pass_a_placed": ("ns_debug_counters", 15),
    "claim_iterations": ("ns_debug_counters", 6), "driver_items": ("ns_debug_counters", 0), "super_batches": ("ns_debug_counters", 1),
    "table_hits": ("ns_debug_counters", 14),
    "merge_items": ("ns_debug_merge_counters", 0), "merge_steps": ("ns_debug_merge_counters", 1), "hi_from_a": ("ns_debug_merge_counters", 2),
    "hi_from_b": ("ns_debug_merge_counters", 3), "hi_from_end": ("ns_debug_merge_counters", 4), "a_exhausted": ("ns_debug_merge_counters", 5),
    "b_exhausted": ("ns_debug_merge_counters", 6), "b_window_1": ("ns_debug_merge_counters", 7), "b_window_2": ("ns_debug_merge_counters", 8),
    "b_window_3": ("ns_debug_merge_counters", 9), "b_window_4": ("ns_debug_merge_counters", 10), "merge_matches": ("ns_debug_merge_counters", 11),
    "tile_items": ("ns_debug_tile_counters", 0),
    "shrinks_between": ("ns_debug_topk_counters", 0), "shrinks_in_step": ("ns_debug_topk_counters", 1),
}

FAMILIES = {}


def family(bodies, events=(), split=None, run=None, merge=True, ks=False):
    def deco(fn):
        fn.bodies, fn.events, fn.split, fn.run, fn.merge, fn.ks = bodies, tuple(events), split, run, merge, ks
        FAMILIES[fn.__name__] = fn
        return fn
    return deco


def plan_rule(counts, n_docs, merge=True):
    """the planner's class of a group with these list sizes, restated with the thresholds this file was written against"""
    cost, cmax = sum(counts), max(counts)
    rest = cost - cmax
    if rest * 32 <= cmax:
        return "thin"
    if len(counts) >= 2 and cost * 64 >= n_docs * 16:
        return "tile"
    if merge and len(counts) == 2 and rest * 8 >= cmax:
        return "merge"
    return "general"


def bodies_by_rule(merge=True):
    def f(n_docs, lists, queries):
        return [plan_rule([len(lists[li][0]) for li in q], n_docs, merge) for q in queries]
    return f


def _doc_len(rng, n):
    return rng.integers(20, 3000, size=n, dtype=np.uint32)


def _tfs(rng, n):
    return rng.integers(1, 9, size=n, dtype=np.uint32)


def _lst(rng, docs):
    d = np.unique(np.asarray(docs, dtype=np.int64)).astype(np.uint32)
    return d, _tfs(rng, len(d))


def _spaced(rng, n, lo, hi, avoid=()):
    """n docs spread evenly over [lo, hi), one per stride with a small jitter, none of them in a bucket (doc >> 9) of `avoid`"""
    stride = (hi - lo) // n
    assert stride >= 2
    d = lo + np.arange(n) * stride + rng.integers(0, max(stride // 2, 1), size=n)
    bad = {int(a) >> 9 for a in avoid}
    for i in range(n):
        while (int(d[i]) >> 9) in bad:
            d[i] += 512
    d = np.unique(d)
    assert len(d) == n and d[-1] < hi + 1024
    return d


def _pad(rng, docs, total, limit):
    """`docs` plus random docs below `limit` up to `total` distinct ones"""
    have = {int(x) for x in docs}
    assert len(have) <= total
    while len(have) < total:
        have.add(int(rng.integers(0, limit)))
    return sorted(have)


N17 = 1 << 17
IDF5 = [1.5, 3.25, 6.0, 2.125, 9.5]
W5 = [1.0, 0.5, 1.0, 0.75, 1.0]
ORDERS5 = [[0, 1, 2, 3, 4], [1, 2, 0, 3, 4], [1, 2, 3, 4, 0], [2, 0, 1, 3, 4]]   # driver first, middle, last; primary not the first foreign


def _driver_window_family(seed, cls, run_start, bucket0_full=False, second_run=None):
    """Lists 0 driver D, 1 primary foreign P (the largest window), 2 / 3 foreign S2 / S3 sharing docs of the run, 4 a foreign
    list of one posting at doc n_docs - 1.  All foreign postings fit one super-batch: thin 40 + 10 + 6 + 1 = 57 <= 64 - 4,
    general 150 + 20 + 15 + 1 = 186 <= 192 - 4; D holds 2000: 57 * 32 <= 2000 is thin, 186 * 32 > 2000 general, and
    2186 postings over 2^17 docs are far below the doc-tile density."""
    rng = np.random.default_rng(seed)
    n = N17
    np_, n2, n3 = (40, 10, 6) if cls == "thin" else (150, 20, 15)
    run = np.arange(run_start, run_start + 9)
    assert run[0] >> 9 == run[-1] >> 9, "the run sits in ONE bucket"
    extra = list(run)
    if second_run is not None:
        extra += list(second_run)
    head = [0, 7, 300, 301, 600] if bucket0_full else [0]   # doc 0; bucket0_full: four entries in bucket 0, one in bucket 1
    base = _spaced(rng, np_ - len(extra) - len(head), 1024, n - 2048, avoid=extra)
    p = np.concatenate([head, base, extra])
    s2 = list(run[[1, 4, 5, 8]]) + ([7, 600] if bucket0_full else []) + [int(base[3])]
    s3 = list(run[[0, 4, 6]]) + [int(base[5])]
    d = np.concatenate([rng.choice(n, 1990, replace=False), run[[0, 2, 4, 7]], rng.choice(base, 4, replace=False), [run[0] - 1, run[-1] + 1]])
    if second_run is not None:
        d = np.concatenate([d, np.asarray(second_run)[[1, 5, 6, 10]]])
        s2 += list(np.asarray(second_run)[[0, 5, 7, 11]])
    lists = [_lst(rng, d), _lst(rng, p), _lst(rng, _pad(rng, s2, n2, n - 1)), _lst(rng, _pad(rng, s3, n3, n - 1)), _lst(rng, [n - 1])]
    assert [len(lists[i][0]) for i in (1, 2, 3)] == [np_, n2, n3]
    foreign = sum(len(lists[i][0]) for i in (1, 2, 3, 4))
    assert foreign <= FB[cls] - 4, (foreign, "all foreign postings fit one super-batch")
    assert max(len(lists[i][0]) for i in (2, 3, 4)) < np_ and len(lists[0][0]) > np_
    return n, _doc_len(rng, n), lists, [list(o) for o in ORDERS5], list(IDF5), list(W5)


FULL_RUN = 40 * 512 + 100                 # bucket 40: general positions ~23 .. 32 of P's window, thin ~6 .. 15 (inside one chunk)
CUT_RUN = np.arange(65530, 65542)         # 6 docs at the end of bucket 127, 6 at the start of bucket 128: straddles doc 65536


@family(bodies=["thin"] * 4, events=["full_lanes", "next_moves", "owner_found", "pass_a_placed", "table_hits"],
        split={"thin": 700}, run=(65530, 65541))
def full_bucket_thin():
    """Full bucket in pass A, thin class (FB = 64, one foreign chunk).  The primary foreign list spans the whole segment and
    holds 9 consecutive docIds in bucket 40 (docs 20580 .. 20588; 512 docs per bucket): positions 4 .. 8 of the run have
    pos >= 4 and fall to the claim loop, which finds the bucket full and moves on to bucket 41.  S2 and S3 hold docs of the
    run (owners found through two foreign terms, after a spill too); the driver holds run docs 0, 2, 4, 7 and the docs next
    to the run.  A second run of 12 docs straddles doc 65536 (buckets 127 | 128, six each: both full): the split variant
    cuts the doc range there (work 2000 + 8 * 57 at split 700, doubled for the thin class: two ranges), which puts its first
    half into the LAST bucket of the range [0, 65536) and makes the spill wrap.  Edges: a one-posting list, doc 0, doc n_docs - 1."""
    return _driver_window_family(11, "thin", FULL_RUN, second_run=CUT_RUN)


@family(bodies=["general"] * 4, events=["full_lanes", "next_moves", "owner_found", "pass_a_placed", "table_hits"],
        split={"general": 2000}, run=(65530, 65541), ks=True)
def full_bucket_general():
    """full_bucket_thin in the general class (FB = 192, three foreign chunks; the run sits inside the first chunk of the
    primary list's window).  Split variant: work 2000 + 8 * 186 at split 2000 gives two ranges (eight at K > 32), all cut
    at multiples of 2^14: doc 65536 is one of the cuts."""
    return _driver_window_family(12, "general", FULL_RUN, second_run=CUT_RUN)


WRAP_RUN = N17 - 12                        # docs 131060 .. 131068: the last bucket (255) of the super-batch [0, 131071]


@family(bodies=["thin"] * 4, events=["full_lanes", "next_moves", "wrap_moves", "owner_found"])
def spill_wrap_thin():
    """Spill and wrap, thin class: the run of 9 sits in the highest docs at or below hi = n_docs - 1, bucket NB - 1 = 255; its
    five overflow lanes move to bucket 0, which the primary list filled in pass A (docs 0, 7, 300, 301), and on to bucket 1.
    A driver posting of the run then walks 255 -> 0 -> 1 to find its entry; the driver's doc next to the run walks the same
    way and finds none."""
    return _driver_window_family(13, "thin", WRAP_RUN, bucket0_full=True)


@family(bodies=["general"] * 4, events=["full_lanes", "next_moves", "wrap_moves", "owner_found"])
def spill_wrap_general():
    """spill_wrap_thin in the general class (the run is the tail of the primary window's third chunk)."""
    return _driver_window_family(14, "general", WRAP_RUN, bucket0_full=True)


@family(bodies=["general"] * 3, events=["carry_chunks", "full_lanes", "next_moves", "pass_a_placed"])
def carry_general():
    """Carry across chunks, general class only (the thin class has one chunk).  The primary list P is the FIRST foreign term
    of every query, so its window starts at flat position 0: postings 60 .. 68 are 9 consecutive docIds of one bucket (chunk 0
    places four, chunk 1 starts in the same bucket with carry_n == 4: its five lanes have pos >= 4), and postings 126 .. 129
    are 4 consecutive docIds of another bucket (two placed by chunk 1; chunk 2 continues at carry_n == 2 and places the other
    two behind them — without the carry they would overwrite the first two)."""
    rng = np.random.default_rng(15)
    n = N17
    run1 = np.arange(60 * 512 + 17, 60 * 512 + 26)     # bucket 60
    run2 = np.arange(130 * 512 + 400, 130 * 512 + 404)  # bucket 130
    a = _spaced(rng, 60, 0, 59 * 512)
    a[0] = 0
    b = _spaced(rng, 57, 62 * 512, 129 * 512)
    c = _spaced(rng, 20, 132 * 512, n - 2048)
    p = np.concatenate([a, run1, b, run2, c])
    assert len(np.unique(p)) == 150 and np.array_equal(np.sort(p)[60:69], run1) and np.array_equal(np.sort(p)[126:130], run2)
    s2 = np.concatenate([run1[[1, 3, 4, 8]], run2[[1, 2]], rng.choice(b, 2, replace=False), rng.choice(n - 1, 12, replace=False)])
    s3 = np.concatenate([run1[[0, 4, 5]], run2[[3]], rng.choice(n - 1, 11, replace=False)])
    d = np.concatenate([rng.choice(n, 1990, replace=False), run1[[0, 2, 4, 7]], run2[[0, 2]], rng.choice(a, 4, replace=False)])
    lists = [_lst(rng, d), _lst(rng, p), _lst(rng, s2), _lst(rng, s3), _lst(rng, [n - 1])]
    foreign = sum(len(lists[i][0]) for i in (1, 2, 3, 4))
    assert foreign <= FB["general"] - 4 and foreign * 32 > len(lists[0][0])
    return n, _doc_len(rng, n), lists, [[0, 1, 2, 3, 4], [1, 0, 2, 3, 4], [1, 2, 3, 4, 0]], list(IDF5), list(W5)


def _primary_choice(seed, cls):
    rng = np.random.default_rng(seed)
    n = N17
    nd = 2000 if cls == "thin" else 300
    r = np.arange(77 * 512 + 5, 77 * 512 + 12)          # 7 docs of bucket 77
    f5 = np.concatenate([r[:3], [9000, 100000]])
    f7 = np.concatenate([r[:6], [64000]])               # six docs of one bucket through the claim loop alone: full bucket, spill
    f3 = [r[1], 30000, n - 1]
    g12a = np.concatenate([r, _spaced(rng, 5, 2048, n - 4096, avoid=r)])
    g12b = np.concatenate([r[2:], _spaced(rng, 7, 2048, n - 4096, avoid=r)])
    h8 = np.concatenate([r[:5], [0, 50000, 120000]])
    h5 = np.concatenate([r[3:6], [50000, 70000]])
    d = np.concatenate([rng.choice(n, nd - 6, replace=False), r[[0, 2, 5]], [50000, 64000, r[-1] + 1]])
    lists = [_lst(rng, d)] + [_lst(rng, x) for x in (f5, f7, f3, g12a, g12b, h8, h5)]
    assert [len(x[0]) for x in lists[1:]] == [5, 7, 3, 12, 12, 8, 5]
    queries = [[0, 1, 2, 3], [1, 2, 0, 3], [1, 2, 3, 0],          # every window < 8: no primary term, no pass A
               [0, 4, 5], [5, 0, 4], [4, 5, 0],                  # two windows tie at 12: the first of them in term order is the primary
               [0, 6, 7], [7, 0, 6], [7, 6, 0]]                  # the largest window is exactly 8
    return n, _doc_len(rng, n), lists, queries, [1.5, 3.25, 6.0, 2.125, 9.5, 4.0, 2.75, 5.5], [1.0, 0.5, 1.0, 0.75, 1.0, 1.0, 0.6, 1.0]


@family(bodies=["thin"] * 9, events=["no_primary", "pass_a_placed", "full_lanes", "next_moves", "owner_found"])
def primary_choice_thin():
    """Choice of the primary foreign term, thin class (driver of 2000; the foreign lists hold 15, 24 and 13 postings in all,
    one super-batch each).  Windows of 5, 7 and 3: wmax < 8, no pass A, and six docs of one bucket go through the claim loop
    alone (full bucket, spill).  Windows of 12 and 12: a tie for the largest window.  Windows of 8 and 5: wmax exactly 8.
    Seven consecutive docs of bucket 77 are shared by all of them."""
    return _primary_choice(16, "thin")


@family(bodies=["general"] * 9, events=["no_primary", "pass_a_placed", "full_lanes", "next_moves", "owner_found"])
def primary_choice_general():
    """primary_choice_thin with a driver of 300 postings: 13 * 32 > 300 puts every group into the general class."""
    return _primary_choice(17, "general")


def _term_counts(seed, cls):
    rng = np.random.default_rng(seed)
    n = N17
    nd, np_ = (4000, 30) if cls == "thin" else (2000, 100)
    run = np.arange(200 * 512 + 50, 200 * 512 + 56)
    p = np.concatenate([run, _spaced(rng, np_ - 6, 1024, n - 2048, avoid=run)])
    ones = rng.choice(n, 62, replace=False)
    ones[:4] = [run[0], run[5], 0, n - 1]               # one-posting lists on the run, at doc 0 and at the last doc
    d = np.concatenate([rng.choice(n, nd - 8, replace=False), run[[0, 3, 5]], ones[4:9]])
    dm = rng.choice(n, 600, replace=False)              # with P = 100: 100 * 8 >= 600, a merge pair while the merge body is on
    lists = [_lst(rng, d), _lst(rng, p)] + [_lst(rng, [x]) for x in ones] + [_lst(rng, dm)]
    assert len(lists) == 65 and len(lists[0][0]) > 600
    queries = [[0, 1], [1, 0]] if cls == "thin" else [[64, 1], [1, 64]]
    for t in (3, 8, 9, 16, 17, 64):
        f = list(range(2, t))                           # t - 2 one-posting lists
        queries += [[0, 1] + f, [1] + f[: len(f) // 2] + [0] + f[len(f) // 2:], [1] + f + [0]]
    idfs = [1.5, 3.25] + [float(2.0 + 0.125 * (i % 40)) for i in range(62)] + [2.5]
    weights = [1.0, 0.5] + [1.0 if i % 3 else 0.75 for i in range(62)] + [1.0]
    return n, _doc_len(rng, n), lists, queries, idfs, weights


@family(bodies=["thin"] * 20, events=["many_terms", "owner_found", "pass_a_placed"], merge=False)
def term_counts_thin():
    """Term counts 2 (merge body off), 3, 8, 9, 16, 17 and 64, the driver first, in the middle and last; from 9 terms on the
    foreign terms are one-posting lists (T <= 8 counts a posting's term with readlanes, T > 8 searches the window ends; 17 and
    more terms run in the 64-term instantiation of the kernel).  Thin class: driver 4000, (30 + 62) * 32 <= 4000; with 63
    active foreign terms the 64-posting budget leaves one posting per window and a super-batch.  Two one-posting lists sit on
    the primary list's run of six docs, two more at doc 0 and at n_docs - 1."""
    return _term_counts(18, "thin")


def _tc_general_bodies(n_docs, lists, queries):
    return ["general"] * len(queries)


@family(bodies=_tc_general_bodies, events=["many_terms", "owner_found", "pass_a_placed", "full_lanes"], merge=False)
def term_counts_general():
    """term_counts_thin in the general class: driver 2000, primary list 100 (100 * 32 > 2000).  The two-term queries pair the
    primary list with a list of 600: general and within the merge ratio, so they take the driver-stream body only because
    the family runs with the merge body off."""
    return _term_counts(19, "general")


def _long(seed, cls):
    rng = np.random.default_rng(seed)
    n = 300_000
    lim = int(0.7 * n)
    starts = [1000 + i * 29000 for i in range(7)]
    runs = np.concatenate([np.arange(s, s + 12) for s in starts])
    p = np.unique(np.concatenate([rng.choice(lim, 520, replace=False), runs]))
    s2 = np.concatenate([rng.choice(lim, 100, replace=False), runs[1::5], rng.choice(p, 10, replace=False)])
    s3 = np.concatenate([rng.choice(lim, 50, replace=False), runs[2::7]])
    if cls == "general":
        d = np.concatenate([rng.choice(n // 2, 5000, replace=False), runs[::3][:20]])      # no driver posting above n / 2
    else:
        d = np.concatenate([n // 5 + rng.choice(n - n // 5, 30000, replace=False), runs[40::3]])   # none below n / 5
    lists = [_lst(rng, d), _lst(rng, p), _lst(rng, s2), _lst(rng, s3), _lst(rng, [n - 1])]
    rest = sum(len(lists[i][0]) for i in (1, 2, 3, 4))
    assert (rest * 32 <= len(lists[0][0])) == (cls == "thin") and rest > 3 * FB[cls]
    queries = [[0, 1, 2, 3, 4], [1, 2, 0, 3], [1, 2, 3, 0], [2, 0, 1]]
    return n, _doc_len(rng, n), lists, queries, list(IDF5), list(W5)


@family(bodies=["general"] * 4, events=["full_lanes", "next_moves", "owner_found", "super_batches"], ks=True)
def long_lists_general():
    """Many super-batches, general class, n_docs = 300000 (not a power of two: the bucket multiplier is rounded).  The primary
    list holds ~600 postings in the first 70 % of the docs with a run of 12 consecutive docIds every 29000 docs (at most two
    buckets: one of them holds >= 6), every list ends on its last window's last posting, the driver has no posting above
    n_docs / 2 (super-batches with foreign postings only), and the queries without the one-posting list at n_docs - 1 end
    with nothing foreign left."""
    return _long(20, "general")


@family(bodies=["thin"] * 4, events=["full_lanes", "next_moves", "owner_found", "super_batches"])
def long_lists_thin():
    """long_lists_general in the thin class: driver of 30000 postings, none below n_docs / 5 (the first super-batches hold
    foreign postings only) and streaming on after the foreign lists end at 70 % (super-batches without foreign postings)."""
    return _long(21, "thin")


# ---------------------------------------------------------------- merge body
N16 = 1 << 16
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513)
LONG = 4090     # 511 * 8 < 4090 <= 512 * 8: the merge ratio falls between the lengths 511 and 512


@family(bodies=["merge"] * 10, events=["merge_items", "hi_from_a", "hi_from_b", "hi_from_end", "a_exhausted", "b_exhausted", "b_window_4",
                                        "merge_matches"], ks=True)
def merge_layouts():
    """Merge body, both term orders each: identical docIds (700 | 700: equal lengths, the first term is A; every round's last
    posting is a match), disjoint interleaved lists (even | odd docs), B entirely below A and B entirely above A (1000 | 300:
    B is exhausted while A goes on, and A while B goes on: steps with b_rem == 0 and with a_rem == 0, windows of four
    chunks), and A = 1024 postings against B = every 256th posting of A plus 200 docs outside A (matches on the rounds' last
    loaded docIds while hi comes from A's round)."""
    rng = np.random.default_rng(30)
    n = N16
    same = np.sort(rng.choice(n, 700, replace=False))
    even = 2 * np.sort(rng.choice(n // 2, 600, replace=False))
    odd = 2 * np.sort(rng.choice(n // 2, 500, replace=False)) + 1
    mid = 20000 + np.sort(rng.choice(20000, 1000, replace=False))
    below = np.sort(rng.choice(15000, 300, replace=False))
    above = 45000 + np.sort(rng.choice(n - 45000, 300, replace=False))
    a = 16 * np.sort(rng.choice(n // 16, 1024, replace=False))
    b = np.concatenate([a[255::256], 16 * rng.choice(n // 16, 200, replace=False) + 5])
    lists = [_lst(rng, x) for x in (same, same, even, odd, mid, below, above, a, b)]
    assert len(lists[8][0]) == 204
    queries = [[0, 1], [1, 0], [2, 3], [3, 2], [4, 5], [5, 4], [4, 6], [6, 4], [7, 8], [8, 7]]
    return n, _doc_len(rng, n), lists, queries, [1.5, 2.5, 3.25, 1.75, 2.125, 6.0, 5.5, 1.25, 4.0], [1.0, 0.5, 1.0, 1.0, 0.75, 1.0, 1.0, 1.0, 0.6]


def _merge_length_queries():
    qs = []
    for i in range(10):
        for j in range(10):
            qs += [[i, 10 + j], [10 + j, i]]
        qs += [[i, 20], [20, i]]
    return qs


@family(bodies=bodies_by_rule(), events=["merge_items", "b_window_1", "b_window_4", "hi_from_a", "merge_matches"])
def merge_lengths():
    """List lengths 1, 63, 64, 65, 255, 256, 257, 511, 512 and 513 (around a chunk, a round and two rounds) paired with each
    other — lists 0 .. 9 against lists 10 .. 19 of the same lengths, which share about a third of their docs — and with one
    list of 4090, in both term orders.  Which pairs take the merge body is the planner's rule (plan_rule): pairs of equal
    lengths do (the first term is A), 64 | 513 does not (64 * 8 < 513) while 65 | 513 does, and against the long list the
    ratio falls between 511 (driver-stream body) and 512 (merge body); pairs with a list of one posting are thin."""
    rng = np.random.default_rng(31)
    n = N16
    pool = rng.choice(n, 3000, replace=False)
    lists = [_lst(rng, rng.choice(pool[:1500], ln, replace=False)) for ln in LENGTHS]
    lists += [_lst(rng, rng.choice(pool[1000:2500], ln, replace=False)) for ln in LENGTHS]
    lists.append(_lst(rng, np.concatenate([pool[:2000], rng.choice(np.setdiff1d(np.arange(n), pool), LONG - 2000, replace=False)])))
    assert len(lists[20][0]) == LONG
    idfs = [float(1.0 + 0.25 * i) for i in range(21)]
    weights = [1.0 if i % 4 else 0.5 for i in range(21)]
    return n, _doc_len(rng, n), lists, _merge_length_queries(), idfs, weights


# ---------------------------------------------------------------- doc-tile body
def _tile_edges(seed, n):
    rng = np.random.default_rng(seed)
    cells = (n + SKIP_DOCS - 1) // SKIP_DOCS
    last_lo = (cells - 1) * SKIP_DOCS                    # first doc of the last cell (partial unless n is a multiple of 1024)
    every2 = np.arange(0, n, 2)
    ends = np.concatenate([np.flatnonzero(rng.random(1024) < 0.4), 3072 + np.flatnonzero(rng.random(min(1024, n - 3072)) < 0.4)])   # cells 0 and 3 only
    in_last = np.arange(last_lo, n)                      # every posting in the last cell
    to_1023 = np.arange(500, 1024)                       # ends on the last doc of cell 0
    first_last = np.concatenate([np.arange(100, 700), in_last[::2]])
    thirds = np.arange(1, n, 3)
    lists = [_lst(rng, x) for x in (every2, ends, in_last, to_1023, first_last, thirds)]
    queries = [[0, 1], [1, 4], [0, 2, 5], [2, 0, 3], [3, 1], [5, 0, 4], [4, 1, 3], [5, 2, 0]]
    return n, _doc_len(rng, n), lists, queries, [1.5, 2.5, 3.25, 1.75, 2.125, 1.25], [1.0, 0.5, 1.0, 1.0, 0.75, 1.0]


TILE_EVENTS = ["tile_items"]


@family(bodies=["tile"] * 8, events=TILE_EVENTS)
def tile_edges_4095():
    """Doc-tile body, n_docs = 1024 * 4 - 1: the last cell misses one doc.  Lists: every second doc; 40 % of cells 0 and 3
    with cells 1 and 2 EMPTY; every doc of the last cell and nothing else; docs 500 .. 1023 (the list ends on a cell's last
    doc); docs of the first and the last cell only; every third doc.  [ends, first_last] and [to_1023, ends] leave the middle
    cells without a posting of any term.  Every group holds >= 0.25 postings per doc and no list dominates."""
    return _tile_edges(40, 4095)


@family(bodies=["tile"] * 8, events=TILE_EVENTS, ks=True)
def tile_edges_4096():
    """tile_edges_4095 with n_docs = 1024 * 4: the last cell is whole and the last list position is the segment's end."""
    return _tile_edges(41, 4096)


@family(bodies=["tile"] * 8, events=TILE_EVENTS)
def tile_edges_4097():
    """tile_edges_4095 with n_docs = 1024 * 4 + 1: the last cell holds ONE doc, and one list is that single posting."""
    return _tile_edges(42, 4097)


# ---------------------------------------------------------------- top-K floods
def _flood(seed, rising):
    rng = np.random.default_rng(seed)
    n = 60000
    docs = np.arange(n)
    doc_len = (70000 - docs if rising else 10001 + docs).astype(np.uint32)   # shorter docs score higher: 60000 distinct lengths
    f0 = np.sort(rng.choice(n, 6000, replace=False))
    f1 = np.sort(rng.choice(n, 5000, replace=False))
    f2 = np.sort(rng.choice(n, 200, replace=False))
    f3 = np.sort(rng.choice(n, 150, replace=False))
    g0, g1 = docs[::3], docs[1::7]
    lists = [(x.astype(np.uint32), np.full(len(x), 2, np.uint32)) for x in (f0, f1, f2, f3, g0, g1)]
    queries = [[0, 1], [1, 0], [0, 2, 3], [2, 0, 3], [4, 2], [2, 4], [4, 5], [5, 4]]
    return n, doc_len, lists, queries, [1.5, 1.5, 1.5, 1.5, 1.5, 1.5], [1.0] * 6


FLOOD_BODIES = ["merge", "merge", "general", "general", "thin", "thin", "tile", "tile"]


@family(bodies=FLOOD_BODIES, events=["shrinks_in_step", "shrinks_between", "merge_items", "tile_items", "driver_items"], ks=True)
def flood_rising():
    """Top-K flood, one query pair per body (merge 6000 | 5000, general 6000 + 200 + 150, thin 20000 + 200, tiles 20000 + 8572
    over 60000 docs).  Every posting has tf 2 and doc lengths FALL by one per docId, so scores rise strictly with the docId:
    every round of 256 offers 256 candidates above theta, the buffer (128 entries up to K = 32, 256 above) overflows in the
    middle of steps and between them.  This family deliberately uses lengths that are a function of the docId."""
    return _flood(50, True)


@family(bodies=FLOOD_BODIES, events=["merge_items", "tile_items", "driver_items"], ks=True)
def flood_falling():
    """flood_rising with doc lengths rising by one per docId: scores fall strictly, so after the first shrink nothing beats
    theta again and the K best are the first docs of the lists."""
    return _flood(51, False)
