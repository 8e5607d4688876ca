"""Directed inputs and the runner of the shared-top-rows tests (ns_ctx_share_rows; k_rscore, ns_row_kernel.hip).  Plain data
and helpers: tests/test_row_sharing_gpu.py runs every case on the product library; run as a script on the counting build
(tests/test_row_sharing_gpu.py starts it in ONE child process) it runs the cases again and writes the consumer's counters.

The common shape: a segment of 5000 docs — four whole 1024-doc cells of the skip grid and a ragged fifth — with one hot list H
of 2500 postings.  The cell size is forced to 1000 postings (NS_ROW_CELL, read at ns_ctx_create), so H is cut into C_H = 4
cells: [0, 1024), [1024, 2048), [2048, 3072), [3072, 5000).  H and a tail are a thin group while the tails hold at most
2500 / 32 = 78 postings; a thin item loads at most 64 foreign postings less one per foreign list per super-batch.

A case is a function returning a dict: n_docs, doc_len, lists [(docIds, tfs)], queries (lists of list numbers), idfs,
weights, and optionally  k (default 10), consumers (the number of consumer items the batch must report; None: at least
one), ref (False: no numpy restatement), events (counters of the counting build that must be above zero), split
(ns_set_tuning's work units per item), fallbacks / row_hits ("some": the stat must be above zero).

The cases of the second part (below `plan_rows`) leave that frame: other segment sizes (n_docs), other cell sizes (row_cell; None:
the library's own 65536), one list under two weights (alias: {list number: the list whose payload it names}), lists without
a skip table (no_skips), a declared producer count (producers) and a direct batch (direct).  They are `exact`: their four
stats must equal `expected_stats`, the numpy restatement of the planner's rule and of the consumer's proof, and each asserts
on the CPU, before anything runs, that its input has the property it was built for."""
import collections
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np

N_DOCS = 5000
CELLS = [(0, 1024), (1024, 2048), (2048, 3072), (3072, 5000)]
ROW_CELL = "1000"
EVENTS = {"consumer_items": 19, "lookups": 28, "lookup_hits": 29, "row_probes": 30, "row_table_hits": 31}   # ns_debug_counters
CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def _base(seed, equal=False, hot=2500):
    rng = np.random.default_rng(seed)
    doc_len = np.full(N_DOCS, 300, np.uint32) if equal else rng.integers(20, 3000, size=N_DOCS, dtype=np.uint32)
    h = np.sort(rng.choice(N_DOCS, size=hot, replace=False)).astype(np.uint32)
    tf = np.ones(hot, np.uint32) if equal else rng.integers(1, 9, size=hot, dtype=np.uint32)
    return rng, doc_len, (h, tf)


def _tail(rng, docs, equal=False):
    d = np.unique(np.asarray(docs, np.int64)).astype(np.uint32)
    return d, (np.ones(len(d), np.uint32) if equal else rng.integers(1, 9, size=len(d), dtype=np.uint32))


def _pick(rng, n, lo=0, hi=N_DOCS, inside=None, outside=None):
    """n distinct docs of [lo, hi), of `inside` or not of `outside` when given"""
    pool = np.arange(lo, hi)
    if inside is not None:
        pool = pool[np.isin(pool, inside)]
    if outside is not None:
        pool = pool[~np.isin(pool, outside)]
    return rng.choice(pool, size=n, replace=False)


def _mk(doc_len, lists, queries, idfs=None, weights=None, **kw):
    n = len(lists)
    idfs = idfs or [1.5 + 0.625 * i for i in range(n)]
    weights = weights or [1.0 if i % 3 else 0.75 for i in range(n)]
    kw.setdefault("n_docs", N_DOCS)
    return dict(doc_len=doc_len, lists=lists, queries=queries, idfs=idfs, weights=weights, **kw)


@case
def tails_1_3_70_200():
    """tails of 1, 3, 70 and 200 postings.  The 70 lie in ONE cell, half of them docs of H: more than the 63 a super-batch
    takes.  The 200 are spread: 200 * 32 > 2500, so that group is not thin and keeps to the scoring launch."""
    rng, dl, H = _base(11)
    t70 = np.concatenate([_pick(rng, 35, 1024, 2048, inside=H[0]), _pick(rng, 35, 1024, 2048, outside=H[0])])
    lists = [H, _tail(rng, _pick(rng, 1)), _tail(rng, _pick(rng, 3)), _tail(rng, t70), _tail(rng, _pick(rng, 200))]
    q = [[0, 1], [0, 2], [0, 3], [0, 4], [0, 1], [0, 3], [0, 2], [0]]
    return _mk(dl, lists, q, consumers=7 * 4, events=("consumer_items", "lookups", "lookup_hits", "row_probes"))


@case
def tail_placement():
    """a tail before the driver in query order, after it, three tails, and a tail that shares docs with another tail and with
    H: three contributions to one doc, in term order"""
    rng, dl, H = _base(12)
    a = _pick(rng, 20)
    both = _pick(rng, 6, inside=H[0])
    lists = [H, _tail(rng, a), _tail(rng, np.concatenate([a[:8], both, _pick(rng, 10)])), _tail(rng, np.concatenate([both[:3], _pick(rng, 12)]))]
    q = [[1, 0], [0, 1], [1, 0, 2], [2, 1, 0], [0, 2, 3], [1, 2, 3, 0], [3, 0, 1, 2], [2, 0]]
    return _mk(dl, lists, q, consumers=8 * 4, events=("lookups", "lookup_hits"))


def _k_case(k, consumers):
    rng, dl, H = _base(13)
    lists = [H, _tail(rng, _pick(rng, 40)), _tail(rng, _pick(rng, 25)), _tail(rng, _pick(rng, 9, 2048, 3072))]
    q = [[0, 1], [1, 0], [0, 2], [0, 3], [0, 1, 2], [0], [3, 0], [0, 2, 3]]
    return _mk(dl, lists, q, k=k, consumers=consumers)


@case
def k_1():
    return _k_case(1, 32)


@case
def k_10():
    return _k_case(10, 32)


@case
def k_32():
    return _k_case(32, 32)


@case
def k_33():
    """K = 33: no group is row-eligible"""
    return _k_case(33, 0)


def _hot_scores(c_doc_len, H, idf, w):
    import rawseg
    acc = rawseg._np_bm25([H], [0], [idf], [w], c_doc_len, rawseg.avgdl_of(c_doc_len))
    return sorted(acc.items(), key=lambda kv: (-float(kv[1]), kv[0]))


@case
def tail_doc_in_the_row():
    """tails that hold the best docs of H in two cells: row entries that hit the table"""
    rng, dl, H = _base(14)
    ranked = _hot_scores(dl, H, 1.5, 0.75)
    best0 = [d for d, _ in ranked if d < 1024][:3]
    best3 = [d for d, _ in ranked if d >= 3072][:2]
    lists = [H, _tail(rng, np.concatenate([best0, _pick(rng, 10, outside=H[0])])), _tail(rng, np.concatenate([best3, best0[:1], _pick(rng, 5)]))]
    q = [[0, 1], [1, 0], [0, 2], [0, 1, 2], [2, 0, 1], [0, 1], [0, 2], [0]]
    return _mk(dl, lists, q, consumers=32, row_hits="some", events=("row_probes", "row_table_hits", "lookup_hits"))


@case
def ties_everywhere():
    """all doc lengths equal and tf = 1: every score of H is the same number and docId order decides every row; the tails
    carry H's idf and weight, so a doc of a tail alone ties with the docs of H alone — at theta, for K = 10"""
    rng, dl, H = _base(15, equal=True)
    t1 = _tail(rng, np.concatenate([_pick(rng, 4, inside=H[0]), _pick(rng, 6, outside=H[0])]), equal=True)
    t2 = _tail(rng, np.concatenate([_pick(rng, 2, 0, 1024, outside=H[0]), [0, 1, 2, 3, 1024, 1025, 3072, 4999]]), equal=True)
    lists = [H, t1, t2]
    q = [[0, 1], [1, 0], [0, 2], [2, 0], [0, 1, 2], [0], [2, 1, 0], [0, 2]]
    return _mk(dl, lists, q, idfs=[2.0, 2.0, 2.0], weights=[1.0, 1.0, 1.0], consumers=32)


@case
def short_cells():
    """H with 1000 postings in each of the first two cells, 40 in the third (its row is complete) and none in the fourth"""
    rng = np.random.default_rng(16)
    dl = rng.integers(20, 3000, size=N_DOCS, dtype=np.uint32)
    h = np.sort(np.concatenate([_pick(rng, 1000, 0, 1024), _pick(rng, 1000, 1024, 2048), _pick(rng, 40, 2048, 3072)])).astype(np.uint32)
    H = (h, rng.integers(1, 9, size=len(h), dtype=np.uint32))
    # a tail of the best docs of the short cell (its row holds them all: no fallback), and tails in the empty cell
    # K = 32 and 36 of the short cell's 40 docs in a tail: more row entries hit the table than 64 - K, and only the row's
    # holding the whole cell proves the item
    lists = [H, _tail(rng, np.concatenate([h[h >= 2048][:36], _pick(rng, 8, 3072, 5000)])), _tail(rng, _pick(rng, 20, 3072, 5000)),
             _tail(rng, _pick(rng, 12))]
    q = [[0, 1], [1, 0], [0, 2], [0, 3], [0, 1, 3], [0], [2, 0], [0, 2, 3]]
    return _mk(dl, lists, q, k=32, consumers=32, fallbacks=0, row_hits="some")


@case
def forced_split():
    """ns_set_tuning's doc-range split at 256 work units: the other groups are cut finer, the consumers keep their cells"""
    rng, dl, H = _base(17)
    lists = [H, _tail(rng, _pick(rng, 30)), _tail(rng, _pick(rng, 900)), _tail(rng, _pick(rng, 100))]
    q = [[0, 1]] * 4 + [[1, 0], [0], [2, 3], [0, 1]]
    return _mk(dl, lists, q, split=256, consumers=7 * 4)


@case
def mixed_batch():
    """eligible groups next to a general, a doc-tile and a merge group (body_shapes.plan_rule names their classes)"""
    import body_shapes
    rng, dl, H = _base(18)
    lists = [H, _tail(rng, _pick(rng, 50)), _tail(rng, _pick(rng, 900)), _tail(rng, _pick(rng, 100)), _tail(rng, _pick(rng, 600)),
             _tail(rng, _pick(rng, 400)), _tail(rng, _pick(rng, 1500)), _tail(rng, _pick(rng, 7))]
    q = [[0, 1], [2, 3], [0, 7], [0, 6], [4, 5], [1, 0, 7], [0], [7, 0], [2, 3, 7]]
    want = ["thin", "general", "thin", "tile", "merge", "thin", "thin", "thin", "general"]
    assert [body_shapes.plan_rule([len(lists[li][0]) for li in g], N_DOCS) for g in q] == want
    return _mk(dl, lists, q, consumers=5 * 4)


@case
def no_eligible_group():
    """a general and a merge group, and three users of H — one short of the rule: no rows at all"""
    rng, dl, H = _base(19)
    lists = [H, _tail(rng, _pick(rng, 50)), _tail(rng, _pick(rng, 900)), _tail(rng, _pick(rng, 100)), _tail(rng, _pick(rng, 600)), _tail(rng, _pick(rng, 400))]
    q = [[2, 3], [4, 5], [0, 1], [1, 0], [0], [1]]
    return _mk(dl, lists, q, consumers=0)


# ---- the planner's rule and the consumer's proof, restated ---------------------------------------------------------------
SKIP_DOCS, SKIP_MIN, ROW_LEN, MAX_TERMS, MIN_USERS, CELL_POSTINGS = 1024, 64, 64, 16, 4, 65536


def _view(c):
    """-> (segments as (n_docs, doc_len, lists, idfs, weights), queries as lists of (segment, list number)); a case with
    `segments` is a several-segment one already"""
    if "segments" in c:
        return [(n, np.ascontiguousarray(dl, np.uint32), ls, c["idfs"][s], c["weights"][s]) for s, (n, dl, ls) in enumerate(c["segments"])], c["queries"]
    return [(c["n_docs"], np.ascontiguousarray(c["doc_len"], np.uint32), c["lists"], c["idfs"], c["weights"])], [[(0, li) for li in q] for q in c["queries"]]


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def row_cells(n_docs, count, cell_postings):
    """the doc ranges a hot list of `count` postings is cut into: a power-of-two cut that leaves at most cell_postings per cell
    on average, capped at one cell per cell of the skip grid; ranges start and end on the grid"""
    cells = 1
    while cells * max(cell_postings, 1) < count and cells * 2 <= n_docs // SKIP_DOCS and cells < 4096:
        cells *= 2
    out = []
    for i in range(cells):
        lo, hi = n_docs * i // cells, n_docs * (i + 1) // cells
        lo -= lo % SKIP_DOCS
        if i + 1 < cells:
            hi -= hi % SKIP_DOCS
        out.append((lo, hi))
    return out


def plan_rows(c, rows=1, pruning=False, and_mode=False, skips=True):
    """Which (query, segment) groups take rows, restated from the header of ns_ctx_share_rows: a group is a candidate when it
    is thin (the lists next to its largest one hold at most 1/32 of that one's postings), in OR mode at K <= 32, of at most
    16 term refs, without a negative idf or weight, not a single list under pruning, and its hot list (the first largest
    one) has a skip table.  A key is (segment, list, idf bits, weight bits); under mode 1 a key is on with at least four
    candidates, under mode 2 always.  -> dict: users {key: candidates}, cells {key that is on: doc ranges}, consumers
    [(query, segment, list numbers, hot list, key)]"""
    segs, queries = _view(c)
    k, alias, no_skips = c.get("k", 10), c.get("alias", {}), c.get("no_skips", ())
    cell = c.get("row_cell", ROW_CELL)
    cell = CELL_POSTINGS if cell is None else int(cell)
    cand = []
    if rows and skips and not and_mode and k <= 32:
        for qi, q in enumerate(queries):
            for s in sorted({s for s, _ in q}):
                n_docs, _, lists, idfs, weights = segs[s]
                g = [li for ss, li in q if ss == s]
                n = [len(lists[li][0]) for li in g]
                cmax = max(n)
                signed = any(np.signbit(np.float32(idfs[li])) or np.signbit(np.float32(weights[li])) for li in g)
                if (sum(n) - cmax) * 32 > cmax or signed or len(g) > MAX_TERMS or cmax < SKIP_MIN or (pruning and len(g) == 1):
                    continue
                hot = g[n.index(cmax)]
                if (s, alias.get(hot, hot)) in no_skips or (len(segs) == 1 and alias.get(hot, hot) in no_skips):
                    continue
                cand.append((qi, s, g, hot, (s, alias.get(hot, hot), _bits(idfs[hot]), _bits(weights[hot]))))
    users = collections.Counter(key for *_, key in cand)
    cells = {key: row_cells(segs[key[0]][0], len(segs[key[0]][2][key[1]][0]), cell) for key, u in users.items() if rows == 2 or u >= MIN_USERS}
    return dict(users=dict(users), cells=cells, consumers=[x for x in cand if x[4] in cells])


def expected_stats(c, plan):
    """(producer items, consumer items, fallbacks, row hits) of one run of the case under `plan`.  A row is the best 64
    postings of the hot list in the cell (score desc, docId asc); a row entry that is a doc of one of the group's tails hits
    the table; the item falls back when more than 64 - K entries hit and the row does not hold the whole cell."""
    import rawseg
    segs, _ = _view(c)
    k = c.get("k", 10)
    rows = {}
    for key, cells in plan["cells"].items():
        s, li = key[:2]
        _, dl, lists, _, _ = segs[s]
        docs, tfs = lists[li]
        x = rawseg.np_contrib(docs, tfs, np.uint32(key[2]).view(np.float32), np.uint32(key[3]).view(np.float32), dl, rawseg.avgdl_of(dl))
        for lo, hi in cells:
            m = (docs >= lo) & (docs < hi)
            d, v = docs[m], x[m]
            rows[key, lo] = (d[np.lexsort((d, -v))][:ROW_LEN], int(m.sum()) <= ROW_LEN)
    fallbacks = row_hits = items = 0
    for _, s, g, hot, key in plan["consumers"]:
        tails = [segs[s][2][li][0] for li in g if li != hot]
        tails = np.unique(np.concatenate(tails)) if tails else np.zeros(0, np.uint32)
        for lo, hi in plan["cells"][key]:
            row, complete = rows[key, lo]
            h = int(np.isin(row, tails).sum())
            items += 1
            row_hits += h
            fallbacks += int(not complete and h > ROW_LEN - k)
    return (sum(len(v) for v in plan["cells"].values()) if items else 0, items, fallbacks, row_hits)


def expected_lookups(c, plan):
    """(look-ups, look-ups that found the doc) of one run: every doc of a consumer group's tails is looked up once in the
    group's hot list"""
    segs, _ = _view(c)
    n = hit = 0
    for _, s, g, hot, _ in plan["consumers"]:
        tails = [segs[s][2][li][0] for li in g if li != hot]
        if tails:
            t = np.unique(np.concatenate(tails))
            n += len(t)
            hit += int(np.isin(t, segs[s][2][hot][0]).sum())
    return n, hit


def _declare(c, prod, cons, rows=1, **kw):
    """the case with its declared producer and consumer counts, which the restated rule must give too"""
    plan = plan_rows(c, rows, **kw)
    got = (sum(len(v) for v in plan["cells"].values()), sum(len(plan["cells"][x[4]]) for x in plan["consumers"]))
    assert got == (prod, cons), (got, prod, cons)
    return dict(c, producers=prod, consumers=cons, exact=True)


# ---- A. cell geometry and the look-up ---------------------------------------------------------------------------------------
def _one_cell(general):
    import body_shapes
    rng, dl, H = _base(31, hot=900)
    best3 = [d for d, _ in _hot_scores(np.ascontiguousarray(dl, np.uint32), H, 1.5, 0.75)][:3]   # row entries that hit the table
    lists = [H, _tail(rng, _pick(rng, 10)), _tail(rng, _pick(rng, 12)), _tail(rng, np.concatenate([best3, _pick(rng, 2, outside=H[0])]))]
    q = [[0, 1], [1, 0], [0, 2], [0], [0, 1, 2], [2, 0], [0, 3], [0, 1]]
    kw = dict(direct=True, row_hits=3, events=("consumer_items", "lookups", "lookup_hits"))
    if general:
        lists += [_tail(rng, _pick(rng, 900)), _tail(rng, _pick(rng, 100))]
        q = q + [[4, 5]]
        assert body_shapes.plan_rule([len(lists[4][0]), len(lists[5][0])], N_DOCS) == "general"
        kw = dict(direct=False, split=256, row_hits=3)
    c = _mk(dl, lists, q, **kw)
    plan = plan_rows(c)
    assert list(plan["cells"].values()) == [[(0, N_DOCS)]] and list(plan["users"].values()) == [8]   # 900 postings < NS_ROW_CELL: one cell
    return _declare(c, 1, 8)


@case
def one_cell_direct():
    """H of 900 postings at NS_ROW_CELL = 1000 is ONE cell: the consumers are whole items, and with every query a consumer
    the batch is direct — k_rscore writes final result rows and no row join runs"""
    return _one_cell(False)


@case
def one_cell_not_direct():
    """the same with one general group that is cut at 256 work units: the consumers stay whole, the batch is joined"""
    return _one_cell(True)


@case
def capped_cells():
    """n_docs = 3000 caps the cut at 2 cells, [0, 1024) and the ragged [1024, 3000), each with far more than NS_ROW_CELL
    postings of H; tails in both, one of them on the docs next to the cut and on the last doc"""
    n = 3000
    rng = np.random.default_rng(32)
    dl = rng.integers(20, 3000, size=n, dtype=np.uint32)
    drop = np.concatenate([_pick(rng, 9, 1, 1023), [1024], _pick(rng, 90, 1025, 2999)])
    h = np.setdiff1d(np.arange(n), drop).astype(np.uint32)
    H = (h, rng.integers(1, 9, size=len(h), dtype=np.uint32))
    assert len(h) == 2900 and int((h < 1024).sum()) == 1015 and int((h >= 1024).sum()) == 1885
    assert 1023 in h and 1024 not in h and 2999 in h
    lists = [H, _tail(rng, [1023, 1024, 2999]), _tail(rng, np.concatenate([drop[:5], _pick(rng, 15, 0, 1024)])),
             _tail(rng, np.concatenate([drop[-12:], _pick(rng, 18, 1024, n)])), _tail(rng, _pick(rng, 10, 0, n))]
    q = [[0, 1], [0, 2], [0, 3], [1, 0, 4], [0], [0, 2, 3], [4, 0], [0, 1, 4]]
    c = _mk(dl, lists, q, n_docs=n, events=("lookups", "lookup_hits", "row_probes"))
    assert list(plan_rows(c)["cells"].values()) == [[(0, 1024), (1024, 3000)]]
    return _declare(c, 2, 16)


def default_cell_size(k=10):
    """NS_ROW_CELL unset: 200 000 postings over 262144 + 700 docs are cut into 4 cells of at most 65536 postings on average, the
    last one ragged.  Tails on the docs next to every cut, in the ragged end, and on the best docs of the last cell."""
    import rawseg
    n = 262144 + 700
    rng = np.random.default_rng(33)
    dl = rng.integers(20, 3000, size=n, dtype=np.uint32)
    h = np.sort(rng.choice(n, size=200_000, replace=False)).astype(np.uint32)
    H = (h, rng.integers(1, 9, size=len(h), dtype=np.uint32))
    x = rawseg.np_contrib(h, H[1], 1.5, 0.75, dl, rawseg.avgdl_of(dl))
    last = h >= 196608
    best = h[last][np.lexsort((h[last], -x[last]))][:5]
    edges = [0, 65535, 65536, 131071, 131072, 196607, 196608, 262143, 262144, n - 1]
    lists = [H, _tail(rng, np.concatenate([edges, _pick(rng, 30, 0, n)])), _tail(rng, np.concatenate([best, _pick(rng, 25, 262144, n)])),
             _tail(rng, _pick(rng, 25, 0, n, inside=h)), _tail(rng, _pick(rng, 1, 0, n))]
    q = [[0, 1], [2, 0], [0, 3], [0], [0, 1, 2], [3, 0, 4], [0, 4], [1, 0, 3]]
    assert max(sum(len(lists[li][0]) for li in g if li) for g in q) <= 100
    c = _mk(dl, lists, q, n_docs=n, k=k, row_cell=None, row_hits="some")
    assert list(plan_rows(c)["cells"].values()) == [[(0, 65536), (65536, 131072), (131072, 196608), (196608, n)]]
    return _declare(c, 4, 32)


LOOKUP_POPULATIONS = [513, 1024, 0, 64, 1023, 9, 1, 512, 65, 8]   # postings of H per cell of the skip grid


@case
def lookup_cell_populations():
    """The by-eighths look-up at every population of a skip cell that ends a step differently: full (1024: exactly what four
    steps resolve), one short of full, 513 / 512, 65 / 64, 9 / 8, one posting, none.  In every skip cell the tails own the
    first and the last doc of H, the docs just below and above them, a doc of H in the middle and a doc in the middle that H
    does not hold — one tail per kind, so that every group stays thin."""
    n = SKIP_DOCS * len(LOOKUP_POPULATIONS)
    rng = np.random.default_rng(34)
    dl = rng.integers(20, 3000, size=n, dtype=np.uint32)
    parts, owners, skipped = [], collections.defaultdict(list), set()
    for ci, p in enumerate(LOOKUP_POPULATIONS):
        b = ci * SKIP_DOCS
        if p == 1024:
            d = b + np.arange(SKIP_DOCS)
        elif p == 1023:
            d = b + np.setdiff1d(np.arange(SKIP_DOCS), [500])
        else:
            d = b + np.sort(rng.choice(np.arange(2, 1022), size=p, replace=False))
        parts.append(d)
        if p == 0:   # the empty cell: its first and its last doc
            owners["below"].append(b)
            owners["above"].append(b + SKIP_DOCS - 1)
            continue
        first, last = int(d[0]), int(d[-1])
        gap = np.setdiff1d(np.arange(first + 1, last), d)
        for kind, doc in (("first", first), ("last", last), ("below", first - 1 if first > 0 else None), ("above", last + 1 if last + 1 < n else None),
                          ("mid", int(d[p // 2]) if p >= 3 else None), ("gap", int(gap[len(gap) // 2]) if len(gap) else None)):
            if doc is None:
                skipped.add((p, kind))
            else:
                owners[kind].append(doc)
    assert skipped == {(1024, "gap"), (1, "mid"), (1, "gap")}, skipped
    h = np.concatenate(parts).astype(np.uint32)
    assert np.bincount(h // SKIP_DOCS, minlength=len(LOOKUP_POPULATIONS)).tolist() == LOOKUP_POPULATIONS
    H = (h, rng.integers(1, 9, size=len(h), dtype=np.uint32))
    kinds = ["first", "last", "below", "above", "mid", "gap"]
    lists = [H] + [_tail(rng, owners[kd]) for kd in kinds]
    assert [len(lists[1 + i][0]) for i in range(6)] == [9, 9, 10, 10, 8, 7]
    for kd, want in (("first", True), ("last", True), ("mid", True), ("gap", False)):
        assert bool(np.isin(owners[kd], h).all()) == want and bool(np.isin(owners[kd], h).any()) == want
    assert not np.isin(owners["below"], h).any() or not np.isin(owners["above"], h).any()
    q = [[0, 1], [2, 0], [0, 3], [0, 4], [0, 5], [6, 0], [0, 1, 2], [0, 3, 4, 5], [6, 5, 0], [0], [1, 2, 3, 0, 4, 5, 6]]
    c = _mk(dl, lists, q, n_docs=n, events=("lookups", "lookup_hits"))
    assert list(plan_rows(c)["cells"].values()) == [[(0, 2048), (2048, 5120), (5120, 7168), (7168, n)]]
    return _declare(c, 4, 4 * len(q))


# ---- B. keys and eligibility ------------------------------------------------------------------------------------------------
def _two_weights(q):
    rng, dl, H = _base(35)
    lists = [H, _tail(rng, _pick(rng, 20)), _tail(rng, _pick(rng, 30)), _tail(rng, np.concatenate([_pick(rng, 4, inside=H[0]), _pick(rng, 4)])), H]
    return _mk(dl, lists, q, idfs=[1.5, 2.125, 2.75, 3.375, 1.5], weights=[1.0, 1.0, 0.75, 1.0, 0.5], alias={4: 0})


@case
def two_weights_one_list():
    """list 4 IS list 0 (the same postings of the payload) named with weight 0.5 instead of 1.0: two keys, two sets of rows"""
    c = _two_weights([[0, 1], [0, 2], [3, 0], [0], [4, 1], [4, 2], [3, 4], [4]])
    assert sorted(plan_rows(c)["users"].values()) == [4, 4]
    return _declare(c, 8, 32)


@case
def two_weights_three_users_each():
    """three users of each weight: six groups name the list, no key reaches four users — no rows"""
    c = _two_weights([[0, 1], [0, 2], [3, 0], [4, 1], [4, 2], [3, 4]])
    assert sorted(plan_rows(c)["users"].values()) == [3, 3]
    return _declare(c, 0, 0)


@case
def two_hot_lists():
    """thin queries on H1 and on H2, and one query that names both: not thin, no row"""
    import body_shapes
    rng, dl, H1 = _base(36)
    h2 = np.sort(rng.choice(N_DOCS, size=2400, replace=False)).astype(np.uint32)
    lists = [H1, (h2, rng.integers(1, 9, size=len(h2), dtype=np.uint32)), _tail(rng, _pick(rng, 20)), _tail(rng, _pick(rng, 30)), _tail(rng, _pick(rng, 8, inside=h2))]
    q = [[0, 2], [0, 3], [2, 0], [0], [0, 1], [1, 2], [1, 4], [3, 1], [1]]
    assert body_shapes.plan_rule([2500, 2400], N_DOCS) != "thin"
    c = _mk(dl, lists, q)
    plan = plan_rows(c)
    assert sorted(plan["users"].values()) == [4, 4] and 4 not in [x[0] for x in plan["consumers"]]
    return _declare(c, 8, 32)


@case
def sixteen_and_seventeen_refs():
    """H plus 15 tails is the consumer's limit of 16 term refs; H plus 16 tails streams.  The 16-ref group is the fourth user."""
    rng, dl, H = _base(37)
    t = _pick(rng, 64).reshape(16, 4)
    lists = [H] + [_tail(rng, row) for row in t]
    q = [list(range(1, 8)) + [0] + list(range(8, 16)), list(range(1, 9)) + [0] + list(range(9, 17)), [0, 1], [2, 0], [0]]
    assert [len(g) for g in q[:2]] == [16, 17] and 64 * 32 <= 2500
    c = _mk(dl, lists, q)
    plan = plan_rows(c)
    assert list(plan["users"].values()) == [4] and [x[0] for x in plan["consumers"]] == [0, 2, 3, 4]
    return _declare(c, 4, 16)


@case
def signed_and_zero():
    """tf = 0 in H and in the tails: those scores are +0.0f and tie on docId, and K = 10 ends inside the tie.  The group with
    the negative-weight tail is no consumer, its neighbours are."""
    import rawseg
    rng, dl, H = _base(38)
    h, tf = H[0], np.zeros(len(H[0]), np.uint32)
    pos = rng.choice(len(h), size=5, replace=False)
    tf[pos] = rng.integers(1, 9, size=5)
    t1 = np.unique(np.concatenate([h[:3], _pick(rng, 5, outside=h)])).astype(np.uint32)   # the first docs of H: in the row, inside the tie
    t1f = np.zeros(len(t1), np.uint32)
    t1f[-2:] = [3, 1]
    t2 = np.unique(np.concatenate([h[3:6], h[pos[:1]], _pick(rng, 2, 3072, 5000)])).astype(np.uint32)
    neg = np.unique(np.concatenate([h[1:2], _pick(rng, 4)])).astype(np.uint32)
    negf = np.array([0] + [2] * (len(neg) - 1), np.uint32)
    lists = [(h, tf), (t1, t1f), (t2, np.zeros(len(t2), np.uint32)), (neg, negf), _tail(rng, _pick(rng, 4))]
    q = [[0, 1], [0, 2], [0, 3], [4, 0], [1, 0, 2], [0]]
    c = _mk(dl, lists, q, idfs=[1.5, 2.125, 2.75, 3.375, 4.0], weights=[1.0, 0.75, 1.0, -0.5, 1.0])
    dlc = np.ascontiguousarray(dl, np.uint32)
    ref = rawseg.reference(lists, q, c["idfs"], c["weights"], dlc, rawseg.avgdl_of(dlc))
    inside = [qi for qi, (keyed, _) in enumerate(ref) if _bits(keyed[9][1]) == 0 and _bits(keyed[10][1]) == 0]
    assert set(inside) >= {0, 1, 5}, inside   # K = 10 cuts through the +0.0f tie
    plan = plan_rows(c)
    assert list(plan["users"].values()) == [5] and [x[0] for x in plan["consumers"]] == [0, 1, 3, 4, 5]
    return _declare(c, 4, 20)


# ---- C. other modes of the context --------------------------------------------------------------------------------------------
def three_segments(rows):
    """Segments 0 and 2 are byte-identical (the same list offsets, scores that tie across segments); segment 1's hot list has
    no skip table, so its groups stream.  Every query names lists in all three, its refs interleaved.  Segment 0's key has
    four users, segment 2's three: query 3 names a 900-posting list next to H there.  Query 4 names tiny lists only: its row of
    K = 10 ends in padding."""
    import body_shapes
    rng, dl, H = _base(39)
    a = [H, _tail(rng, _pick(rng, 20)), _tail(rng, _pick(rng, 30)), _tail(rng, np.concatenate([_pick(rng, 5, inside=H[0]), _pick(rng, 5)])), _tail(rng, _pick(rng, 900)),
         _tail(rng, _pick(rng, 2))]
    rng1, dl1, H1 = _base(40)
    b = [H1, _tail(rng1, _pick(rng1, 25)), _tail(rng1, _pick(rng1, 15)), _tail(rng1, _pick(rng1, 3))]
    segments = [(N_DOCS, dl, a), (N_DOCS, dl1, b), (N_DOCS, dl, a)]
    per = [([0, 1], [0, 1], [0, 1]), ([0, 2], [0, 2], [0, 2]), ([3, 0], [0], [3, 0]), ([0], [1, 0], [0, 4]), ([5], [3], [5])]   # the last: 7 hits, a padded row
    q = []
    for g0, g1, g2 in per:   # refs of the three segments interleaved, each segment's in its own order
        refs, left = [], [[(0, li) for li in g0], [(1, li) for li in g1], [(2, li) for li in g2]]
        while any(left):
            refs += [x.pop(0) for x in left if x]
        q.append(refs)
    assert body_shapes.plan_rule([2500, len(a[4][0])], N_DOCS) != "thin"
    idfs = [[1.5 + 0.625 * i for i in range(len(a))], [1.25 + 0.5 * i for i in range(len(b))], [1.5 + 0.625 * i for i in range(len(a))]]
    weights = [[1.0] * len(a), [0.75] * len(b), [1.0] * len(a)]
    c = dict(segments=segments, queries=q, idfs=idfs, weights=weights, no_skips={(1, 0)})
    users = plan_rows(c, 2)["users"]
    assert {key[0]: u for key, u in users.items()} == {0: 4, 2: 3}
    return _declare(c, 8, 28, rows=2) if rows == 2 else _declare(c, 4, 16, rows=1)


def pruning_input():
    """three two-term thin queries and one single-term query on H"""
    rng, dl, H = _base(41)
    lists = [H, _tail(rng, _pick(rng, 20)), _tail(rng, _pick(rng, 30)), _tail(rng, np.concatenate([_pick(rng, 5, inside=H[0]), _pick(rng, 5)]))]
    c = _mk(dl, lists, [[0, 1], [2, 0], [0, 3], [0]])
    assert list(plan_rows(c)["users"].values()) == [4] and list(plan_rows(c, pruning=True)["users"].values()) == [3]
    return c


def fallback_input():
    """test_fallback_when_the_row_cannot_prove_the_result's input from numpy alone: a tail of the 60 best docs of H in the
    first cell, K = 10 — five items fall back"""
    rng, dl, H = _base(21)
    best60 = [d for d, _ in _hot_scores(np.ascontiguousarray(dl, np.uint32), H, 1.5, 0.75) if d < 1024][:60]
    lists = [H, _tail(rng, best60), _tail(rng, _pick(rng, 5))]
    c = _mk(dl, lists, [[0, 1], [1, 0], [0, 1, 2], [0, 2], [0], [2, 0, 1], [0, 1], [0, 2]])
    c = _declare(c, 4, 32)
    want = expected_stats(c, plan_rows(c))
    assert want[2] == 5 and want[3] >= 300, want
    return c


def many_queries(n=4096):
    """n queries that cycle thin, general and single-term shapes over two hot lists and twelve tails: enough for a plan in
    several slices (3000 queries and more, ns_ctx_set_host_threads)"""
    import body_shapes
    rng, dl, H1 = _base(42)
    h2 = np.sort(rng.choice(N_DOCS, size=2000, replace=False)).astype(np.uint32)
    lists = [H1, (h2, rng.integers(1, 9, size=len(h2), dtype=np.uint32))] + [_tail(rng, _pick(rng, 4 + 3 * i)) for i in range(10)] + \
            [_tail(rng, _pick(rng, 700)), _tail(rng, _pick(rng, 60))]
    shapes = [lambda i: [0, 2 + i % 10], lambda i: [12, 13], lambda i: [i % 2], lambda i: [2 + i % 7, 1, 3 + i % 9], lambda i: [12, 2 + i % 10, 13],
              lambda i: [1, 2 + (i // 3) % 10], lambda i: [3 + i % 9, 0]]
    q = [shapes[i % len(shapes)](i) for i in range(n)]
    want = ["thin", "general", "thin", "thin", "general", "thin", "thin"]
    assert [body_shapes.plan_rule([len(lists[li][0]) for li in g], N_DOCS) for g in q[:7]] == want
    c = _mk(dl, lists, q)
    thin = sum(1 for i in range(n) if want[i % 7] == "thin")
    plan = plan_rows(c)
    assert len(plan["users"]) == 2 and len(plan["consumers"]) == thin
    cells = sorted(len(v) for v in plan["cells"].values())
    assert cells == [2, 4]
    return _declare(c, 6, sum(len(plan["cells"][x[4]]) for x in plan["consumers"]))


@contextlib.contextmanager
def _env(**kv):
    """environment variables that ns_ctx_create reads, set for the block (None: unset) and put back after it"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Runner:
    """One ctx over the case's segment(s), skip tables built, term scores forced shared; batch(rows) scores the case's
    queries with ns_ctx_share_rows(rows).  fork=False: the ctx is created with NS_ROW_FORK=0 and has no side stream."""

    def __init__(self, c, fork=True):
        import rawseg
        self.c = c
        with _env(NS_ROW_CELL=c.get("row_cell", ROW_CELL), **({} if fork else {"NS_ROW_FORK": "0"})):
            if "segments" in c:
                self.seg = rawseg.RawSegments(c["segments"])
            else:
                alias = c.get("alias", {})
                assert sorted(alias) == list(range(len(c["lists"]) - len(alias), len(c["lists"])))   # aliases follow the real lists
                self.seg = rawseg.RawSegment(c["n_docs"], c["doc_len"], c["lists"][:len(c["lists"]) - len(alias)])
        L = self.L = self.seg.L
        self.ctx = self.seg.ctx
        if "segments" in c:
            for sid in range(len(c["segments"])):
                self.seg.build_skips(sid, leave_out=[li for s, li in c.get("no_skips", ()) if s == sid])
            self.qd, self.refs = rawseg.descriptors_multi(c["queries"], self.seg.lists, self.seg.offs, c["idfs"], c["weights"])
        else:
            if c.get("skips", True):
                self.seg.build_skips()
            self.offs = list(self.seg.offs) + [self.seg.offs[alias[li]] for li in sorted(alias)]
            self.qd, self.refs = rawseg.descriptors(c["queries"], c["lists"], self.offs, c["idfs"], c["weights"])
        assert L.ns_ctx_share_scores(self.ctx, 2) == 0
        if c.get("split"):
            assert L.ns_set_tuning(self.ctx, 0, 0, c["split"]) == 0
        self.info = None

    def prepare(self, rows, k=None, flags=0):
        import nsbind
        assert self.L.ns_ctx_share_rows(self.ctx, rows) == 0
        return nsbind.prepare_raw(self.ctx, self.qd, self.refs, k or self.c.get("k", 10), flags)

    def batch(self, rows, k=None, flags=0, shared=True):
        """-> (hits, nhits, found, row stats); shared: whether the batch must report NS_INFO_SHARED (None: either).  The
        batch's info stays in self.info."""
        import nsbind
        b = self.prepare(rows, k, flags)
        try:
            self.info = b.info()
            if shared is not None:
                assert bool(int(self.info.flags) & nsbind.NS_INFO_SHARED) == shared
            b.run()
            hits, nhits, found = b.fetch()
            return hits, nhits, found, b.row_stats()
        finally:
            b.close()

    def release(self):
        self.seg.release()


def same_bytes(a, b, what=""):
    assert a[0].tobytes() == b[0].tobytes(), (what, "hits")
    assert a[1].tobytes() == b[1].tobytes(), (what, "nhits")
    assert a[2].tobytes() == b[2].tobytes(), (what, "found")


def restatement(c):
    """the numpy fp32 restatement of the case's queries (rawseg.reference, or reference_multi for a several-segment case),
    of the queries c["ref_queries"] names when it does (the others are then checked against the rows-off run alone)"""
    import rawseg
    if "segments" in c:
        return rawseg.reference_multi(c["segments"], c["queries"], c["idfs"], c["weights"])
    dl = np.ascontiguousarray(c["doc_len"], np.uint32)
    queries = [c["queries"][qi] for qi in c["ref_queries"]] if "ref_queries" in c else c["queries"]
    return rawseg.reference(c["lists"], queries, c["idfs"], c["weights"], dl, rawseg.avgdl_of(dl))


def check_restatement(c, ref, got, k, and_mode=False):
    import rawseg
    if "segments" in c:
        return rawseg.check_results_multi(ref, got[0], got[1], got[2], k, and_mode)
    at = c.get("ref_queries", slice(None))
    rawseg.check_results(ref, got[0][at], got[1][at], got[2][at], k, and_mode)


def run_case(c, rows=1, fork=True, ref=None, keep=None):
    """the case with rows off and on: byte-identical results, the restatement, the stats the case declares -> stats.
    ref: the case's restatement when the caller has it already; keep: a dict that receives the two runs' results."""
    r = Runner(c, fork)
    try:
        off = r.batch(0)
        on = r.batch(rows)
        n_items = int(r.info.n_items)
    finally:
        r.release()
    if keep is not None:
        keep.update(off=off, on=on)
    assert off[3] == (0, 0, 0, 0)
    same_bytes(off, on, c.get("name", ""))
    k = c.get("k", 10)
    if c.get("ref", True):
        check_restatement(c, ref if ref is not None else restatement(c), on, k)
    prod, cons, fallbacks, row_hits = on[3]
    want = c.get("consumers")
    if want is None:
        assert cons > 0 and prod > 0
    else:
        assert cons == want, (cons, want)
        assert (prod > 0) == (want > 0)
    if want == 0:
        assert on[3] == (0, 0, 0, 0)
    for name, got in (("fallbacks", fallbacks), ("row_hits", row_hits)):
        if c.get(name) == "some":
            assert got > 0, name
        elif c.get(name) is not None:
            assert got == c[name], (name, got)
    if c.get("producers") is not None:
        assert prod == c["producers"], (prod, c["producers"])
    if c.get("exact"):
        want4 = expected_stats(c, plan_rows(c, rows))
        assert on[3] == want4, (on[3], want4)
    if c.get("direct") is not None:   # one work item per query next to the producers: the batch is direct and nothing is joined
        assert (n_items == prod + len(c["queries"])) == c["direct"], (n_items, prod, len(c["queries"]))
    return on[3]


def main(out_path):
    """the counting build: every case that names events, the consumer's counters after each"""
    import nsbind
    assert hasattr(nsbind.hip_lib(), "ns_debug_counters"), "not the counting build"
    rep = {}
    for name, fn in CASES.items():
        c = fn()
        if not c.get("events"):
            continue
        nsbind.debug_counters(reset=True)
        stats = run_case(c)
        cnt = nsbind.debug_counters(reset=True)["ns_debug_counters"]
        rep[name] = {"stats": list(stats), "events": {e: cnt[i] for e, i in EVENTS.items()}}
        if c.get("exact"):   # the input says how many docs are looked up and how many of them the hot list holds
            rep[name]["lookups"] = list(expected_lookups(c, plan_rows(c)))
            assert [cnt[28], cnt[29]] == rep[name]["lookups"], (name, cnt[28], cnt[29], rep[name]["lookups"])
            assert cnt[19] == stats[1], (name, cnt[19], stats)
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print("rows reach OK")


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "nextsearch-api_amd"))
    sys.path.insert(0, here)
    main(sys.argv[1])
