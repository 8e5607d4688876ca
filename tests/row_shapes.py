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
(ns_set_tuning's work units per item), fallbacks / row_hits ("some": the stat must be above zero)."""
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
    return dict(n_docs=N_DOCS, doc_len=doc_len, lists=lists, queries=queries, idfs=idfs, weights=weights, **kw)


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


class Runner:
    """One ctx over the case's segment, skip tables built, term scores forced shared; batch(rows) scores the case's queries
    with ns_ctx_share_rows(rows)"""

    def __init__(self, c):
        import rawseg
        self.c = c
        os.environ["NS_ROW_CELL"] = ROW_CELL
        try:
            self.seg = rawseg.RawSegment(c["n_docs"], c["doc_len"], c["lists"])
        finally:
            del os.environ["NS_ROW_CELL"]
        L = self.seg.L
        self.seg.build_skips()
        assert L.ns_ctx_share_scores(self.seg.ctx, 2) == 0
        if c.get("split"):
            assert L.ns_set_tuning(self.seg.ctx, 0, 0, c["split"]) == 0
        self.qd, self.refs = rawseg.descriptors(c["queries"], c["lists"], self.seg.offs, c["idfs"], c["weights"])

    def prepare(self, rows, k=None):
        import nsbind
        assert self.seg.L.ns_ctx_share_rows(self.seg.ctx, rows) == 0
        return nsbind.prepare_raw(self.seg.ctx, self.qd, self.refs, k or self.c.get("k", 10))

    def batch(self, rows, k=None):
        import nsbind
        b = self.prepare(rows, k)
        try:
            assert int(b.info().flags) & nsbind.NS_INFO_SHARED
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


def run_case(c, rows=1):
    """the case with rows off and on: byte-identical results, the restatement, the stats the case declares -> stats"""
    import rawseg
    r = Runner(c)
    try:
        off = r.batch(0)
        on = r.batch(rows)
    finally:
        r.release()
    assert off[3] == (0, 0, 0, 0)
    same_bytes(off, on, c.get("name", ""))
    k = c.get("k", 10)
    if c.get("ref", True):
        ref = rawseg.reference(c["lists"], c["queries"], c["idfs"], c["weights"], np.ascontiguousarray(c["doc_len"], np.uint32),
                               rawseg.avgdl_of(np.ascontiguousarray(c["doc_len"], np.uint32)))
        rawseg.check_results(ref, on[0], on[1], on[2], k)
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
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print("rows reach OK")


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "nextsearch-api_amd"))
    sys.path.insert(0, here)
    main(sys.argv[1])
