"""Directed inputs of ns_search_sorted (csrc/ns_sorted.hip) and the code that runs them through the raw C-ABI
against the restatement (tests/sorted_ref.py).  All comparisons are exact, score bits included.

Imported by tests/test_sorted_gpu.py for the product library (tile of 2^17 documents), and run as a program in a child
process that loaded the variants or the counting build with NS_FACET_TILE_DOCS=128: there the 300 documents of the small
family span two whole tiles and a part, and the counting build reports which paths of the three kernels the inputs
reached."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "nextsearch-api_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import facet_shapes  # noqa: E402
import filter_ref  # noqa: E402
import nsbind  # noqa: E402
import sorted_ref  # noqa: E402
from rawseg import RawSegments, descriptors_multi  # noqa: E402

AND, ASC = nsbind.NS_FLAG_AND, nsbind.NS_SORT_ASC
SMALL_TILE, N_DOCS = facet_shapes.SMALL_TILE, facet_shapes.N_DOCS
KS = [1, 10, 63, 64, 65, 100]                 # 64 / 65: the boundary between the kept set's two registers
PATTERNS = ["same", "increasing", "decreasing", "half_undated", "zero_one", "pool5"]
# name -> index of ns_debug_sorted_counters (counting build)
SORTED_EVENTS = {"items": 0, "and_intersections": 1, "single_list_items": 2, "and_early_outs": 3, "chunks_skipped": 4, "chunks_inserted": 5,
                 "rows_joined": 6, "score_found": 7, "score_not_found": 8}


def keys_of(pattern, n_docs, seed=5):
    d = np.arange(n_docs, dtype=np.int64)
    if pattern == "same":
        return np.full(n_docs, 20200101, np.uint32)            # the order is segment / docId alone: every tile edge decides a tie
    if pattern == "increasing":
        return (20000101 + d).astype(np.uint32)                 # the entering set keeps changing (newest first)
    if pattern == "decreasing":
        return (0xFFFFFFFE - d).astype(np.uint32)               # ... never changes after the first chunk; the largest legal key
    if pattern == "half_undated":
        return np.where(d % 2 == 0, 0, 19990000 + (d * 7919) % 1000).astype(np.uint32)
    if pattern == "zero_one":
        return (d % 3 == 0).astype(np.uint32)
    assert pattern == "pool5"
    return np.random.default_rng(seed).choice(np.array([0, 1, 20191231, 20200101, 0xFFFFFFFE], dtype=np.uint32), n_docs)


def small_weights(n_lists):
    """distinct idfs and weights per list, so that a wrong list or a wrong order shows in the score bits"""
    return [[1.0 + 0.37 * i for i in range(n_lists)]], [[1.0 if i % 2 == 0 else 0.6 + 0.05 * i for i in range(n_lists)]]


class Family:
    """uploaded segments + key tables + one call's descriptors; the restatement's matched sets and accumulators are cached"""

    def __init__(self, segments, queries, keys, idfs, weights, seg_order=None):
        self.segments, self.queries, self.keys, self.idfs, self.weights = segments, queries, keys, idfs, weights
        self.order = list(range(len(segments))) if seg_order is None else list(seg_order)
        self.segs = RawSegments(segments)
        self.tables, self.cache = {}, {}
        self.qd, self.refs = descriptors_multi(queries, self.segs.lists, self.segs.offs, idfs, weights)

    def table(self, s):
        if s not in self.tables:
            rc, h = nsbind.dockeys_upload(self.segs.ctx, self.keys[s])
            assert rc == 0, self.segs.err()
            self.tables[s] = h
        return self.tables[s]

    def set_keys(self, keys):
        self.drop_tables()
        self.keys = keys

    def drop_tables(self):
        for h in self.tables.values():
            assert nsbind.dockeys_release(self.segs.ctx, h) == 0
        self.tables = {}

    def check(self, k, flags, label):
        rc, hits, keys, nhits, found, _ = nsbind.search_sorted_raw(self.segs.ctx, self.qd, self.refs, k, flags, self.order,
                                                                   [self.segs.segs[s] for s in self.order], [self.table(s) for s in self.order])
        assert rc == 0, (label, self.segs.err())
        ref = sorted_ref.sorted_hits(self.segments, self.queries, self.keys, k, bool(flags & AND), bool(flags & ASC), self.order, self.idfs,
                                     self.weights, self.cache)
        sorted_ref.check(ref, hits, keys, nhits, found, k, label=(label, "flags", hex(flags)))
        return ref, hits, keys, nhits, found

    def release(self):
        if self.segs.ctx:
            self.drop_tables()
        self.segs.release()


def undated_last(ref):
    """key 0 is last in both directions, and alone only when nothing dated is left"""
    for _, hits in ref:
        ks = [kk for _, _, kk, _ in hits]
        first0 = ks.index(0) if 0 in ks else len(ks)
        assert all(kk == 0 for kk in ks[first0:]), ks


def run_small(tile_expected=None):
    """the 300-document family at the loaded library's tile: lists of 0, 1, 63, 64, 65, 128 and 257 postings (one with a
    posting >= n_docs), queries of 0, 1, 2, 8 and 70 refs (one naming a list twice, AND groups with an empty list and with lists
    that share no document), K = 1 .. 100, both directions, OR and AND, without and with skip tables; then the key patterns"""
    tile = nsbind.facet_tile_docs()
    if tile_expected is not None:
        assert tile == tile_expected, (tile, tile_expected)
    lists = facet_shapes.small_lists()
    segments = [(N_DOCS, (5 + np.arange(N_DOCS) % 41).astype(np.uint32), lists)]
    queries = [[(0, li) for li in q] for q in facet_shapes.SMALL_QUERIES]
    idfs, weights = small_weights(len(lists))
    fam = Family(segments, queries, [keys_of("pool5", N_DOCS)], idfs, weights)
    try:
        assert sorted({int(c) for c in fam.qd["term_count"]}) == [0, 1, 2, 8, 70]
        for with_skips in (False, True):
            if with_skips:
                assert facet_shapes.build_skips(fam.segs, 0) == 4
            for k in KS:
                for flags in (0, ASC, AND, AND | ASC):
                    ref = fam.check(k, flags, ("small", "skips", with_skips))[0]
                    undated_last(ref)
        founds = {f for f, _ in fam.check(100, 0, "small")[0]}
        assert 0 in founds and max(founds) > 100                       # found == 0 and found > K are both in play
        for pattern in PATTERNS[:-1]:
            fam.set_keys([keys_of(pattern, N_DOCS)])
            for k in (10, 65, 100):
                for flags in (0, ASC, AND, AND | ASC):
                    ref = fam.check(k, flags, ("pattern", pattern))[0]
                    undated_last(ref)
                    if pattern == "half_undated":                   # dated documents first, whichever direction
                        for qi, (f, hits) in enumerate(ref):
                            dated = sum(int(fam.keys[0][d]) != 0 for d in fam.cache.get(("matched", qi, 0, bool(flags & AND)), np.zeros(0, np.int64)).tolist())
                            assert [kk != 0 for _, _, kk, _ in hits] == [r < dated for r in range(len(hits))], (qi, dated)
    finally:
        fam.release()
    return tile


def run_counts():
    """found < K, == K, == K + 1 and == 0 around K = 64, 65 and 100, one segment of 300 documents"""
    rng = np.random.default_rng(3)
    sizes = [0, 63, 64, 65, 66, 99, 100, 101]
    lists = []
    for m in sizes:
        d = np.sort(rng.choice(N_DOCS, m, replace=False)).astype(np.uint32)
        lists.append((d, (1 + d % 5).astype(np.uint32)))
    segments = [(N_DOCS, rng.integers(5, 60, N_DOCS).astype(np.uint32), lists)]
    queries = [[(0, li)] for li in range(len(sizes))] + [[(0, 1), (0, 1)], [(0, 0), (0, 6)]]
    idfs, weights = small_weights(len(lists))
    fam = Family(segments, queries, [keys_of("pool5", N_DOCS, seed=9)], idfs, weights)
    try:
        for k in (64, 65, 100):
            for flags in (0, ASC):
                ref = fam.check(k, flags, "counts")[0]
                got = {f - k for f, _ in ref}
                assert {-1, 0, 1} <= got and 0 in {f for f, _ in ref}, (k, got)
    finally:
        fam.release()


def multi_family():
    """facet_shapes' three segments (300, 77, 1000 documents) plus queries that leave a segment without a match"""
    segments, queries = facet_shapes.multi_family()
    queries = queries + [[(0, 2), (2, 3)], [(1, 1), (1, 1), (0, 0)]]
    return segments, queries


def run_multi():
    """three segments of different sizes, seg_ids listed as 2, 0, 1: the position in the list orders, not the id; equal keys
    across the segments, so that the position decides; found equals ns_facet_count's and the scoring path's"""
    segments, queries = multi_family()
    idfs = [[1.0 + 0.5 * i for i in range(len(s[2]))] for s in segments]
    weights = [[1.0 if i % 2 else 0.75 for i in range(len(s[2]))] for s in segments]
    keys = [(20200101 + (np.arange(s[0]) % 50)).astype(np.uint32) for s in segments]           # fifty values, equal across segments
    fam = Family(segments, queries, keys, idfs, weights, seg_order=[2, 0, 1])
    try:
        for with_skips in (False, True):
            if with_skips:
                for s in range(3):
                    facet_shapes.build_skips(fam.segs, s)
            for k in (7, 100):
                for flags in (0, ASC, AND, AND | ASC):
                    ref, hits, _, nhits, found = fam.check(k, flags, ("multi", with_skips))
            # equal keys: within one key value the hits of segment 2 (position 0) come before those of segment 0, then 1
            ref = fam.check(100, 0, "multi order")[0]
            seen = [(kk, [2, 0, 1].index(s)) for s, _, kk, _ in ref[6][1]]
            assert seen == sorted(seen, key=lambda t: (-t[0], t[1])) and len({p for _, p in seen}) > 1
        fam.set_keys([keys_of("pool5", s[0], seed=40 + i) for i, s in enumerate(segments)])
        for flags in (0, AND | ASC):
            fam.check(65, flags, "multi pool5")
        # the yardsticks of found: ns_facet_count and the scoring path
        handles = [nsbind.facet_upload(fam.segs.ctx, np.zeros(s[0], np.uint16), 1)[1] for s in segments]
        try:
            for flags in (0, AND):
                _, _, scored, _ = fam.segs.run(fam.qd, fam.refs, 10, flags)
                rc, _, f_found, _ = nsbind.facet_count(fam.segs.ctx, fam.qd, fam.refs, flags, [0, 1, 2], fam.segs.segs, handles, 1)
                assert rc == 0
                found = fam.check(10, flags, "multi found")[4]
                np.testing.assert_array_equal(found, scored.astype(np.uint64))
                np.testing.assert_array_equal(found, f_found)
        finally:
            for h in handles:
                nsbind.facet_release(fam.segs.ctx, h)
    finally:
        fam.release()


def run_product_tile():
    """the product build's tile: n_docs = two tiles + 5, lists that straddle the tile edges (facet_shapes.run_product_tile's)"""
    tile = nsbind.facet_tile_docs()
    n = 2 * tile + 5
    rng = np.random.default_rng(31)
    edges = np.array([0, tile - 1, tile, 2 * tile - 1, 2 * tile, n - 1])
    docs = [np.concatenate([np.arange(tile - 100, tile + 100), np.arange(2 * tile - 50, n)]),
            np.union1d(rng.choice(n, 300, replace=False), edges),
            np.arange(0, n, 997),
            np.arange(tile - 3, tile + 3)]
    lists = [(d.astype(np.uint32), (1 + d % 3).astype(np.uint32)) for d in docs]
    segments = [(n, (5 + np.arange(n) % 50).astype(np.uint32), lists)]
    queries = [[(0, li) for li in q] for q in ([0], [1], [2], [3], [0, 1], [1, 2], [0, 2], [0, 1, 2], [3, 1], [2, 2], [3, 0])]
    idfs, weights = small_weights(len(lists))
    fam = Family(segments, queries, [keys_of("same", n)], idfs, weights)
    try:
        for with_skips in (False, True):
            if with_skips:
                assert facet_shapes.build_skips(fam.segs, 0) == 3
            for pattern in ("same", "pool5"):
                fam.set_keys([keys_of(pattern, n)])
                for k, flags in ((100, 0), (65, ASC), (64, AND), (100, AND | ASC)):
                    fam.check(k, flags, ("product tile", tile, pattern, with_skips))
    finally:
        fam.release()
    return tile, n


def run_filtered():
    """on filtered copies (ns_segment_filter) of the small segment with the SOURCE's key table: equal to the restatement over
    the kept documents, score bits unchanged (the copy has its own norms, equal to the source's)"""
    lists = facet_shapes.small_lists()
    doc_len = (5 + np.arange(N_DOCS) % 41).astype(np.uint32)
    segments = [(N_DOCS, doc_len, lists)]
    queries = [[(0, li) for li in q] for q in facet_shapes.SMALL_QUERIES]
    idfs, weights = small_weights(len(lists))
    keys = [keys_of("pool5", N_DOCS)]
    segs = RawSegments(segments)
    copies = []
    rc, table = nsbind.dockeys_upload(segs.ctx, keys[0])
    assert rc == 0, segs.err()
    try:
        counts = np.array([len(d) for d, _ in lists], dtype=np.uint32)
        keeps = {"alternating": np.arange(N_DOCS) % 2 == 0, "first tile": np.arange(N_DOCS) < SMALL_TILE}
        new_id = 1
        for name, keep in keeps.items():
            masked = [(np.asarray(d, np.uint32), np.asarray(t, np.uint32)) for d, t in filter_ref.mask_lists(lists, keep)]
            msegments = [(N_DOCS, doc_len, masked)]
            cache = {}
            for with_skips in (False, True):
                h, noff, ncnt, _, _, _ = nsbind.segment_filter(segs.ctx, segs.segs[0], new_id, filter_ref.bits_of(keep), segs.offs[0], counts)
                copies.append(h)
                if with_skips:
                    which = np.flatnonzero(ncnt >= 32)
                    bo, cn = np.ascontiguousarray(noff[which]), np.ascontiguousarray(ncnt[which])
                    assert len(which) and segs.L.ns_segment_build_skips(segs.ctx, h, bo.ctypes.data, cn.ctypes.data, len(which)) == 0, segs.err()
                qd = np.zeros(len(queries), dtype=nsbind.QDESC_DTYPE)
                refs = []
                for qi, q in enumerate(queries):
                    qd[qi] = (len(refs), len(q))
                    refs += [(new_id, int(ncnt[li]), int(noff[li]), idfs[0][li], weights[0][li]) for _, li in q]
                refs = np.array(refs, dtype=nsbind.TERM_DTYPE)
                for k, flags in ((100, 0), (10, ASC), (65, AND), (100, AND | ASC)):
                    rc, hits, kk, nhits, found, _ = nsbind.search_sorted_raw(segs.ctx, qd, refs, k, flags, [new_id], [h], [table])
                    assert rc == 0, segs.err()
                    ref = sorted_ref.sorted_hits(msegments, queries, keys, k, bool(flags & AND), bool(flags & ASC), None, idfs, weights, cache)
                    sorted_ref.check(ref, hits, kk, nhits, found, k, label=("filtered", name, with_skips, hex(flags)), ids={0: new_id})
                new_id += 1
    finally:
        for h in copies:
            segs.L.ns_segment_release(segs.ctx, h)
        nsbind.dockeys_release(segs.ctx, table)
        segs.release()


def main(out_path):
    """child process: the small family at NS_FACET_TILE_DOCS = 128, then the other families at that tile; with the counting
    build, the counters of the small family alone"""
    counting = "ns_debug_sorted_counters" in nsbind.debug_counters(reset=True)
    rep = {"tile": run_small(tile_expected=SMALL_TILE), "counting": counting}
    if counting:
        c = nsbind.debug_counters(reset=True)["ns_debug_sorted_counters"]
        rep["events"] = {e: c[i] for e, i in SORTED_EVENTS.items()}
        rep["missed"] = [e for e in SORTED_EVENTS if rep["events"][e] == 0]
        print("sorted", rep["events"], flush=True)
    run_counts()
    run_multi()
    run_filtered()
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print("sorted shapes OK")


if __name__ == "__main__":
    main(sys.argv[1])
