"""Directed inputs of ns_facet_count (csrc/ns_facet.hip) and the code that runs them through the raw C-ABI
against the numpy restatement (tests/facet_ref.py).  All comparisons are exact.

Imported by tests/test_facet_gpu.py for the product library (tile of 2^17 documents), and run as a program in a child
process that loaded the variants or the counting build with NS_FACET_TILE_DOCS=128: there the 300 documents of the small
family span two whole tiles and a part, and the counting build reports which paths of k_fc_count the inputs reached."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "nextsearch-api_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import facet_ref  # noqa: E402
import filter_ref  # noqa: E402
import nsbind  # noqa: E402
from rawseg import RawSegments, descriptors_multi  # noqa: E402

AND = nsbind.NS_FLAG_AND
NS_E_INVAL = -1
SMALL_TILE = 128
N_DOCS = 300                                  # 9 whole bitmap words and 12 bits of a tenth; two whole small tiles and a part
SPECIAL = [0, 127, 128, 255, 256, 299]        # each named by exactly one list
BUCKETS = [1, 7, 1024]
TABLE_KINDS = ["zeros", "modulo", "tile"]
# name -> index of ns_debug_facet_counters (counting build)
FACET_EVENTS = {"items": 0, "and_intersections": 1, "single_list_items": 2, "skip_cuts": 3, "search_cuts": 4, "skip_cell_searches": 5,
                "and_early_outs": 6, "flushed_entries": 7}
REACHED = ["and_intersections", "single_list_items", "skip_cuts", "search_cuts"]   # what the small family is built to reach


def small_lists():
    """Lists of 0, 1, 63, 64, 65, 128 and 257 postings; list 7 lies in the middle tile alone, list 8 has nothing there; list
    6 ends with docId 305 >= n_docs."""
    rng = np.random.default_rng(11)
    pool = np.setdiff1d(np.arange(N_DOCS), SPECIAL)

    def pick(n, among=pool, extra=()):
        return np.sort(np.concatenate([rng.choice(among, n, replace=False), np.array(extra, dtype=np.int64)])).astype(np.uint32)

    mid = pool[(pool >= SMALL_TILE) & (pool < 2 * SMALL_TILE)]
    rim = pool[(pool < SMALL_TILE) | (pool >= 2 * SMALL_TILE)]
    docs = [np.zeros(0, np.uint32), np.array([0], np.uint32), pick(62, extra=[127]), pick(63, extra=[128]), pick(64, extra=[255]),
            pick(127, extra=[256]), pick(255, extra=[299, 305]), pick(40, mid), pick(50, rim)]
    assert [len(d) for d in docs] == [0, 1, 63, 64, 65, 128, 257, 40, 50]
    for d in SPECIAL:
        assert sum(int(d in set(x.tolist())) for x in docs) == 1
    return [(d, (1 + d % 3).astype(np.uint32)) for d in docs]


# queries of 0, 1, 2, 8 and 70 refs; [7, 8] is empty under AND, [0, 5] names the empty list, [4, 4] one list twice
SMALL_QUERIES = [[], [6], [1], [0], [7], [2, 3], [7, 8], [5, 6], [0, 5], [4, 4], list(range(1, 9)), [2 + i % 7 for i in range(70)]]


def table_of(kind, n_docs, n_buckets, tile):
    d = np.arange(n_docs, dtype=np.int64)
    if kind == "zeros":
        return np.zeros(n_docs, np.uint16)
    if kind == "modulo":
        return (d % n_buckets).astype(np.uint16)
    return ((d // tile) % n_buckets).astype(np.uint16)        # every document of a tile shares a bucket


def build_skips(segs, sid, min_count=64):
    """skip tables for the lists of segment sid with at least min_count postings (the engine's rule for small segments)"""
    counts = np.array([len(d) for d, _ in segs.lists[sid]], dtype=np.uint32)
    which = np.flatnonzero(counts >= min_count)
    bo, cn = np.ascontiguousarray(segs.offs[sid][which]), np.ascontiguousarray(counts[which])
    assert segs.L.ns_segment_build_skips(segs.ctx, segs.segs[sid], bo.ctypes.data, cn.ctypes.data, len(which)) == 0, segs.err()
    return len(which)


_REFERENCE = {}   # computed once, shared, never changed


def reference(key, segments, queries, tables, n_buckets, and_mode):
    key = (key, n_buckets, and_mode)
    if key not in _REFERENCE:
        _REFERENCE[key] = facet_ref.counts(segments, queries, tables, n_buckets, and_mode)
    return _REFERENCE[key]


def check_counts(label, segs, segments, queries, qd, refs, tables, n_buckets, seg_order=None, key=None):
    """uploads the tables, runs OR and AND, compares counts and found with the restatement; releases the tables"""
    order = list(range(len(segments))) if seg_order is None else seg_order
    handles = []
    try:
        for s in order:
            rc, h = nsbind.facet_upload(segs.ctx, tables[s], n_buckets)
            assert rc == 0, segs.err()
            handles.append(h)
        for flags in (0, AND):
            rc, counts, found, ms = nsbind.facet_count(segs.ctx, qd, refs, flags, order, [segs.segs[s] for s in order], handles, n_buckets)
            assert rc == 0, (label, segs.err())
            want = reference(key or label, segments, queries, tables, n_buckets, bool(flags))
            what = (label, "B", n_buckets, "AND" if flags else "OR")
            np.testing.assert_array_equal(counts.astype(np.int64), want, err_msg=str(what))
            np.testing.assert_array_equal(found.astype(np.int64), want.sum(axis=1), err_msg=str(what + ("found",)))
    finally:
        for h in handles:
            assert nsbind.facet_release(segs.ctx, h) == 0


def run_small(tile_expected=None):
    """the 300-document family at the loaded library's tile: B = 1, 7, 1024 x three tables, OR and AND, first without skip
    tables, then with them on the lists of >= 64 postings"""
    tile = nsbind.facet_tile_docs()
    if tile_expected is not None:
        assert tile == tile_expected, (tile, tile_expected)
    lists = small_lists()
    segments = [(N_DOCS, np.full(N_DOCS, 9, np.uint32), lists)]
    queries = [[(0, li) for li in q] for q in SMALL_QUERIES]
    segs = RawSegments(segments)
    try:
        idfs, weights = [[1.0] * len(lists)], [[1.0] * len(lists)]
        qd, refs = descriptors_multi(queries, segs.lists, segs.offs, idfs, weights)
        assert sorted({int(c) for c in qd["term_count"]}) == [0, 1, 2, 8, 70]
        for with_skips in (False, True):
            if with_skips:
                assert build_skips(segs, 0) == 4
            for B in BUCKETS:
                for kind in TABLE_KINDS:
                    check_counts(("small", kind), segs, segments, queries, qd, refs, [table_of(kind, N_DOCS, B, SMALL_TILE)], B)
    finally:
        segs.release()
    return tile


def run_product_tile():
    """the product build's tile: n_docs = two tiles + 5, sparse lists of a few hundred postings that straddle the tile edges"""
    tile = nsbind.facet_tile_docs()
    n = 2 * tile + 5
    rng = np.random.default_rng(31)
    edges = np.array([0, tile - 1, tile, 2 * tile - 1, 2 * tile, n - 1])
    docs = [np.concatenate([np.arange(tile - 100, tile + 100), np.arange(2 * tile - 50, n)]),
            np.union1d(rng.choice(n, 300, replace=False), edges),
            np.arange(0, n, 997),
            np.arange(tile - 3, tile + 3)]
    lists = [(d.astype(np.uint32), np.ones(len(d), np.uint32)) for d in docs]
    segments = [(n, np.full(n, 9, np.uint32), lists)]
    queries = [[(0, li) for li in q] for q in ([0], [1], [2], [3], [0, 1], [1, 2], [0, 2], [0, 1, 2], [3, 1], [2, 2], [3, 0])]
    segs = RawSegments(segments)
    try:
        one = [[1.0] * len(lists)]
        qd, refs = descriptors_multi(queries, segs.lists, segs.offs, one, one)
        d = np.arange(n, dtype=np.int64)
        tables = {7: (d % 7).astype(np.uint16), 1024: (d // tile).astype(np.uint16), 50: ((d * 7919) % 50).astype(np.uint16)}
        for with_skips in (False, True):
            if with_skips:
                assert build_skips(segs, 0) == 3
            for B, table in tables.items():
                check_counts(("product tile", tile), segs, segments, queries, qd, refs, [table], B)
    finally:
        segs.release()
    return tile, n


def multi_family():
    """three segments of 300, 77 and 1000 documents, every docId in range"""
    rng = np.random.default_rng(23)
    segments = []
    for n, sizes in ((300, [120, 64, 9, 200]), (77, [30, 77, 5]), (1000, [400, 129, 700, 1])):
        lists = []
        for m in sizes:
            d = np.sort(rng.choice(n, m, replace=False)).astype(np.uint32)
            lists.append((d, (1 + d % 4).astype(np.uint32)))
        segments.append((n, rng.integers(5, 60, n).astype(np.uint32), lists))
    queries = [[(0, 0), (1, 0), (2, 0)], [(1, 1)], [(1, 0), (1, 2)], [(0, 1), (0, 3), (2, 1), (2, 2)], [(2, 3), (0, 2)], [],
               [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (2, 3)], [(2, 2), (2, 2), (0, 3)]]
    return segments, queries


def run_multi():
    """counts sum over segments of different n_docs; seg_ids given as 2, 0, 1; found equals the scoring path's, OR and AND"""
    tile = nsbind.facet_tile_docs()
    segments, queries = multi_family()
    segs = RawSegments(segments)
    try:
        idfs = [[1.0 + 0.5 * i for i in range(len(s[2]))] for s in segments]
        weights = [[1.0] * len(s[2]) for s in segments]
        qd, refs = descriptors_multi(queries, segs.lists, segs.offs, idfs, weights)
        for with_skips in (False, True):
            if with_skips:
                for s in range(3):
                    build_skips(segs, s)
            for B, kind in ((7, "modulo"), (1024, "modulo"), (3, "tile")):
                tables = [table_of(kind, s[0], B, SMALL_TILE) for s in segments]
                check_counts(("multi", kind), segs, segments, queries, qd, refs, tables, B, seg_order=[2, 0, 1])
        # the existing scoring path is the yardstick of `found`
        B = 7
        tables = [table_of("modulo", s[0], B, SMALL_TILE) for s in segments]
        handles = [nsbind.facet_upload(segs.ctx, t, B)[1] for t in tables]
        try:
            for flags in (0, AND):
                _, _, scored, _ = segs.run(qd, refs, 10, flags)
                rc, counts, found, _ = nsbind.facet_count(segs.ctx, qd, refs, flags, [0, 1, 2], segs.segs, handles, B)
                assert rc == 0, segs.err()
                np.testing.assert_array_equal(found, scored.astype(np.uint64), err_msg="found of the scoring path, flags %d" % flags)
                np.testing.assert_array_equal(counts.sum(axis=1, dtype=np.uint64), found)
        finally:
            for h in handles:
                nsbind.facet_release(segs.ctx, h)
    finally:
        segs.release()
    return tile


def run_filtered():
    """on filtered copies (ns_segment_filter) of the small segment: the alternating keep and "first small tile only"; counts
    equal the restatement over the masked lists, with skip tables on the copy and without"""
    lists = small_lists()
    segments = [(N_DOCS, np.full(N_DOCS, 9, np.uint32), lists)]
    queries = [[(0, li) for li in q] for q in SMALL_QUERIES]
    segs = RawSegments(segments)
    copies = []
    try:
        counts = np.array([len(d) for d, _ in lists], dtype=np.uint32)
        keeps = {"alternating": np.arange(N_DOCS) % 2 == 0, "first tile": np.arange(N_DOCS) < SMALL_TILE}
        new_id = 1
        for name, keep in keeps.items():
            masked = filter_ref.mask_lists(lists, keep)
            msegments = [(N_DOCS, segments[0][1], masked)]
            for with_skips in (False, True):
                h, noff, ncnt, kept, _, _ = nsbind.segment_filter(segs.ctx, segs.segs[0], new_id, filter_ref.bits_of(keep), segs.offs[0], counts)
                copies.append(h)
                assert [int(c) for c in ncnt] == [len(d) for d, _ in masked]
                if with_skips:
                    which = np.flatnonzero(ncnt >= 32)
                    bo, cn = np.ascontiguousarray(noff[which]), np.ascontiguousarray(ncnt[which])
                    assert len(which) and segs.L.ns_segment_build_skips(segs.ctx, h, bo.ctypes.data, cn.ctypes.data, len(which)) == 0, segs.err()
                qd = np.zeros(len(queries), dtype=nsbind.QDESC_DTYPE)
                refs = []
                for qi, q in enumerate(queries):
                    qd[qi] = (len(refs), len(q))
                    refs += [(new_id, int(ncnt[li]), int(noff[li]), 1.0, 1.0) for _, li in q]
                refs = np.array(refs, dtype=nsbind.TERM_DTYPE)
                for B, kind in ((7, "modulo"), (1024, "tile")):
                    table = table_of(kind, N_DOCS, B, SMALL_TILE)          # the source's table serves the copy
                    rc, t = nsbind.facet_upload(segs.ctx, table, B)
                    assert rc == 0, segs.err()
                    try:
                        for flags in (0, AND):
                            rc, got, found, _ = nsbind.facet_count(segs.ctx, qd, refs, flags, [new_id], [h], [t], B)
                            assert rc == 0, segs.err()
                            want = reference(("filtered", name, kind), msegments, queries, [table], B, bool(flags))
                            np.testing.assert_array_equal(got.astype(np.int64), want, err_msg=str((name, with_skips, B, flags)))
                            np.testing.assert_array_equal(found.astype(np.int64), want.sum(axis=1))
                    finally:
                        nsbind.facet_release(segs.ctx, t)
                new_id += 1
    finally:
        for h in copies:
            segs.L.ns_segment_release(segs.ctx, h)
        segs.release()


def main(out_path):
    """child process: the small family at NS_FACET_TILE_DOCS = 128, then the other families at that tile; with the counting
    build, the counters of the small family alone"""
    counting = "ns_debug_facet_counters" in nsbind.debug_counters(reset=True)
    rep = {"tile": run_small(tile_expected=SMALL_TILE), "counting": counting}
    if counting:
        c = nsbind.debug_counters(reset=True)["ns_debug_facet_counters"]
        rep["events"] = {e: c[i] for e, i in FACET_EVENTS.items()}
        rep["missed"] = [e for e in REACHED if rep["events"][e] == 0]
        print("facet", rep["events"], flush=True)
    run_multi()
    run_filtered()
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print("facet shapes OK")


if __name__ == "__main__":
    main(sys.argv[1])
