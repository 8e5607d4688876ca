"""Python restatement of the pages past the first K, independent of the kernels and of ns_after_plan.hpp.

A row is (rank, pos, doc, seg, bits): `rank` the mapped rank a larger value of which comes first (ord of the fp32 score bits
for the boolean search, t for the search by date), `pos` the position of the segment in the call's list, `bits` what the
call reports for the hit (score bits, or the key as uploaded).  The full order of a query is boolean_ref.boolean_all's, or a
sort over facet_ref's matched sets with sorted_ref.rank_of; a page is that order cut by a plain tuple comparison."""
import numpy as np

import boolean_ref
import facet_ref
import sorted_ref


def ord32(bits):
    """the kernels' order-preserving map of fp32 bits"""
    bits = int(bits) & 0xFFFFFFFF
    return (~bits & 0xFFFFFFFF) if bits & 0x80000000 else (bits | 0x80000000)


def sort_rank(key, ascending):
    """t of the search by date: larger first, key 0 last in both directions"""
    key = int(key) & 0xFFFFFFFF
    if ascending:
        return (~key & 0xFFFFFFFF) if key else 0
    return key


def position(rank, pos, doc):
    """a place in the total order as a tuple that sorts ascending"""
    return (-int(rank), int(pos), int(doc))


def boolean_rows(segments, queries, seg_order, idfs, weights):
    """per query the whole matched set in order, as rows"""
    order = list(range(len(segments))) if seg_order is None else list(seg_order)
    out = []
    for rows in boolean_ref.boolean_all(segments, queries, order, idfs, weights):
        q = []
        for v, s, d in rows:
            bits = int(np.float32(v).view(np.uint32))
            q.append((ord32(bits), order.index(s), int(d), s, bits))
        assert q == sorted(q, key=lambda r: position(*r[:3]))      # the two statements of the order agree
        out.append(q)
    return out


def sorted_rows(segments, queries, keys, and_mode, ascending, seg_order=None):
    order = list(range(len(segments))) if seg_order is None else list(seg_order)
    out = []
    for q in queries:
        rows = []
        for pos, s in enumerate(order):
            numbers = [li for ss, li in q if ss == s]
            if not numbers:
                continue
            for d in facet_ref.matched(segments[s][2], numbers, int(segments[s][0]), and_mode).tolist():
                rows.append((sort_rank(keys[s][d], ascending), pos, int(d), s, int(keys[s][d])))
        rows.sort(key=lambda r: position(*r[:3]))
        by_ref = sorted(rows, key=lambda r: (sorted_ref.rank_of(r[4], ascending), r[1], r[2]))
        assert rows == by_ref                                      # t descending is sorted_ref's order
        out.append(rows)
    return out


def page(rows, cursor, k):
    """rows: one query's full order; cursor: None or (mapped rank, pos, doc) -> (rest, the first K rows strictly after it)"""
    K = min(max(int(k), 1), 100)
    if cursor is None:
        after = list(rows)
    else:
        c = position(*cursor)
        after = [r for r in rows if (-r[0], r[1], r[2]) > c]          # position(rank, pos, doc) of the row, written out
    return len(after), after[:K]
