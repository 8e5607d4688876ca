"""Numpy / Python restatement of facet counts and date order for boolean queries, independent of the kernels.
Nothing is restated that another restatement already says:

    the matched set of a (query, segment) group      boolean_ref.group_matched
    the score of a matched document                  boolean_ref.group_scores (through boolean_ref.boolean_all)
    the counts                                       np.bincount of the segment's bucket table over the set, summed over segments
    the order                                        sorted_ref.resort / sorted_ref.rank_of
    a page                                           after_ref.page

A query is a list of (segment, list number, role) in query order, as in boolean_ref."""
import numpy as np

import after_ref
import boolean_ref
import sorted_ref


def matched(segments, query, seg_order=None):
    """-> [(position, segment, sorted int64 docIds)] of one query, a group per listed segment the query has a ref in"""
    order = list(range(len(segments))) if seg_order is None else list(seg_order)
    out = []
    for pos, s in enumerate(order):
        refs = [(li, r) for ss, li, r in query if ss == s]
        if refs:
            out.append((pos, s, boolean_ref.group_matched(segments[s][2], refs, int(segments[s][0]))))
    return out


def counts(segments, queries, tables, n_buckets, seg_order=None):
    """tables: one bucket array per segment -> int64 counts[Q][n_buckets]"""
    out = np.zeros((len(queries), n_buckets), dtype=np.int64)
    for qi, q in enumerate(queries):
        for _, s, docs in matched(segments, q, seg_order):
            out[qi] += np.bincount(np.asarray(tables[s], dtype=np.int64)[docs], minlength=n_buckets)
    return out


def rows(everything, keys, ascending, seg_order):
    """everything: boolean_ref.boolean_all's answer (per query the whole matched set as (score, segment, doc)); keys: one uint32
    array per segment -> per query the whole set in date order as after_ref rows with the score bits as a sixth field:
    (mapped rank, position, doc, segment, key as uploaded, score bits)"""
    order = list(seg_order)
    out = []
    for triples in everything:
        q = []
        for v, s, d in sorted_ref.resort(triples, lambda s, d: keys[s][d], order.index, ascending):
            key = int(keys[s][d])
            q.append((after_ref.sort_rank(key, ascending), order.index(s), int(d), s, key, int(np.float32(v).view(np.uint32))))
        assert q == sorted(q, key=lambda r: after_ref.position(*r[:3]))      # the two statements of the order agree
        out.append(q)
    return out


def page(query_rows, cursor, k, ascending, seg_order):
    """cursor: None or (key as uploaded, seg_id, doc) -> (rest, the first K rows strictly after it)"""
    c = None if cursor is None else (after_ref.sort_rank(cursor[0], ascending), list(seg_order).index(cursor[1]), cursor[2])
    return after_ref.page(query_rows, c, k)
