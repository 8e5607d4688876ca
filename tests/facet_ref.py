"""Numpy restatement of facet counts, independent of the kernels.

Per query and segment: the union (OR) or the intersection (AND) of the docId sets of the lists the query names in that
segment, restricted to docId < n_docs; then np.bincount of the segment's bucket table over that set; summed over the
segments.  A list named twice changes nothing (sets); a query without refs counts nothing."""
import numpy as np


def matched(lists, numbers, n_docs, and_mode):
    """the docIds (ascending, distinct, < n_docs) that the lists `numbers` of one segment match"""
    sets = []
    for li in numbers:
        d = np.asarray(lists[li][0], dtype=np.int64)
        sets.append(np.unique(d[d < n_docs]))
    if not sets:
        return np.zeros(0, np.int64)
    out = sets[0]
    for s in sets[1:]:
        out = np.intersect1d(out, s) if and_mode else np.union1d(out, s)
    return out


def counts(segments, queries, tables, n_buckets, and_mode):
    """segments: (n_docs, doc_len, lists) each, as tests/rawseg.py's; queries: lists of (segment, list number); tables: one
    bucket array per segment -> int64 counts[Q][n_buckets]"""
    out = np.zeros((len(queries), n_buckets), dtype=np.int64)
    for qi, q in enumerate(queries):
        for s in sorted({s for s, _ in q}):
            n_docs, _, lists = segments[s]
            docs = matched(lists, [li for ss, li in q if ss == s], int(n_docs), and_mode)
            out[qi] += np.bincount(np.asarray(tables[s], dtype=np.int64)[docs], minlength=n_buckets)
    return out
