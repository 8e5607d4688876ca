"""Numpy / Python restatement of any-of groups in boolean queries, independent of the kernels and of the planner.

A query is a list of (segment, list number, role, clause) in query order; `clause` is any value in [0, 65535] and is read
under MUST alone.  Per (query, segment) group, over the refs the query has in that segment: the MUST refs of equal clause
value form one clause; its refs with count == 0 are dropped (count: the postings of the list as the ref names it, those with
docId >= n_docs included), and a clause ALL of whose refs have count == 0 kills the group.  S = the SHOULD refs with
count > 0, X = the NOT refs with count > 0.  At least one clause: the documents in at least one list of EVERY clause and in no
list of X; no clause, S not empty: the union of S without the union of X; otherwise nothing.  Only docId < n_docs counts.

Nothing is restated that another restatement already says: the score is boolean_ref.group_scores (every MUST and SHOULD ref in
query order, a list named twice added twice; a clause member that does not hold the document adds nothing), the order
boolean_ref.boolean_all's sort, the counts np.bincount, date order and pages boolean_sets_ref.rows / .page, after_ref.page."""
import numpy as np

import after_ref
import boolean_ref
from boolean_ref import MUST, NOT, SHOULD


def strip(queries):
    """the queries without their clause values: boolean_ref's form"""
    return [[(s, li, r) for s, li, r, _ in q] for q in queries]


def group_matched(lists, refs, n_docs):
    """refs: [(list number, role, clause)] of one group -> sorted int64 docIds of its matched set"""
    none = np.zeros(0, np.int64)

    def inside(li):
        d = np.asarray(lists[li][0], dtype=np.int64)
        return np.unique(d[d < n_docs])

    clauses = {}                                   # clause value -> the lists of its refs with count > 0
    for li, r, c in refs:
        if r == MUST:
            clauses.setdefault(int(c), [])
            if len(lists[li][0]) > 0:
                clauses[int(c)].append(li)
    if any(not members for members in clauses.values()):
        return none
    should = [li for li, r, _ in refs if r == SHOULD and len(lists[li][0]) > 0]
    excluded = [li for li, r, _ in refs if r == NOT and len(lists[li][0]) > 0]
    if clauses:
        docs = None
        for members in clauses.values():
            union = none
            for li in members:
                union = np.union1d(union, inside(li))
            docs = union if docs is None else np.intersect1d(docs, union)
    elif should:
        docs = none
        for li in should:
            docs = np.union1d(docs, inside(li))
    else:
        return none
    for li in excluded:
        docs = np.setdiff1d(docs, inside(li))
    return docs.astype(np.int64)


def matched(segments, query, seg_order=None):
    """-> [(position, segment, sorted int64 docIds)] of one query, a group per listed segment the query has a ref in"""
    order = list(range(len(segments))) if seg_order is None else list(seg_order)
    out = []
    for pos, s in enumerate(order):
        refs = [(li, r, c) for ss, li, r, c in query if ss == s]
        if refs:
            out.append((pos, s, group_matched(segments[s][2], refs, int(segments[s][0]))))
    return out


def grouped_all(segments, queries, seg_order=None, idfs=None, weights=None):
    """-> per query the whole matched set as (score fp32, segment, doc) in the canonical order"""
    out = []
    for q in queries:
        rows = []
        for pos, s, docs in matched(segments, q, seg_order):
            if not len(docs):
                continue
            acc = boolean_ref.group_scores(segments[s], [(li, r) for ss, li, r, _ in q if ss == s], idfs[s], weights[s])
            rows += [(np.float32(acc[d]), pos, d, s) for d in docs.tolist()]
        rows.sort(key=lambda t: (-float(t[0]), t[1], t[2]))
        out.append([(v, s, d) for v, _, d, s in rows])
    return out


def hits(everything, k):
    """grouped_all's answer -> per query (found, the first K = clamp(k, 1, 100)): what boolean_ref.check compares with"""
    K = min(max(int(k), 1), 100)
    return [(len(rows), rows[:K]) for rows in everything]


def score_rows(everything, seg_order):
    """grouped_all's answer -> per query the whole set in score order as after_ref rows (mapped rank, position, doc, segment, bits)"""
    order = list(seg_order)
    out = []
    for rows in everything:
        q = []
        for v, s, d in rows:
            bits = int(np.float32(v).view(np.uint32))
            q.append((after_ref.ord32(bits), order.index(s), int(d), s, bits))
        assert q == sorted(q, key=lambda r: after_ref.position(*r[:3]))      # the two statements of the order agree
        out.append(q)
    return out


def counts(segments, queries, tables, n_buckets, seg_order=None):
    """tables: one bucket array per segment -> int64 counts[Q][n_buckets]"""
    out = np.zeros((len(queries), n_buckets), dtype=np.int64)
    for qi, q in enumerate(queries):
        for _, s, docs in matched(segments, q, seg_order):
            out[qi] += np.bincount(np.asarray(tables[s], dtype=np.int64)[docs], minlength=n_buckets)
    return out
