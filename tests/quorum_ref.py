"""Numpy / Python restatement of at-least-m-of-n clauses in boolean queries, independent of the kernels and of the
planner.  It restates the MATCHED SET only.

A query is a list of (segment, list number, role, clause, need) in query order; `clause` and `need` are read under MUST alone,
need 0 reads as 1.  Per (query, segment) group, over the refs the query has in that segment: the MUST refs of equal clause value
form one clause, and they carry one need m.  Its refs with count == 0 are dropped; a list named twice counts once.  The clause
holds for a document that lies in at least m of its DISTINCT lists; a clause with fewer than m distinct lists left kills the
group.  Every clause must hold and no NOT list may; without a clause the SHOULD lists' union decides (grouped_ref's rule).  Only
docId < n_docs counts.

Nothing is restated that another restatement already says: the score is boolean_ref.group_scores over every MUST and SHOULD ref
in query order, the order boolean_ref's sort, found / hits / score rows grouped_ref.hits / .score_rows, the counts np.bincount,
date order and pages boolean_sets_ref.rows / .page and after_ref.page over the answer of quorum_all."""
import numpy as np

import boolean_ref
import grouped_ref
from boolean_ref import MUST, NOT, SHOULD

MAX_NEED = 7

hits = grouped_ref.hits
score_rows = grouped_ref.score_rows


def strip(queries):
    """the queries without their needs: grouped_ref's form"""
    return [[(s, li, r, c) for s, li, r, c, _ in q] for q in queries]


def group_matched(lists, refs, n_docs):
    """refs: [(list number, role, clause, need)] of one group -> sorted int64 docIds of its matched set"""
    none = np.zeros(0, np.int64)
    clauses = {}                                   # clause value -> [need, the distinct lists of its refs with count > 0]
    for li, r, c, m in refs:
        if r != MUST:
            continue
        need = max(int(m), 1)
        assert need <= MAX_NEED
        entry = clauses.setdefault(int(c), [need, []])
        assert entry[0] == need, "the refs of one clause carry one need"
        if len(lists[li][0]) > 0 and li not in entry[1]:
            entry[1].append(li)
    if any(len(members) < need for need, members in clauses.values()):
        return none
    if not clauses:
        return grouped_ref.group_matched(lists, [(li, r, c) for li, r, c, _ in refs], n_docs)
    ok = np.ones(n_docs, bool)
    for need, members in clauses.values():
        count = np.zeros(n_docs, np.int64)
        for li in members:
            d = np.asarray(lists[li][0], dtype=np.int64)
            count[np.unique(d[d < n_docs])] += 1
        ok &= count >= need
    for li, r, _, _ in refs:
        if r == NOT and len(lists[li][0]) > 0:
            d = np.asarray(lists[li][0], dtype=np.int64)
            ok[d[d < n_docs]] = False
    return np.flatnonzero(ok).astype(np.int64)


def matched(segments, query, seg_order=None):
    """-> [(position, segment, sorted int64 docIds)] of one query, a group per listed segment the query has a ref in"""
    order = list(range(len(segments))) if seg_order is None else list(seg_order)
    out = []
    for pos, s in enumerate(order):
        refs = [(li, r, c, m) for ss, li, r, c, m in query if ss == s]
        if refs:
            out.append((pos, s, group_matched(segments[s][2], refs, int(segments[s][0]))))
    return out


def quorum_all(segments, queries, seg_order=None, idfs=None, weights=None):
    """-> per query the whole matched set as (score fp32, segment, doc) in the canonical order (grouped_ref.grouped_all's form)"""
    out = []
    for q in queries:
        rows = []
        for pos, s, docs in matched(segments, q, seg_order):
            if not len(docs):
                continue
            acc = boolean_ref.group_scores(segments[s], [(li, r) for ss, li, r, _, _ in q if ss == s], idfs[s], weights[s])
            rows += [(np.float32(acc[d]), pos, d, s) for d in docs.tolist()]
        rows.sort(key=lambda t: (-float(t[0]), t[1], t[2]))
        out.append([(v, s, d) for v, _, d, s in rows])
    return out


def counts(segments, queries, tables, n_buckets, seg_order=None):
    """tables: one bucket array per segment -> int64 counts[Q][n_buckets]"""
    out = np.zeros((len(queries), n_buckets), dtype=np.int64)
    for qi, q in enumerate(queries):
        for _, s, docs in matched(segments, q, seg_order):
            out[qi] += np.bincount(np.asarray(tables[s], dtype=np.int64)[docs], minlength=n_buckets)
    return out
