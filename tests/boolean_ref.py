"""Numpy / Python restatement of the boolean search, independent of the kernels.

A query is a list of (segment, list number, role) in query order.  Per (query, segment) group, over the refs the query has in
that segment: M = its MUST refs, S = its SHOULD refs with count > 0, X = its NOT refs with count > 0 (count: the postings of
the list as the ref names it, those with docId >= n_docs included).  A MUST ref with count == 0 kills the group.  M not
empty: the intersection of M without the union of X; M empty, S not: the union of S without the union of X; otherwise
nothing.  Only docId < n_docs counts.  The score is rawseg's fp32 restatement accumulator (_np_bm25: +0.0f start, query-term
order, a list named twice added twice) over the group's refs that are not NOT.  The order is a Python sort on (score
descending as floats compare, position of the segment in the call's list ascending, docId ascending)."""
import numpy as np

from rawseg import _np_bm25, avgdl_of

SHOULD, MUST, NOT = 0, 1, 2
PAD_SCORE_BITS, PAD_ID = 0xFF800000, 0xFFFFFFFF


def group_matched(lists, refs, n_docs):
    """refs: [(list number, role)] of one group -> sorted int64 docIds of its matched set"""
    none = np.zeros(0, np.int64)

    def inside(li):
        d = np.asarray(lists[li][0], dtype=np.int64)
        return np.unique(d[d < n_docs])

    must = [li for li, r in refs if r == MUST]
    if any(len(lists[li][0]) == 0 for li in must):
        return none
    should = [li for li, r in refs if r == SHOULD and len(lists[li][0]) > 0]
    excluded = [li for li, r in refs if r == NOT and len(lists[li][0]) > 0]
    if must:
        docs = inside(must[0])
        for li in must[1:]:
            docs = np.intersect1d(docs, inside(li))
    elif should:
        docs = none
        for li in should:
            docs = np.union1d(docs, inside(li))
    else:
        return none
    for li in excluded:
        docs = np.setdiff1d(docs, inside(li))
    return docs.astype(np.int64)


def group_scores(segment, refs, idfs, weights):
    """the accumulator {doc: fp32} of one group over its refs that are not NOT, in query order"""
    n_docs, doc_len, lists = segment
    dl = np.ascontiguousarray(doc_len, dtype=np.uint32)
    numbers = [li for li, r in refs if r != NOT]
    inside = [(np.asarray(d)[np.asarray(d) < n_docs], np.asarray(t)[np.asarray(d) < n_docs]) for d, t in lists]
    return _np_bm25(inside, numbers, [idfs[li] for li in numbers], [weights[li] for li in numbers], dl, avgdl_of(dl))


def boolean_all(segments, queries, seg_order=None, idfs=None, weights=None):
    """-> per query the whole matched set as (score fp32, segment, doc) in the canonical order"""
    order = list(range(len(segments))) if seg_order is None else list(seg_order)
    out = []
    for q in queries:
        rows = []
        for pos, s in enumerate(order):
            refs = [(li, r) for ss, li, r in q if ss == s]
            if not refs:
                continue
            docs = group_matched(segments[s][2], refs, int(segments[s][0]))
            if not len(docs):
                continue
            acc = group_scores(segments[s], refs, idfs[s], weights[s])
            rows += [(np.float32(acc[d]), pos, d, s) for d in docs.tolist()]
        rows.sort(key=lambda t: (-float(t[0]), t[1], t[2]))
        out.append([(v, s, d) for v, _, d, s in rows])
    return out


def boolean_hits(segments, queries, k, seg_order=None, idfs=None, weights=None, cache=None):
    """-> per query (found, the first K = clamp(k, 1, 100) of boolean_all).  cache: a dict the caller keeps per (segments,
    queries, seg_order, idfs, weights): the whole answer depends on nothing else."""
    K = min(max(int(k), 1), 100)
    if cache is not None and "all" in cache:
        everything = cache["all"]
    else:
        everything = boolean_all(segments, queries, seg_order, idfs, weights)
        if cache is not None:
            cache["all"] = everything
    return [(len(rows), rows[:K]) for rows in everything]


def check(ref, hits, nhits, found, k, label="", ids=None):
    """one call's outputs against boolean_hits(...): found, nhits, (seg, doc) order, score bits and the padding of every row's
    tail.  ids: segment index -> the seg_id its hits carry (default: the index)"""
    K = min(max(int(k), 1), 100)
    assert hits.shape[1] == K
    for qi, (want_found, want) in enumerate(ref):
        what = (label, "k", k, "query", qi)
        assert int(found[qi]) == want_found, what + ("found", int(found[qi]), want_found)
        n = int(nhits[qi])
        assert n == len(want) == min(K, want_found), what + ("nhits", n, len(want))
        got = [(int(s), int(d)) for s, d in zip(hits[qi, :n]["seg"], hits[qi, :n]["doc"])]
        exp = [(s if ids is None else ids[s], d) for _, s, d in want]
        if got != exp:
            at = next(i for i in range(n) if got[i] != exp[i])
            raise AssertionError(what + ("(seg, doc) differ first at rank", at, "got", got[at:at + 4], "want", exp[at:at + 4]))
        bits = np.array([v for v, _, _ in want], dtype=np.float32).view(np.uint32)
        np.testing.assert_array_equal(hits[qi, :n]["score"].view(np.uint32), bits, err_msg=str(what))
        tail = hits[qi, n:K]
        assert np.all(tail["score"].view(np.uint32) == PAD_SCORE_BITS) and np.all(tail["seg"] == PAD_ID) and np.all(tail["doc"] == PAD_ID), what + ("padding",)
