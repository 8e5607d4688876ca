"""Numpy / Python restatement of the search sorted by a per-document key, independent of the kernels.

Per query: the matched set of every segment comes from facet_ref.matched (union under OR, intersection under AND, docId <
n_docs).  The order is a Python sort on the one total order  (rank key, position of the segment in the call's list
ascending, docId ascending)  where a larger key is first under newest-first, a smaller NON-ZERO key first under oldest-
first, and key 0 is last in both directions.  The score of a hit is rawseg's fp32 restatement accumulator (_np_bm25: +0.0f
start, query-term order, a list named twice added twice), looked up for the hit's document."""
import numpy as np

import facet_ref
from rawseg import _np_bm25, avgdl_of

PAD_SCORE_BITS, PAD_ID = 0xFF800000, 0xFFFFFFFF


def rank_of(key, ascending):
    """the sort key of the restatement: smaller tuple first"""
    key = int(key)
    if key == 0:
        return (1, 0)
    return (0, key if ascending else -key)


def sorted_hits(segments, queries, keys, k, and_mode, ascending, seg_order=None, idfs=None, weights=None, acc_cache=None):
    """segments: (n_docs, doc_len, lists) each; queries: lists of (segment, list number); keys: one uint32 array per segment;
    seg_order: the segments in the call's order (default 0 .. n-1).  -> per query (found, [(segment, doc, key, score or None)]
    of the first K); scores only when idfs / weights ([segment][list]) are given.  acc_cache: a dict the caller keeps per
    (segments, queries, idfs, weights): the matched sets (per mode) and the accumulators depend on nothing else."""
    order = list(range(len(segments))) if seg_order is None else list(seg_order)
    K = min(max(int(k), 1), 100)
    out = []
    for qi, q in enumerate(queries):
        rows, found = [], 0
        for pos, s in enumerate(order):
            numbers = [li for ss, li in q if ss == s]
            if not numbers:
                continue
            n_docs, doc_len, lists = segments[s]
            mkey = ("matched", qi, s, bool(and_mode))
            if acc_cache is not None and mkey in acc_cache:
                docs = acc_cache[mkey]
            else:
                docs = facet_ref.matched(lists, numbers, int(n_docs), and_mode)
                if acc_cache is not None:
                    acc_cache[mkey] = docs
            found += len(docs)
            for d in docs.tolist():
                rows.append((rank_of(keys[s][d], ascending), pos, d, s))
        rows.sort()
        rows = rows[:K]
        hits = []
        acc_of = {} if acc_cache is None else acc_cache.setdefault(qi, {})
        for _, _, d, s in rows:
            score = None
            if idfs is not None:
                if s not in acc_of:
                    n_docs, doc_len, lists = segments[s]
                    numbers = [li for ss, li in q if ss == s]
                    dl = np.ascontiguousarray(doc_len, dtype=np.uint32)
                    inside = [(lists[li][0][lists[li][0] < n_docs], lists[li][1][lists[li][0] < n_docs]) for li in range(len(lists))]
                    acc_of[s] = _np_bm25(inside, numbers, [idfs[s][li] for li in numbers], [weights[s][li] for li in numbers], dl, avgdl_of(dl))
                score = np.float32(acc_of[s][d])
            hits.append((s, d, int(keys[s][d]), score))
        out.append((found, hits))
    return out


def resort(triples, key_of, pos_of, ascending):
    """(score, seg, doc) triples of a scored search -> the same triples in the total order; key_of(seg, doc), pos_of(seg)"""
    return sorted(triples, key=lambda t: (rank_of(key_of(t[1], t[2]), ascending), pos_of(t[1]), t[2]))


def check(ref, hits, keys, nhits, found, k, label="", ids=None):
    """one call's outputs against sorted_hits(...): found, nhits, (seg, doc) order, keys, score bits where the restatement has
    them, and the padding of every row's tail.  ids: segment index -> the seg_id its hits carry (default: the index)"""
    K = min(max(int(k), 1), 100)
    assert hits.shape[1] == K and keys.shape[1] == K
    for qi, (want_found, want) in enumerate(ref):
        what = (label, "k", k, "query", qi)
        assert int(found[qi]) == want_found, what + ("found", int(found[qi]), want_found)
        n = int(nhits[qi])
        assert n == len(want) == min(K, want_found), what + ("nhits", n, len(want))
        got = [(int(s), int(d)) for s, d in zip(hits[qi, :n]["seg"], hits[qi, :n]["doc"])]
        exp = [(s if ids is None else ids[s], d) for s, d, _, _ in want]
        if got != exp:
            at = next(i for i in range(n) if got[i] != exp[i])
            raise AssertionError(what + ("(seg, doc) differ first at rank", at, "got", got[at:at + 4], "want", exp[at:at + 4]))
        assert [int(x) for x in keys[qi, :n]] == [kk for _, _, kk, _ in want], what + ("keys",)
        if want and want[0][3] is not None:
            bits = np.array([sc for _, _, _, sc in want], dtype=np.float32).view(np.uint32)
            np.testing.assert_array_equal(hits[qi, :n]["score"].view(np.uint32), bits, err_msg=str(what))
        tail = hits[qi, n:K]
        assert np.all(tail["score"].view(np.uint32) == PAD_SCORE_BITS) and np.all(tail["seg"] == PAD_ID) and np.all(tail["doc"] == PAD_ID), what + ("padding",)
        assert np.all(keys[qi, n:K] == 0), what + ("key padding",)
