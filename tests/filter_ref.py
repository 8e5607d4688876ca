"""Numpy restatement of filtered search, independent of the kernels.

The compaction: a posting stays when its docId is below n_docs and its document's bit is set; survivors keep their order, so
the list [off, off + count) of the source becomes [rank(off), rank(off + count)) with rank(x) = survivors in front of
stream position x.  The ranking under a filter: tests/rawseg.py's restatement over the lists masked the same way, with the
ORIGINAL idfs, doc_len and avgdl (a filter chooses among the results, it does not change a score)."""
import numpy as np

import rawseg


def keep_of(bits, n_docs):
    """uint32 bitmap words -> bool per document (bits past n_docs are ignored)"""
    bits = np.asarray(bits, dtype=np.uint32)
    d = np.arange(int(n_docs), dtype=np.int64)
    return ((bits[d >> 5] >> (d & 31).astype(np.uint32)) & 1).astype(bool) if n_docs else np.zeros(0, bool)


def bits_of(keep, fill_tail=False):
    """bool per document -> uint32 words; fill_tail sets the unused bits of the last word (they must not matter)"""
    keep = np.asarray(keep, dtype=bool)
    n = len(keep)
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    for d in np.flatnonzero(keep):
        words[d >> 5] |= np.uint32(1) << np.uint32(d & 31)
    if fill_tail and n % 32:
        words[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    return words


def compact(flat, byte_off, counts, keep):
    """flat: the payload as (n, 2) uint32 {docId, tf}; lists as byte offsets and counts; keep: bool per document.
    -> (filtered payload (kept, 2), new byte offsets, new counts, kept)"""
    flat = np.asarray(flat, dtype=np.uint32).reshape(-1, 2)
    n_docs = len(keep)
    doc = flat[:, 0].astype(np.int64)
    stays = np.zeros(len(flat), dtype=bool)
    inside = doc < n_docs
    stays[inside] = np.asarray(keep, bool)[doc[inside]]
    rank = np.concatenate([[0], np.cumsum(stays)]).astype(np.uint64)
    first = (np.asarray(byte_off, dtype=np.uint64) // np.uint64(8)).astype(np.int64)
    last = first + np.asarray(counts, dtype=np.int64)
    return flat[stays], rank[first] * np.uint64(8), (rank[last] - rank[first]).astype(np.uint32), int(stays.sum())


def mask_lists(lists, keep):
    """lists of (docIds, tfs) -> the same lists without the postings of dropped documents (and of docIds >= n_docs)"""
    out = []
    keep = np.asarray(keep, bool)
    for docs, tfs in lists:
        docs, tfs = np.asarray(docs, np.uint32), np.asarray(tfs, np.uint32)
        m = np.zeros(len(docs), bool)
        inside = docs < len(keep)
        m[inside] = keep[docs[inside].astype(np.int64)]
        out.append((docs[m], tfs[m]))
    return out


def filtered_queries(queries, masked, and_mode):
    """The term refs a filtered query emits: a list without a surviving posting contributes no ref; under AND such a list
    empties the whole (query, segment) group (no kept document of the segment holds every term)."""
    out = []
    for q in queries:
        if and_mode and any(len(masked[li][0]) == 0 for li in q):
            out.append([])
        else:
            out.append([li for li in q if len(masked[li][0])])
    return out


def reference(lists, queries, idfs, weights, doc_len, avgdl, keep):
    """rawseg.reference over the masked lists: per query (OR ranking, AND ranking) of the kept documents.  AND: the kept
    documents that hold EVERY list the query names (an emptied list leaves none)."""
    masked = mask_lists(lists, keep)
    return rawseg.reference(masked, queries, idfs, weights, doc_len, avgdl)


def reference_multi(segments, queries, idfs, weights, keeps, avgdls=None):
    """The ranking of queries (lists of (segment, list number)) over several segments under a filter, as
    rawseg.reference_multi joins it: (score, seg, doc) triples, score desc, seg asc, doc asc, for OR and for AND.  segments:
    (n_docs, doc_len, lists) each; keeps: bool array per segment; avgdls: the segments' own (default: from doc_len)."""
    out = []
    for q in queries:
        both = ([], [])
        for s in sorted({s for s, _ in q}):
            _, doc_len, lists = segments[s]
            dl = np.ascontiguousarray(doc_len, dtype=np.uint32)
            avgdl = avgdls[s] if avgdls is not None else rawseg.avgdl_of(dl)
            (keyed, anded), = reference(lists, [[li for ss, li in q if ss == s]], idfs[s], weights[s], dl, avgdl, keeps[s])
            both[0].extend((v, s, d) for d, v in keyed)
            both[1].extend((v, s, d) for d, v in anded)
        out.append(tuple(sorted(x, key=lambda t: (-float(t[0]), t[1], t[2])) for x in both))
    return out
