"""The "more like this" selection rule restated in numpy for the tests (host/similar.hpp is the authority).

A pair (t, tf) of a document qualifies when tf >= max(min_tf, 1), min_df <= df[t] <= max_df, df[t] >= 1 and 0 < idf[t] < inf.
Its weight is w = float32(tf) * idf[t]: ONE fp32 multiply.  The selection is the first T = clamp(max_terms, 1, 32) qualifying
pairs by (bit pattern of w descending, termId ascending).  idf is an INPUT: the host's bm25_idf(N, df) (glibc logf), which
the tests take from nsh_bm25_idf, as search does.  Test infrastructure only."""
import numpy as np

MAX_TERMS = 32
DEFAULTS = {"max_terms": 25, "min_tf": 1, "min_df": 1, "max_df": 0xFFFFFFFF, "boost": False}


def clamp_terms(max_terms):
    return max(1, min(int(max_terms), MAX_TERMS))


def clamp_k(k):
    """the search behind similar_batch runs with k + 1 <= 100"""
    return max(1, min(int(k), 99))


def doc_offsets(counts):
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.asarray(counts, dtype=np.int64))
    return off


def rank(counts, pairs, df, idf, doc, min_tf=1, min_df=1, max_df=0xFFFFFFFF):
    """-> (terms u32[m], w f32[m]): EVERY qualifying pair of document `doc`, best first"""
    off = doc_offsets(counts)
    p = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)[off[doc]:off[doc + 1]]
    t, tf = p[:, 0], p[:, 1]
    d = np.asarray(df, dtype=np.uint32)[t]
    f = np.asarray(idf, dtype=np.float32)[t]
    with np.errstate(invalid="ignore"):
        ok = (tf >= max(int(min_tf), 1)) & (d >= 1) & (d >= int(min_df)) & (d <= int(max_df)) & (f > 0) & np.isfinite(f)
    t, tf, f = t[ok], tf[ok], f[ok]
    with np.errstate(over="ignore"):
        w = tf.astype(np.float32) * f                                  # one fp32 multiply
    key = (w.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (~t).astype(np.uint64)
    order = np.argsort(key, kind="stable")[::-1]
    return t[order].astype(np.uint32), w[order].astype(np.float32)


def select(counts, pairs, df, idf, doc, T, min_tf=1, min_df=1, max_df=0xFFFFFFFF):
    """-> (terms u32[m], w f32[m]), m <= clamp_terms(T): the selection of document `doc`, best first"""
    t, w = rank(counts, pairs, df, idf, doc, min_tf, min_df, max_df)
    return t[:clamp_terms(T)], w[:clamp_terms(T)]


def select_rows(counts, pairs, df, idf, docs, T, min_tf=1, min_df=1, max_df=0xFFFFFFFF):
    """the arrays ns_docterms_select fills: (term u32[n, T], w f32[n, T], count u32[n]), ~0 / 0.0 past the count"""
    T = clamp_terms(T)
    term = np.full((len(docs), T), 0xFFFFFFFF, dtype=np.uint32)
    w = np.zeros((len(docs), T), dtype=np.float32)
    count = np.zeros(len(docs), dtype=np.uint32)
    cache = {}
    for i, d in enumerate(docs):
        d = int(d)
        if d not in cache:
            cache[d] = select(counts, pairs, df, idf, d, T, min_tf, min_df, max_df)
        t_, w_ = cache[d]
        term[i, :len(t_)], w[i, :len(t_)], count[i] = t_, w_, len(t_)
    return term, w, count


def weights(w, boost):
    """the query weights of a selection: 1.0, or with boost w / w_first (one fp32 division each)"""
    w = np.asarray(w, dtype=np.float32)
    if not boost or len(w) == 0:
        return np.ones(len(w), dtype=np.float32)
    return (w / w[0]).astype(np.float32)
