"""The related-terms rule restated in numpy for the tests (host/related.hpp is the authority), and the engine's
merge across segments.

A row is a set of documents of one segment (sorted, repeats dropped, at most 255).  fg[t] = the row's documents that hold a pair
(t, tf) with tf >= max(min_tf, 1).  t qualifies when fg[t] >= max(min_docs, 1), min_df <= df[t] <= max_df, df[t] >= 1 and
0 < idf[t] < inf.  w = float32(fg) * idf[t]: ONE fp32 multiply.  The selection is the first T = clamp(max_terms, 1, 64) qualifying
terms by (bit pattern of w descending, termId ascending).  idf is an INPUT (the host's bm25_idf).  Test infrastructure only."""
import numpy as np

MAX_TERMS = 64
MAX_OUT = 32
MAX_ROW_DOCS = 255
DEFAULTS = {"max_terms": 10, "min_tf": 1, "min_docs": 2, "min_df": 1, "max_df": 0xFFFFFFFF, "sample": 100}


def clamp_terms(max_terms):
    return max(1, min(int(max_terms), MAX_TERMS))


def clamp_out(max_terms):
    return max(1, min(int(max_terms), MAX_OUT))


def doc_offsets(counts):
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.asarray(counts, dtype=np.int64))
    return off


def row_pairs(counts, pairs, docs):
    """-> (distinct docs ascending, their pairs[m, 2] back to back)"""
    off = doc_offsets(counts)
    ids = np.unique(np.asarray(docs, dtype=np.int64))
    p = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    parts = [p[off[d]:off[d + 1]] for d in ids]
    return ids, (np.concatenate(parts) if parts else np.zeros((0, 2), np.uint32))


def rank(counts, pairs, df, idf, docs, min_tf=1, min_docs=2, min_df=1, max_df=0xFFFFFFFF):
    """-> (terms u32[m], fg u32[m], w f32[m], n distinct docs): EVERY qualifying term of the row, best first"""
    ids, p = row_pairs(counts, pairs, docs)
    assert len(ids) <= MAX_ROW_DOCS
    p = p[p[:, 1] >= max(int(min_tf), 1)]
    t, fg = np.unique(p[:, 0], return_counts=True)                      # term ids are unique inside a document
    d = np.asarray(df, dtype=np.uint32)[t]
    f = np.asarray(idf, dtype=np.float32)[t]
    with np.errstate(invalid="ignore"):
        ok = (fg >= max(int(min_docs), 1)) & (d >= 1) & (d >= int(min_df)) & (d <= int(max_df)) & (f > 0) & np.isfinite(f)
    t, fg, f = t[ok].astype(np.uint32), fg[ok].astype(np.uint32), f[ok]
    with np.errstate(over="ignore"):
        w = fg.astype(np.float32) * f                                  # one fp32 multiply
    key = (w.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (~t).astype(np.uint64)
    order = np.argsort(key, kind="stable")[::-1]
    return t[order], fg[order], w[order].astype(np.float32), len(ids)


def aggregate_rows(counts, pairs, df, idf, rows, T, min_tf=1, min_docs=2, min_df=1, max_df=0xFFFFFFFF):
    """the arrays ns_docterms_aggregate fills: (term u32[n, T], docs u32[n, T], w f32[n, T], count u32[n], ndocs u32[n])"""
    T = clamp_terms(T)
    n = len(rows)
    term, docs, w = np.full((n, T), 0xFFFFFFFF, dtype=np.uint32), np.zeros((n, T), dtype=np.uint32), np.zeros((n, T), dtype=np.float32)
    count, ndocs = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for i, r in enumerate(rows):
        t_, g_, w_, nd = rank(counts, pairs, df, idf, r, min_tf, min_docs, min_df, max_df)
        m = min(len(t_), T)
        term[i, :m], docs[i, :m], w[i, :m], count[i], ndocs[i] = t_[:m], g_[:m], w_[:m], m, nd
    return term, docs, w, count, ndocs


def windows_skipped(counts, pairs, n_terms, rows, W):
    """how many (row, window) steps of the counting kernel find no pair of any document of the row: a row without documents walks
    no window at all; min_tf plays no part (a window whose pairs are all dropped is still swept)"""
    n_win = (int(n_terms) + W - 1) // W
    skipped = 0
    for r in rows:
        ids, p = row_pairs(counts, pairs, r)
        if len(ids):
            skipped += n_win - len(np.unique(p[:, 0] // W))
    return skipped


def merge(segs, N_all, idf_of, lex_df, rows, opt):
    """Engine::terms_batch: segs[s] = {counts, pairs, terms (bytes by term id), df, idf}; lex_df(term bytes) = the lexicon df summed
    over all loaded segments; idf_of(N, df) the engine's bm25_idf; rows of (segment, doc).  One loaded segment: the options reach
    the aggregate as they are; several: it counts with min_docs 1 and no df bounds and the summed numbers are judged.
    -> per row [(term bytes, docs, df, w)], ndocs per row"""
    o = dict(DEFAULTS, **opt)
    one = len(segs) == 1
    out, ndocs = [], []
    for row in rows:
        acc, nd = {}, 0
        for s, seg in enumerate(segs):
            ids = [d for ss, d in row if ss == s]
            if not ids:
                continue
            t, g, _, n = rank(seg["counts"], seg["pairs"], seg["df"], seg["idf"], ids, o["min_tf"], o["min_docs"] if one else 1,
                              o["min_df"] if one else 1, o["max_df"] if one else 0xFFFFFFFF)
            nd += n
            for ti, gi in zip(t[:MAX_TERMS].tolist(), g[:MAX_TERMS].tolist()):
                e = acc.setdefault(seg["terms"][ti], [0, s, ti])
                e[0] += gi
        cands = []
        for term, (docs, pos, tid) in acc.items():
            df = lex_df(term)
            if docs < max(o["min_docs"], 1) or df < 1 or df < o["min_df"] or df > o["max_df"]:
                continue
            f = np.float32(idf_of(N_all, df))
            if not (f > 0 and np.isfinite(f)):
                continue
            w = np.float32(np.float32(docs) * f)
            cands.append((-int(w.view(np.uint32)), pos, tid, term, docs, df, w))
        cands.sort(key=lambda c: c[:3])
        out.append([(term, docs, df, w) for _, _, _, term, docs, df, w in cands])
        ndocs.append(nd)
    return out, ndocs
