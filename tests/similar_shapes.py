"""Directed inputs of the "more like this" selection, shared by tests/test_similar_cpu.py (host restatement
against tests/similar_ref.py) and tests/test_similar_gpu.py (ns_docterms_select against it).  One synthetic segment:
documents of every size class, ties, few and no qualifying pairs, the best key in the last lane of a partial chunk.
Test infrastructure only."""
import numpy as np

import ingest_ref
import nsbind
from test_compact_gpu import size_class_batches

N_DOCS_FOR_IDF = 5000            # the N of bm25_idf(N, df) for this synthetic segment


def idf_of(n_docs, df):
    """the host's bm25_idf (glibc logf), as search computes it; 0 where df == 0"""
    H = nsbind.host_lib()
    out = np.zeros(len(df), dtype=np.float32)
    memo = {}
    for i, d in enumerate(np.asarray(df).tolist()):
        if d:
            if d not in memo:
                memo[d] = H.nsh_bm25_idf(int(n_docs), int(d))
            out[i] = memo[d]
    return out


def directed(cut):
    """-> (part {counts, pairs}, df, idf, docs {name: doc id}).  Documents 0 .. 8 are size_class_batches' source 1 (1, 2, 63, 64,
    65, cut - 1, cut, cut + 1 and 100 003 pairs, tf 1 or 2); the others are appended here."""
    rng = np.random.default_rng(77)
    batches, sizes = size_class_batches(cut)
    base = ingest_ref.build(batches[1])
    assert list(base["counts"]) == sizes
    n_terms = len(base["terms"])
    counts, chunks, docs = [int(c) for c in base["counts"]], [base["pairs"]], {}
    for name, d in zip(("n1", "n2", "n63", "n64", "n65", "cut_minus_1", "cut", "cut_plus_1", "n100003"), range(len(sizes))):
        docs[name] = d
    # df: mostly 1 .. N, every 11th term 0 (no lexicon entry), three reserved ranges set below
    df = rng.integers(1, N_DOCS_FOR_IDF, n_terms).astype(np.uint32)
    df[::11] = 0
    eq = np.arange(2000, 2600)          # terms of ONE df: termId alone orders them
    df[eq] = 37
    dead = np.arange(3000, 3100)        # terms no lexicon holds
    df[dead] = 0
    odd = np.arange(3200, 3208)         # df >= 1 but an idf that is not a positive finite number
    df[odd] = 5

    def add(name, terms, tfs):
        docs[name] = len(counts)
        counts.append(len(terms))
        chunks.append(np.stack([np.asarray(terms, dtype=np.uint32), np.asarray(tfs, dtype=np.uint32)], axis=1).reshape(-1, 2))

    add("n0", [], [])
    for n in (127, 128, 129):
        add("n%d" % n, rng.choice(n_terms, n, replace=False), rng.integers(1, 6, n))
    live = np.flatnonzero(df > 0)
    live = live[(live < 2000) | (live >= 3300)]
    add("few", np.concatenate([dead[:33], live[:7]]), rng.integers(1, 4, 40))                  # 7 qualify: fewer than T = 25 and 32
    add("none", np.concatenate([dead[40:64], odd[:6]]), np.full(30, 3))                      # nothing qualifies
    add("tf1_equal_df", rng.permutation(eq[:100]), np.ones(100))                            # termId alone orders
    # ties in w in groups of three (places 1-3, 4-6, ...): T = 1, 25 and 32 each cut a group; larger termIds come FIRST
    tie_terms = eq[200:245][::-1]
    tie_tf = np.repeat(np.arange(15, 0, -1), 3)
    add("ties_short", tie_terms, tie_tf)
    filler = rng.choice(live[live > 4000], 255, replace=False)
    mix_t, mix_f = np.concatenate([tie_terms, filler]), np.concatenate([tie_tf * 1000, np.ones(255, dtype=np.int64)])
    p = rng.permutation(300)
    order = np.argsort(-mix_t[p], kind="stable")                                             # still: the larger termId earlier in the stream
    add("ties_long", mix_t[p][order], mix_f[p][order])
    for name, n in (("last_lane_wave", 64 * 3 + 37), ("last_lane_block", cut + 64 * 5 + 37)):
        t = rng.choice(live[live > 4000], n, replace=False)
        tf = np.ones(n, dtype=np.int64)
        tf[-1] = 100000                                                                      # the best key is the last pair of the last, partial chunk
        add(name, t, tf)
    # tf and df values to stand next to: tf in {1, 2, 3, 5}, df in {9, 10, 11} and others
    opt_terms = live[100:160].copy()
    df[opt_terms[:20]] = 9
    df[opt_terms[20:40]] = 10
    df[opt_terms[40:]] = 11
    add("options", opt_terms, np.tile([1, 2, 3, 5], 15))
    idf = idf_of(N_DOCS_FOR_IDF, df)
    idf[odd] = np.array([np.nan, np.inf, 0.0, -1.0, -np.inf, -0.0, np.nan, 0.0], dtype=np.float32)
    part = {"counts": np.asarray(counts, dtype=np.uint32), "pairs": np.concatenate([c.astype(np.uint32) for c in chunks])}
    assert int(part["counts"].sum()) == len(part["pairs"])
    return part, df, idf, docs


T_VALUES = (1, 25, 32)
# (min_tf, min_df, max_df): the defaults, then values at and next to the ones document "options" holds
OPTION_SETS = [(1, 1, 0xFFFFFFFF), (0, 0, 0xFFFFFFFF), (2, 1, 0xFFFFFFFF), (3, 1, 0xFFFFFFFF), (4, 1, 0xFFFFFFFF), (5, 1, 0xFFFFFFFF), (6, 1, 0xFFFFFFFF),
               (1, 9, 0xFFFFFFFF), (1, 10, 0xFFFFFFFF), (1, 11, 0xFFFFFFFF), (1, 12, 0xFFFFFFFF), (1, 1, 8), (1, 1, 9), (1, 1, 10), (1, 1, 11),
               (1, 10, 10), (2, 10, 11), (1, 11, 9)]


def assert_rows_equal(got, want, what):
    """term, w (bit patterns) and count arrays equal, the padding included"""
    (gt, gw, gc), (wt, ww, wc) = got, want
    assert np.array_equal(gc, wc), (what, "count")
    assert np.array_equal(gt, wt), (what, "term")
    assert np.array_equal(np.ascontiguousarray(gw).view(np.uint32), np.ascontiguousarray(ww).view(np.uint32)), (what, "w bits")
