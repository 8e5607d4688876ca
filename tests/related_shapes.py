"""Directed inputs of the related-terms aggregate, shared by tests/test_related_cpu.py (host rule against
tests/related_ref.py) and tests/test_related_gpu.py (ns_docterms_aggregate against both).  One synthetic segment of
n_terms = 2 * W + 7 term ids (W = ns_docterms_window()): terms on both sides of every window edge, a window a row never reaches,
byte counters at 255 next to one at 1, rows of 0, 1 and 255 documents, repeats, a document without pairs, a long document, more
than 64 terms of one weight, and every option deciding a term.  Run as a program it checks the loaded HIP library against the
restatement and reports the counting build's event counters (tests/test_related_gpu.py starts it on libnextsearch_hip_count.so).
Test infrastructure only."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "nextsearch-api_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import nsbind  # noqa: E402
import related_ref  # noqa: E402

N_DOCS_FOR_IDF = 5000            # the N of bm25_idf(N, df) for this synthetic segment
COUNTER_NAMES = ("windows skipped", "windows swept", "chunks below min_docs", "chunks below the threshold", "joins", "rows refused",
                 "pairs dropped by min_tf", "rows")


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


def directed(W, cut):
    """-> (part {counts, pairs}, df, idf, docs {name: doc id or list of ids}, rows {name: [doc ids]}, n_terms)"""
    rng = np.random.default_rng(91)
    n_terms = 2 * W + 7
    assert n_terms % 4 != 0
    edge = [W - 1, W, 2 * W - 1, 2 * W, n_terms - 1]
    counts, chunks, docs = [], [], {}

    def add(name, terms, tfs):
        terms, tfs = np.asarray(terms, dtype=np.int64), np.asarray(tfs, dtype=np.int64)
        order = np.argsort(terms, kind="stable")
        assert len(np.unique(terms)) == len(terms)
        d = len(counts)
        counts.append(len(terms))
        chunks.append(np.stack([terms[order], tfs[order]], axis=1).astype(np.uint32).reshape(-1, 2))
        if name is not None:
            docs[name] = d
        return d

    # 255 documents that all hold 4j, 4j + 1, 4j + 2 (j = 25 .. 29), 4j + 3 held by the first alone: 255, 255, 255 and 1 in one word;
    # the edge ids spread over them by small primes
    quad = [4 * j + b for j in range(25, 30) for b in range(3)]
    full = []
    for i in range(255):
        t = list(quad) + ([4 * j + 3 for j in range(25, 30)] if i == 0 else [])
        t += [e for e, m in zip(edge, (2, 3, 5, 7, 11)) if i % m == 0]
        full.append(add(None, t, np.ones(len(t))))
    docs["full"] = full
    docs["extra"] = add(None, quad[:4], np.ones(4))                   # the 256th distinct document
    docs["empty"] = add(None, [], [])
    # short documents over a small topic vocabulary in all three windows, tf 1 .. 5
    topic = np.concatenate([rng.choice(np.arange(200, 3000), 150, replace=False), W + rng.choice(3000, 150, replace=False), 2 * W + np.arange(7)])
    docs["short"] = [add(None, rng.choice(topic, n, replace=False), rng.integers(1, 6, n)) for n in (1, 5, 17, 40, 60, 64, 65, 90, 120, 33, 48, 77)]
    docs["long"] = add(None, rng.choice(n_terms, cut + 1, replace=False), rng.integers(1, 4, cut + 1))
    # the skip path: two documents with pairs in windows 0 and 2 only
    docs["skip"] = [add(None, list(range(500 + k, 520)) + list(range(2 * W, 2 * W + 5 + k)), np.ones(20 - k + 5 + k)) for k in (0, 1)]
    # 80 terms of ONE weight (one df, held by the same three documents), 40 in window 0 and 40 in window 1: term id alone orders them
    ties = list(range(3100, 3140)) + list(range(W + 3100, W + 3140))
    docs["ties"] = [add(None, ties[::-1] if k == 1 else ties, np.full(80, 1 + k)) for k in range(3)]
    # options: 60 terms, df 9 / 10 / 11 by thirds, four documents whose tf pattern (1, 2, 3, 5) is rotated
    opt_terms = np.arange(4000, 4060)
    docs["options"] = [add(None, opt_terms, np.roll(np.tile([1, 2, 3, 5], 15), k)) for k in range(4)]
    # idf that is not a positive finite number, and one so large that w overflows to inf
    odd = np.arange(4100, 4108)
    ovf = 4120
    docs["odd"] = [add(None, list(odd) + [ovf, 4121 + k, 4130], [3] * 8 + [1 if k == 2 else 2, 1, 1]) for k in range(3)]

    df = rng.integers(1, N_DOCS_FOR_IDF, n_terms).astype(np.uint32)
    df[::13] = 0                                                       # no lexicon entry
    df[quad] = 400
    df[[4 * j + 3 for j in range(25, 30)]] = 400
    df[edge] = [50, 60, 70, 80, 90]
    df[ties] = 37
    df[opt_terms[:20]], df[opt_terms[20:40]], df[opt_terms[40:]] = 9, 10, 11
    df[odd] = 5
    df[[ovf, 4130]] = 7
    df[2 * W:2 * W + 7] = [3, 4, 0, 6, 7, 8, 90]
    idf = idf_of(N_DOCS_FOR_IDF, df)
    idf[odd] = np.array([np.nan, np.inf, 0.0, -1.0, -np.inf, -0.0, np.nan, 0.0], dtype=np.float32)
    idf[ovf] = np.float32(3.0e38)
    part = {"counts": np.asarray(counts, dtype=np.uint32), "pairs": np.concatenate([c for c in chunks])}
    assert int(part["counts"].sum()) == len(part["pairs"]) and int(part["pairs"][:, 0].max()) == n_terms - 1

    s = docs["short"]
    rows = {
        "empty": [], "one": [s[3]], "full 255": list(full), "300 ids, 255 distinct": list(full) + full[:45],
        "repeats": [s[1], s[1], s[2], s[2], s[1], s[4], s[4]], "skip": list(docs["skip"]), "ties": list(docs["ties"]),
        "long": [docs["long"], s[0], s[5], s[6]], "a document without pairs": [docs["empty"], s[7], docs["empty"], s[8]],
        "only a document without pairs": [docs["empty"]], "options": list(docs["options"]), "odd": list(docs["odd"]),
        "shared 1": [s[9], s[10]], "shared 2": [s[9], s[11]], "shared 3": [s[9], s[2], s[3]],
        "mixed": s + docs["ties"] + [docs["long"]] + docs["options"] + docs["odd"] + full[:30],
        "unsorted": s[::-1] + full[10:0:-1],
    }
    return part, df, idf, docs, rows, n_terms


T_VALUES = (1, 10, 32, 64)
# (min_tf, min_docs, min_df, max_df): the defaults, then values at and next to the ones the directed documents hold
OPTION_SETS = [(1, 2, 1, 0xFFFFFFFF), (0, 0, 0, 0xFFFFFFFF), (2, 2, 1, 0xFFFFFFFF), (3, 2, 1, 0xFFFFFFFF), (4, 2, 1, 0xFFFFFFFF), (5, 2, 1, 0xFFFFFFFF),
               (6, 1, 1, 0xFFFFFFFF), (1, 1, 1, 0xFFFFFFFF), (1, 3, 1, 0xFFFFFFFF), (1, 4, 1, 0xFFFFFFFF), (1, 254, 1, 0xFFFFFFFF), (1, 255, 1, 0xFFFFFFFF),
               (1, 256, 1, 0xFFFFFFFF), (1, 2, 9, 0xFFFFFFFF), (1, 2, 10, 0xFFFFFFFF), (1, 2, 11, 0xFFFFFFFF), (1, 2, 12, 0xFFFFFFFF), (1, 2, 1, 8), (1, 2, 1, 9),
               (1, 2, 1, 10), (1, 2, 1, 11), (1, 2, 10, 10), (2, 3, 10, 11), (1, 2, 11, 9)]


def descending_source():
    """three documents; the second holds 7 before 5.  ns_docterms_select answers it, the aggregate refuses the handle"""
    part = {"counts": np.asarray([3, 3, 2], np.uint32), "pairs": np.asarray([[0, 1], [2, 1], [4, 2], [1, 1], [7, 2], [5, 1], [0, 1], [7, 1]], np.uint32)}
    df = np.asarray([3, 4, 5, 6, 7, 8, 9, 10], np.uint32)
    return part, df, idf_of(N_DOCS_FOR_IDF, df)


def assert_rows_equal(got, want, what):
    """term, docs, w (bit patterns), count and ndocs arrays equal, the padding included"""
    for name, g, w in zip(("count", "ndocs", "term", "docs"), (got[3], got[4], got[0], got[1]), (want[3], want[4], want[0], want[1])):
        assert np.array_equal(g, w), (what, name)
    assert np.array_equal(np.ascontiguousarray(got[2]).view(np.uint32), np.ascontiguousarray(want[2]).view(np.uint32)), (what, "w bits")


def main(out_path):
    """every directed row under every T and option set on the loaded library; the counting build's counters with it"""
    import ctypes as C
    L = nsbind.hip_lib()
    W, cut = int(L.ns_docterms_window()), int(L.ns_docterms_doc_cut())
    part, df, idf, docs, rows, n_terms = directed(W, cut)
    ctx = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(ctx)) == 0
    dt = nsbind.DocTerms(ctx, part, df, idf)
    counting = hasattr(L, "ns_debug_terms_counters")
    if counting:
        nsbind.debug_counters(reset=True)
    batch = list(rows.values())
    want_skipped = 0
    for T in T_VALUES:
        assert_rows_equal(dt.aggregate(batch, T)[:5], related_ref.aggregate_rows(part["counts"], part["pairs"], df, idf, batch, T), ("child", T))
        want_skipped += related_ref.windows_skipped(part["counts"], part["pairs"], n_terms, batch, W)
    for o in OPTION_SETS[1:]:
        assert_rows_equal(dt.aggregate(batch, 64, *o)[:5], related_ref.aggregate_rows(part["counts"], part["pairs"], df, idf, batch, 64, *o), ("child", o))
        want_skipped += related_ref.windows_skipped(part["counts"], part["pairs"], n_terms, batch, W)
    refused = 0
    try:
        dt.aggregate([docs["full"] + [docs["extra"]]])
    except RuntimeError:
        refused = 1
    rep = {"counting": counting, "window": W, "refused": refused, "want_skipped": want_skipped, "rows": len(batch) * (len(T_VALUES) + len(OPTION_SETS) - 1)}
    if counting:
        rep["counters"] = nsbind.debug_counters()["ns_debug_terms_counters"]
    dt.close()
    L.ns_ctx_destroy(ctx)
    with open(out_path, "w") as f:
        json.dump(rep, f)
    print("related shapes OK")


if __name__ == "__main__":
    main(sys.argv[1])
