"""Deleting documents restated in Python for the tests: the filter ns_forward_merge_keep applies to a source
that comes with a bitmap, over compact_ref's parts (kept_docs, doc_len, counts, pairs u32[n, 2], terms).  Composed with
compact_ref.merge it is the oracle: merge_keep(parts, keeps) == compact_ref.merge([filter_part(p, k) ...]).
Test infrastructure only."""
import numpy as np

import compact_ref


def doc_of_pairs(counts):
    return np.repeat(np.arange(len(counts), dtype=np.int64), np.asarray(counts).astype(np.int64))


def filter_part(part, keep):
    """keep: None (the part passes through unchanged) or a boolean array over the part's documents.  The part loses its
    dropped documents and their pairs and every term no surviving pair names; the surviving terms keep their relative id
    order; the surviving pairs are renumbered.  The pairs of dropped documents are not looked at."""
    if keep is None:
        return part
    keep = np.asarray(keep, dtype=bool)
    counts = np.asarray(part["counts"], dtype=np.uint32)
    assert len(keep) == len(counts)
    pairs = np.asarray(part["pairs"], dtype=np.uint32).reshape(-1, 2)
    surv = pairs[keep[doc_of_pairs(counts)]]
    n_terms = len(part["terms"])
    assert len(surv) == 0 or int(surv[:, 0].max()) < n_terms, "termId >= n_terms in a surviving pair"
    live = np.zeros(n_terms, dtype=bool)
    live[surv[:, 0]] = True
    new_id = (np.cumsum(live) - live).astype(np.uint32)               # surviving terms with a smaller old id
    return {"kept_docs": np.asarray(part["kept_docs"])[keep], "doc_len": np.asarray(part["doc_len"], dtype=np.uint32)[keep],
            "counts": counts[keep], "pairs": np.stack([new_id[surv[:, 0]], surv[:, 1]], axis=1).astype(np.uint32) if len(surv) else surv,
            "terms": [t for t, l in zip(part["terms"], live) if l]}


def merge_keep(parts, keeps):
    """the oracle of ns_forward_merge_keep"""
    return compact_ref.merge([filter_part(p, k) for p, k in zip(parts, keeps)])


def bitmap(keep, garbage_seed=None):
    """boolean array -> the uint32 words ns_forward_merge_keep reads; garbage_seed: random bits at and past len(keep) in the
    last word (they must be ignored) and a word of garbage behind it (which must not be read as documents)"""
    keep = np.asarray(keep, dtype=bool)
    n = len(keep)
    words = np.zeros((n + 31) // 32 + 1, dtype=np.uint32)
    packed = np.packbits(keep, bitorder="little")
    words.view(np.uint8)[:len(packed)] = packed
    if garbage_seed is not None:
        rng = np.random.default_rng(garbage_seed)
        if n % 32:
            words[n // 32] |= np.uint32(int(rng.integers(0, 1 << 32)) & (0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
        words[-1] = rng.integers(0, 1 << 32, dtype=np.uint64).astype(np.uint32)
    return words


def introducing_documents(part):
    """boolean array over the part's documents: the document holds the first occurrence of some term of the part"""
    pairs = np.asarray(part["pairs"], dtype=np.uint32).reshape(-1, 2)
    first = np.full(len(part["terms"]), len(part["counts"]), dtype=np.int64)
    np.minimum.at(first, pairs[:, 0].astype(np.int64), doc_of_pairs(part["counts"]))
    out = np.zeros(len(part["counts"]), dtype=bool)
    out[first[first < len(part["counts"])]] = True
    return out


def survivors(docs, part, keep):
    """the documents of `docs` (what was handed to the part's build) that are in the part and stay"""
    kept = compact_ref.kept_documents(docs, part)
    return kept if keep is None else [d for d, k in zip(kept, keep) if k]
