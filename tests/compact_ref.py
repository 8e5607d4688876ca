"""Compaction restated in Python for the tests: the merge of several segments' forward indexes over
ingest_ref's dict form (kept_docs, doc_len, counts, pairs u32[n, 2], terms) — term walk, remap, sort inside each document,
concatenation — and writers for source segments, among them sources with a PERMUTED term numbering that stand for
segments the reference wrote (it numbers terms in std::unordered_map order).  Test infrastructure only."""
import os

import numpy as np

import ingest_ref


def term_walk(parts):
    """-> (merged term list, per part the u32 array old id -> new id): the parts' term lists in part order, each in its own
    id order; a byte string gets the next free id the first time it is seen."""
    new_id, terms, maps = {}, [], []
    for p in parts:
        m = np.empty(len(p["terms"]), dtype=np.uint32)
        assert len(set(p["terms"])) == len(p["terms"]), "a term twice in one part"
        for old, t in enumerate(p["terms"]):
            tid = new_id.get(t)
            if tid is None:
                tid = new_id[t] = len(terms)
                terms.append(t)
            m[old] = tid
        maps.append(m)
    return terms, maps


def _doc_of(counts):
    return np.repeat(np.arange(len(counts), dtype=np.int64), counts.astype(np.int64))


def sort_inside_documents(counts, pairs):
    """pairs grouped by document -> the same, term ids ascending inside each document"""
    if len(pairs) == 0:
        return pairs.reshape(-1, 2)
    order = np.lexsort((pairs[:, 0], _doc_of(counts)))
    return np.ascontiguousarray(pairs[order])


def merge(parts):
    """parts: list of ingest_ref.build results (or permuted ones) -> the merged forward index in the same form;
    kept_docs is the identity: a merged document's id is its position"""
    terms, maps = term_walk(parts)
    doc_len = np.concatenate([p["doc_len"] for p in parts] + [np.empty(0, dtype=np.uint32)]).astype(np.uint32)
    counts = np.concatenate([p["counts"] for p in parts] + [np.empty(0, dtype=np.uint32)]).astype(np.uint32)
    chunks = []
    for p, m in zip(parts, maps):
        pr = np.asarray(p["pairs"], dtype=np.uint32).reshape(-1, 2)
        assert len(pr) == 0 or int(pr[:, 0].max()) < len(m), "termId >= n_terms"
        chunks.append(np.stack([m[pr[:, 0]], pr[:, 1]], axis=1) if len(pr) else pr)
    pairs = np.concatenate(chunks + [np.empty((0, 2), dtype=np.uint32)]).astype(np.uint32)
    return {"kept_docs": np.arange(len(doc_len), dtype=np.uint32), "doc_len": doc_len, "counts": counts,
            "pairs": sort_inside_documents(counts, pairs), "terms": terms}


def docs_whose_order_changes(parts):
    """per part: how many of its documents have their pairs in another order after the remap (the re-sort's real work)"""
    _, maps = term_walk(parts)
    out = []
    for p, m in zip(parts, maps):
        pr = np.asarray(p["pairs"], dtype=np.uint32).reshape(-1, 2)
        if len(pr) == 0:
            out.append(0)
            continue
        new = m[pr[:, 0]].astype(np.int64)
        doc = _doc_of(p["counts"])
        desc = (new[1:] < new[:-1]) & (doc[1:] == doc[:-1])
        out.append(int(len(np.unique(doc[1:][desc]))))
    return out


def kept_documents(docs, fwd):
    """the documents of `docs` that survived indexing, in docId order"""
    return [docs[int(d)] for d in fwd["kept_docs"]]


def merged_file_bytes(part_docs, parts, merged):
    """the four forward files of the merged segment: part_docs[i] = the documents handed to part i's build"""
    docs = [d for dd, p in zip(part_docs, parts) for d in kept_documents(dd, p)]
    return ingest_ref.file_bytes(docs, merged)


def permute(fwd, seed):
    """the same forward index under another term numbering: the term list shuffled, the pairs renumbered and sorted inside
    each document again — what a segment of the reference looks like next to this project's"""
    rng = np.random.default_rng(seed)
    n = len(fwd["terms"])
    perm = rng.permutation(n).astype(np.uint32)                      # old id -> new id
    terms = [None] * n
    for old, new in enumerate(perm):
        terms[int(new)] = fwd["terms"][old]
    pr = np.asarray(fwd["pairs"], dtype=np.uint32).reshape(-1, 2)
    pairs = np.stack([perm[pr[:, 0]], pr[:, 1]], axis=1) if len(pr) else pr
    return {"kept_docs": fwd["kept_docs"], "doc_len": fwd["doc_len"], "counts": fwd["counts"],
            "pairs": sort_inside_documents(fwd["counts"], pairs), "terms": terms}


def write_forward_files(seg_dir, docs, fwd):
    """docs.bin, stats.bin, forward.bin, terms.bin of `fwd` (any numbering) into seg_dir; docs = the documents handed to
    the build (fwd["kept_docs"] picks the survivors)"""
    os.makedirs(seg_dir, exist_ok=True)
    files = ingest_ref.file_bytes(docs, fwd)
    for name, b in files.items():
        with open(os.path.join(seg_dir, name), "wb") as f:
            f.write(b)
    return files


def read_tree(root):
    """{relative path: bytes} of every file under root"""
    out = {}
    for d, _, files in sorted(os.walk(root)):
        for fn in sorted(files):
            p = os.path.join(d, fn)
            with open(p, "rb") as f:
                out[os.path.relpath(p, root)] = f.read()
    return out


def cut(items, sizes):
    """items cut into consecutive parts of the given sizes (the last part takes the rest)"""
    out, at = [], 0
    for s in sizes:
        out.append(items[at:at + s])
        at += s
    out.append(items[at:])
    return [p for p in out if len(p)]
