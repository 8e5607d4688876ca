"""Indexing restated in Python for the tests: document texts -> docs.bin / stats.bin / forward.bin / terms.bin, what the
reference's `forwardindex` tool does from the string it hands to tokenize onwards (include/textutil.hpp:13-37,
src/ForwardIndex.cpp:139-230), with THIS project's term-id rule (include/nextsearch_hip.h, ns_forward_build): term id =
rank of the term's first kept occurrence in the input (document order, then byte position).  The reference numbers terms
in std::unordered_map iteration order instead; nothing downstream reads the numbering.  Test infrastructure only."""
import os
import re
import struct

import numpy as np

_TOKEN = re.compile(rb"[0-9A-Za-z]+")
STOP_WORDS = frozenset(w.encode() for w in (
    "the a an and or of to in for on with by as is are was were be been it this that from at").split())
assert len(STOP_WORDS) == 24
FILES = ("docs.bin", "stats.bin", "forward.bin", "terms.bin")


def tokenize(text):
    """maximal runs of ASCII alnum bytes (isalnum in the C locale), lower-cased; every other byte separates"""
    return [t.lower() for t in _TOKEN.findall(text)]


def kept_tokens(text):
    """:146-147: tokens shorter than 2 bytes and stop words are dropped"""
    return [t for t in tokenize(text) if len(t) >= 2 and t not in STOP_WORDS]


def as_bytes(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


def build(texts):
    """texts: list of bytes -> dict(kept_docs, doc_len, counts, pairs u32[n, 2], terms list of bytes)"""
    term_id, terms = {}, []
    kept_docs, doc_len, counts, pairs = [], [], [], []
    for d, text in enumerate(texts):
        toks = kept_tokens(text)
        if not toks:                                   # :152-155: the document is dropped, later ones move up
            continue
        tf = {}
        for t in toks:
            tid = term_id.get(t)
            if tid is None:
                tid = term_id[t] = len(terms)
                terms.append(t)
            tf[tid] = tf.get(tid, 0) + 1
        kept_docs.append(d)
        doc_len.append(len(toks))
        counts.append(len(tf))
        pairs.extend(sorted(tf.items()))               # :176
    return {"kept_docs": np.asarray(kept_docs, dtype=np.uint32), "doc_len": np.asarray(doc_len, dtype=np.uint32),
            "counts": np.asarray(counts, dtype=np.uint32), "pairs": np.asarray(pairs, dtype=np.uint32).reshape(-1, 2), "terms": terms}


def _s(b):
    return struct.pack("<I", len(b)) + b


def avgdl(doc_len):
    """:186: (float)total_len / (float)n_docs, total_len in u64"""
    return np.float32(int(np.sum(doc_len.astype(np.uint64)))) / np.float32(len(doc_len))


def file_bytes(docs, fwd):
    """docs: list of dicts / 4-tuples (cord_uid, title, json_relpath, text); fwd = build([texts]) -> {file name: bytes}"""
    rows = [[as_bytes(d[k]) for k in ("cord_uid", "title", "json_relpath")] if isinstance(d, dict) else [as_bytes(x) for x in d[:3]] for d in docs]
    n = len(fwd["kept_docs"])
    out = {}
    out["docs.bin"] = struct.pack("<I", n) + b"".join(
        _s(rows[d][0]) + _s(rows[d][1]) + _s(rows[d][2]) + struct.pack("<I", int(dl)) for d, dl in zip(fwd["kept_docs"], fwd["doc_len"]))
    out["stats.bin"] = struct.pack("<I", n) + (np.asarray([avgdl(fwd["doc_len"])], dtype="<f4").tobytes() if n else struct.pack("<f", 0.0))
    parts, at = [struct.pack("<I", n)], 0
    flat = fwd["pairs"].astype("<u4")
    for c in fwd["counts"]:
        parts.append(struct.pack("<I", int(c)))
        parts.append(flat[at:at + int(c)].tobytes())
        at += int(c)
    out["forward.bin"] = b"".join(parts)
    out["terms.bin"] = struct.pack("<I", len(fwd["terms"])) + b"".join(_s(t) for t in fwd["terms"])
    return out


def doc_text(d):
    return as_bytes(d["text"] if isinstance(d, dict) else d[3])


def index_documents(seg_dir, docs):
    """What nsx::index_documents writes; raises when no document survives (nothing is written)."""
    fwd = build([doc_text(d) for d in docs])
    if len(fwd["kept_docs"]) == 0:
        raise RuntimeError("no document has a token left")
    os.makedirs(seg_dir, exist_ok=True)
    files = file_bytes(docs, fwd)
    for name, b in files.items():
        with open(os.path.join(seg_dir, name), "wb") as f:
            f.write(b)
    return fwd


def doc_term_maps(fwd):
    """per kept document {term bytes: tf}"""
    out, at = [], 0
    for c in fwd["counts"]:
        out.append({fwd["terms"][int(t)]: int(tf) for t, tf in fwd["pairs"][at:at + int(c)]})
        at += int(c)
    return out
