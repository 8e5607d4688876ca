"""Compaction, CPU side: the Python restatement of the merge (tests/compact_ref.py) against the one-shot
build it must equal — the oracle the GPU tests lean on is itself checked here — and the host entry points' behaviour
where no device is needed: a host-only engine refuses, unreadable sources are named before any device is touched."""
import os
import sys

import numpy as np
import pytest

import compact_ref
import ingest_ref
import nsbind
from conftest import sha256_tree
from test_ingest_gpu import as_docs, gen_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import invert_oracle  # noqa: E402


def corpus_with_shared_long_terms(seed, n_docs, words):
    """gen_corpus + two terms of more than 1024 bytes that occur in the first, a middle and the last document"""
    texts = gen_corpus(seed, n_docs, words, vocab=800, long_tokens=())
    rng = np.random.default_rng(seed + 1)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)
    for ln in (1025, 3000):
        big = bytes(rng.choice(letters, ln))
        for at in (0, n_docs // 2, n_docs - 1):
            texts[at] = texts[at] + b" " + big.upper() + b" "
    return texts


# (seed, documents, words per document, sizes of all parts but the last)
CUTS = [
    (11, 900, 60, (300, 1, 250, 149)),                # a one-document part
    (12, 400, 40, (13, 100, 1, 183)),                 # document 13 is empty: the second part's first document is dropped
    (13, 97 * 3, 30, (29, 98, 1, 96)),                # the second part starts with a document of dropped tokens only
]


@pytest.mark.parametrize("seed,n_docs,words,sizes", CUTS)
def test_merge_of_the_parts_equals_the_one_shot_build(seed, n_docs, words, sizes):
    texts = corpus_with_shared_long_terms(seed, n_docs, words)
    part_texts = compact_ref.cut(texts, sizes)
    assert sum(len(p) for p in part_texts) == n_docs and any(len(p) == 1 for p in part_texts)
    parts = [ingest_ref.build(p) for p in part_texts]
    if seed != 11:
        assert any(len(p["kept_docs"]) and p["kept_docs"][0] != 0 for p in parts[1:])   # a part whose first document is dropped
    shared = set(parts[0]["terms"]) & set(parts[-1]["terms"])
    assert sum(1 for t in shared if len(t) > 1024) >= 2
    merged = compact_ref.merge(parts)
    one = ingest_ref.build(texts)
    assert merged["terms"] == one["terms"]
    for k in ("doc_len", "counts", "pairs"):
        assert np.array_equal(merged[k], one[k]), k
    assert ingest_ref.avgdl(merged["doc_len"]).tobytes() == ingest_ref.avgdl(one["doc_len"]).tobytes()
    docs = as_docs(texts)
    part_docs = compact_ref.cut(docs, sizes)
    assert compact_ref.merged_file_bytes(part_docs, parts, merged) == ingest_ref.file_bytes(docs, one)
    changed = compact_ref.docs_whose_order_changes(parts)
    assert changed[0] == 0 and sum(changed[1:]) > 0                   # the re-sort inside the documents is real work


def test_permuted_sources_merge_to_the_same_index_up_to_term_numbering(tmp_path):
    seed, n_docs, words, sizes = CUTS[0]
    texts = corpus_with_shared_long_terms(seed, n_docs, words)
    parts = [ingest_ref.build(p) for p in compact_ref.cut(texts, sizes)]
    permuted = [compact_ref.permute(p, 100 + i) if i % 2 == 0 else p for i, p in enumerate(parts)]
    assert permuted[0]["terms"] != parts[0]["terms"]
    for p in permuted:                                                  # still a well-formed forward index
        at = 0
        for c in p["counts"]:
            ids = p["pairs"][at:at + int(c), 0]
            assert np.all(ids[1:] > ids[:-1])
            at += int(c)
    merged = compact_ref.merge(permuted)
    one = ingest_ref.build(texts)
    assert ingest_ref.doc_term_maps(merged) == ingest_ref.doc_term_maps(one)
    assert set(merged["terms"]) == set(one["terms"]) and len(merged["terms"]) == len(one["terms"])
    assert np.array_equal(merged["doc_len"], one["doc_len"])

    def lists(fwd):
        df, post = invert_oracle.invert(fwd["counts"], fwd["pairs"], len(fwd["terms"]))
        starts = np.concatenate([[0], np.cumsum(df.astype(np.int64))])
        return {t: post[starts[i]:starts[i + 1]].tobytes() for i, t in enumerate(fwd["terms"])}

    assert lists(merged) == lists(one)


def make_index(tmp_path, n_segments=2):
    """an index directory of complete segments written on the CPU (restatement + inversion oracle)"""
    index = tmp_path / "index"
    texts = gen_corpus(21, 60 * n_segments, 30, vocab=300, long_tokens=())
    names = []
    for i in range(n_segments):
        name = "seg_%06u" % i
        seg = str(index / "segments" / name)
        compact_ref.write_forward_files(seg, as_docs(texts[60 * i:60 * (i + 1)]), ingest_ref.build(texts[60 * i:60 * (i + 1)]))
        invert_oracle.lexicon_tool(seg)
        names.append(name.encode())
    with open(index / "manifest.bin", "wb") as f:
        f.write(len(names).to_bytes(4, "little") + b"".join(len(n).to_bytes(4, "little") + n for n in names))
    return str(index)


def test_a_host_only_engine_refuses_and_touches_nothing(tmp_path):
    index = make_index(tmp_path)
    eng = nsbind.Engine(index, -1)
    try:
        before = sha256_tree(index)
        with pytest.raises(RuntimeError, match="host-only engine"):
            eng.compact()
        assert sha256_tree(index) == before and eng.num_segments == 2
    finally:
        eng.close()


def test_a_missing_terms_file_is_named_and_nothing_is_written(tmp_path):
    index = make_index(tmp_path)
    segs = [os.path.join(index, "segments", "seg_%06u" % i) for i in range(2)]
    os.remove(os.path.join(segs[1], "terms.bin"))
    before = sha256_tree(index)
    out = str(tmp_path / "merged")
    with pytest.raises(RuntimeError, match=r"seg_000001.terms\.bin"):
        nsbind.merge_segments(segs, out, device=0)                      # fails on the host, before a device context is made
    assert not os.path.exists(out) and sha256_tree(index) == before
    with open(os.path.join(segs[1], "terms.bin"), "wb") as f:         # and a truncated one
        f.write(b"\x05\x00\x00\x00\x03\x00\x00\x00ab")
    with pytest.raises(RuntimeError, match=r"terms\.bin: truncated"):
        nsbind.merge_segments(segs, out, device=0)
    assert not os.path.exists(out)
