"""Deleting documents, CPU side: the Python restatement of the filter (tests/delete_ref.py) composed with
the merge (tests/compact_ref.py) against what it must equal — indexing the survivors afresh, up to term numbering, and
byte for byte when no surviving term was first seen in a deleted document — and the host entry points where no device is
needed: a host-only engine refuses to delete and touches nothing, and still resolves uids."""
import os
import sys

import numpy as np
import pytest

import compact_ref
import delete_ref
import ingest_ref
import nsbind
from conftest import sha256_tree
from test_ingest_gpu import as_docs, gen_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import invert_oracle  # noqa: E402


def lists_by_term(fwd):
    df, post = invert_oracle.invert(fwd["counts"], fwd["pairs"], len(fwd["terms"]))
    starts = np.concatenate([[0], np.cumsum(df.astype(np.int64))])
    return {t: post[starts[i]:starts[i + 1]].tobytes() for i, t in enumerate(fwd["terms"])}


def assert_equal_up_to_term_numbering(got, one):
    """test_compact_cpu's permuted-sources comparison: per document the same {term: tf}, the same term set, per term string the
    same inverted list, the same doc_len and counts"""
    assert ingest_ref.doc_term_maps(got) == ingest_ref.doc_term_maps(one)
    assert set(got["terms"]) == set(one["terms"]) and len(got["terms"]) == len(one["terms"]) == len(set(got["terms"]))
    assert np.array_equal(got["doc_len"], one["doc_len"]) and np.array_equal(got["counts"], one["counts"])
    assert lists_by_term(got) == lists_by_term(one)
    at = 0
    for c in got["counts"]:                                             # still a well-formed forward index
        ids = got["pairs"][at:at + int(c), 0]
        assert np.all(ids[1:] > ids[:-1])
        at += int(c)


def random_keeps(parts, rate, seed):
    """per part a boolean array; rate 'one': a single survivor in the whole index"""
    rng = np.random.default_rng(seed)
    if rate == "one":
        keeps = [np.zeros(len(p["counts"]), dtype=bool) for p in parts]
        keeps[len(parts) // 2][int(rng.integers(0, len(keeps[len(parts) // 2])))] = True
        return keeps
    return [rng.random(len(p["counts"])) < rate for p in parts]


CORPORA = [(31, 700, 50, (200, 1, 300)), (32, 400, 40, (13, 100, 183)), (33, 291, 30, (29, 98, 96))]


@pytest.mark.parametrize("rate", [0.0, 1.0, "one", 0.5, 0.9, 0.05])
@pytest.mark.parametrize("seed,n_docs,words,sizes", CORPORA)
def test_merge_of_the_filtered_parts_equals_indexing_the_survivors(seed, n_docs, words, sizes, rate):
    texts = gen_corpus(seed, n_docs, words, vocab=700, long_tokens=(1500,))
    docs = as_docs(texts)
    part_docs = compact_ref.cut(docs, sizes)
    parts = [ingest_ref.build([d[3] for d in pd]) for pd in part_docs]
    keeps = random_keeps(parts, rate, seed * 7 + 1)
    got = delete_ref.merge_keep(parts, keeps)
    left = [d for pd, p, k in zip(part_docs, parts, keeps) for d in delete_ref.survivors(pd, p, k)]
    assert len(left) == sum(int(k.sum()) for k in keeps)
    if rate == 0.0:
        assert len(left) == 0 and len(got["doc_len"]) == 0 and got["terms"] == [] and len(got["pairs"]) == 0
        return
    one = ingest_ref.build([d[3] for d in left])
    assert len(one["kept_docs"]) == len(left)                           # every survivor was an indexed document
    assert_equal_up_to_term_numbering(got, one)
    filtered = [delete_ref.filter_part(p, k) for p, k in zip(parts, keeps)]
    files, want = compact_ref.merged_file_bytes(part_docs, filtered, got), ingest_ref.file_bytes(left, one)
    assert files["docs.bin"] == want["docs.bin"] and files["stats.bin"] == want["stats.bin"]
    if rate == 1.0:                                                     # nothing dropped: the plain merge, byte for byte
        plain = compact_ref.merge(parts)
        assert got["terms"] == plain["terms"] and np.array_equal(got["pairs"], plain["pairs"]) and files == want
    elif rate in (0.5, 0.05):
        assert got["terms"] != one["terms"]                             # the numbering really differs: the claim is not vacuous


@pytest.mark.parametrize("seed,n_docs,words,sizes", CORPORA)
def test_byte_identical_when_no_victim_introduces_a_term(seed, n_docs, words, sizes):
    texts = gen_corpus(seed, n_docs, words, vocab=700, long_tokens=(1500,))
    docs = as_docs(texts)
    part_docs = compact_ref.cut(docs, sizes)
    parts = [ingest_ref.build([d[3] for d in pd]) for pd in part_docs]
    rng = np.random.default_rng(seed)
    keeps = []
    for p in parts:
        free = ~delete_ref.introducing_documents(p)                     # documents that introduce no term of their part
        keeps.append(~(free & (rng.random(len(free)) < 0.7)))
    assert sum(int((~k).sum()) for k in keeps) >= 10                    # not vacuous: documents do go (most introduce a term)
    got = delete_ref.merge_keep(parts, keeps)
    left = [d for pd, p, k in zip(part_docs, parts, keeps) for d in delete_ref.survivors(pd, p, k)]
    one = ingest_ref.build([d[3] for d in left])
    assert got["terms"] == one["terms"]
    for k in ("doc_len", "counts", "pairs"):
        assert np.array_equal(got[k], one[k]), k
    filtered = [delete_ref.filter_part(p, k) for p, k in zip(parts, keeps)]
    assert compact_ref.merged_file_bytes(part_docs, filtered, got) == ingest_ref.file_bytes(left, one)


def test_the_filter_does_not_look_at_dropped_documents_and_ignores_dead_duplicates():
    part = ingest_ref.build([b"alpha beta", b"gamma beta delta", b"alpha epsilon"])
    bad = dict(part, pairs=part["pairs"].copy())
    at = int(part["counts"][0])
    bad["pairs"][at, 0] = 99                                            # document 1 names a term that does not exist
    keep = np.array([True, False, True])
    got = delete_ref.filter_part(bad, keep)
    assert got["terms"] == [b"alpha", b"beta", b"epsilon"] and list(got["counts"]) == [2, 2]
    with pytest.raises(AssertionError, match="termId"):
        delete_ref.filter_part(bad, np.array([True, True, False]))
    twice = dict(part, terms=[b"alpha", b"beta", b"gamma", b"alpha", b"epsilon"])   # "delta" renamed: a duplicate byte string
    assert delete_ref.merge_keep([twice], [keep])["terms"] == [b"alpha", b"beta", b"epsilon"]   # the second copy is dead
    with pytest.raises(AssertionError, match="twice"):
        delete_ref.merge_keep([twice], [np.array([True, True, True])])
    words = delete_ref.bitmap(np.array([True, False, True]), garbage_seed=3)
    assert int(words[0]) & 7 == 5 and len(words) == 2


# ---- the host entry points that need no device -------------------------------------------------------------
def make_index(tmp_path, batches):
    """an index directory of complete segments written on the CPU (restatement + inversion oracle)"""
    index = tmp_path / "index"
    names = []
    for i, docs in enumerate(batches):
        name = "seg_%06u" % i
        seg = str(index / "segments" / name)
        compact_ref.write_forward_files(seg, docs, ingest_ref.build([d[3] for d in docs]))
        invert_oracle.lexicon_tool(seg)
        names.append(name.encode())
    with open(index / "manifest.bin", "wb") as f:
        f.write(len(names).to_bytes(4, "little") + b"".join(len(n).to_bytes(4, "little") + n for n in names))
    return str(index)


def three_batches():
    docs = as_docs(gen_corpus(21, 150, 30, vocab=300, long_tokens=()))
    docs = [d for d in docs if ingest_ref.kept_tokens(d[3])]            # docId == position in its batch
    batches = [docs[:40], docs[40:90], docs[90:]]
    dup = batches[0][7][0]
    batches[2][5] = (dup,) + tuple(batches[2][5][1:])                   # one uid twice in the index, in two segments
    batches[2][6] = (dup,) + tuple(batches[2][6][1:])                   # ... and twice in one
    return batches, dup


def test_a_host_only_engine_refuses_to_delete_and_touches_nothing(tmp_path):
    batches, dup = three_batches()
    index = make_index(tmp_path, batches)
    eng = nsbind.Engine(index, -1)
    try:
        before = sha256_tree(index)
        with pytest.raises(RuntimeError, match="host-only engine.*device"):
            eng.delete_documents([dup])
        with pytest.raises(RuntimeError, match="host-only engine.*device"):
            eng.delete_by_id([(0, 1)])
        assert sha256_tree(index) == before and eng.num_segments == 3
    finally:
        eng.close()


def test_find_documents_resolves_uids_on_a_host_only_engine(tmp_path):
    batches, dup = three_batches()
    index = make_index(tmp_path, batches)
    eng = nsbind.Engine(index, -1)
    try:
        assert eng.find_documents([]) == []
        assert eng.find_documents([b"no such uid", "nor this"]) == []
        assert eng.find_documents([batches[1][0][0]]) == [(1, 0)]
        assert eng.find_documents([dup]) == [(0, 7), (2, 5), (2, 6)]
        last = len(batches[2]) - 1
        got = eng.find_documents([batches[2][last][0], b"missing", dup, batches[1][49][0], dup])
        assert got == [(0, 7), (1, 49), (2, 5), (2, 6), (2, last)]      # ascending, duplicates of the request folded
        assert eng.find_documents([dup[:-1]]) == [] and eng.find_documents([dup + b"0"]) == []   # whole uids only
    finally:
        eng.close()
