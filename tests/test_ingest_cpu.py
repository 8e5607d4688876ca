"""Indexing, CPU side: the Python restatement (tests/ingest_ref.py) against what the REAL reference wrote for the
committed corpus (tests/golden/ingest/ingest1.json, tools/gen_golden_ingest.py), and the restatement's file writer
against the inversion oracle's reader.  The fixture sits in a directory of its own: every *.json directly under
tests/golden is taken for a hit-list fixture by conftest.py."""
import base64
import json
import os
import sys

import numpy as np

import ingest_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import invert_oracle  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "ingest", "ingest1.json")


def load_fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def fixture_texts(g):
    return [d["text"].encode("utf-8") for d in g["documents"]]


def test_fixture_holds_the_cases_it_was_built_for():
    g = load_fixture()
    assert os.path.getsize(GOLDEN) <= 260 * 1024
    texts = fixture_texts(g)
    raw = [t for text in texts for t in ingest_ref._TOKEN.findall(text)]
    assert any(t.isupper() and t.isalpha() for t in raw) and any(t.isdigit() for t in raw) and any(len(t) == 1 for t in raw)
    seen = {t.lower() for t in raw}
    assert ingest_ref.STOP_WORDS <= seen
    assert any(t != t.lower() and t.lower() in ingest_ref.STOP_WORDS for t in raw)
    assert any(b >= 0x80 for text in texts for b in text) and any(0 in text for text in texts)
    assert any(len(t) > 5000 for t in raw)
    assert any(text == b"" for text in texts)
    assert any(text and not ingest_ref.kept_tokens(text) and ingest_ref.tokenize(text) for text in texts)   # only dropped tokens
    assert len(g["queries"]) >= 30 and sum(1 for q in g["queries"] if q["hits"]) >= 25


def test_restatement_equals_the_reference_files():
    g = load_fixture()
    fwd = ingest_ref.build(fixture_texts(g))
    files = ingest_ref.file_bytes(g["documents"], fwd)
    assert files["docs.bin"] == base64.b64decode(g["docs_bin_b64"])
    assert files["stats.bin"] == base64.b64decode(g["stats_bin_b64"])
    want = [{k.encode("ascii"): v for k, v in m.items()} for m in g["forward"]]
    assert ingest_ref.doc_term_maps(fwd) == want
    assert set(fwd["terms"]) == set().union(*[set(m) for m in want])
    assert len(fwd["kept_docs"]) < len(g["documents"])                 # some documents are dropped, later ones move up


def test_term_ids_are_first_occurrence_ranks():
    g = load_fixture()
    texts = fixture_texts(g)
    fwd = ingest_ref.build(texts)
    n = len(fwd["terms"])
    assert len(set(fwd["terms"])) == n
    assert sorted(set(int(t) for t in fwd["pairs"][:, 0])) == list(range(n))      # a permutation of 0 .. n_terms - 1 is in use
    order = []
    for text in texts:
        for t in ingest_ref.kept_tokens(text):
            if t not in order:
                order.append(t)
    assert order == fwd["terms"]
    # the reference's own numbering differs (hash-map order) and nothing reads it
    assert g["reference_terms"] != [t.decode() for t in fwd["terms"][:len(g["reference_terms"])]]
    at = 0
    for c in fwd["counts"]:
        ids = fwd["pairs"][at:at + int(c), 0]
        assert np.all(ids[1:] > ids[:-1])
        at += int(c)
    assert at == len(fwd["pairs"]) and int(fwd["pairs"][:, 1].sum()) == int(fwd["doc_len"].sum())


def test_written_files_are_read_back_by_the_inversion_oracle(tmp_path):
    g = load_fixture()
    seg = str(tmp_path / "seg")
    fwd = ingest_ref.index_documents(seg, g["documents"])
    terms = invert_oracle.read_terms(os.path.join(seg, "terms.bin"))
    counts, pairs = invert_oracle.read_forward(os.path.join(seg, "forward.bin"))
    assert terms == fwd["terms"] and np.array_equal(counts, fwd["counts"]) and np.array_equal(pairs, fwd["pairs"])
    n_pairs, kept = invert_oracle.lexicon_tool(seg)
    assert n_pairs == kept == len(fwd["pairs"])                       # no pair is dropped: every term id is in range


def test_tokenizer_rules():
    assert ingest_ref.tokenize(b"Ab\x00cD\xc3\xa9e_f-9Z") == [b"ab", b"cd", b"e", b"f", b"9z"]
    assert ingest_ref.kept_tokens(b"The THE a I x1 of OF to2") == [b"x1", b"to2"]
    fwd = ingest_ref.build([b"ab", b"cd ab", b"", b"the", b"x ab ab"])
    assert list(fwd["kept_docs"]) == [0, 1, 4] and list(fwd["doc_len"]) == [1, 2, 2]
    assert fwd["terms"] == [b"ab", b"cd"] and fwd["pairs"].tolist() == [[0, 1], [0, 1], [1, 1], [0, 2]]
