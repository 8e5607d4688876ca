"""The case table of tests/ingest_shapes.py through the kernels of csrc/ns_ingest.hip (ns_forward_build), through the same
dictionary kernels with every probe colliding (the variants build with the hash narrowed to 0 bits, in a child process),
through compaction's dictionary stage (ns_forward_merge over the two halves of a case) and, for the sweep, through
nsx::index_documents to the four files.  Which paths the cases take is asserted on the CPU (tests/test_ingest_shapes_cpu.py);
here every comparison is exact, on integers and bytes, the raw token count included."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":   # the child process of test_dict_and_long_with_every_probe_colliding
    sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import compact_ref  # noqa: E402
import ingest_ref  # noqa: E402
import ingest_shapes as S  # noqa: E402
import nsbind  # noqa: E402

pytestmark = pytest.mark.gpu
VARIANTS_LIB = os.path.join(ROOT, "nextsearch-api_amd", "libnextsearch_hip_variants.so")


@pytest.fixture(scope="module")
def ctx():
    L = nsbind.hip_lib()
    h = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(h)) == 0
    yield h
    L.ns_ctx_destroy(h)


def assert_case(ctx, case):
    got = nsbind.forward_build_raw(ctx, case.blob, case.offs)
    want, o = ingest_ref.build(S.texts_of(case)), S.oracle(case)
    info = got["info"]
    assert info["n_tokens"] == o["n_tokens"], (case.name, "raw tokens", info["n_tokens"], o["n_tokens"])
    assert info["kept_tokens"] == o["kept_tokens"] == int(want["doc_len"].sum()), (case.name, "kept tokens")
    assert info["n_docs"] == len(case.offs) - 1 and info["kept_docs"] == len(want["kept_docs"]), (case.name, "documents")
    assert info["n_terms"] == len(want["terms"]) and info["n_pairs"] == len(want["pairs"]), (case.name, "terms, pairs")
    for k in ("kept_docs", "doc_len", "counts", "pairs"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (case.name, k)
    assert got["terms"] == want["terms"] == o["terms"], case.name


@pytest.mark.parametrize("group", S.GROUPS)
def test_every_case_equals_the_restatement(ctx, group):
    cases = S.cases_of(group)
    assert cases
    for case in cases:
        assert_case(ctx, case)


def _child():
    assert "variants" in os.path.basename(nsbind.HIP_LIB_PATH) and os.environ["NS_INGEST_HASH_BITS"] == "0"
    L = nsbind.hip_lib()
    h = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(h)) == 0
    try:
        for case in S.cases_of("dict") + S.cases_of("long"):
            assert_case(h, case)
            print("narrowed:", case.name, flush=True)
    finally:
        L.ns_ctx_destroy(h)


def test_dict_and_long_with_every_probe_colliding():
    """NS_INGEST_HASH_BITS=0 in the variants build: every term's home is slot 0, a term is found after as many probes as there are
    terms in front of it, and only the byte comparison tells terms apart (the siblings of a long token too).  Same answers."""
    assert os.path.exists(VARIANTS_LIB), "libnextsearch_hip_variants.so is missing: make -C nextsearch-api_amd variants"
    env = dict(os.environ, NS_HIP_LIB=VARIANTS_LIB, NS_INGEST_HASH_BITS="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("narrowed:") == len(S.cases_of("dict") + S.cases_of("long"))


@pytest.mark.parametrize("group", ["long", "dict"])
def test_the_halves_of_a_case_through_compaction(ctx, group):
    """k_cp_hash's switch at 1024 / 1025 bytes and the wrap in the shared k_ig_insert: the boundary-length terms and the terms
    whose home is the table's last slot are in both sources (tests/test_ingest_shapes_cpu.py asserts it)"""
    for case in S.cases_of(group):
        parts = [ingest_ref.build(h) for h in S.halves(case)]
        want = compact_ref.merge(parts)
        got = nsbind.forward_merge(ctx, parts)
        assert got["terms"] == want["terms"], case.name
        for k in ("doc_len", "counts", "pairs"):
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (case.name, k)
        assert np.array_equal(got["kept_docs"], np.arange(len(want["doc_len"]), dtype=np.uint32)), case.name
        assert got["info"]["n_terms"] == len(want["terms"]) and got["info"]["n_pairs"] == len(want["pairs"]), case.name


def test_the_sweep_end_to_end_to_the_four_files(tmp_path):
    case = S.case_by_name("sweep")
    docs = [(b"uid%05d" % i, b"Title %d" % i, b"pdf_json/%05d.json" % i, t) for i, t in enumerate(S.texts_of(case))]
    seg = str(tmp_path / "sweep")
    st = nsbind.index_documents(seg, docs)
    o = S.oracle(case)
    want = ingest_ref.file_bytes(docs, ingest_ref.build(S.texts_of(case)))
    for fn in ingest_ref.FILES:
        with open(os.path.join(seg, fn), "rb") as f:
            got = f.read()
        assert len(got) == len(want[fn]) and got == want[fn], fn
    assert st["tokens"] == o["n_tokens"] and st["kept_tokens"] == o["kept_tokens"] and st["n_terms"] == len(o["terms"])
    assert st["n_docs"] == len(o["kept_docs"]) and st["pairs"] == len(o["pairs"])


if __name__ == "__main__":
    _child()
