"""The digit plan of the radix sort (csrc/ns_radix_plan.hpp through tests/radix_plan_harness.cpp) against its restatement in
tests/radix_shapes.py, and the case table of that module: every case built, the oracle run on it, the oracle checked a second
way, and the reach flags of the whole table asserted complete.  No device is touched; tests/test_radix_shapes_gpu.py runs the
same table through the kernels."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ingest_ref
import nsbind
import radix_shapes as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "radix_plan_harness.cpp")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import invert_oracle  # noqa: E402

RANGES = sorted({min(max(v, 1), 0xFFFFFFFE) for k in range(33) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1)} | set(range(1, 5001)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("radix_plan") / "radix_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I" + CSRC, "-o", so, HARNESS], check=True)
    lib = C.CDLL(so)
    lib.radix_plan_c.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    lib.radix_plan_c.restype = C.c_uint32
    return lib


def header_plan(lib, key_range):
    pb, bits = (C.c_uint32 * 3)(), C.c_uint32()
    passes = lib.radix_plan_c(key_range, pb, C.byref(bits))
    assert list(pb)[passes:] == [8] * (3 - passes)
    return bits.value, list(pb)[:passes]


def test_the_header_plan_equals_the_restatement(harness):
    assert len(RANGES) > 5000 and RANGES[0] == 1 and RANGES[-1] == 0xFFFFFFFE
    for key_range in RANGES:
        bits, digits = header_plan(harness, key_range)
        assert (bits, digits) == rs.plan(key_range), key_range
        assert bits == max(1, (key_range - 1).bit_length())
        assert 1 <= len(digits) <= 3 and all(8 <= d <= 11 for d in digits), key_range
        assert sum(digits) >= bits, key_range
        if len(digits) == 1:
            assert sum(digits) <= bits + 7, key_range
        assert all(sum(digits) - d < bits for d in digits), key_range          # no pass to spare


def test_the_plans_the_cases_are_named_for(harness):
    table = {256: [8], 257: [9], 512: [9], 1024: [10], 2048: [11], 2049: [8, 8], 65536: [8, 8], 1 << 17: [9, 8], 1 << 18: [9, 9], 1 << 19: [10, 9],
             1 << 20: [10, 10], 1 << 21: [11, 10], 1 << 22: [11, 11], (1 << 22) + 1: [8, 8, 8], 1 << 24: [8, 8, 8], (1 << 24) + 1: [9, 8, 8], 1 << 25: [9, 8, 8],
             70000: [9, 8], 1: [8], 0: [8]}
    for key_range, digits in table.items():
        assert header_plan(harness, key_range)[1] == digits == rs.plan(key_range)[1], key_range
    for n_terms, digits in rs.INSTANTIATION_TERMS:
        assert header_plan(harness, n_terms)[1] == digits


def test_the_library_exports_the_same_plan_and_its_tile(harness):
    L = nsbind.hip_lib()                             # the getters touch no device
    assert L.ns_radix_tile() >= 1024 and L.ns_radix_tile() % 256 == 0
    for key_range in RANGES[::7] + [n for n, _ in rs.INSTANTIATION_TERMS] + [rs.DOC_TERMS, rs.DROP_TERMS, rs.SCAN_TERMS]:
        pb = (C.c_uint32 * 3)()
        passes = L.ns_radix_plan(key_range, pb)
        assert list(pb)[:passes] == rs.plan(key_range)[1], key_range


def python_sorted_oracle(case):
    """the inversion a second way: Python's sorted on (term, input index)"""
    doc = [d for d, c in enumerate(case.counts.tolist()) for _ in range(c)]
    rows = sorted((t, i) for i, (t, _) in enumerate(case.pairs.tolist()) if t < case.n_terms)
    df = [0] * case.n_terms
    for t, _ in rows:
        df[t] += 1
    return df, [[doc[i], case.pairs[i, 1]] for _, i in rows]


def test_the_case_table_reaches_every_flag_and_the_oracle_holds():
    T = int(nsbind.hip_lib().ns_radix_tile())
    cases = rs.all_cases(T)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert {c.name for c in rs.small_cases(T)} | {c.name for c in rs.huge_cases(T)} | {c.name for c in rs.scan_cases(T)} == set(names)
    reached, checked_twice = {}, []
    for c in cases:
        n = len(c.pairs)
        assert c.counts.dtype == np.uint32 and c.pairs.dtype == np.uint32 and c.pairs.shape == (n, 2) and int(c.counts.sum()) == n, c.name
        assert np.array_equal(c.pairs[:, 1], np.arange(n, dtype=np.uint32)), c.name      # tf = the pair's index
        df, postings = invert_oracle.invert(c.counts, c.pairs, c.n_terms)
        if n < 20000:
            df2, post2 = python_sorted_oracle(c)
            assert df.tolist() == df2 and postings.tolist() == post2, c.name
            checked_twice.append(c.name)
        for flag in rs.reach(c, T, df, postings):
            reached.setdefault(flag, []).append(c.name)
        print(c.name, n, c.n_terms, rs.plan(c.n_terms)[1])
    # every case but the two scan sizes has fewer than 20 000 pairs and was checked twice, the three-pass cases included
    assert checked_twice == [c.name for c in rs.small_cases(T) + rs.huge_cases(T)] and len(checked_twice) == len(cases) - 2 == 37
    assert sorted(reached) == sorted(rs.FLAGS), (sorted(set(rs.FLAGS) - set(reached)), sorted(set(reached) - set(rs.FLAGS)))
    # the cases built for a flag reach it themselves
    for flag, name in (("scan_top_one_round_full", "scan_one_round_full"), ("scan_top_two_rounds", "scan_two_rounds"), ("third_pass", "inst_%d" % ((1 << 24) + 1)),
                       ("inst(8,F,F)", "inst_%d" % ((1 << 22) + 1)), ("tile_no_doc_start", "doc_over_whole_tiles"), ("doc_starts_on_tile_pair0", "doc_of_T_then_doc_on_pair0"),
                       ("gt256_starts_in_tile", "T_docs_of_one_pair"), ("empties_leading", "runs_of_empty_docs"), ("empties_on_tile_boundary", "runs_of_empty_docs"),
                       ("empties_trailing", "runs_of_empty_docs"), ("n_lt_64", "n_1"), ("n_lt_64", "n_63"), ("one_digit_tile", "one_term_of_one"),
                       ("one_digit_tile", "one_term_of_70000"), ("one_digit_tile", "one_term_per_tile"), ("equal_pairs_across_lane_group", "equal_pairs"),
                       ("equal_pairs_across_wave", "equal_pairs"), ("equal_pairs_across_tile", "equal_pairs"), ("tile_all_dropped_first", "first_tile_dropped"),
                       ("tile_all_dropped_middle", "middle_tile_dropped"), ("tile_all_dropped_last", "last_tile_dropped"), ("later_pass_tile_past_kept", "kept_2T_of_4T"),
                       ("later_pass_tile_past_kept", "one_kept"), ("kept_zero_multi_pass", "all_dropped"), ("run_seam_at_thread_boundary", "run_seams")):
        assert name in reached[flag], (flag, reached[flag])
    for r in range(4):
        assert "kept_mod4_%d" % r in reached["kept_mod4_%d" % r]
    for r in ("1", "63", "64", "65"):
        assert "last_tile_of_" + r in reached["partial_last_tile_" + r]
    assert "last_tile_of_%d" % (T - 1) in reached["partial_last_tile_T-1"]


def test_the_instantiation_cases_spread_every_digit():
    T = int(nsbind.hip_lib().ns_radix_tile())
    for c in rs.instantiation_cases(T):
        ids = c.pairs[:, 0].astype(np.int64)
        _, digits = rs.plan(c.n_terms)
        assert len(ids) == 3 * T + 17 and ids.min() == 0 and ids.max() == c.n_terms - 1, c.name
        for b, sh in zip(digits, rs.shifts(digits)):
            d = (ids >> sh) & ((1 << b) - 1)
            assert d.min() == 0 and d.max() == min((1 << b) - 1, (c.n_terms - 1) >> sh), (c.name, sh)
            rest = ids & ~(((1 << b) - 1) << sh)                 # two ids that differ in this digit only
            order = np.lexsort((d, rest))
            assert np.any((rest[order][1:] == rest[order][:-1]) & (d[order][1:] != d[order][:-1])), (c.name, sh)


def test_the_dropped_cases_drop_what_they_say():
    T = int(nsbind.hip_lib().ns_radix_tile())
    by_name = {c.name: c for c in rs.dropped_cases(T)}
    for c in by_name.values():
        ids = c.pairs[:, 0]
        assert c.n_terms == rs.DROP_TERMS and set(ids[ids >= c.n_terms].tolist()) <= set(rs.BAD_IDS(c.n_terms)), c.name
    kept = {name: int((c.pairs[:, 0] < c.n_terms).sum()) for name, c in by_name.items()}
    assert kept["all_dropped"] == 0 and kept["one_kept"] == 1 and kept["kept_2T_of_4T"] == 2 * T and len(by_name["kept_2T_of_4T"].pairs) == 4 * T
    assert [kept["kept_mod4_%d" % r] % 4 for r in range(4)] == [0, 1, 2, 3]
    ids = by_name["every_second_dropped"].pairs[:, 0]
    assert (ids[0::2] < rs.DROP_TERMS).all() and (ids[1::2] >= rs.DROP_TERMS).all()
    assert set(ids[1::2].tolist()) == set(rs.BAD_IDS(rs.DROP_TERMS))
    up = rs.upload_case(T)
    good = up.pairs[:, 0] < up.n_terms
    assert not good[:T].any() and not good[-T:].any() and good[T:-T].all() and len(good) == 4 * T


def test_the_ingest_corpora_have_the_plans_they_are_named_for():
    for name, texts, by_term, by_doc in rs.ingest_corpora():
        fwd = ingest_ref.build(texts)
        assert rs.plan(len(fwd["terms"]))[1] == by_term and rs.plan(len(texts))[1] == by_doc, name
        assert 0 < len(fwd["kept_docs"]) <= len(texts)
    n_docs = (1 << 22) + 1
    ids, texts = rs.sparse_corpus(n_docs)
    digits = rs.plan(n_docs)[1]
    assert digits == [8, 8, 8] and ids[0] == 0 and ids[-1] == n_docs - 1 and len(ids) == len(texts) >= 1900
    for b, sh in zip(digits, rs.shifts(digits)):
        assert len(np.unique((ids >> sh) & ((1 << b) - 1))) >= 60                 # the ids differ in every digit
    offs = rs.sparse_offsets(n_docs, ids, texts)
    assert len(offs) == n_docs + 1 and offs[0] == 0 and int(offs[-1]) == sum(len(t) for t in texts)
    assert np.array_equal(np.flatnonzero(np.diff(offs.astype(np.int64))), ids)


def test_building_the_non_empty_documents_alone_is_building_all():
    """what the three-pass GPU test relies on: ingest_ref.build over the non-empty documents, kept_docs mapped back through their
    indices, equals build over every document"""
    ids, texts = rs.sparse_corpus(500, 120, seed=4)
    assert 50 < len(ids) < 500
    every = [b""] * 500
    for i, t in zip(ids, texts):
        every[int(i)] = t
    full, part = ingest_ref.build(every), ingest_ref.build(texts)
    assert np.array_equal(full["kept_docs"], ids[part["kept_docs"]])
    for k in ("doc_len", "counts", "pairs"):
        assert np.array_equal(full[k], part[k]), k
    assert full["terms"] == part["terms"]


def test_the_harness_program_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "radix_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DRADIX_PLAN_MAIN",
                    "-I" + CSRC, "-o", exe, HARNESS], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("ranges, 0 wrong")
