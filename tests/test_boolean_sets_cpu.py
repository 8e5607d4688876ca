"""Facet counts and date order for boolean queries, host side: the laws of the restatement
tests/boolean_sets_ref.py on the directed inputs of tests/boolean_sets_shapes.py, the floors of the GPU suite's equivalence
checks, the cursor kind of the new page mode through tests/boolean_sets_page_harness.cpp, and a host-only engine that says no.
No device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import after_ref
import boolean_ref
import boolean_sets_ref
import boolean_sets_shapes as shapes
import boolean_shapes
import facet_ref
import nsbind
import sorted_ref
from boolean_ref import MUST, NOT, SHOULD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsearch-api_amd", "host")


@pytest.fixture(scope="module", params=[1, 3])
def directed(request):
    """the directed inputs and the restatement's whole answer, computed once per segment count"""
    segments, queries, idfs, weights, order = shapes.directed_inputs(request.param)
    order = list(range(len(segments))) if order is None else order
    return segments, queries, idfs, weights, order, boolean_ref.boolean_all(segments, queries, order, idfs, weights)


# ---- the restatement's own laws -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_buckets", shapes.BUCKETS)
def test_row_sums_are_the_boolean_searchs_found(directed, n_buckets):
    segments, queries, _, _, order, everything = directed
    for kind in ("modulo", "tile"):
        tables = shapes.tables_for(segments, kind, n_buckets)
        counts = boolean_sets_ref.counts(segments, queries, tables, n_buckets, order)
        assert counts.shape == (len(queries), n_buckets)
        assert [int(x) for x in counts.sum(axis=1)] == [len(rows) for rows in everything]
        # and bucket by bucket it is a count of the boolean search's own documents
        for qi, rows in enumerate(everything):
            want = np.zeros(n_buckets, np.int64)
            for _, s, d in rows:
                want[int(tables[s][d])] += 1
            np.testing.assert_array_equal(counts[qi], want)


def test_the_directed_inputs_hold_every_promised_case(directed):
    """each case of shapes.CASES is among the role mixes, with the matched set its name says"""
    segments, queries, _, _, order, everything = directed
    n_segs = len(segments)
    found = {name: len(everything[shapes.ROLE_MIXES.index(q)]) for name, q in shapes.CASES.items()}
    for name in ("MUST and NOT", "SHOULD and NOT", "NOT alone"):
        assert found[name] == 0, (name, found)
    assert found["MUST count == 0"] == (0 if n_segs == 1 else 128)                 # the group dies in the segments that lack the list
    for name in ("one MUST + NOT", "two MUST + NOT", "three MUST + NOT", "SHOULD + NOT", "NOT empties one tile", "MUST list misses a tile", "MUST and SHOULD",
                 "single positive + NOT"):
        assert found[name] >= 2, (name, found)
    assert found["docId >= n_docs"] == found["single positive"] == 256 * n_segs     # 257 postings, one of them past the segment
    assert found["single positive + NOT"] < found["single positive"]
    # per small tile of 128 documents: the exclusion empties the middle one alone; the MUST list has nothing in the middle one
    lists = segments[0][2]
    tile_of = lambda docs: sorted({int(d) // shapes.SMALL_TILE for d in docs})     # noqa: E731
    q = shapes.CASES["NOT empties one tile"]
    before = boolean_ref.group_matched(lists, [(li, r) for li, r in q if r != NOT], shapes.N_DOCS)
    after = boolean_ref.group_matched(lists, q, shapes.N_DOCS)
    assert tile_of(before) == [0, 1, 2] and tile_of(after) == [0, 2]
    assert tile_of(lists[8][0]) == [0, 2] and tile_of(lists[7][0]) == [1]
    assert sorted({len(q) for q in shapes.ROLE_MIXES}) == [0, 1, 2, 3, 4, 8, 70]
    sizes = [len(r) for r in everything]
    for k in (64, 65, 100):                                                        # found on both sides of every K the kept set treats differently
        assert min(sizes) < k < max(sizes)


def unroled(queries):
    return [[(s, li) for s, li, _ in q] for q in queries]


def test_all_should_is_the_or_count_and_the_or_order(directed):
    segments, queries, idfs, weights, order, _ = directed
    plain = [[(s, li, SHOULD) for s, li, _ in q] for q in queries]
    tables = shapes.tables_for(segments, "modulo", 50)
    np.testing.assert_array_equal(boolean_sets_ref.counts(segments, plain, tables, 50, order), facet_ref.counts(segments, unroled(plain), tables, 50, and_mode=False))
    check_order(segments, plain, idfs, weights, order, and_mode=False)


def test_all_must_over_non_empty_lists_is_the_and_count_and_the_and_order():
    segments, queries, idfs, weights = boolean_shapes.same_role_inputs(MUST)
    assert all(len(d) for s in segments for d, _ in s[2])
    order = [2, 0, 1]
    for B in (1, 50):
        tables = shapes.tables_for(segments, "modulo", B)
        np.testing.assert_array_equal(boolean_sets_ref.counts(segments, queries, tables, B, order), facet_ref.counts(segments, unroled(queries), tables, B, and_mode=True))
    check_order(segments, queries, idfs, weights, order, and_mode=True)


def check_order(segments, queries, idfs, weights, order, and_mode):
    """the date order cut to the first K is sorted_ref.sorted_hits: documents, keys, score bits and found"""
    everything = boolean_ref.boolean_all(segments, queries, order, idfs, weights)
    keys = shapes.keys_for(segments, "pool5")
    cache = {}
    for ascending in (False, True):
        rows = boolean_sets_ref.rows(everything, keys, ascending, order)
        for k in (1, 10, 100):
            want = sorted_ref.sorted_hits(segments, unroled(queries), keys, k, and_mode, ascending, order, idfs, weights, cache)
            for qi, (found, hits) in enumerate(want):
                rest, page = boolean_sets_ref.page(rows[qi], None, k, ascending, order)
                assert rest == found == len(rows[qi]), (qi, k)
                assert [(r[3], r[2], r[4]) for r in page] == [(s, d, kk) for s, d, kk, _ in hits], (qi, k, ascending)
                assert [r[5] for r in page] == [int(np.float32(sc).view(np.uint32)) for _, _, _, sc in hits], (qi, k, ascending)


def test_pages_concatenate_to_the_order_and_a_foreign_cursor_cuts_it(directed):
    segments, queries, _, _, order, everything = directed
    keys = shapes.keys_for(segments, "pool5")
    for ascending in (False, True):
        for rows in boolean_sets_ref.rows(everything, keys, ascending, order)[::5]:
            seen, cursor = [], None
            while True:
                rest, page = boolean_sets_ref.page(rows, cursor, 64, ascending, order)
                assert rest == len(rows) - len(seen)
                if not page:
                    break
                seen += page
                cursor = (page[-1][4], page[-1][3], page[-1][2])
            assert seen == rows and len({(r[3], r[2]) for r in seen}) == len(rows)
            # a cursor that is no document: everything of a smaller rank, or of that rank in a later segment or at a larger docId
            c = (20191231, order[0], 1000)
            rest, page = boolean_sets_ref.page(rows, c, 100, ascending, order)
            t = after_ref.sort_rank(c[0], ascending)
            assert rest == sum(1 for r in rows if r[0] < t or (r[0] == t and r[1] > 0))


def test_the_gpu_suites_equivalence_inputs_clear_their_floors():
    for role in (SHOULD, MUST):
        segments, queries, idfs, weights = boolean_shapes.same_role_inputs(role)
        everything = boolean_ref.boolean_all(segments, queries, [2, 0, 1], idfs, weights)
        assert sum(len(r) >= 2 for r in everything) >= shapes.FLOOR_SAME_ROLE[role]
    small = 0
    for segments, queries, idfs, weights, order in (shapes.directed_inputs(1), shapes.directed_inputs(3), shapes.mixed_inputs()):
        order = list(range(len(segments))) if order is None else order
        small += len(shapes.small_sets(boolean_ref.boolean_all(segments, queries, order, idfs, weights)))
    assert small >= shapes.FLOOR_SMALL_SETS, small


# ---- the page mode ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("boolean_sets_page") / "boolean_sets_page_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I" + HOST, "-o", so,
                    os.path.join(ROOT, "tests", "boolean_sets_page_harness.cpp")], check=True)
    lib = C.CDLL(so)
    lib.page_parse_c.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_char_p, C.c_uint32]
    lib.page_text_c.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32]
    lib.page_text_c.restype = None
    return lib


def parse(lib, text, mode):
    out = np.zeros(4, np.uint32)
    err = C.create_string_buffer(256)
    rc = lib.page_parse_c(text.encode(), mode, out.ctypes.data, err, 256)
    return rc, [int(x) for x in out], err.value.decode()


def test_the_boolean_sorted_mode_pages_with_date_cursors(harness):
    mode = harness.page_mode_boolean_sorted()
    assert mode == 4 == nsbind.PAGE_MODES["boolean_sorted"]
    assert [chr(harness.page_kind_c(m)) for m in range(5)] == ["s", "s", "s", "d", "d"]      # the four older modes keep their kind
    assert parse(harness, "", mode) == (0, [0, 0, 0, 0], "")
    assert parse(harness, "d0134a3a5.1.44", mode) == (0, [1, 0x0134A3A5, 1, 44], "")
    assert parse(harness, "dffffffff.4294967295.4294967295", mode)[1] == [1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]
    rc, out, why = parse(harness, "s41a3c28f.0.5121", mode)
    assert rc == -1 and out[0] == 0 and why == "cursor: a cursor of kind 's' does not fit this call, which pages in date order"
    rc, _, why = parse(harness, "d0134a3a5.1.44", 2)                                          # and a date cursor does not fit the score-ordered boolean mode
    assert rc == -1 and why == "cursor: a cursor of kind 'd' does not fit this call, which pages in score order"
    for text, why in (("d0134A3A5.1.44", "rank is not 8 lowercase hex digits"), ("d0134a3a5.01.44", "position has a leading zero"),
                      ("d0134a3a5.1.44 ", "trailing bytes"), ("d0134a3a5.1", "'.' expected after the position"), ("x0134a3a5.1.44", "the kind letter is neither")):
        rc, out, msg = parse(harness, text, mode)
        assert rc == -1 and out[0] == 0 and why in msg, (text, msg)
    buf = C.create_string_buffer(64)
    for c in ((0, 0, 0), (20200101, 2, 299), (0xFFFFFFFE, 7, 0xFFFFFFFF)):
        harness.page_text_c(mode, *c, buf, 64)
        assert buf.value.decode() == nsbind.cursor_text(c, "d")
        assert parse(harness, buf.value.decode(), mode) == (0, [1] + list(c), "")


# ---- a host-only engine -------------------------------------------------------------------------------------------------
def test_a_host_only_engine_refuses_the_new_entries_and_says_so(tmp_path):
    index = str(tmp_path / "index")
    nsbind.gen_index(index, 2, 45, 512, 77, False)
    eng = nsbind.Engine(index, -1)
    try:
        with pytest.raises(RuntimeError, match="facet_boolean_batch_flat: no device context"):
            eng.facet_boolean_batch(["+t000001 t000002 -t000003"], 8)
        with pytest.raises(RuntimeError, match="search_boolean_sorted_batch_flat: no device context"):
            eng.search_boolean_sorted_batch(["+t000001 t000002"], 10)
        with pytest.raises(RuntimeError, match="search_boolean_sorted_batch_flat: no device context"):
            eng.search_boolean_sorted_batch(["t000001"], 10, after=[(20200101, 1, 0)], order="oldest")
        with pytest.raises(RuntimeError, match="search_boolean_faceted: no device context"):
            eng.search_boolean_faceted_json("+t000001 -t000002", 10)
        with pytest.raises(RuntimeError, match="search_boolean_sorted: no device context"):
            eng.search_boolean_sorted_json("+t000001 -t000002", 10)
        for call in (eng.search_boolean_faceted_json, eng.search_boolean_sorted_json):
            body = call("t000001", 10, check=False)
            assert body.startswith('{\n  "error": "') and "no device context" in body
        with pytest.raises(RuntimeError, match="search_page: no device context"):
            eng.search_page_json("+t000001", 10, mode="boolean_sorted")
        body = eng.search_page_json("+t000001", 10, mode="boolean_sorted", check=False)
        assert body.startswith('{\n  "error": "') and "no device context" in body
    finally:
        eng.close()
