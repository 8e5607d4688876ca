"""Pages past the first K, host side (csrc/ns_after_plan.hpp, host/page.hpp): after_last through
tests/after_plan_harness.cpp against the plain tuple comparison of tests/after_ref.py, the cursor's text form through the
host library, and a host-only engine that says no.  No device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import after_ref
import nsbind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")

RANKS = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]
TILES = [(0, 32), (128, 256), (1 << 17, 1 << 18)]
ITEM_POS = 5


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("after_plan") / "after_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "after_plan_harness.cpp")], check=True)
    lib = C.CDLL(so)
    u32, u64 = C.c_uint32, C.c_uint64
    lib.after_last_c.argtypes = [u32] * 6
    lib.after_last_c.restype = u64
    lib.after_last_many.argtypes = [C.c_void_p, u64, C.c_void_p]
    lib.after_last_many.restype = None
    lib.after_all.restype = u64
    lib.after_ord_c.argtypes = [u32]
    lib.after_ord_c.restype = u32
    lib.after_sort_rank_c.argtypes = [u32, C.c_int]
    lib.after_sort_rank_c.restype = u32
    lib.after_in_tile_c.argtypes = [u64]
    return lib


def cursor_docs(lo, hi):
    return [0, (lo - 1) & 0xFFFFFFFF, lo, lo + 1, hi - 2, hi - 1, hi, 0xFFFFFFFF]


def docs_to_test(lo, hi, cdoc):
    """every document of a tile of up to 128; of the large one both ends and the neighbourhood of the cursor"""
    if hi - lo <= 128:
        return range(lo, hi)
    near = {lo, lo + 1, lo + 2, lo + 31, lo + 32, hi - 3, hi - 2, hi - 1, (lo + hi) // 2}
    near |= {d for d in range(cdoc - 2, cdoc + 3) if lo <= d < hi}
    return sorted(near)


def test_after_last_admits_exactly_the_keys_strictly_after_the_cursor(harness):
    """the whole grid: mapped rank x cursor position {before, equal, after the item's} x cursor doc x tile; per document and
    per rank in {r - 1, r, r + 1}: key <= last  ==  the document's place in the order is strictly after the cursor's"""
    cases = [(cr, cpos, cdoc, ITEM_POS, lo, hi) for cr in RANKS for cpos in (ITEM_POS - 1, ITEM_POS, ITEM_POS + 1) for lo, hi in TILES
             for cdoc in cursor_docs(lo, hi)]
    assert len(cases) == 6 * 3 * 3 * 8
    inp = np.array(cases, dtype=np.uint32)
    last = np.zeros(len(cases), dtype=np.uint64)
    harness.after_last_many(inp.ctypes.data, len(cases), last.ctypes.data)
    checked = admitted = 0
    seen = {"zero": 0, "in_tile": 0}
    for (cr, cpos, cdoc, ipos, lo, hi), bound in zip(cases, last.tolist()):
        assert bound == harness.after_last_c(cr, cpos, cdoc, ipos, lo, hi)
        assert bound != harness.after_all() or cr == 0xFFFFFFFF        # ~0 only as "the top rank and everything below"
        cursor = after_ref.position(cr, cpos, cdoc)
        seen["zero"] += bound == 0
        seen["in_tile"] += harness.after_in_tile_c(bound)
        assert bool(harness.after_in_tile_c(bound)) == (cpos == ipos and lo <= cdoc < hi)
        for d in docs_to_test(lo, hi, cdoc):
            for r in (cr - 1, cr, cr + 1):
                if not 0 <= r <= 0xFFFFFFFF:
                    continue
                key = (r << 32) | (~(d - lo) & 0xFFFFFFFF)
                assert key != 0
                want = after_ref.position(r, ipos, d) > cursor
                assert (key <= bound) == want, (hex(cr), cpos, cdoc, lo, hi, "doc", d, "rank", hex(r), hex(bound))
                checked += 1
                admitted += want
    assert checked > 50000 and 0 < admitted < checked
    assert seen["zero"] > 0 and seen["in_tile"] > 0
    # nothing can enter exactly when only lower ranks may and there is none
    assert harness.after_last_c(0, ITEM_POS + 1, 7, ITEM_POS, 0, 32) == 0
    assert harness.after_last_c(0, ITEM_POS, 31, ITEM_POS, 0, 32) != 0 and harness.after_last_c(0, ITEM_POS, 32, ITEM_POS, 0, 32) == 0


def test_the_rank_maps_are_the_kernels(harness):
    bits = [0x00000000, 0x80000000, 0x00000001, 0x3F800000, 0xBF800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0xFFFFFFFF, 0x7FFFFFFF]
    for b in bits:
        assert harness.after_ord_c(b) == after_ref.ord32(b)
    as_float = lambda b: float(np.array([b], np.uint32).view(np.float32)[0])
    finite = [b for b in bits if not np.isnan(as_float(b))]
    by_value = sorted(finite, key=lambda b: (as_float(b), 0 if b & 0x80000000 else 1))          # -0.0 just below +0.0
    assert sorted(finite, key=after_ref.ord32) == by_value
    assert after_ref.ord32(0x80000000) + 1 == after_ref.ord32(0x00000000)
    assert after_ref.ord32(0x7FC00000) > after_ref.ord32(0x7F800000) and after_ref.ord32(0xFFC00000) < after_ref.ord32(0xFF800000)
    for key in (0, 1, 20200101, 0xFFFFFFFE):
        for asc in (False, True):
            assert harness.after_sort_rank_c(key, int(asc)) == after_ref.sort_rank(key, asc)
    assert after_ref.sort_rank(0, True) == after_ref.sort_rank(0, False) == 0 and after_ref.sort_rank(1, True) == 0xFFFFFFFE


def test_page_of_the_restatement():
    rows = [(9, 0, 3, 7, 0), (9, 0, 5, 7, 0), (9, 1, 0, 4, 0), (8, 0, 1, 7, 0), (0, 2, 2, 1, 0)]
    assert after_ref.page(rows, None, 2) == (5, rows[:2])
    assert after_ref.page(rows, (9, 0, 3), 2) == (4, rows[1:3])
    assert after_ref.page(rows, (9, 0, 4), 100) == (4, rows[1:])
    assert after_ref.page(rows, (9, 1, 0xFFFFFFFF), 1) == (2, rows[3:4])
    assert after_ref.page(rows, (0xFFFFFFFF, 0, 0), 0) == (5, rows[:1])
    assert after_ref.page(rows, (0, 2, 2), 5) == (0, [])


# ---- the cursor's text form -----------------------------------------------------------------------------------------------
def test_cursor_text_round_trip():
    assert nsbind.cursor_text((0x41A3C28F, 0, 5121), "s") == "s41a3c28f.0.5121"
    assert nsbind.parse_cursor("s41a3c28f.0.5121", "s") == (0x41A3C28F, 0, 5121)
    for kind in "sd":
        for c in [(0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0x80000000, 12, 299), (0x0000000A, 1, 10), (20200101, 3, 131072)]:
            text = nsbind.cursor_text(c, kind)
            assert text[0] == kind and len(text.split(".")) == 3 and text[1:9] == "%08x" % c[0]
            assert nsbind.parse_cursor(text, kind) == c
    assert nsbind.cursor_text(None, "s") == "" and nsbind.cursor_text(None, "d") == ""


def test_the_empty_string_is_no_cursor():
    assert nsbind.parse_cursor("", "s") is None and nsbind.parse_cursor("", "d") is None


@pytest.mark.parametrize("text, kind, why", [
    ("d41a3c28f.0.5121", "s", "does not fit"),               # the other kind
    ("s41a3c28f.0.5121", "d", "does not fit"),
    ("x41a3c28f.0.5121", "s", "kind letter"),
    ("S41a3c28f.0.5121", "s", "kind letter"),
    ("s41A3C28F.0.5121", "s", "lowercase hex"),               # upper-case hex
    ("s41a3c28.0.5121", "s", "hex"),                          # seven digits
    ("s41a3c28f0.0.5121", "s", r"'\.' expected"),             # nine
    ("s41a3c28f", "s", r"'\.' expected"),                     # missing fields
    ("s41a3c28f.", "s", "position is missing"),
    ("s41a3c28f.0", "s", r"'\.' expected"),
    ("s41a3c28f.0.", "s", "docId is missing"),
    ("s41a3c28f..5", "s", "position is missing"),
    ("s41a3c28f.0.5121 ", "s", "trailing"),                   # a trailing byte
    ("s41a3c28f.0.5121.", "s", "trailing"),
    ("s41a3c28f.0.5121\n", "s", "trailing"),
    (" s41a3c28f.0.5121", "s", "kind letter"),
    ("s41a3c28f.4294967296.1", "s", "overflows"),             # overflow
    ("s41a3c28f.1.4294967296", "s", "overflows"),
    ("s41a3c28f.1.99999999999999999999999", "s", "overflows"),
    ("s41a3c28f.-1.5", "s", "position is missing"),
    ("s41a3c28f.+1.5", "s", "position is missing"),
    ("s41a3c28f.01.5", "s", "leading zero"),
    ("s41a3c28f.1.0x5", "s", "trailing"),
    ("s", "s", "hex"),
])
def test_parse_cursor_is_strict(text, kind, why):
    with pytest.raises(ValueError, match=why):
        nsbind.parse_cursor(text, kind)


def test_the_largest_fields_parse():
    assert nsbind.parse_cursor("dffffffff.4294967295.4294967295", "d") == (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert nsbind.parse_cursor("s00000000.0.0", "s") == (0, 0, 0)


# ---- a host-only engine -----------------------------------------------------------------------------------------------------
def test_a_host_only_engine_answers_no_page_and_says_so(tmp_path):
    index = str(tmp_path / "index")
    nsbind.gen_index(index, 2, 45, 512, 77, False)
    eng = nsbind.Engine(index, -1)
    try:
        with pytest.raises(RuntimeError, match="search_after_batch_flat: no device context"):
            eng.search_after_batch(["t000001 t000002"], 10)
        with pytest.raises(RuntimeError, match="search_after_batch_flat: no device context"):
            eng.search_after_batch(["t000001"], 10, after=[(0x3F800000, 0, 3)], flags=nsbind.NS_FLAG_AND)
        with pytest.raises(RuntimeError, match="search_boolean_after_batch_flat: no device context"):
            eng.search_boolean_after_batch(["+t000001 t000002"], 10, after=[None])
        with pytest.raises(RuntimeError, match="search_sorted_after_batch_flat: no device context"):
            eng.search_sorted_after_batch(["t000001"], 10, after=[(20200101, 1, 0)])
        for mode in ("or", "and", "boolean", "sorted"):
            with pytest.raises(RuntimeError, match="search_page: no device context"):
                eng.search_page_json("t000001", 10, mode=mode)
            body = eng.search_page_json("t000001", 10, mode=mode, check=False)
            assert body.startswith('{\n  "error": "') and "no device context" in body
        # the calls without cursors still say what they said
        with pytest.raises(RuntimeError, match="search_boolean_batch_flat: no device context"):
            eng.search_boolean_batch(["+t000001"], 10)
        with pytest.raises(RuntimeError, match="search_sorted_batch_flat: no device context"):
            eng.search_sorted_batch(["t000001"], 10)
        assert nsbind.parse_cursor("d0134a3a5.1.44", "d") == (0x0134A3A5, 1, 44)
    finally:
        eng.close()
