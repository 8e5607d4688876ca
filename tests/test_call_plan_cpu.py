"""What a ranked call plans between its work items and its device block (csrc/ns_call_plan.hpp):
ranked_call_plan through tests/call_plan_harness.cpp against a restatement in plain Python, on directed shapes.  Every output
is compared exactly and every refusal by its message.  No device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import after_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")

ALL = 0xFFFFFFFFFFFFFFFF
SEG_IDS = [7, 3, 9]                      # the call's segment list: a cursor names an id, an item a position
# (query, segment position, doc_lo, doc_hi): tiles of 32 documents; query 1 has no item, between two that have three
ITEMS = [(0, 0, 0, 32), (0, 0, 32, 50), (0, 1, 0, 32), (2, 0, 0, 32), (2, 0, 32, 50), (2, 2, 0, 20)]
ORD, NEWEST, OLDEST = 0, 1, 2            # the rank maps of the harness


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("call_plan") / "call_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "call_plan_harness.cpp")], check=True)
    lib = C.CDLL(so)
    u32, u64, p = C.c_uint32, C.c_uint64, C.c_void_p
    lib.call_plan.argtypes = [p, u64, u32, u32, p, p, u32, C.c_int, C.c_int, u64, p, p, u64, p, p, C.c_char_p, u32]
    lib.call_plan.restype = C.c_int
    lib.call_item_limit_c.argtypes = [u64, C.c_char_p, u32]
    lib.call_item_limit_c.restype = C.c_int
    lib.call_cand_bytes.restype = u64
    lib.call_max_k.restype = u32
    return lib


def run(lib, items, n_queries, k, cursors, rank_map, reserved, cand_bytes, seg_ids=SEG_IDS):
    """the header's answer as a dict, or the refusal's text"""
    rows = np.array(items, dtype=np.uint32).reshape(-1, 4)
    segs = np.array(seg_ids, dtype=np.uint32)
    cur = None if cursors is None else np.array([c or (0, 0, 0, 0) for c in cursors], dtype=np.uint32)
    q_off = np.full(n_queries + 1, 0xDEADBEEF, dtype=np.uint32)
    cuts = np.zeros((len(items) + n_queries + 1, 4), dtype=np.uint32)
    last = np.zeros(max(len(items), 1), dtype=np.uint64)
    scalars = np.zeros(5, dtype=np.uint64)
    err = C.create_string_buffer(512)
    ok = lib.call_plan(rows.ctypes.data, len(items), n_queries, k, None if cur is None else cur.ctypes.data, segs.ctypes.data, len(seg_ids),
                       rank_map, int(reserved), cand_bytes, q_off.ctypes.data, cuts.ctypes.data, len(cuts), last.ctypes.data,
                       scalars.ctypes.data, err, len(err))
    if not ok:
        return err.value.decode()
    K, paged, n_cuts, n_last, cand_rows = (int(v) for v in scalars)
    return {"K": K, "paged": bool(paged), "q_off": q_off.tolist(), "cuts": [tuple(c) for c in cuts[:n_cuts].tolist()],
            "last": last[:n_last].tolist(), "cand_rows": cand_rows}


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def key_of(rank, slot):
    """a select kernel's key of the document at `slot` of its tile: larger first"""
    return (rank << 32) | (~slot & 0xFFFFFFFF)


def last_of(rank, cpos, cdoc, ipos, lo, hi):
    """the largest key of the tile strictly after the cursor (rank descending, position, docId), 0 when there is none"""
    if (ipos, lo) > (cpos, cdoc):                       # every document of the tile comes after the cursor's at equal rank
        return key_of(rank, 0)
    if (ipos, hi) <= (cpos, cdoc):                      # the tile ends before the cursor's document: lower ranks only
        return key_of(rank - 1, 0) if rank else 0
    return key_of(rank, cdoc + 1 - lo)                  # the tile holds the cursor's document: ties from the next slot on


def plan_ref(items, n_queries, k, cursors, rank_map, reserved, cand_bytes, seg_ids=SEG_IDS):
    K = min(max(k, 1), 100)
    if len(items) >= 1 << 31:
        return "%d work items; cut the batch" % len(items)
    queries = [it[0] for it in items]
    if queries != sorted(queries) or any(q >= n_queries for q in queries):
        return "the work items are not grouped by query"
    q_off = [sum(1 for q in queries if q < b) for b in range(n_queries + 1)]
    rows = cand_bytes // (8 * K)
    cuts, q0 = [], 0
    for q in range(n_queries):
        own = q_off[q + 1] - q_off[q]
        if own > rows:
            return "query %d alone has %d work items; the candidate buffer of %d bytes holds %d rows at K = %d" % (q, own, cand_bytes, rows, K)
        if q_off[q + 1] - q_off[q0] > rows:
            cuts.append((q0, q, q_off[q0], q_off[q]))
            q0 = q
    if n_queries:
        cuts.append((q0, n_queries, q_off[q0], q_off[n_queries]))
    mapped = {ORD: after_ref.ord32, NEWEST: lambda r: after_ref.sort_rank(r, False), OLDEST: lambda r: after_ref.sort_rank(r, True)}[rank_map]
    where = {}
    for q, c in enumerate(cursors or []):
        rank, seg, doc, is_set = c or (0, 0, 0, 0)
        if is_set > 1:
            return "query %d: cursor with set = %d (0 or 1)" % (q, is_set)
        if not is_set:
            continue
        if reserved and rank == 0xFFFFFFFF:
            return "query %d: cursor with the reserved key 0xFFFFFFFF" % q
        if seg not in seg_ids:
            return "query %d: cursor names segment %d, which the call does not list" % (q, seg)
        where[q] = (mapped(rank), seg_ids.index(seg), doc)
    last = [last_of(*where[q], pos, lo, hi) if q in where else ALL for q, pos, lo, hi in items] if where else []
    return {"K": K, "paged": bool(where), "q_off": q_off, "cuts": cuts, "last": last, "cand_rows": max(c[3] - c[2] for c in cuts)}


def both(lib, items, n_queries, k, cursors, rank_map, reserved, cand_bytes=None, seg_ids=SEG_IDS):
    cand_bytes = lib.call_cand_bytes() if cand_bytes is None else cand_bytes
    got = run(lib, items, n_queries, k, cursors, rank_map, reserved, cand_bytes, seg_ids)
    assert got == plan_ref(items, n_queries, k, cursors, rank_map, reserved, cand_bytes, seg_ids)
    return got


# ---- the shapes ------------------------------------------------------------------------------------------------------------------
def test_no_cursor_at_all(harness):
    for cursors in (None, [None, None, None]):          # no array, and an array in which no cursor is set
        got = both(harness, ITEMS, 3, 10, cursors, ORD, False)
        assert got == {"K": 10, "paged": False, "q_off": [0, 3, 3, 6], "cuts": [(0, 3, 0, 6)], "last": [], "cand_rows": 6}


def test_a_query_without_items_between_two_with_items(harness):
    got = both(harness, ITEMS, 3, 10, None, NEWEST, True)
    assert got["q_off"] == [0, 3, 3, 6] and got["cuts"] == [(0, 3, 0, 6)]
    got = both(harness, ITEMS, 5, 10, None, NEWEST, True)          # and two more after the last
    assert got["q_off"] == [0, 3, 3, 6, 6, 6] and got["cuts"] == [(0, 5, 0, 6)]
    got = both(harness, [], 2, 10, [(5, 7, 1, 1), None], NEWEST, True)   # no item at all: paged, and nothing to bound
    assert got["paged"] and got["last"] == [] and got["cuts"] == [(0, 2, 0, 0)] and got["cand_rows"] == 0


@pytest.mark.parametrize("rank_map", [ORD, NEWEST, OLDEST])
def test_a_cursor_on_one_query_of_three(harness, rank_map):
    got = both(harness, ITEMS, 3, 10, [None, None, (5, 7, 40, 1)], rank_map, rank_map != ORD)
    assert got["paged"] and len(got["last"]) == len(ITEMS) and got["last"][:3] == [ALL] * 3
    r = {ORD: 0x80000005, NEWEST: 5, OLDEST: 0xFFFFFFFA}[rank_map]
    assert got["last"][3:] == [((r - 1) << 32) | 0xFFFFFFFF, (r << 32) | (~9 & 0xFFFFFFFF), (r << 32) | 0xFFFFFFFF]
    # the cursor in the second listed segment, on the last document of a tile, and past every document
    for cursor in [(5, 3, 31, 1), (5, 3, 0, 1), (5, 9, 19, 1), (5, 9, 0xFFFFFFFF, 1), (0, 7, 32, 1)]:
        both(harness, ITEMS, 3, 10, [cursor, None, cursor], rank_map, rank_map != ORD)


def test_a_cursor_that_names_an_unlisted_segment_is_refused(harness):
    assert both(harness, ITEMS, 3, 10, [None, None, (5, 5, 40, 1)], NEWEST, True) == "query 2: cursor names segment 5, which the call does not list"
    assert both(harness, ITEMS, 3, 10, [(5, 0, 40, 1), None, None], ORD, False) == "query 0: cursor names segment 0, which the call does not list"
    assert both(harness, ITEMS, 3, 10, [(5, 5, 40, 0), None, None], ORD, False)["paged"] is False     # not set: its fields are not read


def test_set_2_is_refused(harness):
    assert both(harness, ITEMS, 3, 10, [(1, 7, 0, 2), None, (5, 7, 40, 1)], NEWEST, True) == "query 0: cursor with set = 2 (0 or 1)"
    assert both(harness, ITEMS, 3, 10, [None, (0, 0, 0, 0xFFFFFFFF), None], ORD, False) == "query 1: cursor with set = 4294967295 (0 or 1)"


def test_the_reserved_key_with_and_without_reserved_rank(harness):
    cursors = [None, None, (0xFFFFFFFF, 7, 40, 1)]
    for rank_map in (NEWEST, OLDEST):
        assert both(harness, ITEMS, 3, 10, cursors, rank_map, True) == "query 2: cursor with the reserved key 0xFFFFFFFF"
    got = both(harness, ITEMS, 3, 10, cursors, ORD, False)         # a score's bits: ord maps them to 0, below which nothing is
    assert got["last"][3:] == [0, ~9 & 0xFFFFFFFF, 0xFFFFFFFF]
    got = both(harness, ITEMS, 3, 10, [None, None, (0x7FFFFFFF, 7, 40, 1)], ORD, False)    # and the top of the order
    assert got["last"][5] == ALL


def test_k_is_clamped(harness):
    assert harness.call_max_k() == 100
    assert both(harness, ITEMS, 3, 0, None, ORD, False)["K"] == 1
    assert both(harness, ITEMS, 3, 1, None, ORD, False)["K"] == 1
    assert both(harness, ITEMS, 3, 100, None, ORD, False)["K"] == 100
    assert both(harness, ITEMS, 3, 101, None, ORD, False)["K"] == 100
    assert both(harness, ITEMS, 3, 0xFFFFFFFF, None, ORD, False)["K"] == 100
    # the clamped K sizes the rows: at k = 0 a budget of 24 bytes holds three rows of one slot
    assert both(harness, ITEMS, 3, 0, None, ORD, False, cand_bytes=24)["cuts"] == [(0, 2, 0, 3), (2, 3, 3, 6)]


def test_a_small_budget_makes_several_cuts(harness):
    cursors = [None, None, (5, 7, 40, 1)]
    got = both(harness, ITEMS, 3, 10, cursors, NEWEST, True, cand_bytes=3 * 10 * 8)
    assert got["cuts"] == [(0, 2, 0, 3), (2, 3, 3, 6)] and got["cand_rows"] == 3
    assert len(got["last"]) == len(ITEMS)                       # per item of the call, not of a cut
    items = [(q, 0, 32 * t, 32 * t + 32) for q, tiles in enumerate([2, 1, 0, 3, 1, 1]) for t in range(tiles)]
    got = both(harness, items, 6, 7, None, ORD, False, cand_bytes=3 * 7 * 8 + 55)        # three rows and a remainder
    assert got["cuts"] == [(0, 3, 0, 3), (3, 4, 3, 6), (4, 6, 6, 8)] and got["cand_rows"] == 3
    assert both(harness, ITEMS, 3, 10, cursors, NEWEST, True, cand_bytes=2 * 10 * 8) == \
        "query 0 alone has 3 work items; the candidate buffer of 160 bytes holds 2 rows at K = 10"


def test_items_out_of_query_order_and_the_item_limit(harness):
    assert both(harness, [(1, 0, 0, 32), (0, 0, 0, 32)], 2, 10, None, ORD, False) == "the work items are not grouped by query"
    assert both(harness, [(0, 0, 0, 32), (2, 0, 0, 32)], 2, 10, None, ORD, False) == "the work items are not grouped by query"
    err = C.create_string_buffer(128)
    assert harness.call_item_limit_c((1 << 31) - 1, err, len(err)) == 1
    assert harness.call_item_limit_c(1 << 31, err, len(err)) == 0 and err.value == b"2147483648 work items; cut the batch"
    assert harness.call_item_limit_c(5 << 31, err, len(err)) == 0 and err.value == b"10737418240 work items; cut the batch"


def test_the_harness_program_runs_the_same_shapes(tmp_path):
    exe = str(tmp_path / "call_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-DCALL_PLAN_MAIN", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "call_plan_harness.cpp")],
                   check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip().endswith("call_plan_harness: 0 wrong")
