"""Facet counts, host side (host/facet.hpp, Engine::facet_buckets, csrc/ns_facet_plan.hpp): the bucket tables
and labels of a small dated index on a host-only engine, their round trip with the date filter, and the planner's tiles
through tests/facet_plan_harness.cpp.  No device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_ref
import nsbind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
NS_E_INVAL = -1

N_SEG, N_PER_SEG = 2, 45
# the publish_time of document i (of all segments, in manifest order) is DATES[i % 9]; None: no metadata row
DATES = ["2019", "2020-03", "2020-03-15", "2020 Mar", "", None, "2021-11-02", "2020-04", "2019-12-31"]


def date_of(i):
    return DATES[i % len(DATES)]


def write_metadata(index, date_fn, n):
    lines = ["cord_uid,title,publish_time,authors,url"]
    for i in range(n):
        t = date_fn(i)
        if t is not None:
            lines.append('u%08d,Title %d,"%s",A B,http://x/%d' % (i, i, t, i))
    with open(os.path.join(index, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def dated(tmp_path_factory):
    index = str(tmp_path_factory.mktemp("facet_cpu") / "index")
    nsbind.gen_index(index, N_SEG, N_PER_SEG, 512, 77, False)
    write_metadata(index, date_of, N_SEG * N_PER_SEG)
    eng = nsbind.Engine(index, -1)
    yield eng
    eng.close()


def test_year_buckets_and_labels(dated):
    tables, labels = dated.facet_buckets("year")
    assert labels == ["", "2019", "2020", "2021"]
    want = {"2019": 1, "2020-03": 2, "2020-03-15": 2, "2020 Mar": 0, "": 0, None: 0, "2021-11-02": 3, "2020-04": 2, "2019-12-31": 1}
    assert len(tables) == N_SEG
    for s in range(N_SEG):
        assert tables[s].dtype == np.uint16 and len(tables[s]) == N_PER_SEG
        assert [int(b) for b in tables[s]] == [want[date_of(s * N_PER_SEG + d)] for d in range(N_PER_SEG)]


def test_month_buckets_and_labels(dated):
    tables, labels = dated.facet_buckets("month")
    # a document dated only "2019" has the value 201900: a bucket of its own, labelled "2019", in front of 2019's months
    assert labels == ["", "2019", "2019-12", "2020-03", "2020-04", "2021-11"]
    want = {"2019": 1, "2020-03": 3, "2020-03-15": 3, "2020 Mar": 0, "": 0, None: 0, "2021-11-02": 5, "2020-04": 4, "2019-12-31": 2}
    for s in range(N_SEG):
        assert [int(b) for b in tables[s]] == [want[date_of(s * N_PER_SEG + d)] for d in range(N_PER_SEG)]


def test_bucket_zero_is_the_undated_documents(dated):
    for kind in ("year", "month"):
        tables, _ = dated.facet_buckets(kind)
        for s in range(N_SEG):
            undated = [date_of(s * N_PER_SEG + d) in ("2020 Mar", "", None) for d in range(N_PER_SEG)]
            assert [int(b) == 0 for b in tables[s]] == undated
    # what keep_undated adds to an empty range (2030 .. 2030 keeps no dated document)
    tables, _ = dated.facet_buckets("year")
    bits = dated.filter_bits("2030", "2030", True)
    for s in range(N_SEG):
        np.testing.assert_array_equal(filter_ref.keep_of(bits[s], N_PER_SEG), tables[s] == 0)


def test_a_year_bucket_is_what_the_years_filter_keeps(dated):
    tables, labels = dated.facet_buckets("year")
    assert len(labels) > 1
    for b, y in enumerate(labels):
        if b == 0:
            continue
        bits = dated.filter_bits(y, y, False)
        for s in range(N_SEG):
            np.testing.assert_array_equal(filter_ref.bits_of(tables[s] == b), bits[s], err_msg=str((y, s)))


def test_custom_buckets_are_taken_as_given_and_checked(dated):
    custom = [np.arange(N_PER_SEG, dtype=np.uint16) % 3, np.full(N_PER_SEG, 2, np.uint16)]
    tables, labels = dated.facet_buckets("custom", custom=custom, labels=["none", "a", "b"])
    assert labels == ["none", "a", "b"]
    for s in range(N_SEG):
        np.testing.assert_array_equal(tables[s], custom[s])
    with pytest.raises(RuntimeError, match="names bucket 2 of 2"):
        dated.facet_buckets("custom", custom=custom, labels=["none", "a"])
    with pytest.raises(RuntimeError, match="1 bucket arrays for 2 segments"):
        dated.facet_buckets("custom", custom=[custom[0]], labels=["none", "a", "b"])
    with pytest.raises(RuntimeError, match="1 to 1024 buckets"):
        dated.facet_buckets("custom", custom=custom, labels=["l%d" % i for i in range(1025)])


def test_a_host_only_engine_counts_nothing_and_says_so(dated):
    with pytest.raises(RuntimeError, match="no device context"):
        dated.facet_batch(["t000001"], 4, "year")
    with pytest.raises(RuntimeError, match="no device context"):
        dated.search_faceted_json("t000001", 10, "year")
    body = dated.search_faceted_json("t000001", 10, "year", check=False)
    assert body.startswith('{\n  "error": "') and "no device context" in body
    assert dated.facet_tables_on_device() == 0


def test_1024_distinct_months_fail_and_1023_fit(tmp_path):
    index = str(tmp_path / "index")
    nsbind.gen_index(index, 1, 1024, 512, 78, False)
    month = lambda i: "%04d-%02d" % (1900 + i // 12, 1 + i % 12)
    write_metadata(index, month, 1024)
    eng = nsbind.Engine(index, -1)
    try:
        with pytest.raises(RuntimeError, match="1024 distinct values"):
            eng.facet_buckets("month")
        tables, labels = eng.facet_buckets("year")            # the same documents have 86 distinct years
        assert len(labels) == 1 + 86 and labels[1] == "1900" and labels[-1] == "1985"
        write_metadata(index, lambda i: month(i) if i < 1023 else "", 1024)
        eng.reload()
        tables, labels = eng.facet_buckets("month")
        assert len(labels) == 1024 and labels[0] == "" and labels[1] == "1900-01" and labels[1023] == month(1022)
        assert [int(b) for b in tables[0]] == list(range(1, 1024)) + [0]
    finally:
        eng.close()


# ---- the planner -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("facet_plan") / "facet_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "facet_plan_harness.cpp")], check=True)
    lib = C.CDLL(so)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.facet_plan.argtypes = [vp, u32, vp, u32, u32, vp, vp, vp, u32, u32, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64), C.c_char_p, u32]
    lib.facet_product_tile.restype = u32
    return lib


def plan(harness, queries, seg_ids, n_docs, n_postings, tile, and_mode=False):
    """queries: lists of (seg_id, first posting, count) -> (rc, items (n, 6), refs (m, 4), message)"""
    qd = np.zeros(len(queries), dtype=nsbind.QDESC_DTYPE)
    refs = []
    for qi, q in enumerate(queries):
        qd[qi] = (len(refs), len(q))
        refs += [(s, c, first * 8, 1.0, 1.0) for s, first, c in q]
    refs = np.array(refs, dtype=nsbind.TERM_DTYPE) if refs else np.zeros(0, dtype=nsbind.TERM_DTYPE)
    ids, nd, npost = np.array(seg_ids, np.uint32), np.array(n_docs, np.uint32), np.array(n_postings, np.uint64)
    items, out_refs = np.zeros((4096, 6), np.uint32), np.zeros((4096, 4), np.uint32)
    ni, nr = C.c_uint64(), C.c_uint64()
    err = C.create_string_buffer(256)
    rc = harness.facet_plan(qd.ctypes.data, len(qd), refs.ctypes.data if len(refs) else None, len(refs), int(and_mode), ids.ctypes.data,
                            nd.ctypes.data, npost.ctypes.data, len(ids), tile, items.ctypes.data, len(items), C.byref(ni), out_refs.ctypes.data,
                            len(out_refs), C.byref(nr), err, len(err))
    assert ni.value <= len(items) and nr.value <= len(out_refs)
    return rc, items[: ni.value], out_refs[: nr.value], err.value.decode()


def test_the_product_tile_is_2_to_the_17(harness):
    assert harness.facet_product_tile() == 1 << 17


@pytest.mark.parametrize("tile", [32, 128, 1 << 17])
def test_the_tiles_of_every_group_partition_the_documents(harness, tile):
    sizes = [1, tile - 1, tile, tile + 1, 3 * tile + 5]
    seg_ids = [7, 3, 11, 0, 5]                                   # not ascending: a ref names an id, an item a position
    queries = [[(sid, 0, 4)] for sid in seg_ids]                 # one group each
    queries += [[(sid, 0, 4), (sid, 8, 2) ] for sid in seg_ids]  # two lists, one group
    queries += [[(seg_ids[0], 0, 4), (seg_ids[4], 1, 3), (seg_ids[0], 2, 2)], []]   # two groups; no refs at all
    for and_mode in (False, True):
        rc, items, refs, msg = plan(harness, queries, seg_ids, sizes, [16] * 5, tile, and_mode)
        assert rc == 0, msg
        assert len(queries) - 1 not in set(items[:, 0].tolist())              # the query without refs yields no item
        groups = {}
        for q, seg, rb, rc_, lo, hi in items.tolist():
            groups.setdefault((q, seg), []).append((lo, hi, rb, rc_))
        want_groups = {(qi, seg_ids.index(s)) for qi, q in enumerate(queries) for s, _, _ in q}
        assert set(groups) == want_groups
        for (q, seg), tiles in groups.items():
            n = sizes[seg]
            assert [t[0] for t in tiles] == list(range(0, n, tile))            # ascending, starting at 0, on the tile grid
            assert [t[1] for t in tiles] == [min(lo + tile, n) for lo in range(0, n, tile)]   # back to back, ending at n_docs
            assert len({t[2:] for t in tiles}) == 1                            # every tile of a group names the same refs
            rb, cnt = tiles[0][2], tiles[0][3]
            mine = [(first, c) for s, first, c in queries[q] if seg_ids.index(s) == seg]
            assert [(int(r[0]), int(r[2])) for r in refs[rb:rb + cnt]] == mine  # in query order
            assert all(int(r[3]) == 0 for r in refs[rb:rb + cnt])              # the harness registers no skip table


def test_empty_lists_and_empty_segments(harness):
    q = [[(0, 0, 0)], [(0, 0, 0), (0, 0, 5)], [(1, 0, 3)]]
    rc, items, refs, msg = plan(harness, q, [0, 1], [100, 0], [8, 8], 32, and_mode=False)
    assert rc == 0, msg
    # OR: the empty list is dropped; the group left without a list and the segment without documents have no item
    assert sorted(set(items[:, 0].tolist())) == [1] and len(items) == 4 and len(refs) == 1 and int(refs[0][2]) == 5
    rc, items, refs, msg = plan(harness, q, [0, 1], [100, 0], [8, 8], 32, and_mode=True)
    assert rc == 0 and len(items) == 0 and len(refs) == 0                      # AND: an empty list empties its group


@pytest.mark.parametrize("case,match", [
    ("unlisted", "names segment 9"), ("past", "runs past the postings"), ("odd", "not a multiple of 8"), ("twice", "listed twice"),
    ("tile", "not a power of two"), ("refs", "run past the 1 given")])
def test_the_planner_refuses(harness, case, match):
    seg_ids, q, tile = [0, 1], [[(0, 0, 4)]], 128
    if case == "unlisted":
        q = [[(9, 0, 4)]]
    elif case == "past":
        q = [[(1, 6, 3)]]
    elif case == "twice":
        seg_ids = [1, 1]
    elif case == "tile":
        tile = 96
    if case in ("odd", "refs"):
        qd = np.zeros(1, dtype=nsbind.QDESC_DTYPE)
        qd[0] = (0, 2 if case == "refs" else 1)
        refs = np.array([(0, 1, 4 if case == "odd" else 8, 1.0, 1.0)], dtype=nsbind.TERM_DTYPE)
        ids, nd, npost = np.array(seg_ids, np.uint32), np.array([10, 10], np.uint32), np.array([8, 8], np.uint64)
        ni, nr = C.c_uint64(), C.c_uint64()
        err = C.create_string_buffer(256)
        rc = harness.facet_plan(qd.ctypes.data, 1, refs.ctypes.data, 1, 0, ids.ctypes.data, nd.ctypes.data, npost.ctypes.data, 2, tile, None, 0,
                                C.byref(ni), None, 0, C.byref(nr), err, len(err))
        msg = err.value.decode()
    else:
        rc, _, _, msg = plan(harness, q, seg_ids, [10, 10], [8, 8], tile)
    assert rc == NS_E_INVAL and match in msg, (rc, msg)
