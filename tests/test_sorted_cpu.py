"""Search sorted by date, host side (host/sorted.hpp, Engine::sort_keys, csrc/ns_sorted_plan.hpp): the
restatement tests/sorted_ref.py against a brute-force loop, the date keys of a small dated index on a host-only engine, and
the planner's per-query item ranges and sub-batches through tests/sorted_plan_harness.cpp.  No device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nsbind
import sorted_ref
from rawseg import avgdl_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
NS_E_INVAL = -1

N_SEG, N_PER_SEG = 2, 45
# the publish_time of document i (of all segments, in manifest order) is DATES[i % 9]; None: no metadata row
DATES = ["2019", "2020-03", "2020-03-15", "2020 Mar", "", None, "2021-11-02", "2020-04", "2019-12-31", "2020-13-01", "20200315"]


def date_of(i):
    return DATES[i % len(DATES)]


def py_date_key(text):
    """restatement of nsx::date_key: YYYY, YYYY-MM or YYYY-MM-DD, month 1..12, day 1..31; anything else 0"""
    if text is None:
        return 0
    t = text.strip(" \t\r\n")
    parts = t.split("-")
    if not 1 <= len(parts) <= 3 or len(parts[0]) != 4 or any(len(p) != 2 for p in parts[1:]) or not all(p.isascii() and p.isdigit() for p in parts):
        return 0
    y, m, d = int(parts[0]), int(parts[1]) if len(parts) > 1 else 0, int(parts[2]) if len(parts) > 2 else 0
    if y == 0 or (len(parts) > 1 and not 1 <= m <= 12) or (len(parts) > 2 and not 1 <= d <= 31):
        return 0
    return y * 10000 + m * 100 + d


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
    index = str(tmp_path_factory.mktemp("sorted_cpu") / "index")
    nsbind.gen_index(index, N_SEG, N_PER_SEG, 512, 77, False)
    write_metadata(index, date_of, N_SEG * N_PER_SEG)
    eng = nsbind.Engine(index, -1)
    yield eng
    eng.close()


# ---- the restatement ----------------------------------------------------------------------------------------------------
def brute(segments, queries, keys, k, and_mode, ascending, order, idfs, weights):
    """nested loops over documents, no numpy set operation, no shared code with sorted_ref"""
    K = min(max(k, 1), 100)
    f32 = np.float32
    out = []
    for q in queries:
        cand = []
        for pos, s in enumerate(order):
            n_docs, doc_len, lists = segments[s]
            named = [li for ss, li in q if ss == s]
            if not named:
                continue
            avgdl = f32(avgdl_of(np.asarray(doc_len, np.uint32)))
            for d in range(n_docs):
                inl = [d in lists[li][0].tolist() for li in named]
                if not (all(inl) if and_mode else any(inl)):
                    continue
                acc = f32(0.0)
                for li in named:
                    for dd, tf in zip(lists[li][0].tolist(), lists[li][1].tolist()):
                        if dd == d:
                            norm = f32(1.2) * ((f32(1.0) - f32(0.75)) + f32(0.75) * (f32(doc_len[d]) / avgdl))
                            tf = f32(tf)
                            acc = f32(acc + f32(f32(weights[s][li]) * f32(f32(f32(idfs[s][li]) * f32(tf * f32(f32(1.2) + f32(1.0)))) / f32(tf + norm))))
                key = int(keys[s][d])
                if key == 0:
                    group, within = 1, 0
                else:
                    group, within = 0, (key if ascending else 0xFFFFFFFF - key)
                cand.append((group, within, pos, d, s, key, acc))
        cand.sort(key=lambda c: c[:4])
        out.append((len(cand), [(s, d, key, acc) for _, _, _, d, s, key, acc in cand[:K]]))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_restatement_equals_a_brute_force_loop(seed):
    rng = np.random.default_rng(seed)
    segments, keys, idfs, weights = [], [], [], []
    for n in (23, 9, 40):
        lists = []
        for m in rng.integers(0, n + 1, 4):
            d = np.sort(rng.choice(n, int(m), replace=False)).astype(np.uint32)
            lists.append((d, rng.integers(1, 6, len(d)).astype(np.uint32)))
        segments.append((n, rng.integers(3, 50, n).astype(np.uint32), lists))
        keys.append(rng.choice(np.array([0, 0, 5, 7, 20200101, 0xFFFFFFFE], np.uint32), n))
        idfs.append([float(x) for x in rng.uniform(0.5, 4.0, 4)])
        weights.append([1.0, 0.5, 1.0, 0.25])
    queries = [[], [(0, 0)], [(0, 1), (0, 2)], [(0, 0), (1, 1), (2, 2)], [(2, 3), (2, 3), (2, 0)], [(1, 0), (1, 1), (1, 2), (1, 3)],
               [(0, 3), (2, 1), (0, 0), (2, 2)]]
    for order in ([0, 1, 2], [2, 0, 1]):
        for and_mode in (False, True):
            for asc in (False, True):
                for k in (1, 5, 100):
                    got = sorted_ref.sorted_hits(segments, queries, keys, k, and_mode, asc, order, idfs, weights)
                    want = brute(segments, queries, keys, k, and_mode, asc, order, idfs, weights)
                    for qi, ((gf, gh), (wf, wh)) in enumerate(zip(got, want)):
                        assert gf == wf, (qi, gf, wf)
                        assert [(s, d, kk) for s, d, kk, _ in gh] == [(s, d, kk) for s, d, kk, _ in wh], (order, and_mode, asc, k, qi)
                        assert [np.float32(x).view(np.uint32) for _, _, _, x in gh] == [np.float32(x).view(np.uint32) for _, _, _, x in wh]
                        ks = [kk for _, _, kk, _ in gh]
                        assert 0 not in ks or all(kk == 0 for kk in ks[ks.index(0):])          # undated last, both directions


def test_resort_is_the_same_order():
    keys = {(0, 1): 5, (0, 2): 0, (1, 0): 5, (1, 3): 9}
    triples = [(1.0, 0, 2), (2.0, 1, 3), (0.5, 0, 1), (0.7, 1, 0)]
    new = sorted_ref.resort(triples, lambda s, d: keys[(s, d)], lambda s: s, False)
    assert [(s, d) for _, s, d in new] == [(1, 3), (0, 1), (1, 0), (0, 2)]
    old = sorted_ref.resort(triples, lambda s, d: keys[(s, d)], lambda s: s, True)
    assert [(s, d) for _, s, d in old] == [(0, 1), (1, 0), (1, 3), (0, 2)]


# ---- the keys -----------------------------------------------------------------------------------------------------------
def test_date_keys_on_a_host_only_engine(dated):
    for order in ("newest", "oldest"):
        keys = dated.sort_keys(order)
        assert len(keys) == N_SEG
        for s in range(N_SEG):
            assert keys[s].dtype == np.uint32 and len(keys[s]) == N_PER_SEG
            assert [int(x) for x in keys[s]] == [py_date_key(date_of(s * N_PER_SEG + d)) for d in range(N_PER_SEG)]
            assert [int(x) for x in keys[s]] == [nsbind.date_key(date_of(s * N_PER_SEG + d) or "") for d in range(N_PER_SEG)]
    want = {"2019": 20190000, "2020-03": 20200300, "2020-03-15": 20200315, "2020 Mar": 0, "": 0, None: 0, "2021-11-02": 20211102, "2020-13-01": 0,
            "20200315": 0}
    for t, k in want.items():
        assert py_date_key(t) == k
    assert dated.sort_tables_on_device() == 0


def test_custom_keys_are_taken_as_given_and_checked(dated):
    custom = [np.arange(N_PER_SEG, dtype=np.uint32) * 3, np.full(N_PER_SEG, 0xFFFFFFFE, np.uint32)]
    keys = dated.sort_keys("desc", custom=custom)
    for s in range(N_SEG):
        np.testing.assert_array_equal(keys[s], custom[s])
    bad = [custom[0].copy(), custom[1].copy()]
    bad[1][7] = 0xFFFFFFFF
    with pytest.raises(RuntimeError, match="reserved key 0xFFFFFFFF"):
        dated.sort_keys("desc", custom=bad)
    with pytest.raises(RuntimeError, match="1 key arrays for 2 segments"):
        dated.sort_keys("desc", custom=[custom[0]])
    with pytest.raises(RuntimeError, match="3 key arrays for 2 segments"):                   # keys left over past the last segment
        dated.sort_keys("asc", custom=[custom[0], np.zeros(N_PER_SEG + 1, np.uint32)])


def test_a_host_only_engine_sorts_nothing_and_says_so(dated):
    with pytest.raises(RuntimeError, match="no device context"):
        dated.search_sorted_batch(["t000001"], 10)
    with pytest.raises(RuntimeError, match="no device context"):
        dated.search_sorted_json("t000001", 10, "newest")
    body = dated.search_sorted_json("t000001", 10, "oldest", check=False)
    assert body.startswith('{\n  "error": "') and "no device context" in body
    assert dated.sort_tables_on_device() == 0


# ---- the planner --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sorted_plan") / "sorted_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "sorted_plan_harness.cpp")], check=True)
    lib = C.CDLL(so)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.sorted_plan.argtypes = [vp, u32, u32, u32, u64, vp, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64), C.c_char_p, u32]
    lib.sorted_cand_bytes.restype = u64
    lib.sorted_asc_flag.restype = u32
    return lib


def plan(harness, tiles, K, cand_bytes, tile_docs=32):
    tiles = np.array(tiles, np.uint32)
    n = len(tiles)
    q_off, batches, item_q = np.zeros(n + 1, np.uint32), np.zeros((n + 1, 4), np.uint32), np.zeros(int(tiles.sum()) + 1, np.uint32)
    nb, ni = C.c_uint64(), C.c_uint64()
    err = C.create_string_buffer(256)
    rc = harness.sorted_plan(tiles.ctypes.data, n, tile_docs, K, cand_bytes, q_off.ctypes.data, batches.ctypes.data, len(batches), C.byref(nb),
                             item_q.ctypes.data, len(item_q), C.byref(ni), err, len(err))
    assert nb.value <= len(batches) and ni.value <= len(item_q)
    return rc, q_off, batches[: nb.value], item_q[: ni.value], err.value.decode()


def test_the_constants(harness):
    assert harness.sorted_cand_bytes() == 64 << 20                              # DESIGN.md §5q's bound
    assert harness.sorted_asc_flag() == nsbind.NS_SORT_ASC == 0x1000            # collides with no NS_FLAG_* / NS_INFO_* bit
    assert nsbind.NS_SORT_ASC & (1 | 0x100 | 0x200 | 0x400 | 0x800) == 0
    assert harness.sorted_plan_refuses_unordered() == 1


def test_a_querys_item_range_covers_exactly_its_items(harness):
    tiles = [3, 0, 1, 7, 0, 0, 2, 1]
    rc, q_off, batches, item_q, msg = plan(harness, tiles, 100, 64 << 20)
    assert rc == 0, msg
    assert len(item_q) == sum(tiles) and int(q_off[0]) == 0 and int(q_off[-1]) == len(item_q)
    for q, t in enumerate(tiles):
        a, b = int(q_off[q]), int(q_off[q + 1])
        assert b - a == t and all(int(x) == q for x in item_q[a:b])
    assert batches.tolist() == [[0, len(tiles), 0, sum(tiles)]]                  # everything fits one sub-batch


@pytest.mark.parametrize("K", [1, 64, 100])
def test_sub_batches_respect_the_bound_and_partition_the_queries(harness, K):
    rng = np.random.default_rng(K)
    tiles = [int(t) for t in rng.integers(0, 9, 200)]
    bound = 8 * K * 20                                                           # room for 20 rows
    rc, q_off, batches, item_q, msg = plan(harness, tiles, K, bound)
    assert rc == 0, msg
    assert len(batches) > 5
    assert int(batches[0][0]) == 0 and int(batches[-1][1]) == len(tiles)
    for i, (qa, qb, ia, ib) in enumerate(batches.tolist()):
        assert qa < qb and (ia, ib) == (int(q_off[qa]), int(q_off[qb]))
        assert (ib - ia) * K * 8 <= bound                                        # the candidate rows fit
        if i:
            assert qa == batches[i - 1][1]                                       # back to back: a partition
        if qb < len(tiles):                                                      # greedy: the next query would not have fitted
            assert (int(q_off[qb + 1]) - ia) * K * 8 > bound
    # at the product's bound and K = 100: 83 886 rows
    rc, q_off, batches, _, msg = plan(harness, [1] * 10, 100, 64 << 20)
    assert rc == 0 and len(batches) == 1 and (64 << 20) // 800 == 83886


def test_a_query_that_alone_exceeds_the_bound_is_refused(harness):
    """pinned: NS_E_INVAL with a message that names the query, no sub-batch returned; one row less is served"""
    K, rows = 100, 7
    rc, _, batches, _, msg = plan(harness, [2, rows + 1, 1], K, 8 * K * rows)
    assert rc == NS_E_INVAL and len(batches) == 0
    assert "query 1 alone has 8 work items" in msg and "holds 7 rows at K = 100" in msg
    rc, _, batches, _, msg = plan(harness, [2, rows, 1], K, 8 * K * rows)
    assert rc == 0 and batches.tolist() == [[0, 1, 0, 2], [1, 2, 2, 9], [2, 3, 9, 10]]
    rc, _, _, _, msg = plan(harness, [1], 129, 1 << 20)
    assert rc == NS_E_INVAL and "K = 129 outside [1, 128]" in msg
