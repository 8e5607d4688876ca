"""CPU tests of the directed join families (tests/join_shapes.py): the restated path rule is pinned to the sources, every
family is planned through tests/plan_harness.cpp under its own tuning and K and must put every query on the join path it
declares, and the numpy checker of the rank join is itself checked against brute force.  This is what keeps the families
aimed when the planner's cut or a join threshold moves: this test goes red, instead of a GPU test going green on another
path.  No GPU."""
import os
import re

import numpy as np
import pytest

import join_ref
import join_shapes
import rawseg
from test_batch_plan import SEG_DTYPE, check_exactly_once, harness, plan  # noqa: F401  (harness: fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")


def read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_path_rule_matches_the_kernels():
    """join_shapes.path_rule against the constants and conditions of ns_internal.h / ns_kernels.hip"""
    internal, kern = read("nextsearch-api_amd", "csrc", "ns_internal.h"), read("nextsearch-api_amd", "csrc", "ns_kernels.hip")
    m = re.search(r"constexpr bool merge_is_wide\(uint32_t part_count, uint32_t K\) \{ return part_count > (\d+) && part_count >= K; \}", internal)
    assert m and int(m.group(1)) == join_shapes.WAVE
    assert int(re.search(r"constexpr int kMergeStage = (\d+);", kern).group(1)) == join_shapes.MERGE_STAGE
    assert int(re.search(r"constexpr uint32_t kMergeCap = (\d+);", kern).group(1)) == join_shapes.MERGE_CAP
    assert int(re.search(r"constexpr uint32_t kMergeRegRows = (\d+);", kern).group(1)) == join_shapes.MERGE_REG_ROWS
    assert int(re.search(r"#define NS_MAX_K\s+(\d+)", read("include", "nextsearch_hip.h")).group(1)) == join_shapes.MAX_K
    # the order of the tests inside k_merge: wide queries leave, then the sort, then the staged rounds, then the tournament
    a, b, c = kern.index("if (merge_is_wide(pc, K)) return;"), kern.index("if (pc * K <= 64u) {"), kern.index("if (pc <= 64u && pc * K <= (uint32_t)kMergeStage) {")
    assert a < b < c < kern.index("merge_rows_wave(q, pb, pc, part_hits, part_nhits, out_hits, out_nhits, out_found, found, K, heads, lane);")
    assert "hs[r] >= theta) gather_row(tid + r * 256)" in kern and "if (C > kMergeCap) {" in kern
    # the rule at its edges
    R = join_shapes.path_rule
    assert [R(6, 10), R(7, 10), R(2, 32), R(64, 1), R(0, 100), R(0, 10)] == ["sort64", "staged", "sort64", "sort64", "sort64", "sort64"]
    assert [R(32, 64), R(33, 64), R(21, 100), R(64, 100), R(64, 32)] == ["staged", "tournament", "tournament", "tournament", "staged"]
    assert [R(65, 100), R(99, 100), R(100, 100), R(65, 64), R(65, 1), R(64, 1)] == ["tournament", "tournament", "wide", "wide", "wide", "sort64"]


def family_plan_inputs(fam):
    segs = np.zeros(len(fam.segments), SEG_DTYPE)
    offs = []
    for s, (n, doc_len, lists) in enumerate(fam.segments):
        flat, o = rawseg.payload_of(lists)
        offs.append(o)
        segs[s]["n_docs"], segs[s]["n_postings"], segs[s]["norm_safe"] = n, len(flat) // 2, 1
    qd, refs = rawseg.descriptors_multi(fam.queries, [lists for _, _, lists in fam.segments], offs, fam.idfs, fam.weights)
    return segs, qd, refs


def planned(harness, fam, k, flags=0, **over):
    segs, qd, refs = family_plan_inputs(fam)
    variant, min_items, split = fam.tuning
    settings = dict(variant=variant, min_items=min_items, split_postings=split)
    settings.update(over)
    p = plan(harness, segs, qd, refs, k=k, flags=flags, **settings)
    check_exactly_once(p, segs, len(qd))
    return p, [int(x) for x in p.queries(len(qd))["part_count"]]


def predicted_counts(fam):
    """per K: how many queries take each of the four paths, from the family's declaration"""
    return {k: [fam.paths[k].count(p) for p in join_shapes.PATHS] for k in fam.ks}


@pytest.mark.parametrize("name", list(join_shapes.FAMILIES))
def test_family_takes_the_join_paths_it_declares(name, harness):
    fam = join_shapes.FAMILIES[name]()
    for n, doc_len, lists in fam.segments:
        assert n <= 65536 and all(len(d) <= 32768 for d, _ in lists), "keep the restatement's Python loop short"
        assert all(np.all(np.diff(d.astype(np.int64)) > 0) and d[-1] < n for d, _ in lists)
    for k in fam.ks:
        for flags in (0, 1):
            p, pcs = planned(harness, fam, k, flags)
            got = [join_shapes.path_rule(pc, k) for pc in pcs]
            assert got == fam.paths[k], (name, k, flags, pcs, got)
            assert p.direct == 0 and len(set(pcs)) > 1, "a batch of mixed part_count: both join kernels' queries in one batch"
            assert p.n_wide_q == sum(path == "wide" for path in fam.paths[k]) == sum(join_shapes.is_wide(pc, k) for pc in pcs)
            assert p.n_items == 0, "every group is a wave item"
    assert set(fam.events) >= {e for k in fam.ks for e in fam.paths[k]}, "every path the family declares is a counter it must move"


def test_families_cover_the_cases(harness):
    """the (K, pc) cases the families exist for, read off the plans"""
    seen = set()
    for name, fn in join_shapes.FAMILIES.items():
        fam = fn()
        for k in fam.ks:
            seen |= {(k, pc) for pc in planned(harness, fam, k)[1]}
    want = {(10, 6), (32, 2), (10, 7), (1, 64), (100, 0), (10, 0), (64, 32), (64, 33), (100, 21), (100, 64), (100, 100), (100, 12288), (10, 12288)}
    assert want <= seen, sorted(want - seen)
    assert any(k == 100 and 65 <= pc <= 99 for k, pc in seen), "the tournament with more than one row per lane"
    assert any(pc > 256 * join_shapes.MERGE_REG_ROWS for _, pc in seen)


def test_a_changed_tuning_is_noticed(harness):
    """the check above has teeth: under half the split value the family's queries land on other paths"""
    fam = join_shapes.FAMILIES["sort_stage_boundary"]()
    _, pcs = planned(harness, fam, 10, split_postings=fam.tuning[2] // 2)
    assert [join_shapes.path_rule(pc, 10) for pc in pcs] != fam.paths[10]


def test_lone_query_test_segment_is_the_smallest_that_plans_wide(harness):
    """join_shapes.LONE_WIDE_N: at N docs the lone query of test_lone_query_wide_merge_ties_and_thresholds is wide at all its
    K under both its tunings, at N - 1 it no longer is at K = 100"""
    def pc(n, k, min_items):
        segs = np.zeros(1, SEG_DTYPE)
        segs[0]["n_docs"], segs[0]["n_postings"], segs[0]["norm_safe"] = n, (n + 1) // 2, 1
        qd = np.array([(0, 1)], dtype=rawseg.nsbind.QDESC_DTYPE)
        refs = np.array([(0, (n + 1) // 2, 0, 1.75, 1.0)], dtype=rawseg.nsbind.TERM_DTYPE)
        p = plan(harness, segs, qd, refs, k=k, min_items=min_items)
        assert p.n_wide_q == int(join_shapes.is_wide(int(p.queries(1)[0]["part_count"]), k))
        return int(p.queries(1)[0]["part_count"])
    n = join_shapes.LONE_WIDE_N
    for min_items in (0, 20000):
        assert all(join_shapes.is_wide(pc(n, k, min_items), k) for k in (1, 10, 64, 100))
        assert not join_shapes.is_wide(pc(n - 1, 100, min_items), 100)


def test_no_negative_zero_and_ties_exist():
    """the join orders by score bits: no family may produce -0.0f; the flat families do produce equal scores across segments"""
    for name, fn in join_shapes.FAMILIES.items():
        fam = fn()
        ref = rawseg.reference_multi(fam.segments, fam.queries, fam.idfs, fam.weights)
        bits = np.array([v for both in ref for v, _, _ in both[0]], dtype=np.float32).view(np.uint32)
        assert len(bits) and not np.any(bits == 0x80000000) and np.all(bits < 0x7F800000), name
        if name != "wide_unregistered_rows":
            multi = [both[0] for q, both in zip(fam.queries, ref) if len({s for s, _ in q}) > 1]
            assert multi and all(len({s for v, s, _ in keyed if v == keyed[len(keyed) // 2][0]}) > 1 for keyed in multi), name


@pytest.mark.parametrize("with_seg_map", [True, False])
def test_numpy_join_equals_brute_force_on_the_synthetic_rank_rows(with_seg_map):
    for w in join_shapes.RANK_COUNTS:
        for k in join_shapes.RANK_KS:
            hits, nhits, found, seg_map = join_shapes.rank_rows(w, k, with_seg_map=with_seg_map)
            assert hits.shape == (w, join_shapes.RANK_QUERIES, k, 3) and join_shapes.RANK_QUERIES % 4
            got = join_ref.np_join(hits, nhits, found, seg_map, k)
            assert got == join_shapes.brute_join(hits, nhits, found, seg_map, k), (w, k)
            # what the cases are for
            assert got[0] == ([], 0) and (w == 1 or np.any(nhits[:, 2] > k)) and nhits[w - 1, join_shapes.RANK_QUERIES - 1] <= k
            pairs = [(g, d) for hs, _ in got for _, g, d in hs]
            assert all(len(hs) == len(set((g, d) for _, g, d in hs)) for hs, _ in got) and pairs
            if w >= 2:
                assert got[3][1] >= 1 << 32, "found sums past 2^32"
            if with_seg_map and w >= 2 and k >= 10:
                # ties across ranks decided by the GLOBAL segment: some query's winners are not in rank (lane) order
                tops = [hs for hs, _ in got if len(hs) >= 2]
                assert any(a[0] == b[0] and a[1] != b[1] for hs in tops for a, b in zip(hs, hs[1:]))
