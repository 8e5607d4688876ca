"""CPU test of the directed families (tests/body_shapes.py): every family is planned through tests/plan_harness.cpp and
must take the body it was built for.  This is what keeps the families aimed when a planner threshold moves: this test
goes red, instead of a GPU test going green on another body.  No GPU."""
import os
import re

import numpy as np
import pytest

import body_shapes
import rawseg
from test_batch_plan import KIND_SKIP, SEG_DTYPE, check_exactly_once, harness, plan, registered  # noqa: F401  (harness: fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
WHOLE = dict(min_items=1, split_postings=1 << 30)   # the settings the GPU test scores the families in (body_reach.WHOLE)


def body_of(whole):
    assert not whole & 128, "no family is pruned"
    return "merge" if whole & 256 else "thin" if whole & 4 else "tile" if whole & 2 else "general"


def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_match_the_kernels():
    """body_shapes' sizes are derived from these constants; a change of one of them must come back to the families"""
    api, tile, internal, plan_h = read("ns_api.hip"), read("ns_tile_kernel.hip"), read("ns_internal.h"), read("ns_plan.hpp")
    inst = set(re.findall(r"k_uscore<(\d+), (\d+), (?:true|false), CB, TMAX, IMP, PK>", api))
    assert inst == {("512", "192")}
    hk, fb = 512, 192
    assert "dscore_body<HK / 2, 64, AND, CB, IMP, PK>" in tile and "dscore_body<HK / 2, FB, AND, CB, IMP, 0>" in tile
    assert "tscore_body<2 * HK, AND, CB, IMP>" in tile
    assert "dscore_body<HK / 4" not in tile   # k_uscore's table is HK / 2 buckets in both classes
    assert body_shapes.NB == hk // 2 and body_shapes.FB == {"thin": 64, "general": fb}
    assert int(re.search(r"kSkipDocs = (\d+);", internal).group(1)) == body_shapes.SKIP_DOCS == 2 * hk
    assert body_shapes.ROUND == 4 * 64 and "constexpr int DE = 4;" in read("ns_driver_kernel.hip") and "constexpr int DE = 4;" in read("ns_merge_kernel.hip")
    with open(os.path.join(ROOT, "include", "nextsearch_hip.h")) as f:
        assert int(re.search(r"#define NS_MAX_K\s+(\d+)", f.read()).group(1)) == body_shapes.MAX_K
    assert "uint32_t merge_ratio = 8;" in plan_h and "uint32_t tile_dens64 = 16;" in plan_h and "rest * 32 <= hg.cmax" in plan_h
    # the candidate buffer: 128 entries up to K = 32, 256 above
    assert "if (b->K <= 32) {" in api and "launch_uscore<128, 16>" in api and "launch_uscore<256, 16>" in api
    assert body_shapes.CB_SWITCH_K == 32 and {32, 33, 63, 64, 65, 1, 100, body_shapes.MAX_K} <= set(body_shapes.K_SET)


def family_plan_inputs(fn):
    n, doc_len, lists, queries, idfs, weights = fn()
    flat, offs = rawseg.payload_of(lists)
    qd, refs = rawseg.descriptors(queries, lists, offs, idfs, weights)
    segs = np.zeros(1, SEG_DTYPE)
    segs[0]["n_docs"], segs[0]["n_postings"], segs[0]["norm_safe"] = n, len(flat) // 2, 1
    bodies = fn.bodies(n, lists, queries) if callable(fn.bodies) else list(fn.bodies)
    return n, lists, queries, segs, qd, refs, bodies


def per_query(p, n_queries):
    out = [[] for _ in range(n_queries)]
    for w in p.witems:
        out[int(w["query"])].append(w)
    assert p.n_items == 0, "every group of a family is a wave item"
    return out


@pytest.mark.parametrize("name", list(body_shapes.FAMILIES))
def test_family_takes_the_body_it_aims_at(name, harness):
    fn = body_shapes.FAMILIES[name]
    n, lists, queries, segs, qd, refs, bodies = family_plan_inputs(fn)
    assert len(bodies) == len(queries)
    # doc lengths vary (norms differ) unless the family says that its lengths are deliberate
    doc_len = fn()[1]
    assert len(np.unique(doc_len)) > 100
    # the literal expectation agrees with the restated rule: both would have to move together
    assert bodies == [body_shapes.plan_rule([len(lists[li][0]) for li in q], n, fn.merge) for q in queries]
    skip_lists = registered(refs, KIND_SKIP, 64)
    for flags in (0, 1):
        for k in (10, 100):
            # as the GPU test runs them: one item per group
            p = plan(harness, segs, qd, refs, k=k, flags=flags, use_merge=int(fn.merge), **WHOLE)
            check_exactly_once(p, segs, len(qd))
            items = per_query(p, len(queries))
            for qi, q in enumerate(queries):
                assert len(items[qi]) == 1, (name, qi)
                w = items[qi][0]
                assert int(w["term_count"]) == len(q) and int(w["whole"]) & 1
                assert body_of(int(w["whole"])) == bodies[qi], (name, qi, q, hex(int(w["whole"])))
                assert not int(w["whole"]) & (32 | 64), "no skip tables registered: no grid"
            assert p.n_wide == sum(len(q) > 16 for q in queries)
    # skip tables registered: doc-tile groups walk the grid (bit 5); whole driver-stream and merge items need no range ends
    for use in (1, 0):
        p = plan(harness, segs, qd, refs, lists=skip_lists, use_skips=use, use_merge=int(fn.merge), **WHOLE)
        for qi, ws in enumerate(per_query(p, len(queries))):
            grid = bool(int(ws[0]["whole"]) & 32)
            has_table = any(len(lists[li][0]) >= 64 for li in queries[qi])
            assert grid == (bodies[qi] == "tile" and use == 1 and has_table), (name, qi, use)
            assert not int(ws[0]["whole"]) & 64 and body_of(int(ws[0]["whole"])) == bodies[qi]
    # default settings: a small batch is cut into many doc ranges; every range of a group keeps the group's body
    p = plan(harness, segs, qd, refs, use_merge=int(fn.merge))
    check_exactly_once(p, segs, len(qd))
    for qi, ws in enumerate(per_query(p, len(queries))):
        assert {body_of(int(w["whole"])) for w in ws} == {bodies[qi]}, (name, qi)
    # the other merge setting changes nothing but the two-list general groups
    p = plan(harness, segs, qd, refs, use_merge=int(not fn.merge), **WHOLE)
    other = [body_shapes.plan_rule([len(lists[li][0]) for li in q], n, not fn.merge) for q in queries]
    assert [body_of(int(ws[0]["whole"])) for ws in per_query(p, len(queries))] == other


@pytest.mark.parametrize("name", [n for n, f in body_shapes.FAMILIES.items() if f.split])
def test_split_variant_cuts_inside_the_run(name, harness):
    """ns_set_tuning's split value of the family cuts every group's doc range at a doc INSIDE the run of consecutive docIds"""
    fn = body_shapes.FAMILIES[name]
    n, lists, queries, segs, qd, refs, bodies = family_plan_inputs(fn)
    first, last = fn.run
    skip_lists = registered(refs, KIND_SKIP, 64)
    for cls, split in fn.split.items():
        assert set(bodies) == {cls}
        for k in (10, 100):
            for reg, use in ((None, 1), (skip_lists, 1), (skip_lists, 0)):
                p = plan(harness, segs, qd, refs, k=k, lists=reg, use_skips=use, min_items=1, split_postings=split)
                check_exactly_once(p, segs, len(qd))
                for qi, ws in enumerate(per_query(p, len(queries))):
                    assert len(ws) >= 2 and not any(int(w["whole"]) & 1 for w in ws)
                    assert any(first < int(w["doc_lo"]) <= last for w in ws), (name, qi, k, sorted(int(w["doc_lo"]) for w in ws))
                    assert {body_of(int(w["whole"])) for w in ws} == {cls}
                    # range ends from the skip tables (bit 6) exactly when tables are registered and used
                    assert all(bool(int(w["whole"]) & 64) == (reg is not None and use == 1) for w in ws)
