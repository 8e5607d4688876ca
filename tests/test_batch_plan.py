"""CPU tests of the batch planner (nextsearch-api_amd/csrc/ns_plan.hpp) through tests/plan_harness.cpp: the descriptor image
of a batch does not depend on the number of prepare threads, holds every work item exactly once, and the launch-order
modes only permute items inside their classes.  No GPU: the harness plans over fake segments and fixed device pointers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nsbind
import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")

# PlanSettings, in the order plan_batch reads them, with ns_ctx_create's defaults on a 256-CU device
SETTINGS = dict(variant=0, min_items=0, split_postings=0, n_cus=256, use_impacts=1, use_packed=1, use_skips=1, use_merge=1,
                merge_ratio=8, use_pruning=0, share_mode=1, share_ratio=48, share_min_postings=4 << 20, prep_threads=0,
                order_mode=1, order_coarse=3, order_coarse_forced=0, key_pct0=100, key_pct1=100, key_pct2=100, key_pct3=100,
                tile_dens64=16)
OUT = ["bytes", "o_items", "o_witems", "o_terms", "o_groups", "o_queries", "o_segs", "o_wideq", "o_share", "n_items",
       "n_witems", "n_dterms", "n_bgroups", "n_rows", "n_narrow", "n_wide", "direct", "shared", "n_share", "share_postings",
       "all_imp", "all_pk", "pruned", "deal", "deal_shift", "width", "postings", "n_wide_q", "refused", "empty_groups",
       "largest_dealt"]
SEG_DTYPE = np.dtype([("n_docs", "<u4"), ("norm_safe", "<u4"), ("packed", "<u4"), ("pad", "<u4"), ("n_postings", "<u8")])
LIST_DTYPE = np.dtype([("seg", "<u4"), ("kind", "<u4"), ("first", "<u4"), ("count", "<u4"), ("idf_bits", "<u4"), ("entry", "<u4")])
WITEM = np.dtype([(f, "<u4") for f in ("query", "seg", "term_begin", "term_count", "doc_lo", "doc_hi", "out_slot", "whole")])
ITEM = np.dtype([("bounds_off", "<u8")] + [(f, "<u4") for f in ("query", "seg", "term_begin", "term_count", "tile_begin",
                                                                 "tile_end", "out_slot", "pad")])
DQUERY = np.dtype([("part_begin", "<u4"), ("part_count", "<u4")])
KIND_IMP, KIND_SKIP, KIND_BMX = 0, 1, 2


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("plan") / "plan_harness.so")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + CSRC, "-o", so, os.path.join(ROOT, "tests", "plan_harness.cpp"), "-lpthread"], check=True)
    lib = C.CDLL(so)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.plan_batch.argtypes = [vp, vp, u32, vp, u32, vp, vp, u32, u32, u32, vp, u64, vp, vp, C.c_char_p, u32]
    return lib


class Plan:
    def __init__(self, out, image, bucket_pos):
        self.__dict__.update(dict(zip(OUT, (int(x) for x in out))))
        self.image = image
        self.bucket_pos = bucket_pos
        self.witems = np.frombuffer(image, WITEM, self.n_witems, self.o_witems)
        self.items = np.frombuffer(image, ITEM, self.n_items, self.o_items)

    def queries(self, n):
        return np.frombuffer(self.image, DQUERY, n, self.o_queries)


def plan(harness, segs, qd, refs, k=10, flags=0, lists=None, **settings):
    s = dict(SETTINGS, **settings)
    sarr = np.array([s[n] for n in SETTINGS], np.uint64)
    lists = np.zeros(0, LIST_DTYPE) if lists is None else lists
    out = np.zeros(len(OUT), np.uint64)
    bpos = np.zeros(2049, np.uint32)
    err = C.create_string_buffer(512)
    image = np.zeros(64 << 20, np.uint8)
    rc = harness.plan_batch(sarr.ctypes.data, segs.ctypes.data, len(segs), lists.ctypes.data, len(lists), qd.ctypes.data,
                            refs.ctypes.data if len(refs) else None, len(qd), k, flags, image.ctypes.data, image.nbytes,
                            out.ctypes.data, bpos.ctypes.data, err, len(err))
    assert rc == 0, (rc, err.value.decode())
    return Plan(out, image[: int(out[0])].tobytes(), bpos)


@pytest.fixture(scope="module")
def corpus(index_factory):
    d, _ = index_factory(4, 30000)
    eng = nsbind.Engine(d, -1)
    segs = np.zeros(eng.num_segments, SEG_DTYPE)
    for s in range(eng.num_segments):
        info = eng.segment_info(s)
        segs[s]["n_docs"], segs[s]["n_postings"], segs[s]["norm_safe"] = info["n_docs"], info["n_postings"], 1
    cfg5 = eng.build_refs(workloads.cfg5_queries(16384))[:2]
    cfg3 = eng.build_refs(workloads.cfg3_queries(4096))[:2]
    small = eng.build_refs(workloads.cfg5_queries(2048, 2005 + 104729))[:2]
    eng.close()
    return segs, cfg5, cfg3, small


def registered(refs, kind, min_count=0, single=None):
    """one registry entry per distinct list of `refs` (count >= min_count), at consecutive table entries"""
    r = refs if single is None else refs[single]
    r = r[r["count"] >= max(min_count, 1)]
    keys = np.unique(np.stack([r["seg_id"], r["byte_off"] // 8, r["count"], r["idf"].view(np.uint32)], 1), axis=0)
    out = np.zeros(len(keys), LIST_DTYPE)
    out["seg"], out["kind"], out["first"], out["count"], out["idf_bits"] = keys[:, 0], kind, keys[:, 1], keys[:, 2], keys[:, 3]
    out["entry"] = np.arange(len(keys)) * 64
    return out


def single_term(qd, refs):
    """mask of the refs that are alone in their (query, segment) group"""
    q = np.repeat(np.arange(len(qd), dtype=np.uint64), qd["term_count"])
    _, inv, cnt = np.unique(q << np.uint64(32) | refs["seg_id"], return_inverse=True, return_counts=True)
    return cnt[inv] == 1


def check_exactly_once(p, segs, n_queries):
    q = p.queries(n_queries)
    slots = np.concatenate([p.witems["out_slot"], p.items["out_slot"]])
    qs = np.concatenate([p.witems["query"], p.items["query"]])
    if p.direct:
        assert np.array_equal(np.sort(slots), np.arange(n_queries))
        assert np.array_equal(slots, qs) and np.all(q["part_count"] == 1)
    else:
        assert np.array_equal(np.sort(slots), np.arange(p.n_rows))
        assert int(q["part_count"].sum()) == p.n_rows
        order = np.argsort(slots, kind="stable")
        assert np.array_equal(qs[order], np.repeat(np.arange(n_queries), q["part_count"]))   # rows of a query: contiguous ...
        assert np.array_equal(q["part_begin"], np.concatenate([[0], np.cumsum(q["part_count"])[:-1]]))   # ... at part_begin
        # ... and ascending strictly in (segment, doc range): k_merge's staged rounds break ties by the lowest row
        key = np.concatenate([p.witems["seg"].astype(np.int64) << 32 | p.witems["doc_lo"], p.items["seg"].astype(np.int64) << 32 | p.items["tile_begin"]])[order]
        same_q = qs[order][1:] == qs[order][:-1]
        assert np.all(key[1:][same_q] > key[:-1][same_q])
    # the wave items of one (query, segment) group tile [0, n_docs) without overlap
    w = p.witems
    o = np.lexsort((w["doc_lo"], w["seg"], w["query"]))
    w = w[o]
    start = np.ones(len(w), bool)
    start[1:] = (w["query"][1:] != w["query"][:-1]) | (w["seg"][1:] != w["seg"][:-1])
    end = np.roll(start, -1)
    assert np.all(w["doc_lo"][start] == 0)
    assert np.all(w["doc_hi"][end] == segs["n_docs"][w["seg"][end]])
    assert np.all(w["doc_lo"] < w["doc_hi"])
    assert np.all(w["doc_lo"][~start] == w["doc_hi"][np.flatnonzero(~start) - 1])
    # narrow (<= 16 terms) items first, and n_class[0] counts exactly them
    narrow = p.witems["term_count"] <= 16
    assert p.n_narrow == int(narrow.sum()) and np.all(narrow[: p.n_narrow]) and not np.any(narrow[p.n_narrow:])
    assert p.n_narrow + p.n_wide == p.n_witems


def sorted_items(w):
    return np.sort(w.view(np.dtype((np.void, WITEM.itemsize))))


def test_image_independent_of_prepare_threads(harness, corpus):
    segs, (qd, refs), _, _ = corpus
    lists = np.concatenate([registered(refs, KIND_SKIP, 64), registered(refs, KIND_BMX, single=single_term(qd, refs))])
    for mode in (0, 2):
        images = {}
        for t in (1, 2, 5, 8):
            p = plan(harness, segs, qd, refs, lists=lists, prep_threads=t, order_mode=mode, use_pruning=1)
            assert p.width == t
            check_exactly_once(p, segs, len(qd))
            images[t] = p.image
        assert all(images[t] == images[1] for t in images), mode
    assert p.deal and p.largest_dealt > 4096 and p.pruned


def test_order_modes_hold_the_same_items(harness, corpus):
    segs, (qd, refs), (qd3, refs3), (qds, refss) = corpus
    for q, r, k in ((qd, refs, 10), (qd3, refs3, 100), (qds, refss, 10)):
        plans = {m: plan(harness, segs, q, r, k=k, order_mode=m, prep_threads=8) for m in (0, 1, 2)}
        base = plans[0]
        assert not base.deal and plans[2].deal and base.n_narrow >= 64
        for m, p in plans.items():
            check_exactly_once(p, segs, len(q))
            assert np.array_equal(sorted_items(p.witems), sorted_items(base.witems)), m
            assert p.image[: p.o_witems] == base.image[: base.o_witems] and p.image[p.o_terms:] == base.image[base.o_terms:]
            if p.deal:
                step = 1 << p.deal_shift
                for c in range(0, 2048, step):
                    a, b = int(p.bucket_pos[c]), int(p.bucket_pos[c + step])
                    assert np.array_equal(sorted_items(p.witems[a:b]), sorted_items(base.witems[a:b])), (m, c)


def handmade(segs):
    """hand-made term refs: wide groups (20 terms), k_score groups (70 terms), a segment without docs, overlapping lists"""
    refs, qd = [], []

    def query(terms):
        qd.append((len(refs), len(terms)))
        refs.extend(terms)

    per = int(segs[0]["n_postings"]) // 200
    query([(0, 300 + i, 8 * per * i, 1.5, 1.0) for i in range(20)])              # wide: > 16 terms
    query([(1, 200 + i, 8 * 37 * i, 2.0, 1.0) for i in range(70)])               # k_score: > 64 terms
    query([(3, 0, 0, 1.0, 1.0), (0, 5000, 8 * 4000, 1.0, 1.0)])                  # one ref in the empty segment 3
    query([(2, 4000, 0, 1.0, 1.0), (2, 4000, 8 * 1000, 1.25, 1.0)])              # two overlapping lists
    query([])
    r = np.array(refs, nsbind.TERM_DTYPE)
    return np.array(qd, nsbind.QDESC_DTYPE), r


def test_branches_reached(harness, corpus):
    segs, (qd, refs), _, _ = corpus
    empty = segs.copy()
    empty[3]["n_docs"], empty[3]["n_postings"] = 0, 0
    hq, hr = handmade(segs)
    p = plan(harness, empty, hq, hr, share_mode=2)
    check_exactly_once(p, empty, len(hq))
    assert p.n_wide > 0 and p.n_items > 0 and p.empty_groups == 1
    assert not p.shared and p.refused >= 1   # an overlapping list refuses the batch's sharing
    p = plan(harness, segs, qd, refs, share_mode=2)
    check_exactly_once(p, segs, len(qd))
    assert p.shared and p.n_share > 0 and p.refused == 0 and p.all_imp
    # skip-grid groups and pruned single-term groups, in OR and AND mode
    lists = np.concatenate([registered(refs, KIND_SKIP, 64), registered(refs, KIND_BMX, single=single_term(qd, refs))])
    for flags in (0, 1):
        p = plan(harness, segs, qd, refs, flags=flags, lists=lists, use_pruning=1, prep_threads=8)
        check_exactly_once(p, segs, len(qd))
        assert np.any(p.witems["whole"] & (32 | 64)) and np.any(p.witems["whole"] & 128) and p.pruned
    # every list with an impact stream built with its idf: the batch reads it, nothing to share
    p = plan(harness, segs, qd, refs, lists=registered(refs, KIND_IMP), share_mode=2)
    assert p.all_imp and not p.shared


def test_a_lone_query_is_spread_over_the_chip(harness, corpus):
    segs, (qd, refs), _, _ = corpus
    for q in range(3):
        one = qd[q: q + 1].copy()
        r = refs[one[0]["term_begin"]: one[0]["term_begin"] + one[0]["term_count"]]
        one["term_begin"] = 0
        p = plan(harness, segs, one, r)
        check_exactly_once(p, segs, 1)
        assert p.n_witems > 1 and not p.direct
