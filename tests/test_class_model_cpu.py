"""CPU tests of the planner's class model (nextsearch-api_amd/csrc/ns_plan.hpp "class model"; ns_ctx_class_model) through
tests/class_plan_harness.cpp: mode 0 plans what the planner planned before the model existed (digests of the parent commit's
descriptor images under tests/golden/), mode 1 leaves a batch that does not fill the chip alone, and under mode 2 a group's
class and estimate are those of a numpy restatement of the model.  No GPU: the harness plans over fake segments."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import nsbind
import test_batch_plan as tbp
import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "class_model_parent_plan.sha256")

CLASS_SETTINGS = dict(class_model=0, class_margin_pct=0, force_body=0, force_share10=0, force_dens_lo=0, force_dens_hi=0)
OUT = ["bytes", "o_witems", "o_terms", "o_queries", "o_segs", "n_witems", "n_dterms", "n_rows", "width", "n_groups",
       "general", "thin", "tile", "promoted", "margin_pct", "cost_tile16", "cost_visit16", "cost_posting16"]
GROUP = np.dtype([(f, "<u4") for f in ("query", "seg", "term_count", "cls", "promoted", "merge2")] + [(f, "<u8") for f in ("cost", "cmax", "work")])
WORK_FOREIGN, WORK_MERGE, WORK_TILE_OLD, TILE_DOCS = 8, 4, 2, 1024
OCC256 = np.round(256 * (1 - np.exp(-np.arange(65) / 8))).astype(np.int64)   # share of the tiles a list of c postings visits, c / tiles in eighths


def build(src, out_dir, csrc=CSRC):
    so = os.path.join(str(out_dir), os.path.basename(src).replace(".cpp", ".so"))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + csrc, "-o", so, src, "-lpthread"], check=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    lib = build(os.path.join(ROOT, "tests", "class_plan_harness.cpp"), tmp_path_factory.mktemp("classplan"))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.plan_classes.argtypes = [vp, vp, u32, vp, u32, vp, vp, u32, u32, u32, vp, u64, vp, vp, u64, C.c_char_p, u32]
    return lib


class Plan:
    pass


def plan(harness, segs, qd, refs, k=10, flags=0, lists=None, **settings):
    s = dict(tbp.SETTINGS, **CLASS_SETTINGS)
    assert all(n in s for n in settings), settings
    s.update(settings)
    sarr = np.array([s[n] for n in list(tbp.SETTINGS) + list(CLASS_SETTINGS)], np.uint64)
    lists = np.zeros(0, tbp.LIST_DTYPE) if lists is None else lists
    out = np.zeros(len(OUT), np.uint64)
    groups = np.zeros(max(1, 8 * len(qd)), GROUP)
    err = C.create_string_buffer(512)
    image = np.zeros(64 << 20, np.uint8)
    rc = harness.plan_classes(sarr.ctypes.data, segs.ctypes.data, len(segs), lists.ctypes.data, len(lists), qd.ctypes.data,
                              refs.ctypes.data if len(refs) else None, len(qd), k, flags, image.ctypes.data, image.nbytes,
                              out.ctypes.data, groups.ctypes.data, len(groups), err, len(err))
    assert rc == 0, (rc, err.value.decode())
    p = Plan()
    p.__dict__.update(dict(zip(OUT, (int(x) for x in out))))
    assert p.n_groups <= len(groups)
    p.groups = groups[: p.n_groups]
    p.image = image[: p.bytes].tobytes()
    p.witems = np.frombuffer(p.image, tbp.WITEM, p.n_witems, p.o_witems)
    return p


# ---- mode 0 and small batches: the parent's plan -------------------------------------------------------------------------

def corpus_of(index_dir):
    eng = nsbind.Engine(index_dir, -1)
    segs = np.zeros(eng.num_segments, tbp.SEG_DTYPE)
    for s in range(eng.num_segments):
        info = eng.segment_info(s)
        segs[s]["n_docs"], segs[s]["n_postings"], segs[s]["norm_safe"] = info["n_docs"], info["n_postings"], 1
    cfg5 = eng.build_refs(workloads.cfg5_queries(16384))[:2]
    cfg3 = eng.build_refs(workloads.cfg3_queries(4096))[:2]
    small = eng.build_refs(workloads.cfg5_queries(2048, 2005 + 104729))[:2]
    eng.close()
    return segs, cfg5, cfg3, small


@pytest.fixture(scope="module")
def corpus(index_factory):
    return corpus_of(index_factory(4, 30000)[0])   # the inputs of test_batch_plan.py


def parent_cases(segs, cfg5, cfg3, small):
    """name -> the arguments of a plan: the batches of test_batch_plan.py under the settings it plans them with"""
    qd, refs = cfg5
    lists = np.concatenate([tbp.registered(refs, tbp.KIND_SKIP, 64), tbp.registered(refs, tbp.KIND_BMX, single=tbp.single_term(qd, refs))])
    hq, hr = tbp.handmade(segs)
    empty = segs.copy()
    empty[3]["n_docs"], empty[3]["n_postings"] = 0, 0
    cases = {}
    for t in (1, 8):
        for mode in (0, 2):
            cases[f"cfg5_lists_t{t}_order{mode}"] = (segs, qd, refs, dict(lists=lists, prep_threads=t, order_mode=mode, use_pruning=1))
    cases["cfg5_plain"] = (segs, qd, refs, dict(prep_threads=8))
    cases["cfg5_share2"] = (segs, qd, refs, dict(share_mode=2))
    cases["cfg5_and"] = (segs, qd, refs, dict(flags=1, lists=lists, use_pruning=1, prep_threads=8))
    cases["cfg3_k100"] = (segs, cfg3[0], cfg3[1], dict(k=100, prep_threads=8))
    cases["small"] = (segs, small[0], small[1], dict(prep_threads=8, order_mode=2))
    cases["handmade"] = (empty, hq, hr, dict(share_mode=2))
    one = qd[:1].copy()
    cases["lone_query"] = (segs, one, refs[: int(one[0]["term_count"])], {})
    return cases


def digest(image):
    return hashlib.sha256(image).hexdigest()


def test_mode0_is_the_parent_plan(harness, corpus, tmp_path):
    with open(GOLDEN) as f:   # "digest  name" lines, written from the parent commit's ns_plan.hpp through tests/plan_harness.cpp
        golden = {name: dg for dg, name in (line.split() for line in f if line.strip())}
    old = build(os.path.join(ROOT, "tests", "plan_harness.cpp"), tmp_path)   # its PlanSettings leave class_model at the struct's 0
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    old.plan_batch.argtypes = [vp, vp, u32, vp, u32, vp, vp, u32, u32, u32, vp, u64, vp, vp, C.c_char_p, u32]
    cases = parent_cases(*corpus)
    assert sorted(cases) == sorted(golden)
    for name, (segs, qd, refs, kw) in cases.items():
        p0 = plan(harness, segs, qd, refs, class_model=0, **kw)
        assert digest(p0.image) == golden[name], name
        assert digest(tbp.plan(old, segs, qd, refs, **kw).image) == golden[name], name
        # mode 1: none of these batches fills 256 CUs, so none is touched
        p1 = plan(harness, segs, qd, refs, class_model=1, **kw)
        assert p1.image == p0.image and p1.promoted == 0, name
        assert (p1.general, p1.thin, p1.tile) == (p0.general, p0.thin, p0.tile)


# ---- the rule, restated ---------------------------------------------------------------------------------------------------

N_DOCS = 1_000_000
# one segment of 1 M docs (977 tiles); list i holds COUNTS[i] postings
COUNTS = [120000, 60000, 20000, 300000, 40000, 9000, 2500, 700, 150, 64000, 32000, 16000, 8000, 200000, 100000, 50000, 1200, 977, 400000]
FIRST = np.concatenate([[0], np.cumsum(COUNTS)[:-1]]).astype(np.int64)
SEGS = np.zeros(1, tbp.SEG_DTYPE)
SEGS[0]["n_docs"], SEGS[0]["n_postings"], SEGS[0]["norm_safe"] = N_DOCS, int(sum(COUNTS)), 1


def refs_of(queries):
    """queries: lists of list numbers"""
    qd = np.zeros(len(queries), nsbind.QDESC_DTYPE)
    refs = []
    for qi, q in enumerate(queries):
        qd[qi] = (len(refs), len(q))
        refs.extend((0, COUNTS[li], 8 * int(FIRST[li]), 2.0, 1.0) for li in q)
    return qd, np.array(refs, nsbind.TERM_DTYPE)


def model(counts, n_docs, p, margin=None):
    """(class, merge, promoted, work estimate) of a group of lists under class-model mode 2"""
    margin = p.margin_pct if margin is None else margin
    cost, cmax = sum(counts), max(counts)
    rest = cost - cmax
    tiles = -(-n_docs // TILE_DOCS)
    occ = sum(int(OCC256[min(c * 8 // tiles, 64)]) for c in counts)
    tile = (p.cost_tile16 * tiles + p.cost_visit16 * (tiles * occ // 256) + p.cost_posting16 * cost + 15) // 16
    if rest * 32 <= cmax:
        return 1, False, False, cmax + rest * WORK_FOREIGN
    if len(counts) >= 2 and cost * 64 >= n_docs * 16:
        return 2, False, False, tile
    merge = len(counts) == 2 and rest * 8 >= cmax
    general = cmax + rest * (WORK_MERGE if merge else WORK_FOREIGN)
    if len(counts) >= 2 and tile * margin <= general * 100:
        return 2, False, True, tile
    return 0, merge, False, general


QUERIES = [[0, 1, 2],            # the issue's example: 120 k + 60 k + 20 k
           [3, 4, 5], [3, 4], [3, 6, 7], [3, 8], [3],
           [9, 10], [9, 11], [9, 12], [10, 11], [11, 12], [4, 4],       # two lists: against the merge cost, or (9 + 12: 8 : 1) not
           [13, 14], [13, 15, 16], [14, 15, 5], [15, 10, 11], [15, 11, 12, 6], [1, 2, 5, 6, 7, 8],
           [18, 0], [0, 14], [0, 5, 6], [0, 10, 11, 12], [4, 10, 11], [12, 5, 6, 7, 8, 16, 17], [17, 17, 17], [2, 11, 12]]


def check_against_model(p, queries, margin=None):
    assert p.n_groups == len(queries)
    n = [0, 0, 0, 0]
    for g, q in zip(p.groups, queries):
        cls, merge, promoted, work = model([COUNTS[i] for i in q], N_DOCS, p, margin)
        assert (int(g["cls"]), bool(g["merge2"]), bool(g["promoted"]), int(g["work"])) == (cls, merge, promoted, work), q
        n[cls] += 1
        n[3] += promoted
    assert [p.general, p.thin, p.tile, p.promoted] == n


def test_mode2_follows_the_model(harness):
    qd, refs = refs_of(QUERIES)
    p = plan(harness, SEGS, qd, refs, class_model=2)
    check_against_model(p, QUERIES)
    cls = {tuple(q): (int(g["cls"]), bool(g["promoted"]), bool(g["merge2"])) for g, q in zip(p.groups, QUERIES)}
    # both sides of every boundary are present
    assert cls[(0, 1, 2)] == (2, True, False)                                      # heavy foreign share, 0.2 postings per doc: promoted
    assert cls[(0, 5, 6)] == (0, False, False) and cls[(3, 6, 7)] == (1, False, False)  # light foreign share stays; thin stays
    assert cls[(13, 14)] == (2, False, False)                                      # dense by the density rule: no promotion to count
    promoted2 = [q for q in QUERIES if len(q) == 2 and cls[tuple(q)][1]]
    merged2 = [q for q in QUERIES if len(q) == 2 and cls[tuple(q)][2]]
    assert promoted2 and merged2, (promoted2, merged2)                             # two-term groups on both sides of the merge cost
    assert any(v == (0, False, False) for q, v in cls.items() if len(q) >= 3) and sum(v[1] for v in cls.values()) >= 4
    # the margin moves the boundary, and only the boundary
    for margin in (100, 200, 400):
        pm = plan(harness, SEGS, qd, refs, class_model=2, class_margin_pct=margin)
        check_against_model(pm, QUERIES, margin)
    assert plan(harness, SEGS, qd, refs, class_model=2, class_margin_pct=1000).promoted < p.promoted
    # mode 0: the density rule, the old estimate
    p0 = plan(harness, SEGS, qd, refs, class_model=0)
    assert p0.promoted == 0
    for g in p0.groups:
        if g["cls"] == 2:
            assert int(g["work"]) == WORK_TILE_OLD * int(g["cost"])
    # mode 1: this batch is far from filling 256 CUs
    assert plan(harness, SEGS, qd, refs, class_model=1).image == p0.image


def test_mode1_needs_a_full_batch(harness):
    # 4096 copies of the issue's example: 3.1 G work units, 127 k per CU slot share: the batch fills the chip
    q = [[0, 1, 2]] * 4096 + [[0, 5, 6]] * 64
    qd, refs = refs_of(q)
    p1 = plan(harness, SEGS, qd, refs, class_model=1)
    assert p1.promoted == 4096 and p1.tile == 4096 and p1.general == 64
    check_against_model(p1, q)
    p0 = plan(harness, SEGS, qd, refs, class_model=0)
    assert p0.promoted == 0 and p0.general == 4096 + 64 and p0.image != p1.image
    # a forced split is a sweep's setting: the model keeps out of it; a quarter of the batch no longer fills the chip
    assert plan(harness, SEGS, qd, refs, class_model=1, split_postings=65536).promoted == 0
    qs, rs = refs_of(q[:1024])
    assert plan(harness, SEGS, qs, rs, class_model=1).promoted == 0
    assert plan(harness, SEGS, qs, rs, class_model=2).promoted == 1024


def check_tiling(p, n_queries):
    w = p.witems
    assert np.array_equal(np.sort(w["out_slot"]), np.arange(p.n_rows))
    o = np.lexsort((w["doc_lo"], w["query"]))
    w = w[o]
    start = np.ones(len(w), bool)
    start[1:] = w["query"][1:] != w["query"][:-1]
    assert int(start.sum()) == n_queries
    assert np.all(w["doc_lo"][start] == 0) and np.all(w["doc_hi"][np.roll(start, -1)] == N_DOCS)
    assert np.all(w["doc_lo"] < w["doc_hi"]) and np.all(w["doc_lo"][~start] == w["doc_hi"][np.flatnonzero(~start) - 1])
    return w


def test_items_tile_the_doc_space_and_carry_the_class(harness):
    rng = np.random.default_rng(11)
    q = [QUERIES[int(i)] for i in rng.integers(0, len(QUERIES), 12000)]
    qd, refs = refs_of(q)
    skips = np.zeros(len(COUNTS), tbp.LIST_DTYPE)
    for li in range(len(COUNTS)):
        skips[li] = (0, tbp.KIND_SKIP, FIRST[li], COUNTS[li], 0, 1024 * li)
    for lists in (None, skips):
        images = {}
        for t in (1, 3, 8):
            p = plan(harness, SEGS, qd, refs, lists=lists, class_model=2, prep_threads=t, order_mode=2)
            assert p.width == t
            images[t] = p.image
        assert images[1] == images[3] == images[8]          # every descriptor byte is independent of the planner threads
        check_against_model(p, q)
        w = check_tiling(p, len(q))
        # an item runs the body of its group's class: bit 1 doc tiles, bit 2 thin, bit 8 merge
        by_query = {int(g["query"]): g for g in p.groups}
        for it in w[:: 7]:
            g = by_query[int(it["query"])]
            assert bool(it["whole"] & 2) == (g["cls"] == 2) and bool(it["whole"] & 4) == (g["cls"] == 1)
            assert bool(it["whole"] & 256) == bool(g["merge2"]) and not (g["promoted"] and g["merge2"])
        if lists is not None:   # promoted groups walk the skip grid like every tile group
            promoted = {int(g["query"]) for g in p.groups if g["promoted"]}
            assert promoted and all(it["whole"] & 32 for it in w if int(it["query"]) in promoted)


def test_the_estimate_cuts_and_orders_the_promoted_group(harness):
    # a promoted group is cut by the model's estimate, with the doubled share of a tile group: fewer ranges than under mode 0
    q = [[0, 1, 2]] * 4096
    qd, refs = refs_of(q)
    p0, p2 = plan(harness, SEGS, qd, refs, class_model=0), plan(harness, SEGS, qd, refs, class_model=2)
    _, _, promoted, work = model([COUNTS[i] for i in q[0]], N_DOCS, p2)
    assert promoted and np.all(p2.groups["work"] == work) and np.all(p0.groups["work"] == 120000 + 8 * 80000)
    n0, n2 = p0.n_witems // 4096, p2.n_witems // 4096
    assert n0 * 4096 == p0.n_witems and n2 * 4096 == p2.n_witems
    share = 98304

    def ranges(work, sp):
        want = -(-work // sp)
        p2_ = 1
        while p2_ < want:
            p2_ <<= 1
        if want > 1 and want * want * 2 < p2_ * p2_:
            p2_ >>= 1
        return p2_
    assert n0 == ranges(760000, share) and n2 == ranges(work, 2 * share)


def test_forcing_moves_one_bin(harness):
    qd, refs = refs_of(QUERIES)
    base = plan(harness, SEGS, qd, refs, class_model=0)
    moved = 0
    for share10 in range(10):
        for lo, hi in ((2, 4), (4, 8), (8, 12), (12, 16)):
            p = plan(harness, SEGS, qd, refs, class_model=0, force_body=1, force_share10=share10, force_dens_lo=lo, force_dens_hi=hi)
            for g, g0, q in zip(p.groups, base.groups, QUERIES):
                cost, rest = int(g0["cost"]), int(g0["cost"] - g0["cmax"])
                inbin = g0["cls"] == 0 and len(q) >= 3 and rest * 10 // cost == share10 and lo <= cost * 64 // N_DOCS < hi
                assert bool(g["promoted"]) == bool(inbin), (q, share10, lo, hi)
                assert int(g["cls"]) == (2 if inbin else int(g0["cls"]))
                moved += bool(inbin)
            # forced to the general body: the model may not promote the bin
            pg = plan(harness, SEGS, qd, refs, class_model=2, force_body=2, force_share10=share10, force_dens_lo=lo, force_dens_hi=hi)
            p2 = plan(harness, SEGS, qd, refs, class_model=2)
            assert pg.promoted == p2.promoted - sum(1 for g, f in zip(p2.groups, p.groups) if g["promoted"] and f["promoted"])
    assert moved >= 3
