"""CPU tests of the planner's shared top rows (nextsearch-api_amd/csrc/ns_plan.hpp "shared top rows") through
tests/row_plan_harness.cpp: which groups are row-eligible, how keys share producers, that the cells of a key tile the doc
space and every consumer range is its producer's, and that the descriptor image does not depend on the planner threads.
No GPU: the harness plans over a fake segment."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nsbind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")

OUT = ["bytes", "o_witems", "o_terms", "o_ritems", "o_pitems", "n_witems", "n_dterms", "n_ritems", "n_pitems", "n_pterms",
       "n_rows", "direct", "shared", "width"]
SEG_DTYPE = np.dtype([("n_docs", "<u4"), ("norm_safe", "<u4"), ("packed", "<u4"), ("pad", "<u4"), ("n_postings", "<u8")])
LIST_DTYPE = np.dtype([("seg", "<u4"), ("kind", "<u4"), ("first", "<u4"), ("count", "<u4"), ("idf_bits", "<u4"), ("entry", "<u4")])
WITEM_FIELDS = ("query", "seg", "term_begin", "term_count", "doc_lo", "doc_hi", "out_slot", "whole")
WITEM = np.dtype([(f, "<u4") for f in WITEM_FIELDS])
RITEM = np.dtype([(f, "<u4") for f in WITEM_FIELDS + ("row", "dterm")])
DTERM = np.dtype([("list_off", "<u8"), ("count", "<u4"), ("idf", "<f4"), ("weight", "<f4"), ("seg", "<u4"), ("skip", "<u4"), ("bmx", "<u4")])
KIND_SKIP = 1
SKIP_DOCS = 1024

# one segment of 200 000 docs: hot lists H0 (150 000 postings: 4 cells of <= 65536), H1 (70 000: 2 cells), H2 (40 000: 1 cell),
# then tails of 100 postings each
N_DOCS = 200000
HOT = [150000, 70000, 40000]
N_TAILS = 40
COUNTS = HOT + [100] * N_TAILS
FIRST = np.concatenate([[0], np.cumsum(COUNTS)[:-1]]).astype(np.int64)
SEGS = np.zeros(1, SEG_DTYPE)
SEGS[0]["n_docs"], SEGS[0]["n_postings"], SEGS[0]["norm_safe"] = N_DOCS, int(sum(COUNTS)), 1


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rowplan") / "row_plan_harness.so")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + CSRC, "-o", so, os.path.join(ROOT, "tests", "row_plan_harness.cpp"), "-lpthread"], check=True)
    lib = C.CDLL(so)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.plan_rows.argtypes = [vp, vp, u32, vp, u32, vp, vp, u32, u32, u32, vp, u64, vp, C.c_char_p, u32]
    return lib


def skip_lists(which=range(len(COUNTS))):
    out = np.zeros(len(list(which)), LIST_DTYPE)
    for i, li in enumerate(which):
        out[i] = (0, KIND_SKIP, FIRST[li], COUNTS[li], 0, 256 * li)
    return out


def refs_of(queries):
    """queries: lists of (list number, idf, weight)"""
    qd = np.zeros(len(queries), nsbind.QDESC_DTYPE)
    refs = []
    for qi, q in enumerate(queries):
        qd[qi] = (len(refs), len(q))
        refs.extend((0, COUNTS[li], 8 * int(FIRST[li]), idf, w) for li, idf, w in q)
    return qd, np.array(refs, nsbind.TERM_DTYPE)


class Plan:
    pass


def plan(harness, queries, k=10, flags=0, lists=None, row_mode=1, min_users=4, cell=65536, share_mode=2, use_skips=1, threads=1,
         pruning=0, order_mode=1):
    qd, refs = refs_of(queries)
    lists = skip_lists() if lists is None else lists
    settings = np.array([row_mode, min_users, cell, share_mode, use_skips, threads, pruning, order_mode], np.uint64)
    out = np.zeros(len(OUT), np.uint64)
    err = C.create_string_buffer(512)
    image = np.zeros(16 << 20, np.uint8)
    rc = harness.plan_rows(settings.ctypes.data, SEGS.ctypes.data, 1, lists.ctypes.data, len(lists), qd.ctypes.data, refs.ctypes.data,
                           len(qd), k, flags, image.ctypes.data, image.nbytes, out.ctypes.data, err, len(err))
    assert rc == 0, (rc, err.value.decode())
    p = Plan()
    p.__dict__.update(dict(zip(OUT, (int(x) for x in out))))
    p.image = image[: p.bytes].tobytes()
    p.witems = np.frombuffer(p.image, WITEM, p.n_witems, p.o_witems)
    p.ritems = np.frombuffer(p.image, RITEM, p.n_ritems, p.o_ritems)
    p.pitems = np.frombuffer(p.image, WITEM, p.n_pitems, p.o_pitems)
    p.terms = np.frombuffer(p.image, DTERM, p.n_dterms + p.n_pterms, p.o_terms)
    return p


def thin_queries(hot, n, idf=2.0, w=1.0, tails=1):
    """n queries naming hot list `hot` and `tails` tail lists each"""
    return [[(hot, idf, w)] + [(len(HOT) + (i * tails + t) % N_TAILS, 3.0, 1.0) for t in range(tails)] for i in range(n)]


def test_eligibility(harness):
    q = thin_queries(0, 4)
    p = plan(harness, q)
    assert p.shared and p.n_ritems == 4 * 4 and p.n_pitems == 4 and p.n_pterms == 1
    assert len(p.witems) == 0
    # each of these disqualifies on its own
    assert plan(harness, q, k=33).n_ritems == 0
    assert plan(harness, q, k=32).n_ritems == 16
    assert plan(harness, q, flags=nsbind.NS_FLAG_AND).n_ritems == 0
    assert plan(harness, q, lists=skip_lists(range(1, len(COUNTS)))).n_ritems == 0      # the driver has no skip table
    assert plan(harness, q[:3]).n_ritems == 0                                            # three users under mode 1
    assert plan(harness, q[:3], row_mode=2).n_ritems == 12                               # ... which mode 2 waives
    assert plan(harness, q, min_users=5).n_ritems == 0
    p0 = plan(harness, q, share_mode=0)                                                  # a non-sharing batch
    assert not p0.shared and p0.n_ritems == 0 and p0.n_pitems == 0
    assert plan(harness, q, row_mode=0).n_ritems == 0
    # a negative weight (signed input), a general-class group and a group of more than 16 term refs stay where they were
    assert plan(harness, thin_queries(0, 4, w=-1.0)).n_ritems == 0
    assert plan(harness, [[(0, 2.0, 1.0), (1, 2.0, 1.0)]] * 4).n_ritems == 0
    assert plan(harness, thin_queries(0, 4, tails=17)).n_ritems == 0
    assert plan(harness, thin_queries(0, 4, tails=15)).n_ritems == 16
    # a batch without rows keeps the image of a batch planned with rows off
    assert plan(harness, q[:3]).image == plan(harness, q[:3], row_mode=0).image


def test_keys_share_producers(harness):
    same = plan(harness, thin_queries(1, 8))
    assert same.n_pterms == 1 and same.n_pitems == 2 and same.n_ritems == 16
    # another weight: a key of its own, with its own producers.  (Another idf is part of the key as well, but one batch
    # cannot hold it: a list named with two idfs refuses the sharing of term scores, and with it the rows.)
    p = plan(harness, thin_queries(1, 4) + thin_queries(1, 4, idf=2.5))
    assert not p.shared and p.n_pterms == 0 and p.n_ritems == 0
    for other in (thin_queries(1, 4, w=0.5), thin_queries(1, 4, w=2.0)):
        p = plan(harness, thin_queries(1, 4) + other)
        assert p.n_pterms == 2 and p.n_pitems == 4 and p.n_ritems == 16
        pt = p.terms[p.n_dterms:]
        assert np.all(pt["list_off"] == FIRST[1]) and np.all(pt["count"] == COUNTS[1]) and np.all(pt["skip"] == 256 * 1 + 1)
        assert (pt["idf"][0], pt["weight"][0]) != (pt["idf"][1], pt["weight"][1])
        rows = {(int(r["row"]), float(p.terms[r["term_begin"] + r["dterm"]]["weight"]), float(p.terms[r["term_begin"] + r["dterm"]]["idf"]))
                for r in p.ritems}
        for row, w, idf in rows:   # a consumer's row is a row of ITS key
            prod = p.pitems[row]
            t = p.terms[prod["term_begin"]]
            assert (float(t["weight"]), float(t["idf"])) == (w, idf)
    # two hot lists in one batch; the users of the third stay below the rule
    p = plan(harness, thin_queries(0, 5) + thin_queries(1, 4) + thin_queries(2, 3))
    assert p.n_pterms == 2 and p.n_pitems == 4 + 2 and p.n_ritems == 5 * 4 + 4 * 2
    assert len(p.witems) > 0 and set(p.witems["query"].tolist()) == {9, 10, 11}
    # single-term groups on the hot list are users like any other
    p = plan(harness, [[(2, 2.0, 1.0)]] * 4)
    assert p.n_pitems == 1 and p.n_ritems == 4 and p.direct


def check_cells(p):
    # producers of one key: consecutive rows, ranges that tile [0, n_docs) on the skip grid
    assert np.array_equal(p.pitems["out_slot"], np.arange(p.n_pitems))
    for tb in np.unique(p.pitems["term_begin"]):
        cells = p.pitems[p.pitems["term_begin"] == tb]
        assert cells["doc_lo"][0] == 0 and cells["doc_hi"][-1] == N_DOCS
        assert np.array_equal(cells["doc_lo"][1:], cells["doc_hi"][:-1])
        assert np.all(cells["doc_lo"] % SKIP_DOCS == 0) and np.all(cells["doc_lo"] < cells["doc_hi"])
        n = len(cells)
        assert n & (n - 1) == 0
        assert np.all(cells["term_count"] == 1) and np.all(cells["whole"] & 4) and np.all(cells["whole"] & 64)
    # every consumer: its range is its producer's, its hot term is its producer's list, rows of a group are contiguous
    for r in p.ritems:
        prod = p.pitems[r["row"]]
        assert (r["doc_lo"], r["doc_hi"], r["seg"]) == (prod["doc_lo"], prod["doc_hi"], prod["seg"])
        t, pt = p.terms[r["term_begin"] + r["dterm"]], p.terms[prod["term_begin"]]
        for f in ("list_off", "count", "idf", "weight", "skip"):
            assert t[f] == pt[f]
        assert r["whole"] & 4 and r["whole"] & 64 and not r["whole"] & 16 and r["dterm"] < r["term_count"]
    slots = np.concatenate([p.witems["out_slot"], p.ritems["out_slot"]])
    assert np.array_equal(np.sort(slots), np.arange(p.n_rows))
    # a group's consumers tile the doc space too
    o = np.lexsort((p.ritems["doc_lo"], p.ritems["query"]))
    r = p.ritems[o]
    start = np.ones(len(r), bool)
    start[1:] = r["query"][1:] != r["query"][:-1]
    assert np.all(r["doc_lo"][start] == 0) and np.all(r["doc_hi"][np.roll(start, -1)] == N_DOCS)
    assert np.all(r["doc_lo"][~start] == r["doc_hi"][np.flatnonzero(~start) - 1])


def test_cells_tile_the_doc_space(harness):
    q = thin_queries(0, 6, tails=3) + thin_queries(1, 4) + thin_queries(2, 4, tails=2)
    p = plan(harness, q)
    assert p.n_pitems == 4 + 2 + 1
    check_cells(p)
    # the cell size decides the cut: 150 000 postings in cells of at most 20 000 -> 8 cells, of 1 000 -> 128
    for cell, cells in ((20000, 8), (1000, 128), (1 << 20, 1)):
        p = plan(harness, thin_queries(0, 4), cell=cell)
        assert p.n_pitems == cells and p.n_ritems == 4 * cells
        check_cells(p)
    # never more cells than skip-grid cells: 200 000 docs hold 195 whole ones -> 128
    p = plan(harness, thin_queries(0, 4), cell=1)
    assert p.n_pitems == 128
    check_cells(p)
    # consumers are ordered by estimated work, longest first: more tails first
    p = plan(harness, thin_queries(0, 4, tails=1) + thin_queries(0, 4, tails=12))
    tc = p.ritems["term_count"]
    assert np.all(tc[: len(tc) // 2] == 13) and np.all(tc[len(tc) // 2:] == 2)


def test_image_independent_of_planner_threads(harness):
    rng = np.random.default_rng(5)
    q = []
    for i in range(12000):
        hot = int(rng.integers(0, 3))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            q.append([(hot, 2.0, 1.0)])
        elif kind == 1:
            q.append([(hot, 2.0, 1.0), (1 if hot != 1 else 0, 2.0, 1.0)])   # two hot lists: not thin
        else:
            t = [(len(HOT) + int(x), 3.0, 1.0) for x in rng.choice(N_TAILS, size=int(rng.integers(1, 4)), replace=False)]
            t.insert(int(rng.integers(0, len(t) + 1)), (hot, 2.0, 0.5 if i % 7 == 0 else 1.0))
            q.append(t)
    # (order_mode 2: the XCD dealing of the scoring launch's items on, whatever the number of threads; mode 1 turns it on
    # from four threads, for the host time it costs)
    p1 = plan(harness, q, threads=1, order_mode=2)
    p8 = plan(harness, q, threads=8, order_mode=2)
    assert p1.width == 1 and p8.width == 8
    assert p1.n_ritems > 1000 and p1.n_pterms == 6 and len(p1.witems) > 1000
    assert p1.image == p8.image
    check_cells(p8)
