"""What the merge and the inversion plan on the host before they touch the device (csrc/ns_merge_plan.hpp, invert_plan in
csrc/ns_radix_plan.hpp): merge_plan and invert_plan through tests/merge_plan_harness.cpp against a restatement
in plain Python, on directed shapes.  Every output array is compared exactly and every refusal by its message.  The same
cases run once more through the harness built as a program of its own under the host sanitizers.  No device is touched."""
import bisect
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compact_ref
import delete_ref
import nsbind
import radix_shapes as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "merge_plan_harness.cpp")

TILE, WAVE_MAX, DOC_CUT = 4096, 64, 4096     # kIvTile, kCpWaveMax, kCpDocCut: asserted against the header and the library below
PAIR_LIMIT = (1 << 32) - TILE                # the first refused total of pairs
MERGE_ARRAYS = ["term_base", "pair_base", "raw_base", "prefix", "srcpos", "kept_len", "kept_cnt", "live0", "kstart", "klen", "lists"]
MERGE_SCALARS = ["filtered", "raw_pairs", "T", "text_bytes", "n_docs", "n_pairs", "total_len", "n_wave", "n_lds", "n_bigdocs", "n_big"]
INVERT_SCALARS = ["n_tiles", "m_max", "scan_blocks_max", "passes"]


# ---- sources ----------------------------------------------------------------------------------------------------------------
def source(counts, term_lens, first_offset=0, seed=0):
    """a well-formed source: documents of `counts` pairs, terms of `term_lens` bytes; a document of c pairs names the terms
    0 .. c - 1 modulo the number of terms (the plan does not read the pairs; delete_ref does)"""
    rng = np.random.default_rng(seed)
    counts = [int(c) for c in counts]
    n_terms = len(term_lens)
    assert n_terms or not sum(counts)
    ids = np.concatenate([np.arange(c) % max(n_terms, 1) for c in counts] + [np.empty(0, dtype=np.int64)])
    pairs = np.stack([ids, np.ones_like(ids)], axis=1).astype(np.uint32)
    offsets = first_offset + np.concatenate([[0], np.cumsum(term_lens, dtype=np.int64)])
    return {"n_docs": len(counts), "n_pairs": sum(counts), "n_terms": n_terms,
            "doc_len": rng.integers(1, 1000, len(counts)).astype(np.uint32), "counts": np.array(counts, dtype=np.uint32), "pairs": pairs.reshape(-1),
            "term_bytes": np.zeros(first_offset + sum(term_lens), dtype=np.uint8), "term_offsets": offsets.astype(np.uint64) if n_terms else None}


def scalars_only(n_docs=0, n_pairs=0, n_terms=0):
    return {"n_docs": n_docs, "n_pairs": n_pairs, "n_terms": n_terms, "doc_len": None, "counts": None, "pairs": None, "term_bytes": None, "term_offsets": None}


def changed(src, **fields):
    out = dict(src)
    out.update(fields)
    return out


# ---- the words of a case and of an answer (tests/merge_plan_harness.cpp) ---------------------------------------------------
def _array(a):
    if a is None:
        return [0, 0]
    a = np.asarray(a).reshape(-1)
    return [1, len(a)] + [int(v) for v in a]


def merge_case(srcs, keeps, cp_inplace):
    """keeps: None, or per source None or a boolean array over its documents (uploaded as delete_ref.bitmap's words, random
    bits behind the last document)"""
    w = [0, len(srcs), int(cp_inplace), int(keeps is not None)]
    for s, S in enumerate(srcs):
        w += [S["n_docs"], S["n_pairs"], S["n_terms"]]
        for k in ("doc_len", "counts", "pairs", "term_bytes", "term_offsets"):
            w += _array(S[k])
        keep = None if keeps is None else keeps[s]
        w += _array(None if keep is None else delete_ref.bitmap(keep, garbage_seed=7 + s))
    return np.array(w, dtype=np.uint64)


def invert_case(counts, n_pairs, n_terms):
    return np.array([1, len(counts), n_pairs, n_terms] + _array(np.asarray(counts, dtype=np.uint32)), dtype=np.uint64)


def decode(words, scalars, arrays):
    """an answer -> the refusal's text, or {name: value}"""
    words = [int(v) for v in words]
    if words[0] == 0:
        assert len(words) == 2 + words[1]
        return bytes(words[2:]).decode()
    out = dict(zip(scalars, words[1:1 + len(scalars)]))
    at = 1 + len(scalars)
    for name in arrays:
        n = words[at]
        out[name] = words[at + 1:at + 1 + n]
        at += 1 + n
    assert at == len(words)
    return out


def decode_for(case, words):
    return decode(words, MERGE_SCALARS, MERGE_ARRAYS) if int(case[0]) == 0 else decode(words, INVERT_SCALARS, ["prefix", "tile_docs"])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("merge_plan") / "merge_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I" + CSRC, "-o", so, HARNESS], check=True)
    lib = C.CDLL(so)
    lib.plan_case.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.plan_case.restype = C.c_int64
    return lib


def run(lib, case):
    out = np.zeros(1 << 16, dtype=np.uint64)
    n = lib.plan_case(case.ctypes.data, len(case), out.ctypes.data, len(out))
    assert 0 <= n <= len(out), n
    return decode_for(case, out[:n])


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def merge_ref(srcs, keeps, cp_inplace):
    docs = pairs = terms = 0
    for s, S in enumerate(srcs):                                   # the totals read the scalar fields alone
        docs, terms, pairs = docs + S["n_docs"], terms + S["n_terms"], pairs + S["n_pairs"]
        if S["n_pairs"] >= 1 << 32 or pairs >= PAIR_LIMIT:
            return "more than %d pairs up to source %d; this build indexes pairs with 32 bits (compact fewer segments)" % (PAIR_LIMIT - 1, s)
    if docs >= 0xFFFFFFFF:
        return "%d documents; docIds are 32 bits wide (below 2^32 - 1: compact fewer segments)" % docs
    if terms >= 1 << 31:
        return "%d source terms; the dictionary holds fewer than 2^31 (compact fewer segments)" % terms
    nbytes = 0
    for s, S in enumerate(srcs):
        if (S["n_docs"] and (S["doc_len"] is None or S["counts"] is None)) or (S["n_pairs"] and S["pairs"] is None) or (S["n_terms"] and S["term_offsets"] is None):
            return "source %d: null array" % s
        if S["n_terms"]:
            off = [int(v) for v in S["term_offsets"]]
            if off[-1] < off[0]:
                return "source %d: term offsets decrease" % s
            nbytes += off[-1] - off[0]
            if nbytes >= (1 << 32) - 65536:
                return "more than 4 GiB - 64 KiB of term bytes up to source %d; this build addresses them with 32 bits (compact fewer segments)" % s
    for s, S in enumerate(srcs):                                   # source by source: its counts, its offsets, its bytes
        if (int(np.sum(S["counts"], dtype=np.int64)) if S["n_docs"] else 0) != S["n_pairs"]:
            return "source %d: the per-document counts do not sum to n_pairs = %d" % (s, S["n_pairs"])
        off = [int(v) for v in S["term_offsets"]] if S["n_terms"] else [0]
        for t in range(S["n_terms"]):
            if off[t + 1] < off[t]:
                return "source %d: term offsets decrease at term %d" % (s, t)
        if off[-1] != off[0] and S["term_bytes"] is None:
            return "source %d: term_bytes is NULL" % s

    filtered = keeps is not None and any(k is not None for k in keeps)
    keeps = keeps if filtered else [None] * len(srcs)
    # what survives, in the words of delete_ref and compact_ref: a part per source, filtered, then merged
    parts = [{"kept_docs": np.arange(S["n_docs"]), "doc_len": S["doc_len"] if S["n_docs"] else np.empty(0, np.uint32),
              "counts": S["counts"] if S["n_docs"] else np.empty(0, np.uint32), "pairs": S["pairs"] if S["n_pairs"] else np.empty(0, np.uint32),
              "terms": [b"%d" % t for t in range(S["n_terms"])]} for S in srcs]
    stay = [delete_ref.filter_part(p, k) for p, k in zip(parts, keeps)]
    merged = compact_ref.merge(stay)
    counts = [int(c) for c in merged["counts"]]
    out = {"filtered": int(filtered), "raw_pairs": pairs, "T": terms, "text_bytes": nbytes, "n_docs": len(counts), "n_pairs": len(merged["pairs"]),
           "total_len": int(np.sum(merged["doc_len"], dtype=np.int64))}
    assert out["n_pairs"] == sum(counts)
    out["term_base"] = [sum(S["n_terms"] for S in srcs[:s]) for s in range(len(srcs) + 1)]
    out["pair_base"] = [sum(np.asarray(p["pairs"]).size // 2 for p in stay[:s]) for s in range(len(srcs) + 1)]
    out["prefix"] = [sum(counts[:d]) for d in range(len(counts) + 1)]
    out["kstart"], out["klen"], at = [], [], 0
    for S in srcs:
        off = [int(v) for v in S["term_offsets"]] if S["n_terms"] else [0]
        out["kstart"] += [at + o - off[0] for o in off[:-1]]
        out["klen"] += [b - a for a, b in zip(off[:-1], off[1:])]
        at += off[-1] - off[0]
    out.update({"raw_base": [], "srcpos": [], "kept_len": [], "kept_cnt": [], "live0": []})
    if filtered:
        out["raw_base"] = [sum(S["n_pairs"] for S in srcs[:s]) for s in range(len(srcs) + 1)]
        out["kept_len"], out["kept_cnt"] = [int(v) for v in merged["doc_len"]], counts
        for s, (S, k) in enumerate(zip(srcs, keeps)):
            first = np.cumsum(parts[s]["counts"], dtype=np.int64) - parts[s]["counts"]      # a document's first pair in its source
            out["srcpos"] += [out["raw_base"][s] + int(v) for v in (first if k is None else first[np.asarray(k, dtype=bool)])]
            out["live0"] += [int(k is None)] * S["n_terms"]
        out["live0"].append(0)
    wave, lds, big, big_prefix = [], [], [], [0]
    for d, c in enumerate(counts):
        if c < 2:
            continue
        if cp_inplace and c <= WAVE_MAX:
            wave.append(d)
        elif cp_inplace and c <= DOC_CUT:
            lds.append(d)
        else:
            big.append(d)
            big_prefix.append(big_prefix[-1] + c)
    out.update({"n_wave": len(wave), "n_lds": len(lds), "n_bigdocs": len(big), "n_big": big_prefix[-1], "lists": wave + lds + big + big_prefix})
    return out


def invert_ref(counts, n_pairs, n_terms):
    prefix = [0]
    for c in counts:
        prefix.append(prefix[-1] + int(c))
    if prefix[-1] != n_pairs:
        return "the per-document counts sum to %d, not to n_pairs = %d" % (prefix[-1], n_pairs)
    n_tiles = (n_pairs + TILE - 1) // TILE
    digits = rs.plan(n_terms)[1]
    m_max = max((1 << b) * n_tiles for b in digits)
    tile_docs = []
    for t in range(n_tiles):                                       # the last document that starts at or before the pair
        for i in (t * TILE, min((t + 1) * TILE, n_pairs) - 1):
            tile_docs.append(bisect.bisect_right(prefix, i) - 1)
    return {"n_tiles": n_tiles, "m_max": m_max, "scan_blocks_max": (m_max + 1023) // 1024, "passes": len(digits), "prefix": prefix, "tile_docs": tile_docs}


# ---- the cases ----------------------------------------------------------------------------------------------------------------
EDGES = [0, 1, 2, WAVE_MAX, WAVE_MAX + 1, DOC_CUT, DOC_CUT + 1]      # the three class edges: < 2, <= kCpWaveMax, <= kCpDocCut


def merge_cases():
    """-> [(name, srcs, keeps, cp_inplace)]"""
    a = source(EDGES, [3, 1, 4, 1, 5], seed=1)
    b = source([5, 0, 70, 1, 2, 3] + [1] * 31, [2, 7], first_offset=11, seed=2)       # 37 documents: the bitmap's last word is partly used
    no_doc = source([], [4, 4], seed=3)
    no_term = source([0, 0, 0], [], seed=4)
    empty_bytes = source([2, 1], [0, 0, 0], seed=5)
    rng = np.random.default_rng(11)
    some_a, some_b = rng.random(a["n_docs"]) < 0.6, rng.random(b["n_docs"]) < 0.5
    some_a[[2, 4, 6]] = True                                         # a class edge on each side stays
    none_a, none_b = np.zeros(a["n_docs"], dtype=bool), np.zeros(b["n_docs"], dtype=bool)
    cases = [("no source", [], None, True), ("no source, keep given", [], [], True)]
    for inplace in (True, False):
        tag = ", in place" if inplace else ", all big"
        cases += [("class edges" + tag, [a], None, inplace),
                  ("five sources" + tag, [a, no_doc, b, no_term, empty_bytes], None, inplace),
                  ("every bitmap NULL" + tag, [a, no_doc, b, no_term, empty_bytes], [None] * 5, inplace),
                  ("NULL and present bitmaps" + tag, [a, no_doc, b, no_term, empty_bytes], [some_a, None, None, np.ones(3, dtype=bool), None], inplace),
                  ("bitmaps on both" + tag, [a, b], [some_a, some_b], inplace),
                  ("nothing of one source" + tag, [a, b, empty_bytes], [None, none_b, np.array([True, False])], inplace),
                  ("nothing at all" + tag, [a, b], [none_a, none_b], inplace)]
    cases += [("a source alone without a document", [no_doc], None, True), ("a source alone without a term", [no_term], [np.array([True, False, True])], True),
              ("terms with empty bytes alone", [empty_bytes], None, True)]
    # refusals by the arrays
    cases += [("counts above n_pairs", [a, changed(b, counts=b["counts"] + np.uint32(1))], None, True),
              ("counts below n_pairs", [a, changed(b, counts=np.maximum(b["counts"], 1) - np.uint32(1))], [None, some_b], True),
              ("counts above n_pairs, filtered", [changed(a, counts=a["counts"] + np.uint32(2)), b], [none_a, None], True),
              ("offsets decrease in the middle", [a, changed(b, term_offsets=np.array([11, 20, 13, 20], dtype=np.uint64), n_terms=3)], None, True),
              ("offsets decrease from first to last", [changed(a, term_offsets=np.array([9, 12, 13, 17, 18, 8], dtype=np.uint64))], None, True),
              ("term_bytes NULL", [a, changed(b, term_bytes=None)], None, True),
              ("term_bytes NULL, nothing to read", [changed(empty_bytes, term_bytes=None)], None, True),
              ("doc_len NULL", [changed(a, doc_len=None)], None, True), ("pairs NULL", [b, changed(a, pairs=None)], None, True),
              ("term_offsets NULL", [changed(b, term_offsets=None)], None, True),
              ("counts wrong in the first, offsets in the second", [changed(a, n_pairs=a["n_pairs"] + 1), changed(b, term_offsets=np.array([5, 9, 4], dtype=np.uint64))], None, True)]
    # the three 32-bit totals, each at its last accepted and its first refused value: the scalar fields alone, no array
    for name, last_ok in (("pairs", [scalars_only(n_pairs=PAIR_LIMIT - 1)]), ("pairs over two", [scalars_only(n_pairs=PAIR_LIMIT - 8), scalars_only(n_pairs=7)]),
                          ("documents", [scalars_only(n_docs=0xFFFFFFFE)]), ("documents over two", [scalars_only(n_docs=0x80000000), scalars_only(n_docs=0x7FFFFFFE)]),
                          ("terms", [scalars_only(n_terms=(1 << 31) - 1)]), ("terms over two", [scalars_only(n_terms=1 << 30), scalars_only(n_terms=(1 << 30) - 1)])):
        field = {"p": "n_pairs", "d": "n_docs", "t": "n_terms"}[name[0]]
        cases += [("last accepted total of " + name, last_ok, None, True),
                  ("first refused total of " + name, last_ok[:-1] + [changed(last_ok[-1], **{field: last_ok[-1][field] + 1})], None, True)]
    cases.append(("a source of 2^32 pairs", [scalars_only(n_pairs=1 << 32)], None, True))
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def invert_cases():
    """-> [(name, counts, n_pairs, n_terms)]"""
    cases = []
    for n in (TILE - 1, TILE, TILE + 1):
        cases += [("one document of %d" % n, [n], n, 300), ("documents of seven, %d pairs" % n, [7] * (n // 7) + [n % 7], n, 70000)]
    cases += [("empty documents at the front and at the back", [0, 0, 5, 3, 0, 0, 0], 8, 5),
              ("empty documents on both sides of a tile edge", [TILE - 2, 2, 0, 0, 0, 6, 0], TILE + 6, 1 << 22),
              ("a tile edge inside a run of empty documents", [0, TILE, 0, 0, 1], TILE + 1, 2049),
              ("one document over three tiles", [10, 2 * TILE + 100, 3], 2 * TILE + 113, (1 << 22) + 1),
              ("no document", [], 0, 9), ("no pair", [0, 0], 0, 0),
              ("counts above n_pairs", [3, 4], 6, 9), ("counts below n_pairs", [3, 4], TILE, 9)]
    return cases


def all_cases():
    out = [(name, merge_case(s, k, i), lambda s=s, k=k, i=i: merge_ref(s, k, i)) for name, s, k, i in merge_cases()]
    return out + [(name, invert_case(c, n, t), lambda c=c, n=n, t=t: invert_ref(c, n, t)) for name, c, n, t in invert_cases()]


# ---- the tests ----------------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_headers_and_the_librarys(harness):
    k = (C.c_uint32 * 3)()
    harness.plan_consts(k)
    L = nsbind.hip_lib()                             # the getters touch no device
    assert list(k) == [TILE, WAVE_MAX, DOC_CUT] and L.ns_radix_tile() == TILE and L.ns_compact_doc_cut() == DOC_CUT


def test_every_case_equals_the_restatement(harness):
    for name, case, ref in all_cases():
        assert run(harness, case) == ref(), name


def test_the_cases_reach_what_they_are_named_for(harness):
    got = {name: run(harness, merge_case(s, k, i)) for name, s, k, i in merge_cases()}
    refused = {name: g for name, g in got.items() if isinstance(g, str)}
    assert got["no source"] == got["no source, keep given"] and got["no source"]["n_docs"] == 0 and got["no source"]["lists"] == [0]
    for tag in (", in place", ", all big"):
        assert got["every bitmap NULL" + tag] == got["five sources" + tag] and not got["five sources" + tag]["filtered"]
        mix = got["NULL and present bitmaps" + tag]
        assert mix["filtered"] and mix["live0"] == [0] * 5 + [1] * 2 + [1] * 2 + [1] * 3 + [0]           # 1 exactly over the NULL-bitmap sources' terms
        assert 0 < mix["n_docs"] < got["five sources" + tag]["n_docs"]
        one = got["nothing of one source" + tag]
        assert one["pair_base"][1] == one["pair_base"][2] and one["raw_base"][1] != one["raw_base"][2] and one["n_docs"] == 8
        none = got["nothing at all" + tag]
        assert none["n_docs"] == 0 and none["n_pairs"] == 0 and none["prefix"] == [0] and none["raw_pairs"] > 0
    edges, big = got["class edges, in place"], got["class edges, all big"]
    assert (edges["n_wave"], edges["n_lds"], edges["n_bigdocs"], edges["n_big"]) == (2, 2, 1, DOC_CUT + 1)
    assert edges["lists"] == [2, 3, 4, 5, 6, 0, DOC_CUT + 1]
    assert (big["n_wave"], big["n_lds"], big["n_bigdocs"]) == (0, 0, 5) and big["lists"][:5] == [2, 3, 4, 5, 6]
    assert set(refused) == {n for n in got if n.startswith(("counts", "offsets", "term_bytes NULL", "doc_len", "pairs NULL", "term_offsets", "last accepted", "first refused", "a source of 2^32"))} - {"term_bytes NULL, nothing to read"}
    assert refused["offsets decrease in the middle"] == "source 1: term offsets decrease at term 1"
    assert refused["offsets decrease from first to last"] == "source 0: term offsets decrease"
    assert refused["counts wrong in the first, offsets in the second"] == "source 1: term offsets decrease"   # every source's arrays before any walk
    for name in ("pairs", "pairs over two", "documents", "documents over two", "terms", "terms over two"):
        assert refused["last accepted total of " + name] == "source 0: null array", name                        # past the totals, at the first pointer
    assert refused["first refused total of pairs"].startswith("more than %d pairs up to source 0;" % (PAIR_LIMIT - 1))
    assert refused["first refused total of pairs over two"].startswith("more than %d pairs up to source 1;" % (PAIR_LIMIT - 1))
    assert refused["first refused total of documents"].startswith("4294967295 documents;") and refused["first refused total of documents over two"].startswith("4294967295 documents;")
    assert refused["first refused total of terms"].startswith("2147483648 source terms;") and refused["first refused total of terms over two"].startswith("2147483648 source terms;")
    inv = {name: run(harness, invert_case(c, n, t)) for name, c, n, t in invert_cases()}
    assert [inv["one document of %d" % n]["n_tiles"] for n in (TILE - 1, TILE, TILE + 1)] == [1, 1, 2]
    assert inv["empty documents at the front and at the back"]["tile_docs"] == [2, 3]
    assert inv["empty documents on both sides of a tile edge"]["tile_docs"] == [0, 1, 5, 5]
    assert inv["one document over three tiles"]["tile_docs"] == [0, 1, 1, 1, 1, 2] and inv["one document over three tiles"]["passes"] == 3
    assert inv["counts above n_pairs"] == "the per-document counts sum to 7, not to n_pairs = 6"


def test_the_harness_program_under_the_host_sanitizers(tmp_path):
    """the same cases through merge_plan and invert_plan in a program of its own, built with the address and undefined-behaviour
    sanitizers: clean, and the same answers"""
    exe = str(tmp_path / "merge_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMERGE_PLAN_MAIN",
                    "-I" + CSRC, "-o", exe, HARNESS], check=True)
    cases = all_cases()
    with open(tmp_path / "cases", "wb") as f:
        for _, case, _ in cases:
            f.write(np.array([len(case)], dtype=np.uint64).tobytes() + case.tobytes())
    r = subprocess.run([exe, str(tmp_path / "cases"), str(tmp_path / "answers")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "merge_plan_harness: %d cases" % len(cases)
    words = np.fromfile(tmp_path / "answers", dtype=np.uint64)
    at = 0
    for name, case, ref in cases:
        n = int(words[at])
        assert decode_for(case, words[at + 1:at + 1 + n]) == ref(), name
        at += 1 + n
    assert at == len(words)
