"""Related terms, host side (host/related.hpp, csrc/ns_terms_plan.hpp): the host rule through nsbind against the
numpy restatement tests/related_ref.py on every directed shape of tests/related_shapes.py; the plan through
tests/terms_plan_harness.cpp against a restatement here; and tests/related_host_check.cpp, a program of its own under the address
and undefined-behaviour sanitizers.  Integers and fp32 bit patterns, no tolerance.  No device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nsbind
import related_ref
import related_shapes as shapes
from related_shapes import assert_rows_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
HOST = os.path.join(ROOT, "nextsearch-api_amd", "host")
# the CPU suite has no device library call to ask: the directed shapes are built for the product's window and doc cut
W, CUT = 1 << 16, 2048


@pytest.fixture(scope="module")
def directed():
    part, df, idf, docs, rows, n_terms = shapes.directed(W, CUT)
    return {"part": part, "df": df, "idf": idf, "docs": docs, "rows": rows, "n_terms": n_terms}


def want(d, rows, T, o=shapes.OPTION_SETS[0]):
    return related_ref.aggregate_rows(d["part"]["counts"], d["part"]["pairs"], d["df"], d["idf"], rows, T, *o)


def test_the_directed_shapes_are_what_their_names_say(directed):
    d, rows, docs = directed, directed["rows"], directed["docs"]
    assert d["n_terms"] == 2 * W + 7 and d["n_terms"] % 4 != 0
    t, g, w, c, n = want(d, list(rows.values()), 64)
    by = {name: i for i, name in enumerate(rows)}
    assert n[by["empty"]] == 0 and c[by["empty"]] == 0 and n[by["one"]] == 1 and c[by["one"]] == 0           # min_docs 2: one document names nothing
    assert n[by["full 255"]] == 255 == n[by["300 ids, 255 distinct"]] and len(rows["300 ids, 255 distinct"]) == 300
    # 255, 255, 255 and 1 in one word: the three qualify with fg 255, the fourth (held by one document) does not
    full = dict(zip(t[by["full 255"]].tolist(), g[by["full 255"]].tolist()))
    for j in range(25, 30):
        assert full[4 * j] == full[4 * j + 1] == full[4 * j + 2] == 255 and 4 * j + 3 not in full
    for e, m in zip((W - 1, W, 2 * W - 1, 2 * W, d["n_terms"] - 1), (2, 3, 5, 7, 11)):
        assert full[e] == len(range(0, 255, m))                                                            # a term on each side of every window edge
    assert np.array_equal(t[by["full 255"]], t[by["300 ids, 255 distinct"]])
    assert n[by["repeats"]] == 3 and n[by["a document without pairs"]] == 3 and n[by["only a document without pairs"]] == 1
    # the skip path: the row's pairs lie in windows 0 and 2 only
    _, p = related_ref.row_pairs(d["part"]["counts"], d["part"]["pairs"], rows["skip"])
    assert sorted(set((p[:, 0] // W).tolist())) == [0, 2]
    assert related_ref.windows_skipped(d["part"]["counts"], d["part"]["pairs"], d["n_terms"], [rows["skip"], rows["empty"], rows["long"]], W) == 1
    assert d["part"]["counts"][docs["long"]] == CUT + 1
    # more than 64 terms of one weight: the 64 smallest term ids, in order
    assert c[by["ties"]] == 64 and len(set(w[by["ties"]].view(np.uint32).tolist())) == 1
    assert t[by["ties"]].tolist() == (list(range(3100, 3140)) + list(range(W + 3100, W + 3124)))
    # idf 0 / inf / nan never qualify; the overflowing one leads its row with w = inf and fg 3
    odd = by["odd"]
    assert not set(range(4100, 4108)) & set(t[odd].tolist()) and t[odd][0] == 4120 and np.isinf(w[odd][0]) and g[odd][0] == 3
    assert want(d, [rows["odd"]], 64, (2, 2, 1, 0xFFFFFFFF))[1][0][0] == 2                                 # ... and fg 2 under min_tf 2
    # every option decides a term of the options row
    base = set(want(d, [rows["options"]], 64)[0][0].tolist())
    for o in shapes.OPTION_SETS[1:]:
        tt, gg, _, cc, _ = want(d, [rows["options"]], 64, o)
        if o[1] <= 4 and o[0] <= 5 and o != (0, 0, 0, 0xFFFFFFFF) and o != (1, 1, 1, 0xFFFFFFFF):
            assert set(tt[0][:cc[0]].tolist()) != base or gg[0][0] != 4, o
    assert want(d, [rows["full 255"]], 64, (1, 255, 1, 0xFFFFFFFF))[3][0] == 15 and want(d, [rows["full 255"]], 64, (1, 256, 1, 0xFFFFFFFF))[3][0] == 0


@pytest.mark.parametrize("T", shapes.T_VALUES + (0, 1000))
def test_the_host_rule_equals_the_restatement_on_every_shape(directed, T):
    d, batch = directed, list(directed["rows"].values())
    got = nsbind.related_aggregate_host(d["part"], d["df"], d["idf"], batch, T)
    assert got[0].shape == (len(batch), related_ref.clamp_terms(T))
    assert_rows_equal(got, want(d, batch, T), ("batch", T))
    for name, r in d["rows"].items():                                                                      # every row alone
        assert_rows_equal(nsbind.related_aggregate_host(d["part"], d["df"], d["idf"], [r], T), want(d, [r], T), (name, T))


@pytest.mark.parametrize("o", shapes.OPTION_SETS[1:])
def test_the_host_rule_under_every_option_set(directed, o):
    d, batch = directed, list(directed["rows"].values())
    assert_rows_equal(nsbind.related_aggregate_host(d["part"], d["df"], d["idf"], batch, 64, *o), want(d, batch, 64, o), o)


def test_the_host_rule_refuses_what_the_device_call_refuses(directed):
    d, docs = directed, directed["docs"]
    for rows in ([docs["full"] + [docs["extra"]]], [[0, len(d["part"]["counts"])]]):
        with pytest.raises(ValueError):
            nsbind.related_aggregate_host(d["part"], d["df"], d["idf"], rows)
    part, df, idf = shapes.descending_source()
    with pytest.raises(ValueError):
        nsbind.related_aggregate_host(part, df, idf, [[0, 1]])
    assert nsbind.related_aggregate_host(part, df, idf, [[0, 2]], 10, 1, 2)[0][0].tolist()[:2] == [0, 0xFFFFFFFF]   # the row does not visit it
    assert nsbind.related_aggregate_host(part, df, idf, [])[0].shape == (0, 10)


# ---- the plan -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("terms_plan") / "terms_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I" + CSRC, "-o", so, os.path.join(ROOT, "tests", "terms_plan_harness.cpp")], check=True)
    lib = C.CDLL(so)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.terms_plan_run.argtypes = [vp, vp, u32, vp, u32, vp, u64, C.POINTER(u64), vp, vp, vp, C.POINTER(u32), C.c_char_p, u32]
    lib.terms_plan_max_row_docs.restype = u32
    return lib


def plan(harness, rows, counts, row_off=None):
    ids, off = nsbind.related_rows_flat(rows)
    if row_off is not None:
        off = np.asarray(row_off, dtype=np.uint64)
    doc_off = related_ref.doc_offsets(counts).astype(np.uint32)
    n = len(off) - 1
    docs, first, pairs, order = np.zeros(len(ids) + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32)
    nd, over = C.c_uint64(), C.c_uint32()
    err = C.create_string_buffer(256)
    rc = harness.terms_plan_run(ids.ctypes.data, off.ctypes.data, n, doc_off.ctypes.data, len(counts), docs.ctypes.data, len(docs), C.byref(nd), first.ctypes.data,
                                pairs.ctypes.data, order.ctypes.data, C.byref(over), err, len(err))
    return rc, docs[:nd.value].tolist(), first.tolist(), pairs[:n].tolist(), order[:n].tolist(), int(over.value), err.value.decode()


def test_the_plan_equals_its_restatement(harness, directed):
    assert harness.terms_plan_max_row_docs() == 255 == related_ref.MAX_ROW_DOCS
    counts, rows = directed["part"]["counts"], list(directed["rows"].values())
    rc, docs, first, pairs, order, over, msg = plan(harness, rows, counts)
    assert rc == 1 and over == 0 and msg == ""
    uniq = [sorted(set(r)) for r in rows]
    assert docs == [x for r in uniq for x in r] and first == np.concatenate([[0], np.cumsum([len(r) for r in uniq])]).tolist()
    assert pairs == [int(sum(int(counts[x]) for x in r)) for r in uniq]
    assert order == sorted(range(len(rows)), key=lambda i: (-pairs[i], i)) and pairs[order[0]] > pairs[order[-1]] == 0
    assert plan(harness, [], counts)[:5] == (1, [], [0], [], [])


def test_the_plan_refuses_with_a_message(harness, directed):
    counts, docs = directed["part"]["counts"], directed["docs"]
    big = docs["full"] + [docs["extra"]]
    for rows, kw, over, match in (([[1], big, [2]], {}, 1, "row 1 names 256 distinct documents; a row holds at most 255"),
                                  ([big, big + big], {}, 2, "row 0 names 256 distinct documents"),
                                  ([[0, 1], [2, len(counts)]], {}, 0, "doc_ids[3] = %d (row 1), the handle holds %d documents" % (len(counts), len(counts))),
                                  ([[0, 1], [2]], {"row_off": [1, 2, 3]}, 0, "row_off[0] = 1, not 0"),
                                  ([[0, 1], [2]], {"row_off": [0, 2, 1]}, 0, "row_off[2] = 1 is below row_off[1] = 2")):
        rc, d, first, _, _, n_over, msg = plan(harness, rows, counts, **kw)
        assert rc == 0 and d == [] and n_over == over and match in msg, (msg, match)
    assert plan(harness, [docs["full"] + docs["full"][:45]], counts)[0] == 1                               # 300 ids, 255 distinct


def test_the_plan_and_the_host_rule_under_the_sanitizers(tmp_path, directed):
    """tests/related_host_check.cpp, a program of its own, built with -fsanitize=address,undefined and run here on the directed shapes"""
    d, batch = directed, list(directed["rows"].values())
    ids, off = nsbind.related_rows_flat(batch)
    ids = ids[:int(off[-1])]
    shapes_bin, answers = str(tmp_path / "shapes.bin"), str(tmp_path / "answers.bin")
    with open(shapes_bin, "wb") as f:
        f.write(np.asarray([len(d["part"]["counts"]), len(d["part"]["pairs"]), len(d["df"]), len(batch), len(ids)], np.uint64).tobytes())
        for a, t in ((d["part"]["counts"], np.uint32), (d["part"]["pairs"], np.uint32), (d["df"], np.uint32), (d["idf"], np.float32), (off, np.uint64), (ids, np.uint32)):
            f.write(np.ascontiguousarray(a, dtype=t).tobytes())
    exe = str(tmp_path / "related_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + CSRC, "-I" + HOST, "-o", exe, os.path.join(ROOT, "tests", "related_host_check.cpp")], check=True)
    out = subprocess.run([exe, shapes_bin, answers], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "related host check OK" in out.stdout, (out.stdout + out.stderr)[-3000:]
    raw = np.fromfile(answers, dtype=np.uint32)
    n = len(batch)
    assert len(raw) == 3 * n * 64 + 2 * n
    got = (raw[:n * 64].reshape(n, 64), raw[n * 64:2 * n * 64].reshape(n, 64), raw[2 * n * 64:3 * n * 64].reshape(n, 64).view(np.float32), raw[3 * n * 64:3 * n * 64 + n],
           raw[3 * n * 64 + n:])
    assert_rows_equal(got, want(d, batch, 64), "sanitized program")


def test_a_host_only_engine_answers_no_related_terms_and_says_so(tmp_path):
    index = str(tmp_path / "index")
    nsbind.gen_index(index, 2, 45, 512, 77, False)
    eng = nsbind.Engine(index, -1)
    try:
        with pytest.raises(RuntimeError, match="terms_batch: no device context"):
            eng.terms_batch([[(0, 1), (1, 2)]])
        with pytest.raises(RuntimeError, match="related_terms: no device context"):
            eng.related_terms_json("t000001 t000002")
        with pytest.raises(RuntimeError, match=r"\(segment 2, document 0\) is not in the index"):
            eng.terms_batch([[(0, 1), (2, 0)]])
    finally:
        eng.close()
