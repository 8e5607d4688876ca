"""The text rules of indexing (csrc/ns_ingest_text.hpp through tests/ingest_text_harness.cpp) against host/textutil.hpp, against
tests/ingest_ref.py and against their restatement in tests/ingest_shapes.py, and the case table of that module: every case
built, ingest_ref.build on it checked a second way by the byte-loop oracle, and the reach flags of the whole table asserted
complete.  No device is touched; tests/test_ingest_shapes_gpu.py runs the same table through the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compact_ref
import ingest_ref
import ingest_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
HOST = os.path.join(ROOT, "nextsearch-api_amd", "host")
HARNESS = os.path.join(ROOT, "tests", "ingest_text_harness.cpp")
JOIN_LENGTHS = (1025, 1279, 1280, 1281, 65536, 70001)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ingest_text") / "ingest_text_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I" + CSRC, "-I" + HOST, "-o", so, HARNESS], check=True)
    lib = C.CDLL(so)
    for f in (lib.ig_alnum_c, lib.host_alnum_c):
        f.argtypes, f.restype = [C.c_uint32], C.c_int
    lib.stop_words_c.argtypes, lib.stop_words_c.restype = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p], None
    for f in (lib.ig_hash_bytes_c, lib.ig_hash_chunked_c):
        f.argtypes, f.restype = [C.c_char_p, C.c_uint32], C.c_uint64
    lib.ig_const_c.argtypes, lib.ig_const_c.restype = [C.c_int], C.c_uint64
    lib.ig_table_slots_c.argtypes, lib.ig_table_slots_c.restype = [C.c_uint64], C.c_uint64
    return lib


def test_the_byte_class_for_all_256_bytes(harness):
    alnum = [c for c in range(256) if harness.ig_alnum_c(c)]
    assert len(alnum) == 62 and bytes(alnum) == S.ALNUM
    for c in range(256):
        want = ingest_ref._TOKEN.fullmatch(bytes([c])) is not None
        assert bool(harness.ig_alnum_c(c)) == bool(harness.host_alnum_c(c)) == want == S.IS_ALNUM[c], c
    # the kernel hands ig_alnum a byte; a wider value is never alnum either way (the subtraction wraps)
    assert not any(harness.ig_alnum_c(c) for c in (0x100 + ord("a"), 0xFFFFFFFF, 0x130))


def test_the_stop_rule_for_every_word_of_2_3_and_4_bytes(harness):
    alphabet = S.LOWER + S.DIGITS
    assert len(alphabet) == 36 and set(S.STOP) == set(ingest_ref.STOP_WORDS) and len(S.STOP2) == 23
    seen = 0
    for length in (2, 3, 4):
        total = 36 ** length
        ig, host = np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=np.uint8)
        harness.stop_words_c(alphabet, 36, length, ig.ctypes.data, host.ctypes.data)
        want = sorted(sum(alphabet.index(c) * 36 ** j for j, c in enumerate(w)) for w in ingest_ref.STOP_WORDS - {b"a"} if len(w) == length)
        assert np.flatnonzero(ig).tolist() == want, length
        assert np.array_equal(ig, host), length            # the query side and the index side drop the same words
        seen += len(want)
    assert seen == 23
    # a word of upper-case bytes is no stop word to ig_stop: k_ig_keep runs after the text is lower-cased
    ig, host = np.zeros(26 ** 3, dtype=np.uint8), np.zeros(26 ** 3, dtype=np.uint8)
    harness.stop_words_c(S.UPPER, 26, 3, ig.ctypes.data, host.ctypes.data)
    assert not ig.any() and not host.any()


def test_the_joined_chunk_hashes_equal_the_sequential_hash(harness):
    rng = np.random.default_rng(5)
    for length in JOIN_LENGTHS + (1, 255, 256, 257, 1024, 65535, 65537):
        for b in (bytes(rng.integers(0, 256, length, dtype=np.uint8)), b"\xff" * length, S.long_tokens(length)[0]):
            assert harness.ig_hash_chunked_c(b, length) == harness.ig_hash_bytes_c(b, length), length


def test_the_restated_hash_and_constants_are_the_headers(harness):
    assert (S.TILE, S.LONG, S.P, S.MIN_TABLE) == (harness.ig_const_c(0), harness.ig_const_c(1), harness.ig_const_c(3), harness.ig_const_c(4))
    assert harness.ig_const_c(2) == 0xFFFFFFFF and S.TILE == S.THREAD * S.CHUNKS
    # the table of the build and of the merge (csrc/ns_api.hip sizes both with ig_table_slots)
    assert [S.table_slots(k) for k in (0, 1, 512, 513, 1024, 1025)] == [1024, 1024, 1024, 2048, 2048, 4096]
    for k in list(range(0, 3000)) + [(1 << b) + d for b in range(11, 31) for d in (-1, 0, 1)] + [(1 << 31) - 1]:
        assert harness.ig_table_slots_c(k) == S.table_slots(k), k
    n = 0
    for c in S.all_cases():
        o = S.oracle(c)
        for t in o["terms"]:
            h = harness.ig_hash_bytes_c(t, len(t))
            assert S.term_hash(t) == h and S.home_slot(t, o["kept_tokens"]) == h & (S.table_slots(o["kept_tokens"]) - 1), (c.name, t[:20])
            n += 1
    assert n > 3000
    assert S.mix(0) == 0 and S.term_hash(b"") == 0


def test_the_wrap_words_have_the_home_slots_they_are_picked_for():
    o = S.oracle(S.case_by_name("wrap"))
    assert o["kept_tokens"] <= 512
    assert [S.home_slot(S.word(i), o["kept_tokens"]) for i in S.WRAP_LAST] == [1023] * 4
    assert [S.home_slot(S.word(i), o["kept_tokens"]) for i in S.WRAP_BEFORE] == [1022] * 3
    special = {S.word(i) for i in S.WRAP_LAST + S.WRAP_BEFORE}
    assert special <= set(o["terms"])
    raw = {S.case_by_name("wrap").blob[s:e] for s, e, _ in o["kept"]}
    assert all(w in raw and w.upper() in raw for w in special)                       # repeated in other letter case
    first = [t for t in o["terms"] if t in special or t.startswith(b"filler")][:14]
    assert [t in special for t in first] == [False, True] * 7                        # interleaved with other terms


def test_the_case_table_reaches_every_flag_and_the_oracle_holds():
    cases = S.all_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) and {c.group for c in cases} == set(S.GROUPS)
    assert sum(len(S.cases_of(g)) for g in S.GROUPS) == len(cases)
    reached = {}
    for c in cases:
        n_docs = len(c.offs) - 1
        assert isinstance(c.blob, bytes) and len(c.blob) <= 1 << 20 and c.offs.dtype == np.uint64, c.name
        assert n_docs >= 1 and c.offs[0] == 0 and int(c.offs[-1]) == len(c.blob) and np.all(np.diff(c.offs.astype(np.int64)) >= 0), c.name
        texts = S.texts_of(c)
        o, want = S.oracle(c), ingest_ref.build(texts)
        for k in ("kept_docs", "doc_len", "counts", "pairs"):
            assert o[k].dtype == want[k].dtype and np.array_equal(o[k], want[k]), (c.name, k)
        assert o["terms"] == want["terms"], c.name
        assert o["n_tokens"] == sum(len(ingest_ref.tokenize(t)) for t in texts) and o["kept_tokens"] == int(want["doc_len"].sum()), c.name
        flags = S.reach(c)
        assert flags <= set(S.FLAGS), c.name
        for flag in flags:
            reached.setdefault(flag, []).append(c.name)
        print(c.name, c.group, len(c.blob), n_docs, o["n_tokens"], o["kept_tokens"], len(o["terms"]), sorted(flags))
    assert sorted(reached) == sorted(S.FLAGS), sorted(set(S.FLAGS) - set(reached))
    assert len(S.FLAGS) == len(set(S.FLAGS)) == 28
    # the cases built for a flag reach it themselves
    assert set(S.NAMED) <= set(names)
    for name, flags in S.NAMED.items():
        for flag in flags:
            assert name in reached[flag], (name, flag)
    assert {f for flags in S.NAMED.values() for f in flags} == set(S.FLAGS)


def by_name(name):
    c = S.case_by_name(name)
    return c, S.oracle(c)


def test_the_sweep_puts_every_alignment_and_length_where_it_says():
    c, o = by_name("sweep")
    toks = o["tokens"]
    assert len(toks) == 32 * 34 and len({(s % 32, e - s) for s, e, _ in toks}) == 32 * 34
    assert {(s % 32, e - s) for s, e, _ in toks} == {(a, ln) for a in range(32) for ln in range(1, 35)}
    assert {(s % 16, e % 16) for s, e, _ in toks} == {(a, b) for a in range(16) for b in range(16)}
    for k, (s, e, _) in enumerate(toks):
        assert s == k * S.SWEEP_SLOT + k // 34 and e - s == k % 34 + 1                # absolute offsets
    c, o = by_name("sweep_tight")
    assert {s % 16 for s, _, _ in o["tokens"]} == {e % 16 for _, e, _ in o["tokens"]} == set(range(16))
    assert all(not S.IS_ALNUM[c.blob[e]] and S.IS_ALNUM[c.blob[e + 1]] for _, e, _ in o["tokens"][:-1])   # one separator byte


def test_the_text_lengths_and_the_tile_cases():
    for n in S.TEXT_LENGTHS:
        c, o = by_name("len_%d" % n)
        assert len(c.blob) == n and o["tokens"][-1][1] == n and c.blob[-min(n, 2):] == b"Qz"[-min(n, 2):]
    c, o = by_name("tile_straddle")
    spans = [(s, e) for s, e, _ in o["tokens"]]
    assert (S.TILE - 6, S.TILE + 1) in spans and (2 * S.TILE - 1, 2 * S.TILE + 7) in spans and (3 * S.TILE - 4, 3 * S.TILE) in spans
    c, o = by_name("dense_docs")
    assert len(c.offs) - 1 == 4097 and o["n_tokens"] == 4097 and o["kept_docs"].tolist() == [4096] and o["terms"] == [b"zz"]
    assert all(e - s == 1 for s, e, _ in o["tokens"][:4096])
    c, o = by_name("dense_nodocs")
    assert o["n_tokens"] == 4097 and [sum(1 for s, _, _ in o["tokens"] if s // S.TILE == t) for t in (0, 1)] == [2048, 2048]
    c, o = by_name("all_bytes")
    assert np.bincount(o["counts"]).tolist() == [0, 62, 194] and len(o["kept_docs"]) == 256


def test_the_document_splits_sit_where_they_say():
    c, o = by_name("docsplit")
    splits = S.splits_inside_runs(c)
    assert {s % 32 for s in splits} >= set(S.DOCSPLIT_RESIDUES) and S.TILE in splits
    assert sorted(splits.values()).count(2) == 3 and sorted(splits.values()).count(3) == 2
    assert all(c.blob[s - 1:s + 1].isalnum() for s in splits)
    assert o["n_tokens"] == 2 * len(splits) + 1                                      # every split makes two tokens of one run
    c, o = by_name("two_byte_docs")
    assert c.offs.tolist() == list(range(0, len(c.blob) + 1, 2)) and o["terms"] == [b"ab", b"cd"] and len(o["kept_docs"]) == len(c.offs) - 1
    c, o = by_name("stop_split")
    got = [(S.lower(c.blob[s:e]), (s, e, d) in o["kept"]) for s, e, d in o["tokens"]]
    assert got[:4] == [(b"th", True), (b"e", False), (b"wi", True), (b"th", True)] and got[4:6] == [(b"an", False), (b"d", False)]
    c, o = by_name("lowercase")
    ups = {i % 16 for i, b in enumerate(c.blob) if 65 <= b <= 90}
    assert ups == set(range(16))
    for i in range(16):
        at = 64 * i + 16 + i
        assert c.blob[at - 1] in S.NEXT_TO_ALNUM and c.blob[at + 2] in S.NEXT_TO_ALNUM and at % 16 == i
    assert {c.blob[64 * i + 16 + i - 1] for i in range(16)} | {c.blob[64 * i + 16 + i + 2] for i in range(16)} == set(S.NEXT_TO_ALNUM)


def test_the_keep_cases_hold_the_forms_they_say():
    c, o = by_name("stop_forms")
    raw = {c.blob[s:e] for s, e, _ in o["tokens"]}
    kept = {c.blob[s:e] for s, e, _ in o["kept"]}
    for w in S.STOP:
        assert {w, w.upper(), S.mixed(w), w + b"x", w + b"1", b"x" + w} <= raw and (len(w) == 1 or w[:-1] in raw), w
        assert not {w, w.upper(), S.mixed(w)} & kept, w
    assert {b"anda", b"ana", b"wit", b"witx", b"th", b"bee", b"fro"} <= kept and not {b"an", b"and", b"with"} & kept
    c, o = by_name("stop_first_last")
    assert c.blob.startswith(b"the ") and c.blob.endswith(b" with") and o["terms"] == [b"quick", b"fox", b"jumps"]
    assert by_name("stop_only")[1]["kept_tokens"] == 0
    c, o = by_name("stop_across_edges")
    stops = [(s, e) for s, e, _ in o["tokens"] if S.lower(c.blob[s:e]) in S.STOP]
    assert len(stops) == 6 and o["kept_tokens"] == 6
    assert sorted(16 - s % 16 for s, _ in stops) == [1, 1, 2, 2, 3, 3] and sum(1 for s, e in stops if s // S.TILE != (e - 1) // S.TILE) == 3
    c, o = by_name("one_byte_tokens")
    assert sorted(c.blob[s:e] for s, e, _ in o["tokens"] if e - s == 1) == sorted(bytes([b]) for b in S.ALNUM) and o["terms"] == [b"ok"]


def test_the_long_and_dict_cases_and_their_halves():
    for n in S.LONG_LENGTHS:
        c, o = by_name("long_%d" % n)
        t, sib = S.long_tokens(n)
        assert len(t) == n and o["terms"] == [b"head", S.lower(t)] + [S.lower(x) for x in sib] and len(set(o["terms"])) == 5
        assert o["tf_total"][1] == 3 and o["pairs"].tolist()[1] == [1, 2]               # tf 2 in document 0
        # both sources of the compaction test hold the term
        parts = [ingest_ref.build(h) for h in S.halves(c)]
        assert all(S.lower(t) in p["terms"] for p in parts)
    assert [n for n in S.LONG_LENGTHS if S.chunk_tail_empty(n)] == [1025, 1281]
    special = {S.word(i) for i in S.WRAP_LAST + S.WRAP_BEFORE}
    parts = [ingest_ref.build(h) for h in S.halves(S.case_by_name("wrap"))]
    assert all(special <= set(p["terms"]) for p in parts) and sum(len(p["terms"]) for p in parts) <= 512
    # every dict and long case stays at or below 600 distinct terms: the narrowed-hash run probes quadratically
    for c in S.cases_of("dict") + S.cases_of("long"):
        assert len(S.oracle(c)["terms"]) <= 600 and len(c.offs) - 1 >= 2, c.name
        merged = compact_ref.merge([ingest_ref.build(h) for h in S.halves(c)])
        assert sorted(merged["terms"]) == sorted(S.oracle(c)["terms"]), c.name
    assert len(by_name("load_512")[1]["terms"]) == 512 == by_name("load_512")[1]["kept_tokens"]
    assert len(by_name("load_513")[1]["terms"]) == 513 == by_name("load_513")[1]["kept_tokens"]
    c, o = by_name("first_occurrence")
    assert o["kept_docs"].tolist() == [1, 3, 4] and o["terms"] == [b"zebra", b"apple", b"mango", b"kiwi"]
    c, o = by_name("same_bytes")
    assert o["terms"] == [b"alpha", b"beta", b"gamma", b"delta"] and o["kept_docs"].tolist() == [0, 1, 3, 4, 5]


def test_the_docs_cases():
    assert [len(S.case_by_name("ndocs_%d" % n).offs) - 1 for n in S.N_DOCS] == [1, 2, 3, 255, 256, 257]
    c, o = by_name("empty_docs")
    lens = np.diff(c.offs.astype(np.int64))
    runs, run = [], 0
    for ln in lens.tolist() + [1]:
        if ln == 0:
            run += 1
        elif run:
            runs.append(run)
            run = 0
    assert runs == [1, 1, 2, 300, 1] and lens[0] == 0 and lens[-1] == 0 and int(c.offs[-2]) == len(c.blob)
    assert o["kept_docs"].tolist() == [1, 3, 6, 8, 12, 313, 315]
    c, o = by_name("empty_mostly")
    assert o["kept_docs"].tolist() == [300]


def test_the_harness_program_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "ingest_text_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DINGEST_TEXT_MAIN",
                    "-I" + CSRC, "-I" + HOST, "-o", exe, HARNESS], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("lengths, 0 wrong")
