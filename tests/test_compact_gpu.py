"""Compaction on the device (csrc/ns_compact.hip behind ns_forward_merge, ns_forward_invert, nsx::merge_segments,
Engine::compact).  The oracle is exact: with this project's term-id rule, merging the segments of batches
D1 .. Dn gives byte for byte the segment ONE add_documents(D1 + .. + Dn) writes (tests/test_compact_cpu.py checks that
claim on the CPU).  Everything here is integers and bytes: every comparison is exact."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np
import pytest

import compact_ref
import ingest_ref
import nsbind
from conftest import sha256_tree
from test_ingest_gpu import GOLDEN, as_docs, gen_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import invert_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
NS_E_INVAL, NS_E_STATE = -1, -5


# ---- helpers ------------------------------------------------------------------------------------
def new_engine(index, batches, device=0):
    """a fresh index directory fed with one add_documents per batch"""
    os.makedirs(index)
    eng = nsbind.Engine.create(index, device)
    for b in batches:
        eng.add_documents(b)
    return eng


def manifest_names(index):
    with open(os.path.join(index, "manifest.bin"), "rb") as f:
        b = f.read()
    (n,) = struct.unpack_from("<I", b, 0)
    pos, out = 4, []
    for _ in range(n):
        (ln,) = struct.unpack_from("<I", b, pos)
        out.append(b[pos + 4:pos + 4 + ln].decode())
        pos += 4 + ln
    return out


def write_manifest(index, names):
    with open(os.path.join(index, "manifest.bin"), "wb") as f:
        f.write(struct.pack("<I", len(names)) + b"".join(struct.pack("<I", len(n)) + n.encode() for n in names))


def seg_dir(index, name):
    return os.path.join(index, "segments", name)


def rows(eng, queries, k, flags):
    hits, nhits, found, usable = eng.search_batch(queries, k, flags)
    return hits, nhits, found, usable.astype(bool)


def assert_same_rows(a, b, what):
    """doc, segment, score bits, nhits, found, usable of every query equal"""
    (ha, na, fa, ua), (hb, nb, fb, ub) = a, b
    assert np.array_equal(ua, ub), what
    assert np.array_equal(na[ua], nb[ua]) and np.array_equal(fa[ua], fb[ua]), what
    live = (np.arange(ha.shape[1])[None, :] < na[:, None]) & ua[:, None]
    for f in ("doc", "seg"):
        assert np.array_equal(ha[f][live], hb[f][live]), (what, f)
    assert np.array_equal(ha["score"].view(np.uint32)[live], hb["score"].view(np.uint32)[live]), (what, "score bits")
    return int(live.sum())


def make_queries(terms, n, seed):
    """n queries of 1 .. 4 words: frequent terms (early ids), rare ones, stop words and words no document holds"""
    rng = np.random.default_rng(seed)
    pool = [t.decode() for t in terms if len(t) <= 16]
    out = []
    for i in range(n):
        m = int(rng.integers(1, 5))
        ws = []
        for _ in range(m):
            r = rng.random()
            if r < 0.5:
                ws.append(pool[int(min(len(pool) - 1, rng.zipf(1.3) - 1))])
            elif r < 0.9:
                ws.append(pool[int(rng.integers(0, len(pool)))])
            elif r < 0.95:
                ws.append("the")
            else:
                ws.append("zzqx%d" % i)
        out.append(" ".join(ws))
    return out


def assert_same_searches(eng_a, eng_b, terms, n_queries, seed, what):
    queries = make_queries(terms, n_queries, seed)
    live = 0
    for k in (10, 100):
        for flags in (nsbind.NS_FLAG_OR, nsbind.NS_FLAG_AND):
            live += assert_same_rows(rows(eng_a, queries, k, flags), rows(eng_b, queries, k, flags), (what, k, flags))
    assert live > n_queries                                            # the comparison is not vacuous
    prefixes = sorted({t[:n] for t in terms[:4000] for n in (1, 2, 3) if len(t) <= 16})[:600] + [b"zzqx", b"Quo"]
    assert eng_a.suggest_batch(prefixes, 10) == eng_b.suggest_batch(prefixes, 10), what


def assert_forward_equal(got, want, what):
    assert got["terms"] == want["terms"], what
    for k in ("doc_len", "counts", "pairs"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(got["kept_docs"], np.arange(len(want["doc_len"]), dtype=np.uint32)), what


@pytest.fixture()
def ctx():
    L = nsbind.hip_lib()
    h = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(h)) == 0
    yield h
    L.ns_ctx_destroy(h)


# ---- 1 + 3: the one-shot oracle, and searches over both ------------------------------------------
BIG_SIZES = (3000, 1, 2500, 4000)                                      # five uneven batches, one a single document


def big_corpus():
    texts = gen_corpus(3100, 10400, 380, vocab=30000, long_tokens=(70001, 90000))
    # the tokens of more than 70 000 bytes occur in a second part as well (in the last batch, in another letter case)
    longs = [t for t in ingest_ref.tokenize(texts[3]) + ingest_ref.tokenize(texts[10]) if len(t) > 70000]
    assert len(longs) >= 4
    texts[10000] = texts[10000] + b" " + longs[0].upper() + b"," + longs[-1]
    return texts


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("compact_big")
    texts = big_corpus()
    docs = as_docs(texts)
    batches = compact_ref.cut(docs, BIG_SIZES)
    assert len(batches) == 5 and sorted(len(b) for b in batches)[0] == 1
    a, b = str(tmp / "parts"), str(tmp / "oneshot")
    eng_a, eng_b = new_engine(a, batches), new_engine(b, [docs])
    assert eng_a.num_segments == 5 and eng_b.num_segments == 1
    st = eng_a.compact()
    print("compact:", st)
    yield {"a": a, "b": b, "eng_a": eng_a, "eng_b": eng_b, "texts": texts, "docs": docs, "stats": st}
    eng_a.close()
    eng_b.close()


def test_compacted_segment_equals_the_one_shot_segment_byte_for_byte(big):
    fwd = ingest_ref.build(big["texts"])
    assert len(fwd["kept_docs"]) >= 10000 and len(fwd["pairs"]) >= 1_000_000   # every kernel runs more than one tile
    assert max(len(t) for t in fwd["terms"]) > 70000
    st = big["stats"]
    assert st["sources"] == 5 and st["n_docs"] == len(fwd["kept_docs"]) and st["n_terms"] == len(fwd["terms"]) and st["pairs"] == len(fwd["pairs"])
    assert st["terms_in"] > st["n_terms"]
    names = manifest_names(big["a"])
    assert names == ["seg_000005"] and big["eng_a"].num_segments == 1
    assert sorted(os.listdir(os.path.join(big["a"], "segments"))) == names       # remove_sources: the five sources are gone
    got, want = compact_ref.read_tree(seg_dir(big["a"], names[0])), compact_ref.read_tree(seg_dir(big["b"], "seg_000000"))
    assert sorted(got) == sorted(want) and len(got) == 4 + 1 + 128
    for fn in sorted(want):
        assert len(got[fn]) == len(want[fn]) and got[fn] == want[fn], fn
    files = ingest_ref.file_bytes(big["docs"], fwd)
    for fn in ingest_ref.FILES:
        assert got[fn] == files[fn], fn


def test_searches_over_the_compacted_index_equal_the_one_shot_index(big):
    fwd_terms = invert_oracle.read_terms(os.path.join(seg_dir(big["b"], "seg_000000"), "terms.bin"))
    assert_same_searches(big["eng_a"], big["eng_b"], fwd_terms, 3000, 7, "big")


def test_reference_parity_after_two_halves_and_a_compaction(tmp_path):
    with open(GOLDEN) as f:
        g = json.load(f)
    docs = g["documents"]
    eng = new_engine(str(tmp_path / "index"), [docs[:len(docs) // 2], docs[len(docs) // 2:]])
    try:
        assert eng.num_segments == 2
        eng.compact()
        assert eng.num_segments == 1
        hits, nhits, found, usable = eng.search_batch([q["query"] for q in g["queries"]], g["k"], 0)
        for i, q in enumerate(g["queries"]):
            n = int(nhits[i])
            got = [[int(h["seg"]), int(h["doc"]), int(np.asarray(h["score"]).view(np.uint32))] for h in hits[i, :n]]
            assert (int(found[i]) if usable[i] else -1) == q["found"] and got == q["hits"], q["query"]   # the REAL reference's answers
    finally:
        eng.close()


# ---- 2: every size class of the sort inside a document ---------------------------------------------
def size_class_batches(cut):
    """source 0: one document that introduces 120 000 words in order; source 1: documents of 1, 2, 63, 64, 65, cut - 1, cut,
    cut + 1 and 100 003 distinct words, each document's words a range of its own in random order (the first two descending),
    so that the first-occurrence order inside source 1 is not the merged one"""
    rng = np.random.default_rng(5)
    sizes = [1, 2, 63, 64, 65, cut - 1, cut, cut + 1, 100_003]
    words = [b"w%06d" % i for i in range(sum(sizes) + 1000)]
    src1, at = [], 500
    for n in sizes:
        pick = at + rng.permutation(n)
        if n >= 2 and pick[0] < pick[1]:
            pick[[0, 1]] = pick[[1, 0]]
        at += n
        src1.append(b" ".join(words[int(i)] + (b" " + words[int(i)]) * int(i % 3 == 0) for i in pick))
    return [[b"Start " + b" ".join(words)], src1], sizes


def test_every_size_class_of_the_document_sort(tmp_path, ctx):
    L = nsbind.hip_lib()
    cut = int(L.ns_compact_doc_cut())
    assert 64 < cut < 100_000
    batches, sizes = size_class_batches(cut)
    parts = [ingest_ref.build(b) for b in batches]
    assert list(parts[1]["counts"]) == sizes and int(parts[0]["counts"][0]) > 100_000
    changed = compact_ref.docs_whose_order_changes(parts)
    assert changed == [0, len(sizes) - 1]                              # every later document of two or more terms really changes
    want = compact_ref.merge(parts)
    one = ingest_ref.build(batches[0] + batches[1])
    assert_forward_equal(want, one, "oracle")
    assert_forward_equal(nsbind.forward_merge(ctx, parts), want, "in place")
    assert L.ns_ctx_use_docsort(ctx, 0) == 0                           # the four-pass radix sort for every document: same bytes
    assert_forward_equal(nsbind.forward_merge(ctx, parts), want, "radix")
    assert L.ns_ctx_use_docsort(ctx, 1) == 0
    # and through the files
    a, b = str(tmp_path / "parts"), str(tmp_path / "oneshot")
    docs = as_docs(batches[0] + batches[1])
    eng_a, eng_b = new_engine(a, [docs[:len(batches[0])], docs[len(batches[0]):]]), new_engine(b, [docs])
    try:
        eng_a.compact()
        name = manifest_names(a)[0]
        assert compact_ref.read_tree(seg_dir(a, name)) == compact_ref.read_tree(seg_dir(b, "seg_000000"))
    finally:
        eng_a.close()
        eng_b.close()


# ---- 4: sources with another term numbering ---------------------------------------------------------
def test_permuted_sources(tmp_path):
    texts = gen_corpus(41, 1500, 90, vocab=3000, long_tokens=(70001,))
    docs = as_docs(texts)
    sizes = (400, 1, 600)
    part_docs = compact_ref.cut(docs, sizes)
    parts = [ingest_ref.build([d[3] for d in pd]) for pd in part_docs]
    sources = [compact_ref.permute(p, 50 + i) if i != 1 else p for i, p in enumerate(parts)]
    index = str(tmp_path / "index")
    segs = []
    for i, (pd, s) in enumerate(zip(part_docs, sources)):
        segs.append(seg_dir(index, "seg_%06u" % i))
        compact_ref.write_forward_files(segs[-1], pd, s)                # (a merge reads a source's four forward files only)
    out = seg_dir(str(tmp_path / "merged"), "seg_000000")
    st = nsbind.merge_segments(segs, out)
    want = compact_ref.merge(sources)                                   # the stated term walk over the permuted lists
    assert st["n_terms"] == len(want["terms"]) and st["pairs"] == len(want["pairs"])
    files = compact_ref.merged_file_bytes(part_docs, sources, want)
    got = compact_ref.read_tree(out)
    for fn in ingest_ref.FILES:
        assert got[fn] == files[fn], fn
    oracle_dir = str(tmp_path / "oracle_seg")
    compact_ref.write_forward_files(oracle_dir, [d for pd, s in zip(part_docs, sources) for d in compact_ref.kept_documents(pd, s)], want)
    invert_oracle.lexicon_tool(oracle_dir)
    assert got == compact_ref.read_tree(oracle_dir)
    # the numbering is not what a search reads: same answers as the one-shot index
    write_manifest(str(tmp_path / "merged"), ["seg_000000"])
    eng_a, eng_b = nsbind.Engine(str(tmp_path / "merged"), 0), new_engine(str(tmp_path / "oneshot"), [docs])
    try:
        assert_same_searches(eng_a, eng_b, ingest_ref.build(texts)["terms"], 1500, 9, "permuted")
    finally:
        eng_a.close()
        eng_b.close()


# ---- 5: a range ---------------------------------------------------------------------------------------
def test_compacting_a_range_of_the_manifest(tmp_path):
    texts = gen_corpus(61, 1000, 70, vocab=2000, long_tokens=())
    d = compact_ref.cut(as_docs(texts), (150, 300, 1, 350))
    assert len(d) == 5
    a, b = str(tmp_path / "five"), str(tmp_path / "three")
    eng_a, eng_b = new_engine(a, d), new_engine(b, [d[0], d[1] + d[2] + d[3], d[4]])
    try:
        st = eng_a.compact(1, 3)
        assert st["sources"] == 3 and manifest_names(a) == ["seg_000000", "seg_000005", "seg_000004"]
        assert [eng_a.segment_name(i) for i in range(eng_a.num_segments)] == ["seg_000000", "seg_000005", "seg_000004"]
        assert sorted(os.listdir(os.path.join(a, "segments"))) == ["seg_000000", "seg_000004", "seg_000005"]
        assert compact_ref.read_tree(seg_dir(a, "seg_000005")) == compact_ref.read_tree(seg_dir(b, "seg_000001"))
        assert_same_searches(eng_a, eng_b, ingest_ref.build(texts)["terms"], 1500, 3, "range")   # segment positions in the hits included
        # ranges that hold fewer than two segments: success, nothing touched
        before = sha256_tree(a)
        for first, count in ((0, 1), (2, 5), (7, 3), (1, 0)):
            eng_a.compact(first, count)
        assert sha256_tree(a) == before and eng_a.num_segments == 3
    finally:
        eng_a.close()
        eng_b.close()


# ---- 6: failures leave everything alone ----------------------------------------------------------------
def test_refused_sources_leave_the_index_and_the_engine_alone(tmp_path):
    """Every case is a refused INPUT: found on the host while the files are read, or by a flag word the kernels set next to
    their bounds checks.  Nothing here can fault the device."""
    texts = gen_corpus(71, 600, 60, vocab=1500, long_tokens=())
    index = str(tmp_path / "index")
    eng = new_engine(index, compact_ref.cut(as_docs(texts), (200, 200)))
    try:
        queries = make_queries(ingest_ref.build(texts)["terms"], 300, 1)
        want = rows(eng, queries, 10, 0)
        victim = seg_dir(index, "seg_000001")
        fwd_path, terms_path = os.path.join(victim, "forward.bin"), os.path.join(victim, "terms.bin")
        fwd_bytes, terms_bytes = open(fwd_path, "rb").read(), open(terms_path, "rb").read()
        terms = invert_oracle.read_terms(terms_path)
        twice = [terms[0]] + [terms[0]] + terms[2:]
        bad_pair = bytearray(fwd_bytes)
        assert struct.unpack_from("<I", bad_pair, 4)[0] >= 1           # the first document has a pair
        struct.pack_into("<I", bad_pair, 8, len(terms))                # termId == n_terms
        cases = [
            ("truncated forward.bin", fwd_path, fwd_bytes[:len(fwd_bytes) // 2], r"seg_000001.forward\.bin: truncated"),
            ("missing terms.bin", terms_path, None, r"seg_000001.terms\.bin: missing"),
            ("termId >= n_terms", fwd_path, bytes(bad_pair), r"source 1: a pair's termId.*seg_000001"),
            ("a term twice", terms_path, struct.pack("<I", len(twice)) + b"".join(ingest_ref._s(t) for t in twice), r"source 1: one byte string occurs twice.*seg_000001"),
        ]
        for what, path, content, message in cases:
            if content is None:
                os.remove(path)
            else:
                with open(path, "wb") as f:
                    f.write(content)
            before = sha256_tree(index)
            with pytest.raises(RuntimeError, match=message):
                eng.compact()
            assert sha256_tree(index) == before, what
            assert eng.num_segments == 3 and manifest_names(index) == ["seg_000000", "seg_000001", "seg_000002"], what
            assert_same_rows(rows(eng, queries, 10, 0), want, what)
            with open(fwd_path, "wb") as f:
                f.write(fwd_bytes)
            with open(terms_path, "wb") as f:
                f.write(terms_bytes)
        eng.compact()                                                   # with the files restored it goes through
        assert eng.num_segments == 1
    finally:
        eng.close()


# ---- 7: sources kept or removed, the cache, determinism, several device contexts ---------------------------
def test_kept_sources_cache_determinism_and_a_multi_device_engine(tmp_path):
    texts = gen_corpus(81, 900, 60, vocab=1500, long_tokens=())
    batches = compact_ref.cut(as_docs(texts), (300, 1, 400))
    terms = ingest_ref.build(texts)["terms"]
    index = str(tmp_path / "index")
    eng = new_engine(index, batches)
    try:
        word = terms[0].decode()
        eng.set_cache(True)
        body_before = eng.search_json(word, 10)
        assert '"from_cache": true' in eng.search_json(word, 10) and '"from_cache"' not in body_before and eng.cache_size() >= 1
        sources = [seg_dir(index, n) for n in manifest_names(index)]
        kept = {s: compact_ref.read_tree(s) for s in sources}
        eng.compact(remove_sources=False)
        assert eng.error() == "" and manifest_names(index) == ["seg_000004"]
        assert {s: compact_ref.read_tree(s) for s in sources} == kept   # the sources are still there, byte for byte
        body_after = eng.search_json(word, 10)
        fresh = nsbind.Engine(index, 0)
        try:
            # no pre-compaction body is served: the first answer after the call is computed, over the new index
            assert '"from_cache"' not in body_after and body_after == fresh.search_json(word, 10) and body_after != body_before
        finally:
            fresh.close()
        # the same sources merged twice more: identical bytes
        m1, m2 = str(tmp_path / "m1"), str(tmp_path / "m2")
        nsbind.merge_segments(sources, m1)
        nsbind.merge_segments(sources, m2)
        first = compact_ref.read_tree(seg_dir(index, "seg_000004"))
        assert compact_ref.read_tree(m1) == first and compact_ref.read_tree(m2) == first
    finally:
        eng.close()
    # a two-context engine compacts (the reload replicates) and answers like a one-context engine on the result
    index2 = str(tmp_path / "index2")
    new_engine(index2, batches).close()
    multi = nsbind.Engine(index2, [0, 0])
    try:
        assert multi.num_devices == 2 and multi.num_segments == 4
        multi.compact()
        assert multi.num_segments == 1 and sorted(os.listdir(os.path.join(index2, "segments"))) == ["seg_000004"]
        single = nsbind.Engine(index2, 0)
        try:
            queries = make_queries(terms, 1000, 5)
            for k, flags in ((10, 0), (100, 1)):
                assert_same_rows(rows(multi, queries, k, flags), rows(single, queries, k, flags), ("multi", k, flags))
        finally:
            single.close()
    finally:
        multi.close()
    assert compact_ref.read_tree(seg_dir(index2, "seg_000004")) == first


# ---- 8: the raw ABI ---------------------------------------------------------------------------------------------
def test_raw_c_abi_codes_limits_and_handle_lifetime():
    L = nsbind.hip_lib()
    ctx = C.c_void_p()
    assert L.ns_ctx_create(0, C.byref(ctx)) == 0
    h = C.c_void_p()
    info = nsbind.NsForwardInfo(struct_size=C.sizeof(nsbind.NsForwardInfo))
    part = ingest_ref.build([b"Alpha beta alpha. The gamma", b"", b"beta delta"])
    other = ingest_ref.build([b"delta alpha epsilon", b"gamma gamma"])
    # NULL arguments
    arr, keep = nsbind.forward_sources([part])
    assert L.ns_forward_merge(None, arr, 1, C.byref(h)) == NS_E_INVAL
    assert L.ns_forward_merge(ctx, arr, 1, None) == NS_E_INVAL
    assert L.ns_forward_merge(ctx, None, 1, C.byref(h)) == NS_E_INVAL and not h.value
    assert L.ns_forward_invert(None, None, None, None, None) == NS_E_INVAL
    # n_src == 0: an empty result
    assert L.ns_forward_merge(ctx, None, 0, C.byref(h)) == 0 and h.value
    assert L.ns_forward_get_info(h, C.byref(info)) == 0 and info.kept_docs == 0 and info.n_terms == 0 and info.n_pairs == 0
    assert L.ns_forward_fetch(h, None, None, None, None, None, None) == 0
    kept = C.c_uint64(77)
    assert L.ns_forward_invert(h, None, None, C.byref(kept), None) == 0 and kept.value == 0
    L.ns_forward_destroy(h)
    # one source that follows the project's rule comes back unchanged
    got = nsbind.forward_merge(ctx, [part], invert=True)
    assert_forward_equal(got, part, "one source")
    assert got["info"]["n_docs"] == got["info"]["kept_docs"] == 2 and got["info"]["n_tokens"] == got["info"]["kept_tokens"] == int(part["doc_len"].sum())
    df, post = invert_oracle.invert(part["counts"], part["pairs"], len(part["terms"]))
    assert np.array_equal(got["df"], df) and np.array_equal(got["postings"], post)
    # two sources against the restatement, inverted where they lie
    got = nsbind.forward_merge(ctx, [part, other], invert=True)
    want = compact_ref.merge([part, other])
    assert_forward_equal(got, want, "two sources")
    df, post = invert_oracle.invert(want["counts"], want["pairs"], len(want["terms"]))
    assert np.array_equal(got["df"], df) and np.array_equal(got["postings"], post)
    # refused inputs name the source
    def refused(parts, message, patch=None):
        arr, keep = nsbind.forward_sources(parts)
        if patch:
            patch(arr)
        assert L.ns_forward_merge(ctx, arr, len(parts), C.byref(h)) == NS_E_INVAL and not h.value
        assert message in L.ns_last_error(ctx), L.ns_last_error(ctx)

    bad = dict(other, pairs=np.array([[0, 1], [1, 1], [2, 1], [4, 2]], dtype=np.uint32))
    refused([part, bad], b"source 1: a pair's termId")
    refused([part, dict(other, terms=[b"delta", b"alpha", b"delta", b"gamma"])], b"source 1: one byte string occurs twice")
    refused([dict(part, terms=[b"alpha", b"alpha", b"gamma", b"delta"]), other], b"source 0: one byte string occurs twice")
    refused([part, dict(other, counts=np.array([3, 2], dtype=np.uint32))], b"source 1: the per-document counts")

    def decreasing(arr):
        to = np.array([0, 5, 3, 12, 17], dtype=np.uint64)
        keep.append(to)
        arr[1].term_offsets = to.ctypes.data
    refused([part, other], b"source 1: term offsets decrease", decreasing)
    # the limits, from the counts alone: no payload array of these sizes exists
    def huge_pairs(arr):
        arr[1].n_pairs = (1 << 32) - 4096
    refused([part, other], b"pairs", huge_pairs)

    def huge_docs(arr):
        arr[0].n_docs = 1 << 31
        arr[1].n_docs = (1 << 31) - 1
    refused([part, other], b"documents", huge_docs)

    def huge_terms(arr):
        arr[1].n_terms = 1 << 31
    refused([part, other], b"source terms", huge_terms)

    def huge_bytes(arr):
        to = np.array([0, 5, 9, 14, (1 << 32) - 65536], dtype=np.uint64)
        keep.append(to)
        arr[1].term_offsets = to.ctypes.data
    refused([part, other], b"term bytes", huge_bytes)
    # lifetime: fetched twice, destroyed once; orphaned, not dangling, when the ctx goes first
    arr, keep = nsbind.forward_sources([part, other])
    assert L.ns_forward_merge(ctx, arr, 2, C.byref(h)) == 0
    assert L.ns_forward_get_info(h, C.byref(info)) == 0 and info.kept_docs == 4
    L.ns_ctx_destroy(ctx)
    assert L.ns_forward_get_info(h, C.byref(info)) == 0 and info.kept_docs == 4
    assert L.ns_forward_fetch(h, None, None, None, None, None, None) == NS_E_STATE
    assert L.ns_forward_invert(h, None, None, C.byref(kept), None) == NS_E_STATE
    L.ns_forward_destroy(h)
