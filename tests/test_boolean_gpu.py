"""Boolean queries on the GPU (csrc/ns_boolean.hip, Engine::search_boolean_batch_flat, Engine::search_boolean).

1. The raw C-ABI against the restatement tests/boolean_ref.py on the directed inputs of tests/boolean_shapes.py: in this process
   on the product library (one window holds the 300-document families; a family of two product tiles + 5 documents hits the
   product's window and tile edges), and in ONE child process on the variants build with tiles of 128 and windows of 32
   documents.
2. Equivalence with the scoring path on the same raw inputs: all SHOULD == NS_FLAG_OR, all MUST == NS_FLAG_AND, NOT refs == the
   search over filtered copies that drop the excluded documents.
3. A child on the counting build asserts that the inputs reach every counted path of the two kernels.
4. Refusals.
5. The engine: `a b`, `+a +b`, `a b -c`, `+a b` against search_batch / search_filtered_batch, with and without a date filter;
   the JSON of search_boolean is search's with the "boolean" member; the ns_tool subcommand prints it.
Every comparison is exact."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import boolean_ref
import boolean_shapes
import nsbind
from boolean_ref import MUST, NOT, SHOULD
from conftest import PKG, VARIANTS_LIB
from rawseg import RawSegments, descriptors_multi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_LIB = os.path.join(PKG, "libnextsearch_hip_count.so")
NS_E_INVAL = -1
AND = nsbind.NS_FLAG_AND
# A child loads a library, creates a context and runs the small families: a few seconds of work, 60 s for a shared device.
CHILD_TIMEOUT_S = 60
IN_TEST_BUILD = os.path.basename(os.environ.get("NS_HIP_LIB", "")) not in ("", "libnextsearch_hip.so")


# ---- 1: the raw ABI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_segs", [1, 3])
def test_directed_role_mixes_equal_the_restatement(n_segs):
    """lists of 0 .. 257 postings, queries of 0, 1, 2, 3, 4, 8 and 70 refs per segment, every role mix, K = 1, 10, 63, 64, 65,
    100, with and without skip tables, roles == NULL (here: whatever tile and window the loaded library has)"""
    boolean_shapes.run_directed(n_segs)


def test_tied_scores_across_segments():
    boolean_shapes.run_tied()


def test_found_around_k():
    boolean_shapes.run_counts()


def test_two_product_tiles_and_five_documents():
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process: the family is built for the product's tile and window")
    tile, n = boolean_shapes.run_product_tile()
    assert tile == 1 << 17 and n == 262149


def child(lib, tmp_path):
    assert os.path.exists(lib), os.path.basename(lib) + " is missing: make -C nextsearch-api_amd all"
    out = str(tmp_path / "boolean.json")
    env = dict(os.environ, NS_HIP_LIB=lib, NS_FACET_TILE_DOCS=str(boolean_shapes.SMALL_TILE), NS_BOOL_WIN_DOCS=str(boolean_shapes.SMALL_WIN))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "boolean_shapes.py"), out], env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "boolean shapes OK" in r.stdout, tail
    with open(out) as f:
        return json.load(f)


def test_tiles_of_128_and_windows_of_32_documents_in_the_variants_build(tmp_path):
    """the same families where 300 documents are two whole tiles and a part, four windows each: every edge decides a tie"""
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process")
    rep = child(VARIANTS_LIB, tmp_path)
    assert rep["tile"] == boolean_shapes.SMALL_TILE and not rep["counting"]


# ---- 2: equivalence with the scoring path -------------------------------------------------------------------------------
def test_one_role_for_every_ref_is_the_scoring_path():
    covered = boolean_shapes.run_same_role_equals_the_scoring_path()
    assert covered[SHOULD] >= boolean_shapes.FLOOR_SAME_ROLE[SHOULD] and covered[MUST] >= boolean_shapes.FLOOR_SAME_ROLE[MUST], covered


def test_excluded_refs_are_the_search_over_filtered_copies():
    assert boolean_shapes.run_excluded_equals_the_search_over_filtered_copies() >= 2 * boolean_shapes.FLOOR_EXCLUDED


# ---- 3: the counting build ----------------------------------------------------------------------------------------------
def test_the_directed_inputs_reach_their_paths_in_the_counting_build(tmp_path):
    """every counter of ns_debug_boolean_counters was reached"""
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process")
    rep = child(COUNT_LIB, tmp_path)
    assert rep["tile"] == boolean_shapes.SMALL_TILE and rep["counting"]
    assert not rep["missed"], rep
    ev = rep["events"]
    for e in boolean_shapes.BOOLEAN_EVENTS:
        assert ev[e] > 0, (e, ev)
    assert ev["windows"] > ev["items"] > 0 and ev["windows"] > ev["windows_left_early"]


# ---- 4: refusals --------------------------------------------------------------------------------------------------------
def test_refusals():
    """each NS_E_INVAL with a message and nothing launched: the output arrays keep their fill"""
    L = nsbind.hip_lib()
    segments, queries = boolean_shapes.multi_family()
    segs = RawSegments(segments)
    other = RawSegments(segments[:1])
    try:
        ctx = segs.ctx
        one = [[1.0] * len(s[2]) for s in segments]
        qd, refs = descriptors_multi(queries, segs.lists, segs.offs, one, one)
        roles = (np.arange(len(refs)) % 3).astype(np.uint8)

        def refused(rc, match):
            assert rc == NS_E_INVAL, rc
            msg = L.ns_last_error(ctx).decode()
            assert match in msg, msg

        def run(qd=qd, refs=refs, roles=roles, ids=(0, 1, 2), hs=None):
            rc, hits, nhits, found, _ = nsbind.search_boolean_raw(ctx, qd, refs, roles, 10, list(ids), segs.segs if hs is None else hs)
            if rc != 0:
                assert np.all(hits.view(np.uint8) == 0xAB) and np.all(nhits == 0xABABABAB) and np.all(found == 0xABABABAB), "a refused call writes nothing"
            return rc

        assert run() == 0
        refused(run(ids=(0, 1), hs=segs.segs[:2]), "names segment 2, which the call does not list")
        refused(run(ids=(0, 1, 1)), "seg_id 1 is listed twice")
        past = refs.copy()
        past["byte_off"][0] = 8 * 10 ** 6
        refused(run(refs=past), "runs past the postings")
        odd = refs.copy()
        odd["byte_off"][0] += 4
        refused(run(refs=odd), "not a multiple of 8")
        over = qd.copy()
        over["term_count"][-1] = len(refs) + 1
        refused(run(qd=over), "run past the")
        bad = roles.copy()
        bad[3] = 3
        refused(run(roles=bad), "ref 3: role 3 is none of NS_ROLE_SHOULD, NS_ROLE_MUST, NS_ROLE_NOT")
        nan = refs.copy()
        nan["idf"][0] = np.nan
        refused(run(refs=nan, roles=np.zeros(len(refs), np.uint8)), "ref 0: idf or qweight is not finite")
        inf = refs.copy()
        inf["qweight"][1] = np.inf
        refused(run(refs=inf, roles=np.ones(len(refs), np.uint8)), "ref 1: idf or qweight is not finite")
        assert run(refs=nan, roles=np.full(len(refs), 2, np.uint8)) == 0            # under NOT the numbers are never read
        refused(run(hs=[other.segs[0], segs.segs[1], segs.segs[2]]), "segment 0 is not a published segment of this ctx")
        # null arguments, straight through ctypes
        K = 10
        hits = np.zeros((len(qd), K), nsbind.HIT_DTYPE)
        nh, fnd = np.zeros(len(qd), np.uint32), np.zeros(len(qd), np.uint64)
        sid = np.array([0, 1, 2], np.uint32)
        sa = (C.c_void_p * 3)(*[s.value for s in segs.segs])
        args = [ctx, qd.ctypes.data, len(qd), refs.ctypes.data, roles.ctypes.data, len(refs), K, sid.ctypes.data, sa, 3, hits.ctypes.data, nh.ctypes.data,
                fnd.ctypes.data, None]
        assert L.ns_search_boolean(*args) == 0                                   # device_ms_out may be NULL
        assert L.ns_search_boolean(*(args[:12] + [None, None])) == 0              # found_out too
        a = list(args)
        a[4] = None
        assert L.ns_search_boolean(*a) == 0                                      # roles == NULL: all SHOULD
        for at, match in ((1, "null argument"), (3, "null argument"), (10, "null argument"), (11, "null argument"),
                          (7, "null segment arrays"), (8, "null segment arrays")):
            a = list(args)
            a[at] = None
            refused(L.ns_search_boolean(*a), match)
        a = list(args)
        a[9] = 0
        refused(L.ns_search_boolean(*a), "no segment listed")
        a = list(args)
        a[8] = (C.c_void_p * 3)(segs.segs[0].value, None, segs.segs[2].value)
        refused(L.ns_search_boolean(*a), "segment 1 is NULL")
        assert L.ns_search_boolean(None, *args[1:]) == NS_E_INVAL
        # no queries: NS_OK, nothing touched, whatever else is passed
        assert L.ns_search_boolean(ctx, None, 0, None, None, 0, 10, None, None, 0, None, None, None, None) == 0
        out2 = (C.c_float * 2)()
        assert L.ns_boolean_kernel_ms(out2, 1) == 0 and out2[0] > 0.0 and out2[1] > 0.0
        assert L.ns_boolean_kernel_ms(out2, 0) == 0 and out2[0] == 0.0 and out2[1] == 0.0
        assert L.ns_boolean_kernel_ms(None, 0) == NS_E_INVAL
    finally:
        other.release()
        segs.release()


# ---- 5: the engine ------------------------------------------------------------------------------------------------------
WORDS = ["w%03d" % i for i in range(40)]
SIZES = [260, 230, 120]
# word -> (segments that hold it, every n-th document of them)
RARE = {"rarea": ((0, 2), 7), "rareb": ((1,), 5), "rarec": ((0, 1, 2), 11), "rared": ((2,), 3)}
COMMON = ["w000", "w001", "w002", "w003"]                                       # present in every segment (asserted)


def make_docs(seg, n, seed):
    """-> (documents for add_documents, the set of words of each)"""
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(len(WORDS)) + 2.0)
    p /= p.sum()
    docs, sets = [], []
    for i in range(n):
        words = [WORDS[j] for j in rng.choice(len(WORDS), int(rng.integers(6, 30)), p=p)]
        words += [w for w, (where, every) in RARE.items() if seg in where and i % every == 0 for _ in range(1 + i % 3)]
        docs.append((b"s%dd%04d" % (seg, i), b"Title %d" % i, b"pdf_json/%d_%d.json" % (seg, i), " ".join(words).encode()))
        sets.append(set(words))
    return docs, sets


def date_of(seg, i):
    r = (i * 7 + seg * 3) % 11
    y = 2018 + (i + seg) % 4
    if r < 6:
        return "%04d-%02d-%02d" % (y, 1 + i % 12, 1 + i % 28)
    if r < 8:
        return "%04d-%02d" % (y, 1 + i % 12)
    return ["%04d" % y, "", None][r - 8]


@pytest.fixture(scope="module")
def served(tmp_path_factory):
    index = str(tmp_path_factory.mktemp("boolean_gpu") / "index")
    os.makedirs(index)
    eng = nsbind.Engine.create(index, 0)
    sets, lines = [], ["cord_uid,title,publish_time,authors,url"]
    for s, n in enumerate(SIZES):
        docs, ws = make_docs(s, n, 1 + s)
        eng.add_documents(docs)
        sets.append(ws)
        for i, d in enumerate(docs):
            t = date_of(s, i)
            if t is not None:
                lines.append("%s,T,%s,A B,http://x" % (d[0].decode(), t))
    with open(os.path.join(index, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.reload()
    assert eng.num_segments == 3
    # the precondition of the identities below: common words in every segment, rare words in some
    for w in COMMON:
        assert all(sum(w in d for d in sets[s]) >= 2 for s in range(3)), w
    for w, (where, _) in RARE.items():
        assert [any(w in d for d in sets[s]) for s in range(3)] == [s in where for s in range(3)], w
    eng.set_cache(False)
    yield {"index": index, "eng": eng, "sets": sets}
    eng.close()


def bits_where(sets, pred):
    """one keep-bitmap per segment: the documents whose word set satisfies pred"""
    out = []
    for ws in sets:
        words = np.zeros((len(ws) + 31) // 32, np.uint32)
        for d, w in enumerate(ws):
            if pred(w):
                words[d >> 5] |= np.uint32(1) << np.uint32(d & 31)
        out.append(words)
    return out


def same(label, got, want):
    """(hits, nhits, found, has) of the boolean call against the search's; returns the queries with found >= 2"""
    hits, nhits, found, has = got
    w_hits, w_nhits, w_found, w_has = want
    assert list(has) == list(w_has), label
    np.testing.assert_array_equal(found, np.where(w_has, w_found, 0), err_msg=str(label))
    np.testing.assert_array_equal(nhits, np.where(w_has, w_nhits, 0), err_msg=str(label))
    for q in range(len(found)):
        n = int(nhits[q])
        for field in ("seg", "doc"):
            np.testing.assert_array_equal(hits[q, :n][field], w_hits[q, :n][field], err_msg=str((label, q, field)))
        np.testing.assert_array_equal(hits[q, :n]["score"].view(np.uint32), w_hits[q, :n]["score"].view(np.uint32), err_msg=str((label, q)))
        tail = hits[q, n:]
        assert np.all(tail["score"].view(np.uint32) == boolean_ref.PAD_SCORE_BITS) and np.all(tail["seg"] == boolean_ref.PAD_ID) and np.all(tail["doc"] == boolean_ref.PAD_ID)
    return int(np.sum(found >= 2))


PLAIN = ["w000", "w001 w002", "w003 w010 w020", "w030", "zzzzqq w004", "zzzzqq", "the of", "", "w002 W002", "rarea", "rareb rarec", "rared rarea w039",
         "covid-19 w001"]
REQUIRED = [["w000"], ["w001", "w002"], ["w003", "w000", "w002"], ["w001", "w001"], ["w002", "w003"]]
EXCLUDES = [("w001 w002", "w000"), ("w003", "w001"), ("rarea w010", "rarec"), ("w000 w001 w002 w003", "w004"), ("rareb", "rareb"), ("w005 w006", "zzzzqq"),
            ("w002", "rared")]
ANCHORED = [("w000", "w001 w002"), ("rarea", "w000 w003"), ("w002", "w002 rarec"), ("rared", "rareb w001")]


@pytest.mark.parametrize("K", [10, 100])
def test_plain_words_are_the_or_search_and_required_words_the_and_search(served, K):
    eng = served["eng"]
    covered = same(("a b", K), eng.search_boolean_batch(PLAIN, K), eng.search_batch(PLAIN, K, 0))
    assert covered >= 8, covered
    plus = [" ".join("+" + w for w in q) for q in REQUIRED]
    covered = same(("+a +b", K), eng.search_boolean_batch(plus, K), eng.search_batch([" ".join(q) for q in REQUIRED], K, AND))
    assert covered >= 4, covered


@pytest.mark.parametrize("date", [None, ("2019", "2020-06", True)], ids=["whole", "dated"])
def test_excluded_and_anchored_words_are_searches_under_a_bitmap(served, date):
    """`a b -c` == the OR search of `a b` over the documents without c; `+a b` == the OR search of `a b` over the documents with
    a; under a date filter's handle both hold against the bitmap AND-ed with the filter's"""
    eng, sets = served["eng"], served["sets"]
    K = 100
    hd = eng.open_filter(*date) if date else 0
    dbits = eng.filter_bits(*date) if date else None
    covered = 0
    try:
        if date:                                                                 # the plain identities under the handle
            covered += same(("a b", date), eng.search_boolean_batch(PLAIN, K, handle=hd), eng.search_filtered_batch(hd, PLAIN, K, 0))
            plus = [" ".join("+" + w for w in q) for q in REQUIRED]
            same(("+a +b", date), eng.search_boolean_batch(plus, K, handle=hd), eng.search_filtered_batch(hd, [" ".join(q) for q in REQUIRED], K, AND))
        for words, c in EXCLUDES:
            bits = bits_where(sets, lambda w: c not in w)
            if dbits:
                bits = [b & d for b, d in zip(bits, dbits)]
            h = eng.open_filter(bits=bits)
            try:
                covered += same((words, "-" + c, date), eng.search_boolean_batch([words + " -" + c], K, handle=hd), eng.search_filtered_batch(h, [words], K, 0))
            finally:
                eng.close_filter(h)
        for a, rest in ANCHORED:
            bits = bits_where(sets, lambda w: a in w)
            if dbits:
                bits = [b & d for b, d in zip(bits, dbits)]
            h = eng.open_filter(bits=bits)
            try:
                covered += same(("+" + a, rest, date), eng.search_boolean_batch(["+" + a + " " + rest], K, handle=hd),
                                eng.search_filtered_batch(h, [a + " " + rest], K, 0))
            finally:
                eng.close_filter(h)
        assert covered >= 8, covered
    finally:
        if hd:
            eng.close_filter(hd)
    if hd:
        with pytest.raises(RuntimeError, match="stale"):
            eng.search_boolean_batch(PLAIN, 10, handle=hd)


def test_a_required_word_that_a_segment_lacks_leaves_that_segment_out(served):
    eng, sets = served["eng"], served["sets"]
    queries = ["+w000 +rarea", "+w000 +rareb", "+rared w000", "+w000 +zzzzqq", "+zzzzqq", "w000 +zzzzqq -w001", "-w000", "-w000 -w001", "+the", "- +", "+w000 -w000"]
    hits, nhits, found, has = eng.search_boolean_batch(queries, 100)
    assert list(has) == [1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1]                        # exclusions alone, stop words alone: not usable
    for q, (need, lacking) in enumerate(((("w000", "rarea"), 1), (("w000", "rareb"), 0), (("rared",), 0))):
        want = sum(all(w in d for w in need) for s in range(3) for d in sets[s])
        assert int(found[q]) == want >= 2, (q, int(found[q]), want)
        assert lacking not in {int(x) for x in hits[q, :int(nhits[q])]["seg"]}
        per_seg = [sum(all(w in d for w in need) for d in sets[s]) for s in range(3)]
        assert per_seg[lacking] == 0 and sum(1 for n in per_seg if n) < 3
    for q in (3, 4, 5, 10):                                                      # a word nobody holds is required; a word is required and excluded
        assert int(found[q]) == 0 and int(nhits[q]) == 0
    assert np.all(found[6:10] == 0) and np.all(nhits[6:10] == 0)
    assert np.all(hits[3]["seg"] == boolean_ref.PAD_ID)


def with_boolean(base, must, must_not, should):
    """the search body with the "boolean" member in front, in dump(2) layout"""
    member = json.dumps({"must": must, "must_not": must_not, "should": should}, indent=2)
    member = "\n".join("  " + line for line in member.split("\n"))
    assert base.startswith("{\n")
    return '{\n  "boolean": ' + member.lstrip() + ",\n" + base[2:]


def test_search_boolean_is_the_search_body_with_the_boolean_member(served):
    eng = served["eng"]
    try:
        for q, k in (("w001 w002", 10), ("rarea", 100), ("zzzzqq", 3), ("the of", 3), ("", 5)):
            words = [w for w, _ in nsbind.parse_boolean(q)]
            assert eng.search_boolean_json(q, k) == with_boolean(eng.search_json(q, k), [], [], words), q
        body = eng.search_boolean_json("+w001 w002 -w003 +rarec", 7)
        j = json.loads(body)
        assert list(j)[0] == "boolean" and j["boolean"] == {"must": ["w001", "rarec"], "must_not": ["w003"], "should": ["w002"]}
        assert j["query"] == "+w001 w002 -w003 +rarec" and j["k"] == 7 and 2 <= j["found"] and len(j["results"]) == min(7, j["found"])
        assert body == with_boolean(body[:2] + body[body.index('  "found"'):], j["boolean"]["must"], j["boolean"]["must_not"], j["boolean"]["should"])
        hits, nhits, _, _ = eng.search_boolean_batch(["+w001 w002 -w003 +rarec"], 7)
        assert [(e["docId"], e["segment"]) for e in j["results"]] == [(int(h["doc"]), eng.segment_name(int(h["seg"]))) for h in hits[0, :int(nhits[0])]]
        j = json.loads(eng.search_boolean_json("-w001", 5))
        assert "found" not in j and j["results"] == [] and j["boolean"] == {"must": [], "must_not": ["w001"], "should": []}
        # under a filter: search_filtered's body
        base = eng.search_filtered_json("w001 w002", 50, "2019-06", "2020")
        body = eng.search_boolean_json("w001 w002", 50, date_filter=("2019-06", "2020", False))
        assert body == with_boolean(base, [], [], ["w001", "w002"])
        assert list(json.loads(body))[:2] == ["boolean", "filter"]
        bad = eng.search_boolean_json("w000", 3, date_filter=("2019-13", "", False), check=False)
        assert bad.startswith('{\n  "error": "') and "is not YYYY, YYYY-MM or YYYY-MM-DD" in bad
    finally:
        eng.reload()                                                            # closes search_filtered's filters
        eng.set_cache(False)


def test_ns_tool_search_boolean(served):
    eng = served["eng"]
    tool = os.path.join(PKG, "ns_tool")
    try:
        want = eng.search_boolean_json("+w001 w002 -w003", 50)
        out = subprocess.run([tool, "search-boolean", served["index"], "-", "-", "50", "+w001", "w002", "-w003"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout == want + "\n"
        want = eng.search_boolean_json("w000 -rarec", 3, date_filter=("", "2019", False))
        out = subprocess.run([tool, "search-boolean", served["index"], "-", "2019", "3", "w000 -rarec"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout == want + "\n"
    finally:
        eng.reload()
        eng.set_cache(False)
