"""Search sorted by date on the GPU (csrc/ns_sorted.hip, Engine::search_sorted_batch_flat, Engine::search_sorted).

1. The raw C-ABI against the restatement tests/sorted_ref.py on the directed inputs of tests/sorted_shapes.py: in this process
   on the product library (one tile of 2^17 documents holds the small family; a family of two product tiles + 5 documents
   hits the product's tile edges), and in ONE child process on the variants build with tiles of 128 documents.
2. A child on the counting build asserts that the inputs reach every counted path of the three kernels.
3. The engine: found and usable equal the search's; a query with at most K matches returns the search's hits re-sorted, score
   bits included, with and without a filter; the newest year's hits agree with the facet counts; the JSON of search_sorted
   is search's with "results" re-sorted plus the "sort" member.
Every comparison is exact."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nsbind
import sorted_ref
import sorted_shapes
from conftest import PKG, VARIANTS_LIB
from rawseg import RawSegments, descriptors_multi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_LIB = os.path.join(PKG, "libnextsearch_hip_count.so")
NS_E_INVAL = -1
AND, ASC = nsbind.NS_FLAG_AND, nsbind.NS_SORT_ASC
# A child loads a library, creates a context and runs the small families: a few seconds of work, 30 s for a shared device.
CHILD_TIMEOUT_S = 30
IN_TEST_BUILD = os.path.basename(os.environ.get("NS_HIP_LIB", "")) not in ("", "libnextsearch_hip.so")


# ---- 1: the raw ABI -----------------------------------------------------------------------------------------------------
def test_small_family_equals_the_restatement():
    """lists of 0 .. 257 postings, queries of 0, 1, 2, 8 and 70 refs, K = 1, 10, 63, 64, 65, 100, both directions, OR and
    AND, with and without skip tables; then the key patterns (here: whatever tile the loaded library has)"""
    sorted_shapes.run_small()


def test_found_around_k():
    sorted_shapes.run_counts()


def test_two_product_tiles_and_five_documents():
    tile, n = sorted_shapes.run_product_tile()
    assert n == 2 * tile + 5
    if not IN_TEST_BUILD:
        assert tile == 1 << 17 and n == 262149


def test_several_segments_and_found_of_the_scoring_path():
    sorted_shapes.run_multi()


def test_on_filtered_copies():
    sorted_shapes.run_filtered()


def child(lib, tmp_path):
    assert os.path.exists(lib), os.path.basename(lib) + " is missing: make -C nextsearch-api_amd all"
    out = str(tmp_path / "sorted.json")
    env = dict(os.environ, NS_HIP_LIB=lib, NS_FACET_TILE_DOCS=str(sorted_shapes.SMALL_TILE))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sorted_shapes.py"), out], env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "sorted shapes OK" in r.stdout, tail
    with open(out) as f:
        return json.load(f)


def test_tiles_of_128_documents_in_the_variants_build(tmp_path):
    """the same families where 300 documents are two whole tiles and a part: every tile edge decides a tie"""
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process")
    rep = child(VARIANTS_LIB, tmp_path)
    assert rep["tile"] == sorted_shapes.SMALL_TILE and not rep["counting"]


def test_the_directed_inputs_reach_their_paths_in_the_counting_build(tmp_path):
    """every counter of ns_debug_sorted_counters was reached; an OR hit that one of its query's lists does not hold was scored"""
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process")
    rep = child(COUNT_LIB, tmp_path)
    assert rep["tile"] == sorted_shapes.SMALL_TILE and rep["counting"]
    assert not rep["missed"], rep
    ev = rep["events"]
    for e in sorted_shapes.SORTED_EVENTS:
        assert ev[e] > 0, (e, ev)
    assert ev["score_not_found"] > 0 and ev["items"] > ev["single_list_items"] + ev["and_early_outs"]


def test_refusals():
    """each NS_E_INVAL with a message and nothing launched: the output arrays keep their fill"""
    L = nsbind.hip_lib()
    segments, queries = sorted_shapes.multi_family()
    segs = RawSegments(segments)
    tabs = []
    try:
        ctx = segs.ctx
        one = [[1.0] * len(s[2]) for s in segments]
        qd, refs = descriptors_multi(queries, segs.lists, segs.offs, one, one)

        def refused(rc, match):
            assert rc == NS_E_INVAL, rc
            msg = L.ns_last_error(ctx).decode()
            assert match in msg, msg

        # ns_dockeys_upload
        keys = np.zeros(300, np.uint32)
        h = C.c_void_p()
        refused(L.ns_dockeys_upload(ctx, 300, keys.ctypes.data, None), "out is NULL")
        refused(L.ns_dockeys_upload(ctx, 300, None, C.byref(h)), "keys is NULL")
        assert L.ns_dockeys_upload(None, 300, keys.ctypes.data, C.byref(h)) == NS_E_INVAL
        for at in (0, 299):
            bad = keys.copy()
            bad[at] = 0xFFFFFFFF
            rc, h = nsbind.dockeys_upload(ctx, bad)
            refused(rc, "reserved key 0xFFFFFFFF")
            assert not h.value
        bad[299] = 0xFFFFFFFE                                                    # the largest legal key
        bad[0] = 0
        rc, h = nsbind.dockeys_upload(ctx, bad)
        assert rc == 0
        tabs.append(h)

        def table(n):
            rc, t = nsbind.dockeys_upload(ctx, np.arange(n, dtype=np.uint32))
            assert rc == 0, segs.err()
            tabs.append(t)
            return t

        good = [table(s[0]) for s in segments]
        short = table(299)

        def run(qd=qd, refs=refs, ids=(0, 1, 2), hs=None, ts=None, flags=0):
            rc, hits, kk, nhits, found, _ = nsbind.search_sorted_raw(ctx, qd, refs, 10, flags, list(ids), segs.segs if hs is None else hs, good if ts is None else ts)
            if rc != 0:
                assert np.all(hits.view(np.uint8) == 0xAB) and np.all(kk == 0xABABABAB) and np.all(nhits == 0xABABABAB) and np.all(found == 0xABABABAB), \
                    "a refused call writes nothing"
            return rc

        assert run() == 0
        refused(run(ts=[short, good[1], good[2]]), "keys 299 documents, its segment has 300")
        refused(run(ids=(0, 1), hs=segs.segs[:2], ts=good[:2]), "names segment 2, which the call does not list")
        refused(run(ids=(0, 1, 1)), "seg_id 1 is listed twice")
        refused(run(flags=0x100), "only NS_FLAG_AND and NS_SORT_ASC")
        past = refs.copy()
        past["byte_off"][0] = 8 * 10 ** 6
        refused(run(refs=past), "runs past the postings")
        odd = refs.copy()
        odd["byte_off"][0] += 4
        refused(run(refs=odd), "not a multiple of 8")
        over = qd.copy()
        over["term_count"][-1] = len(refs) + 1
        refused(run(qd=over), "run past the")
        # null arguments, straight through ctypes
        K = 10
        hits, kk = np.zeros((len(qd), K), nsbind.HIT_DTYPE), np.zeros((len(qd), K), np.uint32)
        nh, fnd = np.zeros(len(qd), np.uint32), np.zeros(len(qd), np.uint64)
        sid = np.array([0, 1, 2], np.uint32)
        sa = (C.c_void_p * 3)(*[s.value for s in segs.segs])
        ta = (C.c_void_p * 3)(*[t.value for t in good])
        args = [ctx, qd.ctypes.data, len(qd), refs.ctypes.data, len(refs), K, 0, sid.ctypes.data, sa, ta, 3, hits.ctypes.data, kk.ctypes.data,
                nh.ctypes.data, fnd.ctypes.data, None]
        assert L.ns_search_sorted(*args) == 0                                   # device_ms_out may be NULL
        assert L.ns_search_sorted(*(args[:14] + [None, None])) == 0              # found_out too
        for at, match in ((1, "null argument"), (3, "null argument"), (11, "null argument"), (12, "null argument"), (13, "null argument"),
                          (7, "null segment arrays"), (8, "null segment arrays"), (9, "null segment arrays")):
            a = list(args)
            a[at] = None
            refused(L.ns_search_sorted(*a), match)
        a = list(args)
        a[10] = 0
        refused(L.ns_search_sorted(*a), "no segment listed")
        a = list(args)
        a[8] = (C.c_void_p * 3)(segs.segs[0].value, None, segs.segs[2].value)
        refused(L.ns_search_sorted(*a), "segment or key table 1 is NULL")
        assert L.ns_search_sorted(None, *args[1:]) == NS_E_INVAL
        # no queries: NS_OK, nothing touched, whatever else is passed
        assert L.ns_search_sorted(ctx, None, 0, None, 0, 10, 0, None, None, None, 0, None, None, None, None, None) == 0
        refused(L.ns_dockeys_release(ctx, None), "does not belong to this ctx")
    finally:
        for t in tabs:
            L.ns_dockeys_release(segs.ctx, t)
        segs.release()


# ---- 2: the engine ------------------------------------------------------------------------------------------------------
WORDS = ["w%03d" % i for i in range(60)]
RARE = {"rare%02d" % i: n for i, n in enumerate([2, 3, 7, 19, 40, 64, 99, 100])}      # word -> documents that hold it, over all segments
QUERIES = ["w000", "w001 w002", "w003 w010 w020", "w055", "zzzzqq w004", "zzzzqq", "the of", "", "w002 W002",
           "rare00", "rare01", "rare02 rare03", "rare04", "rare05 rare00", "rare06", "rare07", "rare02 rare01 rare00", "rare03 rare04"]
SIZES = [260, 230, 120]
RARE_DOCS = {w: set(np.random.default_rng(100 + i).choice(sum(SIZES), n, replace=False).tolist()) for i, (w, n) in enumerate(RARE.items())}


def make_docs(seg, n, seed, base):
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(len(WORDS)) + 2.0)
    p /= p.sum()
    docs = []
    for i in range(n):
        words = [WORDS[j] for j in rng.choice(len(WORDS), int(rng.integers(8, 40)), p=p)]
        g = base + i                                                             # the document's number over all segments
        words += [w for w in RARE if g in RARE_DOCS[w] for _ in range(1 + g % 3)]
        docs.append((b"s%dd%04d" % (seg, i), b"Title %d" % i, b"pdf_json/%d_%d.json" % (seg, i), " ".join(words).encode()))
    return docs


def date_of(seg, i):
    """four years, by day, by month and by year; undated: empty, malformed, no row (None)"""
    r = (i * 7 + seg * 3) % 11
    y = 2018 + (i + seg) % 4
    if r < 5:
        return "%04d-%02d-%02d" % (y, 1 + i % 12, 1 + i % 28)
    if r < 7:
        return "%04d-%02d" % (y, 1 + i % 12)
    if r == 7:
        return "%04d" % y
    return ["", "Spring 2020", None][r - 8]


def make_index(tmp):
    index = str(tmp / "index")
    os.makedirs(index)
    eng = nsbind.Engine.create(index, 0)
    batches, base = [], 0
    for s, n in enumerate(SIZES):
        batches.append(make_docs(s, n, 1 + s, base))
        base += n
    for b in batches:
        eng.add_documents(b)
    lines = ["cord_uid,title,publish_time,authors,url"]
    for s, b in enumerate(batches):
        for i, d in enumerate(b):
            t = date_of(s, i)
            if t is not None:
                lines.append("%s,T,%s,A B,http://x" % (d[0].decode(), t))
    with open(os.path.join(index, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.reload()
    return index, eng


@pytest.fixture(scope="module")
def served(tmp_path_factory):
    index, eng = make_index(tmp_path_factory.mktemp("sorted_gpu"))
    assert eng.num_segments == 3
    yield {"index": index, "eng": eng}
    eng.close()


def test_tables_are_built_by_the_first_call_and_freed_by_reload(served):
    eng = served["eng"]
    eng.reload()
    assert eng.sort_tables_on_device() == 0                                     # never by reload()
    keys = eng.sort_keys("newest")                                              # host only: still nothing on the device
    assert [len(x) for x in keys] == SIZES and eng.sort_tables_on_device() == 0
    eng.search_sorted_batch(QUERIES[:2], 10, "newest")
    assert eng.sort_tables_on_device() == 3                                     # one per (kind, segment)
    eng.search_sorted_batch(QUERIES[:2], 10, "oldest", flags=AND)
    assert eng.sort_tables_on_device() == 3                                     # both directions read the same table
    eng.search_sorted_batch(QUERIES[:2], 10, "desc", custom=[np.arange(n, dtype=np.uint32) for n in SIZES])
    assert eng.sort_tables_on_device() == 6
    eng.release_sorted()
    assert eng.sort_tables_on_device() == 0
    eng.search_sorted_batch(QUERIES[:2], 10, "newest")
    eng.reload()
    assert eng.sort_tables_on_device() == 0


def resorted(hits_row, n, keys, ascending):
    triples = [(h["score"], int(h["seg"]), int(h["doc"])) for h in hits_row[:n]]
    return sorted_ref.resort(triples, lambda s, d: int(keys[s][d]), lambda s: s, ascending)


def check_against_search(eng, keys, scored, got, K, ascending, label):
    """found and usable equal the search's; where 2 <= found <= K the sorted hits are the search's hits re-sorted, score bits
    included.  Returns how many queries that covered."""
    s_hits, s_nhits, s_found, s_has = scored
    hits, kk, nhits, found, has = got
    assert list(has) == list(s_has), label
    np.testing.assert_array_equal(found, np.where(s_has, s_found, 0), err_msg=str(label))
    np.testing.assert_array_equal(nhits, np.where(s_has, np.minimum(s_found, K), 0).astype(np.uint32), err_msg=str(label))
    covered = 0
    for q in range(len(found)):
        n = int(nhits[q])
        want_keys = [int(keys[int(h["seg"])][int(h["doc"])]) for h in hits[q, :n]]
        assert [int(x) for x in kk[q, :n]] == want_keys, (label, q)
        tail = hits[q, n:]
        assert np.all(tail["score"].view(np.uint32) == sorted_ref.PAD_SCORE_BITS) and np.all(tail["seg"] == sorted_ref.PAD_ID) and np.all(kk[q, n:] == 0)
        if not (has[q] and 2 <= int(found[q]) <= K):
            continue
        covered += 1
        want = resorted(s_hits[q], int(s_nhits[q]), keys, ascending)
        assert [(int(h["seg"]), int(h["doc"])) for h in hits[q, :n]] == [(s, d) for _, s, d in want], (label, q)
        np.testing.assert_array_equal(hits[q, :n]["score"].view(np.uint32), np.array([sc for sc, _, _ in want], np.float32).view(np.uint32),
                                      err_msg=str((label, q)))
    return covered


@pytest.mark.parametrize("flags", [0, AND], ids=["or", "and"])
def test_found_is_the_searchs_and_small_result_sets_are_the_searchs_hits_resorted(served, flags):
    eng = served["eng"]
    keys = eng.sort_keys("newest")
    scored = eng.search_batch(QUERIES, 100, flags)
    for order in ("newest", "oldest"):
        got = eng.search_sorted_batch(QUERIES, 100, order, flags=flags)
        covered = check_against_search(eng, keys, scored, got, 100, order == "oldest", (order, flags))
        assert covered >= 4, covered                                            # the floor: the check passes on something
        # the first page of a larger K is a prefix of nothing else: K = 7 returns the first 7 of K = 100
        few = eng.search_sorted_batch(QUERIES, 7, order, flags=flags)
        for q in range(len(QUERIES)):
            n = int(few[2][q])
            assert n == min(7, int(got[2][q]))
            np.testing.assert_array_equal(few[0][q, :n], got[0][q, :n])
    assert int(scored[2].max()) > 100                                           # and some query has more matches than a page


@pytest.mark.parametrize("flags", [0, AND], ids=["or", "and"])
def test_under_an_open_filter_the_same_holds_against_the_filtered_search(served, flags):
    eng = served["eng"]
    keys = eng.sort_keys("newest")
    h = eng.open_filter("2019", "2020", keep_undated=True)
    try:
        scored = eng.search_filtered_batch(h, QUERIES, 100, flags)
        total = 0
        for order in ("newest", "oldest"):
            got = eng.search_sorted_batch(QUERIES, 100, order, flags=flags, handle=h)
            total += check_against_search(eng, keys, scored, got, 100, order == "oldest", ("filtered", order, flags))
            for q in range(len(QUERIES)):                                        # nothing outside the filter comes back
                for x in got[1][q, :int(got[2][q])]:
                    assert x == 0 or 20190000 <= int(x) <= 20209999
        assert total >= 4
    finally:
        eng.close_filter(h)
    with pytest.raises(RuntimeError, match="stale"):
        eng.search_sorted_batch(QUERIES, 10, "newest", handle=h)


@pytest.mark.parametrize("K", [3, 100])
def test_the_newest_years_hits_agree_with_the_facet_counts(served, K):
    eng = served["eng"]
    labels = eng.facet_buckets("year")[1]
    counts, _, _ = eng.facet_batch(QUERIES, len(labels), "year")
    hits, kk, nhits, found, has = eng.search_sorted_batch(QUERIES, K, "newest")
    checked = 0
    for q in range(len(QUERIES)):
        dated = [b for b in range(1, len(labels)) if counts[q, b]]
        if not dated:
            continue
        b = dated[-1]                                                            # labels ascend: the highest non-empty year
        in_year = sum(int(x) // 10000 == int(labels[b]) for x in kk[q, :int(nhits[q])])
        assert in_year == min(K, int(counts[q, b])), (q, labels[b])
        checked += 1
    assert checked >= 8
    eng.release_facets()


def resorted_body(eng, body, keys, ascending, name):
    """search's JSON text with the entries of "results" in date order and the "sort" member behind "segments" """
    head = '  "results": [\n'
    if head not in body:
        assert '  "results": [],\n' in body
        return body[:-2] + ',\n  "sort": "%s"\n}' % name
    a = body.index(head) + len(head)
    b = body.index("\n  ],\n", a)
    blocks = [blk if blk.endswith("\n    }") else blk + "\n    }" for blk in body[a:b].split("\n    },\n")]
    pos = {eng.segment_name(s): s for s in range(eng.num_segments)}
    ent = [(json.loads(blk), blk) for blk in blocks]
    ent.sort(key=lambda e: (sorted_ref.rank_of(keys[pos[e[0]["segment"]]][e[0]["docId"]], ascending), pos[e[0]["segment"]], e[0]["docId"]))
    return body[:a] + ",\n".join(blk for _, blk in ent) + body[b:-2] + ',\n  "sort": "%s"\n}' % name


def test_search_sorted_is_the_search_body_with_the_results_in_date_order(served):
    eng = served["eng"]
    keys = eng.sort_keys("newest")
    eng.set_cache(False)
    try:
        for q, k in (("rare02 rare03", 100), ("rare01", 5), ("rare04", 100), ("zzzzqq", 3), ("the of", 3), ("rare00", 2)):
            base = eng.search_json(q, k)
            for order in ("newest", "oldest"):
                body = eng.search_sorted_json(q, k, order)
                assert body == resorted_body(eng, base, keys, order == "oldest", order), (q, order)
                j = json.loads(body)
                assert j["sort"] == order and list(j)[-1] == "sort"
                times = [e.get("publish_time", "") for e in j["results"]]
                dated = [t for t in times if nsbind.date_key(t)]
                assert times[:len(dated)] == dated                              # undated entries last, decorated as search's are
                assert [nsbind.date_key(t) for t in dated] == sorted((nsbind.date_key(t) for t in dated), reverse=(order == "newest"))
        # a page of a large result set: the K newest of all matches, which the score-ranked page does not hold
        j = json.loads(eng.search_sorted_json("w000", 5, "newest"))
        assert j["found"] > 100 and len(j["results"]) == 5 and all(e["publish_time"].startswith("2021") for e in j["results"])
        # under a filter: search_filtered's body
        base = eng.search_filtered_json("rare04 rare03", 100, "2019-06", "2020")
        body = eng.search_sorted_json("rare04 rare03", 100, "oldest", date_filter=("2019-06", "2020", False))
        assert body == resorted_body(eng, base, keys, True, "oldest")
        j = json.loads(body)
        assert list(j)[0] == "filter" and 2 <= j["found"] <= 100 and len(j["results"]) == j["found"]
        body = eng.search_sorted_json("rare01", 5, "desc", custom=[np.arange(n, dtype=np.uint32) + 1 for n in SIZES])
        assert json.loads(body)["sort"] == "custom"
        bad = eng.search_sorted_json("w000", 3, "newest", date_filter=("2019-13", "", False), check=False)
        assert bad.startswith('{\n  "error": "') and "is not YYYY, YYYY-MM or YYYY-MM-DD" in bad
    finally:
        eng.set_cache(True)
        eng.reload()                                                            # closes search_filtered's filters


def test_ns_tool_search_sorted(served):
    eng = served["eng"]
    tool = os.path.join(PKG, "ns_tool")
    try:
        want = eng.search_sorted_json("rare02 rare03", 50, "newest")
        out = subprocess.run([tool, "search-sorted", served["index"], "newest", "-", "-", "50", "rare02", "rare03"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout == want + "\n"
        want = eng.search_sorted_json("w000", 3, "oldest", date_filter=("", "2019", False))
        out = subprocess.run([tool, "search-sorted", served["index"], "oldest", "-", "2019", "3", "w000"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout == want + "\n"
        bad = subprocess.run([tool, "search-sorted", served["index"], "best", "-", "-", "3", "w000"], capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2 and "newest or oldest" in bad.stderr
    finally:
        eng.reload()
