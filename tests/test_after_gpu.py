"""Pages past the first K on the GPU (csrc/ns_after.hip, ns_search_boolean_after, ns_search_sorted_after, Engine::search_after_batch_flat,
Engine::search_page).

1. The raw C-ABI against the restatement tests/after_ref.py on the families of tests/after_shapes.py: walks (the last hit of a
   page handed back until nothing is left) and arbitrary cursors, in this process on the product library, in ONE child on the
   variants build with tiles of 128 and windows of 32 documents (there also the sub-batches), and in ONE child on the counting
   build, which reports ns_debug_after_counters.
2. The product build's tile and window edges.
3. Refusals.
4. The engine: search_after_batch against search_batch and search_boolean_batch, with and without a date filter;
   search_page's JSON followed from page to page; the ns_tool subcommand.
Every comparison is exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import after_shapes
import nsbind
import sorted_shapes
from conftest import PKG, VARIANTS_LIB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_LIB = os.path.join(PKG, "libnextsearch_hip_count.so")
AND = nsbind.NS_FLAG_AND
# A child loads a library, creates a context and runs the small families: 60 s for a shared device.
CHILD_TIMEOUT_S = 60
IN_TEST_BUILD = os.path.basename(os.environ.get("NS_HIP_LIB", "")) not in ("", "libnextsearch_hip.so")


# ---- 1: the raw ABI -----------------------------------------------------------------------------------------------------
def test_boolean_walks_visit_the_whole_ranking_once():
    """every role mix, one and three segments, K = 7, 64, 65, 100"""
    pages = after_shapes.run_boolean_walks()
    assert pages[("directed 3", 7)] > pages[("directed 3", 100)] > 2, pages


def test_a_walk_at_k_1_through_tied_scores():
    assert after_shapes.run_tied_walk() == 901


@pytest.mark.parametrize("pattern", sorted_shapes.PATTERNS)
def test_sorted_walks_visit_the_whole_order_once(pattern):
    """OR / AND x newest / oldest, K = 7, 64, 65, 100, one and three segments"""
    pages = after_shapes.run_sorted_walks(pattern)
    assert pages[("multi", 0, 7)] > pages[("multi", 0, 100)] > 2, pages


def test_arbitrary_boolean_cursors_equal_the_restatement():
    after_shapes.run_boolean_cursors()


def test_arbitrary_sorted_cursors_equal_the_restatement():
    after_shapes.run_sorted_cursors()


def child(lib, tmp_path):
    assert os.path.exists(lib), os.path.basename(lib) + " is missing: make -C nextsearch-api_amd all"
    out = str(tmp_path / "after.json")
    env = dict(os.environ, NS_HIP_LIB=lib, NS_FACET_TILE_DOCS=str(after_shapes.SMALL_TILE), NS_BOOL_WIN_DOCS=str(after_shapes.SMALL_WIN))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "after_shapes.py"), out], env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "after shapes OK" in r.stdout, tail
    with open(out) as f:
        return json.load(f)


def test_tiles_of_128_and_windows_of_32_documents_in_the_variants_build(tmp_path):
    """the same families where a cursor falls before, inside and behind tiles of its own segment; and a batch whose work
    items cross the candidate buffer at K = 100, every query with a cursor of its own"""
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process")
    rep = child(VARIANTS_LIB, tmp_path)
    assert rep["tile"] == after_shapes.SMALL_TILE and not rep["counting"]
    sb = rep["sub_batches"]
    assert sb["items"] > sb["max_items"] == (64 << 20) // 800, sb


def test_the_cursor_families_reach_every_counter_in_the_counting_build(tmp_path):
    """every counter of ns_debug_after_counters is above 0; a batch of unset cursors leaves them at 0"""
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process")
    rep = child(COUNT_LIB, tmp_path)
    assert rep["tile"] == after_shapes.SMALL_TILE and rep["counting"]
    assert rep["unset"] == {e: 0 for e in nsbind.AFTER_EVENTS}, rep["unset"]
    for which in ("boolean", "sorted"):
        for e in nsbind.AFTER_EVENTS:
            assert rep[which][e] > 0, (which, e, rep[which])
        assert rep[which]["bounded_items"] > rep[which]["bound_in_tile"] and rep[which]["bounded_items"] > rep[which]["bound_zero"]


# ---- 2: the product's edges ---------------------------------------------------------------------------------------------
def test_cursors_at_the_product_window_and_tile_edges():
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process: the family is built for the product's tile and window")
    tile, n = after_shapes.run_product_edges()
    assert tile == 1 << 17 and n == 262149


# ---- 3: refusals --------------------------------------------------------------------------------------------------------
def test_refusals():
    after_shapes.run_refusals()


# ---- 4: the engine ------------------------------------------------------------------------------------------------------
WORDS = ["w%03d" % i for i in range(40)]
SIZES = [260, 230, 120]
# word -> (segments that hold it, every n-th document of them)
RARE = {"rarea": ((0, 2), 7), "rareb": ((1,), 5), "rarec": ((0, 1, 2), 11), "rared": ((2,), 3)}


def make_docs(seg, n, seed):
    """documents for add_documents: common words by a skewed draw, rare words in some segments only"""
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(len(WORDS)) + 2.0)
    p /= p.sum()
    docs = []
    for i in range(n):
        words = [WORDS[j] for j in rng.choice(len(WORDS), int(rng.integers(6, 30)), p=p)]
        words += [w for w, (where, every) in RARE.items() if seg in where and i % every == 0 for _ in range(1 + i % 3)]
        docs.append((b"s%dd%04d" % (seg, i), b"Title %d" % i, b"pdf_json/%d_%d.json" % (seg, i), " ".join(words).encode()))
    return docs


def date_of(seg, i):
    """full dates, months, years, empty dates and documents without a metadata row"""
    r = (i * 7 + seg * 3) % 11
    y = 2018 + (i + seg) % 4
    if r < 6:
        return "%04d-%02d-%02d" % (y, 1 + i % 12, 1 + i % 28)
    if r < 8:
        return "%04d-%02d" % (y, 1 + i % 12)
    return ["%04d" % y, "", None][r - 8]


@pytest.fixture(scope="module")
def served(tmp_path_factory):
    index = str(tmp_path_factory.mktemp("after_gpu") / "index")
    os.makedirs(index)
    eng = nsbind.Engine.create(index, 0)
    lines = ["cord_uid,title,publish_time,authors,url"]
    for s, n in enumerate(SIZES):
        docs = make_docs(s, n, 1 + s)
        eng.add_documents(docs)
        for i, d in enumerate(docs):
            t = date_of(s, i)
            if t is not None:
                lines.append("%s,T,%s,A B,http://x" % (d[0].decode(), t))
    with open(os.path.join(index, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.reload()
    assert eng.num_segments == 3
    eng.set_cache(False)
    yield {"index": index, "eng": eng}
    eng.close()


PLAIN = ["w000", "w001 w002", "w003 w010 w020", "w030", "zzzzqq w004", "zzzzqq", "the of", "", "rarea", "rareb rarec", "rared rarea w039"]
# words every segment holds: with them `+a +b` is the AND search (a required word that a segment lacks takes that segment out
# of the boolean answer, while the AND search goes on with the words the segment has)
REQUIRED = ["w000", "w001 w002", "w003 w000 w002", "w001 w001", "w002 w003", "the of", ""]
DATE = ("2019", "2020-06", True)


def same_rows(label, got, want):
    hits, nhits, found, has = got
    w_hits, w_nhits, w_found, w_has = want
    assert list(has) == list(w_has), label
    np.testing.assert_array_equal(found, np.where(w_has, w_found, 0), err_msg=str(label))
    np.testing.assert_array_equal(nhits, np.where(w_has, w_nhits, 0), err_msg=str(label))
    for q in range(len(found)):
        n = int(nhits[q])
        assert hits[q, :n].tobytes() == w_hits[q, :n].tobytes(), (label, q)
        assert np.all(hits[q, n:]["doc"] == 0xFFFFFFFF) and np.all(hits[q, n:]["score"].view(np.uint32) == 0xFF800000), (label, q)


def walk_engine(call, K, Q):
    """-> per query the concatenated (score bits, seg, doc) of all pages, and the first page's found"""
    cursors, seen, total = None, [[] for _ in range(Q)], None
    for _ in range(1000):
        hits, nhits, found, rest, has = call(cursors)
        if total is None:
            total = found.copy()
        np.testing.assert_array_equal(found, total)
        nxt = [None] * Q if cursors is None else list(cursors)
        for q in range(Q):
            n = int(nhits[q])
            assert int(rest[q]) == int(total[q]) - len(seen[q]) and n == min(K, int(rest[q])), (q, int(rest[q]), n)
            seen[q] += [(int(h["score"].view(np.uint32)), int(h["seg"]), int(h["doc"])) for h in hits[q, :n]]
            if n:
                nxt[q] = seen[q][-1]
        if not np.any(nhits):
            return seen, total
        cursors = nxt
    raise AssertionError("the walk does not end")


@pytest.mark.parametrize("date", [None, DATE], ids=["whole", "dated"])
def test_search_after_is_search_on_page_one_and_the_boolean_ranking_to_the_end(served, date):
    eng = served["eng"]
    hd = eng.open_filter(*date) if date else 0
    try:
        for flags, as_boolean in ((0, lambda q: q), (AND, lambda q: " ".join("+" + w for w in q.split()))):
            for K in (10, 100):
                want = eng.search_filtered_batch(hd, PLAIN, K, flags) if hd else eng.search_batch(PLAIN, K, flags)
                hits, nhits, found, rest, has = eng.search_after_batch(PLAIN, K, flags=flags, handle=hd)
                same_rows(("page 1", flags, K, date), (hits, nhits, found, has), want)
                np.testing.assert_array_equal(rest, found)
            # walked to the end: search_boolean_batch of the same terms at K = 100 is the head of it, found its length
            K = 7
            texts = REQUIRED if flags else PLAIN
            seen, total = walk_engine(lambda c: eng.search_after_batch(texts, K, after=c, flags=flags, handle=hd), K, len(texts))
            b_hits, b_nhits, b_found, b_has = eng.search_boolean_batch([as_boolean(q) for q in texts], 100, handle=hd)
            assert max(int(t) for t in total) > 100
            for q in range(len(texts)):
                assert len(seen[q]) == int(total[q]) == int(b_found[q]), (q, len(seen[q]), int(total[q]), int(b_found[q]))
                assert len(set((s, d) for _, s, d in seen[q])) == len(seen[q])
                head = [(int(h["score"].view(np.uint32)), int(h["seg"]), int(h["doc"])) for h in b_hits[q, :int(b_nhits[q])]]
                assert seen[q][:len(head)] == head, (q, flags)
                order = [(-after_shapes.after_ref.ord32(b), s, d) for b, s, d in seen[q]]
                assert order == sorted(order), (q, flags)
            # the boolean and the sorted calls page the same way
            bq = [as_boolean(q) for q in texts]
            b_seen, b_total = walk_engine(lambda c: eng.search_boolean_after_batch(bq, 64, after=c, handle=hd), 64, len(bq))
            assert b_seen == seen and list(b_total) == list(total)

        def sorted_call(c):
            hits, keys, nhits, found, rest, has = eng.search_sorted_after_batch(PLAIN, 65, after=c, order="oldest", handle=hd)
            hits = hits.copy()
            hits["score"] = keys.view(np.float32)                              # walk_engine hands the rank back: here the key
            return hits, nhits, found, rest, has
        s_seen, s_total = walk_engine(sorted_call, 65, len(PLAIN))
        first = eng.search_sorted_batch(PLAIN, 65, order="oldest", handle=hd)
        for q in range(len(PLAIN)):
            n = int(first[2][q])
            assert [(k, s, d) for k, s, d in s_seen[q][:n]] == [(int(first[1][q, i]), int(first[0][q, i]["seg"]), int(first[0][q, i]["doc"])) for i in range(n)]
            assert len(s_seen[q]) == int(s_total[q]) and len(set((s, d) for _, s, d in s_seen[q])) == len(s_seen[q])
            order = [(-after_shapes.after_ref.sort_rank(k, True), s, d) for k, s, d in s_seen[q]]
            assert order == sorted(order), q
    finally:
        if hd:
            eng.close_filter(hd)


def follow(eng, query, k, **kw):
    """search_page_json from the first page along "next" -> the bodies"""
    bodies, cursor = [], ""
    for _ in range(500):
        body = eng.search_page_json(query, k, cursor=cursor, **kw)
        bodies.append(body)
        page = json.loads(body)["page"]
        assert page["cursor"] == cursor
        if "next" not in page:
            return bodies
        cursor = page["next"]
    raise AssertionError("the pages do not end")


def test_search_page_follows_next_through_exactly_found_documents(served):
    eng = served["eng"]
    try:
        cases = [("w001 w002", 25, dict(mode="or"), lambda: eng.search_json("w001 w002", 25)),
                 ("w001 w002", 25, dict(mode="and"), None),
                 ("+w001 w002 -w003", 30, dict(mode="boolean"), lambda: eng.search_boolean_json("+w001 w002 -w003", 30)),
                 ("w001 w002", 40, dict(mode="sorted", order="newest"), lambda: eng.search_sorted_json("w001 w002", 40, order="newest")),
                 ("w000", 100, dict(mode="sorted", order="oldest", date_filter=DATE), lambda: eng.search_sorted_json("w000", 100, order="oldest", date_filter=DATE)),
                 ("w000 w003", 9, dict(mode="or", date_filter=DATE), lambda: eng.search_filtered_json("w000 w003", 9, *DATE)),
                 ("w000", 10, dict(mode="boolean", date_filter=DATE), lambda: eng.search_boolean_json("w000", 10, date_filter=DATE))]
        for query, k, kw, existing in cases:
            bodies = follow(eng, query, k, **kw)
            first = json.loads(bodies[0])
            if existing is not None:
                base = json.loads(existing())
                assert first["results"] == base["results"] and first["found"] == base["found"], (query, kw)
                rest = {m: v for m, v in first.items() if m != "page"}
                assert rest == base and list(first) == sorted(first), (query, kw)      # the mode's body plus "page", keys in dump order
            found = first["found"]
            assert found > k and len(bodies) == -(-found // k), (query, kw, found, len(bodies))
            seen = []
            for i, b in enumerate(bodies):
                j = json.loads(b)
                member = "\n".join("  " + line for line in json.dumps(j["page"], indent=2).split("\n"))
                assert b.startswith("{\n  \"") and "\n  \"page\": " + member.lstrip() + ",\n  \"query\": " in b, (query, kw)     # dump(2) layout
                assert j["found"] == found and j["page"]["offset"] == len(seen), (query, kw, i)
                seen += [(e["segment"], e["docId"]) for e in j["results"]]
                assert j["page"]["remaining"] == found - len(seen) and ("next" in j["page"]) == (len(seen) < found), (query, kw, i)
            assert len(seen) == found == len(set(seen)), (query, kw)
        # failures: a cursor of the wrong kind, a position past the index, a position the filter keeps nothing of, a broken cursor
        for kw, cursor, why in ((dict(mode="or"), "d0134a3a5.0.1", "does not fit"), (dict(mode="sorted"), "s3f800000.0.1", "does not fit"),
                                (dict(mode="or"), "s3f800000.3.1", "names position 3, the index has 3 segments"),
                                (dict(mode="boolean"), "s3f800000.4294967295.1", "names position 4294967295"),
                                (dict(mode="or"), "s3f800000.0", "expected"),
                                (dict(mode="or", date_filter=("1990", "1991", False)), "s3f800000.1.1", "of which the filter keeps nothing")):
            body = eng.search_page_json("w000", 5, cursor=cursor, check=False, **kw)
            assert body.startswith('{\n  "error": "') and why in json.loads(body)["error"], body
            with pytest.raises(RuntimeError, match="search_page failed"):
                eng.search_page_json("w000", 5, cursor=cursor, **kw)
        # a query without usable terms has no "found" and no "next"
        j = json.loads(eng.search_page_json("the of", 5))
        assert "found" not in j and j["results"] == [] and j["page"] == {"cursor": "", "offset": 0, "remaining": 0}
    finally:
        eng.reload()                                                            # closes search_filtered's filters
        eng.set_cache(False)


def test_ns_tool_page(served):
    eng = served["eng"]
    tool = os.path.join(PKG, "ns_tool")
    try:
        first = eng.search_page_json("w001 w002", 20)
        nxt = json.loads(first)["page"]["next"]
        want = eng.search_page_json("w001 w002", 20, cursor=nxt)
        out = subprocess.run([tool, "page", served["index"], "or", "-", "-", "20", nxt, "w001", "w002"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout == want + "\n" and json.loads(want)["page"]["offset"] == 20
        want = eng.search_page_json("w000", 7, mode="sorted", order="oldest", date_filter=("", "2019", False))
        out = subprocess.run([tool, "page", served["index"], "oldest", "-", "2019", "7", "-", "w000"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout == want + "\n"
        out = subprocess.run([tool, "page", served["index"], "or", "-", "-", "7", "d0134a3a5.0.1", "w000"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 1 and "does not fit" in out.stderr
    finally:
        eng.reload()
        eng.set_cache(False)
