"""Facet counts and date order for boolean queries on the GPU (csrc/ns_boolean_sets.hip, Engine::facet_boolean_batch_flat,
Engine::search_boolean_sorted_batch_flat, Engine::search_boolean_faceted / _sorted).

1. The raw C-ABI against the restatement tests/boolean_sets_ref.py on the directed inputs of tests/boolean_sets_shapes.py: in
   this process on the product library (one tile holds a 300-document segment; a family of two product tiles + 5 documents
   hits the product's tile edges), and in ONE child process on the variants build with tiles of 128 documents.
2. Exact equivalences on the same raw inputs: roles == NULL == ns_facet_count / ns_search_sorted under NS_FLAG_OR, all MUST ==
   under NS_FLAG_AND, found == ns_search_boolean's, and where found <= 100 the same (segment, doc, score bits) triples.
3. A child on the counting build asserts that the inputs reach every counted path of the three kernels.
4. Refusals.
5. The engine on a small generated index: facets, date order, JSON, pages, ns_tool.
Every comparison is exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import boolean_sets_shapes as shapes
import nsbind
import test_boolean_gpu as bq
from boolean_ref import MUST, SHOULD
from conftest import PKG, VARIANTS_LIB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_LIB = os.path.join(PKG, "libnextsearch_hip_count.so")
# A child loads a library, creates a context and runs the small families: a few seconds of work, 60 s for a shared device.
CHILD_TIMEOUT_S = 60
IN_TEST_BUILD = os.path.basename(os.environ.get("NS_HIP_LIB", "")) not in ("", "libnextsearch_hip.so")


# ---- 1: the raw ABI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_segs", [1, 3])
def test_directed_role_mixes_equal_the_restatement(n_segs):
    """every role mix at 1, 50 and 1024 buckets and K = 1, 10, 63, 64, 65, 100 in both directions, with and without skip
    tables, keys with ties and undated documents, roles == NULL (here: whatever tile the loaded library has)"""
    shapes.run_directed(n_segs)


def test_found_around_k():
    shapes.run_counts()


def test_date_order_paged_to_exhaustion():
    pages = shapes.run_walks()
    assert pages[(1, 0)] >= 257 and pages[(10, 0)] == pages[(10, shapes.ASC)] >= 30 and pages[(64, 0)] >= 5, pages


def test_cursors_that_are_no_document_of_the_set():
    shapes.run_cursors()


def test_two_product_tiles_and_five_documents():
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process: the family is built for the product's tile")
    tile, n = shapes.run_product_tile()
    assert tile == 1 << 17 and n == 262149


def child(lib, tmp_path):
    assert os.path.exists(lib), os.path.basename(lib) + " is missing: make -C nextsearch-api_amd all"
    out = str(tmp_path / "boolean_sets.json")
    env = dict(os.environ, NS_HIP_LIB=lib, NS_FACET_TILE_DOCS=str(shapes.SMALL_TILE))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "boolean_sets_shapes.py"), out], env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "boolean sets shapes OK" in r.stdout, tail
    with open(out) as f:
        return json.load(f)


def test_tiles_of_128_documents_in_the_variants_build(tmp_path):
    """the same families where 300 documents are two whole tiles and a part: every tile edge decides a tie, a MUST list misses
    a tile, an exclusion empties one; and one query whose work items do not fit the candidate buffer"""
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process")
    rep = child(VARIANTS_LIB, tmp_path)
    assert rep["tile"] == shapes.SMALL_TILE and not rep["counting"]
    assert rep["past_the_buffer"] == (64 << 20) // 800 + 1


# ---- 2: equivalences ----------------------------------------------------------------------------------------------------
def test_one_role_for_every_ref_is_the_unroled_call():
    covered = shapes.run_same_role_equals_the_unroled_calls()
    assert covered[SHOULD] >= shapes.FLOOR_SAME_ROLE[SHOULD] and covered[MUST] >= shapes.FLOOR_SAME_ROLE[MUST], covered


def test_found_and_small_sets_are_the_boolean_searchs():
    assert shapes.run_equals_the_boolean_search() >= shapes.FLOOR_SMALL_SETS


# ---- 3: the counting build ----------------------------------------------------------------------------------------------
def test_the_directed_inputs_reach_their_paths_in_the_counting_build(tmp_path):
    """every counter of ns_debug_boolean_sets_counters was reached"""
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process")
    rep = child(COUNT_LIB, tmp_path)
    assert rep["tile"] == shapes.SMALL_TILE and rep["counting"]
    assert not rep["missed"], rep
    ev = rep["events"]
    for e in shapes.EVENTS:
        assert ev[e] > 0, (e, ev)
    assert ev["items"] > ev["single_list_items"] > 0


# ---- 4: refusals --------------------------------------------------------------------------------------------------------
def test_refusals():
    shapes.run_refusals()


def test_a_refused_call_between_two_runs_changes_no_byte_of_the_second():
    """ns_facet_count, ns_search_sorted_after, ns_search_boolean_after, ns_facet_count_boolean and ns_search_sorted_boolean share
    one scaffold: after a call that one of them refuses, each answers as before, from the pooled block"""
    shapes.run_refused_between_two_runs()


# ---- 5: the engine ------------------------------------------------------------------------------------------------------
served = bq.served                                   # the boolean engine tests' generated index: three segments, dated documents
QUERIES = ["w001 w002", "+w001 +w002", "w001 w002 -w000", "+w001 w002 -w000", "+rarea w003 -rarec", "rareb -w001", "-w000", "+zzzzqq w001", ""]
DATE = ("2019", "2020-06", True)


@pytest.mark.parametrize("date", [None, DATE], ids=["whole", "dated"])
def test_facets_of_a_boolean_query_are_its_found_year_by_year(served, date):
    eng = served["eng"]
    tables, labels = eng.facet_buckets("year")
    assert labels[0] == "" and labels[1:] == ["2018", "2019", "2020", "2021"]
    hd = eng.open_filter(*date) if date else 0
    try:
        _, _, b_found, b_has = eng.search_boolean_batch(QUERIES, 10, handle=hd)
        counts, found, has = eng.facet_boolean_batch(QUERIES, len(labels), handle=hd)
        np.testing.assert_array_equal(found, b_found)
        np.testing.assert_array_equal(has, b_has)
        assert list(has) == [1, 1, 1, 1, 1, 1, 0, 1, 0]
        np.testing.assert_array_equal(counts.sum(axis=1, dtype=np.uint64), found)
        assert int(np.sum(found >= 2)) >= 5, found                       # the identities below are about something
        for b, year in enumerate(labels):
            # the bucket's documents as a date filter of their own: bucket 0 is what keep_undated adds to an empty range
            if b == 0:
                bounds = ("2030", "2030", True)
            elif date is None or year == "2019":
                bounds = (year, year, False)
            elif year == "2020":
                bounds = ("2020", date[1], False)                        # the year cut by the filter's upper bound
            else:
                bounds = None                                             # outside the filter
            want = np.zeros_like(found)
            if bounds:
                h = eng.open_filter(*bounds)
                try:
                    _, _, want, _ = eng.search_boolean_batch(QUERIES, 10, handle=h)
                finally:
                    eng.close_filter(h)
            np.testing.assert_array_equal(counts[:, b].astype(np.uint64), want, err_msg=str((year, date)))
        assert int(counts[:, 0].sum()) > 0 and int(counts[:, labels.index("2019")].sum()) > 0
    finally:
        if hd:
            eng.close_filter(hd)
    if hd:
        with pytest.raises(RuntimeError, match="stale"):
            eng.facet_boolean_batch(QUERIES, len(labels), handle=hd)


@pytest.mark.parametrize("date", [None, DATE], ids=["whole", "dated"])
def test_date_order_of_a_boolean_query_is_its_matched_set_by_key(served, date):
    eng = served["eng"]
    K = 100
    hd = eng.open_filter(*date) if date else 0
    try:
        b_hits, b_nhits, b_found, b_has = eng.search_boolean_batch(QUERIES, K, handle=hd)
        covered = 0
        for order in ("newest", "oldest"):
            keys_of = eng.sort_keys(order)
            hits, keys, nhits, found, rest, has = eng.search_boolean_sorted_batch(QUERIES, K, order=order, handle=hd)
            np.testing.assert_array_equal(found, b_found)
            np.testing.assert_array_equal(rest, b_found)
            np.testing.assert_array_equal(nhits, b_nhits)
            np.testing.assert_array_equal(has, b_has)
            for q in range(len(QUERIES)):
                n = int(nhits[q])
                assert [int(x) for x in keys[q, :n]] == [int(keys_of[int(h["seg"])][int(h["doc"])]) for h in hits[q, :n]]
                rows = [(int(keys[q, i]), int(hits[q, i]["seg"]), int(hits[q, i]["doc"])) for i in range(n)]
                assert rows == sorted(rows, key=lambda r: (after_rank(r[0], order == "oldest"), r[1], r[2])), (q, order)
                if int(found[q]) <= K:                                   # the whole set: the score-ordered answer's documents and score bits
                    triples = lambda h: sorted((int(x["seg"]), int(x["doc"]), int(x["score"].view(np.uint32))) for x in h[q, :n])  # noqa: E731
                    assert triples(hits) == triples(b_hits), (q, order)
                    covered += int(n >= 2)
        assert covered >= 4, covered
    finally:
        if hd:
            eng.close_filter(hd)


def after_rank(key, ascending):
    """smaller first: a dated document before an undated one, then by the key in the direction"""
    return (1, 0) if key == 0 else (0, key if ascending else -key)


def test_the_json_bodies_are_search_booleans_plus_one_member(served):
    eng = served["eng"]
    try:
        for q, k, date in (("+w001 w002 -w000", 10, None), ("w001 w002", 50, None), ("rareb -w001", 100, None), ("-w000", 5, None), ("", 5, None),
                           ("+w001 w002 -w003", 20, ("2019-06", "2020", False))):
            base = eng.search_boolean_json(q, k, date_filter=date)
            body = eng.search_boolean_faceted_json(q, k, date_filter=date)
            j, jb = json.loads(body), json.loads(base)
            assert list(j)[:2] == ["boolean", "facets"] and body == json.dumps(j, indent=2, sort_keys=True, ensure_ascii=False)
            facets = j.pop("facets")
            assert j == jb and list(facets) == ["year"]
            if date is None:                                                   # the member is the batch call's row: nonzero buckets, in bucket order
                labels = eng.facet_buckets("year")[1]
                counts, _, _ = eng.facet_boolean_batch([q], len(labels))
                assert facets["year"] == [{"count": int(c), "value": labels[b]} for b, c in enumerate(counts[0]) if c]
                assert sum(e["count"] for e in facets["year"]) == (jb.get("found", 0))
            else:
                assert sum(e["count"] for e in facets["year"]) == jb["found"] >= 2 and all("2019" <= e["value"] <= "2020" for e in facets["year"])
            for order in ("newest", "oldest"):
                body = eng.search_boolean_sorted_json(q, k, order=order, date_filter=date)
                j = json.loads(body)
                assert body == json.dumps(j, indent=2, sort_keys=True, ensure_ascii=False)
                assert j.pop("sort") == order
                results, base_results = j.pop("results"), dict(jb).pop("results")
                assert j == {m: v for m, v in jb.items() if m != "results"}
                assert len(results) == len(base_results)
                if jb.get("found", 0) <= k:
                    ident = lambda rs: sorted((e["segment"], e["docId"], e["score"]) for e in rs)      # noqa: E731
                    assert ident(results) == ident(base_results)
                if date is None:
                    hits, _, nhits, _, _, _ = eng.search_boolean_sorted_batch([q], k, order=order)
                    assert [(e["docId"], e["segment"]) for e in results] == [(int(h["doc"]), eng.segment_name(int(h["seg"]))) for h in hits[0, :int(nhits[0])]]
        # all optional words: the members are search_faceted's and search_sorted's
        assert json.loads(eng.search_boolean_faceted_json("w001 w002", 10))["facets"] == json.loads(eng.search_faceted_json("w001 w002", 10))["facets"]
        assert json.loads(eng.search_boolean_sorted_json("w001 w002", 10))["results"] == json.loads(eng.search_sorted_json("w001 w002", 10))["results"]
        for call in (eng.search_boolean_faceted_json, eng.search_boolean_sorted_json):
            bad = call("w000", 3, date_filter=("2019-13", "", False), check=False)
            assert bad.startswith('{\n  "error": "') and "is not YYYY, YYYY-MM or YYYY-MM-DD" in bad
    finally:
        eng.reload()                                                            # closes the cached filters
        eng.set_cache(False)


@pytest.mark.parametrize("order", ["newest", "oldest"])
def test_search_page_walks_a_boolean_query_in_date_order(served, order):
    eng = served["eng"]
    q, k = "+w001 w002 -w000", 7
    whole = json.loads(eng.search_boolean_sorted_json(q, 100, order=order))
    assert 2 * k < whole["found"] <= 100
    cursor, seen, pages = "", [], 0
    while True:
        body = eng.search_page_json(q, k, cursor=cursor, mode="boolean_sorted", order=order)
        j = json.loads(body)
        assert body == json.dumps(j, indent=2, sort_keys=True, ensure_ascii=False)
        assert list(j)[0] == "boolean" and j["sort"] == order and j["found"] == whole["found"] and j["boolean"] == whole["boolean"]
        assert j["page"]["cursor"] == cursor and j["page"]["offset"] == len(seen)
        seen += j["results"]
        assert j["page"]["remaining"] == whole["found"] - len(seen)
        pages += 1
        if "next" not in j["page"]:
            break
        cursor = j["page"]["next"]
        assert cursor.startswith("d") and nsbind.parse_cursor(cursor, "d") is not None
        assert pages < 20
    assert seen == whole["results"] and pages == -(-whole["found"] // k)
    bad = eng.search_page_json(q, k, cursor="s41a3c28f.0.5", mode="boolean_sorted", order=order, check=False)
    assert bad.startswith('{\n  "error": "') and "a cursor of kind 's' does not fit this call, which pages in date order" in bad
    bad = eng.search_page_json(q, k, cursor=cursor or "d0134a3a5.0.5", mode="boolean", check=False)
    assert "a cursor of kind 'd' does not fit this call" in bad
    # the score-ordered boolean mode still pages as before
    j = json.loads(eng.search_page_json(q, k, mode="boolean"))
    assert "sort" not in j and j["page"]["next"].startswith("s")


def test_ns_tool_boolean_faceted_and_sorted(served):
    eng = served["eng"]
    tool = os.path.join(PKG, "ns_tool")
    try:
        want = eng.search_boolean_faceted_json("+w001 w002 -w003", 50)
        out = subprocess.run([tool, "search-boolean-faceted", served["index"], "year", "-", "-", "50", "+w001", "w002", "-w003"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout == want + "\n"
        want = eng.search_boolean_sorted_json("w000 -rarec", 3, order="oldest", date_filter=("", "2019", False))
        out = subprocess.run([tool, "search-boolean-sorted", served["index"], "oldest", "-", "2019", "3", "w000 -rarec"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout == want + "\n", out.stderr
        want = eng.search_page_json("+w001 w002", 5, mode="boolean_sorted", order="newest")
        out = subprocess.run([tool, "page", served["index"], "boolean-newest", "-", "-", "5", "-", "+w001 w002"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout == want + "\n", out.stderr
    finally:
        eng.reload()
        eng.set_cache(False)
