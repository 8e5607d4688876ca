"""Per-document boost factors in ranked boolean search on the GPU (ns_docboost_upload, ns_search_boosted_after: the BOOST
instantiations of k_bq_select in csrc/ns_boolean.hip).

1. The raw C-ABI against the restatement tests/boost_ref.py on the directed inputs of tests/boost_shapes.py: in this process on
   the product library (one tile and one window hold a 300-document segment; a family of a product tile + 37 documents puts
   matched documents at 8191 | 8192 and 131071 | 131072), and in ONE child process on the variants build with tiles of 128 and
   windows of 32 documents.
2. Exact equivalences on the same raw inputs: boosts == NULL == ns_search_quorum_after, an all-1.0f table == it through the
   boosted kernels: hits, nhits, found and rest, byte for byte, for the four dialect forms.
3. A child on the counting build asserts that the inputs reach every counter of the boosted sweep and that the three BOOST
   instantiations are the ones that ran.
4. Refusals.
5. The engine: decay tables, term weights, JSON bodies, pages, ns_tool, the table cache.
Every comparison is exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import boost_ref
import boost_shapes as shapes
import nsbind
import test_boolean_gpu as bq
from conftest import PKG, VARIANTS_LIB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_LIB = os.path.join(PKG, "libnextsearch_hip_count.so")
# A child loads a library, creates a context and runs the small families: a few seconds of work, 60 s for a shared device.
CHILD_TIMEOUT_S = 60
IN_TEST_BUILD = os.path.basename(os.environ.get("NS_HIP_LIB", "")) not in ("", "libnextsearch_hip.so")


# ---- 1: the raw ABI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_segs", [1, 3])
def test_directed_cases_equal_the_restatement(n_segs):
    """inverted ranking, all-zero factors, zero against negative, product ties, edges, K = 1, 64, 65, 100 with more than K matched,
    three segments with different tables: every case under every table (here: whatever tile and window the loaded library has)"""
    shapes.run_directed(n_segs)


def test_each_dialect_form_under_a_table():
    shapes.run_dialects()


def test_cursors_on_absent_ranks_on_tie_runs_and_behind_the_last_document():
    shapes.run_cursors()


def test_pages_of_three_walk_the_whole_boosted_ranking():
    pages = shapes.run_walks()
    assert pages["3"] >= 20 and pages["1"] == 34 and pages["100"] == 10, pages


def test_under_a_filtered_copy_of_a_segment():
    shapes.run_filter()


def test_documents_at_the_edges_of_a_product_window_and_tile():
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process: the family is built for the product's tile")
    tile, n = shapes.run_product_tile()
    assert tile == 1 << 17 and n == (1 << 17) + 37


def child(lib, tmp_path):
    assert os.path.exists(lib), os.path.basename(lib) + " is missing: make -C nextsearch-api_amd all"
    out = str(tmp_path / "boost.json")
    env = dict(os.environ, NS_HIP_LIB=lib, NS_FACET_TILE_DOCS=str(shapes.SMALL_TILE), NS_BOOL_WIN_DOCS=str(shapes.SMALL_WIN))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "boost_shapes.py"), out], env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "boost shapes OK" in r.stdout, tail
    with open(out) as f:
        return json.load(f)


def test_tiles_of_128_and_windows_of_32_documents_in_the_variants_build(tmp_path):
    """the same families where 300 documents are two whole tiles and a part, four windows each: matched documents on both sides of
    every window and tile edge, more than K matched documents per item; then the walks, the cursors, the dialects, the filter and
    the equivalences at that size"""
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process")
    rep = child(VARIANTS_LIB, tmp_path)
    assert rep["tile"] == shapes.SMALL_TILE and not rep["counting"]
    assert rep["ones"] >= 8 and rep["pages"]["3"] >= 20


# ---- 2: equivalences ----------------------------------------------------------------------------------------------------
def test_without_tables_and_under_tables_of_ones_the_call_is_its_sibling():
    assert shapes.run_null_and_ones_are_the_sibling() >= 8


# ---- 3: the counting build ----------------------------------------------------------------------------------------------
def test_the_directed_inputs_reach_the_boosted_sweep_in_the_counting_build(tmp_path):
    """every counter of ns_debug_boolean_boost_counters was reached; every work item of k_bq_select ran a BOOST instantiation, and
    each of the three did"""
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process")
    rep = child(COUNT_LIB, tmp_path)
    assert rep["tile"] == shapes.SMALL_TILE and rep["counting"]
    d, c, f = rep["events_directed"], rep["events_cursors"], rep["events_dialects"]
    for ev in (d, c, f):
        assert ev["items"] == ev["select_items"] > 0, ev                      # no unboosted instantiation of the kernel ran
        assert ev["items"] == ev["items_boolean"] + ev["items_grouped"] + ev["items_quorum"] and 0 < ev["items_swept"] <= ev["items"], ev
        assert ev["documents_multiplied"] > ev["items_swept"], ev
    assert d["items_quorum"] == d["items"] and d["keys_clipped"] == 0 and d["windows_all_zero"] > 0, d      # needs given: the quorum form; no cursor
    assert c["keys_clipped"] > 0, c
    assert f["items_boolean"] > 0 and f["items_grouped"] > 0 and f["items_quorum"] == 0, f                  # roles / clauses / needs NULL


# ---- 4: refusals --------------------------------------------------------------------------------------------------------
def test_refusals():
    shapes.run_refusals()


# ---- 5: the engine ------------------------------------------------------------------------------------------------------
served = bq.served                                   # the boolean engine tests' generated index: three segments, dated documents

# 38, 18, 18 and 35 matched documents (few enough to see a whole ranking in one page of 100), several hundred, none, and no term
QUERIES = ["+(w001 w002 w003)~2 -w000 w004", "+(w001 w002 w003)~3 -w000 w004", "+w003 +w004 -w000 w001", "+rareb w001 w002", "w001 w002 w003 ~2", "+(w001 zzzzqq)~2", ""]
DECAY = dict(kind="exponential", weight=0.8, origin="2021-06-15", scale_days=200.0, offset_days=30.0, undated=0.1)


def boosted_want(eng, queries, tables, k=100):
    """the boosted ranking of queries that match at most 100 documents: the quorum call's whole answer (the engine's own unboosted
    scores), one np.float32 multiply per document, boost_ref's order -> per query [(seg, doc, product bits)] or None (too many)"""
    hits, nhits, found, rest, has = eng.search_quorum_after_batch(queries, 100)
    out = []
    for q in range(len(queries)):
        if not has[q] or int(found[q]) > 100:
            out.append(None if has[q] else [])
            continue
        everything = [[(h["score"], int(h["seg"]), int(h["doc"])) for h in hits[q, :int(nhits[q])]]]
        rows = boost_ref.boosted_rows(everything, tables, [0, 1, 2])[0]
        out.append([(r[3], r[2], r[4]) for r in rows][:k])
    return out


def got_rows(hits, nhits, q):
    return [(int(h["seg"]), int(h["doc"]), int(h["score"].view(np.uint32))) for h in hits[q, :int(nhits[q])]]


def test_weight_zero_and_no_spec_are_the_quorum_engine_call(served):
    eng = served["eng"]
    try:
        for k in (10, 100):
            want = eng.search_quorum_after_batch(QUERIES, k)
            for boost in (None, dict(kind="exponential", weight=0.0, scale_days=30.0, undated=0.0), dict(kind="linear", weight=0.0, origin="2019")):
                got = eng.search_boosted_after_batch(QUERIES, k, boost=boost)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), (k, boost)
        assert int(want[2][0]) >= 9 and int(want[2][4]) > 100 and list(want[4]) == [1, 1, 1, 1, 1, 1, 0]
        table = np.concatenate(eng.boost_table(dict(kind="linear", weight=0.0)))
        assert table.tobytes() == np.ones(len(table), np.float32).tobytes()
    finally:
        eng.release_boosts()


def test_a_custom_table_and_the_decays_rank_by_the_product(served):
    """the engine's hits under a custom table, an exponential and a linear decay against boost_ref over the engine's own table
    (nsh_engine_boost_table) and its own unboosted scores: (segment, docId, product bits), exactly"""
    eng = served["eng"]
    sizes = [eng.segment_info(s)["n_docs"] for s in range(3)]
    custom = [(((np.arange(n) * 5 + s) % 9) / 2.0).astype(np.float32) for s, n in enumerate(sizes)]          # 0 .. 4 in halves, zeros among them
    try:
        changed = 0
        for boost in (dict(kind="custom", custom=custom), DECAY, dict(kind="linear", weight=1.0, origin="", scale_days=900.0, undated=0.0)):
            tables = eng.boost_table(boost)
            if boost["kind"] == "custom":
                assert all(a.tobytes() == b.tobytes() for a, b in zip(tables, custom))
            else:
                flat = np.concatenate(tables)
                assert len(set(flat.tolist())) > 10 and flat.min() >= 0.0 and np.all(np.isfinite(flat))
            want = boosted_want(eng, QUERIES, tables)
            plain = eng.search_quorum_after_batch(QUERIES, 100)
            for k in (3, 100):
                hits, nhits, found, rest, has = eng.search_boosted_after_batch(QUERIES, k, boost=boost)
                assert found.tobytes() == plain[2].tobytes() and rest.tobytes() == found.tobytes() and has.tobytes() == plain[4].tobytes()
                for q in range(len(QUERIES)):
                    if want[q] is not None:
                        assert got_rows(hits, nhits, q) == want[q][:k], (boost["kind"], k, QUERIES[q])
            changed += sum(want[q] is not None and [r[:2] for r in want[q]] != [r[:2] for r in got_rows(plain[0], plain[1], q)] for q in range(len(QUERIES)))
            assert eng.boost_tables_on_device() == 3
        assert changed >= 6 and sum(w is not None and len(w) >= 5 for w in want) >= 3      # the rankings really change, and there is something to rank
    finally:
        eng.release_boosts()


def test_a_term_weight_is_the_qweight_of_its_terms(served):
    eng = served["eng"]
    one = eng.search_boosted_after_batch(["w001", "+(w001 w002)", "w001 w002"], 100)
    two = eng.search_boosted_after_batch(["w001^2", "+(w001 w002)^4", "w001^0.5 w002^0.5"], 100)
    for q, factor in enumerate((2.0, 4.0, 0.5)):                                 # a power of two scales every addend and every rounding alike
        n = int(one[1][q])
        assert n >= 5 and int(two[1][q]) == n and int(two[2][q]) == int(one[2][q])
        assert two[0][q, :n]["doc"].tobytes() == one[0][q, :n]["doc"].tobytes() and two[0][q, :n]["seg"].tobytes() == one[0][q, :n]["seg"].tobytes()
        assert (one[0][q, :n]["score"] * np.float32(factor)).tobytes() == two[0][q, :n]["score"].tobytes()
    # a weight changes the ranking where it should: w004's documents rise
    a = eng.search_boosted_after_batch(["w003 w004"], 100)
    b = eng.search_boosted_after_batch(["w003 w004^50"], 100)
    assert int(a[2][0]) == int(b[2][0]) and got_rows(a[0], a[1], 0) != got_rows(b[0], b[1], 0)
    top = [(int(h["seg"]), int(h["doc"])) for h in b[0][0, :3]]
    assert all("w004" in served["sets"][s][d] for s, d in top)
    # and a text without a weight is the quorum call
    assert all(x.tobytes() == y.tobytes() for x, y in zip(eng.search_boosted_after_batch(QUERIES, 10), eng.search_quorum_after_batch(QUERIES, 10)))


def test_the_json_body_is_the_quorum_body_with_boosted_and_boost(served):
    eng = served["eng"]
    try:
        q = "+(w001 W002 w003)~2^1.5 +w004^2 -(w000 rarec)^3 rareb^0.25 w005 ~1"
        body = eng.search_boosted_json(q, 10, boost=DECAY)
        j = json.loads(body)
        assert body == json.dumps(j, indent=2, sort_keys=True, ensure_ascii=False)            # keys sorted, dump(2) layout
        assert j["boost"] == {"kind": "exponential", "offset_days": 30.0, "origin": "2021-06-15", "scale_days": 200.0, "undated": 0.1, "weight": 0.8}
        assert j["boosted"] == {"min_should": 1, "must": [{"need": 2, "terms": ["w001", "w002", "w003"], "weight": 1.5}, {"need": 1, "terms": ["w004"], "weight": 2.0}],
                                "must_not": ["w000", "rarec"], "should": [{"term": "rareb", "weight": 0.25}, {"term": "w005", "weight": 1.0}]}
        assert list(j)[:2] == ["boost", "boosted"] and "quorum" not in j
        hits, nhits, found, _, has = eng.search_boosted_after_batch([q], 10, boost=DECAY)
        assert j["found"] == int(found[0]) and [(e["docId"], e["segment"]) for e in j["results"]] == [(int(h["doc"]), eng.segment_name(int(h["seg"]))) for h in hits[0, :int(nhits[0])]]
        # a text without a weight and no spec: the quorum body but for the member's name and the entries' form
        plain = "+(w001 w002 w003)~2 -w000 w004"
        jb, jq = json.loads(eng.search_boosted_json(plain, 20)), json.loads(eng.search_quorum_json(plain, 20))
        assert "boost" not in jb
        member, quorum = jb.pop("boosted"), jq.pop("quorum")
        assert jb == jq and jb["found"] >= 9
        assert member["min_should"] == quorum["min_should"] and member["must_not"] == quorum["must_not"]
        assert [{m: c[m] for m in ("need", "terms")} for c in member["must"]] == quorum["must"] and all(c["weight"] == 1.0 for c in member["must"])
        assert [e["term"] for e in member["should"]] == quorum["should"]
        # under a date filter: "boost" < "boosted" < "filter"
        body = eng.search_boosted_json(plain, 20, boost=dict(kind="linear", scale_days=500.0), date_filter=("2019", "2020-06", True))
        j = json.loads(body)
        assert body == json.dumps(j, indent=2, sort_keys=True, ensure_ascii=False) and list(j)[:3] == ["boost", "boosted", "filter"]
        assert j["boost"]["kind"] == "linear" and j["boost"]["origin"] == ""
        bad = eng.search_boosted_json(plain, 5, boost=dict(kind="linear", scale_days=0.0), check=False)
        assert bad.startswith('{\n  "error": "') and "scale_days must be above 0" in bad
        bad = eng.search_boosted_json("+(w001 w002)~8", 5, check=False)
        assert bad.startswith('{\n  "error": "') and "asks for 8 of a clause's terms (at most 7)" in bad
    finally:
        eng.reload()                                                            # closes the cached filters
        eng.set_cache(False)


def test_search_page_walks_a_boosted_query(served):
    """pages of 4 concatenate to the full boosted ranking; cursors of kind 's' over the product bits"""
    eng = served["eng"]
    q, k = "+(w001 w002 w003)~2 -w000 w004^3", 4
    try:
        for boost in (DECAY, None):
            whole = json.loads(eng.search_boosted_json(q, 100, boost=boost))
            assert 2 * k < whole["found"] <= 100
            cursor, seen, pages = "", [], 0
            while True:
                body = eng.search_boosted_page_json(q, k, cursor=cursor, boost=boost) if boost else eng.search_page_json(q, k, cursor=cursor, mode="boosted")
                j = json.loads(body)
                assert body == json.dumps(j, indent=2, sort_keys=True, ensure_ascii=False)
                assert j["boosted"] == whole["boosted"] and j.get("boost") == whole.get("boost") and j["found"] == whole["found"] and "quorum" not in j
                assert j["page"]["cursor"] == cursor and j["page"]["offset"] == len(seen)
                seen += j["results"]
                assert j["page"]["remaining"] == whole["found"] - len(seen)
                pages += 1
                if "next" not in j["page"]:
                    break
                cursor = j["page"]["next"]
                assert cursor.startswith("s") and nsbind.parse_cursor(cursor, "s") is not None
                assert pages < 40
            assert seen == whole["results"] and pages == -(-whole["found"] // k)
        assert json.loads(eng.search_boosted_json(q, 100, boost=DECAY))["results"] != json.loads(eng.search_boosted_json(q, 100))["results"]
        bad = eng.search_boosted_page_json(q, k, cursor="d0134a3a5.0.5", boost=DECAY, check=False)
        assert bad.startswith('{\n  "error": "') and "does not fit this call" in bad
    finally:
        eng.release_boosts()


def test_ns_tool_search_boosted(served):
    eng = served["eng"]
    tool = os.path.join(PKG, "ns_tool")
    try:
        def run(*args):
            out = subprocess.run([tool] + list(args), capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stderr
            return out.stdout

        q = "+(w001 w002 w003)~2^1.5 -w000 w004^3"
        assert run("search-boosted", served["index"], "exponential", "0.8", "200", "30", "2021-06-15", "-", "-", "20", "+(w001", "w002", "w003)~2^1.5", "-w000", "w004^3") == \
            eng.search_boosted_json(q, 20, boost=dict(kind="exponential", weight=0.8, origin="2021-06-15", scale_days=200.0, offset_days=30.0, undated=1.0)) + "\n"
        assert run("search-boosted", served["index"], "linear", "1", "700", "0", "-", "-", "2020", "5", q) == \
            eng.search_boosted_json(q, 5, boost=dict(kind="linear", weight=1.0, scale_days=700.0), date_filter=("", "2020", False)) + "\n"
        assert run("search-boosted", served["index"], "none", "0", "0", "0", "-", "-", "-", "7", q) == eng.search_boosted_json(q, 7) + "\n"
    finally:
        eng.reload()
        eng.set_cache(False)


def test_the_table_cache_and_its_release_on_reload(served):
    eng = served["eng"]
    try:
        eng.release_boosts()
        assert eng.boost_tables_on_device() == 0
        eng.search_boosted_after_batch(["w001^2"], 5)                           # term weights alone need no table
        assert eng.boost_tables_on_device() == 0
        eng.boost_table(DECAY)                                                  # host only
        assert eng.boost_tables_on_device() == 0
        a = eng.search_boosted_after_batch(QUERIES, 10, boost=DECAY)
        assert eng.boost_tables_on_device() == 3
        b = eng.search_boosted_after_batch(QUERIES, 10, boost=dict(DECAY))
        assert eng.boost_tables_on_device() == 3 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        c = eng.search_boosted_after_batch(QUERIES, 10, boost=dict(DECAY, scale_days=20.0))     # another spec takes the set's place
        assert eng.boost_tables_on_device() == 3 and c[0].tobytes() != a[0].tobytes()
        eng.release_boosts()
        assert eng.boost_tables_on_device() == 0
        d = eng.search_boosted_after_batch(QUERIES, 10, boost=DECAY)
        assert eng.boost_tables_on_device() == 3 and all(x.tobytes() == y.tobytes() for x, y in zip(a, d))
        # under an open filter the same tables serve the filter's copies
        handle = eng.open_filter("2019", "2020", False)
        f = eng.search_boosted_after_batch(QUERIES, 100, boost=DECAY, handle=handle)
        g = eng.search_quorum_after_batch(QUERIES, 100, handle=handle)
        assert f[2].tobytes() == g[2].tobytes() and 0 < int(f[2][0]) < int(a[2][0]) and eng.boost_tables_on_device() == 3
        tables = eng.boost_table(DECAY)
        for q in range(len(QUERIES)):                                           # the filter's copies keep the docIds: the same factors
            if int(g[2][q]) <= 100 and g[4][q]:
                rows = boost_ref.boosted_rows([[(h["score"], int(h["seg"]), int(h["doc"])) for h in g[0][q, :int(g[1][q])]]], tables, [0, 1, 2])[0]
                assert got_rows(f[0], f[1], q) == [(r[3], r[2], r[4]) for r in rows], QUERIES[q]
        eng.close_filter(handle)
        with pytest.raises(RuntimeError, match="search_boosted_after_batch_flat: boost: weight .* is outside \\[0, 1\\]"):
            eng.search_boosted_after_batch(QUERIES, 10, boost=dict(DECAY, weight=2.0))
        eng.reload()
        assert eng.boost_tables_on_device() == 0
    finally:
        eng.reload()
        eng.set_cache(False)
