"""Prefix terms on the device (host/prefix.hpp, Engine::search_prefixed_after_batch_flat over ns_segment_union),
against a REWRITTEN CORPUS: engine A holds small texts in three segments, two of them the same texts, so scores tie across
segments; engine B holds the same texts with every word under a prefix replaced, token for token, by one word that occurs nowhere
else.  Document lengths, N and avgdl are then equal, and B's list of that word IS the blended term: the union of the expansions'
lists, the tf summed, the df its size.  A's prefixed answers must equal B's boosted answers in docIds, ranks, found, rest and
score bits."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nsbind
from test_compact_gpu import new_engine

pytestmark = pytest.mark.gpu

# the words under each prefix, and the one word B holds in their place
FAMILIES = {
    "vaccin": ["vaccine", "vaccines", "vaccination", "vaccinated"],
    "immun": ["immune", "immunity", "immunization"],
    "vir": ["virus", "viral", "virology"],
    "dose": ["dose", "doses", "dosed"],                    # the prefix equals a whole term
    "hamst": ["hamster", "hamsters"],                      # in segments 0 and 1 only
}
ONE_WORD = {p: "q" + p + "q" for p in FAMILIES}
PLAIN = ["safety", "mouse", "trial", "efficacy", "cohort"] + ["w%02d" % i for i in range(30)]
K_PAGE = 3
DECAY = dict(kind="exponential", weight=0.8, origin="2021-06-15", scale_days=200.0, offset_days=30.0, undated=0.1)

# (A's text, B's text); each prefix has at least two expansions in a segment
CASES = [
    ("vaccin*", "qvaccinq"),
    ("+vaccin* safety -mouse", "+qvaccinq safety -mouse"),
    ("-vaccin* safety", "-qvaccinq safety"),
    ("+(vaccin* immun*)~1 trial^2", "+(qvaccinq qimmunq)~1 trial^2"),
    ("vir*^0.5 vir*", "qvirq^0.5 qvirq"),
    ("dose*", "qdoseq"),                                   # a prefix that equals a whole term
    ("hamst* efficacy", "qhamstq efficacy"),               # a prefix absent from segment 2
    ("+hamst* safety", "+qhamstq safety"),                 # ... as a required term: a zero-count ref there
    ("+(vaccin* dose* mouse)~2 -hamst* cohort^0.25 vir* ~1", "+(qvaccinq qdoseq mouse)~2 -qhamstq cohort^0.25 qvirq ~1"),
    ("VACCIN* Immun*, vir*", "qvaccinq qimmunq qvirq"),
    ("safety trial", "safety trial"),                      # no prefix in a batch that has some
]
A_TEXTS, B_TEXTS = [a for a, _ in CASES], [b for _, b in CASES]


def make_texts(seg, n, seed, with_hamsters):
    rng = np.random.default_rng(seed)
    words = PLAIN + [w for p, ws in FAMILIES.items() for w in ws if with_hamsters or p != "hamst"]
    p = 1.0 / (np.arange(len(words)) % 17 + 2.0)
    p /= p.sum()
    return [[words[j] for j in rng.choice(len(words), int(rng.integers(6, 30)), p=p)] for _ in range(n)]


def as_docs(seg, texts, rewrite=None):
    out = []
    for i, words in enumerate(texts):
        text = " ".join(rewrite.get(w, w) for w in words) if rewrite else " ".join(words)
        out.append((b"s%dd%04d" % (seg, i), b"Title %d" % i, b"pdf_json/%d_%d.json" % (seg, i), text.encode()))
    return out


def write_metadata(index, batches):
    lines = ["cord_uid,title,publish_time,authors,url"]
    for s, b in enumerate(batches):
        for i, d in enumerate(b):
            t = ["%04d-%02d-%02d" % (2019 + (i + s) % 3, 1 + i % 12, 1 + i % 28), "2021-%02d" % (1 + i % 12), "2020", ""][i % 4]
            lines.append("%s,T,%s,A B,http://x" % (d[0].decode(), t))
    with open(os.path.join(index, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")


def make_engine(tmp, name, texts, rewrite):
    index = str(tmp / name)
    batches = [as_docs(s, t, rewrite) for s, t in enumerate(texts)]
    eng = new_engine(index, batches)
    write_metadata(index, batches)
    eng.reload()
    eng.set_cache(False)
    return eng


@pytest.fixture(scope="module")
def corpora(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("prefix_gpu")
    same = make_texts(0, 220, 1, True)
    texts = [same, same, make_texts(2, 170, 2, False)]
    a = make_engine(tmp, "a", texts, None)
    b = make_engine(tmp, "b", texts, {w: ONE_WORD[p] for p, ws in FAMILIES.items() for w in ws})
    assert a.num_segments == b.num_segments == 3
    for s in range(3):
        ia, ib = a.segment_info(s), b.segment_info(s)
        assert ia["n_docs"] == ib["n_docs"] and ia["avgdl"] == ib["avgdl"] and np.array_equal(a.segment_doc_len(s), b.segment_doc_len(s))
    yield {"a": a, "b": b, "texts": texts, "tmp": tmp}
    a.close()
    b.close()


def same(label, got, want):
    """hits (doc, seg, score bits), nhits, found, rest, has_found of two calls"""
    for name, x, y in zip(("hits", "nhits", "found", "rest", "has_found"), got, want):
        if name == "hits":
            for f in ("doc", "seg"):
                assert np.array_equal(x[f], y[f]), (label, f)
            assert np.array_equal(x["score"].view(np.uint32), y["score"].view(np.uint32)), (label, "score bits")
        else:
            assert np.array_equal(x, y), (label, name, x, y)


def expansions_per_segment(eng, prefix, max_expansions=0):
    terms, _ = eng.expand_prefix(prefix, max_expansions)
    return [sum(1 for t in terms if (eng.lookup(s, t) or {"df": 0})["df"] > 0) for s in range(eng.num_segments)]


def test_every_prefix_has_what_its_case_needs(corpora):
    """the condition against an empty test: from "prefixes", every prefix of every case has at least two expansions, and at least
    two of them hold a list in one segment; `hamst` holds none in segment 2"""
    a = corpora["a"]
    seen = set()
    for text in A_TEXTS:
        j = json.loads(a.search_prefixed_json(text, 5))
        for e in j["prefixes"]:
            assert e["expansions"] == len(FAMILIES[e["prefix"]]) >= 2 and e["truncated"] is False, (text, e)
            per_seg = expansions_per_segment(a, e["prefix"])
            assert max(per_seg) >= 2, (text, e, per_seg)
            seen.add(e["prefix"])
    assert seen == set(FAMILIES)
    assert expansions_per_segment(a, "hamst") == [2, 2, 0] and expansions_per_segment(a, "dose") == [3, 3, 3]
    assert a.expand_prefix("dose")[0] == ["dose", "dosed", "doses"]


@pytest.mark.parametrize("k", [1, 10, 100])
def test_prefixed_on_a_equals_boosted_on_b(corpora, k):
    a, b = corpora["a"], corpora["b"]
    got = a.search_prefixed_after_batch(A_TEXTS, k)
    want = b.search_boosted_after_batch(B_TEXTS, k)
    same(("batch", k), got, want)
    assert all(int(f) > 0 for f in want[2]) and list(want[4]) == [1] * len(CASES)
    for i, (ta, tb) in enumerate(CASES):                                        # and query by query: a batch of one makes its own derived segments
        same((ta, k), a.search_prefixed_after_batch([ta], k), tuple(x[i:i + 1] for x in want))
    if k == 100:
        segs = {int(s) for s in want[0][0, :int(want[1][0])]["seg"]}
        assert {0, 1} <= segs                                                   # ties across the two equal segments
        hamster = want[0][7, :int(want[1][7])]
        assert len(hamster) and 2 not in set(hamster["seg"].tolist())           # the required prefix is absent from segment 2


def test_a_one_expansion_prefix_is_the_plain_term(corpora):
    a = corpora["a"]
    assert a.expand_prefix("safet") == (["safety"], False) and a.expand_prefix("vaccinat") == (["vaccinated", "vaccination"], False)
    one = ["safet*", "+safet* vaccine -mous*", "trial* ~1", "hamsters*^2 w01"]
    plain = ["safety", "+safety vaccine -mouse", "trial ~1", "hamsters^2 w01"]
    for k in (10, 100):
        got = a.search_prefixed_after_batch(one, k)
        same(("one expansion", k), got, a.search_boosted_after_batch(plain, k))
        assert all(int(f) > 0 for f in got[2])


def test_a_prefix_without_a_match_answers_as_an_unknown_word(corpora):
    a = corpora["a"]
    assert a.expand_prefix("zzq") == ([], False)
    got = a.search_prefixed_after_batch(["zzq*", "zzq* safety", "+zzq* safety", "-zzq* safety", "+(zzq* vaccin*)~1"], 10)
    want = a.search_boosted_after_batch(["zzqzz", "zzqzz safety", "+zzqzz safety", "-zzqzz safety", "+(zzqzz vaccine)~1"], 10)
    same("no match", tuple(g[:4] for g in got), tuple(w[:4] for w in want))
    assert list(got[2][:4]) == [0, int(want[2][1]), 0, int(want[2][3])] and int(got[2][1]) > 0
    assert int(got[2][4]) > int(want[2][4]) > 0                                  # the group keeps its other member, which is a union


def test_max_expansions_keeps_the_best_two(corpora):
    a, texts = corpora["a"], corpora["texts"]
    kept, truncated = a.expand_prefix("vaccin", 2)
    sums = {w: sum((a.lookup(s, w) or {"df": 0})["df"] for s in range(3)) for w in FAMILIES["vaccin"]}
    assert truncated and kept == sorted(sorted(sums, key=lambda w: (-sums[w], w))[:2]) and len(set(sums.values())) >= 2
    b2 = make_engine(corpora["tmp"], "b2", texts, {w: "qvaccinq" for w in kept})
    try:
        for k in (10, 100):
            got = a.search_prefixed_after_batch(["vaccin*", "+vaccin* safety", "vaccin* safety^2"], k, max_expansions=2)
            same(("two kept", k), got, b2.search_boosted_after_batch(["qvaccinq", "+qvaccinq safety", "qvaccinq safety^2"], k))
        full = a.search_prefixed_after_batch(["vaccin*"], 10)
        assert int(full[2][0]) > int(got[2][0]) > 0
        j = json.loads(a.search_prefixed_json("vaccin*", 5, max_expansions=2))
        assert j["prefixes"] == [{"expansions": 2, "prefix": "vaccin", "truncated": True}]
        with pytest.raises(RuntimeError, match="max_expansions 65536 is outside"):
            a.search_prefixed_after_batch(["vaccin*"], 5, max_expansions=65536)
    finally:
        b2.close()


def test_pages_of_three_equal_the_first_thirty(corpora):
    a, b = corpora["a"], corpora["b"]
    whole = a.search_prefixed_after_batch(A_TEXTS, 100)
    Q = len(A_TEXTS)
    after, seen = [None] * Q, [[] for _ in range(Q)]
    for page in range(10):
        hits, nhits, found, rest, has = a.search_prefixed_after_batch(A_TEXTS, K_PAGE, after=after)
        w_hits, w_nhits, _, w_rest, _ = b.search_boosted_after_batch(B_TEXTS, K_PAGE, after=after)
        assert np.array_equal(found, whole[2]) and np.array_equal(rest, w_rest) and np.array_equal(nhits, w_nhits)
        for q in range(Q):
            n = int(nhits[q])
            assert int(rest[q]) == max(int(found[q]) - len(seen[q]), 0)
            rows = [(int(h["seg"]), int(h["doc"]), int(h["score"].view(np.uint32))) for h in hits[q, :n]]
            assert rows == [(int(h["seg"]), int(h["doc"]), int(h["score"].view(np.uint32))) for h in w_hits[q, :n]]
            seen[q] += rows
            after[q] = (rows[-1][2], rows[-1][0], rows[-1][1]) if n else after[q]
    for q in range(Q):
        want = [(int(h["seg"]), int(h["doc"]), int(h["score"].view(np.uint32))) for h in whole[0][q, :min(int(whole[1][q]), 30)]]
        assert seen[q][:30] == want and len(want) == min(int(whole[2][q]), 30), A_TEXTS[q]
    assert sum(len(s) == 30 for s in seen) >= 6


def test_a_decay_passes_through(corpora):
    a, b = corpora["a"], corpora["b"]
    try:
        for k in (10, 100):
            got = a.search_prefixed_after_batch(A_TEXTS, k, boost=DECAY)
            same(("decay", k), got, b.search_boosted_after_batch(B_TEXTS, k, boost=DECAY))
        plain = a.search_prefixed_after_batch(A_TEXTS, 100)
        assert np.array_equal(got[2], plain[2]) and got[0].tobytes() != plain[0].tobytes()
        assert a.boost_tables_on_device() == 3
    finally:
        a.release_boosts()
        b.release_boosts()


def test_the_json_bodies(corpora):
    a, b = corpora["a"], corpora["b"]
    try:
        q = "+(vaccin* immun*)~1 trial^2 -hamst* vir*^0.5 vaccin*"
        body = a.search_prefixed_json(q, 10, boost=DECAY)
        j = json.loads(body)
        assert body == json.dumps(j, indent=2, sort_keys=True, ensure_ascii=False)            # keys sorted, dump(2) layout
        assert j["prefixes"] == [{"expansions": 4, "prefix": "vaccin", "truncated": False}, {"expansions": 3, "prefix": "immun", "truncated": False},
                                 {"expansions": 2, "prefix": "hamst", "truncated": False}, {"expansions": 3, "prefix": "vir", "truncated": False}]
        assert j["prefixed"] == {"min_should": 0, "must": [{"need": 1, "terms": ["vaccin*", "immun*"], "weight": 1.0}], "must_not": ["hamst*"],
                                 "should": [{"term": "trial", "weight": 2.0}, {"term": "vir*", "weight": 0.5}, {"term": "vaccin*", "weight": 1.0}]}
        assert j["boost"]["kind"] == "exponential" and "boosted" not in j and "filter" not in j
        hits, nhits, found, _, has = a.search_prefixed_after_batch([q], 10, boost=DECAY)
        assert j["found"] == int(found[0]) > 0
        assert [(e["docId"], e["segment"]) for e in j["results"]] == [(int(h["doc"]), a.segment_name(int(h["seg"]))) for h in hits[0, :int(nhits[0])]]
        # but for the two members (and the segment names), B's boosted body
        ja, jb = json.loads(a.search_prefixed_json("vaccin* safety", 20)), json.loads(b.search_boosted_json("qvaccinq safety", 20))
        assert ja["prefixes"] == [{"expansions": 4, "prefix": "vaccin", "truncated": False}] and ja["found"] == jb["found"] > 20
        assert [(e["docId"], e["score"]) for e in ja["results"]] == [(e["docId"], e["score"]) for e in jb["results"]]
        # a text without a prefix: the boosted body with the member renamed and an empty list
        jp, jq = json.loads(a.search_prefixed_json("+safety trial^2", 10)), json.loads(a.search_boosted_json("+safety trial^2", 10))
        assert jp.pop("prefixes") == [] and jp.pop("prefixed") == jq.pop("boosted") and jp == jq
        # pages
        whole = json.loads(a.search_prefixed_json(q, 100, boost=DECAY))
        cursor, seen, pages = "", [], 0
        while pages < 12:
            body = a.search_prefixed_page_json(q, K_PAGE, cursor=cursor, boost=DECAY)
            p = json.loads(body)
            assert body == json.dumps(p, indent=2, sort_keys=True, ensure_ascii=False)
            assert p["prefixes"] == whole["prefixes"] and p["prefixed"] == whole["prefixed"] and p["found"] == whole["found"]
            assert p["page"]["cursor"] == cursor and p["page"]["offset"] == len(seen)
            seen += p["results"]
            pages += 1
            if "next" not in p["page"]:
                break
            cursor = p["page"]["next"]
            assert cursor.startswith("s")
        assert pages >= 4 and seen == whole["results"][:len(seen)]
        bad = a.search_prefixed_page_json(q, K_PAGE, cursor="d0134a3a5.0.5", check=False)
        assert bad.startswith('{\n  "error": "') and "does not fit this call" in bad
    finally:
        a.release_boosts()


def test_a_filter_is_refused_and_no_derived_segment_stays(corpora):
    a = corpora["a"]
    handle = a.open_filter("2019", "2020", False)
    try:
        with pytest.raises(RuntimeError, match="search_prefixed_after_batch_flat: a filter is refused"):
            a.search_prefixed_after_batch(["vaccin*"], 5, handle=handle)
        with pytest.raises(RuntimeError, match="a filter is refused"):
            a.search_prefixed_after_batch(["safety"], 5, handle=handle)             # with or without a prefix
    finally:
        a.close_filter(handle)
    for body in (a.search_prefixed_json("vaccin*", 5, date_filter=("2019", "2020", False), check=False),
                 a.search_prefixed_page_json("vaccin*", 5, date_filter=("2019", "2020", False), check=False)):
        assert body.startswith('{\n  "error": "') and "a filter is refused" in body
    bad = a.search_prefixed_json("+(vaccin* immun*)~8", 5, check=False)
    assert bad.startswith('{\n  "error": "') and "asks for 8 of a clause's terms (at most 7)" in bad   # a failure behind the unions releases them too
    a.reload()                                                                       # closes the filter search_filtered cached
    a.set_cache(False)
    a.search_prefixed_after_batch(A_TEXTS, 10)
    # the derived ids, above the eight filters' ranges, are free again: they can be uploaded
    L, ctx = nsbind.hip_lib(), a.ctx
    dl = np.ones(4, np.uint32)
    payload = np.array([0, 1, 2, 1], np.uint32)
    for sid in range(9 * 3, 10 * 3):
        h = C.c_void_p()
        assert L.ns_segment_upload(ctx, sid, 4, C.c_float(1.0), dl.ctypes.data, payload.ctypes.data, payload.nbytes, C.byref(h)) == 0, L.ns_last_error(ctx)
        assert L.ns_segment_release(ctx, h) == 0
