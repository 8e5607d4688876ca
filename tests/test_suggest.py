"""Autocomplete: Engine::suggest (src/api_engine.cpp:91-107,:164-187; src/api_autocomplete.cpp) over the sorted table and
the gfx950 prefix top-k kernel (csrc/ns_suggest.hip).

CPU: the table of a host-only engine against a Python restatement, the request split, the limit clamp, and the
failure of suggest without a device.  GPU: byte-equal JSON against the reference's own output (tests/golden/suggest,
tools/gen_golden_suggest.py), random prefixes and batch shapes against the restatement, raw ns_ac_* on hand-made tables,
reload, and the multi-device engine."""
import base64
import ctypes as C
import json
import os
import random
import shutil

import numpy as np
import pytest

import nsbind
import suggest_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "suggest")
FIXTURES = sorted(f[:-5] for f in os.listdir(GOLDEN) if f.endswith(".json"))


def _fixture(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def _cases(fx):
    for c in fx["cases"]:
        yield base64.b64decode(c["input_b64"]), c["limit"], c["json"], [base64.b64decode(s) for s in c["suggestions_b64"]]


@pytest.fixture(scope="module")
def fixture_index(tmp_path_factory, index_factory):
    """name -> index dir of a golden fixture (generated from its recorded parameters)"""
    cache = {}

    def make(name):
        if name not in cache:
            p = _fixture(name)["params"]
            if p["kind"] == "gen":
                cache[name] = index_factory(p["n_segments"], p["docs_per_segment"], p["vocab"], p["seed"], p["legacy"])[0]
            else:
                d = str(tmp_path_factory.mktemp("tiny") / "index")
                segs = [[(base64.b64decode(t), df) for t, df in seg] for seg in p["segments_b64"]]
                suggest_ref.write_tiny_index(d, segs)
                cache[name] = d
        return cache[name]

    return make


# ---------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("name", FIXTURES)
def test_table_of_a_host_only_engine_equals_the_restatement(fixture_index, name):
    d = fixture_index(name)
    eng = nsbind.Engine(d, -1)
    terms, scores, _ = eng.suggest_table()
    eng.close()
    want_terms, want_scores = suggest_ref.table(d)
    assert terms == want_terms
    assert [int(s) for s in scores] == want_scores
    assert all(terms[i] <= terms[i + 1] for i in range(len(terms) - 1))


def test_tiny_table_keeps_duplicates_drops_short_terms_and_wraps(fixture_index):
    eng = nsbind.Engine(fixture_index("tiny1"), -1)
    terms, scores, _ = eng.suggest_table()
    eng.close()
    table = list(zip(terms, [int(s) for s in scores]))
    # "covid" (5 + 1), "co-vid" (3), "COVID" (2): three entries of one string, by score
    assert [e for e in table if e[0] == b"covid"] == [(b"covid", 6), (b"covid", 3), (b"covid", 2)]
    assert (b"ab", 0) in table and (b"ab", 1) in table            # df 0 stays, "ab!" normalises onto "ab"
    assert (b"zz", 0) in table and table.count((b"zz", 0)) == 2   # df 0 in both raw spellings
    assert (b"wrap", (0xFFFFFFF0 + 0x20) & 0xFFFFFFFF) in table   # u32 sum wraps
    assert all(len(t) >= 2 for t in terms)                        # "c", "c.", "-x-", "..." dropped
    assert (b"caf", 2) in table                                   # bytes >= 0x80 are not alnum


def test_every_golden_answer_from_the_table_and_the_restated_ranking(fixture_index):
    """The host table + (score desc, term asc) reproduce every suggestion list of the reference (no device)."""
    for name in FIXTURES:
        eng = nsbind.Engine(fixture_index(name), -1)
        terms, scores, _ = eng.suggest_table()
        eng.close()
        for inp, limit, _, want in _cases(_fixture(name)):
            assert suggest_ref.suggest(terms, scores, inp, limit) == want, (name, inp, limit)


@pytest.mark.parametrize("inp,base,prefix", [
    (b"covid", b"", b"covid"), (b"New COVID va", b"New COVID ", b"va"), (b"cov!?", b"", b"cov"), (b"  co ", b"  ", b"co"),
    (b"", b"", b""), (b"!!!", b"", b""), (b"The Covid-19 pa", b"The Covid-19 ", b"pa"), (b"caf\xc3\xa9 Co", b"caf\xc3\xa9 ", b"co"),
    (b"\xc3\xa9T", b"\xc3\xa9", b"t"), (b"vi\x00", b"", b"vi"), (b"\x00t00", b"\x00", b"t00"), (b"a\nB", b"a\n", b"b"),
    (b"covid-19", b"covid-", b"19"), (b"X", b"", b"x"),
])
def test_base_prefix_split(inp, base, prefix):
    assert nsbind.suggest_split(inp) == (base, prefix)
    assert suggest_ref.split(inp) == (base, prefix)


def test_limit_clamp():
    L = nsbind.host_lib().nsh_suggest_clamp_limit
    assert [L(x) for x in (-3, 0, 1, 5, 10, 11, 1 << 30, -(1 << 30))] == [1, 1, 1, 5, 10, 10, 10, 1]


def test_suggest_on_a_host_only_engine_fails_with_a_message(fixture_index):
    eng = nsbind.Engine(fixture_index("tiny1"), -1)
    with pytest.raises(RuntimeError, match="no CPU autocomplete path"):
        eng.suggest_json("co", 5)
    with pytest.raises(RuntimeError, match="no CPU autocomplete path"):
        eng.suggest_batch_raw(["co", "vi"], 5)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_json_byte_equal_to_the_reference(fixture_index, name):
    eng = nsbind.Engine(fixture_index(name), 0)
    terms = eng.suggest_table()[0]
    n_json = 0
    for inp, limit, want_json, want in _cases(_fixture(name)):
        if want_json is not None:   # (null: the reference's dump(2) throws on invalid UTF-8; the suggestions still count)
            assert eng.suggest_json(inp, limit) == want_json.encode("utf-8"), (inp, limit)
            n_json += 1
        assert eng.suggest_batch([inp], limit, terms)[0] == want, (inp, limit)
    # the whole fixture as one batch
    cases = list(_cases(_fixture(name)))
    for limit in sorted({c[1] for c in cases}):
        ins = [c[0] for c in cases if c[1] == limit]
        got = eng.suggest_batch(ins, limit, terms)
        assert got == [c[3] for c in cases if c[1] == limit]
    eng.close()
    assert n_json > 0


def _random_inputs(terms, scores, n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        t = terms[rng.randrange(len(terms))]
        p = t[:rng.randint(1, len(t))]
        r = rng.random()
        if r < 0.15:
            p = p.upper()
        elif r < 0.3:
            p = b"some Words " + p
        elif r < 0.35:
            p = p + b"?! "
        elif r < 0.4:
            p = p + bytes([rng.choice(b"qxz09")])
        out.append(p)
    return out


@pytest.mark.gpu
def test_random_prefixes_and_batch_shapes_against_the_restatement(fixture_index):
    eng = nsbind.Engine(fixture_index("barrel3"), 0)
    terms, scores, _ = eng.suggest_table()
    scores = [int(s) for s in scores]
    assert len(terms) == 65536
    ins = _random_inputs(terms, scores, 4000, 17)
    for limit in (1, 5, 10):
        got = eng.suggest_batch(ins, limit, terms)
        for inp, g in zip(ins, got):
            assert g == suggest_ref.suggest(terms, scores, inp, limit), (inp, limit)
    big = _random_inputs(terms, scores, 16384, 18)
    want = {}
    for Q in (1, 63, 64, 65, 16384):
        got = eng.suggest_batch(big[:Q], 7, terms)
        for q in range(Q):
            if q not in want:
                want[q] = suggest_ref.suggest(terms, scores, big[q], 7)
            assert got[q] == want[q], (Q, big[q])
    # batch == single calls
    full = eng.suggest_batch(big, 7, terms)
    for q in range(0, 16384, 97):
        assert eng.suggest_batch([big[q]], 7, terms)[0] == full[q]
        js = json.loads(eng.suggest_json(big[q], 7).decode("utf-8", "surrogateescape"))
        assert js["limit"] == 7 and [s.encode("utf-8", "surrogateescape") for s in js["suggestions"]] == full[q]
    eng.close()


def _ctx():
    h = C.c_void_p()
    assert nsbind.hip_lib().ns_ctx_create(0, C.byref(h)) == 0
    return h


def _brute(terms, scores, prefix, L):
    hits = [i for i, t in enumerate(terms) if t.startswith(prefix)]
    return sorted(hits, key=lambda i: (-scores[i], terms[i], i))[:L]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 64 * 64 + 1])
def test_raw_ac_tables_of_every_size(n):
    ctx = _ctx()
    try:
        rng = random.Random(n)
        terms = sorted(b"%c%05d" % (rng.choice(b"ab"), rng.randrange(100000)) for _ in range(n))
        for scores in ([7] * n, [rng.randrange(4) for _ in range(n)]):   # all equal: ties across block and node boundaries
            ac = nsbind.AcTable(ctx, terms, scores)
            assert ac.rc == 0
            prefixes = [b"", b"a", b"b", b"c", b"a0", b"b1", b"a00", b"b99999", b"a123456"]
            prefixes += [t[:k] for t in rng.sample(terms, min(n, 40)) for k in (2, 3, 4, 6)]
            for L in (1, 3, 10):
                idx, cnt, _ = ac.suggest(prefixes, L)
                for q, p in enumerate(prefixes):
                    want = _brute(terms, scores, p, L)
                    assert list(idx[q, :cnt[q]]) == want, (n, p, L)
                    assert all(v == 0xFFFFFFFF for v in idx[q, cnt[q]:])
            ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


@pytest.mark.gpu
def test_raw_ac_ranges_that_start_and_end_mid_block():
    """One distinct prefix per run of terms, runs placed across level-0 blocks and level-1 nodes; long prefixes (> 8
    bytes) take the pool comparison."""
    ctx = _ctx()
    try:
        rng = random.Random(3)
        terms, k = [], 0
        while len(terms) < 3 * 4096 + 77:
            run = rng.choice([1, 5, 63, 64, 65, 130, 700, 4100])
            terms += [b"pre%06dx%04d" % (k, j) for j in range(run)]
            k += 1
        scores = [rng.randrange(1 << 32) if rng.random() < 0.5 else 3 for _ in terms]
        ac = nsbind.AcTable(ctx, terms, scores)
        assert ac.rc == 0
        prefixes = [b"pre%06d" % i for i in range(k)] + [b"pre%06dx" % i for i in range(k)] + [b"pre%06dx%02d" % (i, 0) for i in range(k)]
        prefixes += [b"pre", b"pr", b"pre9", b"pre000000x0000", b"pre000000x00000"]
        idx, cnt, _ = ac.suggest(prefixes, 10)
        for q, p in enumerate(prefixes):
            assert list(idx[q, :cnt[q]]) == _brute(terms, scores, p, 10), p
        ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(ctx)


@pytest.mark.gpu
def test_raw_ac_upload_rejects_bad_tables():
    L = nsbind.hip_lib()
    ctx = _ctx()
    try:
        assert nsbind.AcTable(ctx, [b"bb", b"ab"], [1, 1]).rc == -1   # NS_E_INVAL: not in byte order
        assert b"byte order" in L.ns_last_error(ctx)
        pool = b"x"
        offs = np.array([0, 1 << 32], dtype=np.uint64)   # a 4 GiB pool: rejected before any byte is read
        sc = np.array([1], dtype=np.uint32)
        h = C.c_void_p()
        assert L.ns_ac_upload(ctx, pool, offs.ctypes.data, sc.ctypes.data, 1, C.byref(h)) == -1
        assert b"4 GiB" in L.ns_last_error(ctx)
        ok = nsbind.AcTable(ctx, [b"ab", b"ab", b"abc"], [1, 2, 3])
        assert ok.rc == 0
        with pytest.raises(RuntimeError):
            ok.suggest([b"a"], 11)
        ok.close()
    finally:
        L.ns_ctx_destroy(ctx)


@pytest.mark.gpu
def test_reload_follows_a_segment_added_to_the_manifest(index_factory, tmp_path):
    src, _ = index_factory(3, 2000, 65536, 1337, False)
    d = str(tmp_path / "index")
    shutil.copytree(src, d)
    names = suggest_ref.read_manifest(d)
    suggest_ref.write_manifest(d, names[:2])
    eng = nsbind.Engine(d, 0)
    t2, s2, _ = eng.suggest_table()
    assert (t2, [int(s) for s in s2]) == suggest_ref.table(d)
    ins = [b"t0001", b"co", b"vi", b"t00", b"pa"]
    before = eng.suggest_batch(ins, 10, t2)
    suggest_ref.write_manifest(d, names)
    eng.reload()
    t3, s3, _ = eng.suggest_table()
    s3 = [int(s) for s in s3]
    assert (t3, s3) == suggest_ref.table(d)
    after = eng.suggest_batch(ins, 10, t3)
    assert after == [suggest_ref.suggest(t3, s3, x, 10) for x in ins]
    assert s3 != [int(s) for s in s2]   # the df sums moved
    assert before == [suggest_ref.suggest(t2, [int(s) for s in s2], x, 10) for x in ins]
    eng.close()


@pytest.mark.gpu
def test_multi_device_engine_answers_the_same(fixture_index):
    d = fixture_index("barrel3")
    one = nsbind.Engine(d, 0)
    two = nsbind.Engine(d, [0, 0])
    terms = one.suggest_table()[0]
    ins = [c[0] for c in _cases(_fixture("barrel3"))]
    assert two.suggest_batch(ins, 10, terms) == one.suggest_batch(ins, 10, terms)
    for x in ins[:50]:
        assert two.suggest_json(x, 5) == one.suggest_json(x, 5)
    two.close()
    one.close()
