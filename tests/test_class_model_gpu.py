"""The class model on the GPU (ns_ctx_class_model; nextsearch-api_amd/csrc/ns_plan.hpp "class model"): groups that the model
sends to the doc-tile body instead of the driver-stream body score byte-identically.  One generated segment of 8192 docs
(8 tiles); every case is prepared under mode 0 (the density rule) and mode 2 (the model, whatever the batch size), must
report the promotion (ns_batch_class_stats), give the same bytes, and equal the C oracle (tests/orc.py).  Three inputs that
query strings cannot say (a signed weight with a tf = 0 posting, a list that ends inside its last tile, a list with no
posting in some tile) run on a hand-made segment of the same size against the numpy restatement of tests/rawseg.py."""
import numpy as np
import pytest

import nsbind
import orc
import rawseg
import workloads

pytestmark = pytest.mark.gpu
T = workloads.term_name
N_DOCS = 8192


def words(*ranks):
    return " ".join(T(r) for r in ranks)


# list lengths on this index follow 0.6 * 8192 / rank: ranks 4, 7, 123 hold 1267 + 673 + 39 postings
THREE = words(4, 7, 123)
EIGHT = words(10, 14, 20, 30, 40, 60, 90, 14)        # eight term refs, one list twice; 0.23 postings per doc
THIN = [words(1, 200), words(1, 300), words(1, 250, 400), words(1, 222)]   # one hot list and short tails: thin groups
DENSE = words(2, 3, 4)                               # 0.65 postings per doc: a tile group by the density rule already
MIX = [THREE, EIGHT, words(5, 9, 50), words(6, 8, 77, 140), DENSE, T(3), words(12, 15)] + THIN


@pytest.fixture(scope="module")
def index(index_factory):
    return index_factory(1, N_DOCS, 4096)[0]


@pytest.fixture(scope="module")
def oracle(index):
    ora = orc.Oracle(index)
    cache = {}

    def ask(queries, k, flags):
        key = (tuple(queries), k, flags)
        if key not in cache:
            cache[key] = ora.search_batch(list(queries), k, flags)
        return cache[key]

    yield ask
    ora.close()


@pytest.fixture()
def engine(index):
    eng = nsbind.Engine(index, 0)
    yield eng
    eng.close()


def scored(eng, queries, k, flags, mode):
    eng.class_model(mode)
    b = eng.prepare(queries, k, flags)
    try:
        stats = b.class_stats()
        n_items = int(b.info().n_items)
        b.run()
        hits, nhits, found = b.fetch()[:3]
        rows = b.row_stats()
    finally:
        b.close()
    return (hits, nhits, found), stats, n_items, rows


def check_oracle(got, want, queries, k, flags):
    gh, gn, gf = got
    oh, on, of, ou = want
    for q in range(len(queries)):
        if not ou[q]:
            continue
        n = int(on[q])
        assert int(gn[q]) == n and int(gf[q]) == int(of[q]), (queries[q], k, flags)
        assert n == min(int(gf[q]), nsbind.clamp_k(k))
        assert np.array_equal(gh[q, :n]["doc"], oh[q, :n]["doc"]), (queries[q], k, flags)
        assert np.array_equal(gh[q, :n]["score"].view(np.uint32), oh[q, :n]["score"].view(np.uint32)), (queries[q], k, flags)


def both_modes(eng, oracle, queries, k=10, flags=0, promoted=None):
    off, s0, n0, r0 = scored(eng, queries, k, flags, 0)
    on, s2, n2, r2 = scored(eng, queries, k, flags, 2)
    assert s0[3] == 0 and sum(s0[:3]) == sum(s2[:3]) == len(queries)
    assert s2[3] == (promoted if promoted is not None else s2[3]) and s2[3] > 0, (s0, s2)
    assert s2[2] == s0[2] + s2[3] and s2[0] == s0[0] - s2[3] and s2[1] == s0[1]     # promoted groups leave class 0 for the tiles, thin ones stay
    for a, b in zip(off, on):
        assert a.tobytes() == b.tobytes()
    check_oracle(on, oracle(queries, k, flags), queries, k, flags)
    return (s0, n0, r0), (s2, n2, r2)


@pytest.mark.parametrize("k", [10, 32, 33, 100])
def test_three_and_eight_terms(engine, oracle, k):
    both_modes(engine, oracle, [THREE, EIGHT], k=k, promoted=2)


def test_and_mode(engine, oracle):
    both_modes(engine, oracle, [THREE, EIGHT, words(5, 9, 50)], flags=nsbind.NS_FLAG_AND, promoted=3)


def test_four_ranges_join_in_k_merge(engine, oracle):
    # one chunk per group (min_items 1) and 450 work units per item: the promoted group's modelled cost (about 3 500 units at
    # the doubled share of a tile group) cuts it into four ranges on the tile grid, whose partial rows k_merge joins
    engine.set_tuning(0, 1, 450)
    (s0, n0, _), (s2, n2, _) = both_modes(engine, oracle, [THREE] * 3, promoted=3)
    assert n2 == 4 * 3, n2


@pytest.mark.parametrize("share", [0, 2])
def test_shared_scores_on_and_off(engine, oracle, share):
    engine.share_scores(share)
    eng_flags = []
    for mode in (0, 2):
        engine.class_model(mode)
        b = engine.prepare(MIX, 10, 0)
        eng_flags.append(bool(int(b.info().flags) & nsbind.NS_INFO_SHARED))
        b.close()
    assert eng_flags == [share == 2, share == 2]
    both_modes(engine, oracle, MIX)


def test_impact_streams_present(engine, oracle):
    engine.build_impacts()
    engine.class_model(2)
    b = engine.prepare(MIX, 10, 0)
    assert int(b.info().flags) & nsbind.NS_INFO_IMPACTS
    b.close()
    both_modes(engine, oracle, MIX)


def test_thin_groups_stay_row_consumers(engine, oracle):
    L = nsbind.hip_lib()
    engine.share_scores(2)
    assert L.ns_ctx_share_rows(engine.ctx, 2) == 0
    (s0, _, r0), (s2, _, r2) = both_modes(engine, oracle, MIX)
    assert r0[1] > 0 and r2[:2] == r0[:2]          # the same producers and consumers in both modes
    assert s2[1] == s0[1] >= len(THIN)


# ---- what query strings cannot say: a hand-made segment of the same size ------------------------------------------------

def raw_case():
    rng = np.random.default_rng(23)
    doc_len = rng.integers(20, 3000, size=N_DOCS, dtype=np.uint32)

    def lst(docs, zero_tf_at=()):
        d = np.unique(np.asarray(docs, np.int64)).astype(np.uint32)
        tf = rng.integers(1, 9, size=len(d), dtype=np.uint32)
        tf[list(zero_tf_at)] = 0
        return d, tf

    lists = [
        lst(rng.choice(N_DOCS, 1200, replace=False), zero_tf_at=(0, 17, 600)),           # 0: tf = 0 postings (scored with a signed weight)
        lst(rng.choice(N_DOCS, 700, replace=False)),                                     # 1
        lst(rng.choice(7 * 1024 + 300, 40, replace=False)),                              # 2: ends inside the last tile it reaches
        lst(np.concatenate([rng.choice(np.arange(0, 2048), 300, replace=False),          # 3: no posting in tiles 2, 3 and 6
                            rng.choice(np.arange(4096, 6144), 250, replace=False), rng.choice(np.arange(7168, 8000), 120, replace=False)])),
        lst(rng.choice(np.arange(1024, 1024 + 700), 400, replace=False)),                # 4: one tile only
    ]
    queries = [[0, 1, 2], [3, 1, 2], [0, 3, 2], [1, 3, 4, 2], [4, 3, 2], [2, 3, 4, 2]]
    idfs = [1.5, 2.125, 3.0, 2.75, 1.875]
    weights = [-0.75, 1.0, 1.0, 0.5, -1.25]
    return doc_len, lists, queries, idfs, weights


def test_signed_zero_tf_partial_and_empty_tiles():
    doc_len, lists, queries, idfs, weights = raw_case()
    ref = rawseg.reference(lists, queries, idfs, weights, doc_len, rawseg.avgdl_of(doc_len))
    seg = rawseg.RawSegment(N_DOCS, doc_len, lists)
    try:
        L = seg.L
        seg.build_skips()
        qd, refs = rawseg.descriptors(queries, lists, seg.offs, idfs, weights)
        for flags in (0, nsbind.NS_FLAG_AND):
            res = {}
            for mode in (0, 2):
                assert L.ns_ctx_class_model(seg.ctx, mode) == 0
                b = nsbind.prepare_raw(seg.ctx, qd, refs, 10, flags)
                try:
                    stats = b.class_stats()
                    b.run()
                    res[mode] = b.fetch()[:3]
                finally:
                    b.close()
                assert stats[3] == (len(queries) if mode == 2 else 0), (mode, stats)
            for a, b_ in zip(res[0], res[2]):
                assert a.tobytes() == b_.tobytes()
            rawseg.check_results(ref, *res[2], 10, and_mode=bool(flags))
    finally:
        seg.release()
