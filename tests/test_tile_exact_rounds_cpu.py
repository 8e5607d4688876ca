"""The fixture of tests/test_tile_exact_rounds_gpu.py, built with numpy, and the coverage claim it has to meet.

The doc-tile body scores a term that has a skip table ("a term on the skip grid") cell by cell of 1024 docs: the term's
postings of the cell in full rounds of 256, then at most ONE partial round of 1..255 postings, as straight-line code for
1, 2, 3 or 4 chunks of 64 with one lane mask on the last chunk (csrc/ns_tile_kernel.hip, tile_round_exact).  The fixture
CONSTRUCTS the per-cell posting counts of three dense lists so that every shape of that dispatch occurs; this file checks,
without a GPU, that it really does, and that the docs shared by the three lists pin the fp32 accumulation order.
"""
import numpy as np

CELL = 1024                      # docs per skip-table cell == docs per tile of the doc-tile body (kSkipDocs)
N_CELLS_FULL = 24
N_DOCS = N_CELLS_FULL * CELL + 500   # a 25th cell cut short by n_docs
# per-cell posting counts every grid term has to see (cells 0 .. 18 of list 0; lists 1 and 2 see them rotated)
SHAPES = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 511, 512, 513, 1024]
TAIL = [300, 700, 1000, 2, 900]  # cells 19 .. 23
LAST = [200, 65, 500]            # the short last cell (500 docs), per dense list
ROT = [0, 7, 13]
N_SHORT = 90                     # the short list: a cursor term unless a table is registered for it (>= 64: it may get one)


def cell_counts(li):
    r = ROT[li]
    return SHAPES[r:] + SHAPES[:r] + TAIL + [LAST[li]]


def make_fixture():
    """-> dict(n_docs, doc_len, avgdl, lists=[(docIds, tfs)] * 4, counts=[per-cell counts] * 3); lists 0..2 dense, 3 short."""
    rng = np.random.default_rng(20261016)
    doc_len = rng.integers(20, 3000, size=N_DOCS, dtype=np.uint32)
    avgdl = float(np.float32(doc_len.astype(np.float64).mean()))
    lists, counts = [], []
    for li in range(3):
        cc = cell_counts(li)
        parts = []
        for c, n in enumerate(cc):
            lo, hi = c * CELL, min((c + 1) * CELL, N_DOCS)
            parts.append(np.sort(rng.choice(np.arange(lo, hi, dtype=np.uint32), size=n, replace=False)))
        docs = np.concatenate(parts).astype(np.uint32)
        lists.append((docs, rng.integers(1, 9, size=docs.size, dtype=np.uint32)))
        counts.append(cc)
    short = np.sort(rng.choice(N_DOCS, size=N_SHORT, replace=False)).astype(np.uint32)
    lists.append((short, rng.integers(1, 5, size=N_SHORT, dtype=np.uint32)))
    return {"n_docs": N_DOCS, "doc_len": doc_len, "avgdl": avgdl, "lists": lists, "counts": counts}


def term_scores(fx, li, idf, w):
    """fp32 restatement of src/api_engine.cpp:477-480 for one list (every operation rounds to fp32): w * bm25."""
    f = np.float32
    docs, tfs = fx["lists"][li]
    dl = fx["doc_len"][docs].astype(np.float32)
    norm = f(1.2) * ((f(1.0) - f(0.75)) + f(0.75) * (dl / f(fx["avgdl"])))
    tf = tfs.astype(np.float32)
    s = (f(idf) * (tf * (f(1.2) + f(1.0)))) / (tf + norm)
    return (f(w) * s).astype(np.float32)


def expected(fx, q, idfs, wts, k, conj=False):
    """The reference's answer for the query `q` (list indices, in accumulation order): (docIds, score bits, found)."""
    acc = np.zeros(fx["n_docs"], dtype=np.float32)
    hit = np.zeros(fx["n_docs"], dtype=np.uint32)
    for li, idf, w in zip(q, idfs, wts):
        docs = fx["lists"][li][0]
        acc[docs] = acc[docs] + term_scores(fx, li, idf, w)   # docIds are unique inside a list; fp32 + fp32 -> fp32
        hit[docs] += 1
    members = np.nonzero(hit == len(q) if conj else hit > 0)[0]
    order = np.lexsort((members, -acc[members].astype(np.float64)))[:k]   # best score first, ties by docId
    top = members[order]
    return top.astype(np.uint32), acc[top].view(np.uint32), int(members.size)


def test_fixture_covers_every_shape_of_the_exact_rounds():
    fx = make_fixture()
    assert fx["n_docs"] % CELL != 0 and fx["n_docs"] // CELL >= 24
    for li in range(3):
        docs = fx["lists"][li][0]
        assert np.all(np.diff(docs.astype(np.int64)) > 0)
        got = np.bincount(docs // CELL, minlength=N_CELLS_FULL + 1).tolist()
        assert got == fx["counts"][li]                       # the lists really hold what was constructed
        assert set(SHAPES) <= set(got)                        # every shape the issue lists, for EVERY grid term
        partial = {((n % 256 + 63) // 64, (n % 256) % 64 == 0) for n in got if n % 256}
        # the partial round: 1 .. 4 chunks with a ragged last chunk, 1 .. 3 with a full one (four full chunks ARE a full
        # round: the cell of exactly 256 postings below), after 0, 1 and more full rounds
        assert {(c, False) for c in (1, 2, 3, 4)} | {(c, True) for c in (1, 2, 3)} <= partial
        assert 256 in got and 0 in got and 1024 in got
        assert {n // 256 for n in got if n % 256} >= {0, 1, 2}
        assert got[-1] > 0                                    # the last cell, cut short by n_docs, holds postings
    short = fx["lists"][3][0]
    assert short.size >= 64 and np.bincount(short // CELL).max() <= 64   # a cursor term never needs more than one chunk per cell
    # the group is dense enough for the doc-tile class with two of the dense lists already (>= 0.25 postings per doc)
    assert (fx["lists"][0][0].size + fx["lists"][1][0].size) * 4 >= fx["n_docs"]
    # ... and no list is "thin" next to another (the planner's other class): rest * 32 > largest
    sizes = [fx["lists"][li][0].size for li in range(3)]
    assert (sum(sizes) - max(sizes)) * 32 > max(sizes)


def test_fixture_pins_the_accumulation_order():
    """Docs shared by the three dense lists whose three fp32 additions give different bits in another term order: a body that
    added the same postings in the wrong order would not reproduce the reference."""
    fx = make_fixture()
    idfs = {0: 1.7, 1: 0.9, 2: 2.3}
    a = expected(fx, [0, 1, 2], [idfs[0], idfs[1], idfs[2]], [1.0] * 3, fx["n_docs"], conj=True)
    b = expected(fx, [2, 1, 0], [idfs[2], idfs[1], idfs[0]], [1.0] * 3, fx["n_docs"], conj=True)
    assert a[2] == b[2] and a[2] >= 500                      # the same shared docs, many of them
    sa = dict(zip(a[0].tolist(), a[1].tolist()))
    sb = dict(zip(b[0].tolist(), b[1].tolist()))
    differ = [d for d in sa if sa[d] != sb[d]]
    assert len(differ) >= 20, len(differ)
    # in full rounds, in partial rounds and in the short last cell alike
    cells = {d // CELL for d in differ}
    assert N_CELLS_FULL in cells and len(cells) >= 10
