"""The pooled one-shot calls that sit on CallBlock (csrc/ns_api.hip): ns_forward_build, ns_forward_merge(_keep),
ns_invert_forward / ns_forward_invert, ns_segment_filter, ns_docterms_select, ns_sem_topk, ns_ac_suggest, ns_ac_fuzzy and
ns_ac_fuzzy_prefix.
Every call here runs at a small shape through the raw C ABI; what is compared is every output byte (the times are not
output).  The reference is each call on a ctx of its own, whose pool is empty: a block that a call gets from the pool of a
shared ctx was another call's, often another family's, and nothing of it may show.  The refusals are host-side argument
checks (and the merge's own refusal of a source): no call here faults."""
import ctypes as C
import random

import numpy as np
import pytest

import correct_ref
import filter_ref
import fuzzy_shapes
import ingest_ref
import nsbind
import rawseg
from test_ingest_gpu import gen_corpus

pytestmark = pytest.mark.gpu
NS_E_INVAL = -1
KB64 = 64 << 10
FL_CHUNK = 64                                # kFlChunk of csrc/ns_filter.hip: postings per chunk of ns_segment_filter
FL_SIZES = [FL_CHUNK - 1, FL_CHUNK, FL_CHUNK + 1, 300]
FL_DOCS = 203                                # no multiple of 32: the bitmap's last word is partly used
FL_NEW_ID = 9


def _new_ctx():
    h = C.c_void_p()
    assert nsbind.hip_lib().ns_ctx_create(0, C.byref(h)) == 0
    return h


_INPUTS = {}   # made once, shared, never changed


def inputs():
    if _INPUTS:
        return _INPUTS
    L = nsbind.hip_lib()
    I = _INPUTS
    # ---- the forward index: a few dozen short documents in two parts, and a longer text for the uneven blocks ----
    texts = gen_corpus(5, 48, 12, vocab=300, long_tokens=())
    I["texts"] = texts
    I["parts"] = [ingest_ref.build(texts[:30]), ingest_ref.build(texts[30:])]
    assert all(len(p["counts"]) > 10 and len(p["terms"]) > 20 for p in I["parts"])
    keep = np.ones(len(I["parts"][0]["counts"]), dtype=bool)
    keep[1::3] = False
    I["keeps"] = [keep, None]
    I["texts_split"] = gen_corpus(6, 60, 60, vocab=2000, long_tokens=())
    # ---- ns_docterms_select: documents on both sides of the cut between the wave and the workgroup kernel ----
    cut = int(L.ns_docterms_doc_cut())
    rng = np.random.default_rng(11)
    sizes = [1, 7, 64, 129, cut - 1, cut, cut + 1, cut + 300]
    n_terms = 3 * cut
    pairs = np.concatenate([np.stack([rng.choice(n_terms, n, replace=False), rng.integers(1, 6, n)], axis=1) for n in sizes]).astype(np.uint32)
    df = rng.integers(1, 5000, n_terms).astype(np.uint32)
    df[::11] = 0
    I["dt_part"] = {"counts": np.asarray(sizes, dtype=np.uint32), "pairs": pairs}
    I["dt_df"], I["dt_idf"] = df, rng.uniform(0.1, 9.0, n_terms).astype(np.float32)
    I["dt_ids"] = np.asarray([7, 0, 5, 2, 6, 4, 1, 3, 6], dtype=np.uint32)
    assert sum(sizes[d] <= cut for d in I["dt_ids"]) >= 2 and sum(sizes[d] > cut for d in I["dt_ids"]) >= 2
    # ---- ns_sem_topk: two groups of queries (eight to a group), two banned rows per query, every slot of the answer taken ----
    V = rng.standard_normal((300, 24)).astype(np.float32)
    V = (V / np.sqrt((V.astype(np.float64) ** 2).sum(axis=1))[:, None]).astype(np.float32)
    qrows = rng.choice(300, size=11, replace=False)
    bans = [sorted({int(qrows[i]), int(qrows[(i + 1) % 11])}) for i in range(11)]
    I["sem_V"], I["sem_Q"] = V, V[qrows].copy()
    I["sem_ban_off"] = np.concatenate([[0], np.cumsum([len(b) for b in bans])]).astype(np.uint32)
    I["sem_ban_rows"] = np.array([r for b in bans for r in b], dtype=np.uint32)
    # ---- autocomplete, correction and completion on a table of a few hundred terms ----
    prng = random.Random(300)
    terms = fuzzy_shapes.hand_made(300, prng)
    I["ac_terms"], I["ac_scores"] = terms, [prng.choice([0, 1, 2, 3, 3, 7, 1 << 31]) for _ in terms]
    I["ac_prefixes"] = [b"", b"a", b"a0", b"b", b"b0000", b"zz", b"A", b"a" * 64] + [prng.choice(terms)[:prng.randint(1, 4)] for _ in range(20)]
    I["fz_queries"] = [correct_ref.random_edits(prng, prng.choice(terms), prng.randint(0, 3), b"ab019-") for _ in range(40)] + [b"", b"a00001", b"zzzz"]
    I["fz_edits"] = np.array([prng.randrange(3) for _ in I["fz_queries"]], dtype=np.uint8)
    # ---- ns_segment_filter: sources of n postings in three lists (the middle one shares its chunks with both neighbours), n on
    # both sides of one chunk and a few hundred; every third document dropped, the bits behind the last document set ----
    I["fl_doc_len"] = rng.integers(1, 90, FL_DOCS).astype(np.uint32)
    I["fl_lists"] = {}
    for n in FL_SIZES:
        cuts = [n // 3, n // 3, n - 2 * (n // 3)]
        I["fl_lists"][n] = [(np.sort(rng.choice(FL_DOCS, m, replace=False)).astype(np.uint32), rng.integers(1, 9, m).astype(np.uint32)) for m in cuts]
    keep = np.ones(FL_DOCS, dtype=bool)
    keep[2::3] = False
    I["fl_bits"] = filter_ref.bits_of(keep, fill_tail=True)
    I["fl_want"] = {n: filter_ref.compact(rawseg.payload_of(ls)[0].reshape(-1, 2), rawseg.payload_of(ls)[1], [len(d) for d, _ in ls], keep)
                    for n, ls in I["fl_lists"].items()}
    return I


def _flat32(items):
    data, offs = nsbind.flat_inputs(items)
    return data if data else None, offs.astype(np.uint32)


class Session:
    """One ctx with the handles the calls need, made when first asked for."""

    def __init__(self):
        self.L, self.ctx, self.I = nsbind.hip_lib(), _new_ctx(), inputs()
        self.dt = self.sem = self.ac = None
        self.fl = {}

    def close(self):
        for h, _, _ in self.fl.values():
            assert self.L.ns_segment_release(self.ctx, h) == 0
        if self.dt:
            self.dt.close()
        if self.sem:
            assert self.L.ns_sem_release(self.ctx, self.sem) == 0
        if self.ac:
            self.ac.close()
        self.L.ns_ctx_destroy(self.ctx)

    def err(self):
        return self.L.ns_last_error(self.ctx).decode()

    # ---- the calls: -> list of bytes, one per output array ----
    def build(self, texts):
        got = nsbind.forward_build(self.ctx, texts)
        info = {k: v for k, v in got["info"].items() if k != "device_ms"}
        return [got[k].tobytes() for k in ("kept_docs", "doc_len", "counts", "pairs")] + [b"\0".join(got["terms"]), repr(sorted(info.items())).encode()], got["info"]

    def merged(self, got):
        info = {k: v for k, v in got["info"].items() if k != "device_ms"}
        assert got["invert_ms"] > 0.0
        return [got[k].tobytes() for k in ("kept_docs", "doc_len", "counts", "pairs", "df", "postings")] + [b"\0".join(got["terms"]), repr(sorted(info.items())).encode()]

    def merge(self, radix=False):
        assert self.L.ns_ctx_use_docsort(self.ctx, 0 if radix else 1) == 0   # radix: every document goes through the merge's third block
        try:
            return self.merged(nsbind.forward_merge(self.ctx, self.I["parts"], invert=True))
        finally:
            assert self.L.ns_ctx_use_docsort(self.ctx, 1) == 0

    def merge_keep(self):
        return self.merged(nsbind.forward_merge_keep(self.ctx, self.I["parts"], self.I["keeps"], invert=True))

    def invert(self, timed, n_pairs=None):
        p = self.I["parts"][0]
        pairs, n_terms = np.ascontiguousarray(p["pairs"]), len(p["terms"])
        df, post = np.full(n_terms, 0xABABABAB, dtype=np.uint32), np.full((len(pairs), 2), 0xABABABAB, dtype=np.uint32)
        kept, ms = C.c_uint64(), C.c_float(-1.0)
        rc = self.L.ns_invert_forward(self.ctx, p["counts"].ctypes.data, len(p["counts"]), pairs.ctypes.data, len(pairs) if n_pairs is None else n_pairs,
                                      n_terms, df.ctypes.data, post.ctypes.data, C.byref(kept), C.byref(ms) if timed else None)
        assert rc != 0 or not timed or ms.value > 0.0
        return rc, [df.tobytes(), post[:kept.value].tobytes(), bytes(C.c_uint64(kept.value))]

    def filter(self, n, timed, new_id=FL_NEW_ID):
        """the filtered copy of the source of n postings under new_id, released again: the lists' new places, the payload read
        back from the new segment, the number kept"""
        if n not in self.fl:
            flat, offs = rawseg.payload_of(self.I["fl_lists"][n])
            h, dl = C.c_void_p(), self.I["fl_doc_len"]
            assert self.L.ns_segment_upload(self.ctx, FL_SIZES.index(n), FL_DOCS, C.c_float(rawseg.avgdl_of(dl)), dl.ctypes.data, flat.ctypes.data, flat.nbytes, C.byref(h)) == 0, self.err()
            self.fl[n] = (h, offs, np.array([len(d) for d, _ in self.I["fl_lists"][n]], dtype=np.uint32))
        src, offs, counts = self.fl[n]
        noff, ncnt, payload = np.full(3, 0xABABABAB, dtype=np.uint64), np.full(3, 0xABABABAB, dtype=np.uint32), np.full((n, 2), 0xABABABAB, dtype=np.uint32)
        kept, ms, h = C.c_uint64(), C.c_float(-1.0), C.c_void_p()
        rc = self.L.ns_segment_filter(self.ctx, src, new_id, self.I["fl_bits"].ctypes.data, offs.ctypes.data, counts.ctypes.data, 3, noff.ctypes.data, ncnt.ctypes.data,
                                      payload.ctypes.data, C.byref(kept), C.byref(ms) if timed else None, C.byref(h))
        if rc != 0:
            assert not h.value
            return rc, []
        assert not timed or ms.value > 0.0
        assert self.L.ns_segment_release(self.ctx, h) == 0
        w_payload, w_off, w_cnt, w_kept = self.I["fl_want"][n]
        assert kept.value == w_kept and 0 < w_kept < n and np.array_equal(noff, w_off) and np.array_equal(ncnt, w_cnt) and np.array_equal(payload[:w_kept], w_payload)
        return rc, [noff.tobytes(), ncnt.tobytes(), payload[:kept.value].tobytes(), bytes(C.c_uint64(kept.value))]

    def select(self, timed, ids=None):
        if not self.dt:
            self.dt = nsbind.DocTerms(self.ctx, self.I["dt_part"], self.I["dt_df"], self.I["dt_idf"])
        ids = self.I["dt_ids"] if ids is None else np.asarray(ids, dtype=np.uint32)
        term, w, cnt = (np.full(s, 0x5A5A5A5A, dtype=np.uint32) for s in ((len(ids), 25), (len(ids), 25), len(ids)))
        ms = C.c_float(-1.0)
        rc = self.L.ns_docterms_select(self.dt.h, ids.ctypes.data, len(ids), 25, 1, 1, 0xFFFFFFFF, term.ctypes.data, w.ctypes.data, cnt.ctypes.data,
                                       C.byref(ms) if timed else None)
        assert rc != 0 or not timed or ms.value > 0.0
        return rc, [term.tobytes(), w.tobytes(), cnt.tobytes()]

    def sem_topk(self, timed, topk=5):
        I = self.I
        if not self.sem:
            self.sem = C.c_void_p()
            assert self.L.ns_sem_upload(self.ctx, I["sem_V"].ctypes.data, I["sem_V"].shape[0], I["sem_V"].shape[1], C.byref(self.sem)) == 0, self.err()
        n_q = len(I["sem_Q"])
        rows, sims, cnt = np.zeros((n_q, topk), dtype=np.uint32), np.zeros((n_q, topk), dtype=np.float32), np.zeros(n_q, dtype=np.uint32)
        ms = C.c_float(-1.0)
        rc = self.L.ns_sem_topk(self.ctx, self.sem, I["sem_Q"].ctypes.data, n_q, topk, C.c_float(-2.0), I["sem_ban_off"].ctypes.data, I["sem_ban_rows"].ctypes.data,
                                rows.ctypes.data, sims.ctypes.data, cnt.ctypes.data, C.byref(ms) if timed else None)
        if rc == 0:
            assert (cnt == topk).all()           # min_sim = -2: every slot is the call's (it leaves the slots past a count alone)
            assert not timed or ms.value > 0.0
        return rc, [rows.tobytes(), sims.tobytes(), cnt.tobytes()]

    def table(self):
        if not self.ac:
            self.ac = nsbind.AcTable(self.ctx, self.I["ac_terms"], self.I["ac_scores"])
            assert self.ac.rc == 0 and self.ac.build_fuzzy()[0] == 0
        return self.ac

    def suggest(self, timed, offs=None):
        ac = self.table()
        data, offs32 = _flat32(self.I["ac_prefixes"])
        n_q = len(offs32) - 1
        if offs is not None:
            offs32 = np.asarray(offs, dtype=np.uint32)
        idx, cnt = np.full((n_q, 10), 0xABABABAB, dtype=np.uint32), np.full(n_q, 0xABABABAB, dtype=np.uint32)
        ms = C.c_float(-1.0)
        rc = self.L.ns_ac_suggest(self.ctx, ac.h, data, offs32.ctypes.data, n_q, 10, idx.ctypes.data, cnt.ctypes.data, C.byref(ms) if timed else None)
        assert rc != 0 or not timed or ms.value > 0.0
        return rc, [idx.tobytes(), cnt.tobytes()]

    def fuzzy(self, complete, timed, edits=None, offs=None):
        ac = self.table()
        data, offs32 = _flat32(self.I["fz_queries"])
        n_q = len(offs32) - 1
        if offs is not None:
            offs32 = np.asarray(offs, dtype=np.uint32)
        ed = self.I["fz_edits"] if edits is None else np.asarray(edits, dtype=np.uint8)
        idx, dist, cnt = np.full((n_q, 10), 0xABABABAB, dtype=np.uint32), np.full((n_q, 10), 0xAB, dtype=np.uint8), np.full(n_q, 0xABABABAB, dtype=np.uint32)
        ms = C.c_float(-1.0)
        fn = self.L.ns_ac_fuzzy_prefix if complete else self.L.ns_ac_fuzzy
        rc = fn(self.ctx, ac.h, data, offs32.ctypes.data, n_q, ed.ctypes.data, 1 if complete else 0, 10, idx.ctypes.data, dist.ctypes.data, cnt.ctypes.data,
                C.byref(ms) if timed else None)
        assert rc != 0 or not timed or ms.value > 0.0
        return rc, [idx.tobytes(), dist.tobytes(), cnt.tobytes()]


def _ok(res):
    assert res[0] == 0, res[0]
    return res[1]


# name -> (family, call).  Each timed call once with and once without device_ms_out (the forward handle's time is not optional).
CALLS = {
    "build": ("build", lambda s: s.build(s.I["texts"])[0]),
    "build_split": ("build", lambda s: s.build(s.I["texts_split"])[0]),
    "merge": ("merge", lambda s: s.merge()),
    "merge_radix": ("merge", lambda s: s.merge(radix=True)),
    "merge_keep": ("merge", lambda s: s.merge_keep()),
    "invert": ("invert", lambda s: _ok(s.invert(True))),
    "invert_untimed": ("invert", lambda s: _ok(s.invert(False))),
    "filter_below_a_chunk": ("filter_chunk", lambda s: _ok(s.filter(FL_CHUNK - 1, True))),
    "filter_a_chunk": ("filter_chunk", lambda s: _ok(s.filter(FL_CHUNK, True))),
    "filter_above_a_chunk": ("filter_chunk", lambda s: _ok(s.filter(FL_CHUNK + 1, False))),
    "filter": ("filter", lambda s: _ok(s.filter(300, True))),
    "filter_untimed": ("filter", lambda s: _ok(s.filter(300, False))),
    "select": ("select", lambda s: _ok(s.select(True))),
    "select_untimed": ("select", lambda s: _ok(s.select(False))),
    "sem": ("sem", lambda s: _ok(s.sem_topk(True))),
    "sem_untimed": ("sem", lambda s: _ok(s.sem_topk(False))),
    "suggest": ("suggest", lambda s: _ok(s.suggest(True))),
    "suggest_untimed": ("suggest", lambda s: _ok(s.suggest(False))),
    "fuzzy": ("fuzzy", lambda s: _ok(s.fuzzy(False, True))),
    "fuzzy_untimed": ("fuzzy", lambda s: _ok(s.fuzzy(False, False))),
    "fuzzy_prefix": ("complete", lambda s: _ok(s.fuzzy(True, True))),
    "fuzzy_prefix_untimed": ("complete", lambda s: _ok(s.fuzzy(True, False))),
}


def run_round(s, order=None):
    out = {}
    for name in order or list(CALLS):
        out[name] = CALLS[name][1](s)
        assert len(out[name]) >= 2 and all(isinstance(b, bytes) for b in out[name]), name
    return out


_REFERENCE = {}   # every call on a ctx of its own: computed once, shared, never changed


def reference():
    if not _REFERENCE:
        for name in CALLS:
            s = Session()
            try:
                _REFERENCE[name] = CALLS[name][1](s)
            finally:
                s.close()
    return _REFERENCE


def _refused(s, fn_name, rc):
    assert rc == NS_E_INVAL, (fn_name, rc)
    assert s.err().startswith(fn_name + ": "), s.err()


def test_a_refused_call_between_two_runs_changes_no_byte_of_the_second():
    s = Session()
    L, I = s.L, s.I
    try:
        first = run_round(s)
        assert first == reference()
        assert np.frombuffer(first["suggest"][1], dtype=np.uint32).sum() > 0 and np.frombuffer(first["fuzzy"][2], dtype=np.uint32).sum() > 0   # the runs are about something
        n_q, n_f = len(I["ac_prefixes"]), len(I["fz_queries"])
        # ns_forward_build: offsets that decrease
        text, h = b"Alpha beta alpha. The gamma", C.c_void_p()
        offs = np.asarray([0, 17, 5], dtype=np.uint64)
        _refused(s, "ns_forward_build", L.ns_forward_build(s.ctx, text, len(text), offs.ctypes.data, 2, C.byref(h)))
        assert not h.value
        # ns_docterms_select: a doc id past the handle
        _refused(s, "ns_docterms_select", s.select(True, ids=[0, len(I["dt_part"]["counts"]), 1])[0])
        # ns_sem_topk: topk out of range
        _refused(s, "ns_sem_topk", s.sem_topk(True, topk=65)[0])
        # ns_invert_forward: per-document counts that do not sum to n_pairs
        _refused(s, "ns_invert_forward", s.invert(True, n_pairs=len(I["parts"][0]["pairs"]) - 1)[0])
        # the merge: a source whose counts do not sum (refused on the host), and one that names a term twice (refused by the merge
        # itself after its dictionary stage, with its blocks out of the pool)
        short = dict(I["parts"][1], counts=I["parts"][1]["counts"][:-1], doc_len=I["parts"][1]["doc_len"][:-1])
        twice = dict(I["parts"][1], terms=[I["parts"][1]["terms"][0]] + I["parts"][1]["terms"][1:-1] + [I["parts"][1]["terms"][0]])
        for fn_name, bits in (("ns_forward_merge", None), ("ns_forward_merge_keep", nsbind.keep_bitmaps(I["keeps"]))):
            for bad, why in ((short, "do not sum to n_pairs"), (twice, "occurs twice")):
                arr, alive = nsbind.forward_sources([I["parts"][0], bad])
                rc = L.ns_forward_merge(s.ctx, arr, 2, C.byref(h)) if bits is None else L.ns_forward_merge_keep(s.ctx, arr, bits[0], 2, C.byref(h))
                _refused(s, fn_name, rc)
                assert "source 1" in s.err() and why in s.err() and not h.value, s.err()
        # ns_segment_filter: a new_seg_id already in use (the source's own), after the call's host-side checks only
        assert s.filter(300, True, new_id=FL_SIZES.index(300))[0] == NS_E_INVAL and s.err() == "segment %d already uploaded" % FL_SIZES.index(300), s.err()
        # ns_ac_suggest and ns_ac_fuzzy_prefix: offsets that decrease; ns_ac_fuzzy: more edits than the corrector allows
        down = [5, 3] + [3] * (n_q - 1)
        _refused(s, "ns_ac_suggest", s.suggest(True, offs=down)[0])
        _refused(s, "ns_ac_fuzzy", s.fuzzy(False, True, edits=[3] * n_f)[0])
        _refused(s, "ns_ac_fuzzy_prefix", s.fuzzy(True, False, offs=[5, 3] + [3] * (n_f - 1))[0])
        assert run_round(s) == first
    finally:
        s.close()


def test_pooled_blocks_carry_nothing_from_call_to_call():
    want = reference()
    names = list(CALLS)
    # neighbours of different families: a call's block is one that another family's call has just returned
    by_family = {}
    for n in names:
        by_family.setdefault(CALLS[n][0], []).append(n)
    weave = [fam.pop(0) for _ in range(max(map(len, by_family.values()))) for fam in by_family.values() if fam]
    assert sorted(weave) == sorted(names) and all(CALLS[a][0] != CALLS[b][0] for a, b in zip(weave, weave[1:]))
    for order in (weave, weave[::-1] + weave[::2]):
        s = Session()
        try:
            for name in order:
                assert CALLS[name][1](s) == want[name], name
        finally:
            s.close()
    # NOTE: the ABI does not report block sizes, so the figures below restate the layouts of csrc/ns_api.hip by hand (the regions
    # of each call, 256-byte rounding, eight queries to a group of ns_sem_topk, the pool's 64 KiB smallest bucket).  They keep
    # the SHAPES honest; they do not follow a layout that changes.  Whoever changes one of these layouts or pool_quantise
    # has to redo this arithmetic, or the property it stands for is gone while the assertions still hold.
    # the shapes: the small calls' blocks all quantise to the pool's smallest bucket, 64 KiB, so they do change hands ...
    I = inputs()
    n_q, n_f = len(I["ac_prefixes"]), len(I["fz_queries"])
    assert len(I["dt_ids"]) * (2 * 4 + 2 * 25 * 4 + 4) + 5 * 256 <= KB64                       # ns_docterms_select: ids, list, term, w, count
    assert (n_q + 1) * 4 + sum(map(len, I["ac_prefixes"])) + n_q * 11 * 4 + 512 <= KB64        # ns_ac_suggest: the image and the answers
    assert 7 * 4 + (300 // FL_CHUNK + 2) * (8 + 4) + 2 * 4 + 3 * (4 + 4 + 4 + 8) + 9 * 256 <= KB64   # ns_segment_filter: the bitmap, a mask and a base per chunk, the lists
    assert 16 * 24 * 4 + 8 * 5 * 5 * 8 + 2 * 9 * 4 + 8 * 4 + 22 * 4 + 16 * (2 * 5 + 1) * 4 + 8 * 256 <= KB64   # ns_sem_topk: its eight regions, two groups of 8
    # ... and ns_forward_build's second and third block differ: B holds three words per token (12 B x n_tokens + its scan
    # sums: at most 64 KiB up to 5000 tokens), C more than 60 B per kept token (past 64 KiB from 1100 kept tokens on)
    s = Session()
    try:
        info = s.build(I["texts_split"])[1]
        assert info["n_tokens"] <= 5000 and info["kept_tokens"] >= 1100, info
    finally:
        s.close()
