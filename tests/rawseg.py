"""Raw-segment helper of the tests that drive the C-ABI directly: a segment made of hand-built posting lists, queries over
list numbers, and the numpy fp32 restatement of the reference's scoring that every such test checks against.

The restatement (`_np_bm25`) is independent of the kernels and of the C oracle: accumulators start at +0.0f, terms are
added in query-term order, and a term's contribution is  w * ((idf * (tf * 2.2f)) / (tf + norm))  with every operation
rounded to fp32 (src/api_engine.cpp:449, 477-480 of the reference)."""
import ctypes as C

import numpy as np

import nsbind


def np_contrib(docs, tfs, idf, w, doc_len, avgdl):
    """one list's contributions  w * ((idf * (tf * 2.2f)) / (tf + norm))  per posting, every operation rounded to fp32"""
    f = np.float32
    dl = doc_len[docs].astype(np.float32)
    norm = f(1.2) * ((f(1.0) - f(0.75)) + f(0.75) * (dl / f(avgdl)))
    tf = tfs.astype(np.float32)
    s = (f(idf) * (tf * (f(1.2) + f(1.0)))) / (tf + norm)
    return f(w) * s


def _np_bm25(seg_lists, refs_idx, idfs, weights, doc_len, avgdl):
    """fp32 restatement of src/api_engine.cpp:477-480 in numpy (every operation rounds to fp32)."""
    f = np.float32
    acc = {}
    for li, idf, w in zip(refs_idx, idfs, weights):
        docs, tfs = seg_lists[li]
        x = np_contrib(docs, tfs, idf, w, doc_len, avgdl)
        for d, v in zip(docs.tolist(), x.tolist()):
            acc[d] = f(acc.get(d, f(0.0)) + f(v))
    return acc


def avgdl_of(doc_len):
    return float(np.float32(doc_len.astype(np.float64).mean()))


def payload_of(lists):
    """lists of (docIds, tfs) -> (the segment's posting payload: u32 {docId, tf} pairs back to back, byte offset of each list)"""
    parts = [np.stack([np.asarray(d, np.uint32), np.asarray(t, np.uint32)], axis=1).astype(np.uint32).ravel() for d, t in lists]
    flat = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
    offs = np.cumsum([0] + [len(p) * 4 for p in parts])[:-1].astype(np.uint64)
    return flat, offs


def descriptors(queries, lists, offs, idfs, weights, seg_id=0):
    """queries (lists of list numbers) -> (QDESC array, TERM array); a list keeps its idf and weight wherever it is named"""
    qd = np.zeros(len(queries), dtype=nsbind.QDESC_DTYPE)
    refs = []
    for qi, q in enumerate(queries):
        qd[qi] = (len(refs), len(q))
        for li in q:
            refs.append((seg_id, len(lists[li][0]), int(offs[li]), idfs[li], weights[li]))
    return qd, np.array(refs, dtype=nsbind.TERM_DTYPE)


class RawSegment:
    """One ctx with one uploaded segment; release() frees both (use try / finally)."""

    def __init__(self, n_docs, doc_len, lists, device=0):
        self.L = nsbind.hip_lib()
        self.n_docs, self.lists = int(n_docs), lists
        self.doc_len = np.ascontiguousarray(doc_len, dtype=np.uint32)
        assert len(self.doc_len) == self.n_docs
        self.avgdl = avgdl_of(self.doc_len)
        self.flat, self.offs = payload_of(lists)
        self.counts = np.array([len(d) for d, _ in lists], dtype=np.uint32)
        self.ctx = C.c_void_p()
        assert self.L.ns_ctx_create(device, C.byref(self.ctx)) == 0
        self.seg = C.c_void_p()
        rc = self.L.ns_segment_upload(self.ctx, 0, self.n_docs, C.c_float(self.avgdl), self.doc_len.ctypes.data, self.flat.ctypes.data,
                                      self.flat.nbytes, C.byref(self.seg))
        if rc != 0:
            msg = self.L.ns_last_error(self.ctx)
            self.L.ns_ctx_destroy(self.ctx)
            self.ctx = None
            raise AssertionError(msg)

    def err(self):
        return self.L.ns_last_error(self.ctx)

    def build_skips(self, min_count=64):
        which = np.flatnonzero(self.counts >= min_count)
        bo, cn = np.ascontiguousarray(self.offs[which]), np.ascontiguousarray(self.counts[which])
        assert self.L.ns_segment_build_skips(self.ctx, self.seg, bo.ctypes.data, cn.ctypes.data, len(which)) == 0, self.err()

    def build_impacts(self, idfs, leave_out=()):
        which = np.array([i for i in np.flatnonzero(self.counts > 0) if i not in leave_out], dtype=np.int64)
        bo, cn = np.ascontiguousarray(self.offs[which]), np.ascontiguousarray(self.counts[which])
        fi = np.array([idfs[i] for i in which], dtype=np.float32)
        assert self.L.ns_segment_build_impacts(self.ctx, self.seg, bo.ctypes.data, cn.ctypes.data, fi.ctypes.data, len(which)) == 0, self.err()

    def build_blockmax(self, idfs, which):
        which = np.asarray(which, dtype=np.int64)
        bo, cn = np.ascontiguousarray(self.offs[which]), np.ascontiguousarray(self.counts[which])
        fi = np.array([idfs[i] for i in which], dtype=np.float32)
        assert self.L.ns_segment_build_blockmax(self.ctx, self.seg, bo.ctypes.data, cn.ctypes.data, fi.ctypes.data, len(which)) == 0, self.err()

    def build_packed(self):
        assert self.L.ns_segment_build_packed(self.ctx, self.seg) == 0, self.err()

    def run(self, qd, refs, k, flags=nsbind.NS_FLAG_OR):
        """-> (hits, nhits, found, info flags) of one staged batch"""
        b = nsbind.prepare_raw(self.ctx, qd, refs, k, flags)
        try:
            info = int(b.info().flags)
            b.run()
            hits, nhits, found = b.fetch()
        finally:
            b.close()
        return hits, nhits, found, info

    def release(self):
        if self.ctx:
            nsbind.close_batches_of(self.ctx)
            if self.seg:
                self.L.ns_segment_release(self.ctx, self.seg)
            self.L.ns_ctx_destroy(self.ctx)
            self.ctx = None


def reference(lists, queries, idfs, weights, doc_len, avgdl):
    """per query: the restatement's (doc, score) pairs in the canonical order (score desc, docId asc) — of all docs some term
    ref touches (OR), and of the docs that EVERY term ref of the query holds (the AND filter over the same groups)"""
    out = []
    for q in queries:
        acc = _np_bm25(lists, q, [idfs[li] for li in q], [weights[li] for li in q], doc_len, avgdl)
        members = set(lists[q[0]][0].tolist()) if q else set()
        for li in q[1:]:
            members &= set(lists[li][0].tolist())
        keyed = sorted(acc.items(), key=lambda kv: (-float(kv[1]), kv[0]))
        out.append((keyed, [kv for kv in keyed if kv[0] in members]))
    return out


def check_results(ref, hits, nhits, found, k, and_mode=False, label=""):
    """`found`, `nhits`, docs in the canonical order and score BITS of every query against `reference(...)`; and_mode: against
    the reference's AND filter."""
    for qi, both in enumerate(ref):
        keyed = both[1] if and_mode else both[0]
        what = (label, "AND" if and_mode else "OR", "k", k, "query", qi)
        assert int(found[qi]) == len(keyed), what + ("found", int(found[qi]), len(keyed))
        keyed = keyed[:k]
        n = int(nhits[qi])
        assert n == len(keyed), what + ("nhits", n, len(keyed))
        got_docs = [int(d) for d in hits[qi, :n]["doc"]]
        assert got_docs == [d for d, _ in keyed], what + ("docs", got_docs[:8], [d for d, _ in keyed[:8]])
        want_bits = np.array([v for _, v in keyed], dtype=np.float32).view(np.uint32)
        np.testing.assert_array_equal(hits[qi, :n]["score"].view(np.uint32), want_bits, err_msg=str(what))


# ---- several segments in one ctx (tests/join_shapes.py): a term ref names (segment, list) -------------------------------
PAD_SCORE_BITS, PAD_ID = 0xFF800000, 0xFFFFFFFF   # the tail of a result row past nhits: -inf, seg = doc = 0xFFFFFFFF


def descriptors_multi(queries, seg_lists, seg_offs, idfs, weights):
    """queries (lists of (segment, list number)) -> (QDESC array, TERM array); idfs / weights: [segment][list]"""
    qd = np.zeros(len(queries), dtype=nsbind.QDESC_DTYPE)
    refs = []
    for qi, q in enumerate(queries):
        qd[qi] = (len(refs), len(q))
        for s, li in q:
            refs.append((s, len(seg_lists[s][li][0]), int(seg_offs[s][li]), idfs[s][li], weights[s][li]))
    refs = np.array(refs, dtype=nsbind.TERM_DTYPE) if refs else np.zeros(0, dtype=nsbind.TERM_DTYPE)
    return qd, refs


class RawSegments:
    """One ctx with several uploaded segments, ids 0 .. n-1 in the order given; `segments` holds (n_docs, doc_len, lists) per
    segment.  release() frees everything (use try / finally)."""

    def __init__(self, segments, device=0):
        self.L = nsbind.hip_lib()
        self.ctx = C.c_void_p()
        assert self.L.ns_ctx_create(device, C.byref(self.ctx)) == 0
        self.segs, self.doc_len, self.avgdl, self.lists, self.offs, self._keep = [], [], [], [], [], []
        for sid, (n_docs, doc_len, lists) in enumerate(segments):
            dl = np.ascontiguousarray(doc_len, dtype=np.uint32)
            assert len(dl) == int(n_docs)
            flat, offs = payload_of(lists)
            h = C.c_void_p()
            rc = self.L.ns_segment_upload(self.ctx, sid, int(n_docs), C.c_float(avgdl_of(dl)), dl.ctypes.data, flat.ctypes.data, flat.nbytes, C.byref(h))
            if rc != 0:
                msg = self.L.ns_last_error(self.ctx)
                self.release()
                raise AssertionError(msg)
            self.segs.append(h)
            self.doc_len.append(dl)
            self.avgdl.append(avgdl_of(dl))
            self.lists.append(lists)
            self.offs.append(offs)
            self._keep.append(flat)

    def err(self):
        return self.L.ns_last_error(self.ctx)

    run = RawSegment.run

    def build_skips(self, sid, min_count=64, leave_out=()):
        """skip tables for segment sid's lists of at least min_count postings, except the list numbers in leave_out"""
        counts = np.array([len(d) for d, _ in self.lists[sid]], dtype=np.uint32)
        which = np.array([i for i in np.flatnonzero(counts >= min_count) if i not in leave_out], dtype=np.int64)
        bo, cn = np.ascontiguousarray(self.offs[sid][which]), np.ascontiguousarray(counts[which])
        assert self.L.ns_segment_build_skips(self.ctx, self.segs[sid], bo.ctypes.data, cn.ctypes.data, len(which)) == 0, self.err()

    def release(self):
        if self.ctx:
            nsbind.close_batches_of(self.ctx)
            for h in self.segs:
                self.L.ns_segment_release(self.ctx, h)
            self.L.ns_ctx_destroy(self.ctx)
            self.ctx = None


def reference_multi(segments, queries, idfs, weights):
    """per query: the restatement's (score, seg, doc) triples in the join's canonical order (score desc, seg asc, doc asc), of
    every doc some term ref touches (OR) and of the docs that hold EVERY term ref the query names in their segment (AND);
    `reference()` per segment, joined"""
    out = []
    for q in queries:
        both = ([], [])
        for s in sorted({s for s, _ in q}):
            n_docs, doc_len, lists = segments[s]
            dl = np.ascontiguousarray(doc_len, dtype=np.uint32)
            (keyed, anded), = reference(lists, [[li for ss, li in q if ss == s]], idfs[s], weights[s], dl, avgdl_of(dl))
            both[0].extend((v, s, d) for d, v in keyed)
            both[1].extend((v, s, d) for d, v in anded)
        out.append(tuple(sorted(x, key=lambda t: (-float(t[0]), t[1], t[2])) for x in both))
    return out


def check_results_multi(ref, hits, nhits, found, k, and_mode=False, label=""):
    """`found`, `nhits`, segs and docs in the canonical order, score BITS and the padding of the row's tail, for every query,
    against `reference_multi(...)`"""
    for qi, both in enumerate(ref):
        keyed = both[1] if and_mode else both[0]
        what = (label, "AND" if and_mode else "OR", "k", k, "query", qi)
        assert int(found[qi]) == len(keyed), what + ("found", int(found[qi]), len(keyed))
        keyed = keyed[:k]
        n = int(nhits[qi])
        assert n == len(keyed), what + ("nhits", n, len(keyed))
        got = [(int(s), int(d)) for s, d in zip(hits[qi, :n]["seg"], hits[qi, :n]["doc"])]
        want = [(s, d) for _, s, d in keyed]
        if got != want:
            at = next(i for i in range(n) if got[i] != want[i])
            raise AssertionError(what + ("(seg, doc) differ first at rank", at, "got", got[at:at + 4], "want", want[at:at + 4]))
        want_bits = np.array([v for v, _, _ in keyed], dtype=np.float32).view(np.uint32)
        np.testing.assert_array_equal(hits[qi, :n]["score"].view(np.uint32), want_bits, err_msg=str(what))
        tail = hits[qi, n:k]
        assert np.all(tail["score"].view(np.uint32) == PAD_SCORE_BITS) and np.all(tail["seg"] == PAD_ID) and np.all(tail["doc"] == PAD_ID), what + ("padding",)
