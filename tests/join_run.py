"""Runs the directed join families of tests/join_shapes.py through the raw C-ABI against the numpy restatement
(tests/rawseg.py), and the synthetic rank rows through ns_merge_rank_rows against the numpy join (tests/join_ref.py).

Imported by tests/test_join_shapes_gpu.py for the product library, and by tests/body_reach.py in the child process that
loaded the counting build: there `reach()` resets the join counters around every family, and reports them next to the
per-path query counts that the family's declaration (pinned to the planner by tests/test_join_shapes_cpu.py) predicts."""
import ctypes as C

import numpy as np

import join_ref
import join_shapes
import nsbind
from rawseg import RawSegments, check_results_multi, descriptors_multi, reference_multi

AND = nsbind.NS_FLAG_AND
_REFERENCE = {}   # family name -> reference_multi(...): computed once, shared, never changed


def reference_of(name, fam):
    if name not in _REFERENCE:
        _REFERENCE[name] = reference_multi(fam.segments, fam.queries, fam.idfs, fam.weights)
    return _REFERENCE[name]


def run_family(name):
    """OR and AND at every K of the family, then shared term scores (NS_INFO_SHARED asserted) at its shared_k, all under the
    family's own tuning; one ctx, always released.  -> the K of every batch that ran"""
    fam = join_shapes.FAMILIES[name]()
    ref = reference_of(name, fam)
    segs = RawSegments(fam.segments)
    ran = []
    try:
        L, ctx = segs.L, segs.ctx
        qd, refs = descriptors_multi(fam.queries, segs.lists, segs.offs, fam.idfs, fam.weights)
        assert L.ns_set_tuning(ctx, *fam.tuning) == 0, segs.err()

        def go(label, k, flags, want=0):
            hits, nhits, found, info = segs.run(qd, refs, k, flags)
            ran.append(k)
            assert info & want == want, (name, label, "batch info flags", hex(info), "want", hex(want))
            check_results_multi(ref, hits, nhits, found, k, and_mode=bool(flags & AND), label=(name, label))

        assert L.ns_ctx_share_scores(ctx, 0) == 0
        for k in fam.ks:
            go("in place", k, 0)
            go("in place", k, AND)
        assert L.ns_ctx_share_scores(ctx, 2) == 0
        go("shared term scores", fam.shared_k, 0, want=nsbind.NS_INFO_SHARED)
        go("shared term scores", fam.shared_k, AND, want=nsbind.NS_INFO_SHARED)
    finally:
        segs.release()
    return ran


def predicted_path_counts(name, ran):
    """counters 0 .. 3 after batches at the K values `ran`: one count per query and batch, on the path the family declares"""
    fam = join_shapes.FAMILIES[name]()
    return [sum(fam.paths[k].count(p) for k in ran) for p in join_shapes.PATHS]


_HIP = None


def hip_runtime():
    """the HIP runtime this process has loaded already (libnextsearch_hip.so links it), for the device buffers of the rank rows"""
    global _HIP
    if _HIP is None:
        nsbind.hip_lib()
        with open("/proc/self/maps") as f:
            path = next(line.split()[-1] for line in f if "libamdhip64" in line)
        _HIP = C.CDLL(path)
        _HIP.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP.hipFree.argtypes = [C.c_void_p]
    return _HIP


class DeviceArrays:
    """device copies of numpy arrays (hipMalloc / hipMemcpy); fetch(i) copies one back; always free()"""

    def __init__(self, *arrays):
        self.hip, self.host, self.ptr = hip_runtime(), [np.ascontiguousarray(a) for a in arrays], []
        for a in self.host:
            p = C.c_void_p()
            assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0
            self.ptr.append(p)
            assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0   # hipMemcpyHostToDevice

    def fetch(self, i):
        assert self.hip.hipDeviceSynchronize() == 0
        out = np.empty_like(self.host[i])
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptr[i], out.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        return out

    def free(self):
        for p in self.ptr:
            self.hip.hipFree(p)
        self.ptr = []


def merge_rank_rows(ctx, dev, n_ranks, n_queries, k, stride):
    """ns_merge_rank_rows on DeviceArrays(hits, nhits, found, seg_map or a dummy, out hits, out nhits, out found); stride 0: no seg_map"""
    p = dev.ptr
    return nsbind.hip_lib().ns_merge_rank_rows(ctx, p[0], p[1], p[2], n_ranks, n_queries, k, p[3] if stride else None, stride, p[4], p[5], p[6])


def run_rank_case(n_ranks, k, with_seg_map=True, ctx=None):
    """one synthetic case of join_shapes.rank_rows through ns_merge_rank_rows, checked against the numpy join: `found`, nhits,
    (score bits, global seg, doc) of every entry and the padding of the tail"""
    L = nsbind.hip_lib()
    own = ctx is None
    if own:
        ctx = C.c_void_p()
        assert L.ns_ctx_create(0, C.byref(ctx)) == 0
    dev = None
    try:
        hits, nhits, found, seg_map = join_shapes.rank_rows(n_ranks, k, with_seg_map=with_seg_map)
        want = join_ref.np_join(hits, nhits, found, seg_map, k)
        Q = nhits.shape[1]
        dev = DeviceArrays(hits, nhits, found, seg_map if with_seg_map else np.zeros(4, np.int32), np.full((Q, k, 3), 7, np.int32),
                           np.full(Q, 7, np.int32), np.full(Q, 7, np.int64))
        assert merge_rank_rows(ctx, dev, n_ranks, Q, k, seg_map.shape[1] if with_seg_map else 0) == 0, L.ns_last_error(ctx)
        oh, on, of = dev.fetch(4), dev.fetch(5), dev.fetch(6)
        for q, (rows, fsum) in enumerate(want):
            what = ("ranks", n_ranks, "k", k, "seg_map", with_seg_map, "query", q)
            assert int(of[q]) == fsum, what + ("found", int(of[q]), fsum)
            assert int(on[q]) == len(rows), what + ("nhits", int(on[q]), len(rows))
            got = [tuple(int(x) & 0xFFFFFFFF for x in oh[q, i]) for i in range(len(rows))]
            assert got == rows, what + (got[:6], rows[:6])
            tail = oh[q, len(rows):].view(np.uint32)
            assert np.all(tail[:, 0] == 0xFF800000) and np.all(tail[:, 1:] == 0xFFFFFFFF), what + ("padding",)
    finally:
        if dev:
            dev.free()
        if own:
            L.ns_ctx_destroy(ctx)


def reach():
    """counting build: {"families": {name: {...}}, "rank_join": {...}, "missed": {...}}"""
    ev = join_shapes.JOIN_EVENTS
    out = {"families": {}, "missed": {}}
    for name in join_shapes.FAMILIES:
        nsbind.debug_counters(reset=True)
        ran = run_family(name)
        c = nsbind.debug_counters(reset=True)[join_shapes.JOIN_GETTER]
        fam = join_shapes.FAMILIES[name]()
        named = {e: c[i] for e, i in ev.items()}
        want = predicted_path_counts(name, ran)
        out["families"][name] = {"events": named, "asserted": list(fam.events), "batches_at_k": ran, "predicted_path_queries": want}
        missed = [e for e in fam.events if named[e] == 0]
        if c[:4] != want:
            missed.append("per-path query counts %s, predicted %s" % (c[:4], want))
        if missed:
            out["missed"][name] = missed
        print("join", name, {e: named[e] for e in fam.events}, flush=True)
    nsbind.debug_counters(reset=True)
    run_rank_case(3, 10)
    c = nsbind.debug_counters(reset=True)[join_shapes.JOIN_GETTER]
    out["rank_join"] = {"events": {e: c[i] for e, i in ev.items()}, "queries": join_shapes.RANK_QUERIES}
    if c[ev["rank_join"]] != join_shapes.RANK_QUERIES or c[ev["rank_join_tie_rounds"]] == 0:
        out["missed"]["rank_join"] = [c[ev["rank_join"]], c[ev["rank_join_tie_rounds"]]]
    print("join rank rows", {e: c[ev[e]] for e in ("rank_join", "rank_join_tie_rounds")}, flush=True)
    return out
