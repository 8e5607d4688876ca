#!/usr/bin/env python3
"""Deleting documents timed on tools/ingest_bench.py's seeded corpus of about --mb MB as ONE segment (one
ns_forward_build: by 5j the arrays a compaction into one segment holds).  GPU box only.  Legs, alternating in one process,
medians and every single figure reported; all device times are the HIP events inside the calls (info.device_ms):
  merge       ns_forward_merge of the one source: the parent's unchanged path, the baseline
  keep_<p>    ns_forward_merge_keep of the same source with a seeded random bitmap that drops p % of the documents
              (p = 0: an all-ones bitmap, every stage of the filter runs and nothing goes)
  keep_<p>_full  only when the process runs on the variants build (NS_HIP_LIB=.../libnextsearch_hip_variants.so): the same
              with NS_KEEP_FULL_SEARCH set, every pair searches the whole document prefix instead of its tile's few
              documents (the A/B behind the product's one gather path; the product library has no such switch)
The filter's cost is keep - merge at p = 0; at p > 0 the later stages work on fewer pairs, so the difference mixes both.
--engine-mb > 0: an index of that many MB in one segment, Engine::delete_documents of 1 % of its documents, split into the
device part, the rest of the call (files) and a reload timed on its own.
--profile: warm-up and --reps calls of each kind only, for a `rocprofv3 --kernel-trace --stats` run of its own.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ingest_bench import corpus  # noqa: E402

RATES = (0, 1, 10, 50)                                                  # per cent of the documents dropped


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--engine-mb", type=int, default=0)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import nsbind
    L = nsbind.hip_lib()
    t0 = time.perf_counter()
    docs = corpus(args.mb << 20, 11)
    print(f"# generated {sum(len(d) for d in docs) / 1e6:.0f} MB in {len(docs)} documents, {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    ctx = C.c_void_p()
    if L.ns_ctx_create(0, C.byref(ctx)) != 0:
        sys.exit("no device: " + L.ns_last_error(None).decode())
    part = nsbind.forward_build(ctx, docs)
    text_mb = sum(len(d) for d in docs) / 1e6
    del docs
    n_docs, n_pairs = len(part["counts"]), len(part["pairs"])
    arr, alive = nsbind.forward_sources([part])
    rng = np.random.default_rng(5)
    keeps = {p: rng.random(n_docs) >= p / 100.0 for p in RATES}
    bits = {p: nsbind.keep_bitmaps([k]) for p, k in keeps.items()}
    info = nsbind.NsForwardInfo(struct_size=C.sizeof(nsbind.NsForwardInfo))

    def run(p, tiles=True):
        """p None: ns_forward_merge; else ns_forward_merge_keep with RATES' bitmap -> device ms, pairs, terms, call s"""
        h = C.c_void_p()
        if tiles:
            os.environ.pop("NS_KEEP_FULL_SEARCH", None)
        else:
            os.environ["NS_KEEP_FULL_SEARCH"] = "1"                     # read at every call by the variants build only
        t = time.perf_counter()
        rc = L.ns_forward_merge(ctx, arr, 1, C.byref(h)) if p is None else L.ns_forward_merge_keep(ctx, arr, bits[p][0], 1, C.byref(h))
        call_s = time.perf_counter() - t
        if rc != 0:
            sys.exit("merge: " + L.ns_last_error(ctx).decode())
        L.ns_forward_get_info(h, C.byref(info))
        out = {"ms": info.device_ms, "pairs": info.n_pairs, "terms": info.n_terms, "docs": info.kept_docs, "call_s": call_s, "device_bytes": info.device_bytes}
        L.ns_forward_destroy(h)
        return out

    ab = "variants" in os.path.basename(nsbind.HIP_LIB_PATH)
    kinds = [(None, True)] + [(p, True) for p in RATES] + ([(p, False) for p in RATES] if ab else [])
    for k in kinds:                                                     # warm-up: code objects, pool blocks
        run(*k)
    if args.profile:
        for _ in range(args.reps):
            for k in kinds[:1 + len(RATES)]:
                run(*k)
        print(json.dumps({"profile": True, "reps": args.reps, "pairs": n_pairs, "kinds": ["merge"] + ["keep_%d" % p for p in RATES]}))
        return
    res = {k: [] for k in kinds}
    for _ in range(args.reps):
        for k in kinds:
            res[k].append(run(*k))
    os.environ.pop("NS_KEEP_FULL_SEARCH", None)
    L.ns_ctx_destroy(ctx)
    med = statistics.median
    base_ms = med([r["ms"] for r in res[(None, True)]])
    base_call = med([r["call_s"] for r in res[(None, True)]])
    out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "text_mb": text_mb, "docs": n_docs, "terms": len(part["terms"]), "pairs": n_pairs, "reps": args.reps,
           "merge": {"ms": summary([r["ms"] for r in res[(None, True)]]), "call_s": summary([r["call_s"] for r in res[(None, True)]]), "host_and_upload_s": base_call - base_ms * 1e-3,
                     "what": "ns_forward_merge of the one source: the unchanged path, the baseline"}}
    for p in RATES:
        on = res[(p, True)]
        ms = med([r["ms"] for r in on])
        surv = on[0]["pairs"]
        out["keep_%d" % p] = {"dropped_percent": p, "docs_out": on[0]["docs"], "pairs_out": surv, "terms_out": on[0]["terms"],
                              "ms": summary([r["ms"] for r in on]), "call_s": summary([r["call_s"] for r in on]),
                              "ms_minus_merge": ms - base_ms, "ms_over_merge": ms / base_ms, "device_bytes": on[0]["device_bytes"],
                              # the host's walk over counts and bitmaps and the extra uploads lie outside the HIP events: they show here
                              "call_s_minus_merge": med([r["call_s"] for r in on]) - base_call, "host_and_upload_s": med([r["call_s"] for r in on]) - ms * 1e-3}
        if ab:
            off = res[(p, False)]
            out["keep_%d" % p].update(ms_full_search=summary([r["ms"] for r in off]), full_search_over_tiles=med([r["ms"] for r in off]) / ms)
    k0 = out["keep_0"]
    filt_ms = k0["ms_minus_merge"]
    out["filter"] = {"what": "keep_0 - merge: every stage of the filter with nothing dropped, so that the later stages do the baseline's work",
                     "ms": filt_ms, "algorithmic_bytes_per_surviving_pair": 16,
                     "effective_GBps_if_16B_per_pair": 16.0 * n_pairs / (filt_ms * 1e-3) / 1e9 if filt_ms > 0 else None,
                     "equivalent_bytes_per_pair_at_4TBps": filt_ms * 1e-3 * 4e12 / n_pairs,
                     "note": "time-derived figures: no memory counters were collected for this file"}
    out["same_as_merge_when_nothing_is_dropped"] = k0["pairs_out"] == n_pairs and k0["terms_out"] == len(part["terms"]) and k0["docs_out"] == n_docs
    if args.engine_mb:
        out["engine"] = engine_leg(nsbind, args)
    print(json.dumps(out))


def engine_leg(nsbind, args):
    docs = corpus(args.engine_mb << 20, 11)
    tmp = tempfile.mkdtemp(prefix="ns_delete_idx_")
    try:
        index = os.path.join(tmp, "index")
        os.makedirs(index)
        eng = nsbind.Engine.create(index, 0)
        eng.add_documents([(b"u%d" % j, b"t", b"p", d) for j, d in enumerate(docs)])
        rng = np.random.default_rng(9)
        victims = [b"u%d" % int(j) for j in np.flatnonzero(rng.random(len(docs)) < 0.01)]
        t = time.perf_counter()
        st = eng.delete_documents(victims)
        wall = time.perf_counter() - t
        t = time.perf_counter()
        eng.reload()
        reload_s = time.perf_counter() - t
        eng.close()
        device_s = (st["merge_ms"] + st["invert_ms"]) * 1e-3
        return {"text_mb": args.engine_mb, "docs": len(docs), "uids": len(victims), "stats": st, "wall_s": wall,
                "device_s": device_s, "copies_s": st["call_s"] - device_s, "reload_s_timed_alone": reload_s,
                "files_s": st["total_s"] - st["call_s"] - reload_s,
                "what": "device: HIP events of ns_forward_merge_keep + ns_forward_invert; copies: the rest of the two calls and the fetch; reload: a second reload() of the same index timed on its own; files: total - call - reload (reading the four forward files, writing the segment, the manifest, removing the old directory)"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
