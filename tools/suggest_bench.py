#!/usr/bin/env python3
"""Autocomplete throughput and latency on the device (Engine::suggest_batch / Engine::suggest, csrc/ns_suggest.hip).

Workload: a batch of 16384 requests whose prefixes (1-8 bytes) are cut from terms drawn in proportion to their score
(df), about 20 % of them behind a multi-word base.  Two indexes: cfg5's (1 segment x 1M docs, 65536 terms) and a
generated index with more than 1M distinct lexicon terms.  Per index, one JSON line with
  * suggestions/s (and requests/s) host -> host through the batch API, median of --repeats timed calls;
  * the kernel's time per batch (device events around k_ac_suggest, median);
  * the latency of one Engine::suggest (JSON text) request, median and p99;
  * the table build inside reload() (host sums, normalising, sort) and its upload + device tree build.
Every timed call's outputs are compared with the first call's, and a sample with the Python restatement.

    python tools/suggest_bench.py [--repeats 20] [--latency 2000] [--index cfg5|big|all]
Kernel times for a trace: rocprofv3 --kernel-trace --stats -d DIR -- python tools/suggest_bench.py --repeats 5 --latency 0
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nsbind  # noqa: E402
import suggest_ref  # noqa: E402

# name: (n_segments, docs_per_segment, vocab)
INDEXES = {
    "cfg5": (1, 1_000_000, 65536),
    "big": (1, 50_000, 1_100_000),
}
_WORDS = [b"new", b"The", b"what is", b"covid", b"Latest", b"how to", b"vaccine for"]


def workload(terms, scores, n, seed):
    """n request inputs: a term drawn by score (df + 1), a 1-8 byte prefix of it; ~20 % behind a multi-word base"""
    rng = random.Random(seed)
    w = np.asarray(scores, dtype=np.float64) + 1.0
    pick = np.random.default_rng(seed).choice(len(terms), size=n, p=w / w.sum())
    out = []
    for i in pick:
        t = terms[int(i)]
        p = t[:rng.randint(1, min(8, len(t)))]
        if rng.random() < 0.2:
            p = b" ".join(rng.sample(_WORDS, rng.randint(1, 2))) + b" " + p
        out.append(p)
    return out


def pct(xs, q):
    return float(np.percentile(np.asarray(xs), q))


def run_index(name, args, tmp):
    nseg, docs, vocab = INDEXES[name]
    d = os.path.join(tmp, name)
    t0 = time.perf_counter()
    nsbind.gen_index(d, nseg, docs, vocab, 1337, False)
    gen_s = time.perf_counter() - t0
    eng = nsbind.Engine(d, 0)
    terms, scores, build_ms = eng.suggest_table()
    # reload() again (warm page cache, code objects loaded): the build and upload times of a steady reload
    eng.reload()
    terms, scores, build_ms = eng.suggest_table()
    t0 = time.perf_counter()
    eng.reload()
    reload_ms = (time.perf_counter() - t0) * 1e3
    terms, scores, _ = eng.suggest_table()
    build_ms2, upload_ms = eng.suggest_build_times()
    scores = [int(s) for s in scores]
    ins = workload(terms, scores, args.batch, 11)
    L = 5

    # batch: warm-up, then timed calls; outputs compared with the first call's and (sample) with the restatement
    idx0, cnt0, base0, _ = eng.suggest_batch_raw(ins, L)
    for q in range(0, len(ins), max(1, len(ins) // 500)):
        want = suggest_ref.suggest(terms, scores, ins[q], L)
        got = [ins[q][:int(base0[q])] + terms[int(i)] for i in idx0[q, :int(cnt0[q])]]
        assert got == want, (ins[q], got, want)
    flat = nsbind.flat_inputs(ins)   # the batch as the C API takes it: bytes + offsets, built once
    for _ in range(3):
        eng.suggest_batch_raw(ins, L, flat)
    secs, kms = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        idx, cnt, base, ms = eng.suggest_batch_raw(ins, L, flat)
        secs.append(time.perf_counter() - t0)
        kms.append(ms)
        assert np.array_equal(idx, idx0) and np.array_equal(cnt, cnt0) and np.array_equal(base, base0)
    n_sugg = int(cnt0.sum())
    med = pct(secs, 50)

    # one request: Engine::suggest (JSON text), host clock around the synchronous call
    lat = []
    for i in range(min(args.latency, len(ins))):
        x = ins[i]
        t0 = time.perf_counter()
        eng.suggest_json(x, L)
        lat.append((time.perf_counter() - t0) * 1e6)
    lat = lat[len(lat) // 10:]   # the first tenth is warm-up
    eng.close()
    return {
        "index": name, "n_segments": nseg, "docs_per_segment": docs, "vocab": vocab, "table_terms": len(terms),
        "gen_index_s": round(gen_s, 2), "batch": len(ins), "limit": L, "suggestions_per_batch": n_sugg,
        "repeats": args.repeats,
        "batch_ms_median": round(med * 1e3, 4), "batch_ms_min": round(min(secs) * 1e3, 4),
        "batch_ms_p90": round(pct(secs, 90) * 1e3, 4),
        "requests_per_s": round(len(ins) / med, 1), "suggestions_per_s": round(n_sugg / med, 1),
        "kernel_ms_median": round(pct(kms, 50), 4),
        "single_request_us_median": round(pct(lat, 50), 2) if lat else None,
        "single_request_us_p99": round(pct(lat, 99), 2) if lat else None,
        "table_build_ms": round(build_ms2, 2), "table_upload_and_tree_ms": round(upload_ms, 2),
        "reload_ms_whole_index": round(reload_ms, 1),
        "outputs_checked": "every timed call == first call; sampled rows == Python restatement",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--latency", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--index", default="all", choices=["all"] + list(INDEXES))
    args = ap.parse_args()
    names = list(INDEXES) if args.index == "all" else [args.index]
    with tempfile.TemporaryDirectory(prefix="ns_suggest_bench_") as tmp:
        for name in names:
            print(json.dumps(run_index(name, args, tmp)), flush=True)


if __name__ == "__main__":
    main()
