#!/usr/bin/env python3
"""Typo-tolerant completion throughput and latency on the device (ns_ac_fuzzy_prefix / Engine::complete_batch /
Engine::complete, csrc/ns_fuzzy.hip k_fp_*).  One JSON line per (workload, prefix_len) appended to
profiles/complete/complete_bench.jsonl.

Workloads: tools/correct_bench.py's two, typed only in part: each of its 16384 misspelt tokens (a term drawn by score, 1-2
random edits) is cut after 3 to 8 bytes; auto edits, L = 5, prefix_len 0 and 1:
  cfg5    the engine on cfg5's index (1 segment x 1M docs, 65536 equal-length terms); also one Engine::complete to JSON
          (median / p99)
  words   a raw table of about 1.1M generated pseudo-words of 3-14 bytes with Zipf scores (ns_ac_* on a context)
Reported: batch host -> host (median of --repeats calls), kernel time from events, candidates per second (the (query,
candidate) pairs inside the length window and the fixed prefix's range, counted by the host baseline, over the kernel
time), the share of them that reaches the DP, and the A/B signature filter on / off (alternating order).
Yardstick: tools/complete_host_baseline.cpp (-O2, one thread; make -C nextsearch-api_amd complete_host_baseline) on the
same workload; its answers must equal the device's.

    python tools/complete_bench.py [--repeats 20] [--workload cfg5|words|all] [--batch 16384] [--baseline-queries 0]
"""
import argparse
import ctypes as C
import json
import os
import random
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import nsbind  # noqa: E402
import correct_ref  # noqa: E402
import correct_bench as cb  # noqa: E402


def typed(terms, scores, n, seed):
    """correct_bench's misspelt tokens, each cut after 3..8 bytes"""
    rng = random.Random(seed)
    return [t[:rng.randint(3, 8)] for t in cb.misspelt(terms, scores, n, seed)]


def report(name, prefix_len, n_terms, queries, first, secs, kms, base, extra):
    Q = len(queries)
    k_s = cb.pct(kms, 50) / 1e3
    out = {"workload": name, "prefix_len": prefix_len, "table_terms": n_terms, "batch": Q, "limit": 5, "max_edits": "auto",
           "repeats": len(secs), "batch_ms_median": round(cb.pct(secs, 50) * 1e3, 4), "batch_ms_min": round(min(secs) * 1e3, 4),
           "kernel_ms_median": round(k_s * 1e3, 4), "answers_per_batch": int(first[2].sum())}
    if base:
        bq = base["n_q"]
        pairs_batch = base["pairs"] * Q / bq                  # the baseline may have been given the first bq queries only
        out.update({"host_baseline_queries": bq, "host_baseline_scan_s": base["scan_s"], "candidates_per_query": round(base["pairs"] / bq, 1),
                    "candidates_per_s_device": float("%.4g" % (pairs_batch / k_s)) if k_s > 0 else None,
                    "candidates_per_s_host_1_thread": float("%.4g" % (base["pairs"] / base["scan_s"])) if base["scan_s"] > 0 else None,
                    "dp_share_of_candidates": round(base["reached_dp"] / max(base["pairs"], 1), 5), "table_candidates": base["candidates"],
                    "outputs_checked": "every timed call == first call; host baseline answers == device answers"})
    out.update(extra)
    return out


def run_cfg5(args, tmp, exe):
    d = os.path.join(tmp, "cfg5")
    nsbind.gen_index(d, 1, args.cfg5_docs, 65536, 1337, False)
    eng = nsbind.Engine(d, 0)
    terms, scores, _ = eng.suggest_table()
    inputs = typed(terms, scores, args.batch, 11)
    edits = [correct_ref.auto_edits(len(t)) for t in inputs]
    flat = nsbind.flat_inputs(inputs)
    eng.complete_batch_raw(inputs[:1], 5)
    for prefix_len in (0, 1):
        def call():
            idx, dist, cnt, _, ms = eng.complete_batch_raw(inputs, 5, -1, prefix_len, flat)
            return idx, dist, cnt, ms
        first, secs, kms = cb.measure(call, args.repeats)
        bq = args.baseline_queries or len(inputs)
        base = cb.host_baseline(exe, tmp, terms, scores, inputs[:bq], edits[:bq], 5, prefix_len, *first[:3]) if exe else None
        extra = cb.sig_ab(call, max(4, args.repeats // 2))
        if prefix_len == 1 and args.latency:   # Engine::complete fixes the first byte
            lat = []
            for i in range(min(args.latency, len(inputs) - 1)):
                x = inputs[i + 1] + b" " + inputs[i]
                t0 = time.perf_counter()
                eng.complete_json(x, 5)
                lat.append((time.perf_counter() - t0) * 1e6)
            lat = lat[len(lat) // 10:]
            extra.update({"complete_us_median": round(cb.pct(lat, 50), 2), "complete_us_p99": round(cb.pct(lat, 99), 2)})
        yield report("cfg5", prefix_len, len(terms), inputs, first, secs, kms, base, extra)
    eng.close()


def run_words(args, tmp, exe):
    terms, scores = cb.pseudo_words(args.words, 7)
    queries = typed(terms, scores, args.batch, 12)
    edits = np.array([correct_ref.auto_edits(len(t)) for t in queries], dtype=np.uint8)
    ctx = C.c_void_p()
    assert nsbind.hip_lib().ns_ctx_create(0, C.byref(ctx)) == 0
    ac = nsbind.AcTable(ctx, terms, scores)
    assert ac.rc == 0
    rc, build_ms = ac.build_fuzzy()
    assert rc == 0
    for prefix_len in (0, 1):
        call = lambda: ac.fuzzy_prefix(queries, edits, prefix_len, 5)   # noqa: E731
        first, secs, kms = cb.measure(call, args.repeats)
        bq = args.baseline_queries or len(queries)
        base = cb.host_baseline(exe, tmp, terms, scores, queries[:bq], edits[:bq], 5, prefix_len, *first[:3]) if exe else None
        extra = {"build_fuzzy_kernel_ms": round(build_ms, 3)}
        extra.update(cb.sig_ab(call, max(4, args.repeats // 2)))
        yield report("words", prefix_len, len(terms), queries, first, secs, kms, base, extra)
    ac.close()
    nsbind.hip_lib().ns_ctx_destroy(ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--latency", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--words", type=int, default=1_100_000)
    ap.add_argument("--cfg5-docs", type=int, default=1_000_000)
    ap.add_argument("--baseline-queries", type=int, default=0, help="queries given to the host baseline (0 = the whole batch)")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--workload", default="all", choices=["all", "cfg5", "words"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complete", "complete_bench.jsonl"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="ns_complete_bench_") as tmp:
        exe = None
        if not args.no_baseline:
            exe = os.path.join(ROOT, "nextsearch-api_amd", "complete_host_baseline")
            if not os.path.exists(exe):
                subprocess.run(["make", "-C", os.path.join(ROOT, "nextsearch-api_amd"), "complete_host_baseline"], check=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            for name, run in (("cfg5", run_cfg5), ("words", run_words)):
                if args.workload in ("all", name):
                    for line in run(args, tmp, exe):
                        print(json.dumps(line), flush=True)
                        f.write(json.dumps(line) + "\n")
                        f.flush()


if __name__ == "__main__":
    main()
