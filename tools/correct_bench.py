#!/usr/bin/env python3
"""Spelling correction throughput and latency on the device (ns_ac_fuzzy / Engine::correct_batch / Engine::did_you_mean,
csrc/ns_fuzzy.hip).  One JSON line per (workload, prefix_len) into profiles/correct/correct_bench.jsonl.

Workloads, 16384 misspelt tokens each (a term drawn by score, 1-2 random edits), auto edits, L = 5, prefix_len 0 and 1:
  cfg5    the engine on cfg5's index (1 segment x 1M docs, 65536 equal-length terms): neither the length window nor the
          signature helps much; also one Engine::did_you_mean to JSON (median / p99)
  words   a raw table of about 1.1M generated pseudo-words of 3-14 bytes with Zipf scores (ns_ac_* on a context)
Reported: batch host -> host (median of --repeats calls), kernel time from events, candidate pairs per second
(Q x n / kernel time), the share of (query, candidate-in-window) pairs that reach the DP (counted by the host baseline,
which applies the same filters), ns_ac_build_fuzzy time and bytes, and the A/B signature filter on / off (alternating).
Yardstick: tools/correct_host_baseline.cpp (-O2, one thread) on the same workload; its answers must equal the device's.

    python tools/correct_bench.py [--repeats 20] [--workload cfg5|words|all] [--batch 16384] [--baseline-queries 0]
Kernel times for a trace (a run of its own): rocprofv3 --kernel-trace --stats -d DIR -- python tools/correct_bench.py --repeats 5
"""
import argparse
import ctypes as C
import json
import os
import random
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nsbind  # noqa: E402
import correct_ref  # noqa: E402

_SYL = [b"ka", b"to", b"mi", b"ren", b"sol", b"va", b"qu", b"el", b"dor", b"bi", b"nu", b"sha", b"pe", b"lim", b"ox", b"ra", b"zen", b"fu", b"gi",
        b"cor", b"vi", b"rus", b"an", b"ti", b"ge", b"no", b"me", b"pro", b"te", b"in", b"mu", b"ne", b"lo", b"gy", b"ph", b"st", b"ch", b"19"]


def pct(xs, q):
    return float(np.percentile(np.asarray(xs), q))


def pseudo_words(n, seed):
    rng = random.Random(seed)
    out = set()
    while len(out) < n:
        w = b"".join(rng.choice(_SYL) for _ in range(rng.randint(2, 6)))
        if 3 <= len(w) <= 14:
            out.add(w)
    terms = sorted(out)
    ranks = np.random.default_rng(seed).permutation(n) + 1
    return terms, np.maximum(1, (2_000_000 / ranks).astype(np.int64)).astype(np.uint32)


def misspelt(terms, scores, n, seed):
    rng = random.Random(seed)
    w = np.asarray(scores, dtype=np.float64) + 1.0
    pick = np.random.default_rng(seed).choice(len(terms), size=n, p=w / w.sum())
    alphabet = b"abcdefghijklmnopqrstuvwxyz0123456789"
    return [correct_ref.random_edits(rng, terms[int(i)], rng.randint(1, 2), alphabet) for i in pick]


def write_workload(path, terms, scores, queries, edits, L, prefix_len):
    offs = np.zeros(len(terms) + 1, np.uint64)
    offs[1:] = np.cumsum([len(t) for t in terms])
    qo = np.zeros(len(queries) + 1, np.uint32)
    qo[1:] = np.cumsum([len(t) for t in queries])
    with open(path, "wb") as f:
        f.write(struct.pack("<4I", len(terms), len(queries), L, prefix_len))
        f.write(offs.tobytes() + b"".join(terms) + np.asarray(scores, np.uint32).tobytes())
        f.write(qo.tobytes() + b"".join(queries) + np.asarray(edits, np.uint8).tobytes())


def host_baseline(exe, tmp, terms, scores, queries, edits, L, prefix_len, idx, dist, cnt):
    """runs the one-thread host program; its answers must equal the device's rows for the same queries"""
    w, a = os.path.join(tmp, "workload.bin"), os.path.join(tmp, "answers.bin")
    write_workload(w, terms, scores, queries, edits, L, prefix_len)
    line = json.loads(subprocess.run([exe, w, a], check=True, capture_output=True, text=True).stdout)
    raw = open(a, "rb").read()
    Q = len(queries)
    h_idx = np.frombuffer(raw[:Q * L * 4], np.uint32).reshape(Q, L)
    h_dist = np.frombuffer(raw[Q * L * 4:Q * L * 5], np.uint8).reshape(Q, L)
    h_cnt = np.frombuffer(raw[Q * L * 5:], np.uint32)
    assert np.array_equal(h_idx, idx[:Q]) and np.array_equal(h_dist, dist[:Q]) and np.array_equal(h_cnt, cnt[:Q]), "host baseline != device"
    return line


def measure(call, repeats):
    """call() -> (idx, dist, cnt, kernel ms); warm-up, then timed calls whose outputs must equal the first call's"""
    first = call()
    for _ in range(2):
        call()
    secs, kms = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        got = call()
        secs.append(time.perf_counter() - t0)
        kms.append(got[3])
        assert all(np.array_equal(x, y) for x, y in zip(got[:3], first[:3]))
    return first, secs, kms


def sig_ab(call, repeats):
    """signature filter on / off, alternating order; kernel ms medians"""
    on, off = [], []
    for r in range(repeats):
        for flag in ((0, 1) if r % 2 == 0 else (1, 0)):
            os.environ["NS_FUZZY_NO_SIG"] = str(flag)
            (off if flag else on).append(call()[3])
    os.environ["NS_FUZZY_NO_SIG"] = "0"
    return {"kernel_ms_sig_on": round(pct(on, 50), 4), "kernel_ms_sig_off": round(pct(off, 50), 4)}


def report(name, prefix_len, n_terms, queries, first, secs, kms, base, extra):
    Q = len(queries)
    k_s = pct(kms, 50) / 1e3
    out = {"workload": name, "prefix_len": prefix_len, "table_terms": n_terms, "batch": Q, "limit": 5, "max_edits": "auto",
           "repeats": len(secs), "batch_ms_median": round(pct(secs, 50) * 1e3, 4), "batch_ms_min": round(min(secs) * 1e3, 4),
           "kernel_ms_median": round(k_s * 1e3, 4), "answers_per_batch": int(first[2].sum()),
           "pairs_per_s_device": float("%.4g" % (Q * n_terms / k_s)) if k_s > 0 else None}
    if base:
        bq = base["n_q"]
        host_rate = bq * n_terms / base["scan_s"]
        out.update({"host_baseline_queries": bq, "host_baseline_scan_s": base["scan_s"], "pairs_per_s_host_1_thread": float("%.4g" % host_rate),
                    "window_pairs_share": round(base["pairs"] / (bq * n_terms), 5), "dp_share_of_window_pairs": round(base["reached_dp"] / max(base["pairs"], 1), 5),
                    "dp_share_of_all_pairs": round(base["reached_dp"] / (bq * n_terms), 6), "candidates": base["candidates"],
                    "device_over_host_1_thread": round(out["pairs_per_s_device"] / host_rate, 2),
                    "device_over_16_host_threads_worth": round(out["pairs_per_s_device"] / host_rate / 16, 2),
                    "outputs_checked": "every timed call == first call; host baseline answers == device answers"})
    out.update(extra)
    return out


def run_cfg5(args, tmp, exe):
    d = os.path.join(tmp, "cfg5")
    nsbind.gen_index(d, 1, args.cfg5_docs, 65536, 1337, False)
    eng = nsbind.Engine(d, 0)
    terms, scores, _ = eng.suggest_table()
    queries = misspelt(terms, scores, args.batch, 11)
    edits = [correct_ref.auto_edits(len(t)) for t in queries]
    flat = nsbind.flat_inputs(queries)
    eng.correct_batch_raw(queries[:1], 5)
    build_ms = eng.correct_build_ms()
    for prefix_len in (0, 1):
        call = lambda: eng.correct_batch_raw(queries, 5, -1, prefix_len, flat)   # noqa: E731
        first, secs, kms = measure(call, args.repeats)
        bq = args.baseline_queries or len(queries)
        base = host_baseline(exe, tmp, terms, scores, queries[:bq], edits[:bq], 5, prefix_len, *first[:3]) if exe else None
        extra = {"build_fuzzy_ms_first_call": round(build_ms, 3), "build_fuzzy_bytes": (base["candidates"] * 12 + 69 * 4) if base else None}
        extra.update(sig_ab(call, max(4, args.repeats // 2)))
        if prefix_len == 0 and args.latency:
            lat = []
            for i in range(min(args.latency, len(queries) - 1)):
                x = queries[i] + b" " + queries[i + 1]
                t0 = time.perf_counter()
                eng.did_you_mean_json(x, 5)
                lat.append((time.perf_counter() - t0) * 1e6)
            lat = lat[len(lat) // 10:]
            extra.update({"did_you_mean_us_median": round(pct(lat, 50), 2), "did_you_mean_us_p99": round(pct(lat, 99), 2)})
        yield report("cfg5", prefix_len, len(terms), queries, first, secs, kms, base, extra)
    eng.close()


def run_words(args, tmp, exe):
    terms, scores = pseudo_words(args.words, 7)
    queries = misspelt(terms, scores, args.batch, 12)
    edits = np.array([correct_ref.auto_edits(len(t)) for t in queries], dtype=np.uint8)
    ctx = C.c_void_p()
    assert nsbind.hip_lib().ns_ctx_create(0, C.byref(ctx)) == 0
    ac = nsbind.AcTable(ctx, terms, scores)
    assert ac.rc == 0
    rc, build_ms = ac.build_fuzzy()
    assert rc == 0
    for prefix_len in (0, 1):
        call = lambda: ac.fuzzy(queries, edits, prefix_len, 5)   # noqa: E731
        first, secs, kms = measure(call, args.repeats)
        bq = args.baseline_queries or len(queries)
        base = host_baseline(exe, tmp, terms, scores, queries[:bq], edits[:bq], 5, prefix_len, *first[:3]) if exe else None
        extra = {"build_fuzzy_kernel_ms": round(build_ms, 3), "build_fuzzy_bytes": (base["candidates"] * 12 + 69 * 4) if base else None}
        extra.update(sig_ab(call, max(4, args.repeats // 2)))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correct", "correct_bench.jsonl"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="ns_correct_bench_") as tmp:
        exe = None
        if not args.no_baseline:
            exe = os.path.join(tmp, "correct_host_baseline")
            subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "correct_host_baseline.cpp")], check=True)
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
