#!/usr/bin/env python3
"""Related terms timed on tools/ingest_bench.py's seeded corpus of about --mb MB as ONE segment (one
Engine::add_documents).  GPU box only.  Writes <out-dir>/related_bench_<mb>mb_<library>_w<log2 W>.json (default out-dir
profiles/related) and prints the same JSON line.  The rows are the top 100 of a search batch of --queries two-word queries.
  (a) ns_docterms_aggregate over the rows, HIP events inside the call: device ms, rows/s and pairs/s (the forward pairs of the
      rows' distinct documents); the same rows by the one-thread host rule (nsh_related_aggregate_host), compared bit for bit;
      ns_docterms_select over the same documents, which reads the same pairs: the natural yardstick.
  (b) one Engine::related_terms to JSON, median over --latency-reps queries (search, aggregate, merge, JSON).
The W A/B: run it once on the product library and once on the variants build with NS_TERMS_WINDOW_15=1 (--part aggregate)."""
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from ingest_bench import corpus  # noqa: E402
import invert_oracle  # noqa: E402


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--queries", type=int, default=512)
    ap.add_argument("--latency-reps", type=int, default=100)
    ap.add_argument("--part", choices=("all", "aggregate"), default="all")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "related"))
    args = ap.parse_args()
    import nsbind
    L = nsbind.hip_lib()
    W = int(L.ns_docterms_window())
    t0 = time.perf_counter()
    docs = corpus(args.mb << 20, 11)
    text_mb = sum(len(d) for d in docs) / 1e6
    print(f"# generated {text_mb:.0f} MB in {len(docs)} documents, {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    tmp = tempfile.mkdtemp(prefix="ns_related_idx_")
    try:
        index = os.path.join(tmp, "index")
        os.makedirs(index)
        eng = nsbind.Engine.create(index, 0)
        t0 = time.perf_counter()
        eng.add_documents([(b"u%d" % j, b"t", b"p", d) for j, d in enumerate(docs)])
        print(f"# indexed in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        del docs
        seg = os.path.join(index, "segments", eng.segment_name(0))
        counts, pairs = invert_oracle.read_forward(os.path.join(seg, "forward.bin"))
        terms = invert_oracle.read_terms(os.path.join(seg, "terms.bin"))
        part = {"counts": counts, "pairs": pairs}
        df, idf = eng.similar_term_stats(0)
        n_docs, n_pairs = len(counts), len(pairs)
        # two-word queries of middling df; the rows are their top 100
        rng = np.random.default_rng(5)
        mid = np.flatnonzero((df >= max(20, n_docs // 2000)) & (df <= max(40, n_docs // 50)))
        picks = rng.choice(mid, (args.queries, 2))
        queries = [(terms[a] + b" " + terms[b]).decode() for a, b in picks.tolist()]
        h, n, _, _ = eng.search_batch(queries, 100)
        rows = [h["doc"][q, :int(n[q])].astype(np.uint32).tolist() for q in range(len(queries))]
        row_pairs = int(sum(int(counts[np.unique(r)].sum()) for r in rows if len(r)))
        out = {"library": os.path.basename(nsbind.HIP_LIB_PATH), "window": W, "text_mb": text_mb, "docs": n_docs, "terms": len(df), "pairs": n_pairs,
               "reps": args.reps, "rows": len(rows), "docs_per_row": sum(len(r) for r in rows) / len(rows), "pairs_of_the_rows": row_pairs,
               "windows_per_row": (len(df) + W - 1) // W}
        ctx = C.c_void_p()
        if L.ns_ctx_create(0, C.byref(ctx)) != 0:
            sys.exit("no device: " + L.ns_last_error(None).decode())
        dt = nsbind.DocTerms(ctx, part, df, idf)
        first = dt.aggregate(rows, 10)                                   # warm-up: code objects, pool block, the handle's order check
        ms, call = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            got = dt.aggregate(rows, 10)
            call.append(time.perf_counter() - t0)
            ms.append(got[5])
        med = statistics.median(ms) * 1e-3
        out["aggregate"] = {"what": "ns_docterms_aggregate over the rows, T = 10, default options; device ms = HIP events around k_ta_count",
                            "first_call_device_ms": first[5], "device_ms": summary(ms), "call_s": summary(call), "rows_per_s": len(rows) / med, "pairs_per_s": row_pairs / med}
        if args.part == "all":
            t0 = time.perf_counter()
            host = nsbind.related_aggregate_host(part, df, idf, rows, 10)
            host_s = time.perf_counter() - t0
            same = all(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)) for a, b in zip(got[:5], host))
            ids = np.concatenate([np.unique(r) for r in rows if len(r)]).astype(np.uint32)
            dt.select(ids, 25)
            sel = [dt.select(ids, 25, garbage=False)[3] for _ in range(args.reps)]
            out["aggregate"].update({"host_one_thread_s": host_s, "host_pairs_per_s": row_pairs / host_s, "device_over_host": host_s / med,
                                     "call_over_host": host_s / statistics.median(call), "equals_host_rule": bool(same)})
            out["select_yardstick"] = {"what": "ns_docterms_select (T = 25) over the rows' distinct documents: the same pairs read once, no counting",
                                       "documents": len(ids), "device_ms": summary(sel), "aggregate_over_select": med / (statistics.median(sel) * 1e-3)}
        dt.close()
        L.ns_ctx_destroy(ctx)
        if args.part == "all":
            eng.related_terms_json(queries[0])
            lat = []
            for q in queries[:args.latency_reps]:
                t0 = time.perf_counter()
                eng.related_terms_json(q)
                lat.append(time.perf_counter() - t0)
            out["latency"] = {"what": "one Engine::related_terms(query) to JSON: the search with K = 100, one aggregate row, the merge",
                              "ms": {"median": statistics.median(lat) * 1e3, "min": min(lat) * 1e3, "max": max(lat) * 1e3, "n": len(lat)}}
        eng.close()
        os.makedirs(args.out_dir, exist_ok=True)
        name = "related_bench_%dmb_%s_w%d.json" % (args.mb, out["library"].replace("libnextsearch_hip", "lib").replace(".so", ""), W.bit_length() - 1)
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
