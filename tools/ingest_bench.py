#!/usr/bin/env python3
"""Indexing: document texts -> forward index on the device (ns_forward_build), timed on a seeded corpus of
about --mb MB next to the project's own single-thread host path (tools/ingest_host_baseline.cpp: host/textutil.hpp's
tokeniser + a hash map, compiled here with g++).  GPU box only.  Device and host runs alternate; medians are reported.
Prints one JSON line: MB/s of text and M tokens/s for the device part (HIP events, upload excluded), for the whole call
(upload, device part, result fetch) and for the host path, and whether both produced the same (doc, term, tf) sum."""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd"))

STOP = b"the a an and or of to in for on with by as is are was were be been it this that from at".split()
SEPS = [b" ", b" ", b" ", b" ", b" ", b", ", b". ", b"\n", b"-", b" (", b") ", b"\xc3\xa9 "]


def corpus(n_bytes, seed, doc_bytes=4096, vocab=200_000):
    """Seeded Zipf text, assembled with numpy: -> list of documents (bytes) of about doc_bytes each, n_bytes in all"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)
    words = []
    for i in range(vocab):
        if i % 4 == 1 and i // 4 < len(STOP):
            w = STOP[i // 4]
        else:
            w = bytes(rng.choice(letters, int(rng.integers(2, 12))))
            if i % 11 == 0:
                w = w.capitalize()
        words.append(w + SEPS[i % len(SEPS)])
    pool = np.frombuffer(b"".join(words), dtype=np.uint8)
    wlen = np.asarray([len(w) for w in words], dtype=np.int64)
    wstart = np.concatenate([[0], np.cumsum(wlen)[:-1]])
    docs, done = [], 0
    while done < n_bytes:
        want = min(64 << 20, n_bytes - done)
        ranks = np.minimum(rng.zipf(1.15, want // 5) - 1, vocab - 1)
        lens = wlen[ranks]
        ends = np.cumsum(lens)
        cut = int(np.searchsorted(ends, want)) + 1
        ranks, lens, ends = ranks[:cut], lens[:cut], ends[:cut]
        total = int(ends[-1])
        idx = np.repeat(wstart[ranks] - (ends - lens), lens) + np.arange(total, dtype=np.int64)
        chunk = pool[idx].tobytes()
        for at in range(0, total, doc_bytes):
            docs.append(chunk[at:at + doc_bytes])          # (a cut inside a word: the document boundary separates)
        done += total
    return docs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    args = ap.parse_args()
    import nsbind
    L = nsbind.hip_lib()
    t0 = time.perf_counter()
    docs = corpus(args.mb << 20, 11)
    blob = b"".join(docs)
    offs = np.zeros(len(docs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.fromiter((len(d) for d in docs), dtype=np.uint64, count=len(docs)))
    print(f"# generated {len(blob) / 1e6:.0f} MB in {len(docs)} documents in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    tmp = tempfile.mkdtemp(prefix="ns_ingest_")
    exe, tf = os.path.join(tmp, "ingest_host_baseline"), os.path.join(tmp, "texts.bin")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "nextsearch-api_amd", "host"),
                           os.path.join(ROOT, "tools", "ingest_host_baseline.cpp"), "-o", exe])
    with open(tf, "wb") as f:
        f.write(struct.pack("<I", len(docs)))
        for d in docs:
            f.write(struct.pack("<I", len(d)))
            f.write(d)
    del docs
    ctx = C.c_void_p()
    if L.ns_ctx_create(0, C.byref(ctx)) != 0:
        sys.exit("no device: " + L.ns_last_error(None).decode())

    def device_run():
        h = C.c_void_p()
        t = time.perf_counter()
        rc = L.ns_forward_build(ctx, blob, len(blob), offs.ctypes.data, len(offs) - 1, C.byref(h))
        if rc != 0:
            sys.exit("ns_forward_build: " + L.ns_last_error(ctx).decode())
        t_build = time.perf_counter() - t
        info = nsbind.NsForwardInfo(struct_size=C.sizeof(nsbind.NsForwardInfo))
        L.ns_forward_get_info(h, C.byref(info))
        kept, dl, cnt = (np.zeros(info.kept_docs, dtype=np.uint32) for _ in range(3))
        pairs = np.zeros((info.n_pairs, 2), dtype=np.uint32)
        tb, to = np.zeros(max(1, info.term_bytes), dtype=np.uint8), np.zeros(info.n_terms + 1, dtype=np.uint64)
        L.ns_forward_fetch(h, kept.ctypes.data, dl.ctypes.data, cnt.ctypes.data, pairs.ctypes.data, tb.ctypes.data, to.ctypes.data)
        t_call = time.perf_counter() - t
        L.ns_forward_destroy(h)
        doc = np.repeat(np.arange(1, info.kept_docs + 1, dtype=np.uint64), cnt)
        check = int((doc * np.uint64(1000003) + pairs[:, 0].astype(np.uint64) * np.uint64(7919) + pairs[:, 1].astype(np.uint64)).sum(dtype=np.uint64))
        return {"device_ms": info.device_ms, "build_s": t_build, "call_s": t_call, "check": check,
                "info": {k: getattr(info, k) for k, _ in info._fields_ if k not in ("struct_size", "pad")}}

    device_run()                                                       # warm-up: code objects, pool blocks
    dev, host = [], []
    for r in range(max(args.reps, args.host_reps)):
        if r < args.reps:
            dev.append(device_run())
        if r < args.host_reps:
            host.append(json.loads(subprocess.check_output([exe, tf]).decode()))
    L.ns_ctx_destroy(ctx)
    mb = len(blob) / 1e6
    info = dev[0]["info"]
    med = statistics.median
    d_ms, b_s, c_s = med(d["device_ms"] for d in dev), med(d["build_s"] for d in dev), med(d["call_s"] for d in dev)
    out = {"text_mb": mb, "docs": info["n_docs"], "kept_docs": info["kept_docs"], "tokens": info["n_tokens"], "kept_tokens": info["kept_tokens"],
           "terms": info["n_terms"], "pairs": info["n_pairs"], "device_bytes_per_text_byte": info["device_bytes"] / len(blob),
           "device_part": {"ms": d_ms, "mb_per_s": mb / (d_ms * 1e-3), "mtokens_per_s": info["n_tokens"] / (d_ms * 1e-3) / 1e6, "all_ms": [d["device_ms"] for d in dev]},
           "build_call": {"s": b_s, "mb_per_s": mb / b_s, "includes": "upload of the text, device part"},
           "whole_call": {"s": c_s, "mb_per_s": mb / c_s, "mtokens_per_s": info["n_tokens"] / c_s / 1e6, "includes": "upload, device part, fetch of the result"},
           "identical_runs": len({d["check"] for d in dev}) == 1}
    if host:
        h_s = med(h["seconds"] for h in host)
        out["host_single_thread"] = {"s": h_s, "mb_per_s": mb / h_s, "mtokens_per_s": host[0]["tokens"] / h_s / 1e6, "all_s": [h["seconds"] for h in host],
                                     "kind": "host/textutil.hpp tokeniser + std::unordered_map, text in memory -> pairs in memory"}
        out["same_result_as_host"] = (host[0]["check"] == dev[0]["check"] and host[0]["terms"] == info["n_terms"] and host[0]["pairs"] == info["n_pairs"]
                                      and host[0]["tokens"] == info["n_tokens"] and host[0]["kept_tokens"] == info["kept_tokens"])
        out["speedup_device_part_vs_host"] = h_s / (d_ms * 1e-3)
        out["speedup_whole_call_vs_host"] = h_s / c_s
    print(json.dumps(out))


if __name__ == "__main__":
    main()
