#!/usr/bin/env python3
"""Generate tests/golden/suggest/*.json from the REAL reference: its own Engine::reload + Engine::suggest(...).dump(2)
(src/api_engine.cpp:91-107,:164-187), driven by tools/ref_suggest_driver.cpp.

The driver is compiled into a temporary directory against the reference translation units that `make -C oracle ref`
leaves in oracle/_ref/ (nothing under oracle/ changes; the binary is neither kept nor needed on a GPU machine).  The
fixtures are data: the index parameters (this repo's generator, or the raw terms of a tiny hand-made index), and per
request the input bytes, the limit, the reference's JSON text (null where dump(2) throws) and its suggestions.

    python tools/gen_golden_suggest.py [--ref DIR]        (DIR: the reference checkout, as oracle/Makefile's REF)
    python tools/gen_golden_suggest.py --time             (CPU timing of the reference's trie, for tools/suggest_bench.py)
"""
import argparse
import base64
import json
import os
import random
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nsbind  # noqa: E402
import suggest_ref  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "suggest")
REF_OBJS = ["api_segment", "api_autocomplete", "api_metadata", "semantic_embedding", "api_engine"]
LIMITS = [-3, 0, 1, 5, 10, 11]

FIXTURES = {
    # 3 barrel segments over the full vocabulary: ties, df summed over segments, the 8 real words plus t%06u
    "barrel3": dict(kind="gen", n_segments=3, docs_per_segment=2000, vocab=65536, seed=1337, legacy=False, sample=8, sample_seed=5),
    "legacy1": dict(kind="gen", n_segments=1, docs_per_segment=2000, vocab=4096, seed=7, legacy=True, sample=4, sample_seed=6),
    # raw terms that normalise alike or to < 2 bytes, df 0, a u32 wrap (tests/suggest_ref.py TINY_SEGMENTS)
    "tiny1": dict(kind="tiny"),
}

EDGE_INPUTS = [
    b"t", b"c", b"v", b"0",                      # single characters: the widest ranges
    b"covid", b"covidx", b"coronavirus", b"coronavirus1",
    b"CO", b"CoV", b"COVID",                     # upper case
    b"covid vacc", b"New COVID va", b"The Covid-19 pa", b"what is t0001",   # multi-word, mixed-case base
    b"cov!", b"cov  ", b"cov?!.", b"  co ",      # trailing punctuation / spaces
    b"", b"!!!", b"   ", b"-", b"...?",          # empty, punctuation only
    b"caf\xc3\xa9 co", b"\xc3\xa9t", b"na\xc3\xafve vi",   # bytes >= 0x80 (valid UTF-8)
    b"\xffco", b"co\xff",                        # invalid UTF-8 (the reference's dump(2) throws)
    b"\x01co", b"co\tvi", b"a\nb", b"\x00t00", b"vi\x00",   # control bytes
    b"zzzz", b"qqq", b"t99999999",               # no match
    b"t" + b"0" * 40, b"coronavirusxxxxxxxxxxxxxxxxxxxxxxxxxxxx",   # longer than any term
    b"wr", b"ab", b"zz", b"ca", b"caf", b"v",    # tiny index's duplicates, df 0, wrap
]


def build_driver(ref, workdir):
    obj = os.path.join(ROOT, "oracle", "_ref")
    missing = [o for o in REF_OBJS if not os.path.exists(os.path.join(obj, o + ".o"))]
    if missing:
        sys.exit(f"oracle/_ref lacks {missing}: run `make -C oracle ref` first")
    exe = os.path.join(workdir, "ref_suggest_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-I" + os.path.join(obj, "shim"), "-I" + os.path.join(ref, "include"), "-I" + ref,
                           os.path.join(ROOT, "tools", "ref_suggest_driver.cpp")] + [os.path.join(obj, o + ".o") for o in REF_OBJS] +
                          ["-o", exe, "-lpthread"])
    return exe


def write_requests(path, reqs):
    with open(path, "wb") as f:
        for limit, b in reqs:
            f.write(struct.pack("<iI", limit, len(b)) + b)


def run_driver(exe, index_dir, reqs, workdir):
    rq, out = os.path.join(workdir, "req.bin"), os.path.join(workdir, "out.bin")
    write_requests(rq, reqs)
    subprocess.check_call([exe, "json", index_dir, rq, out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    data = open(out, "rb").read()
    pos, res = 0, []
    for _ in reqs:
        dumped = data[pos]
        (n,) = struct.unpack_from("<I", data, pos + 1)
        text = data[pos + 5:pos + 5 + n]
        pos += 5 + n
        (cnt,) = struct.unpack_from("<I", data, pos)
        pos += 4
        sugg = []
        for _ in range(cnt):
            (m,) = struct.unpack_from("<I", data, pos)
            sugg.append(data[pos + 4:pos + 4 + m])
            pos += 4 + m
        res.append((text.decode("utf-8") if dumped else None, sugg))
    assert pos == len(data)
    return res


def make_index(p, index_dir):
    if p["kind"] == "gen":
        nsbind.gen_index(index_dir, p["n_segments"], p["docs_per_segment"], p["vocab"], p["seed"], p["legacy"])
    else:
        suggest_ref.write_tiny_index(index_dir, suggest_ref.TINY_SEGMENTS)


def inputs_for(p, index_dir):
    ins = list(EDGE_INPUTS)
    if p["kind"] == "gen":
        terms, _ = suggest_ref.table(index_dir)
        rng = random.Random(p["sample_seed"])
        picks = [b"covid", b"coronavirus"] + rng.sample(terms, p["sample"])
        for t in picks:
            ins += [t[:i] for i in range(1, len(t) + 1)]   # every prefix of the sampled terms
    seen, out = set(), []
    for b in ins:
        if b not in seen:
            seen.add(b)
            out.append(b)
    return out


def b64(b):
    return base64.b64encode(b).decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--time", action="store_true", help="time the reference's trie build and lookup on this CPU")
    args = ap.parse_args()
    work = tempfile.mkdtemp(prefix="ns_golden_suggest_")
    try:
        exe = build_driver(args.ref, work)
        if args.time:
            time_reference(exe, work)
            return
        os.makedirs(OUT_DIR, exist_ok=True)
        for name, p in FIXTURES.items():
            idx = os.path.join(work, name)
            make_index(p, idx)
            ins = inputs_for(p, idx)
            reqs = [(lim, b) for b in ins for lim in LIMITS]
            res = run_driver(exe, idx, reqs, work)
            cases = [{"input_b64": b64(b), "limit": lim, "json": js, "suggestions_b64": [b64(s) for s in sg]}
                     for (lim, b), (js, sg) in zip(reqs, res)]
            params = dict(p)
            if p["kind"] == "tiny":
                params["segments_b64"] = [[[b64(t), df] for t, df in seg] for seg in suggest_ref.TINY_SEGMENTS]
            fx = {"name": name, "params": params, "limits": LIMITS, "cases": cases}
            with open(os.path.join(OUT_DIR, name + ".json"), "w") as f:
                json.dump(fx, f, separators=(",", ":"))
                f.write("\n")
            n_sugg = sum(len(c["suggestions_b64"]) for c in cases)
            print(f"{name}: {len(cases)} cases, {n_sugg} suggestions, {sum(1 for c in cases if c['json'] is None)} without JSON")
    finally:
        shutil.rmtree(work, ignore_errors=True)


def time_reference(exe, work):
    """The reference's trie on this CPU: build time and mean Engine::suggest latency (tools/suggest_bench.py's baseline)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import suggest_bench
    for name, (nseg, docs, vocab) in suggest_bench.INDEXES.items():
        idx = os.path.join(work, name)
        nsbind.gen_index(idx, nseg, docs, vocab, 1337, False)
        terms, scores = suggest_ref.table(idx)
        inputs = suggest_bench.workload(terms, scores, 16384, 11)
        rq = os.path.join(work, "req.bin")
        write_requests(rq, [(5, b) for b in inputs])
        out = subprocess.check_output([exe, "time", idx, rq, "3"], stderr=subprocess.DEVNULL).decode().strip()
        print(json.dumps({"index": name, "terms": len(terms), "reference_cpu": json.loads(out)}))
        shutil.rmtree(idx, ignore_errors=True)


if __name__ == "__main__":
    main()
