#!/usr/bin/env python3
"""Generate tests/golden/ingest/ingest1.json from the REAL reference: its `forwardindex` tool (src/ForwardIndex.cpp,
compiled where it lies into a temporary directory with oracle/Makefile's shim include path and -Dcontains=count), its
`lexicon` tool and its engine (oracle/_ref/lexicon, oracle/_ref/ref_driver: `make -C oracle ref`).

The tool writes a small CORD-shaped corpus (metadata.csv + JSON files), runs the three programs and records DATA only:
  documents   {cord_uid, title, json_relpath, text} in metadata.csv order, text = what extract_text_from_cord_json
              (include/cordjson.hpp:21-49) yields for the JSON file: title, abstract sections, body sections, each + "\\n"
  docs_bin / stats_bin   the reference's files (base64)
  forward     the reference's forward.bin decoded through its terms.bin: per kept document {term: tf}
  queries     query text, and the reference's answer at K = 10: found, hits [seg, doc, fp32 score bits]
Queries whose reference answer holds two equal scores among its first 20 hits are not recorded: the reference leaves the
order inside such a run to its hash table, and the fixture is compared exactly.

Cases the reference's own front end cannot produce, which therefore live in the generated corpora of
tests/test_ingest_gpu.py instead: a document that ENDS inside a token followed by one that starts with alnum bytes
(extract_text_from_cord_json ends every field with "\\n"), bytes that are not valid UTF-8 (the JSON parser refuses
them), and the 70 000-byte token (fixture size).

    python tools/gen_golden_ingest.py [--ref DIR] [--time-mb N]
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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ingest_ref  # noqa: E402
import invert_oracle  # noqa: E402
import orc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ingest", "ingest1.json")
REF_BIN = os.path.join(ROOT, "oracle", "_ref")
K = 10
STOP = "the a an and or of to in for on with by as is are was were be been it this that from at".split()
WORDS = ("covid virus vaccine pandemic sars cov2 infection patients clinical study protein cell cells immune response "
         "antibody hospital respiratory disease treatment outbreak transmission health data model analysis results "
         "method methods viral rna genome sequence mutation variant severe acute syndrome coronavirus influenza fever "
         "cough lung lungs pneumonia mortality risk factors age children adults trial drug therapy dose placebo cohort "
         "sample samples test testing pcr assay positive negative symptoms onset days weeks hospitalised icu ventilator "
         "oxygen 19 2019 2020 h1n1 mers ace2 il6 t0 y2 x9 b117 n95 3d 42 1000 care workers mask masks public policy").split()


def build_forwardindex(ref, work):
    shim = os.path.join(REF_BIN, "shim")
    if not os.path.isdir(shim):
        sys.exit("oracle/_ref/shim is missing: run `make -C oracle ref` first")
    exe = os.path.join(work, "forwardindex")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-Dcontains=count", "-I" + shim, "-I" + os.path.join(ref, "include"), "-I" + ref,
                           os.path.join(ref, "src", "ForwardIndex.cpp"), "-o", exe])
    return exe


def styled(rng, w):
    r = rng.random()
    return w.upper() if r < 0.08 else w.capitalize() if r < 0.25 else w


def sentence(rng, n):
    out = []
    for _ in range(n):
        r = rng.random()
        if r < 0.30:
            w = rng.choice(STOP)
        elif r < 0.33:
            w = rng.choice("abcxyz7")                       # one-byte tokens
        else:
            w = WORDS[min(int(rng.paretovariate(0.9)) - 1, len(WORDS) - 1)]
        out.append(styled(rng, w) + rng.choice([" ", " ", " ", ", ", ". ", "-", " (", ") ", "; ", "/", "\t"]))
    return "".join(out)


def corpus(seed=20261016):
    """-> list of (cord_uid, title, json dict or None)"""
    rng = random.Random(seed)
    docs = []
    docs.append(("uid00000", "T0 fox", {"title": "T0 fox The Quick brown", "abstract": [{"text": "Y2 SARS-CoV2 covid 19 body"}], "body_text": []}))
    for i in range(1, 140):
        j = {"title": sentence(rng, rng.randint(2, 7))}
        j["abstract"] = [{"text": sentence(rng, rng.randint(3, 25))} for _ in range(rng.randint(0, 2))]
        j["body_text"] = [{"text": sentence(rng, rng.randint(5, 40))} for _ in range(rng.randint(0, 3))]
        docs.append(("uid%05d" % i, j["title"].strip(), j))
    big = "".join(rng.choice("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789") for _ in range(5200))
    special = [
        ("every stop word, in some case", {"title": " ".join(styled(rng, w) for w in STOP) + " THE A An", "abstract": [], "body_text": []}),   # dropped
        ("empty", {}),                                                                                                           # dropped: no text
        ("utf8", {"title": "café naïve überärzte covid virus 中文abc中12", "abstract": [{"text": "α-helix βsheet"}], "body_text": []}),
        ("nul", {"title": "vac\u0000cine covid\u0000 \u0000sars", "abstract": [], "body_text": [{"text": "a\u0000b \u0000\u0000 pandemic"}]}),
        ("digits", {"title": "19 2020 007 42 4 8 15 16 23", "abstract": [], "body_text": []}),
        ("one byte tokens only", {"title": "a b c d e f 1 2 3 x-y-z", "abstract": [], "body_text": []}),                           # dropped
        ("long token", {"title": "long " + big + " token", "abstract": [{"text": big.lower() + " " + big.upper()}], "body_text": []}),
        ("upper", {"title": "COVID VIRUS VACCINE THE PANDEMIC", "abstract": [{"text": "CoViD cOvId"}], "body_text": []}),
        ("quoted, title", {"title": "covid, virus and \"masks\"", "abstract": [], "body_text": []}),
        ("separators only", {"title": " .,;:!?-()[]{} \t", "abstract": [{"text": "\n\n"}], "body_text": []}),                      # dropped
    ]
    for n, (title, j) in enumerate(special):
        docs.append(("spec%04d" % n, title, j))
    return docs


def extract_text(j):
    """include/cordjson.hpp:21-49"""
    out = ""
    if isinstance(j.get("title"), str):
        out += j["title"] + "\n"
    for key in ("abstract", "body_text"):
        if isinstance(j.get(key), list):
            for sec in j[key]:
                if isinstance(sec.get("text"), str):
                    out += sec["text"] + "\n"
    return out


def csv_field(s):
    return '"' + s + '"' if "," in s else s     # (the reference's split_csv_line toggles on every quote and drops it)


def write_corpus(root, docs):
    os.makedirs(os.path.join(root, "document_parses", "pdf_json"))
    rows = ["cord_uid,sha,title,pdf_json_files,pmc_json_files"]
    out = []
    for uid, title, j in docs:
        rel = "document_parses/pdf_json/%s.json" % uid
        with open(os.path.join(root, rel), "w") as f:
            json.dump(j, f)                       # ensure_ascii: NUL and non-ASCII travel as \\uXXXX escapes
        rows.append(",".join([uid, "0" * 8, csv_field(title), rel, ""]))
        out.append({"cord_uid": uid, "title": title.replace('"', ""), "json_relpath": rel, "text": extract_text(j)})
    with open(os.path.join(root, "metadata.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")
    return out


def decode_forward(seg):
    terms = invert_oracle.read_terms(os.path.join(seg, "terms.bin"))
    counts, pairs = invert_oracle.read_forward(os.path.join(seg, "forward.bin"))
    out, at = [], 0
    for c in counts:
        out.append({terms[int(t)].decode("ascii"): int(tf) for t, tf in pairs[at:at + int(c)]})
        at += int(c)
    return terms, out


def candidate_queries(rng):
    qs = ["covid", "COVID virus", "sars cov2", "covid 19", "the of and", "zzzzzz", "vaccine trial placebo", "T0 fox", "y2 body",
          "caf na ve", "abc 12", "helix sheet", "vac cine", "007 42", "pandemic response", "x", "", "h1n1 influenza", "ace2 protein"]
    for _ in range(80):
        qs.append(" ".join(styled(rng, rng.choice(WORDS[:60])) for _ in range(rng.randint(1, 4))))
    return qs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--time-mb", type=int, default=0, help="time the reference's forwardindex on about N MB of generated text instead")
    args = ap.parse_args()
    work = tempfile.mkdtemp(prefix="ns_golden_ingest_")
    try:
        exe = build_forwardindex(args.ref, work)
        if args.time_mb:
            return time_reference(exe, work, args.time_mb)
        root, index = os.path.join(work, "cord"), os.path.join(work, "index")
        seg = os.path.join(index, "segments", "seg_000000")
        os.makedirs(seg)
        documents = write_corpus(root, corpus())
        subprocess.check_call([exe, root, seg], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        subprocess.check_call([os.path.join(REF_BIN, "lexicon"), seg], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        with open(os.path.join(index, "manifest.bin"), "wb") as f:
            f.write(struct.pack("<II", 1, len("seg_000000")) + b"seg_000000")
        terms, fwd = decode_forward(seg)
        # the restatement must agree with what was just produced (else the recorded texts are not what the reference tokenised)
        mine = ingest_ref.build([d["text"].encode("utf-8") for d in documents])
        assert ingest_ref.doc_term_maps(mine) == [{k.encode(): v for k, v in m.items()} for m in fwd], "restatement != reference"
        files = ingest_ref.file_bytes(documents, mine)
        for name in ("docs.bin", "stats.bin"):
            assert files[name] == open(os.path.join(seg, name), "rb").read(), name
        rng = random.Random(7)
        queries = []
        cands = candidate_queries(rng)
        wide = orc.run_ref_driver(index, cands, 20, work)
        top = orc.run_ref_driver(index, cands, K, work)
        for q, w, t in zip(cands, wide, top):
            bits = [h[2] for h in w["hits"]]
            if len(set(bits)) != len(bits) or not q.strip():
                continue
            queries.append({"query": q, "found": t["found"], "hits": [list(h) for h in t["hits"]]})
            if len(queries) == 40:
                break
        fx = {"name": "ingest1", "k": K, "documents": documents,
              "docs_bin_b64": base64.b64encode(open(os.path.join(seg, "docs.bin"), "rb").read()).decode(),
              "stats_bin_b64": base64.b64encode(open(os.path.join(seg, "stats.bin"), "rb").read()).decode(),
              "reference_terms": [t.decode("ascii") for t in terms[:12]],
              "forward": fwd, "queries": queries}
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(fx, f, separators=(",", ":"))
            f.write("\n")
        print(f"{len(documents)} documents in, {len(fwd)} kept, {len(terms)} terms, {len(queries)} queries "
              f"({sum(1 for q in queries if q['hits'])} with hits), {os.path.getsize(OUT)} bytes")
    finally:
        shutil.rmtree(work, ignore_errors=True)


def time_reference(exe, work, mb):
    """The reference's forwardindex on this CPU over generated text (tools/ingest_bench.py quotes it, as another machine)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ingest_bench
    texts = ingest_bench.corpus(mb << 20, 11)
    root = os.path.join(work, "cord_t")
    docs = [("u%07d" % i, "t", {"title": "", "abstract": [], "body_text": [{"text": t.decode("latin-1")}]}) for i, t in enumerate(texts)]
    write_corpus(root, docs)
    t0 = time.time()
    subprocess.check_call([exe, root, os.path.join(work, "seg_t")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    dt = time.time() - t0
    n = sum(len(t) for t in texts)
    print(json.dumps({"reference_forwardindex_cpu": {"text_mb": n / 1e6, "seconds": dt, "mb_per_s": n / 1e6 / dt, "includes": "JSON parsing and file IO"}}))


if __name__ == "__main__":
    main()
