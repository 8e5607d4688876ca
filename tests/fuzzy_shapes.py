"""Directed inputs of the corrector's and completion's kernels (csrc/ns_fuzzy.hip) and the code that runs
them through raw ns_ac_fuzzy / ns_ac_fuzzy_prefix against the restatements tests/correct_ref.py and tests/complete_ref.py.
Every comparison is exact: index, distance, count and the ~0u / 0xff tails.

Six families, each built in plain Python from a fixed seed:

  seam      terms of 9 .. 20 bytes at every pool offset mod 4, twins that differ in one byte at 7, 8, 9, m - 2 or m - 1, and
            queries with each kind of edit at those indices: the head/pool seam, the funnel of fz_load4, a term's last dword
  queue     1024 terms of one length; query p finds term p alone, wherever p lands in the LDS queue of signature survivors
  anagrams  permutations of one byte set (all pass the signature, all far) around one near candidate: dead lanes next to a
            live one, and the wave's early exit when nothing is near
  keep      §5l's 1296 terms with ascending and descending scores: the keep buffer overflows and is reduced
  slices    the hand-made 4097 terms: the best L are ties on both sides of slot 1024; with a fixed prefix the later slices are empty
  build     repeated strings and zero scores across entry 4096, mixed lengths in every 64 entries

Imported by tests/test_fuzzy_shapes_cpu.py (the families' own claims) and tests/test_fuzzy_shapes_gpu.py (the product library),
and run as a program in a child process that loaded the counting build: there ns_debug_fuzzy_counters reports which paths
the inputs reached (FUZZY_EVENTS), and the counts that depend on the table and the queries alone are restated here."""
import ctypes as C
import functools
import itertools
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "nextsearch-api_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import complete_ref  # noqa: E402
import correct_ref  # noqa: E402
import nsbind  # noqa: E402

# name -> index of ns_debug_fuzzy_counters (counting build)
FUZZY_EVENTS = {"sig_tested": 0, "sig_rejected": 1, "dp_full_waves": 2, "dp_full_with_rest": 3, "dp_tail_waves": 4, "dp_early_exit": 5,
                "dp_dead_lane_rows": 6, "load4_funnel": 7, "load4_last_dword": 8, "transposed": 9, "keep_reduced": 10, "empty_slices": 11,
                "multi_slice_queries": 12, "long_bucket": 13, "build_dropped_zero": 14, "build_dropped_repeat": 15,
                "build_multi_length_rounds": 16}
FAMILIES = ["seam", "queue", "anagrams", "keep", "slices", "build"]
# what each family is built to reach
REACHED = {"seam": ("load4_funnel", "load4_last_dword", "transposed"),
           "queue": ("dp_full_with_rest", "dp_tail_waves", "sig_rejected"),
           "anagrams": ("dp_early_exit", "dp_dead_lane_rows"),
           "keep": ("keep_reduced",),
           "slices": ("multi_slice_queries", "empty_slices", "long_bucket"),
           "build": ("build_multi_length_rounds",)}
SLICE = 1024           # candidates per workgroup of k_fz_scan / k_fp_scan (ac_fuzzy_call)
CHUNK = 4096           # entries per wave of the build kernels (kFzChunk)
L = 10
SEAM_LENGTHS = range(9, 21)
SIG_BITS = (1 << 37) - 1


# ---- the signature rule, restated ---------------------------------------------------------------------------------------
def sig_pass_fuzzy(q, c, e):
    """the corrector's test: the byte classes [0-9], [a-z] and "other" that one string has and the other lacks, at most 2 e"""
    return bin((complete_ref.sig(q) ^ complete_ref.sig(c)) & SIG_BITS).count("1") <= 2 * e


def sig_pass_prefix(q, c, e):
    """completion's test, one-sided: at most e classes of the query that the candidate lacks; past 66 bytes there is no signature"""
    miss = complete_ref.sig_missing(q, c)
    return miss is None or miss <= e


def _popcount(a):
    return np.unpackbits(np.ascontiguousarray(a, dtype=np.uint64).view(np.uint8).reshape(len(a), 8), axis=1).sum(axis=1)


def sig_counts(terms, scores, queries, edits, complete, prefix_len=0):
    """-> (candidates the device gives to the signature test, how many of them it rejects) over a batch: per query every
    candidate inside its length window (n - e .. n + e, or from n - e upwards) that shares its fixed prefix; the same rules as
    sig_pass_fuzzy / sig_pass_prefix, over the whole table at once"""
    cand = np.asarray(correct_ref.candidates(terms, scores), dtype=bool)
    lens = np.array([len(t) for t in terms], dtype=np.int64)
    sigs = np.array([complete_ref.sig(t) for t in terms], dtype=np.uint64)
    long_ = lens > complete_ref.MAX_LEN + complete_ref.MAX_EDITS
    tested = rejected = 0
    for q, e in zip(queries, edits):
        n, e = len(q), int(e)
        if n == 0 or n > correct_ref.MAX_LEN:
            continue
        ok = cand & (lens >= n - e)
        if not complete:
            ok &= lens <= n + e
        p = q[:min(prefix_len, n)]
        if p:
            ok &= np.array([t.startswith(p) for t in terms], dtype=bool)
        qs = np.uint64(complete_ref.sig(q))
        if complete:
            fail = (_popcount(qs & ~sigs[ok]) > e) & ~long_[ok]
        else:
            fail = _popcount(qs ^ sigs[ok]) > 2 * e
        tested += int(ok.sum())
        rejected += int(fail.sum())
    return tested, rejected


def slot_positions(terms, scores, n, e, complete):
    """{index: position} of a query of n bytes among its candidates, in the order the scan deals them out: by length (from
    n - e; everything past 66 bytes is one bucket), by index inside a length"""
    cand = correct_ref.candidates(terms, scores)
    top = complete_ref.MAX_LEN + complete_ref.MAX_EDITS + 1
    rows = [(min(len(t), top), i) for i, t in enumerate(terms) if cand[i] and len(t) >= n - e and (complete or len(t) <= n + e)]
    return {i: k for k, (_, i) in enumerate(sorted(rows))}


def queue_trace(passes):
    """one slice of the scan, restated for the tests of the families' own claims: passes[x] = whether position x of a query's
    candidates passes the signature.  Four waves take 64 positions each, 256 apart; a wave queues its survivors, runs the DP on
    the top 64 once that many wait, and on the remainder at the end.  -> (DP calls on a full wave, of those the ones that left
    a remainder, DP calls on a remainder, {position: (call, lane)} of every survivor)"""
    full = rest = tail = 0
    where = {}
    for wave in range(4):
        waiting, call = [], 0
        for base in range(wave * 64, len(passes), 256):
            waiting += [x for x in range(base, min(base + 64, len(passes))) if passes[x]]
            if len(waiting) >= 64:
                for lane, x in enumerate(waiting[-64:]):
                    where[x] = (wave, call, lane)
                del waiting[-64:]
                full, rest, call = full + 1, rest + bool(waiting), call + 1
        if waiting:
            tail += 1
            for lane, x in enumerate(waiting):
                where[x] = (wave, call, lane)
    return full, rest, tail, where


def pool_offsets(terms):
    """offset of each term in the pool that AcTable uploads: the running sum of the sorted terms' lengths (ns_ac_upload keeps
    the caller's offsets, and the device pool is aligned far beyond a dword)"""
    return [0] + list(itertools.accumulate(len(t) for t in terms))[:-1]


# ---- the families -------------------------------------------------------------------------------------------------------
# A family: {"terms", "scores", "calls": [(kind, queries, edits, prefix_len, L, one_per_call)], ...}; kind "fuzzy" | "prefix"
def _edit_indices(m):
    return [i for i in sorted({6, 7, 8, 9, m - 2, m - 1}) if i < m]


def _group_offsets(m):
    """how many pool offsets mod 4 the back-to-back terms of one group of length m take (m = 9: three terms, the stem and two twins)"""
    return 1 if m % 4 == 0 else 2 if m % 2 == 0 or m == 9 else 4


def _twin_indices(m):
    return [i for i in sorted({7, 8, 9, m - 2, m - 1}) if i < m]


def seam_edits(stem, rng, alpha):
    """[(kind, index, string)]: each of deletion, insertion, substitution and neighbour transposition at each index of
    {6, 7, 8, 9, m - 2, m - 1} that exists"""
    out = []
    for i in _edit_indices(len(stem)):
        other = [c for c in alpha if c != stem[i]]
        out.append(("del", i, stem[:i] + stem[i + 1:]))
        out.append(("ins", i, stem[:i] + bytes([rng.choice(other)]) + stem[i:]))
        out.append(("sub", i, stem[:i] + bytes([rng.choice(other)]) + stem[i + 1:]))
        if i + 1 < len(stem):
            out.append(("swap", i, stem[:i] + bytes([stem[i + 1], stem[i]]) + stem[i + 2:]))
    return out


@functools.lru_cache(maxsize=None)
def seam():
    rng = random.Random(5)
    alpha = b"bcdefghi"
    firsts = b"0123456789abcdefghijklmnopqrstuvwxyz"
    groups = []                                  # in sort order: a group's terms share their first byte, and no other term has it
    for m in SEAM_LENGTHS:
        for _ in range(4 // _group_offsets(m)):   # e.g. a group of one length a multiple of 4 has ONE offset mod 4
            stem = bytearray([firsts[len(groups)]])
            while len(stem) < m:
                c = rng.choice(alpha)
                if c != stem[-1]:
                    stem.append(c)
            stem = bytes(stem)
            twins = {}
            for x in _twin_indices(m):
                twins[x] = stem[:x] + bytes([rng.choice([c for c in alpha if c != stem[x]])]) + stem[x + 1:]
            groups.append((stem, twins))
    # fillers, placed deliberately: one of 1 .. 3 bytes in front of a group moves it (and all that follows) to another offset
    terms, covered, at = [], {m: set() for m in SEAM_LENGTHS}, 0
    for stem, twins in groups:
        m = len(stem)
        members = sorted([stem] + list(twins.values()))
        new = {k: {(at + k + j * m) % 4 for j in range(len(members))} - covered[m] for k in range(4)}
        k = max(range(4), key=lambda k: (len(new[k]), -k))
        if k:
            terms.append(stem[:1] + b"-" * (k - 1))
        terms += members
        covered[m] |= new[k]
        at += k + len(members) * m
    assert terms == sorted(terms) and len(set(terms)) == len(terms)
    scores = list(range(1, len(terms) + 1))
    rng.shuffle(scores)                          # distinct: a misread byte changes a distance or a rank
    stems = [g[0] for g in groups]
    edits = {s: seam_edits(s, rng, alpha) for s in stems}
    qs = sorted({s for s in stems} | {x for s in stems for _, _, x in edits[s]})
    cuts = sorted({x[:k] for x in qs for k in (8, 9, 10, len(x))})
    calls = [("fuzzy", qs + qs, [1] * len(qs) + [2] * len(qs), 0, L, False),          # every string under both bounds
             ("prefix", cuts + cuts, [1] * len(cuts) + [2] * len(cuts), 0, L, False)]
    return {"terms": terms, "scores": scores, "calls": calls, "stems": stems, "twins": {g[0]: g[1] for g in groups}, "edits": edits}


def seam_grid(fam):
    """{(length, pool offset mod 4)} over the family's terms of 9 .. 20 bytes"""
    return {(len(t), o % 4) for t, o in zip(fam["terms"], pool_offsets(fam["terms"])) if len(t) in SEAM_LENGTHS}


@functools.lru_cache(maxsize=None)
def queue():
    """512 terms over a..l and 512 over m..x, 12 bytes, one score.  About two thirds of each half are permutations of their 12
    letters (one signature), the others draw with repetition (about 8 letters).  A query made from a permutation passes most of
    its half: a wave's queue goes past 64 and keeps a remainder; one made from the others passes few: everything waits for the
    tail call.  The other half never passes."""
    rng = random.Random(12)
    terms = set()
    for letters in (b"abcdefghijkl", b"mnopqrstuvwx"):
        half = set()
        while len(half) < 512:
            if rng.random() < 0.68:
                t = list(letters)
                rng.shuffle(t)
            else:
                t = [rng.choice(letters) for _ in range(12)]
            half.add(bytes(t))
        terms |= half
    terms = sorted(terms)
    queries = [t[:5] + b"z" + t[6:] for t in terms]
    calls = [(kind, queries, [2] * 1024, 0, L, one) for kind in ("fuzzy", "prefix") for one in (False, True)]
    return {"terms": terms, "scores": [3] * len(terms), "calls": calls, "queries": queries}


@functools.lru_cache(maxsize=None)
def anagrams():
    """256 permutations of abcdefghijkl: one length, one signature, so slot order is index order and every 64 consecutive
    slots are one wave of the DP.  `near` is one transposition away from the first query; everything else is far from both
    queries (the restatement finds nothing else within two edits)."""
    rng = random.Random(21)
    letters = list(b"abcdefghijkl")

    def perm():
        t = letters[:]
        rng.shuffle(t)
        return bytes(t)

    near = perm()
    q_near = near[:8] + bytes([near[9], near[8]]) + near[10:]          # the transposition sits on the head/pool seam
    while True:
        q_none = perm()
        if correct_ref.osa(q_none, near) > 4:
            break
    terms = {near}
    while len(terms) < 256:
        t = perm()
        if t not in (q_near, q_none) and min(correct_ref.osa(q, t) for q in (q_near, q_none)) > 2 and \
                min(complete_ref.pd(q, t) for q in (q_near, q_none)) > 2:
            terms.add(t)
    terms = sorted(terms)
    calls = [(kind, [q_near, q_none], [2, 2], 0, L, True) for kind in ("fuzzy", "prefix")]   # one query per call: the counters tell them apart
    return {"terms": terms, "scores": [5] * len(terms), "calls": calls, "near": terms.index(near), "q_near": q_near, "q_none": q_none}


def early_exit_row(q, wave, e=2):
    """the first row i < |q| by which a DP wave over the candidates `wave` has left the row loop, or None.  Row i's smallest
    cell over all columns is pd(q[:i], c); the band's cells are no smaller, so once two rows in sequence lie above e for every
    candidate, no lane is within e and the wave breaks (it may break sooner, never later).  A candidate within e of the whole
    query has a cell within e in every row of its band (the cells of its best alignment), so its wave returns None."""
    dead_before = False
    for i in range(1, len(q)):
        dead = all(complete_ref.pd(q[:i], c) > e for c in wave)
        if dead and dead_before:
            return i
        dead_before = dead
    return None


@functools.lru_cache(maxsize=None)
def keep(descending=False):
    """§5l's table and the queries of tests/test_correct_gpu.py and tests/test_complete_gpu.py on it"""
    abc = b"0123456789abcdefghijklmnopqrstuvwxyz"
    terms = sorted(b"aaaa" + bytes([x, y]) for x in abc for y in abc)
    scores = list(range(1, len(terms) + 1))
    if descending:
        scores.reverse()
    fq, pq = [b"aaaa--", b"aaaazz", b"aaaa"], [b"z", b"zz", b"a", b"aa", b"za", b"-"]
    calls = [("fuzzy", fq, [2] * len(fq), 0, k, False) for k in (1, 5, L)] + [("prefix", pq, [2] * len(pq), 0, k, False) for k in (1, 5, L)]
    return {"terms": terms, "scores": scores, "calls": calls}


def hand_made(n, rng):
    """the hand-made table of tests/test_complete_gpu.py: mostly one length, with repeated strings, terms past 8, past 66 and
    past 255 bytes and bytes outside [0-9a-z]"""
    extra = [b"a00001", b"a00001", b"a00001", b"b1", b"", b"a", b"A-b_9", b"a0\xc3\xa9t\xc3\xa9", b"a000 1", b"b00002abcdefgh",
             b"b00002abcdefhg", b"b00002abcdefghijklmnopqrstuvwxyz0123456789", b"a" * 63, b"a" * 64, b"a" * 65, b"a" * 66, b"a" * 67,
             b"a" * 80, b"a" * 300, b"b" * 64 + b"c", b"b" * 64 + b"c", b"b" * 70 + b"xyz", b"a0000", b"a000001"]
    base = set()
    while len(base) < n - len(extra):
        base.add(b"%c%05d" % (rng.choice(b"ab"), rng.randrange(100000)))
    return sorted(list(base) + extra)


def straddles(terms, scores, answer, n, e, complete):
    """the answer is L ties in distance and score, with members on both sides of slot SLICE of the query's candidates"""
    pos = slot_positions(terms, scores, n, e, complete)
    at = [pos[i] for i, _ in answer]
    return len(answer) == L and len({(d, scores[i]) for i, d in answer}) == 1 and min(at) < SLICE <= max(at)


@functools.lru_cache(maxsize=None)
def slices():
    rng = random.Random(200 + 4097)
    terms = hand_made(4097, rng)
    scores = [7] * len(terms)
    tab = correct_ref.Table(terms, scores)
    six = [t for t in terms if len(t) == 6 and t[:1] == b"a" and t.isalnum()]
    while True:   # a query two substitutions away from a term, past its third byte: its best L are all at distance 2
        q = bytearray(rng.choice(six))
        for x in rng.sample((3, 4, 5), 2):
            q[x] = rng.choice([c for c in b"0123456789" if c != q[x]])
        q = bytes(q)
        if straddles(terms, scores, tab.fuzzy(q, 2, 0, L), len(q), 2, False) and tab.fuzzy(q, 2, 3, L):
            break
    calls = [("fuzzy", [q, b"a00001", b"b99999"], [2, 2, 2], p, k, False) for p in (0, 3) for k in (L, 3)]
    calls += [("prefix", [b"zz", q, q[:4], b"a0", b"b" * 62 + b"cb"], [2, 2, 1, 0, 2], p, L, False) for p in (0, 3)]
    return {"terms": terms, "scores": scores, "calls": calls, "q": q}


@functools.lru_cache(maxsize=None)
def build():
    """4400 entries of 5 .. 12 bytes in no order of length; runs of one string repeated 3 .. 7 times at entries 60 .. 66 and
    4093 .. 4099 (the second across entry CHUNK, the first across a wave of 64), score 0 on single entries and inside, at the head of and
    all over such runs, on both sides of entry CHUNK"""
    rng = random.Random(33)
    distinct = set()
    while len(distinct) < 4400 - 6 - 6:
        distinct.add(b"c" + bytes(rng.choice(b"0123") for _ in range(rng.randint(4, 11))))
    distinct = sorted(distinct)
    terms = []
    for t in distinct:
        terms += [t] * (7 if len(terms) in (60, CHUNK - 3) else 1)
    assert len(terms) == 4400 and terms == sorted(terms)
    scores = [rng.choice([0, 1, 1, 2, 2, 3, 3, 3]) for _ in terms]
    for i, s in ((60, 2), (61, 0), (62, 2), (CHUNK - 3, 1), (CHUNK - 2, 1), (CHUNK - 1, 0), (CHUNK, 1), (CHUNK + 1, 0), (CHUNK + 2, 1),
                 (CHUNK - 5, 0), (CHUNK + 5, 0)):
        scores[i] = s
    # a run whose head has score 0: none of it is a candidate
    at = CHUNK + 40
    terms[at + 1] = terms[at + 2] = terms[at]
    scores[at:at + 3] = [0, 2, 3]
    terms.sort()
    assert all(terms[at + k] == terms[at] for k in (1, 2))
    near = list(range(58, 68)) + list(range(CHUNK - 8, CHUNK + 8)) + list(range(at - 1, at + 4))
    picks = [terms[i] for i in near] + [rng.choice(terms) for _ in range(20)]
    queries = sorted({correct_ref.random_edits(rng, t, k, b"0123c") for t in picks for k in (0, 1, 2)})
    edits = [1 + (k % 2) for k in range(len(queries))]
    calls = [("fuzzy", queries, edits, 0, L, False), ("prefix", [q[:6] for q in queries], edits, 1, 3, False)]
    return {"terms": terms, "scores": scores, "calls": calls}


def build_dropped(fam):
    """(entries dropped for score 0, entries dropped as repeats), as fz_classify tells them apart: the score is looked at first"""
    zero = sum(int(s) == 0 for s in fam["scores"])
    return zero, len(fam["terms"]) - sum(correct_ref.candidates(fam["terms"], fam["scores"])) - zero


def tables_of(name):
    """a family's tables: keep has two"""
    return [keep(False), keep(True)] if name == "keep" else [globals()[name]()]


# ---- running them -------------------------------------------------------------------------------------------------------
_REFERENCE = {}   # computed once, shared, never changed


def reference(name):
    """per table and call of a family: the expected [(index, distance)] of every query"""
    if name not in _REFERENCE:
        out = []
        for fam in tables_of(name):
            ftab = correct_ref.Table(fam["terms"], fam["scores"])
            ptab = complete_ref.Table(fam["terms"], fam["scores"])
            want = {}
            for kind, queries, edits, prefix_len, k, _ in fam["calls"]:
                ask = ftab.fuzzy if kind == "fuzzy" else ptab.complete
                key = (kind, tuple(queries), tuple(edits), prefix_len, k)
                if key not in want:
                    want[key] = [ask(q, int(e), prefix_len, k) for q, e in zip(queries, edits)]
            out.append(want)
        _REFERENCE[name] = out
    return _REFERENCE[name]


def _compare(what, want, k, idx, dist, cnt):
    assert idx.shape == dist.shape == (len(want), k) and cnt.shape == (len(want),), what
    for q, w in enumerate(want):
        k = int(cnt[q])
        got = list(zip(idx[q, :k].tolist(), dist[q, :k].tolist()))
        assert got == w, (what, q, got, w)
        assert (idx[q, k:] == 0xFFFFFFFF).all() and (dist[q, k:] == 0xFF).all(), (what, q)


def run_family(name, counters=None):
    """uploads the family's tables, builds their side structures and compares every call with the restatement.  counters: a
    dict that receives {"build": [...], "calls": [[...], ...]} of ns_debug_fuzzy_counters, read after the builds and after every
    call of the library (the counting build)"""
    h = C.c_void_p()
    assert nsbind.hip_lib().ns_ctx_create(0, C.byref(h)) == 0
    try:
        wants = reference(name)
        if counters is not None:
            nsbind.fuzzy_counters(reset=True)
            counters["build"], counters["calls"] = [0] * len(FUZZY_EVENTS), []
        for t, fam in enumerate(tables_of(name)):
            ac = nsbind.AcTable(h, fam["terms"], fam["scores"])
            assert ac.rc == 0 and ac.build_fuzzy()[0] == 0
            if counters is not None:
                counters["build"] = [a + b for a, b in zip(counters["build"], nsbind.fuzzy_counters(reset=True))]
            for kind, queries, edits, prefix_len, k, one_per_call in fam["calls"]:
                ask = ac.fuzzy if kind == "fuzzy" else ac.fuzzy_prefix
                want = wants[t][(kind, tuple(queries), tuple(edits), prefix_len, k)]
                what = (name, t, kind, prefix_len, k, one_per_call)
                if one_per_call:
                    for q in range(len(queries)):
                        idx, dist, cnt, _ = ask(queries[q:q + 1], edits[q:q + 1], prefix_len, k)
                        _compare(what + (q,), want[q:q + 1], k, idx, dist, cnt)
                        if counters is not None:
                            counters["calls"].append(nsbind.fuzzy_counters(reset=True))
                else:
                    idx, dist, cnt, _ = ask(queries, edits, prefix_len, k)
                    _compare(what, want, k, idx, dist, cnt)
                    if counters is not None:
                        counters["calls"].append(nsbind.fuzzy_counters(reset=True))
            ac.close()
    finally:
        nsbind.hip_lib().ns_ctx_destroy(h)


def exact_counts(name):
    """{event: restated count} of what depends on the family's table and queries alone, not on how the work is cut"""
    if name == "queue":
        fam = queue()
        tested = rejected = 0
        for kind, queries, edits, prefix_len, _, _ in fam["calls"]:
            a, b = sig_counts(fam["terms"], fam["scores"], queries, edits, kind == "prefix", prefix_len)
            tested, rejected = tested + a, rejected + b
        return {"sig_tested": tested, "sig_rejected": rejected}
    if name == "build":
        zero, repeat = build_dropped(build())
        return {"build_dropped_zero": zero, "build_dropped_repeat": repeat}
    return {}


def main(out_path):
    """child process: every family on the loaded library; with the counting build, each family's counters (the builds' and the
    calls' summed), the events of its REACHED tuple that stayed 0, and the restated exact counts next to the counted ones"""
    counting = nsbind.fuzzy_counters(reset=True) is not None
    rep = {"counting": counting, "events": {}, "missed": [], "exact": {}}
    for name in FAMILIES:
        c = {} if counting else None
        run_family(name, c)
        if not counting:
            continue
        total = [sum(v) for v in zip(c["build"], *c["calls"])]
        ev = {e: total[i] for e, i in FUZZY_EVENTS.items()}
        rep["events"][name] = ev
        rep["missed"] += [name + "." + e for e in REACHED[name] if ev[e] == 0]
        if exact_counts(name):
            rep["exact"][name] = {e: [ev[e], want] for e, want in exact_counts(name).items()}
        if name == "anagrams":   # per call: fuzzy near, fuzzy none, prefix near, prefix none
            per = [{e: v[i] for e, i in FUZZY_EVENTS.items()} for v in c["calls"]]
            rep["anagrams_calls"] = per
            rep["missed"] += ["anagrams.q_near.dp_dead_lane_rows"] * (per[0]["dp_dead_lane_rows"] == 0)
            rep["missed"] += ["anagrams.q_none.dp_early_exit"] * (per[1]["dp_early_exit"] == 0)
        print("fuzzy", name, ev, flush=True)
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
        f.write("\n")
    print("fuzzy shapes OK")


if __name__ == "__main__":
    main(sys.argv[1])
