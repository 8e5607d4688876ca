"""Directed shapes for the radix sort and the scans of csrc/ns_invert.hip (k_iv_hist_w, k_iv_pass, k_iv_runs, k_iv_scan_*), which
lie under index inversion (invert_run), text ingest and compaction (ig_sort, ig_scan).  Numpy only; no device is touched.

A case is (name, counts u32[n_docs], pairs u32[n, 2], n_terms); what the device must return for it is
oracle/invert_oracle.invert(counts, pairs, n_terms), a stable argsort plus a bincount.  Every pair's tf is its index in the
input unless a case says otherwise: any misplaced or swapped pair, two equal (term, doc) pairs in the wrong order included,
shows in the bytes.

reach(case, T, df, postings) names the paths of the kernels and of the host code that a case takes.  Each flag is a condition on
the inputs, on the digit plan as restated here (plan) and on the oracle's output; nothing a device returned enters it.  FLAGS is
the list the whole table must reach; tests/test_radix_shapes_cpu.py asserts that, and the GPU file asserts that the library's
ns_radix_plan is the plan the flags were computed from.

T is ns_radix_tile(), the pairs one workgroup sorts per pass; a wave of the workgroup takes T / 4 consecutive pairs in steps of
LANES.  Shapes are built from T.

Left out: the three-pass plans wider than [9, 8, 8] through ns_invert_forward.  They start at n_terms = 2^25 + 1, where each
array of df's size is 128 MiB and more per copy.  The instantiations k_iv_pass<9 | 10 | 11, false, false> cannot occur in an
inversion at all below that.  ig_sort, the sort of ns_forward_build and of compaction, launches k_iv_pass<B, false, false> for
every pass, a single one included (csrc/ns_api.hip, ig_sort: its input is keys and values already), so the
corpora at the end of this module reach them through one-pass sorts: 9 and 11 bits here, 10 in the suite's older corpora.  The
three-pass corpus sorts [8, 8, 8]."""
import collections

import numpy as np

LANES = 64


def BAD_IDS(n_terms):
    """the termIds a case drops"""
    return (n_terms, n_terms + 1, 0xFFFFFFFE, 0xFFFFFFFF)


Case = collections.namedtuple("Case", "name counts pairs n_terms group")


# ---- the digit plan, restated ------------------------------------------------------------------------------------------------
def plan(key_range):
    """-> (bits, [digit of pass 0, ...]): bits = the width of key_range - 1 (at least 1); ceil(bits / 11) passes; every pass takes
    an even share of the bits still to sort, rounded up, but no less than 8 and no more than 11."""
    bits = max(1, (int(key_range) - 1).bit_length()) if key_range else 1
    passes = -(-bits // 11)
    digits, left = [], bits
    for p in range(passes):
        share = -(-left // (passes - p))
        digits.append(min(11, max(8, share)))
        left = max(0, left - digits[-1])
    return bits, digits


def shifts(digits):
    return [sum(digits[:p]) for p in range(len(digits))]


# ---- building blocks ---------------------------------------------------------------------------------------------------------
def with_tf(ids):
    """pairs u32[n, 2]: (termId, the pair's index)"""
    ids = np.asarray(ids, dtype=np.uint32)
    return np.stack([ids, np.arange(len(ids), dtype=np.uint32)], axis=1)


def docs_for(n, rng, lo=0, hi=40):
    """document lengths in [lo, hi] that sum to n exactly (the last one is cut)"""
    out, left = [], n
    while left > 0:
        c = min(left, int(rng.integers(lo, hi + 1)))
        out.append(c)
        left -= c
    return np.asarray(out, dtype=np.uint32)


def spread_ids(n_terms, n, rng):
    """n ids below n_terms in which every digit of the plan takes its lowest and its highest value: 0 and n_terms - 1, ids that
    differ from 0 in one digit only (that digit at 1 and at its highest value), ids that differ from n_terms - 1 in one digit
    only, among uniform ids."""
    _, digits = plan(n_terms)
    top = n_terms - 1
    special = [0, top]
    for b, sh in zip(digits, shifts(digits)):
        mask = (1 << b) - 1
        high = min(mask, top >> sh)                       # the highest value this digit takes below n_terms
        for v in (1, high):
            if (v << sh) < n_terms:
                special.append(v << sh)
        for v in (0, high):
            x = (top & ~(mask << sh)) | (v << sh)
            if x < n_terms:
                special.append(x)
    ids = rng.integers(0, n_terms, n).astype(np.uint32)
    at = np.arange(0, n, 3)
    ids[at] = np.asarray(special, dtype=np.uint32)[rng.integers(0, len(special), len(at))]
    ids[:len(special)] = special                          # each of them at least once
    return ids


def drop(ids, where, n_terms):
    """ids with the positions `where` (bool mask or indices) replaced by the dropped termIds, in rotation"""
    ids = np.array(ids, dtype=np.uint32)
    idx = np.flatnonzero(where) if np.asarray(where).dtype == bool else np.asarray(where)
    bad = np.asarray(BAD_IDS(n_terms), dtype=np.uint32)
    ids[idx] = bad[np.arange(len(idx)) % len(bad)]
    return ids


# ---- the case table ----------------------------------------------------------------------------------------------------------
INSTANTIATION_TERMS = [(1024, [10]), (2048, [11]), (2049, [8, 8]), ((1 << 18) + 1, [10, 9]), ((1 << 19) + 1, [10, 10]), ((1 << 20) + 1, [11, 10]),
                       ((1 << 21) + 1, [11, 11]), (1 << 22, [11, 11]), ((1 << 22) + 1, [8, 8, 8]), ((1 << 24) + 1, [9, 8, 8])]
SCAN_TERMS = 2048                # one pass of 11 bits: 2048 counters per tile
DOC_TERMS = 300                  # one pass of 9 bits: only the first pass's docId logic varies
DROP_TERMS = 70000               # two passes: the second reads the number of kept pairs from the device


def instantiation_cases(T):
    out = []
    for i, (n_terms, digits) in enumerate(INSTANTIATION_TERMS):
        assert plan(n_terms)[1] == digits, (n_terms, digits)
        rng = np.random.default_rng(100 + i)
        n = 3 * T + 17
        group = "huge" if n_terms > (1 << 23) else "inst"
        out.append(Case("inst_%d" % n_terms, docs_for(n, rng), with_tf(spread_ids(n_terms, n, rng)), n_terms, group))
    return out


def scan_cases(T):
    """2048 counters per tile: 512 tiles are 2^20 counters, the last size k_iv_scan_top takes in one round; 513 tiles and a pair
    take two."""
    out = []
    for name, n in (("scan_one_round_full", 512 * T), ("scan_two_rounds", 513 * T + 1)):
        rng = np.random.default_rng(7)
        counts = np.full(n // 64 + 1, 64, dtype=np.uint32)
        counts[-1] = n - 64 * (n // 64)
        out.append(Case(name, counts, with_tf(rng.integers(0, SCAN_TERMS, n)), SCAN_TERMS, "scan"))
    return out


def doc_cases(T):
    rng = np.random.default_rng(21)
    ids = lambda n: rng.integers(0, DOC_TERMS, n)   # noqa: E731
    mk = lambda name, counts: Case(name, np.asarray(counts, dtype=np.uint32), with_tf(ids(int(np.sum(counts)))), DOC_TERMS, "docs")   # noqa: E731
    out = [mk("doc_of_T_then_doc_on_pair0", [T, 37]),
           mk("doc_over_whole_tiles", [3 * T + 17]),
           mk("T_docs_of_one_pair", [1] * T + [3] * 30)]
    # 1000 empty documents at the very start, exactly on a tile boundary, in the middle of a tile and after the last pair
    first_tile = list(docs_for(T, rng, 1, 40))
    out.append(mk("runs_of_empty_docs", [0] * 1000 + first_tile + [0] * 1000 + list(docs_for(700, rng, 1, 40)) + [0] * 1000
                  + list(docs_for(900, rng, 1, 40)) + [0] * 1000))
    for r in (1, 63, 64, 65, T - 1):
        out.append(mk("last_tile_of_%d" % r, docs_for(T + r, rng)))
    for n in (1, 63):
        out.append(mk("n_%d" % n, docs_for(n, rng, 1, 9)))
    return out


def one_digit_cases(T):
    n = 2 * T + 5
    rng = np.random.default_rng(33)
    out = [Case("one_term_of_one", docs_for(n, rng), with_tf(np.zeros(n)), 1, "digit"),
           Case("one_term_of_70000", docs_for(n, rng), with_tf(np.full(n, 54321)), 70000, "digit")]
    per_tile = np.asarray([69999, 0, 40000, 255, 256], dtype=np.uint32)          # a tile is one run of one id; the last tile is partial
    n = 4 * T + 5
    out.append(Case("one_term_per_tile", docs_for(n, rng), with_tf(per_tile[np.arange(n) // T]), 70000, "digit"))
    return out


def equal_pair_cases(T):
    """200 copies of one (term, doc) pair, six pairs apart, from before the last wave of tile 0 into tile 1: neighbours lie in
    different steps of a wave, in different waves and in different tiles.  All of them belong to document 1."""
    rng = np.random.default_rng(44)
    wave = T // 4
    counts = [T - wave - 200, wave + 600, 500]
    n = sum(counts)
    ids = rng.integers(0, DOC_TERMS, n)
    ids[T - wave - 60 + 6 * np.arange(200)] = 123
    return [Case("equal_pairs", np.asarray(counts, dtype=np.uint32), with_tf(ids), DOC_TERMS, "docs")]


def dropped_cases(T):
    nt = DROP_TERMS
    rng = np.random.default_rng(55)
    out = []

    def mk(name, n, where):
        ids = drop(spread_ids(nt, n, rng), where(n), nt)
        out.append(Case(name, docs_for(n, rng), with_tf(ids), nt, "drop"))

    def span(lo, hi):
        return lambda n: (np.arange(n) >= lo) & (np.arange(n) < hi)

    mk("every_second_dropped", 3 * T + 17, lambda n: np.arange(n) % 2 == 1)
    mk("first_tile_dropped", 3 * T + 17, span(0, T))
    mk("middle_tile_dropped", 3 * T + 17, span(T, 2 * T))
    mk("last_tile_dropped", 3 * T + 1000, span(3 * T, 4 * T))
    mk("all_dropped", 2 * T + 5, span(0, 4 * T))
    mk("one_kept", 2 * T + 5, lambda n: np.arange(n) != T + 7)
    for r in range(4):                                    # about half dropped, the number kept fixed modulo 4
        def where(n, r=r):
            bad = rng.random(n) < 0.5
            good = np.flatnonzero(~bad)
            bad[good[:(len(good) - r) % 4]] = True
            return bad
        mk("kept_mod4_%d" % r, 3 * T + 17, where)
    mk("kept_2T_of_4T", 4 * T, lambda n: (np.arange(n) // T) % 2 == 0)
    # k_iv_runs gives a thread four consecutive sorted keys: runs of 8, 12 and 4 pairs end on a thread's last key
    ids = np.repeat(np.asarray([69999, 7, 300], dtype=np.uint32), [8, 12, 4])
    ids = np.concatenate([ids, np.asarray(BAD_IDS(nt), dtype=np.uint32)])
    ids = ids[rng.permutation(len(ids))]
    out.append(Case("run_seams", docs_for(len(ids), rng, 0, 5), with_tf(ids), nt, "drop"))
    return out


def small_cases(T):
    """every case but the two scan sizes and 2^24 + 1 terms, which are tests of their own"""
    return [c for c in instantiation_cases(T) if c.group != "huge"] + doc_cases(T) + one_digit_cases(T) + equal_pair_cases(T) + dropped_cases(T)


def huge_cases(T):
    return [c for c in instantiation_cases(T) if c.group == "huge"]


def all_cases(T):
    return small_cases(T) + huge_cases(T) + scan_cases(T)


def upload_case(T):
    """for ns_segment_upload_inverted: the first and the last tile entirely dropped, so the stream is much shorter than announced.
    tf is 1 .. 5 here: the segment is scored."""
    n_terms, n = 700, 4 * T
    rng = np.random.default_rng(66)
    ids = drop(rng.integers(0, n_terms, n), (np.arange(n) < T) | (np.arange(n) >= 3 * T), n_terms)
    pairs = np.stack([ids, rng.integers(1, 6, n).astype(np.uint32)], axis=1)
    return Case("upload_first_and_last_tile_dropped", docs_for(n, rng, 0, 40), pairs, n_terms, "upload")


# ---- reach -------------------------------------------------------------------------------------------------------------------
FLAGS = (["inst(%d,%s,%s)" % (b, f, l) for b in (8, 9, 10, 11) for f, l in (("T", "T"), ("T", "F"), ("F", "T"))] + ["inst(8,F,F)"]
         + ["third_pass", "scan_top_one_round_full", "scan_top_two_rounds", "tile_no_doc_start", "doc_starts_on_tile_pair0",
            "gt256_starts_in_tile", "empties_leading", "empties_on_tile_boundary", "empties_trailing"]
         + ["partial_last_tile_%s" % r for r in ("1", "63", "64", "65", "T-1")]
         + ["n_lt_64", "one_digit_tile", "equal_pairs_across_lane_group", "equal_pairs_across_wave", "equal_pairs_across_tile",
            "tile_all_dropped_first", "tile_all_dropped_middle", "tile_all_dropped_last", "later_pass_tile_past_kept",
            "kept_zero_multi_pass", "kept_mod4_0", "kept_mod4_1", "kept_mod4_2", "kept_mod4_3", "run_seam_at_thread_boundary"])


def reach(case, T, df, postings):
    """the set of flags of one case; df, postings: the oracle's output for it"""
    counts, pairs, n_terms = case.counts, case.pairs, case.n_terms
    n, n_docs = len(pairs), len(counts)
    ids = pairs[:, 0]
    keep = ids < n_terms
    kept = int(keep.sum())
    assert kept == len(postings) == int(np.sum(df, dtype=np.uint64))
    n_tiles = -(-n // T)
    _, digits = plan(n_terms)
    tile_of = np.arange(n) // T
    prefix = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    doc = np.repeat(np.arange(n_docs), counts)                         # the document of every pair
    got = set()

    for p, b in enumerate(digits):                                     # a pass counts when it has an item to place
        if (n if p == 0 else kept) > 0:
            got.add("inst(%d,%s,%s)" % (b, "T" if p == 0 else "F", "T" if p == len(digits) - 1 else "F"))
        m = (1 << b) * n_tiles                                         # the counters k_iv_scan_* scan; 1024 per block sum
        if m == 1 << 20:
            got.add("scan_top_one_round_full")
        if 1024 < -(-m // 1024) <= 2048:
            got.add("scan_top_two_rounds")
    if len(digits) == 3 and kept > 0:
        got.add("third_pass")

    if n:
        t_first, t_last = np.arange(n_tiles) * T, np.minimum(np.arange(1, n_tiles + 1) * T, n) - 1
        if np.any(doc[t_first] == doc[t_last]):                       # the marking loop of the first pass has nothing to mark
            got.add("tile_no_doc_start")
        starts = np.flatnonzero(np.diff(doc)) + 1                     # the pairs at which a document starts, but for pair 0
        if np.any(starts % T == 0):
            got.add("doc_starts_on_tile_pair0")
        if len(starts) and np.bincount(starts // T).max() > 256:      # more than one stride of the 256 marking threads
            got.add("gt256_starts_in_tile")
        empty = np.flatnonzero(counts == 0)
        if n_docs >= 2 and not counts[:2].any():
            got.add("empties_leading")
        if n_docs >= 2 and not counts[-2:].any():
            got.add("empties_trailing")
        at = prefix[empty]
        if np.any((at % T == 0) & (at > 0) & (at < n)):
            got.add("empties_on_tile_boundary")
        if n > T:
            for r, name in ((1, "1"), (63, "63"), (64, "64"), (65, "65"), (T - 1, "T-1")):
                if n % T == r:
                    got.add("partial_last_tile_" + name)
        if n < 64:
            got.add("n_lt_64")

        # a full tile of kept pairs with one value of the first pass's digit: one counter per wave reaches T / 4, the tile's T
        d0 = (ids.astype(np.int64) & ((1 << digits[0]) - 1))
        for t in range(n // T):
            s = slice(t * T, (t + 1) * T)
            if keep[s].all() and (d0[s] == d0[t * T]).all():
                got.add("one_digit_tile")

        # equal (term, doc) pairs that are neighbours among their copies, and where the two lie
        key = ids.astype(np.int64) * max(n_docs, 1) + doc
        order = np.argsort(key, kind="stable")
        same = np.flatnonzero((key[order][1:] == key[order][:-1]) & keep[order][1:])
        i, j = order[same], order[same + 1]
        wave = T // 4
        if np.any((i // LANES != j // LANES) & (i // wave == j // wave)):
            got.add("equal_pairs_across_lane_group")
        if np.any((i // wave != j // wave) & (i // T == j // T)):
            got.add("equal_pairs_across_wave")
        if np.any(i // T != j // T):
            got.add("equal_pairs_across_tile")

        kept_per_tile = np.bincount(tile_of, weights=keep, minlength=n_tiles)
        if n_tiles >= 3 and kept > 0:
            if kept_per_tile[0] == 0:
                got.add("tile_all_dropped_first")
            if np.any(kept_per_tile[1:-1] == 0):
                got.add("tile_all_dropped_middle")
            if kept_per_tile[-1] == 0:
                got.add("tile_all_dropped_last")
        if len(digits) >= 2 and kept > 0 and -(-kept // T) < n_tiles:   # a later pass's workgroup whose first item lies past the kept ones
            got.add("later_pass_tile_past_kept")
        if len(digits) >= 2 and kept == 0:
            got.add("kept_zero_multi_pass")
        if 0 < kept < n:                                               # k_iv_runs reads the count from the device; its last thread has kept % 4 keys
            got.add("kept_mod4_%d" % (kept % 4))

        # in the sorted keys, a run longer than a thread's four keys ends on index 4t + 3 and another such run starts on 4t + 4
        skeys = np.repeat(np.arange(n_terms), df) if n_terms <= (1 << 20) else np.sort(ids[keep])
        ends = np.flatnonzero(np.diff(skeys)) if kept else np.zeros(0, dtype=np.int64)
        for e in ends[ends % 4 == 3]:
            if df[skeys[e]] >= 4 and df[skeys[e + 1]] >= 4:
                got.add("run_seam_at_thread_boundary")
                break
    return got


# ---- corpora for the sorts of ns_forward_build (ig_sort by term over n_terms, then by document over n_docs) ---------------------
def word(i):
    return b"w%05dx" % i                                              # at least two bytes and no stop word: every token is kept


def corpus(n_docs, n_words, per_doc, seed, empty_every=0):
    """n_docs texts over n_words distinct words, every word used: document d holds its share of the words in order, then random
    ones, some of them twice"""
    rng = np.random.default_rng(seed)
    share = -(-n_words // n_docs)
    texts = []
    for d in range(n_docs):
        if empty_every and d % empty_every == empty_every - 1:
            texts.append(b"")
            continue
        own = [w % n_words for w in range(d * share, (d + 1) * share)]
        ws = own + [int(x) for x in rng.integers(0, n_words, per_doc)]
        texts.append(b" ".join(word(w) for w in ws))
    return texts


def ingest_corpora():
    """(name, texts, digits of the sort by term, digits of the sort by document)"""
    return [("docs_11_bits", corpus(1500, 300, 6, 1, empty_every=50), [9], [11]),
            ("terms_11_bits", corpus(40, 1500, 60, 2), [11], [8]),
            ("both_11_bits", corpus(1500, 1500, 6, 3, empty_every=50), [11], [11])]


def sparse_corpus(n_docs=(1 << 22) + 1, n_full=2000, seed=9):
    """-> (ids of the non-empty documents, ascending, their texts): the first and the last document are among them, and the ids
    differ in every digit of plan(n_docs)"""
    rng = np.random.default_rng(seed)
    ids = np.unique(np.concatenate([[0, n_docs - 1], rng.integers(0, n_docs, n_full)]))
    texts = [b" ".join(word(int(w)) for w in rng.integers(0, 50, int(rng.integers(1, 5)))) for _ in ids]
    return ids, texts


def sparse_offsets(n_docs, ids, texts):
    """the u64 offsets of ns_forward_build for n_docs documents of which `ids` hold `texts` and the others nothing"""
    lens = np.zeros(n_docs + 1, dtype=np.uint64)
    lens[np.asarray(ids) + 1] = [len(t) for t in texts]
    return np.cumsum(lens, dtype=np.uint64)
