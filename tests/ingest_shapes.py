"""Directed shapes for the tokeniser and the dictionary stage of csrc/ns_ingest.hip (k_ig_text, k_ig_keep, k_ig_kept,
k_ig_hash_long, k_ig_insert) and for the same dictionary kernels under compaction (k_cp_hash in csrc/ns_compact.hip).  Numpy
and Python only; no device is touched.

A case is (name, group, blob, offs): the text of all documents back to back and the u64 offsets of its len(offs) - 1 documents,
the arguments of ns_forward_build.  Tokens and document boundaries sit at stated ABSOLUTE byte offsets: a Canvas is filled with
separator bytes and the tokens are put where the case wants them.  What the device must return is ingest_ref.build over the
documents; oracle() below says the same a second way, with a byte loop instead of a regular expression, and also yields the raw
tokens (dropped ones included) with their positions, which the reach flags and the exact token count need.

reach(case) names the paths of the kernels that a case takes.  Each flag is a condition on the input bytes, the offsets, the
hash as restated here (term_hash, home_slot) and the oracle's output; nothing a device returned enters it.  FLAGS is the list the
whole table must reach and NAMED the flags each case is built for; tests/test_ingest_shapes_cpu.py asserts both, and that the
constants and the hash restated here are those of csrc/ns_ingest_text.hpp."""
import collections
import functools

import numpy as np

THREAD = 16                      # text bytes per thread of k_ig_text
TILE = 4096                      # kIgTile: text bytes per workgroup
LONG = 1024                      # kIgLong: longer tokens are hashed by a workgroup
CHUNKS = 256                     # the threads of k_ig_hash_long
MIN_TABLE = 1024                 # kIgMinTable: the smallest dictionary table (table_slots below is ig_table_slots)
P = 0x9E3779B97F4A7C15           # kIgP
M64 = (1 << 64) - 1

DIGITS, UPPER, LOWER = b"0123456789", b"ABCDEFGHIJKLMNOPQRSTUVWXYZ", b"abcdefghijklmnopqrstuvwxyz"
ALNUM = DIGITS + UPPER + LOWER
IS_ALNUM = [c in ALNUM for c in range(256)]
TO_LOWER = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))
STOP = tuple(w.encode() for w in ("the", "a", "an", "and", "or", "of", "to", "in", "for", "on", "with", "by", "as", "is", "are", "was",
                                  "were", "be", "been", "it", "this", "that", "from", "at"))
STOP2 = tuple(w for w in STOP if len(w) >= 2)          # what the stop rule (not the length rule) drops
NEXT_TO_ALNUM = b"/:@[`{"                               # '0' - 1, '9' + 1, 'A' - 1, 'Z' + 1, 'a' - 1, 'z' + 1
SEPS = b" .,;\x00\xff/:@[`{-\n\t\x80"

Case = collections.namedtuple("Case", "name group blob offs")


# ---- the oracle: a byte loop and a first-occurrence dictionary -----------------------------------------------------------------
def lower(b):
    return bytes(b).translate(TO_LOWER)


def raw_tokens(blob, offs):
    """-> [(start, end, doc)]: maximal runs of alnum bytes inside each document; `end` is one past the last byte"""
    out = []
    for d in range(len(offs) - 1):
        i, e = int(offs[d]), int(offs[d + 1])
        while i < e:
            if not IS_ALNUM[blob[i]]:
                i += 1
                continue
            j = i + 1
            while j < e and IS_ALNUM[blob[j]]:
                j += 1
            out.append((i, j, d))
            i = j
    return out


def _oracle(blob, offs):
    toks = raw_tokens(blob, offs)
    kept = [(s, e, d) for s, e, d in toks if e - s >= 2 and lower(blob[s:e]) not in STOP]
    term_id, terms, tf_total = {}, [], []
    kept_docs, doc_len, counts, pairs = [], [], [], []
    at = 0
    while at < len(kept):
        d, tf = kept[at][2], {}
        end = at
        while end < len(kept) and kept[end][2] == d:
            t = lower(blob[kept[end][0]:kept[end][1]])
            tid = term_id.get(t)
            if tid is None:
                tid = term_id[t] = len(terms)
                terms.append(t)
                tf_total.append(0)
            tf[tid] = tf.get(tid, 0) + 1
            tf_total[tid] += 1
            end += 1
        kept_docs.append(d)
        doc_len.append(end - at)
        counts.append(len(tf))
        pairs.extend(sorted(tf.items()))
        at = end
    return {"tokens": toks, "kept": kept, "n_tokens": len(toks), "kept_tokens": len(kept), "tf_total": tf_total,
            "kept_docs": np.asarray(kept_docs, dtype=np.uint32), "doc_len": np.asarray(doc_len, dtype=np.uint32),
            "counts": np.asarray(counts, dtype=np.uint32), "pairs": np.asarray(pairs, dtype=np.uint32).reshape(-1, 2), "terms": terms}


@functools.lru_cache(maxsize=None)
def _oracle_by_name(name):
    c = case_by_name(name)
    return _oracle(c.blob, c.offs)


def oracle(case):
    """the expected forward index in ingest_ref.build's form plus tokens / kept [(start, end, doc)], n_tokens, kept_tokens,
    tf_total per term; computed once per case of the table"""
    return _oracle_by_name(case.name) if case.name in _names() else _oracle(case.blob, case.offs)


def texts_of(case):
    return [case.blob[int(case.offs[d]):int(case.offs[d + 1])] for d in range(len(case.offs) - 1)]


# ---- the hash and the table, restated -------------------------------------------------------------------------------------------
def mix(h):
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    return h ^ (h >> 33)


def term_hash(b):
    h = 0
    for c in b:
        h = (h * P + c + 1) & M64
    return mix(h ^ len(b))


def table_slots(n_kept):
    cap = MIN_TABLE
    while cap < 2 * n_kept:
        cap <<= 1
    return cap


def home_slot(b, n_kept):
    return term_hash(b) & (table_slots(n_kept) - 1)


def chunk_tail_empty(length):
    """a token hashed by a workgroup whose last threads get no bytes"""
    chunk = -(-length // CHUNKS)
    return length > LONG and (CHUNKS - 1) * chunk >= length


# ---- building blocks -----------------------------------------------------------------------------------------------------------
class Canvas:
    """n separator bytes (every kind, by position); put() writes bytes at an absolute offset, once"""

    def __init__(self, n):
        self.buf = bytearray(SEPS[i % len(SEPS)] for i in range(n))
        self.used = bytearray(n)
        self.bounds = [0]

    def put(self, at, b):
        assert 0 <= at and at + len(b) <= len(self.buf) and not any(self.used[at:at + len(b)]), (at, len(b))
        self.buf[at:at + len(b)] = b
        self.used[at:at + len(b)] = b"\x01" * len(b)
        return at + len(b)

    def sep(self, at, b):
        """a chosen separator byte (not marked used: it is no token)"""
        assert not IS_ALNUM[b] and not self.used[at]
        self.buf[at] = b

    def boundary(self, at, times=1):
        """a document starts at `at`; times > 1: times - 1 empty documents in front of it"""
        assert self.bounds[-1] <= at <= len(self.buf)
        self.bounds.extend([at] * times)

    def case(self, name, group):
        return Case(name, group, bytes(self.buf), np.asarray(self.bounds + [len(self.buf)], dtype=np.uint64))


def from_texts(name, group, texts):
    offs = np.zeros(len(texts) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(t) for t in texts], dtype=np.uint64)
    return Case(name, group, b"".join(texts), offs)


def rand_token(rng, length):
    return bytes(np.frombuffer(ALNUM, dtype=np.uint8)[rng.integers(0, len(ALNUM), length)])


def word(i):
    return b"w%04d" % i


# ---- group `edges`: k_ig_text ---------------------------------------------------------------------------------------------------
SWEEP_SLOT = 96


def sweep_case():
    """start mod 32 = 0 .. 31 times length 1 .. 34, each once, in a slot of its own; a document every four slots"""
    rng = np.random.default_rng(11)
    combos = [(a, ln) for a in range(32) for ln in range(1, 35)]
    cv = Canvas(len(combos) * SWEEP_SLOT)
    for k, (a, ln) in enumerate(combos):
        if k and k % 4 == 0:
            cv.boundary(k * SWEEP_SLOT)
        cv.put(k * SWEEP_SLOT + a, rand_token(rng, ln))
    return cv.case("sweep", "edges")


def sweep_tight_case():
    """the same lengths with ONE separator byte between tokens: both neighbours of every thread edge are live"""
    rng = np.random.default_rng(12)
    lengths = [ln for _ in range(3) for ln in range(1, 35)] + [int(x) for x in rng.integers(1, 35, 400)]
    cv = Canvas(sum(lengths) + len(lengths))
    at = 0
    for k, ln in enumerate(lengths):
        if k and k % 50 == 0:
            cv.boundary(at)
        at = cv.put(at, rand_token(rng, ln)) + 1
    return cv.case("sweep_tight", "edges")


TEXT_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8192)


def length_case(n):
    """n bytes of tokens; the last one, `Qz`, ends at n"""
    rng = np.random.default_rng(100 + n)
    cv = Canvas(n)
    at = 0
    while at < n - 3:
        tok = rand_token(rng, int(rng.integers(1, 8)))[:n - 3 - at]
        at = cv.put(at, tok) + 1
    cv.put(max(0, n - 2), b"Qz"[-min(n, 2):])
    if n >= 16:
        cv.boundary(n // 2)
    return cv.case("len_%d" % n, "edges")


def tile_straddle_case():
    """tokens over a tile edge with one byte on the far side / on the near side, and one that ends on the edge exactly"""
    cv = Canvas(4 * TILE - 5)
    cv.put(TILE - 6, b"Straddl")                  # [4090, 4097): one byte in tile 1
    cv.put(2 * TILE - 1, b"sTRADDLE")             # [8191, 8199): one byte in tile 1
    cv.put(3 * TILE - 4, b"Edge")                 # ends on the edge; the next tile starts with a separator
    cv.put(3 * TILE + 1, b"after")
    cv.put(0, b"first")
    cv.put(4 * TILE - 9, b"Last")
    cv.boundary(2 * TILE + 7)
    return cv.case("tile_straddle", "edges")


def dense_docs_case():
    """4096 documents of one alnum byte: 4096 starts and 4096 ends in tile 0, all dropped; `zz` survives"""
    body = bytes(ALNUM[i % len(ALNUM)] for i in range(TILE))
    offs = np.asarray(list(range(TILE + 1)) + [TILE + 2], dtype=np.uint64)
    return Case("dense_docs", "edges", body + b"zz", offs)


def dense_nodocs_case():
    return from_texts("dense_nodocs", "edges", [b"a." * TILE + b"zz"])


DOCSPLIT_RESIDUES = (0, 1, 15, 16, 17, 31)


def docsplit_case():
    """document boundaries inside alnum runs (no separator between the documents), at every listed residue mod 32, at a
    multiple of 4096, and two and three at one offset (empty documents in the middle of a word)"""
    cv = Canvas(TILE + 1024)
    for k, r in enumerate(DOCSPLIT_RESIDUES):
        o = 128 * (k + 1) + r
        cv.put(o - 5, b"LeftH" + b"rigHt")
        cv.boundary(o)
    for k, (r, times) in enumerate(((0, 2), (16, 2), (0, 3), (16, 3), (7, 2))):
        o = 1024 + 128 * k + r
        cv.put(o - 4, b"emp" + b"T" + b"Ydoc")
        cv.boundary(o, times)
    cv.put(TILE - 6, b"tileEn" + b"Dstart")
    cv.boundary(TILE)
    cv.put(TILE + 1000, b"tail")
    return cv.case("docsplit", "edges")


def docsplit_last_word_case(n, o):
    cv = Canvas(n)
    cv.put(o - 4, (b"abcD" + b"Efgh")[:4 + n - o])
    cv.boundary(o)
    return cv.case("docsplit_last_word_%d" % o, "edges")


def two_byte_docs_case():
    """abcdabcd..., a document every 2 bytes: every second bit of the document bitmap is set"""
    n_docs = (TILE + 64) // 2
    return from_texts("two_byte_docs", "edges", [(b"aB", b"Cd")[d & 1] for d in range(n_docs)])


def lowercase_case():
    """upper-case letters at every position mod 16, each pair over the next position too (15 -> the next thread's byte 0), with
    the six bytes next to the alnum ranges on both sides; a run of upper case over three threads"""
    cv = Canvas(64 * 16 + 128)
    for p in range(16):
        at = 64 * p + 16 + p
        cv.sep(at - 1, NEXT_TO_ALNUM[p % 6])
        cv.put(at, bytes([UPPER[p], UPPER[25 - p]]))
        cv.sep(at + 2, NEXT_TO_ALNUM[(p + 3) % 6])
    cv.put(64 * 16 + 7, UPPER + DIGITS + UPPER[::-1])
    return cv.case("lowercase", "edges")


def all_bytes_case():
    """xq?zq with every byte value in the middle, a document each"""
    return from_texts("all_bytes", "edges", [b"xq" + bytes([c]) + b"zq" for c in range(256)])


def edges_cases():
    return ([sweep_case(), sweep_tight_case()] + [length_case(n) for n in TEXT_LENGTHS]
            + [tile_straddle_case(), dense_docs_case(), dense_nodocs_case(), docsplit_case(), docsplit_last_word_case(35, 32),
               docsplit_last_word_case(50, 48), two_byte_docs_case(), lowercase_case(), all_bytes_case()])


# ---- group `keep`: k_ig_keep ----------------------------------------------------------------------------------------------------
def mixed(w):
    """neither w nor w.upper(): the first byte lower, the rest upper (one-byte words: upper)"""
    return w[:1] + w[1:].upper() if len(w) > 1 else w.upper()


def stop_forms_case():
    texts = []
    for i, w in enumerate(STOP):
        forms = [w, w.upper(), mixed(w), w.capitalize(), w + b"x", w + b"1", b"x" + w, w[:-1], w.upper() + b"X", b"9" + w.upper()]
        texts.append(SEPS[i % len(SEPS):i % len(SEPS) + 1].join(forms) + b"\n")
    texts.append(b"an and anda ana AN AND ANDA ANA an. and, wit with witx with")
    return from_texts("stop_forms", "keep", texts)


def stop_first_last_case():
    return from_texts("stop_first_last", "keep", [b"the quick fox", b" jumps with"])


def stop_only_case():
    return from_texts("stop_only", "keep", [b"THE"])


FOUR = (b"with", b"were", b"been", b"this", b"that", b"from")


def stop_across_edges_case():
    """four-byte stop words with 1, 2 and 3 bytes in front of a 16-byte edge and of a tile edge; next to each, the same word
    with its last byte changed, which stays"""
    cv = Canvas(3 * TILE + 64)
    for k, (edge, front) in enumerate(((48, 1), (112, 2), (176, 3), (TILE, 1), (2 * TILE, 2), (3 * TILE, 3))):
        w = FOUR[k]
        cv.put(edge - front, w.upper() if k & 1 else w)
        cv.put(edge - front + 32, w[:3] + b"q")
    cv.boundary(TILE + 100)
    return cv.case("stop_across_edges", "keep")


def stop_split_case():
    """th|e: `th` stays, `e` goes.  wi|th: both stay.  an|d: both go.  t|he, fro|m, b|e|en with an empty document inside"""
    cv = Canvas(256)
    for at, w, cut in ((8, b"the", 2), (40, b"wiTH", 2), (72, b"and", 2), (100, b"The", 1), (135, b"from", 3), (170, b"been", 1)):
        cv.put(at, w)
        cv.boundary(at + cut)
    cv.boundary(172, 2)
    cv.put(200, b"keep")
    return cv.case("stop_split", "keep")


def one_byte_case():
    return from_texts("one_byte_tokens", "keep", [b"".join(bytes([c, SEPS[i % len(SEPS)]]) for i, c in enumerate(ALNUM)) + b"ok"])


def keep_cases():
    return [stop_forms_case(), stop_first_last_case(), stop_only_case(), stop_across_edges_case(), stop_split_case(), one_byte_case()]


# ---- group `long`: k_ig_kept / k_ig_hash_long -----------------------------------------------------------------------------------
LONG_LENGTHS = (1023, 1024, 1025, 1279, 1280, 1281, 65536, 70001)


def other_byte(c):
    return b"0" if c != b"0" else b"1"


def long_tokens(length):
    """-> (token, [first byte differs, last byte differs, last byte removed])"""
    t = rand_token(np.random.default_rng(7000 + length), length)
    return t, [other_byte(t[:1]) + t[1:], t[:-1] + other_byte(t[-1:]), t[:-1]]


def long_case(length):
    """document 0: the token twice in different letter case (tf 2) and a sibling; document 1: the other siblings and the token
    again, so that both halves of the case hold it"""
    t, sib = long_tokens(length)
    return from_texts("long_%d" % length, "long", [b"head " + t + b" " + t.swapcase() + b"," + sib[0] + b".", sib[1] + b" " + t.upper() + b"\x00" + sib[2]])


def long_cases():
    return [long_case(n) for n in LONG_LENGTHS]


# ---- group `dict`: k_ig_insert --------------------------------------------------------------------------------------------------
WRAP_LAST = (46, 153, 380, 480)          # word(i) with home slot 1023 of 1024
WRAP_BEFORE = (3764, 4602, 6026)         # ... with home slot 1022


def wrap_case():
    """seven terms whose home slots are the table's last two: at least five of them are placed past the last slot, in slot 0
    onwards.  Interleaved with other terms, repeated in other letter case, in both halves of the documents."""
    special = [word(i) for i in WRAP_LAST + WRAP_BEFORE]
    texts = []
    for d in range(6):
        parts = []
        for j, w in enumerate(special[d % 3:] + special[:d % 3]):
            parts += [b"filler%d" % ((d * 7 + j) % 23), w.upper() if (d + j) & 1 else w, b"of"]
        texts.append(b" ".join(parts))
    return from_texts("wrap", "dict", texts)


def load_case(n_terms):
    """n_terms kept tokens, all distinct, eight to a document, with dropped tokens in between"""
    texts = []
    for at in range(0, n_terms, 8):
        texts.append(b" the ".join(b"t%04d" % i if i & 1 else b"T%04d" % i for i in range(at, min(n_terms, at + 8))) + b" a\n")
    return from_texts("load_%d" % n_terms, "dict", texts)


def first_occurrence_case():
    return from_texts("first_occurrence", "dict", [b"The A OF", b"ZEBRA apple Zebra", b"a I", b"apple zebra mango", b"MANGO Apple kiwi"])


def same_bytes_case():
    doc = b"Alpha beta, gamma-alpha. BETA"
    return from_texts("same_bytes", "dict", [doc, doc, b"", doc.upper(), doc.lower(), b"delta " + doc])


def dict_cases():
    return [wrap_case(), load_case(512), load_case(513), first_occurrence_case(), same_bytes_case()]


# ---- group `docs`: k_ig_docmark, the binary search of k_ig_kept, k_ig_docemit ------------------------------------------------------
N_DOCS = (1, 2, 3, 255, 256, 257)


def ndocs_case(n_docs):
    return from_texts("ndocs_%d" % n_docs, "docs", [b"doc%d common Word%d " % (d, d % 7) for d in range(n_docs)])


def empty_docs_case():
    texts = ([b"", b"alpha beta", b"", b"gamma", b"", b"", b"delta alpha ", b"the of a", b"epsilon;", b"  ..  ", b"AND", b"b c", b" eta"]
             + [b""] * 300 + [b"zeta alpha", b"\x00\xff", b"theta", b""])
    return from_texts("empty_docs", "docs", texts)


def empty_mostly_case():
    """300 empty documents first, one kept document, 300 more, the text's end"""
    return from_texts("empty_mostly", "docs", [b""] * 300 + [b"only one"] + [b""] * 300)


def docs_cases():
    return [ndocs_case(n) for n in N_DOCS] + [empty_docs_case(), empty_mostly_case()]


# ---- the table -------------------------------------------------------------------------------------------------------------------
GROUPS = ("edges", "keep", "long", "dict", "docs")


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(edges_cases() + keep_cases() + long_cases() + dict_cases() + docs_cases())


@functools.lru_cache(maxsize=None)
def _names():
    return frozenset(c.name for c in all_cases())


def case_by_name(name):
    return next(c for c in all_cases() if c.name == name)


def cases_of(group):
    return [c for c in all_cases() if c.group == group]


def case_names(group):
    return [c.name for c in cases_of(group)]


def halves(case):
    """the documents of a case as two sources for compaction"""
    texts = texts_of(case)
    assert len(texts) >= 2
    return texts[:len(texts) // 2], texts[len(texts) // 2:]


# ---- reach -------------------------------------------------------------------------------------------------------------------------
FLAGS = ("start_at_thread_byte0", "end_at_thread_byte15", "token_spans_thread", "token_spans_tile", "partial_last_thread",
         "last_token_ends_at_n", "docsplit_sh0_bit16", "docsplit_sh16_nextword", "docsplit_last_word", "empty_docs_inside_run",
         "tile_4096_starts", "all_256_bytes", "stop_exact", "stop_plus_one", "stop_minus_one", "stop_split_by_doc",
         "len_1024_thread_hash", "len_1025_group_hash", "long_chunk_tail_empty", "long_twice_one_term", "long_siblings_distinct",
         "probe_wraps_table", "table_load_half", "table_doubles", "empty_first", "empty_last_at_n", "empty_run_300",
         "dropped_only_doc_between_kept")


def splits_inside_runs(case):
    """{offset: how many documents start there} for the document starts that have an alnum byte on both sides"""
    n, blob = len(case.blob), case.blob
    out = collections.Counter()
    for o in case.offs[1:-1].tolist():
        if 0 < o < n and IS_ALNUM[blob[o - 1]] and IS_ALNUM[blob[o]]:
            out[o] += 1
    return out


def run_around(blob, o):
    """the maximal alnum run around offset o, document boundaries ignored, lower-cased"""
    a, b = o, o
    while a > 0 and IS_ALNUM[blob[a - 1]]:
        a -= 1
    while b < len(blob) and IS_ALNUM[blob[b]]:
        b += 1
    return lower(blob[a:b])


def reach(case):
    blob, offs, n = case.blob, case.offs.tolist(), len(case.blob)
    n_docs = len(offs) - 1
    o = oracle(case)
    toks = o["tokens"]
    raw = collections.Counter(blob[s:e] for s, e, _ in toks if e - s <= 8)
    out = set()
    # k_ig_text: thread i0 / 16 reads text[i0 - 1] for a token on its byte 0 and text[i0 + 16] for one on its byte 15
    if any(s % THREAD == 0 and s > 0 for s, _, _ in toks):
        out.add("start_at_thread_byte0")
    if any(e % THREAD == 0 and e < n for _, e, _ in toks):
        out.add("end_at_thread_byte15")
    if any(s // THREAD != (e - 1) // THREAD for s, e, _ in toks):
        out.add("token_spans_thread")
    if any(s // TILE != (e - 1) // TILE for s, e, _ in toks):
        out.add("token_spans_tile")
    if n % THREAD:
        out.add("partial_last_thread")
    if toks and toks[-1][1] == n:
        out.add("last_token_ends_at_n")
    # the thread in front of the split has the token's end on its byte 15 and reads the split's bit: i0 = split - 16, so
    # i0 & 31 == 0 (bit 16 of its own word) when the split is 16 mod 32, 16 (bit 0 of the next word) when it is 0 mod 32
    splits = splits_inside_runs(case)
    if any(s % 32 == 16 for s in splits):
        out.add("docsplit_sh0_bit16")
    if any(s % 32 == 0 for s in splits):
        out.add("docsplit_sh16_nextword")
    if any(s % THREAD == 0 and s >> 5 == (n - 1) >> 5 for s in splits):
        out.add("docsplit_last_word")
    if any(times >= 2 for times in splits.values()):
        out.add("empty_docs_inside_run")
    if toks:
        n_tiles = (n + TILE - 1) // TILE
        starts = np.bincount(np.asarray([s for s, _, _ in toks]) // TILE, minlength=n_tiles)
        ends = np.bincount((np.asarray([e for _, e, _ in toks]) - 1) // TILE, minlength=n_tiles)
        if np.any((starts == TILE) & (ends == TILE)):
            out.add("tile_4096_starts")
    middles = {blob[offs[d] + 2] for d in range(n_docs) if offs[d + 1] - offs[d] == 5 and blob[offs[d]:offs[d] + 2] == b"xq" and blob[offs[d] + 3:offs[d + 1]] == b"zq"}
    if len(middles) == 256:
        out.add("all_256_bytes")
    # k_ig_keep
    if all(raw[w] and raw[w.upper()] and raw[mixed(w)] for w in STOP2):
        out.add("stop_exact")
    if all(any(raw[w + bytes([c])] for c in LOWER) and any(raw[w + bytes([c])] for c in DIGITS) and any(raw[bytes([c]) + w] for c in LOWER) for w in STOP2):
        out.add("stop_plus_one")
    if all(raw[w[:-1]] for w in STOP2):
        out.add("stop_minus_one")
    if any(run_around(blob, s) in STOP2 for s in splits):
        out.add("stop_split_by_doc")
    # k_ig_kept / k_ig_hash_long
    lens = {e - s for s, e, _ in o["kept"]}
    if LONG in lens:
        out.add("len_1024_thread_hash")
    if LONG + 1 in lens:
        out.add("len_1025_group_hash")
    if any(chunk_tail_empty(ln) for ln in lens):
        out.add("long_chunk_tail_empty")
    terms = set(o["terms"])
    for t, tf in zip(o["terms"], o["tf_total"]):
        if len(t) <= LONG:
            continue
        if tf >= 2 and len({blob[s:e] for s, e, _ in o["kept"] if e - s == len(t) and lower(blob[s:e]) == t}) >= 2:
            out.add("long_twice_one_term")
        if other_byte(t[:1]) + t[1:] in terms and t[:-1] + other_byte(t[-1:]) in terms and t[:-1] in terms:
            out.add("long_siblings_distinct")
    # k_ig_insert: more terms with a home among the last j slots than j: whatever the order of arrival, one is placed past the end
    if terms:
        cap = table_slots(o["kept_tokens"])
        homes = sorted((term_hash(t) & (cap - 1) for t in terms if len(t) <= 64), reverse=True)
        if any(cap - h <= j for j, h in enumerate(homes)):
            out.add("probe_wraps_table")
    if o["kept_tokens"] == MIN_TABLE // 2 == len(terms):
        out.add("table_load_half")
    if o["kept_tokens"] == MIN_TABLE // 2 + 1:
        out.add("table_doubles")
    # documents
    kept_docs = set(o["kept_docs"].tolist())
    has_raw = {d for _, _, d in toks}
    if n_docs > 1 and offs[1] == 0:
        out.add("empty_first")
    if n_docs > 1 and offs[n_docs - 1] == n and n > 0:
        out.add("empty_last_at_n")
    run = 0
    for d in range(n_docs):
        if offs[d + 1] == offs[d]:
            run += 1
            continue
        if run >= 300 and d in kept_docs:
            out.add("empty_run_300")
        run = 0
    if kept_docs and any(min(kept_docs) < d < max(kept_docs) for d in has_raw - kept_docs):
        out.add("dropped_only_doc_between_kept")
    return out


# the flags a case is built for
NAMED = {
    "sweep": ("start_at_thread_byte0", "end_at_thread_byte15", "token_spans_thread"),
    "sweep_tight": ("start_at_thread_byte0", "end_at_thread_byte15", "token_spans_thread", "token_spans_tile"),
    "len_1": ("partial_last_thread", "last_token_ends_at_n"), "len_15": ("partial_last_thread", "last_token_ends_at_n"),
    "len_16": ("last_token_ends_at_n",), "len_17": ("partial_last_thread", "last_token_ends_at_n", "token_spans_thread"),
    "len_4097": ("partial_last_thread", "last_token_ends_at_n", "token_spans_tile"), "len_8192": ("last_token_ends_at_n",),
    "tile_straddle": ("token_spans_tile", "partial_last_thread"),
    "dense_docs": ("tile_4096_starts", "last_token_ends_at_n"),
    "docsplit": ("docsplit_sh0_bit16", "docsplit_sh16_nextword", "empty_docs_inside_run"),
    "docsplit_last_word_32": ("docsplit_sh16_nextword", "docsplit_last_word", "last_token_ends_at_n"),
    "docsplit_last_word_48": ("docsplit_sh0_bit16", "docsplit_last_word", "last_token_ends_at_n"),
    "two_byte_docs": ("docsplit_sh0_bit16", "docsplit_sh16_nextword", "docsplit_last_word"),
    "all_bytes": ("all_256_bytes",),
    "stop_forms": ("stop_exact", "stop_plus_one", "stop_minus_one"),
    "stop_across_edges": ("token_spans_thread", "token_spans_tile"),
    "stop_split": ("stop_split_by_doc", "empty_docs_inside_run"),
    "long_1024": ("len_1024_thread_hash",),
    "long_1025": ("len_1025_group_hash", "long_chunk_tail_empty", "long_twice_one_term", "long_siblings_distinct"),
    "long_1279": ("long_twice_one_term", "long_siblings_distinct"),
    "long_1280": ("long_twice_one_term", "long_siblings_distinct"),
    "long_1281": ("long_chunk_tail_empty", "long_twice_one_term", "long_siblings_distinct"),
    "long_65536": ("long_twice_one_term", "long_siblings_distinct"),
    "long_70001": ("long_twice_one_term", "long_siblings_distinct"),
    "wrap": ("probe_wraps_table",), "load_512": ("table_load_half",), "load_513": ("table_doubles",),
    "empty_docs": ("empty_first", "empty_last_at_n", "empty_run_300", "dropped_only_doc_between_kept"),
    "empty_mostly": ("empty_first", "empty_last_at_n", "empty_run_300"),
}
