"""Autocomplete restated in Python for the tests (src/api_autocomplete.cpp + src/api_engine.cpp:91-107,:164-187), and
a writer of tiny hand-made indexes whose raw terms exercise the normalisation (legacy layout, the reference's format:
nextsearch-api_amd/host/index_format.hpp).  Test infrastructure only."""
import bisect
import os
import struct

_ALNUM = frozenset(b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")


def normalize(raw):
    """normalize_token: ASCII alnum bytes only (C locale), lower-cased"""
    return bytes(c for c in raw if c in _ALNUM).lower()


def split(user_input):
    """-> (base, prefix): the last alnum run (trailing non-alnum bytes skipped) is the prefix, lower-cased"""
    b = user_input
    end = len(b)
    while end > 0 and b[end - 1] not in _ALNUM:
        end -= 1
    start = end
    while start > 0 and b[start - 1] in _ALNUM:
        start -= 1
    return b[:start], b[start:end].lower()


def clamp_limit(limit):
    return max(1, min(int(limit), 10))


def read_lexicons(seg_dir):
    """{raw term: df} of one segment (first record of a term wins, as the loader's emplace does)"""
    files = sorted(f for f in os.listdir(seg_dir) if f.startswith("lexicon"))
    if "lexicon.bin" in files and any(f.startswith("lexicon_b") for f in files):
        files = [f for f in files if f.startswith("lexicon_b")]
    out = {}
    for fn in files:
        data = open(os.path.join(seg_dir, fn), "rb").read()
        (n,) = struct.unpack_from("<I", data, 0)
        pos = 4
        for _ in range(n):
            (ln,) = struct.unpack_from("<I", data, pos)
            term = data[pos + 4:pos + 4 + ln]
            pos += 4 + ln
            _tid, df, _off, _cnt = struct.unpack_from("<IIQI", data, pos)
            pos += 20
            out.setdefault(term, df)
    return out


def read_manifest(index_dir):
    data = open(os.path.join(index_dir, "manifest.bin"), "rb").read()
    (n,) = struct.unpack_from("<I", data, 0)
    pos, names = 4, []
    for _ in range(n):
        (ln,) = struct.unpack_from("<I", data, pos)
        names.append(data[pos + 4:pos + 4 + ln].decode())
        pos += 4 + ln
    return names


def write_manifest(index_dir, names):
    with open(os.path.join(index_dir, "manifest.bin"), "wb") as f:
        f.write(struct.pack("<I", len(names)))
        for s in names:
            f.write(struct.pack("<I", len(s)) + s.encode())


def table(index_dir):
    """The sorted (term, score) table: df summed per raw term over the manifest's segments (u32 wrap), normalised,
    < 2 bytes dropped, duplicates kept, ordered by (bytes, score desc)."""
    sums = {}
    for name in read_manifest(index_dir):
        for term, df in read_lexicons(os.path.join(index_dir, "segments", name)).items():
            sums[term] = (sums.get(term, 0) + df) & 0xFFFFFFFF
    ents = [(normalize(t), s) for t, s in sums.items()]
    ents = [e for e in ents if len(e[0]) >= 2]
    ents.sort(key=lambda e: (e[0], -e[1]))
    return [e[0] for e in ents], [e[1] for e in ents]


_TOP_CACHE = {}


def _top10(terms, scores, prefix):
    """indices of the best 10 terms starting with prefix by (score desc, term asc); remembered per table and prefix"""
    key = (id(terms), id(scores), prefix)
    hit = _TOP_CACHE.get(key)
    if hit is not None and hit[0] is terms and hit[1] is scores:
        return hit[2]
    lo = bisect.bisect_left(terms, prefix)
    hi = lo
    while hi < len(terms) and terms[hi].startswith(prefix):
        hi += 1
    best = sorted(range(lo, hi), key=lambda i: (-int(scores[i]), terms[i]))[:10]
    _TOP_CACHE[key] = (terms, scores, best)
    return best


def suggest(terms, scores, user_input, limit):
    """The reference's answer over a sorted table: base + the best L terms with the prefix by (score desc, term asc)"""
    L = clamp_limit(limit)
    base, prefix = split(user_input)
    if not prefix or not terms:
        return []
    return [base + terms[i] for i in _top10(terms, scores, prefix)[:L]]


def write_tiny_index(index_dir, segments):
    """segments: one list of (raw term bytes, df) per segment.  Legacy layout, 8 docs per segment; a term with df 0 gets a
    record with count 0."""
    n_docs = 8
    os.makedirs(os.path.join(index_dir, "segments"), exist_ok=True)
    names = []
    for si, recs in enumerate(segments):
        name = "seg_%06d" % si
        names.append(name)
        d = os.path.join(index_dir, "segments", name)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "stats.bin"), "wb") as f:
            f.write(struct.pack("<If", n_docs, 100.0))
        with open(os.path.join(d, "docs.bin"), "wb") as f:
            f.write(struct.pack("<I", n_docs))
            for i in range(n_docs):
                uid = b"d%d_%d" % (si, i)
                f.write(struct.pack("<I", len(uid)) + uid + struct.pack("<I", 0) + struct.pack("<I", 0) + struct.pack("<I", 100))
        lex, inv, off = [], [], 0
        for tid, (term, df) in enumerate(recs):
            cnt = min(df, n_docs)
            lex.append(struct.pack("<I", len(term)) + term + struct.pack("<IIQI", tid, df, off, cnt))
            for doc in range(cnt):
                inv.append(struct.pack("<II", doc, 1))
            off += cnt * 8
        with open(os.path.join(d, "lexicon.bin"), "wb") as f:
            f.write(struct.pack("<I", len(recs)) + b"".join(lex))
        with open(os.path.join(d, "inverted.bin"), "wb") as f:
            f.write(b"".join(inv))
    write_manifest(index_dir, names)


# Raw terms that normalise alike, to fewer than 2 bytes, or carry a df of 0 (the tiny fixture index); the df sums of
# "co-vid" + "COVID" exceed neither u32 nor the others, but "wrap" is summed past 2^32 over the two segments.
TINY_SEGMENTS = [
    [(b"covid", 5), (b"co-vid", 3), (b"COVID", 2), (b"c", 9), (b"c.", 4), (b"-x-", 7), (b"ab", 0), (b"ab!", 1),
     (b"cat", 3), (b"car", 3), (b"Car", 1), (b"caf\xc3\xa9", 2), (b"wrap", 0xFFFFFFF0), (b"v1", 1), (b"v2", 1), (b"...", 6)],
    [(b"covid", 1), (b"cat", 2), (b"wrap", 0x20), (b"zz", 0), (b"Zz", 0), (b"c", 1), (b"cab", 5)],
]
