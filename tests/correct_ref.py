"""Spelling correction restated for the tests: which table entries are candidates, optimal string
alignment over bytes, the prefix rule, the ranking and the did_you_mean JSON.  Two versions of the search: plain Python for
small cases, and numpy over a fixed-width byte matrix (the whole dictionary per DP step) for the large ones.  Neither
uses a filter of the device's (no signature, no band): every eligible entry gets the full DP.  Test infrastructure only."""
import json

import numpy as np

import suggest_ref

MAX_LEN = 64      # NS_FUZZY_MAX_LEN
MAX_EDITS = 2
STOPWORDS = frozenset(b"the a an and or of to in for on with by as is are was were be been it this that from at".split())


def auto_edits(normalized_len):
    return 0 if normalized_len < 3 else 1 if normalized_len <= 5 else 2


def osa(a, b):
    """optimal string alignment distance of two byte strings (unbounded, full table)"""
    n, m = len(a), len(b)
    d = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        d[i][0] = i
    for j in range(m + 1):
        d[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            v = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
            if i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                v = min(v, d[i - 2][j - 2] + 1)
            d[i][j] = v
    return d[n][m]


def candidates(terms, scores):
    """per entry: score != 0 and not the same bytes as the entry before it"""
    return [int(scores[i]) != 0 and (i == 0 or terms[i] != terms[i - 1]) for i in range(len(terms))]


def fuzzy_plain(terms, scores, query, max_edits, prefix_len, L):
    """-> [(index, distance)] best first; L already clamped"""
    if not query or len(query) > MAX_LEN:
        return []
    p = query[:min(prefix_len, len(query))]
    cand = candidates(terms, scores)
    hits = []
    for i, t in enumerate(terms):
        if not cand[i] or abs(len(t) - len(query)) > max_edits or not t.startswith(p):
            continue
        d = osa(query, t)
        if d <= max_edits:
            hits.append((d, -int(scores[i]), i))
    hits.sort()
    return [(i, d) for d, _, i in hits[:L]]


def random_edits(rng, w, k, alphabet):
    """w after k random edits (deletion, insertion, substitution, transposition of neighbours), for the tests' queries"""
    w = bytearray(w)
    for _ in range(k):
        op = rng.randrange(4)
        pos = rng.randrange(len(w) + 1)
        if op == 0 and w:
            del w[min(pos, len(w) - 1)]
        elif op == 1:
            w.insert(pos, rng.choice(alphabet))
        elif op == 2 and w:
            w[min(pos, len(w) - 1)] = rng.choice(alphabet)
        elif len(w) >= 2:
            p = min(pos, len(w) - 2)
            w[p], w[p + 1] = w[p + 1], w[p]
    return bytes(w)


class Table:
    """The dictionary as a byte matrix: row i = term i, zero-padded to the widest term a query can reach."""

    def __init__(self, terms, scores):
        self.terms = terms
        self.n = len(terms)
        self.scores = np.asarray(scores, dtype=np.int64).reshape(self.n)
        self.lens = np.array([len(t) for t in terms], dtype=np.int64).reshape(self.n)
        self.width = max(1, min(int(self.lens.max()) if self.n else 1, MAX_LEN + MAX_EDITS))
        self.mat = np.zeros((self.n, self.width), dtype=np.uint8)
        for i, t in enumerate(terms):
            k = min(len(t), self.width)
            self.mat[i, :k] = np.frombuffer(t[:k], dtype=np.uint8)
        self.cand = np.asarray(candidates(terms, scores), dtype=bool).reshape(self.n)
        self._memo = {}

    def fuzzy(self, query, max_edits, prefix_len, L):
        """-> [(index, distance)] best first; L already clamped (the best 10 are remembered per query, edits and prefix)"""
        key = (query, max_edits, min(prefix_len, len(query)))
        if key not in self._memo:
            self._memo[key] = self._top10(query, max_edits, key[2])
        return self._memo[key][:L]

    def _top10(self, query, e, p):
        rows, d = self.within(query, e, p)
        order = np.lexsort((rows, -self.scores[rows], d))[:10]
        return [(int(rows[k]), int(d[k])) for k in order]

    def within(self, query, e, p):
        """-> (indices, distances) of every candidate within e edits of the query that shares its first p bytes"""
        none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
        n = len(query)
        if n == 0 or n > MAX_LEN or self.n == 0:
            return none
        q = np.frombuffer(query, dtype=np.uint8)
        ok = self.cand & (np.abs(self.lens - n) <= e)
        if p:
            pw = min(p, self.width)
            ok &= (self.lens >= p) & (self.mat[:, :pw] == q[:pw]).all(axis=1)
        rows = np.nonzero(ok)[0]
        if len(rows) == 0:
            return none
        W = min(self.width, n + e)                       # cells past column n + e never reach D[n][m], m <= n + e
        c = self.mat[rows, :W]
        R = len(rows)
        ar = np.arange(W + 1, dtype=np.int16)
        prev2 = None
        prev = np.broadcast_to(ar, (R, W + 1)).copy()    # D[0][j] = j
        for i in range(1, n + 1):
            cur = np.empty((R, W + 1), dtype=np.int16)
            cur[:, 0] = i
            sub = prev[:, :-1] + (c != q[i - 1])
            np.minimum(sub, prev[:, 1:] + 1, out=sub)
            if i > 1 and W > 1:
                tr = (c[:, :-1] == q[i - 1]) & (c[:, 1:] == q[i - 2])            # a[i-1] == b[j-2] and a[i-2] == b[j-1]
                t = np.where(tr, prev2[:, :-2] + 1, np.int16(1 << 14))
                np.minimum(sub[:, 1:], t, out=sub[:, 1:])
            cur[:, 1:] = sub
            cur = np.minimum.accumulate(cur - ar, axis=1) + ar                   # the insertions: D[i][j] <= D[i][j-1] + 1
            prev2, prev = prev, cur
        m = np.minimum(self.lens[rows], W)
        d = prev[np.arange(R), m].astype(np.int64)
        keep = d <= e
        return rows[keep], d[keep]


def tokens(query):
    """[(start, end, lower-cased token)] of the alnum runs of a query (bytes)"""
    out, i = [], 0
    while i < len(query):
        while i < len(query) and query[i] not in suggest_ref._ALNUM:
            i += 1
        a = i
        while i < len(query) and query[i] in suggest_ref._ALNUM:
            i += 1
        if i > a:
            out.append((a, i, query[a:i].lower()))
    return out


def did_you_mean(table, known_terms, query, limit):
    """The JSON bytes of Engine::did_you_mean over `table` (a Table); known_terms: the raw lexicon terms (a set of bytes)"""
    L = suggest_ref.clamp_limit(limit)
    terms, corrected, at, changed = [], b"", 0, False
    for a, b, tok in tokens(query):
        if len(tok) < 2 or tok in STOPWORDS:
            continue
        known = tok in known_terms
        sugg = [] if known else table.fuzzy(tok, auto_edits(len(tok)), 0, L)
        if sugg:
            corrected += query[at:a] + table.terms[sugg[0][0]]
            at, changed = b, True
        terms.append({"known": known, "token": tok.decode("latin-1"),
                      "suggestions": [{"distance": d, "score": int(table.scores[i]), "term": table.terms[i].decode("latin-1")} for i, d in sugg]})
    corrected += query[at:]
    doc = {"changed": changed, "corrected": corrected.decode("latin-1"), "query": query.decode("latin-1"), "terms": terms}
    return json.dumps(doc, indent=2, sort_keys=True, ensure_ascii=False).encode("latin-1")
