"""Typo-tolerant completion restated for the tests: the prefix distance pd(q, c) = min over 0 <= j <= |c| of
osa(q, c[:j]), the candidates, the fixed prefix, the ranking and the complete JSON.  Two versions of the search, neither with
a filter of the device's (no signature, no early exit), both on correct_ref's optimal string alignment, which is not
written again here:

  plain   osa(q, c[:j]) for every j, on every eligible entry
  numpy   for every j of the band n - e .. n + e (osa(q, c[:j]) >= |n - j|, so no other j can be within e): the DISTINCT
          strings c[:j] of the table as a correct_ref.Table of their own, whose within() is the D[n][j] of all of them
          in one numpy pass; an entry's distance is the minimum over the band's columns.  (correct_ref.Table.within is
          checked against correct_ref.osa by tests/test_correct_cpu.py, and the two versions here against each other
          by tests/test_complete_cpu.py.)

Test infrastructure only."""
import functools
import json

import numpy as np

import correct_ref
import suggest_ref

MAX_LEN = correct_ref.MAX_LEN
MAX_EDITS = correct_ref.MAX_EDITS
_FAR = 1 << 20


@functools.lru_cache(maxsize=1 << 18)
def pd(q, c):
    """the prefix distance (unbounded; remembered per pair).  osa(q, c[:j]) >= j - |q|, which from j = 2 |q| on is no less than
    osa(q, b"") = |q|"""
    return min(correct_ref.osa(q, c[:j]) for j in range(min(len(c), 2 * len(q)) + 1))


def complete_plain(terms, scores, query, max_edits, prefix_len, L):
    """-> [(index, distance)] best first; L already clamped"""
    if not query or len(query) > MAX_LEN:
        return []
    p = query[:min(prefix_len, len(query))]
    cand = correct_ref.candidates(terms, scores)
    hits = []
    for i, t in enumerate(terms):
        if not cand[i] or len(t) < len(query) - max_edits or not t.startswith(p):
            continue
        d = pd(query, t)
        if d <= max_edits:
            hits.append((d, -int(scores[i]), i))
    hits.sort()
    return [(i, d) for d, _, i in hits[:L]]


def sig(t):
    """the device's byte-class set (bits 0..35 = [0-9a-z], bit 36 = any other byte): for the tests that must contain an
    answer ON the bound of the signature filter, never used by the restatement itself"""
    s = 0
    for c in t:
        s |= 1 << (c - 48) if 48 <= c <= 57 else 1 << (10 + c - 97) if 97 <= c <= 122 else 1 << 36
    return s


def sig_missing(q, c):
    """popcount(sig_q & ~sig_c); a candidate past 66 bytes has no signature on the device (None)"""
    return None if len(c) > MAX_LEN + MAX_EDITS else bin(sig(q) & ~sig(c)).count("1")


class Table:
    """The dictionary for the numpy version: correct_ref.Table (byte matrix, lengths, candidates) plus, per column j, the
    table of the distinct c[:j]."""

    def __init__(self, terms, scores):
        self.base = correct_ref.Table(terms, scores)
        self.terms = terms
        self.n = len(terms)
        self.scores = self.base.scores
        self._cuts = {}
        self._near = {}
        self._memo = {}

    def _cut(self, j):
        """-> (rows with at least j bytes, for each of them its row in the table of the distinct c[:j], that table, for each
        distinct c[:j] the row of c[:j - 1] in the table before it)"""
        if j not in self._cuts:
            rows = np.nonzero(self.base.lens >= j)[0]
            sub = inv = parent = None
            if len(rows):
                uniq, first, inv = np.unique(self.base.mat[rows, :j], axis=0, return_index=True, return_inverse=True)
                inv = np.asarray(inv).reshape(-1)
                sub = correct_ref.Table([u.tobytes() for u in uniq], [1] * len(uniq))
                if j > 1:
                    prows, pinv, _, _ = self._cut(j - 1)
                    parent = pinv[np.searchsorted(prows, rows[first])]
            self._cuts[j] = (rows, inv, sub, parent)
        return self._cuts[j]

    def distances(self, query, e):
        """-> (entries whose prefix distance is within e, those distances); candidates or not; remembered per query and e"""
        key = (query, e)
        if key in self._near:
            return self._near[key]
        n = len(query)
        out = np.full(self.n, _FAR, dtype=np.int64)
        for j in range(max(n - e, 0), n + e + 1):
            if j == 0:
                out[:] = correct_ref.osa(query, b"")          # every string has the empty prefix
                continue
            if j > self.base.width:
                break
            rows, inv, sub, parent = self._cut(j)
            if sub is None:
                break
            mask = None
            if j > 1 and sub.n >= 4 * self._cut(j - 1)[2].n:
                # Many distinct c[:j] per distinct c[:j - 1]: only the children of a c[:j - 1] within e + 1 get the DP.
                # Dropping the last byte of u costs at most one edit more (it was matched or substituted: delete its
                # partner instead; inserted: one edit fewer; transposed: match one of the pair and delete the other),
                # so osa(q, u) <= e needs osa(q, u[:-1]) <= e + 1.
                psub = self._cut(j - 1)[2]
                near = np.zeros(psub.n, dtype=bool)
                near[psub.within(query, e + 1, 0)[0]] = True
                mask = near[parent]
            keep = sub.cand
            if mask is not None:
                sub.cand = mask
            try:
                u, d = sub.within(query, e, 0)
            finally:
                sub.cand = keep
            du = np.full(sub.n, _FAR, dtype=np.int64)
            du[u] = d
            out[rows] = np.minimum(out[rows], du[inv])
        hit = np.nonzero(out <= e)[0]
        if len(self._near) >= 4096:
            self._near.clear()
        self._near[key] = (hit, out[hit])
        return self._near[key]

    def complete(self, query, max_edits, prefix_len, L):
        """-> [(index, distance)] best first; L already clamped (the best 10 are remembered per query, edits and prefix)"""
        key = (query, max_edits, min(prefix_len, len(query)))
        if key not in self._memo:
            self._memo[key] = self._top10(*key)
        return self._memo[key][:L]

    def within(self, query, e, p):
        """-> (indices, distances) of every candidate whose prefix distance is within e and that shares the query's first p bytes"""
        none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
        if not query or len(query) > MAX_LEN or self.n == 0:
            return none
        rows, d = self.distances(query, e)
        ok = self.base.cand[rows]
        if p:
            q = np.frombuffer(query, dtype=np.uint8)
            pw = min(p, self.base.width)
            ok &= (self.base.lens[rows] >= p) & (self.base.mat[rows, :pw] == q[:pw]).all(axis=1)
        return rows[ok], d[ok]

    def _top10(self, query, e, p):
        rows, d = self.within(query, e, p)
        order = np.lexsort((rows, -self.scores[rows], d))[:10]
        return [(int(rows[k]), int(d[k])) for k in order]


def complete_json(table, user_input, limit, max_edits=-1, prefix_len=1):
    """The JSON bytes of Engine::complete over `table` (a Table)"""
    L = suggest_ref.clamp_limit(limit)
    base, prefix = suggest_ref.split(user_input)
    e = correct_ref.auto_edits(len(prefix)) if max_edits < 0 else max_edits
    hits = table.complete(prefix, e, prefix_len, L)
    doc = {"limit": L, "query": user_input.decode("latin-1"),
           "suggestions": [{"distance": d, "score": int(table.scores[i]), "suggestion": (base + table.terms[i]).decode("latin-1"),
                            "term": table.terms[i].decode("latin-1")} for i, d in hits]}
    return json.dumps(doc, indent=2, sort_keys=True, ensure_ascii=False).encode("latin-1")
