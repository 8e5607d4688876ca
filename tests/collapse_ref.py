"""Numpy / Python restatement of ns_search_collapsed, independent of the kernels and of the planner, and of
Engine::collapse_table's title and author rules (host/collapse.hpp).

The device side.  boost_ref.boosted_rows gives the sibling's whole matched set per query in its one total order (ord(bits of
fp32(score * factor)) descending, position of the segment in the call's list, docId).  Walking it front to back, a document
whose non-zero key an earlier document carried is deleted; key 0 stands alone.  The first K of what remains are the hits.
`others` of a hit is a plain count over the same rows: the documents with the hit's key, minus one; 0 for key 0."""
import re

K_MAX = 100


def collapse_rows(rows, keys):
    """rows: one query's after_ref rows (mapped rank, position, doc, segment, bits) in boosted order; keys: per segment (indexed
    by segment number, or a dict) one uint32 per document -> [(row, key, others)] of the collapsed ranking, whole"""
    count = {}
    for r in rows:
        g = int(keys[r[3]][r[2]])
        if g:
            count[g] = count.get(g, 0) + 1
    seen, out = set(), []
    for r in rows:
        g = int(keys[r[3]][r[2]])
        if g:
            if g in seen:
                continue
            seen.add(g)
        out.append((r, g, count[g] - 1 if g else 0))
    return out


def collapsed(all_rows, keys, k):
    """per query (hits [(segment, doc, bits)], groups, others, nhits, found) at K = clamp(k, 1, 100)"""
    K = min(max(int(k), 1), K_MAX)
    out = []
    for rows in all_rows:
        whole = collapse_rows(rows, keys)
        page = whole[:K]
        out.append(([(r[3], r[2], r[4]) for r, _, _ in page], [g for _, g, _ in page], [o for _, _, o in page], len(page), len(rows)))
    return out


def distinct_total(rows, keys):
    """distinct non-zero keys in the matched set + matched key-0 documents"""
    gs = [int(keys[r[3]][r[2]]) for r in rows]
    return len({g for g in gs if g}) + sum(1 for g in gs if not g)


def check(label, want, hits, groups, others, nhits, found, k):
    """one call's outputs against collapsed(): exact, the padded tail included (score -inf, seg and doc 0xFFFFFFFF, group 0,
    others 0); others may be None (the call skipped that pass)"""
    import numpy as np

    K = min(max(int(k), 1), K_MAX)
    for q, (w_hits, w_groups, w_others, w_n, w_found) in enumerate(want):
        what = (label, "k", k, "query", q)
        assert int(nhits[q]) == w_n, what + ("nhits", int(nhits[q]), w_n)
        assert int(found[q]) == w_found, what + ("found", int(found[q]), w_found)
        got = [(int(h["seg"]), int(h["doc"]), int(h["score"].view(np.uint32))) for h in hits[q, :w_n]]
        assert got == w_hits, what + ("hits", got[:8], w_hits[:8])
        assert [int(g) for g in groups[q, :w_n]] == w_groups, what + ("groups",)
        if others is not None:
            assert [int(o) for o in others[q, :w_n]] == w_others, what + ("others", [int(o) for o in others[q, :w_n]][:8], w_others[:8])
            assert not np.any(others[q, w_n:K]), what + ("others tail",)
        tail = hits[q, w_n:K]
        assert np.all(tail["score"].view(np.uint32) == 0xFF800000) and np.all(tail["seg"] == 0xFFFFFFFF) and np.all(tail["doc"] == 0xFFFFFFFF), what + ("tail",)
        assert not np.any(groups[q, w_n:K]), what + ("groups tail",)


# ---- collapse_table's rules ---------------------------------------------------------------------------------------------
def normalise(text):
    """lower-cased alphanumeric ASCII tokens joined by one space (the project's tokenizer splits on everything else)"""
    return " ".join(re.findall(r"[a-z0-9]+", text.lower()))


def dense_keys(fields_per_segment):
    """fields_per_segment: per segment, in manifest order, the documents' field texts -> per segment a list of uint32 keys: a dense
    id from 1 by first appearance of the normalised text, 0 for an empty one"""
    ids, out = {}, []
    for fields in fields_per_segment:
        keys = []
        for text in fields:
            n = normalise(text)
            if not n:
                keys.append(0)
                continue
            if n not in ids:
                ids[n] = len(ids) + 1
            keys.append(ids[n])
        out.append(keys)
    return out
