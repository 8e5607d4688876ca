"""Numpy restatement of ns_segment_union's rule, independent of the kernels and of csrc/ns_union_plan.hpp.

flat: the source's payload as (n, 2) uint32 {docId, tf}.  Member i is flat[member_off[i] / 8 : + member_cnt[i]]; group g names
the members [group_begin[g], group_begin[g + 1]).
  one member          the list as it stands, a docId >= n_docs included
  two or more         np.add.at of the tf into a dense uint32 table over the docIds < n_docs (the sum wraps), then nonzero:
                      docId-ascending {doc, sum}
  none, or all empty  no posting"""
import numpy as np


def union(flat, member_off, member_cnt, group_begin, n_docs):
    """-> per group (docIds uint32, tfs uint32)"""
    flat = np.asarray(flat, dtype=np.uint32).reshape(-1, 2)
    out = []
    for g in range(len(group_begin) - 1):
        b, e = int(group_begin[g]), int(group_begin[g + 1])
        parts = [flat[int(member_off[i]) // 8: int(member_off[i]) // 8 + int(member_cnt[i])] for i in range(b, e)]
        if e - b == 1:
            out.append((parts[0][:, 0].copy(), parts[0][:, 1].copy()))
            continue
        table = np.zeros(int(n_docs), dtype=np.uint32)
        for p in parts:
            inside = p[p[:, 0] < n_docs]
            np.add.at(table, inside[:, 0].astype(np.int64), inside[:, 1])      # uint32: wraps
        docs = np.flatnonzero(table).astype(np.uint32)
        out.append((docs, table[docs].copy()))
    return out


def bound(member_cnt, group_begin, n_docs):
    """the capacity of the new payload in postings: the single groups' counts plus, per group of two or more members,
    min(sum of member counts, n_docs)"""
    total = 0
    for g in range(len(group_begin) - 1):
        b, e = int(group_begin[g]), int(group_begin[g + 1])
        s = sum(int(c) for c in member_cnt[b:e])
        total += s if e - b == 1 else min(s, int(n_docs))
    return total


def rounds(member_cnt, group_begin, n_docs, scratch):
    """rounds of table scratch: groups of two or more members with a posting, max(1, scratch // (4 * n_docs)) a round"""
    tabled = sum(1 for g in range(len(group_begin) - 1)
                 if group_begin[g + 1] - group_begin[g] >= 2 and sum(int(c) for c in member_cnt[group_begin[g]:group_begin[g + 1]]) > 0)
    per = max(int(scratch) // (4 * max(int(n_docs), 1)), 1)
    return (tabled + per - 1) // per


def lists_of(payload, byte_off, counts):
    """the lists of a payload as the returned offsets name them -> [(docIds, tfs)]"""
    payload = np.asarray(payload, dtype=np.uint32).reshape(-1, 2)
    return [(payload[int(o) // 8: int(o) // 8 + int(c), 0].copy(), payload[int(o) // 8: int(o) // 8 + int(c), 1].copy()) for o, c in zip(byte_off, counts)]


def check_layout(byte_off, counts, n_postings):
    """lists start at multiples of 8, lie inside the payload and do not overlap"""
    spans = sorted((int(o), int(o) + 8 * int(c)) for o, c in zip(byte_off, counts) if int(c))
    for o, _ in spans:
        assert o % 8 == 0
    for (a0, a1), (b0, _) in zip(spans, spans[1:]):
        assert a1 <= b0, ("lists overlap", a0, a1, b0)
    assert not spans or spans[-1][1] <= 8 * int(n_postings)
