"""Shapes for the foreign windows of the driver-stream body (ns_driver_kernel.hip NS_PLAN_FOREIGN; the rule is
ns_internal.h foreign_slack / foreign_window).  Plain data and constructors, no GPU use, in the form of tests/body_shapes.py:
a shape returns (n_docs, doc_len, lists, queries, idfs, weights) and carries the class every query's group must take.
tests/test_window_shapes_cpu.py plans them; tests/test_foreign_windows_gpu.py scores them against the numpy restatement and
counts their windows on the counting build (tests/foreign_reach.py).

n_docs = 2^17 throughout.  Lists are uniform random docIds, so that tools/dbg/window_sim.py's expectation applies; list 0 is
the driver (the longest list) and the queries put it first, in the middle and last.  Sizes against the thresholds restated in
body_shapes.plan_rule: thin when the other lists hold <= 1/32 of the driver, doc tiles from 0.25 postings per doc (32768)."""
import numpy as np

import body_shapes

N17 = 1 << 17
SHAPES = {}


def shape(cls):
    def deco(fn):
        fn.cls = cls
        SHAPES[fn.__name__] = fn
        return fn
    return deco


def _build(seed, sizes, orders):
    rng = np.random.default_rng(seed)
    lists = []
    for i, s in enumerate(sizes):
        d = np.sort(rng.choice(N17, s, replace=False)).astype(np.uint32)
        lists.append((d, rng.integers(1, 9, size=s, dtype=np.uint32)))
    idfs = [float(1.25 + 0.375 * (i % 23)) for i in range(len(sizes))]
    weights = [1.0 if i % 3 else 0.75 for i in range(len(sizes))]
    assert sizes[0] == max(sizes) and sizes.count(sizes[0]) == 1, "list 0 is the driver"
    return N17, rng.integers(20, 3000, size=N17, dtype=np.uint32), lists, [list(o) for o in orders], idfs, weights


@shape("general")
def general_tails():
    """driver 12000, primary foreign list 4000, tails of 120, 60, 25 and 9: ~22 super-batches whose end the tails decide"""
    return _build(61, [12000, 4000, 120, 60, 25, 9], [[0, 1, 2, 3, 4, 5], [2, 1, 0, 5, 3, 4], [5, 4, 3, 2, 1, 0]])


@shape("general")
def general_whole_list_boundary():
    """three foreign terms with 189 postings in all (Rf + nact == 192 == FB: whole lists, one super-batch, whatever the slack)
    and with 190 (one past: the proportional rule decides)"""
    return _build(62, [2000, 150, 30, 9, 10], [[0, 1, 2, 3], [1, 2, 3, 0], [0, 1, 2, 4], [1, 0, 4, 2]])


@shape("general")
def general_40_terms():
    """40 foreign terms of 30 postings: the 64-term instantiation; 3 * 40 postings of slack would be more than half of the
    192, so c >= 3 falls back to 1 (c = 2 does not)"""
    f = list(range(1, 41))
    return _build(63, [3000] + [30] * 40, [[0] + f, f[:20] + [0] + f[20:], f + [0]])


@shape("general")
def general_tiny_tails():
    """tails of 2, 1 and 1 postings, shorter than any slack above 1, next to a primary list of 4000"""
    return _build(64, [12000, 4000, 2, 1, 1], [[0, 1, 2, 3, 4], [2, 3, 1, 0, 4], [4, 3, 2, 1, 0]])


@shape("thin")
def thin_tails():
    """driver 40000, tails of 600, 300 and 200 (1100 * 32 <= 40000): ~25 super-batches of one 64-posting chunk"""
    return _build(65, [40000, 600, 300, 200], [[0, 1, 2, 3], [1, 0, 3, 2], [3, 2, 1, 0]])


@shape("thin")
def thin_20_single_postings():
    """20 one-posting tails: 21 terms (the 64-term instantiation), everything fits one super-batch"""
    f = list(range(1, 21))
    return _build(66, [5000] + [1] * 20, [[0] + f, f[:10] + [0] + f[10:], f + [0]])


COUNTED = ("general_tails", "thin_tails")     # the first shape of each class: counted by tests/foreign_reach.py
FB = body_shapes.FB
SPLIT = 1000     # ns_set_tuning split value at which every group of every shape is cut into two doc ranges or more
