"""Numpy / Python restatement of per-document boost factors in ranked boolean search, independent of the kernels,
of the planner and of host/boost.hpp.

The device side.  The matched set and every document's score are the quorum sibling's (quorum_ref.quorum_all).  A boosted score
is ONE np.float32 multiply of that finished score with the document's factor; its bits are the rank.  The total order is
(ord(bits) descending, position of the segment in the call's list, docId), after_ref's rows, cut by a cursor as after_ref.page
cuts them.  -0.0f (a negative score times 0.0f) has the bits 0x80000000 and so sorts just below +0.0f.

The host side.  The decay rule in float64: per document a civil day number from its date key (a missing month or day reads as
1), age = max(0, |days(origin) - days(key)| - offset_days), f = 2^(-age / scale_days) (exponential) or max(0, 1 - age /
scale_days) (linear), the factor (1 - weight) + weight * f rounded once to fp32; an undated document's f is `undated`."""
import math

import numpy as np

import after_ref

CUSTOM, EXPONENTIAL, LINEAR = 0, 1, 2


def product_bits(score, factor):
    """bits of fp32(score * factor): one rounded multiply"""
    with np.errstate(over="ignore", under="ignore"):
        return int((np.float32(score) * np.float32(factor)).view(np.uint32))


def boosted_rows(everything, boosts, seg_order):
    """everything: quorum_ref.quorum_all's (or grouped_ref.grouped_all's) answer, per query [(score fp32, segment, doc)];
    boosts: per segment one float32 factor per document -> per query the whole matched set in boosted order as after_ref rows
    (mapped rank, position, doc, segment, product bits)"""
    order = list(seg_order)
    out = []
    for rows in everything:
        q = []
        for v, s, d in rows:
            bits = product_bits(v, boosts[s][int(d)])
            q.append((after_ref.ord32(bits), order.index(s), int(d), s, bits))
        q.sort(key=lambda r: after_ref.position(*r[:3]))
        out.append(q)
    return out


# ---- the decay rule ---------------------------------------------------------------------------------------------------
def civil_days(y, m, d):
    """days since 1970-01-01 of the proleptic Gregorian date (the well-known era / day-of-era arithmetic)"""
    y -= m <= 2
    era = (y if y >= 0 else y - 399) // 400
    yoe = y - era * 400
    doy = (153 * (m + (-3 if m > 2 else 9)) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


def days_of_key(key):
    """a date key Y * 10000 + M * 100 + D (missing parts 0, read as 1) -> its day number; key 0 is undated: None"""
    key = int(key)
    if key == 0:
        return None
    return civil_days(key // 10000, max(key // 100 % 100, 1), max(key % 100, 1))


def decay_table(keys, kind, weight, origin_key, scale_days, offset_days, undated):
    """keys: the date keys of the documents; origin_key: a date key, or 0 for the newest dated document (largest day number) of
    `keys` -> (float32 factors, the float64 values before the rounding)"""
    days = [days_of_key(k) for k in keys]
    if origin_key:
        origin = days_of_key(origin_key)
    else:
        dated = [d for d in days if d is not None]
        origin = max(dated) if dated else 0
    exact = np.empty(len(days), dtype=np.float64)
    for i, d in enumerate(days):
        if d is None:
            f = float(undated)
        else:
            age = max(0.0, abs(float(origin - d)) - float(offset_days))
            f = math.pow(2.0, -age / float(scale_days)) if kind == EXPONENTIAL else max(0.0, 1.0 - age / float(scale_days))
        exact[i] = (1.0 - float(weight)) + float(weight) * f
    return exact.astype(np.float32), exact


def ulps_apart(a, b):
    """distance in fp32 ulps of two arrays of non-negative finite float32"""
    return np.abs(np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64) - np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64))
