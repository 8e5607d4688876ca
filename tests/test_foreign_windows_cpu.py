"""CPU tests of the driver-stream body's foreign-window rule (ns_internal.h foreign_slack / foreign_scale / foreign_window)
through tests/window_harness.cpp, which compiles the very lines the kernel compiles.  For FB = 64 (thin class) and FB = 192
(general class), every slack constant of the sweep and the reciprocal moved by -2 .. +2 ulp (the device takes it with
v_rcp_f32, 1 ulp):

  budget     the windows sum to at most FB (the flat arrays of a super-batch hold FB postings)
  bounds     1 <= w_t <= rem_t wherever rem_t > 0, and w_t == 0 where rem_t == 0
  whole      when everything left fits (Rf + nact <= FB) every window is the whole rest of its list: the directed families
             of tests/body_shapes.py pin their single super-batch on this
  fall-back  whenever reduction (a) Rf + nact <= FB or (b) FB - c * nact < FB / 2 applies, the windows are those of the rule
             without slack, which the harness writes out on its own

over random rem vectors of 1 .. 63 active terms, every small vector of up to three terms, lists shorter than c, totals of
FB - 1, FB and FB + 1 (Rf + nact), and one list of 2^31 postings next to tiny ones."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsearch-api_amd", "csrc")
FBS = (64, 192)
CS = (1, 2, 3, 4, 6)
NUDGES = (-2, -1, 0, 1, 2)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("win") / "window_harness.so")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(rocm, "include"), "-I" + CSRC, "-o", so, os.path.join(ROOT, "tests", "window_harness.cpp")], check=True)
    lib = C.CDLL(so)
    vp, u32 = C.c_void_p, C.c_uint32
    lib.plan_windows_batch.argtypes = [vp, u32, u32, u32, u32, C.c_int, vp, vp, vp]
    lib.plan_windows_batch.restype = None
    lib.slack_constants.argtypes = [vp]
    lib.slack_constants.restype = None
    return lib


def plan(lib, rem, c, fb, nudge):
    rem = np.ascontiguousarray(rem, dtype=np.uint32)
    m, n = rem.shape
    w, w0, info = np.zeros((m, n), np.uint32), np.zeros((m, n), np.uint32), np.zeros((m, 3), np.uint32)
    lib.plan_windows_batch(rem.ctypes.data, m, n, c, fb, nudge, w.ctypes.data, w0.ctypes.data, info.ctypes.data)
    return w, w0, info


def check(lib, rem, label):
    """every property, for every FB, c and nudge; -> the slack in effect per (FB, c) at nudge 0, for the callers that pin it"""
    rem = np.ascontiguousarray(rem, dtype=np.uint32)
    assert rem.shape[1] <= 63
    rem64 = rem.astype(np.int64)
    nact, total = (rem64 > 0).sum(axis=1), rem64.sum(axis=1)
    assert total.max() < 2 ** 32, "the kernel's Rf saturates at 2^32 - 1: upload rejects such segments"
    eff = {}
    for fb, c, nudge in itertools.product(FBS, CS, NUDGES):
        w, w0, info = plan(lib, rem, c, fb, nudge)
        what = (label, "FB", fb, "c", c, "nudge", nudge)
        w64 = w.astype(np.int64)
        assert np.array_equal(info[:, 0], nact) and np.array_equal(info[:, 1], total), what
        assert (w64.sum(axis=1) <= fb).all(), what + ("budget", rem[np.argmax(w64.sum(axis=1))].tolist())
        assert (w64[rem64 == 0] == 0).all() and (w64[rem64 > 0] >= 1).all() and (w64 <= rem64).all(), what + ("bounds",)
        fits = total + nact <= fb                                  # reduction (a)
        many = fb - c * nact < fb // 2                             # reduction (b)
        assert np.array_equal(w[fits], rem[fits]), what + ("whole",)
        want_c = np.where(fits | many, 1, c)
        assert np.array_equal(info[:, 2], want_c), what + ("slack in effect",)
        red = fits | many
        assert np.array_equal(w[red], w0[red]), what + ("fall-back",)
        if c == 1:
            assert np.array_equal(w, w0), what + ("c = 1 is the rule without slack",)
        else:
            full = ~red                                             # slack in effect: a list shorter than c is taken whole
            short = full[:, None] & (rem64 > 0) & (rem64 <= c)
            assert np.array_equal(w[short], rem[short]), what + ("lists no longer than c",)
            assert (w64[full[:, None] & (rem64 > c)] >= c).all(), what + ("at least c postings",)
        if nudge == 0:
            eff[fb, c] = info[:, 2].copy()
    return eff


def test_the_shipped_constants_are_in_the_swept_set(harness):
    out = np.zeros(2, np.uint32)
    harness.slack_constants(out.ctypes.data)
    assert int(out[0]) in CS and int(out[1]) in CS


def test_random_vectors_of_1_to_63_active_terms(harness):
    rng = np.random.default_rng(7)
    rows = []
    for n in range(1, 64):
        for scale in (1, 3, 30, 400, 20000, 3_000_000):
            for _ in range(6):
                r = np.zeros(63, np.int64)
                r[rng.permutation(63)[:n]] = 1 + rng.integers(0, scale, size=n)
                rows.append(r)
    # the df law of the generator: one hot list, a few tails
    for _ in range(500):
        n = int(rng.integers(1, 7))
        r = np.zeros(63, np.int64)
        r[:n] = (600000.0 / rng.integers(1, 65536, size=n)).astype(np.int64) + 1
        rows.append(r)
    check(harness, np.array(rows), "random")


def test_every_small_vector_of_up_to_three_terms(harness):
    vals = list(range(0, 9)) + [61, 62, 63, 64, 65, 95, 96, 97, 187, 188, 189, 190, 191, 192, 193, 1000]
    rows = [(a, b, c) for a in vals for b in vals for c in vals]
    check(harness, np.array(rows), "exhaustive")


def test_lists_shorter_than_the_slack(harness):
    rows = []
    for big in (500, 5000, 50000):
        for tails in itertools.product((1, 2, 3, 5), repeat=3):
            rows.append((big,) + tails)
            rows.append(tails + (big,))
    check(harness, np.array(rows), "short lists")


@pytest.mark.parametrize("fb", FBS)
def test_totals_around_the_whole_list_boundary(harness, fb):
    """Rf + nact == FB - 1, FB (everything fits: whole lists, one super-batch) and FB + 1 (the first total at which the
    proportional rule, with or without slack, decides)"""
    rng = np.random.default_rng(fb)
    rows, want_fit = [], []
    for nact in (1, 2, 3, 4, 7, 16, 31):
        for off in (-1, 0, 1):
            total = fb + off - nact
            for _ in range(20):
                cuts = np.sort(rng.choice(np.arange(1, total), nact - 1, replace=False)) if nact > 1 else np.zeros(0, np.int64)
                r = np.zeros(63, np.int64)
                r[:nact] = np.diff(np.concatenate([[0], cuts, [total]]))
                assert r.sum() == total and (r[:nact] > 0).all()
                rows.append(r)
                want_fit.append(off <= 0)
    rem = np.array(rows)
    eff = check(harness, rem, "boundary")
    fit = np.array(want_fit)
    for c in CS:
        assert (eff[fb, c][fit] == 1).all()
        w, _, _ = plan(harness, rem, c, fb, 0)
        assert np.array_equal(w[fit], rem[fit].astype(np.uint32))


def test_one_huge_list_next_to_tiny_ones(harness):
    rows = []
    for tails in ((1,), (1, 1), (2, 9), (1, 2, 3, 4), (25, 60, 120), tuple([1] * 20), tuple([3] * 40), tuple([1] * 62)):
        for huge in (2 ** 31, 2 ** 31 - 1, 2 ** 31 + 12345):
            r = np.zeros(63, np.int64)
            r[0] = huge
            r[1:1 + len(tails)] = tails
            rows.append(r)
            rows.append(np.roll(r, 5))
    check(harness, np.array(rows), "huge")


def test_many_foreign_terms_fall_back_to_no_slack(harness):
    """40 terms of 30 postings: c = 3 would take 120 of the 192 postings (more than half), c = 2 takes 80 and stays; 63 terms
    fall back at every c > 1 in both classes"""
    r40 = np.zeros((1, 63), np.int64)
    r40[0, :40] = 30
    r63 = np.full((1, 63), 30, np.int64)
    e40, e63 = check(harness, r40, "40 terms"), check(harness, r63, "63 terms")
    assert [int(e40[192, c][0]) for c in CS] == [1, 2, 1, 1, 1]
    assert all(int(e40[64, c][0]) == 1 for c in CS)
    assert all(int(e63[fb, c][0]) == 1 for fb in FBS for c in CS)
