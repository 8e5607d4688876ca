// CPU harness of the driver-stream body's foreign-window rule (nextsearch-api_amd/csrc/ns_internal.h foreign_slack /
// foreign_scale / foreign_window) for tests/test_foreign_windows_cpu.py: one plan over the `rem` vector of a wave, the way
// NS_PLAN_FOREIGN of ns_driver_kernel.hip strings the three functions together.  Built by the test with the host compiler;
// not part of the product.
#include <hip/hip_runtime.h>
#include <math.h>

#include "ns_internal.h"

using namespace ns;

// the reciprocal the device takes with v_rcp_f32 (1 ulp): 1 / x rounded to fp32, moved by `nudge` ulps
static float rcp_nudged(float x, int nudge) {
    float r = 1.0f / x;
    for (int i = 0; i < nudge; i++) r = nextafterf(r, INFINITY);
    for (int i = 0; i > nudge; i--) r = nextafterf(r, 0.0f);
    return r;
}

static void totals(const uint32_t* rem, uint32_t n, uint32_t* nact, uint32_t* Rf) {
    uint32_t a = 0, s = 0;
    for (uint32_t t = 0; t < n; t++) {
        a += rem[t] > 0;
        s = (s + rem[t] < s) ? 0xFFFFFFFFu : (s + rem[t]);   // saturating, as the kernel's Rf
    }
    *nact = a; *Rf = s;
}

// rem[0 .. n): postings left per lane (0: the driver's lane, an exhausted list).  w[t] = 0 where rem[t] == 0, as the kernel's w_n.
// info: {nact, Rf, slack in effect}
extern "C" void plan_windows(const uint32_t* rem, uint32_t n, uint32_t c, uint32_t FB, int nudge, uint32_t* w, uint32_t* info) {
    uint32_t nact, Rf;
    totals(rem, n, &nact, &Rf);
    const uint32_t ce = foreign_slack(c, FB, nact, Rf);
    const float scale = foreign_scale(ce, FB, nact, rcp_nudged((float)(Rf > 1u ? Rf : 1u), nudge));
    for (uint32_t t = 0; t < n; t++) w[t] = rem[t] > 0 ? foreign_window(rem[t], ce, scale) : 0u;
    info[0] = nact; info[1] = Rf; info[2] = ce;
}

// the rule before slack existed, written out as the kernel had it: w = min(rem, 1 + floor(rem * (FB - nact) / Rf))
extern "C" void plan_windows_without_slack(const uint32_t* rem, uint32_t n, uint32_t FB, int nudge, uint32_t* w) {
    uint32_t nact, Rf;
    totals(rem, n, &nact, &Rf);
    const float scale = (float)((int)FB - (int)nact) * rcp_nudged((float)(Rf > 1u ? Rf : 1u), nudge);
    for (uint32_t t = 0; t < n; t++) {
        uint32_t x = 1u + (uint32_t)((float)rem[t] * scale);
        x = (x < rem[t]) ? x : rem[t];
        w[t] = rem[t] > 0 ? x : 0u;
    }
}

// m plans at once: rem, w and w0 (without slack) are m x n row-major, info m x 3
extern "C" void plan_windows_batch(const uint32_t* rem, uint32_t m, uint32_t n, uint32_t c, uint32_t FB, int nudge, uint32_t* w,
                                   uint32_t* w0, uint32_t* info) {
    for (uint32_t i = 0; i < m; i++) {
        plan_windows(rem + (size_t)i * n, n, c, FB, nudge, w + (size_t)i * n, info + (size_t)i * 3);
        plan_windows_without_slack(rem + (size_t)i * n, n, FB, nudge, w0 + (size_t)i * n);
    }
}

extern "C" void slack_constants(uint32_t* out) { out[0] = kWinSlackThin; out[1] = kWinSlackGen; }
