// C entry points over csrc/ns_radix_plan.hpp for tests/test_radix_shapes_cpu.py (built by g++ inside the test; no HIP, no device).
// With -DRADIX_PLAN_MAIN it is a program of its own that walks the key ranges of the test and checks what every plan must
// satisfy, for a run under the host sanitizers.
#include <cstdint>
#include <cstdio>

#include "ns_radix_plan.hpp"

extern "C" {

// pbits_out: the digits of the three passes (8 for a pass not used); *bits_out: the width sorted.  Returns the number of passes.
uint32_t radix_plan_c(uint32_t key_range, uint32_t* pbits_out, uint32_t* bits_out) {
    const ns::RadixPlan r = ns::radix_plan(key_range);
    for (int p = 0; p < 3; p++) pbits_out[p] = (uint32_t)r.pbits[p];
    *bits_out = (uint32_t)r.bits;
    return (uint32_t)r.passes;
}

}  // extern "C"

#ifdef RADIX_PLAN_MAIN
static unsigned long long g_bad = 0, g_seen = 0;

static void check(uint32_t key_range) {
    const ns::RadixPlan r = ns::radix_plan(key_range);
    g_seen++;
    int width = 1;                                   // of key_range - 1, counted bit by bit
    for (uint64_t top = key_range > 1 ? (uint64_t)key_range - 1 : 0; top >> width; width++) {}
    bool ok = r.bits == width && r.passes >= 1 && r.passes <= 3 && (r.passes - 1) * 11 < width && width <= r.passes * 11;   // no more passes than 11-bit digits need
    int sum = 0;
    for (int p = 0; ok && p < r.passes; p++) { ok = r.pbits[p] >= 8 && r.pbits[p] <= 11; sum += r.pbits[p]; }
    for (int p = r.passes; ok && p < 3; p++) ok = r.pbits[p] == 8;
    ok = ok && sum >= width && (r.passes > 1 || sum <= width + 7);
    for (int p = 0; ok && p < r.passes; p++) ok = sum - r.pbits[p] < width;   // no pass to spare
    if (!ok) {
        std::printf("radix_plan_harness: WRONG: key_range %u: bits %d, %d passes of %d %d %d\n", key_range, r.bits, r.passes, r.pbits[0], r.pbits[1], r.pbits[2]);
        g_bad++;
    }
}

int main() {
    for (int k = 0; k <= 32; k++)
        for (int64_t v = (1ll << k) - 1; v <= (1ll << k) + 1; v++)
            check((uint32_t)(v < 1 ? 1 : v > 0xFFFFFFFEll ? 0xFFFFFFFEll : v));   // clipped to 1 .. 0xFFFFFFFE
    for (uint32_t v = 1; v <= 5000; v++) check(v);
    std::printf("radix_plan_harness: %llu ranges, %llu wrong\n", g_seen, g_bad);
    return g_bad ? 1 : 0;
}
#endif
