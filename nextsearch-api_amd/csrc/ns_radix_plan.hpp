// The digit plan of the LSD radix sort in csrc/ns_invert.hip, for index inversion (invert_run) and for the sorts of text ingest
// and compaction (ig_sort): a pure function of the key range.  Host code only, like ns_call_plan.hpp: no HIP type and no
// runtime call; tests/radix_plan_harness.cpp compiles it with g++ for the CPU suite.
#pragma once
#include <algorithm>
#include <cstdint>

namespace ns {

struct RadixPlan {
    int bits = 1;                   // the width of key_range - 1, at least 1
    int passes = 1;                 // ceil(bits / 11), 1 .. 3
    int pbits[3] = {8, 8, 8};       // the digit of pass p, lowest first: 8 .. 11 bits each, as even as possible
};

// The keys are the values below key_range (nothing else takes part in the sort), so the plan follows from key_range alone:
// no device -> host sync decides it.  The passes' digits cover `bits`; a digit is never narrower than 8 bits, the narrowest
// k_iv_hist_w / k_iv_pass instantiation.
inline RadixPlan radix_plan(uint32_t key_range) {
    RadixPlan r;
    while (r.bits < 32 && key_range > 1 && ((key_range - 1) >> r.bits) != 0) r.bits++;
    r.passes = std::max(1, (r.bits + 10) / 11);
    int left = r.bits;
    for (int p = 0; p < r.passes; p++) {
        const int share = (left + (r.passes - p) - 1) / (r.passes - p);
        r.pbits[p] = std::min(11, std::max(8, share));
        left = std::max(0, left - r.pbits[p]);
    }
    return r;
}

}  // namespace ns
