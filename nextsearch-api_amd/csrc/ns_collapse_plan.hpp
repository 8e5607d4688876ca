// One hit per group: what ns_search_collapsed adds to a ranked call's plan (ns_call_plan.hpp), and the look-up
// its count kernel shares with the host.  Host code only, like ns_call_plan.hpp: no HIP type and no runtime call;
// tests/collapse_host_check.cpp compiles it with g++ for the CPU suite.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ns_boolean_plan.hpp"
#include "ns_call_plan.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NS_CL_HD __host__ __device__
#else
#define NS_CL_HD
#endif

namespace ns {

// First index of sorted[0 .. n) (ascending by .x) whose .x is not below g; n when there is none.  k_cl_count looks a matched
// document's group up among the query's hit groups with it.
template <class Pair>
NS_CL_HD inline uint32_t cl_lower_bound(const Pair* sorted, uint32_t n, uint32_t g) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (sorted[mid].x < g) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// What the collapsed call adds to a RankedPlan's block: the groups and others rows next to the hits, one more timed stage per cut
// when others are asked for, and the dynamic LDS of the count kernel (the quorum planes over a whole tile, as k_bs_count's).
struct CollapsePlan {
    bool count = false;          // others_out != NULL: k_cl_count runs after each cut's join
    uint32_t stages = 2;         // timed stages per cut: select, join (, count)
    size_t out_slots = 0;        // n_queries x K: hits, groups and others have one entry per slot
    size_t count_lds = 0;        // bytes of dynamic LDS of a k_cl_count launch
};

// `planes`: the counter planes of the call's largest need (bq_need_planes).  False, with `err` set, for a plan the collapsed
// call cannot run: one with cursors, or more planes than a need can ask for.
inline bool collapse_plan(const RankedPlan& plan, uint32_t n_queries, bool want_others, uint32_t planes, CollapsePlan& out, std::string& err) {
    out = CollapsePlan();
    if (plan.K < 1 || plan.K > kSdRowSlots) { err = fc_format("K = %u outside [1, %u]", plan.K, kSdRowSlots); return false; }
    if (plan.paged) { err = "a collapsed call has no cursor"; return false; }
    if (planes > 3u) { err = fc_format("%u counter planes; at most 3", planes); return false; }
    out.count = want_others;
    out.stages = want_others ? 3u : 2u;
    out.out_slots = (size_t)n_queries * plan.K;
    out.count_lds = want_others ? (size_t)planes * (kFcTileDocs / 8u) : 0;
    return true;
}

// others[] as k_bq_join_collapsed initialises it for a slot of a query (it calls this), and what k_cl_count's atomic adds make of
// it: the fused subtraction (0xFFFFFFFF + n wraps to n - 1).
NS_CL_HD inline uint32_t cl_others_seed(uint32_t group, bool have) { return (have && group != 0u) ? 0xFFFFFFFFu : 0u; }
inline uint32_t cl_others_value(uint32_t seed, uint32_t matched_of_group) { return seed + matched_of_group; }

}  // namespace ns
