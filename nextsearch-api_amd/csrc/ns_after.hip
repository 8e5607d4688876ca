// SPDX-License-Identifier: MIT
// Pages past the first K: what k_sd_select<AND, true> (ns_sorted.hip) and k_bq_select<true> (ns_boolean.hip)
// share.  A launch with AFTER = true reads last[blockIdx.x] (ns_after_plan.hpp's after_last, planned on the host) once; in
// the sweep a key above it becomes 0 before it is offered to the kept set, with a select and no branch, so that all 64
// lanes still call the insert together and the threshold ballot skips chunks as before.  The keys that stay are counted per
// lane, reduced like the matched count and added to rest[query] with one integer atomic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ns_after_plan.hpp"

namespace ns {

#ifdef NS_COUNT
// Counting build only: events of the AFTER = true launches since the last reset (ns_debug_after_counters).  0 items with a
// bound other than ~0, 1 items whose bound falls inside their own tile, 2 items whose bound is 0, 3 keys the bound dropped,
// 4 keys that passed a bound other than ~0.
constexpr int kNsAcnt = 5;
__device__ unsigned long long g_ns_acnt[kNsAcnt];
#define NS_ACNT(i, v) do { if (threadIdx.x == 0) atomicAdd(&g_ns_acnt[(i)], (unsigned long long)(v)); } while (0)
#else
#define NS_ACNT(i, v)
#endif

// per item, once
__device__ __forceinline__ void af_count_item(uint64_t last) {
#ifdef NS_COUNT
    if (last != kAfterAll) {
        NS_ACNT(0, 1);
        if (after_in_tile(last)) NS_ACNT(1, 1);
        if (last == 0ull) NS_ACNT(2, 1);
    }
#else
    (void)last;
#endif
}

// key (0 = none) -> the key if it may enter, else 0; kept counts the keys that may
__device__ __forceinline__ uint64_t af_clip(uint64_t key, uint64_t last, uint32_t& kept) {
    const bool in = key != 0ull && key <= last;
    kept += in ? 1u : 0u;
#ifdef NS_COUNT
    if (last != kAfterAll && key != 0ull) atomicAdd(&g_ns_acnt[in ? 4 : 3], 1ull);
#endif
    return in ? key : 0ull;
}

}  // namespace ns
