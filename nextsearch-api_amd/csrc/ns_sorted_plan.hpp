// Search sorted by a per-document key: what ns_search_sorted adds to the facet planner (ns_facet_plan.hpp cuts
// the work items).  Per query the range of its items, and the cut of a batch into sub-batches whose candidate rows
// (items x K x 8 B) fit a fixed buffer.  Host code only, like ns_facet_plan.hpp: no HIP runtime call and no device pointer;
// tests/sorted_plan_harness.cpp compiles it with g++ for the CPU suite.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "ns_facet_plan.hpp"

namespace ns {

// sort direction, or-ed into ns_search_sorted's flags (NS_SORT_DESC / NS_SORT_ASC of nextsearch_hip.h)
static constexpr uint32_t kSdAscFlag = 0x1000u;
// The candidate buffer never exceeds this many bytes: 64 MiB = 83 886 items at K = 100, 8 Mi items at K = 1.
static constexpr uint64_t kSdCandBytes = 64ull << 20;
// A row of the candidate buffer has K slots; k_sd_join numbers a query's candidates item * kSdRowSlots + slot.
static constexpr uint32_t kSdRowSlots = 128;

// Queries [q_begin, q_end) and their items [item_begin, item_end) of one launch of the three kernels.
struct SdBatch {
    uint32_t q_begin, q_end;
    uint32_t item_begin, item_end;
};

// q_off[q] .. q_off[q + 1]: the items of query q.  fc_plan emits items query by query, so the range is contiguous and in
// plan order (segment position, then tile).  False when the items are not grouped like that.
inline bool sd_query_items(const std::vector<FcItem>& items, uint32_t n_queries, std::vector<uint32_t>& q_off) {
    q_off.assign((size_t)n_queries + 1, 0u);
    uint32_t q = 0;
    for (size_t i = 0; i < items.size(); i++) {
        const uint32_t iq = items[i].query;
        if (iq >= n_queries || iq < q) return false;
        while (q < iq) q_off[++q] = (uint32_t)i;
    }
    while (q < n_queries) q_off[++q] = (uint32_t)items.size();
    return true;
}

// Cuts the queries into sub-batches, greedily and in order: a sub-batch takes queries while its items' rows
// (items x K x 8 B) still fit cand_bytes.  Every query lands in exactly one sub-batch (queries without items too).  A
// single query whose rows alone exceed the bound is REFUSED (NS_E_INVAL, err set, nothing usable in `out`): its index
// would have to hold more than cand_bytes / (8 K) tiles, 10^10 documents at the product's tile and K = 100.
inline int sd_cut(const std::vector<uint32_t>& q_off, uint32_t n_queries, uint32_t K, uint64_t cand_bytes, std::vector<SdBatch>& out,
                  std::string& err) {
    out.clear();
    if (K < 1 || K > kSdRowSlots) { err = fc_format("K = %u outside [1, %u]", K, kSdRowSlots); return NS_E_INVAL; }
    const uint64_t max_items = cand_bytes / (8ull * K);
    uint32_t q0 = 0;
    for (uint32_t q = 0; q < n_queries; q++) {
        const uint64_t own = q_off[q + 1] - q_off[q];
        if (own > max_items) {
            out.clear();
            err = fc_format("query %u alone has %llu work items; the candidate buffer of %llu bytes holds %llu rows at K = %u", q,
                            (unsigned long long)own, (unsigned long long)cand_bytes, (unsigned long long)max_items, K);
            return NS_E_INVAL;
        }
        if ((uint64_t)q_off[q + 1] - q_off[q0] > max_items) {
            out.push_back(SdBatch{q0, q, q_off[q0], q_off[q]});
            q0 = q;
        }
    }
    if (n_queries) out.push_back(SdBatch{q0, n_queries, q_off[q0], q_off[n_queries]});
    return NS_OK;
}

}  // namespace ns
