// Pages past the first K: a cursor is a position (rank, segment, docId) in the total order of a ranked call
// (ns_search_boolean_after, ns_search_sorted_after); the call answers with the first K matched documents STRICTLY AFTER it.
// k_bq_select and k_sd_select keep the best keys of a work item, where a key is
//     (rank_mapped << 32) | ~(docId - doc_lo)        larger first, never 0
// so the cursor becomes, per item, the largest key that may still enter the kept set: after_last.  The bound is inclusive (an
// exclusive one would overflow at rank_mapped = 0xFFFFFFFF).  Host and device code, no HIP type and no runtime call, like
// ns_boolean_plan.hpp; tests/after_plan_harness.cpp compiles it with g++ for the CPU suite.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NS_AFTER_HD __host__ __device__
#else
#define NS_AFTER_HD
#endif

namespace ns {

// no cursor: every key may enter
static constexpr uint64_t kAfterAll = ~0ull;

// the order-preserving map of fp32 bits that k_bq_select ranks by (bq_ord): negative -> ~bits, else bits | 0x80000000
NS_AFTER_HD inline uint32_t after_ord(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
// the rank k_sd_select sorts by (sd_key): the key newest first, ~key oldest first, key 0 last in both directions
NS_AFTER_HD inline uint32_t after_sort_rank(uint32_t key, bool asc) { return asc ? (key ? ~key : 0u) : key; }

// The largest key of the item (segment position item_pos, documents [doc_lo, doc_hi), doc_hi - doc_lo <= 2^17) that comes
// strictly after the cursor (rank_mapped, cursor_pos, cursor_doc); 0 when none can.
//     item in an earlier segment, or in the cursor's with every document <= cursor_doc    strictly lower ranks only
//     item in a later segment, or in the cursor's with every document > cursor_doc        the cursor's rank and below
//     the tile that holds cursor_doc                                                      lower ranks, and ties with a larger docId
NS_AFTER_HD inline uint64_t after_last(uint32_t rank_mapped, uint32_t cursor_pos, uint32_t cursor_doc, uint32_t item_pos, uint32_t doc_lo,
                                       uint32_t doc_hi) {
    const uint64_t ties = ((uint64_t)rank_mapped << 32) | 0xFFFFFFFFull;
    const uint64_t below = rank_mapped ? (((uint64_t)(rank_mapped - 1u) << 32) | 0xFFFFFFFFull) : 0ull;
    if (item_pos < cursor_pos) return below;
    if (item_pos > cursor_pos) return ties;
    if (cursor_doc < doc_lo) return ties;
    if (cursor_doc >= doc_hi) return below;
    // the key of cursor_doc itself is (rank << 32) | ~(cursor_doc - doc_lo), its low word >= ~2^17: one below it never wraps
    return ((uint64_t)rank_mapped << 32) | (uint32_t)(~(cursor_doc - doc_lo) - 1u);
}

// what the counting build tells apart (ns_debug_after_counters)
NS_AFTER_HD inline bool after_in_tile(uint64_t last) { return last != 0ull && (uint32_t)last != 0xFFFFFFFFu; }

}  // namespace ns
