// What a ranked call (ns_search_sorted*, ns_search_boolean*, ns_search_grouped_after) plans between its
// planner's work items and its device block: the items of each query, the cut into sub-batches whose candidate rows fit the
// buffer (ns_sorted_plan.hpp), the cursors turned into one bound per item (ns_after_plan.hpp) and the sizes that follow.
// Host code only, like ns_sorted_plan.hpp: no HIP type and no runtime call; tests/call_plan_harness.cpp compiles it with g++
// for the CPU suite.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "ns_after_plan.hpp"
#include "ns_sorted_plan.hpp"

namespace ns {

// A launch grid holds fewer than 2^31 workgroups, and an item is one: every call that launches one kernel over its items
// (the facet counts) or cuts them first (the ranked calls) refuses more.
inline bool call_item_limit(uint64_t n_items, std::string& err) {
    if (n_items < (1ull << 31)) return true;
    err = fc_format("%llu work items; cut the batch", (unsigned long long)n_items);
    return false;
}

// Pages past the first K: the cursors of one call -> last[item].  rank_of maps a cursor's rank as the
// caller gives it to the rank the kernel's keys carry.  False, with `err` set, for a cursor the call refuses.  any_set: at
// least one query has a cursor (otherwise `last` stays empty and the AFTER = false kernels run).
template <class RankOf>
inline bool after_plan(const ns_cursor* after, uint32_t n_queries, const std::vector<FcSegView>& views, const std::vector<FcItem>& items,
                       RankOf rank_of, bool reserved_rank, std::vector<uint64_t>& last, bool& any_set, std::string& err) {
    last.clear();
    any_set = false;
    if (!after) return true;
    std::vector<uint32_t> pos_of(n_queries, 0u);
    for (uint32_t q = 0; q < n_queries; q++) {
        const ns_cursor& c = after[q];
        if (c.set > 1u) { err = fc_format("query %u: cursor with set = %u (0 or 1)", q, c.set); return false; }
        if (!c.set) continue;
        if (reserved_rank && c.rank == 0xFFFFFFFFu) { err = fc_format("query %u: cursor with the reserved key 0xFFFFFFFF", q); return false; }
        uint32_t pos = 0;
        while (pos < views.size() && views[pos].seg_id != c.seg_id) pos++;
        if (pos == views.size()) { err = fc_format("query %u: cursor names segment %u, which the call does not list", q, c.seg_id); return false; }
        pos_of[q] = pos;
        any_set = true;
    }
    if (!any_set) return true;
    last.resize(items.size());
    for (size_t i = 0; i < items.size(); i++) {
        const FcItem& it = items[i];
        const ns_cursor& c = after[it.query];
        last[i] = c.set ? after_last(rank_of(c.rank), pos_of[it.query], c.doc_id, it.seg, it.doc_lo, it.doc_hi) : kAfterAll;
    }
    return true;
}

struct RankedPlan {
    uint32_t K = 0;                 // k clamped to [1, NS_MAX_K]
    std::vector<uint32_t> q_off;    // n_queries + 1: the items of query q (sd_query_items)
    std::vector<SdBatch> cuts;      // one launch of the call's kernels each (sd_cut)
    std::vector<uint64_t> last;     // per item of the call; empty: no query has a cursor
    bool paged = false;             // some query has a cursor: the AFTER = true kernels run
    uint64_t cand_rows = 0;         // items of the largest cut: the candidate buffer is cand_rows x K x 8 B <= cand_bytes
};

// The checks fire in this order: the item limit, the grouping by query, the cut, the cursors.  False with `err` set (the
// caller puts its name in front), and nothing usable in `out`.  cand_bytes is kSdCandBytes in every call; the tests pass less.
template <class RankOf>
inline bool ranked_call_plan(const std::vector<FcItem>& items, uint32_t n_queries, uint32_t k, const ns_cursor* after,
                             const std::vector<FcSegView>& views, RankOf rank_of, bool reserved_rank, uint64_t cand_bytes, RankedPlan& out,
                             std::string& err) {
    out.K = std::min<uint32_t>(std::max<uint32_t>(k, 1u), NS_MAX_K);
    out.cand_rows = 0;
    if (!call_item_limit(items.size(), err)) return false;
    if (!sd_query_items(items, n_queries, out.q_off)) { err = "the work items are not grouped by query"; return false; }
    if (sd_cut(out.q_off, n_queries, out.K, cand_bytes, out.cuts, err) != NS_OK) return false;
    if (!after_plan(after, n_queries, views, items, rank_of, reserved_rank, out.last, out.paged, err)) return false;
    for (const SdBatch& c : out.cuts) out.cand_rows = std::max<uint64_t>(out.cand_rows, c.item_end - c.item_begin);
    return true;
}

// A call whose select kernel exists with AFTER = true alone (ns_search_boosted_after with tables): a plan without
// a cursor gets the bound that lets every key pass for each of its items, so that rest counts what found counts.
inline void ranked_plan_bound_all(size_t n_items, RankedPlan& plan) {
    if (plan.paged) return;
    plan.last.assign(n_items, kAfterAll);
    plan.paged = true;
}

}  // namespace ns
