// Facet counts: term refs -> (query, segment) groups -> work items of k_fc_count, one per doc-range tile.
// Host code only, like ns_plan.hpp: no HIP runtime call and no device pointer; tests/facet_plan_harness.cpp compiles it
// with g++ for the CPU suite.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "../../include/nextsearch_hip.h"

namespace ns {

// Documents per tile of the product build: the tile's matched set is a bitmap of kFcTileDocs / 8 = 16 KiB in LDS.
static constexpr uint32_t kFcTileDocs = 1u << 17;
static constexpr uint32_t kFcMaxBuckets = 1024;
// a test tile (variants and counting builds): a power of two, whole bitmap words, at most the product's
inline bool fc_tile_ok(uint32_t t) { return t >= 32 && t <= kFcTileDocs && (t & (t - 1)) == 0; }

// One posting list of a group, in the group's order.
struct FcRef {
    uint64_t first;   // index of the list's first posting in its segment's payload
    uint32_t count;
    uint32_t skip;    // 0: no skip table; else 1 + index of the list's first entry in the segment's skip tables
};
// Work item == one workgroup of k_fc_count: one (query, segment) group over the documents [doc_lo, doc_hi).
struct FcItem {
    uint32_t query;
    uint32_t seg;         // position in the call's segment list
    uint32_t ref_begin;   // into FcRef[]
    uint32_t ref_count;   // >= 1
    uint32_t doc_lo, doc_hi;
};
// What the cut knows of a listed segment.
struct FcSegView {
    uint32_t seg_id = 0, n_docs = 0;
    uint64_t n_postings = 0;
    std::function<uint32_t(uint32_t first, uint32_t count)> skip_of;   // may be empty: no tables
};

inline std::string fc_format(const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}

// Checks the descriptors and cuts the items.  Per query the refs are grouped by segment (in the order of the call's segment
// list, refs of a group in query order).  OR: a ref without postings is dropped, a group left without refs has no item.
// AND: a group with such a ref matches nothing and has no item.  Every other group gets one item per tile of
// [0, n_docs), the last one shorter.  Returns NS_OK, or NS_E_INVAL with `err` set and nothing usable in the outputs.
inline int fc_plan(const ns_query_desc* qd, uint32_t n_queries, const ns_term_ref* refs, uint32_t n_refs, bool and_mode,
                   const FcSegView* segs, uint32_t n_segs, uint32_t tile_docs, std::vector<FcRef>& out_refs,
                   std::vector<FcItem>& out_items, std::string& err) {
    out_refs.clear();
    out_items.clear();
    if (!fc_tile_ok(tile_docs)) { err = fc_format("facet tile of %u documents: not a power of two in [32, %u]", tile_docs, kFcTileDocs); return NS_E_INVAL; }
    std::vector<std::pair<uint32_t, uint32_t>> by_id(n_segs);   // (seg_id, position)
    for (uint32_t i = 0; i < n_segs; i++) by_id[i] = {segs[i].seg_id, i};
    std::sort(by_id.begin(), by_id.end());
    for (uint32_t i = 1; i < n_segs; i++)
        if (by_id[i].first == by_id[i - 1].first) { err = fc_format("seg_id %u is listed twice", by_id[i].first); return NS_E_INVAL; }
    auto slot_of = [&](uint32_t id) -> int64_t {
        auto it = std::lower_bound(by_id.begin(), by_id.end(), std::make_pair(id, 0u));
        return (it != by_id.end() && it->first == id) ? (int64_t)it->second : -1;
    };
    std::vector<std::pair<uint32_t, uint32_t>> order;   // (position of the segment, ref index) of one query
    for (uint32_t q = 0; q < n_queries; q++) {
        const uint64_t tb = qd[q].term_begin, tc = qd[q].term_count;
        if (tb + tc > n_refs) { err = fc_format("query %u: refs [%llu, %llu) run past the %u given", q, (unsigned long long)tb, (unsigned long long)(tb + tc), n_refs); return NS_E_INVAL; }
        order.clear();
        for (uint64_t r = tb; r < tb + tc; r++) {
            const ns_term_ref& t = refs[r];
            const int64_t slot = slot_of(t.seg_id);
            if (slot < 0) { err = fc_format("ref %llu names segment %u, which the call does not list", (unsigned long long)r, t.seg_id); return NS_E_INVAL; }
            if (t.byte_off % 8 != 0) { err = fc_format("ref %llu: byte offset %llu is not a multiple of 8", (unsigned long long)r, (unsigned long long)t.byte_off); return NS_E_INVAL; }
            if (t.byte_off / 8 + t.count > segs[slot].n_postings) { err = fc_format("ref %llu runs past the postings of segment %u", (unsigned long long)r, t.seg_id); return NS_E_INVAL; }
            order.push_back({(uint32_t)slot, (uint32_t)r});
        }
        std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (size_t i = 0; i < order.size();) {
            size_t j = i;
            while (j < order.size() && order[j].first == order[i].first) j++;
            const FcSegView& sv = segs[order[i].first];
            const uint32_t begin = (uint32_t)out_refs.size();
            bool dead = false;
            for (size_t k = i; k < j; k++) {
                const ns_term_ref& t = refs[order[k].second];
                if (!t.count) { dead = dead || and_mode; continue; }
                const uint64_t first = t.byte_off / 8;
                const uint32_t skip = (sv.skip_of && first < (1ull << 32)) ? sv.skip_of((uint32_t)first, t.count) : 0u;
                out_refs.push_back(FcRef{first, t.count, skip});
            }
            const uint32_t count = (uint32_t)out_refs.size() - begin;
            if (dead || !count || !sv.n_docs) out_refs.resize(begin);
            else
                for (uint64_t lo = 0; lo < sv.n_docs; lo += tile_docs)
                    out_items.push_back(FcItem{q, order[i].first, begin, count, (uint32_t)lo, (uint32_t)std::min<uint64_t>(lo + tile_docs, sv.n_docs)});
            i = j;
        }
    }
    return NS_OK;
}

}  // namespace ns
