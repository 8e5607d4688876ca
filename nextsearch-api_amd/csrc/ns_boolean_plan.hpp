// Boolean queries: term refs with a role each -> (query, segment) groups -> work items of k_bq_select, one per
// doc-range tile of the facet tile size.  Host code only, like ns_facet_plan.hpp: no HIP runtime call and no device
// pointer; tests/boolean_plan_harness.cpp compiles it with g++ for the CPU suite.  fc_plan and ns_sorted_plan.hpp are
// untouched: the items are FcItems, sd_query_items and sd_cut apply to them as they are.
// Any-of groups: bq_plan_grouped takes a clause value per ref next to its role; bq_plan is that call without
// clause values (tests/grouped_plan_harness.cpp compiles both).
// At-least-m-of-n clauses: bq_plan_quorum takes a need per ref next to its clause value; bq_plan_grouped is that
// call without needs (tests/quorum_plan_harness.cpp compiles all three).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "ns_sorted_plan.hpp"

namespace ns {

// role of a ref (NS_ROLE_SHOULD / NS_ROLE_MUST / NS_ROLE_NOT of nextsearch_hip.h)
static constexpr uint32_t kBqShould = 0, kBqMust = 1, kBqNot = 2;
// Documents per window of the product build: k_bq_select walks a tile in windows whose fp32 accumulators (4 B per
// document) and three bitmaps live in LDS: 32 KiB + 3 KiB at 2^13.
static constexpr uint32_t kBqWinDocs = 1u << 13;
// The largest window a test build may ask for: 128 KiB + 12 KiB + the 4 KiB row exchange still fit the 160 KiB of a CU.
static constexpr uint32_t kBqMaxWinDocs = 1u << 15;
// a test window (variants and counting builds): a power of two, whole bitmap words
inline bool bq_win_ok(uint32_t w) { return w >= 32 && w <= kBqMaxWinDocs && (w & (w - 1)) == 0; }

// One posting list of a group, in the group's (= the query's) order.
struct BqRef {
    FcRef list;
    uint32_t role;
    float idf, qweight;   // unused under kBqNot
    uint32_t clause;      // bq_plan_grouped with clause values, MUST refs: the clause's dense index within the group; else 0
                          // bq_plan_quorum with needs, MUST refs: bq_clause_word's packing of index, need and the duplicate flag
};
static_assert(sizeof(BqRef) == 32, "BqRef is uploaded as it is");

// At-least-m-of-n: the largest need a clause may carry, and how BqRef::clause holds it.  Bits 0..15 the dense
// index (a group has at most 65536 clause values), bits 16..18 the need (1..7; 0 where the call had no needs, read as 1), bit 19
// "does not count": an earlier surviving ref of the same clause names the same list, so this ref is cut and scored but not counted.
static constexpr uint32_t kBqMaxNeed = 7;
static constexpr uint32_t kBqClauseMask = 0xFFFFu, kBqNeedShift = 16u, kBqNeedMask = 7u, kBqDupBit = 1u << 19;
inline constexpr uint32_t bq_clause_word(uint32_t dense, uint32_t need, bool dup) { return dense | (need << kBqNeedShift) | (dup ? kBqDupBit : 0u); }
inline constexpr uint32_t bq_clause_index(uint32_t word) { return word & kBqClauseMask; }
inline constexpr uint32_t bq_clause_need(uint32_t word) { return ((word >> kBqNeedShift) & kBqNeedMask) ? ((word >> kBqNeedShift) & kBqNeedMask) : 1u; }
// counter planes of a clause with this need: the planes count to 2^p - 1 and saturate there
inline constexpr uint32_t bq_need_planes(uint32_t need) { return need <= 1u ? 0u : need <= 3u ? 2u : 3u; }

// Checks the descriptors and cuts the items.  Per query the refs are grouped by segment (in the order of the call's segment
// list, refs of a group in query order, each with its role; roles == nullptr: all SHOULD).  Per group: a MUST ref without
// postings kills the group; SHOULD and NOT refs without postings are dropped; a group left without a MUST or SHOULD ref
// matches nothing.  Every other group gets one item per tile of [0, n_docs), the last one shorter, query by query.  A ref
// that scores (MUST, SHOULD) must have a finite idf and qweight.  Returns NS_OK, or NS_E_INVAL with `err` set and nothing
// usable in the outputs.
// Grouped: clauses[r] (parallel to refs; read under kBqMust only) names the clause of a MUST ref.  Per group
// the MUST refs of equal value form one clause, of which a document must hold at least one list: its refs without postings
// are dropped, and a clause ALL of whose refs are without postings kills the group.  BqRef::clause is the clause's dense
// index within the group, numbered by first appearance among the refs that survive.  clauses == nullptr: every MUST ref is
// a clause of its own, clause stays 0, and the output is bq_plan's byte for byte.
// Quorum: needs[r] (parallel to refs; read under kBqMust only; 0 reads as 1; above kBqMaxNeed refused) says how
// many DISTINCT lists of the ref's clause a document must lie in.  The refs of one clause in one group must agree on it.  Two refs
// name the same list when their byte offset and count are equal; the later one gets kBqDupBit and is not counted.  A clause with
// fewer distinct lists with postings than its need kills the group (need 1: bq_plan_grouped's rule).  BqRef::clause is
// bq_clause_word(...); max_need is the largest need among the refs that were emitted (0: none).  needs == nullptr: bq_plan_grouped,
// byte for byte, and max_need = 0; needs without clauses is refused.
inline int bq_plan_quorum(const ns_query_desc* qd, uint32_t n_queries, const ns_term_ref* refs, const uint8_t* roles, const uint16_t* clauses,
                          const uint8_t* needs, uint32_t n_refs, const FcSegView* segs, uint32_t n_segs, uint32_t tile_docs,
                          std::vector<BqRef>& out_refs, std::vector<FcItem>& out_items, uint32_t& max_need, std::string& err) {
    out_refs.clear();
    out_items.clear();
    max_need = 0;
    auto refuse = [&](const std::string& why) { out_refs.clear(); out_items.clear(); max_need = 0; err = why; return NS_E_INVAL; };
    if (needs && !clauses) return refuse("needs without clauses: a need belongs to a clause");
    if (!fc_tile_ok(tile_docs)) return refuse(fc_format("facet tile of %u documents: not a power of two in [32, %u]", tile_docs, kFcTileDocs));
    std::vector<std::pair<uint32_t, uint32_t>> by_id(n_segs);   // (seg_id, position)
    for (uint32_t i = 0; i < n_segs; i++) by_id[i] = {segs[i].seg_id, i};
    std::sort(by_id.begin(), by_id.end());
    for (uint32_t i = 1; i < n_segs; i++)
        if (by_id[i].first == by_id[i - 1].first) return refuse(fc_format("seg_id %u is listed twice", by_id[i].first));
    auto slot_of = [&](uint32_t id) -> int64_t {
        auto it = std::lower_bound(by_id.begin(), by_id.end(), std::make_pair(id, 0u));
        return (it != by_id.end() && it->first == id) ? (int64_t)it->second : -1;
    };
    std::vector<std::pair<uint32_t, uint32_t>> order;   // (position of the segment, ref index) of one query
    std::vector<uint8_t> live(clauses ? 65536u : 0u, 0);   // per clause value: 1 = named by the group, 2 = a ref of it has postings
    std::vector<uint32_t> dense(clauses ? 65536u : 0u, 0);  // per clause value that survives: its dense index
    const bool quorum = needs && clauses && roles;
    std::vector<uint8_t> need_of(quorum ? 65536u : 0u, 0);      // per clause value of the group: its need (0 = not seen yet)
    std::vector<uint32_t> distinct(quorum ? 65536u : 0u, 0);    // per clause value of the group: its distinct lists with postings
    struct Named { uint16_t clause; uint64_t off; uint32_t count; uint32_t k; };
    std::vector<Named> named;                                   // the MUST refs with postings of one group
    std::vector<uint8_t> dup;                                   // per ref of the group (k - i): 1 = kBqDupBit
    for (uint32_t q = 0; q < n_queries; q++) {
        const uint64_t tb = qd[q].term_begin, tc = qd[q].term_count;
        if (tb + tc > n_refs) return refuse(fc_format("query %u: refs [%llu, %llu) run past the %u given", q, (unsigned long long)tb, (unsigned long long)(tb + tc), n_refs));
        order.clear();
        for (uint64_t r = tb; r < tb + tc; r++) {
            const ns_term_ref& t = refs[r];
            const uint32_t role = roles ? roles[r] : kBqShould;
            if (role > kBqNot) return refuse(fc_format("ref %llu: role %u is none of NS_ROLE_SHOULD, NS_ROLE_MUST, NS_ROLE_NOT", (unsigned long long)r, role));
            const int64_t slot = slot_of(t.seg_id);
            if (slot < 0) return refuse(fc_format("ref %llu names segment %u, which the call does not list", (unsigned long long)r, t.seg_id));
            if (t.byte_off % 8 != 0) return refuse(fc_format("ref %llu: byte offset %llu is not a multiple of 8", (unsigned long long)r, (unsigned long long)t.byte_off));
            if (t.byte_off / 8 + t.count > segs[slot].n_postings) return refuse(fc_format("ref %llu runs past the postings of segment %u", (unsigned long long)r, t.seg_id));
            if (role != kBqNot && !(std::isfinite(t.idf) && std::isfinite(t.qweight))) return refuse(fc_format("ref %llu: idf or qweight is not finite", (unsigned long long)r));
            if (quorum && role == kBqMust && needs[r] > kBqMaxNeed)
                return refuse(fc_format("ref %llu: a need of %u (query %u); at most %u", (unsigned long long)r, (uint32_t)needs[r], q, kBqMaxNeed));
            order.push_back({(uint32_t)slot, (uint32_t)r});
        }
        std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (size_t i = 0; i < order.size();) {
            size_t j = i;
            while (j < order.size() && order[j].first == order[i].first) j++;
            const FcSegView& sv = segs[order[i].first];
            const uint32_t begin = (uint32_t)out_refs.size();
            bool dead = false;
            uint32_t positive = 0, n_clauses = 0;
            if (clauses && roles) {
                for (size_t k = i; k < j; k++)
                    if (roles[order[k].second] == kBqMust) {
                        uint8_t& l = live[clauses[order[k].second]];
                        l = std::max<uint8_t>(l, refs[order[k].second].count ? 2 : 1);
                    }
                for (size_t k = i; k < j; k++)
                    if (roles[order[k].second] == kBqMust) dead = dead || live[clauses[order[k].second]] == 1;
            }
            if (quorum) {
                named.clear();
                dup.assign(j - i, 0);
                bool differ = false;
                uint32_t differ_clause = 0, differ_a = 0, differ_b = 0;
                for (size_t k = i; k < j; k++) {
                    const uint32_t r = order[k].second;
                    if (roles[r] != kBqMust) continue;
                    const uint16_t c = clauses[r];
                    const uint8_t need = needs[r] ? needs[r] : 1;
                    if (!need_of[c]) need_of[c] = need;
                    else if (need_of[c] != need && !differ) { differ = true; differ_clause = c; differ_a = need_of[c]; differ_b = need; }
                    if (refs[r].count) named.push_back(Named{c, refs[r].byte_off, refs[r].count, (uint32_t)(k - i)});
                }
                if (differ) return refuse(fc_format("query %u: the refs of clause %u carry the needs %u and %u", q, differ_clause, differ_a, differ_b));
                std::sort(named.begin(), named.end(), [](const Named& a, const Named& b) {
                    return a.clause != b.clause ? a.clause < b.clause : a.off != b.off ? a.off < b.off : a.count != b.count ? a.count < b.count : a.k < b.k;
                });
                for (size_t a = 0; a < named.size(); a++) {
                    const bool same = a && named[a].clause == named[a - 1].clause && named[a].off == named[a - 1].off && named[a].count == named[a - 1].count;
                    if (same) dup[named[a].k] = 1;
                    else distinct[named[a].clause]++;
                }
                for (size_t k = i; k < j; k++)
                    if (roles[order[k].second] == kBqMust) dead = dead || distinct[clauses[order[k].second]] < need_of[clauses[order[k].second]];
            }
            for (size_t k = i; k < j; k++) {
                const ns_term_ref& t = refs[order[k].second];
                const uint32_t role = roles ? roles[order[k].second] : kBqShould;
                if (!t.count) { dead = dead || (role == kBqMust && !clauses); continue; }
                const uint64_t first = t.byte_off / 8;
                const uint32_t skip = (sv.skip_of && first < (1ull << 32)) ? sv.skip_of((uint32_t)first, t.count) : 0u;
                uint32_t clause = 0;
                if (clauses && role == kBqMust) {
                    const uint16_t c = clauses[order[k].second];
                    if (live[c] == 2) { live[c] = 3; dense[c] = n_clauses++; }   // 3 = numbered
                    clause = quorum ? bq_clause_word(dense[c], need_of[c], dup[k - i] != 0) : dense[c];
                }
                out_refs.push_back(BqRef{FcRef{first, t.count, skip}, role, t.idf, t.qweight, clause});
                positive += role != kBqNot;
            }
            if (clauses && roles)
                for (size_t k = i; k < j; k++)
                    if (roles[order[k].second] == kBqMust) {
                        live[clauses[order[k].second]] = 0;
                        if (quorum) need_of[clauses[order[k].second]] = 0, distinct[clauses[order[k].second]] = 0;
                    }
            const uint32_t count = (uint32_t)out_refs.size() - begin;
            if (dead || !positive || !sv.n_docs) out_refs.resize(begin);
            else {
                if (quorum)
                    for (uint32_t k = begin; k < begin + count; k++)
                        if (out_refs[k].role == kBqMust) max_need = std::max(max_need, bq_clause_need(out_refs[k].clause));
                for (uint64_t lo = 0; lo < sv.n_docs; lo += tile_docs)
                    out_items.push_back(FcItem{q, order[i].first, begin, count, (uint32_t)lo, (uint32_t)std::min<uint64_t>(lo + tile_docs, sv.n_docs)});
            }
            i = j;
        }
    }
    return NS_OK;
}

inline int bq_plan_grouped(const ns_query_desc* qd, uint32_t n_queries, const ns_term_ref* refs, const uint8_t* roles, const uint16_t* clauses,
                           uint32_t n_refs, const FcSegView* segs, uint32_t n_segs, uint32_t tile_docs, std::vector<BqRef>& out_refs,
                           std::vector<FcItem>& out_items, std::string& err) {
    uint32_t max_need;
    return bq_plan_quorum(qd, n_queries, refs, roles, clauses, nullptr, n_refs, segs, n_segs, tile_docs, out_refs, out_items, max_need, err);
}

inline int bq_plan(const ns_query_desc* qd, uint32_t n_queries, const ns_term_ref* refs, const uint8_t* roles, uint32_t n_refs,
                   const FcSegView* segs, uint32_t n_segs, uint32_t tile_docs, std::vector<BqRef>& out_refs,
                   std::vector<FcItem>& out_items, std::string& err) {
    return bq_plan_grouped(qd, n_queries, refs, roles, nullptr, n_refs, segs, n_segs, tile_docs, out_refs, out_items, err);
}

}  // namespace ns
