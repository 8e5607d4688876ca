// SPDX-License-Identifier: MIT
// What ns_segment_union plans before it touches the device.  Host only: no HIP header, no device symbol;
// tests/union_plan_harness.cpp compiles it with g++ alone.
//
// The new payload is [the single groups' lists, in group order][the multi groups' unions, in round order].  A posting is 8 B,
// so every list starts at a multiple of 8.  The single part is known here; the multi part is packed on the device, round by
// round, behind a running base that starts at the single part's size.
//   single group   one member: copied verbatim by k_un_copy, one wave item per 64 postings
//   multi group    two or more members: one uint32_t[n_docs] table in a round; k_un_add adds every member posting into it,
//                  one wave item per 64 consecutive postings of ONE member, so the table is wave-uniform
//   round          the multi groups whose tables share the scratch: R = max(1, scratch / (4 * n_docs)) tables, in group
//                  order.  A multi group without a posting (or of a segment without documents) needs no table and is in no round:
//                  its count is 0.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace ns {

constexpr uint32_t kUnChunk = 64;                      // postings per wave item == table entries per mark chunk == lanes of a wave
constexpr uint64_t kUnDefaultScratch = 64ull << 20;    // table bytes per round (ns_ctx_union_scratch(ctx, 0))
constexpr uint64_t kUnMaxScratch = 16ull << 30;        // R * ceil(n_docs / 64) then stays far below 2^32

struct UnCopyItem { uint32_t src, dst, n; };      // postings [src, src + n) of the source go to [dst, dst + n) of the copy, n <= 64
struct UnAddItem { uint32_t src, n, table; };     // postings [src, src + n) of the source are added into table `table` of the round, n <= 64
struct UnRound {
    uint32_t first_table;   // index into UnionPlan::tabled of the round's first group
    uint32_t n_tables;
    uint32_t first_item;    // the round's wave items in UnionPlan::add_items
    uint32_t n_items;
};

struct UnionPlan {
    std::vector<uint32_t> single_off;     // per group: where a single group's list starts in the new payload (postings); multi groups: 0
    std::vector<UnCopyItem> copy_items;
    std::vector<uint32_t> tabled;         // the multi groups with a posting, in group order
    std::vector<UnRound> rounds;
    std::vector<UnAddItem> add_items;     // round by round
    uint64_t single_postings = 0;         // the running base's first value
    uint64_t bound = 0;                   // capacity of the new payload in postings: singles + per multi group min(sum of member counts, n_docs)
    uint32_t tables_per_round = 1;
};

// tables that fit in `scratch` bytes, and always at least one
inline uint32_t union_tables_per_round(uint64_t scratch, uint32_t n_docs) {
    const uint64_t one = (uint64_t)std::max<uint32_t>(n_docs, 1) * 4;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(scratch / one, 1), 0xFFFFFFFFull);
}

// member_first[i] = member_off[i] / 8.  group_begin is non-decreasing from 0 (the caller's check).
inline UnionPlan union_plan(const uint32_t* member_first, const uint32_t* member_cnt, const uint32_t* group_begin, uint32_t n_groups,
                            uint32_t n_docs, uint64_t scratch) {
    UnionPlan p;
    p.single_off.assign(n_groups, 0);
    p.tables_per_round = union_tables_per_round(scratch, n_docs);
    std::vector<uint64_t> sums(n_groups, 0);
    for (uint32_t g = 0; g < n_groups; g++) {
        const uint32_t b = group_begin[g], e = group_begin[g + 1];
        for (uint32_t i = b; i < e; i++) sums[g] += member_cnt[i];
        if (e - b == 1) {
            p.single_off[g] = (uint32_t)p.single_postings;
            for (uint32_t at = 0; at < member_cnt[b]; at += kUnChunk)
                p.copy_items.push_back({member_first[b] + at, (uint32_t)p.single_postings + at, std::min(member_cnt[b] - at, kUnChunk)});
            p.single_postings += member_cnt[b];
        } else if (e - b >= 2 && sums[g] && n_docs) {
            p.tabled.push_back(g);
            p.bound += std::min<uint64_t>(sums[g], n_docs);
        }
    }
    p.bound += p.single_postings;
    for (uint32_t t0 = 0; t0 < p.tabled.size(); t0 += p.tables_per_round) {
        UnRound r{t0, (uint32_t)std::min<uint64_t>(p.tables_per_round, p.tabled.size() - t0), (uint32_t)p.add_items.size(), 0};
        for (uint32_t t = 0; t < r.n_tables; t++) {
            const uint32_t g = p.tabled[t0 + t];
            for (uint32_t i = group_begin[g]; i < group_begin[g + 1]; i++)
                for (uint32_t at = 0; at < member_cnt[i]; at += kUnChunk)
                    p.add_items.push_back({member_first[i] + at, std::min(member_cnt[i] - at, kUnChunk), t});
        }
        r.n_items = (uint32_t)p.add_items.size() - r.first_item;
        p.rounds.push_back(r);
    }
    return p;
}

}  // namespace ns
