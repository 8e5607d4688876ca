// SPDX-License-Identifier: MIT
// One hit per group, the count pass of ns_search_collapsed: how many matched documents of the whole call carry
// each hit's group.  The collapsing kept set (CgSet / cg_insert), the COLLAPSE instantiations of k_bq_select and the join
// (k_bq_join_collapsed) are in ns_boolean.hip; this file holds what runs after the join, once more over the same work items.
//   k_cl_count    one workgroup of 256 threads per item.
//                   groups  the query's hit groups (at most K <= 128 values, written by the join) are read into LDS and ranked
//                           among themselves: s_sorted[rank] = (group, r).  The groups of a query's hits are distinct, so the
//                           ranks are; key 0 is no group and is left out.  A query without a grouped hit ends the item here
//                           (workgroup-uniform).
//                   match   bs_matched (ns_boolean_sets.hip): the tile's matched set, role by role, every dialect form; an item
//                           of one ref is its in-tile postings, as in k_bs_count.
//                   sweep   per matched document one gather of its group, 4 B; a binary search over s_sorted; one LDS atomic add
//                           on the counter of the hit's rank r.
//                   flush   the nonzero counters go into others[q * K + r] with global integer atomics, as k_bs_count flushes.
//                 The join left 0xFFFFFFFF in others[] for a hit with a group, so the sum is the group's matched documents minus
//                 one; unsigned wrap-around is the subtraction.  No dependence on the item order.
// Every docId read from a list is tested against the tile before it indexes LDS or the group table.
// Static LDS: 34 KiB per workgroup (2 x 16 KiB bitmaps, 1 KiB of sorted groups, 512 B of counters, 512 B of ranks); QUORUM launches
// add their counter planes behind it, as k_bs_count's do.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ns_boolean_plan.hpp"
#include "ns_collapse_plan.hpp"

namespace ns {

template <bool GROUPED, bool QUORUM>
__global__ void __launch_bounds__(256) k_cl_count(const FcItem* __restrict__ items, const BqRef* __restrict__ refs,
                                                  const DevFcSeg* __restrict__ segs, const DevBqSeg* __restrict__ bqs, uint32_t K,
                                                  const uint32_t* __restrict__ nhits, const uint32_t* __restrict__ groups,
                                                  uint32_t* __restrict__ others) {
    __shared__ uint32_t s_bm[kFcTileDocs / 32u];
    __shared__ uint32_t s_tmp[kFcTileDocs / 32u];
    __shared__ uint2 s_sorted[kSdRowSlots];      // (group, rank of the hit), ascending by group
    __shared__ uint32_t s_grp[kSdRowSlots];      // the query's hit groups by rank of the hit; 0 = none
    __shared__ uint32_t s_cnt[kSdRowSlots];
    __shared__ uint32_t s_n;                     // the query's hits with a group
    extern __shared__ __attribute__((aligned(16))) uint32_t s_cl_planes[];   // QUORUM: 16 KiB per plane of the launch, else none
    const FcItem it = items[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    NS_CLCNT(13, 1);
    const uint32_t nh = min(nhits[it.query], K);   // K <= kSdRowSlots: the call's plan clamps it
    if (tid < kSdRowSlots) {
        s_grp[tid] = tid < nh ? groups[(size_t)it.query * K + tid] : 0u;
        s_cnt[tid] = 0u;
    }
    __syncthreads();
    uint32_t mine = 0, below = 0, total = 0;
    if (tid < kSdRowSlots) {
        mine = s_grp[tid];
        for (uint32_t j = 0; j < nh; j++) {
            const uint32_t g = s_grp[j];
            total += g != 0u;
            below += g != 0u && g < mine;
        }
        if (mine) s_sorted[below] = make_uint2(mine, tid);
    }
    if (tid == 0) s_n = total;
    __syncthreads();
    const uint32_t ng = s_n;
    if (ng == 0u) { NS_CLCNT(11, 1); return; }     // (workgroup-uniform) no hit of the query has a group
    const DevFcSeg sg = segs[it.seg];
    const BqRef* __restrict__ rf = refs + it.ref_begin;
    const uint32_t* __restrict__ grp = bq_group_table(bqs, it.seg);
    const uint32_t n_words = (it.doc_hi - it.doc_lo + 31u) / 32u;   // <= kFcTileDocs / 32: the tile is the host's, at most the product's
    // one matched document d of the tile (d < doc_hi <= n_docs = the table's length: the call checked)
    auto count_doc = [&](uint32_t d) {
        const uint32_t g = grp[d];
        if (!g) return;
        const uint32_t at = cl_lower_bound(s_sorted, ng, g);
        if (at < ng && s_sorted[at].x == g) {
            atomicAdd(&s_cnt[s_sorted[at].y], 1u);
#ifdef NS_COUNT
            atomicAdd(&g_ns_clcnt[10], 1ull);
#endif
        }
    };
    if (it.ref_count == 1u) {
        uint64_t lo, hi;
        fc_cut(sg, rf[0].list, it.doc_lo, it.doc_hi, lane, lo, hi);
        for (uint64_t i = lo + tid; i < hi; i += 256u) {
            const uint32_t d = sg.postings[i].x;
            if (d >= it.doc_lo && d < it.doc_hi) count_doc(d);
        }
    } else {
        if (!bs_matched<GROUPED, QUORUM>(it, sg, rf, n_words, s_bm, s_tmp, QUORUM ? s_cl_planes : nullptr)) return;   // (workgroup-uniform)
        for (uint32_t w = tid; w < n_words; w += 256u) {
            uint32_t bits = s_bm[w];
            while (bits) {
                const uint32_t d = it.doc_lo + w * 32u + (uint32_t)__builtin_ctz(bits);   // < doc_hi: only such bits are set
                bits &= bits - 1u;
                count_doc(d);
            }
        }
    }
    __syncthreads();
    if (tid < nh) {
        const uint32_t c = s_cnt[tid];
        if (c) atomicAdd(&others[(size_t)it.query * K + tid], c);
    }
}

}  // namespace ns
