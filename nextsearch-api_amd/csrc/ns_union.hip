// SPDX-License-Identifier: MIT
// A derived segment of copied lists and union lists: ns_segment_union publishes, as an ordinary segment, the
// lists a call names (single groups, copied verbatim) and the unions of several lists with the tf summed per document (multi
// groups), so that the planner and every scoring body work on a blended term unchanged.  The host plans everything that does
// not depend on the postings' docIds (ns_union_plan.hpp); the multi groups go through dense tables in rounds:
//   k_un_copy     a wave takes one item: up to 64 neighbouring postings of a single group and their per-posting norms go to
//                 the place the host gave them (8 B + 4 B per lane, coalesced)
//   k_un_add      a wave takes one item: up to 64 consecutive postings of ONE member, so the table is wave-uniform; lane l
//                 adds its tf into table[docId] with a global atomic whose result nobody reads.  Integer adds commute: the
//                 table is exact whatever the order.  A docId >= n_docs is dropped.
//   k_un_mark     a wave takes 64 neighbouring entries of a table and stores the ballot of the non-zero ones as mask[chunk]
//                 and its popcount as cnt[chunk] (k_fl_mark's shape; the last chunk of a table is partial).  Chunks never
//                 span two tables.
//   scan (§5i's)  base[chunk] = entries in front of the chunk within the round; base[n_chunks] = the round's postings
//   k_un_scatter  lane with a set bit stores {doc, table[doc]} and norm[doc] at run[r] + base[chunk] + its rank in the mask:
//                 docId-ascending within a table, tables in the round's order
//   k_un_lists    one thread per table of the round: the group's place in the new payload; thread 0 also stores
//                 run[r + 1] = run[r] + base[n_chunks].  run[] lives on the device: no round waits for the host.
//   k_un_pad      the kPadPostings entries behind the last posting, whose place only the device knows until the call ends
// All stores are plain stores; no kernel waits on another workgroup.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ns_union_plan.hpp"

namespace ns {

__global__ void __launch_bounds__(256) k_un_copy(const uint2* __restrict__ postings, const float* __restrict__ pnorm,
                                                 const UnCopyItem* __restrict__ items, uint32_t n_items,
                                                 uint2* __restrict__ out, float* __restrict__ pnorm_out) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6); w < n_items; w += gridDim.x * 4u) {   // w: wave-uniform
        const UnCopyItem it = items[w];
        if (lane >= it.n) continue;
        out[it.dst + lane] = postings[it.src + lane];
        pnorm_out[it.dst + lane] = pnorm[it.src + lane];
    }
}

// tables: the round's tables, n_docs entries each, zeroed
__global__ void __launch_bounds__(256) k_un_add(const uint2* __restrict__ postings, const UnAddItem* __restrict__ items, uint32_t n_items,
                                                uint32_t n_docs, uint32_t* __restrict__ tables) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6); w < n_items; w += gridDim.x * 4u) {
        const UnAddItem it = items[w];
        if (lane >= it.n) continue;
        const uint2 p = postings[it.src + lane];
        if (p.x < n_docs) atomicAdd(tables + (size_t)it.table * n_docs + p.x, p.y);
    }
}

// mask, cnt: n_tables * cpt + 1 words with cpt = ceil(n_docs / 64) (the last of each is 0: the scan's total then is base[n_chunks])
__global__ void __launch_bounds__(256) k_un_mark(const uint32_t* __restrict__ tables, uint32_t n_tables, uint32_t n_docs, uint32_t cpt,
                                                 uint64_t* __restrict__ mask, uint32_t* __restrict__ cnt) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_chunks = n_tables * cpt;
    for (uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6); c <= n_chunks; c += gridDim.x * 4u) {
        const uint32_t t = c / cpt, doc = (c % cpt) * kUnChunk + lane;
        bool named = false;
        if (c < n_chunks && doc < n_docs) named = tables[(size_t)t * n_docs + doc] != 0u;
        const uint64_t m = __ballot(named);
        if (lane == 0) {
            mask[c] = m;
            cnt[c] = (uint32_t)__popcll(m);
        }
    }
}

// base: the exclusive scan of cnt; run: the postings written before this round
__global__ void __launch_bounds__(256) k_un_scatter(const uint32_t* __restrict__ tables, uint32_t n_tables, uint32_t n_docs, uint32_t cpt,
                                                    const uint64_t* __restrict__ mask, const uint32_t* __restrict__ base,
                                                    const uint32_t* __restrict__ run, const float* __restrict__ norm,
                                                    uint2* __restrict__ out, float* __restrict__ pnorm_out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_chunks = n_tables * cpt;
    const uint32_t first = *run;
    for (uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6); c < n_chunks; c += gridDim.x * 4u) {
        const uint64_t m = mask[c];
        if (!((m >> lane) & 1ull)) continue;                      // a set bit implies doc < n_docs
        const uint32_t t = c / cpt, doc = (c % cpt) * kUnChunk + lane;
        const uint32_t at = first + base[c] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        out[at] = make_uint2(doc, tables[(size_t)t * n_docs + doc]);
        pnorm_out[at] = norm[doc];
    }
}

// groups: the round's groups, one per table; run[1] is the next round's run[0]
__global__ void __launch_bounds__(256) k_un_lists(const uint32_t* __restrict__ groups, uint32_t n_tables, uint32_t cpt,
                                                  const uint32_t* __restrict__ base, uint32_t* __restrict__ run,
                                                  uint64_t* __restrict__ new_byte_off, uint32_t* __restrict__ new_counts) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tables) return;
    const uint32_t first = run[0], a = base[t * cpt], b = base[(t + 1) * cpt];
    new_byte_off[groups[t]] = (uint64_t)(first + a) * 8u;
    new_counts[groups[t]] = b - a;
    if (t == 0) run[1] = first + base[n_tables * cpt];
}

// n_pad entries behind the last posting: docId ~0 (never taken), norm 0
__global__ void __launch_bounds__(256) k_un_pad(const uint32_t* __restrict__ run, uint32_t n_pad, uint2* __restrict__ out, float* __restrict__ pnorm_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_pad) return;
    out[*run + i] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    pnorm_out[*run + i] = 0.0f;
}

}  // namespace ns
