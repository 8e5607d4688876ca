// SPDX-License-Identifier: MIT
// Facet counts: for a batch of queries, the number of distinct matched documents per bucket of a
// per-document bucket table, from the posting lists alone (8 B per posting; no score, no norm).  ns_facet_count cuts the
// batch into work items on the host (ns_facet_plan.hpp): one (query, segment) group over one tile of kFcTileDocs documents.
//   k_fc_check   at upload: is every bucket id of a table < n_buckets?
//   k_fc_count   one workgroup of 256 threads per item:
//     cut      per list the postings inside the tile: from the list's skip table where it has one (1024-doc cells; a tile
//              edge inside a cell is found by a search inside that cell), otherwise by a search over the list.  A search is
//              wave-wide: 64 probes per step, one ballot, so a list of 2^24 postings takes four steps.  A tile that starts
//              at document 0 or ends at n_docs needs no search on that side.
//     mark     the tile's matched set is a bitmap in LDS (16 KiB for 2^17 documents); postings are read 256 per step
//              (64 per wave, coalesced) and OR-ed in with LDS atomics.  Every docId is tested against the tile, so a list
//              that is not ascending can lose counts but cannot write outside the bitmap.
//     AND      the first list marks the bitmap, every further list marks a second one, which is AND-ed in and cleared in
//              one pass.  A list without a posting in the tile ends the item.
//     sweep    per set bit one gather of bucket_of_doc (2 B) and one LDS atomic add into the tile's histogram (4 KiB)
//     flush    nonzero histogram entries go to the query's row with global integer atomics: the result does not depend
//              on the order in which the items run
//   A group of ONE list needs no bitmap: its postings are its documents and go straight into the histogram.
// LDS: 20 KiB per workgroup (OR), 36 KiB (AND).  All stores to global memory are atomic adds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ns_facet_plan.hpp"
#include "ns_internal.h"

namespace ns {

struct DevFcSeg {
    const uint2* postings;
    const uint32_t* skips;      // the segment's skip tables (nullptr: none; then no ref carries FcRef::skip)
    const uint16_t* buckets;    // bucket_of_doc
    uint32_t n_docs;
    uint32_t pad;
};

#ifdef NS_COUNT
// Counting build only: events of k_fc_count over all items since the last reset (ns_debug_facet_counters).  0 items,
// 1 items that intersected two bitmaps (AND), 2 single-list items, 3 cuts taken from a skip table, 4 cuts by a search over
// the list, 5 skip-table cuts that searched inside a cell, 6 AND items ended by a list without a posting in the tile,
// 7 histogram entries flushed.
constexpr int kNsFcnt = 8;
__device__ unsigned long long g_ns_fcnt[kNsFcnt];
#define NS_FCNT(i, v) do { if (threadIdx.x == 0) atomicAdd(&g_ns_fcnt[(i)], (unsigned long long)(v)); } while (0)
#else
#define NS_FCNT(i, v)
#endif

__global__ void __launch_bounds__(256) k_fc_check(const uint16_t* __restrict__ buckets, uint32_t n_docs, uint32_t n_buckets,
                                                  uint32_t* __restrict__ bad) {
    bool b = false;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_docs; i += gridDim.x * 256u) b = b || buckets[i] >= n_buckets;
    if (b) atomicOr(bad, 1u);
}

// The first index i in [a, b) with postings[i].x >= doc, or b.  Called by all 64 lanes of a wave with the same arguments;
// every index read lies in [a, b), whatever the order of the list.
__device__ __forceinline__ uint64_t fc_lower_bound(const uint2* __restrict__ postings, uint64_t a, uint64_t b, uint32_t doc, uint32_t lane) {
    if (a > b) a = b;
    while (b - a > 64u) {
        const uint64_t step = (b - a + 63u) / 64u;
        const uint64_t i = a + lane * step;
        const bool less = i < b && postings[i].x < doc;
        const uint32_t c = (uint32_t)__popcll(__ballot(less));   // ascending: the probes below `doc` are the first c
        if (c == 0u) return a;
        const uint64_t nb = a + c * step;
        a += (c - 1u) * step + 1u;
        b = nb < b ? nb : b;
    }
    const uint64_t i = a + lane;
    const bool less = i < b && postings[i].x < doc;
    return a + (uint32_t)__popcll(__ballot(less));
}

// The postings [lo, hi) of list rf that can lie in the documents [doc_lo, doc_hi); doc_lo < doc_hi <= n_docs.
__device__ __forceinline__ void fc_cut(const DevFcSeg& sg, const FcRef& rf, uint32_t doc_lo, uint32_t doc_hi, uint32_t lane,
                                       uint64_t& lo, uint64_t& hi) {
    const uint64_t first = rf.first, end = rf.first + rf.count;
    if (rf.skip) {
        const uint32_t* __restrict__ sk = sg.skips + (rf.skip - 1u);   // entries 0 .. ceil(n_docs / kSkipDocs) + 1
        const uint32_t cl = doc_lo / kSkipDocs, ch = doc_hi / kSkipDocs;
        lo = sk[cl];
        hi = sk[ch];
        NS_FCNT(3, 1);
        if (doc_lo % kSkipDocs) { lo = fc_lower_bound(sg.postings, max(lo, first), min((uint64_t)sk[cl + 1u], end), doc_lo, lane); NS_FCNT(5, 1); }
        if (doc_hi % kSkipDocs) { hi = fc_lower_bound(sg.postings, max(hi, first), min((uint64_t)sk[ch + 1u], end), doc_hi, lane); NS_FCNT(5, 1); }
        lo = min(max(lo, first), end);
        hi = min(max(hi, lo), end);
        return;
    }
    lo = first;
    hi = end;
    if (doc_lo != 0u) { lo = fc_lower_bound(sg.postings, first, end, doc_lo, lane); NS_FCNT(4, 1); }
    if (doc_hi < sg.n_docs) { hi = fc_lower_bound(sg.postings, lo, end, doc_hi, lane); NS_FCNT(4, 1); }
}

// postings [lo, hi) -> bits of the tile's bitmap
__device__ __forceinline__ void fc_mark(const uint2* __restrict__ postings, uint64_t lo, uint64_t hi, uint32_t doc_lo, uint32_t doc_hi,
                                        uint32_t* bm) {
    for (uint64_t i = lo + threadIdx.x; i < hi; i += 256u) {
        const uint32_t d = postings[i].x;
        if (d >= doc_lo && d < doc_hi) atomicOr(&bm[(d - doc_lo) >> 5], 1u << ((d - doc_lo) & 31u));
    }
}

template <bool AND>
__global__ void __launch_bounds__(256) k_fc_count(const FcItem* __restrict__ items, const FcRef* __restrict__ refs,
                                                  const DevFcSeg* __restrict__ segs, uint32_t n_buckets, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_hist[kFcMaxBuckets];
    __shared__ uint32_t s_bm[kFcTileDocs / 32u];
    __shared__ uint32_t s_and[AND ? kFcTileDocs / 32u : 1u];
    const FcItem it = items[blockIdx.x];
    const DevFcSeg sg = segs[it.seg];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t n_words = (it.doc_hi - it.doc_lo + 31u) / 32u;   // <= kFcTileDocs / 32: the tile is the host's, at most the product's
    NS_FCNT(0, 1);
    for (uint32_t b = tid; b < n_buckets; b += 256u) s_hist[b] = 0u;
    bool any = true;   // the same in every thread: the cuts depend on the item alone
    if (it.ref_count == 1u) {
        uint64_t lo, hi;
        fc_cut(sg, refs[it.ref_begin], it.doc_lo, it.doc_hi, lane, lo, hi);
        NS_FCNT(2, 1);
        __syncthreads();
        for (uint64_t i = lo + tid; i < hi; i += 256u) {
            const uint32_t d = sg.postings[i].x;
            if (d >= it.doc_lo && d < it.doc_hi) atomicAdd(&s_hist[sg.buckets[d]], 1u);
        }
    } else {
        for (uint32_t w = tid; w < n_words; w += 256u) {
            s_bm[w] = 0u;
            if (AND) s_and[w] = 0u;
        }
        __syncthreads();
        for (uint32_t r = 0; r < it.ref_count; r++) {
            uint64_t lo, hi;
            fc_cut(sg, refs[it.ref_begin + r], it.doc_lo, it.doc_hi, lane, lo, hi);
            if (AND) {
                if (lo == hi) { any = false; NS_FCNT(6, 1); break; }
                if (r == 0u) {
                    fc_mark(sg.postings, lo, hi, it.doc_lo, it.doc_hi, s_bm);
                    __syncthreads();
                } else {
                    fc_mark(sg.postings, lo, hi, it.doc_lo, it.doc_hi, s_and);
                    __syncthreads();
                    for (uint32_t w = tid; w < n_words; w += 256u) {
                        s_bm[w] &= s_and[w];
                        s_and[w] = 0u;
                    }
                    __syncthreads();
                    if (r == 1u) NS_FCNT(1, 1);
                }
            } else {
                fc_mark(sg.postings, lo, hi, it.doc_lo, it.doc_hi, s_bm);
            }
        }
        __syncthreads();
        if (any)
            for (uint32_t w = tid; w < n_words; w += 256u) {
                uint32_t bits = s_bm[w];
                while (bits) {
                    const uint32_t d = it.doc_lo + w * 32u + (uint32_t)__builtin_ctz(bits);   // < doc_hi: only such bits are set
                    bits &= bits - 1u;
                    atomicAdd(&s_hist[sg.buckets[d]], 1u);
                }
            }
    }
    __syncthreads();
    if (!any) return;
    uint32_t* __restrict__ row = counts + (size_t)it.query * n_buckets;
    for (uint32_t b = tid; b < n_buckets; b += 256u) {
        const uint32_t c = s_hist[b];
        if (c) {
            atomicAdd(&row[b], c);
#ifdef NS_COUNT
            atomicAdd(&g_ns_fcnt[7], 1ull);
#endif
        }
    }
}

}  // namespace ns
