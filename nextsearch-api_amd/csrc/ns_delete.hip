// SPDX-License-Identifier: MIT
// Deleting documents on the device: the filter in front of §5j's merge.  ns_forward_merge_keep hands every
// source a bitmap of the documents that stay; what these kernels leave behind is the input of the unchanged dictionary,
// remap and docsort stages of csrc/ns_compact.hip, all of it in device memory.
//
// The host walks the per-document counts anyway (ns_forward_merge builds the document prefix from them), so it also knows
// which documents stay, where each one's pairs lie in the sources as uploaded (srcpos) and the surviving documents' pair
// prefix.  What only the pairs can tell is which TERMS stay, and the pairs are the bulk of the data:
//   k_cp_keep_gather  one pass over the SURVIVING pairs: pair i of the result is read from its place in the upload and
//                     stored, termId untouched, at position i; a termId below the source's n_terms marks
//                     live[term_base[s] + termId] with a plain store of 1 (idempotent: the outcome does not depend on
//                     scheduling).  The pairs of dropped documents are never read.  A termId out of range marks nothing
//                     and is left to k_cp_remap, which reports the smallest such source as it does in a plain merge.
//   scan (§5i's)      rank[k] = live terms in front of source term k; rank[T] = how many terms stay
//   k_cp_keep_terms   the surviving terms' (start, length) in rank order - the dictionary stage's "tokens" - and the
//                     per-source base of the surviving terms; the term bytes stay where they were uploaded
//   ... k_cp_hash, k_ig_insert .. k_ig_termid, k_cp_dup over the surviving terms ...
//   k_cp_keep_map     (source, OLD term id) -> new id = newid[rank]: k_cp_remap then runs over the gathered pairs with the
//                     sources' old term bases, so the renumbering "new id = surviving terms with a smaller old id" costs
//                     no pass of its own
// Per surviving pair the filter reads 8 bytes and writes 8.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ns {

constexpr uint32_t kCpKeepTile = 1024;    // surviving pairs per workgroup of k_cp_keep_gather (four per lane)

// the last x in [lo, hi) with base[x] <= i, given base[lo] <= i < base[hi]
__device__ __forceinline__ uint32_t cp_range_of(const uint32_t* __restrict__ base, uint32_t lo, uint32_t hi, uint32_t i) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (base[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// prefix[n_docs + 1]: the surviving documents' pair prefix; srcpos[d]: first pair of surviving document d in `raw`.
// kTiled (the product): the documents and sources of a tile's first and last pair are found once per workgroup and bound
// every lane's search (a tile spans few documents).  kTiled == false searches the whole prefix for every pair: the A/B
// baseline, launched by the variants build only (NS_KEEP_FULL_SEARCH).
template <bool kTiled>
__global__ void __launch_bounds__(256) k_cp_keep_gather(const uint2* __restrict__ raw, const uint32_t* __restrict__ prefix,
                                                        const uint32_t* __restrict__ srcpos, uint32_t n_docs, uint32_t n_pairs,
                                                        const uint32_t* __restrict__ pair_base, const uint32_t* __restrict__ term_base,
                                                        uint32_t n_src, uint2* __restrict__ pairs, uint32_t* __restrict__ live) {
    __shared__ uint32_t s_bound[4];                                   // documents of the first / last pair, sources of them
    const uint32_t first = blockIdx.x * kCpKeepTile;
    const uint32_t last = min(first + kCpKeepTile, n_pairs) - 1u;     // (first < n_pairs: the grid covers n_pairs)
    if (kTiled) {
        if (threadIdx.x < 4) {
            const uint32_t i = (threadIdx.x & 1u) ? last : first;
            s_bound[threadIdx.x] = (threadIdx.x & 2u) ? cp_source_of(pair_base, n_src, i) : cp_source_of(prefix, n_docs, i);
        }
        __syncthreads();
    }
    const uint32_t d_lo = kTiled ? s_bound[0] : 0u, d_hi = kTiled ? s_bound[1] + 1u : n_docs;
    const uint32_t s_lo = kTiled ? s_bound[2] : 0u, s_hi = kTiled ? s_bound[3] + 1u : n_src;
#pragma unroll
    for (uint32_t j = 0; j < kCpKeepTile / 256; j++) {
        const uint32_t i = first + j * 256 + threadIdx.x;             // a wave's lanes: 64 neighbouring 8-byte pairs
        if (i > last) break;
        const uint32_t d = cp_range_of(prefix, d_lo, d_hi, i);
        const uint2 p = raw[srcpos[d] + (i - prefix[d])];
        pairs[i] = p;
        const uint32_t s = cp_range_of(pair_base, s_lo, s_hi, i);
        const uint32_t tb = term_base[s];
        if (p.x < term_base[s + 1] - tb) live[tb + p.x] = 1u;
    }
}

// rank: the exclusive scan of live over T + 1 entries.  Thread k < T places source term k when it stays; thread k <= n_src
// writes the per-source base of the surviving terms.
__global__ void __launch_bounds__(256) k_cp_keep_terms(const uint32_t* __restrict__ live, const uint32_t* __restrict__ rank, uint32_t T,
                                                       const uint32_t* __restrict__ kstart_in, const uint32_t* __restrict__ klen_in,
                                                       const uint32_t* __restrict__ term_base, uint32_t n_src,
                                                       uint32_t* __restrict__ kstart, uint32_t* __restrict__ klen, uint32_t* __restrict__ live_base) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k < T && live[k]) {
        const uint32_t r = rank[k];
        kstart[r] = kstart_in[k];
        klen[r] = klen_in[k];
    }
    if (k <= n_src) live_base[k] = rank[term_base[k]];
}

// map[term_base[s] + t] = new id of source s's term t as the sources numbered it; a dead term's entry is never read (no
// surviving pair names it)
__global__ void __launch_bounds__(256) k_cp_keep_map(const uint32_t* __restrict__ live, const uint32_t* __restrict__ rank, uint32_t T,
                                                     const uint32_t* __restrict__ newid, uint32_t* __restrict__ map) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= T) return;
    map[k] = live[k] ? newid[rank[k]] : 0xFFFFFFFFu;
}

}  // namespace ns
