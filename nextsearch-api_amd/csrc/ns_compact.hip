// SPDX-License-Identifier: MIT
// Compaction on the device: the forward indexes of several segments -> the forward index of ONE segment,
// the step in front of ns_forward_invert.  Nothing is tokenised again: a source hands over its documents' {termId, tf}
// pairs and its term list, and the merge is §5i's dictionary stage run over term STRINGS instead of tokens.
//
// Over the sources' term bytes back to back (the "text", < 4 GiB - 64 KiB) with one "token" per source term:
//   k_cp_hash         per source term: its source (binary search in the per-source term prefix) and §5i's 64-bit polynomial
//                     hash; terms longer than kIgLong bytes go to k_ig_hash_long as they do in §5i
//   k_ig_insert, k_ig_first, scan, k_ig_termid, k_ig_term_bytes   unchanged: the smallest token index of a term is its first
//                     occurrence in the walk "sources in order, each term list in its own id order"; the rank of that
//                     occurrence is the new term id; k_ig_termid's token -> term id array IS the (source, old id) -> new id map
//   k_cp_dup          a second table keyed by (source, new id): two terms of ONE source with the same bytes meet in one slot;
//                     the smallest such source is reported (a minimum: independent of arrival order)
//   k_cp_remap        one pass over all pairs: source of a pair from the per-source pair prefix, termId through the map;
//                     a termId >= the source's n_terms is reported the same way and leaves the pair alone
//   k_cp_docsort_*    the pairs are grouped by document already; only the order inside a document is wrong.  Documents of at
//                     most 64 pairs are sorted in one wave's registers, documents of at most kCpDocCut pairs in LDS by a
//                     workgroup each, both in place: one read and one write of the pairs.  Longer documents go through
//                     the global radix sort (k_cp_big_gather -> by term id -> k_cp_big_rekey -> by document ->
//                     k_cp_big_scatter), as §5i's sort 1 + sort 2 do for every pair.
//
// Term ids inside a document are distinct after the remap (duplicates were refused), so a pair's 64-bit value
// termId << 32 | tf is a unique key, stability does not matter and every correct sorting network gives the same bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ns_index_consts.hpp"   // kCpWaveMax, kCpDocCut
#include "ns_ingest_text.hpp"

namespace ns {

constexpr uint64_t kCpPad = ~0ull;        // sorts behind every pair (termId 0xFFFFFFFF is refused: it is >= n_terms)

// the last s with base[s] <= i (base has n_src + 1 entries; empty sources share their base with the next one)
__device__ __forceinline__ uint32_t cp_source_of(const uint32_t* __restrict__ base, uint32_t n_src, uint32_t i) {
    uint32_t lo = 0, hi = n_src;                                      // base[lo] <= i < base[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (base[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) k_cp_hash(const uint8_t* __restrict__ text, const uint32_t* __restrict__ kstart,
                                                 const uint32_t* __restrict__ klen, uint32_t n_tok, const uint32_t* __restrict__ term_base,
                                                 uint32_t n_src, uint64_t hash_mask, uint32_t* __restrict__ ksrc, uint64_t* __restrict__ khash,
                                                 uint32_t* __restrict__ long_list, uint32_t* __restrict__ long_count) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_tok) return;
    ksrc[k] = cp_source_of(term_base, n_src, k);
    const uint32_t s = kstart[k], len = klen[k];
    if (len > kIgLong) {
        long_list[atomicAdd(long_count, 1u)] = k;                     // (the list's order is never read: each entry writes its own khash)
        return;
    }
    khash[k] = ig_hash_bytes(text + s, len) & hash_mask;
}

// table: `mask + 1` slots of (source << 32 | new id), at least twice the source terms; *dup_src = the smallest source that
// holds one byte string twice (0xFFFFFFFF: none)
__global__ void __launch_bounds__(256) k_cp_dup(const uint32_t* __restrict__ newid, const uint32_t* __restrict__ ksrc, uint32_t n_tok,
                                                unsigned long long* __restrict__ table, uint32_t mask, uint32_t* __restrict__ dup_src) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_tok) return;
    const uint32_t src = ksrc[k];
    const unsigned long long key = ((unsigned long long)src << 32) | newid[k];
    uint32_t slot = (uint32_t)(ig_mix(key) & mask);
    for (;;) {
        const unsigned long long cur = atomicCAS(&table[slot], (unsigned long long)kCpPad, key);
        if (cur == (unsigned long long)kCpPad) return;
        if (cur == key) { atomicMin(dup_src, src); return; }
        slot = (slot + 1u) & mask;
    }
}

// in place; map[term_base[s] + t] = new id of source s's term t; *bad_src = the smallest source with a termId >= its n_terms
__global__ void __launch_bounds__(256) k_cp_remap(uint2* __restrict__ pairs, uint32_t n_pairs, const uint32_t* __restrict__ pair_base,
                                                  const uint32_t* __restrict__ term_base, uint32_t n_src, const uint32_t* __restrict__ map,
                                                  uint32_t* __restrict__ bad_src) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs) return;
    const uint32_t s = cp_source_of(pair_base, n_src, i);
    const uint2 p = pairs[i];
    const uint32_t tb = term_base[s];
    if (p.x >= term_base[s + 1] - tb) { atomicMin(bad_src, s); return; }
    pairs[i] = make_uint2(map[tb + p.x], p.y);
}

__device__ __forceinline__ uint64_t cp_key(uint2 p) { return ((uint64_t)p.x << 32) | p.y; }
__device__ __forceinline__ uint2 cp_pair(uint64_t k) { return make_uint2((uint32_t)(k >> 32), (uint32_t)k); }

// One wave per document of 2 .. 64 pairs (four documents per workgroup): a pair per lane, bitonic network over the lanes.
// The whole document is in registers before the first store, so the sort is in place.
__global__ void __launch_bounds__(256) k_cp_docsort_wave(uint2* __restrict__ pairs, const uint32_t* __restrict__ doc_prefix,
                                                         const uint32_t* __restrict__ list, uint32_t n_list) {
    const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_list) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t d = list[w], s = doc_prefix[d], c = doc_prefix[d + 1] - s;   // c <= 64
    uint64_t key = lane < c ? cp_key(pairs[s + lane]) : kCpPad;
    // the network only has to be as wide as the document: lanes >= width hold padding that already sorts last
    uint32_t width = 2;
    while (width < c) width <<= 1;
#pragma unroll
    for (uint32_t k = 2; k <= 64; k <<= 1) {
        if (k > width) break;                                         // (wave-uniform)
#pragma unroll
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, (int)j, 64);
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), (int)j, 64);
            const uint64_t other = ((uint64_t)hi << 32) | lo;
            const bool up = (lane & k) == 0, lower = (lane & j) == 0;
            key = (lower == up) ? (key < other ? key : other) : (key < other ? other : key);
        }
    }
    if (lane < c) pairs[s + lane] = cp_pair(key);
}

// One workgroup per document of 65 .. kCpDocCut pairs: bitonic sort of the 64-bit keys in LDS, padded to a power of two.
// Compare-exchange t of a step works on elements i and i | j with i = t with a zero bit inserted at j's position: for
// j >= 32 neighbouring lanes touch neighbouring 8-byte words (no bank conflict), below that a wave's accesses fold onto
// half the banks.
__global__ void __launch_bounds__(256) k_cp_docsort_lds(uint2* __restrict__ pairs, const uint32_t* __restrict__ doc_prefix,
                                                        const uint32_t* __restrict__ list) {
    __shared__ uint64_t s_key[kCpDocCut];
    const uint32_t d = list[blockIdx.x], s = doc_prefix[d], c = doc_prefix[d + 1] - s;   // 64 < c <= kCpDocCut
    uint32_t n2 = 128;
    while (n2 < c) n2 <<= 1;                                           // <= kCpDocCut (a power of two itself)
    for (uint32_t i = threadIdx.x; i < n2; i += 256) s_key[i] = i < c ? cp_key(pairs[s + i]) : kCpPad;
    __syncthreads();
    for (uint32_t k = 2; k <= n2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < n2 / 2; t += 256) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), p = i | j;
                const uint64_t a = s_key[i], b = s_key[p];
                if ((a > b) == ((i & k) == 0)) { s_key[i] = b; s_key[p] = a; }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < c; i += 256) pairs[s + i] = cp_pair(s_key[i]);
}

// ---- documents beyond the cut (and every document when the in-place kernels are switched off): the global radix sort ----
// big_prefix[L] = pairs of the listed documents in front of the L-th one (n_list + 1 entries); item q of the gathered array is
// pair q - big_prefix[L] of document list[L].
__global__ void __launch_bounds__(256) k_cp_big_gather(const uint2* __restrict__ pairs, const uint32_t* __restrict__ doc_prefix,
                                                       const uint32_t* __restrict__ list, const uint32_t* __restrict__ big_prefix, uint32_t n_list,
                                                       uint32_t n_big, uint32_t* __restrict__ keys, uint2* __restrict__ vals) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_big) return;
    const uint32_t L = cp_source_of(big_prefix, n_list, q);
    const uint2 p = pairs[doc_prefix[list[L]] + (q - big_prefix[L])];
    keys[q] = p.x;
    vals[q] = make_uint2(L, p.y);
}
// after the sort by term id: key = the document's place in the list, value = {termId, tf}
__global__ void __launch_bounds__(256) k_cp_big_rekey(const uint32_t* __restrict__ keys_in, const uint2* __restrict__ vals_in, uint32_t n_big,
                                                      uint32_t* __restrict__ keys_out, uint2* __restrict__ vals_out) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_big) return;
    const uint2 v = vals_in[q];
    keys_out[q] = v.x;
    vals_out[q] = make_uint2(keys_in[q], v.y);
}
// after the stable sort by document: item q lies in its document's range again, term ids ascending
__global__ void __launch_bounds__(256) k_cp_big_scatter(const uint32_t* __restrict__ keys, const uint2* __restrict__ vals, uint32_t n_big,
                                                        const uint32_t* __restrict__ doc_prefix, const uint32_t* __restrict__ list,
                                                        const uint32_t* __restrict__ big_prefix, uint2* __restrict__ pairs) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_big) return;
    const uint32_t L = keys[q];
    pairs[doc_prefix[list[L]] + (q - big_prefix[L])] = vals[q];
}

}  // namespace ns
