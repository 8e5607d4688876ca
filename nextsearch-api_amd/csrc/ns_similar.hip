// SPDX-License-Identifier: MIT
// "More like this" on the device: for a batch of source documents the T <= 32 most telling terms of each,
// from the document's forward pairs {termId, tf} and the segment's df / idf by term id.  The rule is host/similar.hpp's:
//   a pair qualifies when tf >= min_tf, min_df <= df <= max_df, df >= 1 and 0 < idf < inf;  w = (float)tf * idf, ONE fp32
//   multiply (the library is built with -ffp-contract=off and there is nothing to contract it with);  the selection is
//   the first T pairs by key = (w bits << 32) | ~termId, descending.  w > 0, so a key is never 0: 0 is "no pair".
// No logf runs here: idf arrives from the host (glibc's value, the one search uses).
//
//   k_ml_check    upload time: one pass over the pairs, a termId >= n_terms sets a flag word next to the bounds check (as
//                 k_cp_remap reports its bad source).  Selection can then index df / idf without a check of its own.
//   k_ml_wave     one wave per listed document of at most kMlDocCut pairs, four documents per workgroup.  The pairs are
//                 read once, 64 at a time as 8-byte loads, the next chunk's load in flight while this one is worked on; the
//                 df / idf gathers are the random accesses.  The wave keeps the 64 best keys so far SORTED in its registers,
//                 one per lane.  A chunk in which no lane beats the current T-th key is skipped on a ballot; otherwise the
//                 chunk is sorted by the bitonic network of k_cp_docsort_wave (ascending), max'ed lane by lane with the
//                 kept set (descending) — the 64 largest of the 128, as a bitonic sequence — and one bitonic merge of six
//                 steps sorts that again.  A document of at most 64 pairs is one chunk.
//   k_ml_block    one workgroup per longer document: wave v takes chunks v, v + 4, ... as above, the four kept sets meet
//                 in LDS and wave 0 merges them the same way.
// No atomics; every store is a plain vector store; every index is bounded by the handle's own arrays (doc ids are checked
// on the host before the launch).
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ns {

constexpr uint32_t kMlMaxTerms = 32;      // T <= 32 (host/similar.hpp kSimilarMaxTerms)
// pairs of a document that one wave streams alone (32 chunks); longer documents get a workgroup
// (ns_docterms_doc_cut() hands it to the tests)
constexpr uint32_t kMlDocCut = 2048;

__global__ void __launch_bounds__(256) k_ml_check(const uint2* __restrict__ pairs, uint32_t n_pairs, uint32_t n_terms, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs) return;
    if (pairs[i].x >= n_terms) *bad = 1u;                              // (every writer stores the same word)
}

struct MlRule { uint32_t min_tf, min_df, max_df; };

__device__ __forceinline__ uint64_t ml_key(uint2 p, const uint32_t* __restrict__ df, const float* __restrict__ idf, MlRule r) {
    const uint32_t d = df[p.x];
    const float f = idf[p.x];
    const bool ok = p.y >= r.min_tf && d >= 1u && d >= r.min_df && d <= r.max_df && f > 0.0f && f <= 3.402823466e+38f;
    const float w = (float)p.y * f;
    return ok ? ((uint64_t)__float_as_uint(w) << 32) | (uint32_t)~p.x : 0ull;
}

__device__ __forceinline__ uint64_t ml_shfl_xor(uint64_t key, uint32_t j) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, (int)j, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), (int)j, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t ml_shfl(uint64_t key, uint32_t src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)key, (int)src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(key >> 32), (int)src, 64);
    return ((uint64_t)hi << 32) | lo;
}

// ascending over the 64 lanes
__device__ __forceinline__ uint64_t ml_sort_up(uint64_t key, uint32_t lane) {
#pragma unroll
    for (uint32_t k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint64_t other = ml_shfl_xor(key, j);
            const bool up = (lane & k) == 0, lower = (lane & j) == 0;
            key = (lower == up) ? (key < other ? key : other) : (key < other ? other : key);
        }
    }
    return key;
}
// a bitonic sequence over the 64 lanes -> descending
__device__ __forceinline__ uint64_t ml_merge_down(uint64_t key, uint32_t lane) {
#pragma unroll
    for (uint32_t j = 32; j > 0; j >>= 1) {
        const uint64_t other = ml_shfl_xor(key, j);
        key = ((lane & j) == 0) ? (key < other ? other : key) : (key < other ? key : other);
    }
    return key;
}
// kept: descending; up: ascending -> the 64 largest of both, descending
__device__ __forceinline__ uint64_t ml_join(uint64_t kept, uint64_t up, uint32_t lane) {
    return ml_merge_down(kept < up ? up : kept, lane);
}

// chunks first, first + step, ... < n_chunks of the document whose pairs are [s, s + c): the wave's 64 best keys, descending
__device__ __forceinline__ uint64_t ml_stream(const uint2* __restrict__ pairs, uint32_t s, uint32_t c, uint32_t first, uint32_t step,
                                              const uint32_t* __restrict__ df, const float* __restrict__ idf, MlRule r, uint32_t T, uint32_t lane) {
    uint64_t kept = 0;
    const uint32_t n_chunks = (c + 63u) / 64u;
    uint32_t at = first * 64u + lane;                                  // (c < 2^32 - 4096: no wrap before the bound is seen)
    uint2 nxt = make_uint2(0u, 0u);
    if (first < n_chunks && at < c) nxt = pairs[s + at];
    for (uint32_t ch = first; ch < n_chunks; ch += step) {
        const uint2 p = nxt;
        const bool live = at < c;
        at += step * 64u;
        if (ch + step < n_chunks && at < c) nxt = pairs[s + at];       // the next chunk's load goes out before this one's gathers
        const uint64_t key = live ? ml_key(p, df, idf, r) : 0ull;
        const uint64_t thr = ml_shfl(kept, T - 1u);                    // the current T-th key (0 while fewer are kept)
        if (__ballot(key > thr) == 0ull) continue;                     // (wave-uniform)
        kept = ml_join(kept, ml_sort_up(key, lane), lane);
    }
    return kept;
}

__device__ __forceinline__ void ml_store(uint64_t kept, uint32_t lane, uint32_t T, uint32_t row, uint32_t* __restrict__ term_out,
                                         uint32_t* __restrict__ w_out, uint32_t* __restrict__ count_out) {
    const unsigned long long have = __ballot(kept != 0ull && lane < T);
    if (lane < T) {
        term_out[(size_t)row * T + lane] = ~(uint32_t)kept;            // no pair: ~0u
        w_out[(size_t)row * T + lane] = (uint32_t)(kept >> 32);       // no pair: the bits of 0.0f
    }
    if (lane == 0) count_out[row] = (uint32_t)__popcll(have);
}

// list[w]: the row (position in the caller's doc_ids) this wave answers
__global__ void __launch_bounds__(256) k_ml_wave(const uint2* __restrict__ pairs, const uint32_t* __restrict__ doc_off,
                                                 const uint32_t* __restrict__ df, const float* __restrict__ idf, const uint32_t* __restrict__ doc_ids,
                                                 const uint32_t* __restrict__ list, uint32_t n_list, MlRule r, uint32_t T,
                                                 uint32_t* __restrict__ term_out, uint32_t* __restrict__ w_out, uint32_t* __restrict__ count_out) {
    const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_list) return;                                           // (wave-uniform; no barrier in this kernel)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = list[w], d = doc_ids[row], s = doc_off[d], c = doc_off[d + 1] - s;
    const uint64_t kept = ml_stream(pairs, s, c, 0u, 1u, df, idf, r, T, lane);
    ml_store(kept, lane, T, row, term_out, w_out, count_out);
}

__global__ void __launch_bounds__(256) k_ml_block(const uint2* __restrict__ pairs, const uint32_t* __restrict__ doc_off,
                                                  const uint32_t* __restrict__ df, const float* __restrict__ idf, const uint32_t* __restrict__ doc_ids,
                                                  const uint32_t* __restrict__ list, MlRule r, uint32_t T,
                                                  uint32_t* __restrict__ term_out, uint32_t* __restrict__ w_out, uint32_t* __restrict__ count_out) {
    __shared__ uint64_t s_kept[4][64];
    const uint32_t lane = threadIdx.x & 63u, v = threadIdx.x >> 6;
    const uint32_t row = list[blockIdx.x], d = doc_ids[row], s = doc_off[d], c = doc_off[d + 1] - s;
    uint64_t kept = ml_stream(pairs, s, c, v, 4u, df, idf, r, T, lane);
    s_kept[v][lane] = kept;
    __syncthreads();
    if (v != 0) return;
#pragma unroll
    for (uint32_t o = 1; o < 4; o++) kept = ml_join(kept, s_kept[o][63u - lane], lane);   // read backwards: ascending
    ml_store(kept, lane, T, row, term_out, w_out, count_out);
}

}  // namespace ns
