// SPDX-License-Identifier: MIT
// A filtered copy of a segment's posting stream: ns_segment_filter keeps the postings whose document has
// its bit set in a keep-bitmap and publishes them as an ordinary segment, so that the planner and every scoring body work on
// a filter unchanged.  The passes run over the FLAT stream, chunk by chunk of 64 postings, whatever the list boundaries:
//   k_fl_mark     a wave takes 64 neighbouring postings (8 B per lane, coalesced), tests each docId's keep bit and stores the
//                 wave's 64-bit ballot as mask[chunk] and its popcount as cnt[chunk].  A docId >= n_docs is dropped, so the
//                 bits past n_docs in the bitmap's last word are never looked at.  The bitmap stays in global memory: it is
//                 n_docs / 8 bytes (125 KB for a million documents), read-only and shared by every workgroup, i.e. it lives
//                 in L2; a copy in LDS would cost every workgroup the whole bitmap for the few KB of postings it marks.
//   scan (§5i's)  base[chunk] = survivors in front of the chunk; base[n_chunks] = how many postings stay
//   k_fl_scatter  reads the postings again and their per-posting norms; survivor of lane l goes to
//                 base[chunk] + popcount(mask & lanes below l), posting and norm together (a posting's norm depends on its
//                 document alone, so the copy needs no k_pnorm pass)
//   k_fl_lists    one thread per list: [off, off + count) becomes [rank(off), rank(off + count)) with
//                 rank(x) = base[x / 64] + popcount(mask[x / 64] & bits below x % 64); no posting is read.  Compaction keeps
//                 the order, so every list stays docId-ascending.
// Per posting 8 B (mark) + 12 B (scatter) are read; per surviving posting 12 B are written.  All stores are plain stores.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ns {

constexpr uint32_t kFlChunk = 64;   // postings per chunk == lanes of a wave

// does the posting at stream position i stay?  (i < n is the caller's)
__device__ __forceinline__ bool fl_keeps(const uint32_t* __restrict__ bits, uint32_t n_docs, uint32_t doc) {
    return doc < n_docs && ((bits[doc >> 5] >> (doc & 31u)) & 1u) != 0u;
}

// mask: n_chunks + 1 words, cnt: n_chunks + 1 words (the last of each is 0: rank(n) then needs no special case)
__global__ void __launch_bounds__(256) k_fl_mark(const uint2* __restrict__ postings, uint32_t n, const uint32_t* __restrict__ bits,
                                                 uint32_t n_docs, uint64_t* __restrict__ mask, uint32_t* __restrict__ cnt) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_chunks = (n + kFlChunk - 1) / kFlChunk;
    for (uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6); c <= n_chunks; c += gridDim.x * 4u) {   // c: wave-uniform
        const uint32_t i = c * kFlChunk + lane;
        bool keep = false;
        if (c < n_chunks && i < n) keep = fl_keeps(bits, n_docs, postings[i].x);
        const uint64_t m = __ballot(keep);
        if (lane == 0) {
            mask[c] = m;
            cnt[c] = (uint32_t)__popcll(m);
        }
    }
}

// base: the exclusive scan of cnt
__global__ void __launch_bounds__(256) k_fl_scatter(const uint2* __restrict__ postings, const float* __restrict__ pnorm, uint32_t n,
                                                    const uint64_t* __restrict__ mask, const uint32_t* __restrict__ base,
                                                    uint2* __restrict__ out, float* __restrict__ pnorm_out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_chunks = (n + kFlChunk - 1) / kFlChunk;
    for (uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6); c < n_chunks; c += gridDim.x * 4u) {
        const uint64_t m = mask[c];
        if (!((m >> lane) & 1ull)) continue;                      // a set bit implies c * 64 + lane < n
        const uint32_t i = c * kFlChunk + lane;
        const uint32_t at = base[c] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        out[at] = postings[i];
        pnorm_out[at] = pnorm[i];
    }
}

// survivors in front of stream position x, 0 <= x <= n
__device__ __forceinline__ uint32_t fl_rank(const uint64_t* __restrict__ mask, const uint32_t* __restrict__ base, uint32_t x) {
    const uint32_t c = x / kFlChunk, r = x % kFlChunk;
    return base[c] + (uint32_t)__popcll(mask[c] & ((1ull << r) - 1ull));   // r == 0: the empty mask
}

__global__ void __launch_bounds__(256) k_fl_lists(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ counts, uint32_t n_lists,
                                                  const uint64_t* __restrict__ mask, const uint32_t* __restrict__ base,
                                                  uint64_t* __restrict__ new_byte_off, uint32_t* __restrict__ new_counts) {
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    if (l >= n_lists) return;
    const uint32_t a = fl_rank(mask, base, starts[l]);
    const uint32_t b = fl_rank(mask, base, starts[l] + counts[l]);
    new_byte_off[l] = (uint64_t)a * 8u;
    new_counts[l] = b - a;
}

}  // namespace ns
