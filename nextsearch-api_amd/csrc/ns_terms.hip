// SPDX-License-Identifier: MIT
// Related terms on the device: for a batch of ROWS — sets of at most 255 documents of one segment — the
// T <= 64 terms that tell the set apart, from the documents' forward pairs {termId, tf} behind an ns_docterms handle and
// the segment's df / idf by term id.  The rule is host/related.hpp's:
//   fg[t] = the row's documents that hold (t, tf) with tf >= min_tf;  t qualifies when fg[t] >= min_docs,
//   min_df <= df <= max_df, df >= 1 and 0 < idf < inf;  w = (float)fg * idf, ONE fp32 multiply;  the selection is the first
//   T terms by key = (w bits << 32) | ~termId, descending.  No division and no logf run here.
//
//   k_ta_order    once per handle (ns_docterms_aggregate caches the answer): one thread per pair, a termId that does not
//                 exceed its predecessor's sets a flag word unless a document begins there (a search of the offsets, taken
//                 only at such a descent).  The counting below relies on ascending ids inside a document.
//   k_ta_count    one workgroup per row, thread j < 255 owns document j.  The term-id space is walked in windows of W ids
//                 with ONE BYTE per id in LDS: ids are unique inside a document, documents inside a row, and a row has at
//                 most 255 of them, so a byte never carries into its neighbour.  Per window each thread finds its
//                 document's slice from the cursor the last window left (gallop + bisection); a window no document
//                 reaches into is skipped on one workgroup-uniform test; otherwise the slices are streamed by groups of 16
//                 lanes with 8-byte loads and counted with LDS atomics, then the table is swept one uint32 per lane
//                 and cleared as it is read.  Byte b of a wave's 64 words is a chunk of 64 candidates: one with no counter
//                 at min_docs is skipped on a ballot before any df / idf gather, the others enter §5n's kept set exactly as
//                 ml_stream's chunks do (ml_shfl, ml_sort_up, ml_join of ns_similar.hip).  Each wave keeps its own set; the
//                 four meet in LDS as in k_ml_block and wave 0 stores the row.  fg of a stored term comes back from w: w is
//                 strictly increasing in fg while finite, so a bisection over 1..255 with the same multiply finds it; a w that
//                 overflowed to inf is recounted from the pairs.
// Every store is a plain vector store; the only atomics are the LDS byte counters (and the counting build's event
// counters).  Every global index is bounded by the handle's arrays (doc ids and offsets are checked on the host, termIds
// at upload) and every LDS index by the window.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ns {

constexpr uint32_t kTaMaxTerms = 64;          // T <= 64: one key per lane (host/related.hpp kRelatedMaxTerms)
constexpr uint32_t kTaWindowLog2 = 16;        // W = 65536 ids, a table of 64 KiB (DESIGN.md §5aa has the A/B against 2^15)

#ifdef NS_COUNT
// Counting build only: events of k_ta_count since the last reset (ns_debug_terms_counters).  0 windows skipped, 1 windows
// swept, 2 chunks skipped because no counter reached min_docs, 3 chunks skipped on the threshold ballot, 4 joins, 5 rows
// refused (counted on the host, patched in by the getter), 6 pairs dropped by min_tf, 7 rows.
constexpr int kNsTacnt = 8;
__device__ unsigned long long g_ns_tacnt[kNsTacnt];
#define NS_TACNT(i, v) do { atomicAdd(&g_ns_tacnt[(i)], (unsigned long long)(v)); } while (0)
#else
#define NS_TACNT(i, v) do { } while (0)
#endif

__global__ void __launch_bounds__(256) k_ta_order(const uint2* __restrict__ pairs, uint32_t n_pairs, const uint32_t* __restrict__ doc_off,
                                                  uint32_t n_docs, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0 || i >= n_pairs) return;
    if (pairs[i - 1].x < pairs[i].x) return;
    uint32_t lo = 0, hi = n_docs + 1;                                  // the first of doc_off[0 .. n_docs] that is >= i
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (doc_off[mid] < i) lo = mid + 1; else hi = mid;
    }
    if (lo > n_docs || doc_off[lo] != i) *bad = 1u;                    // (every writer stores the same word)
}

struct TaRule { uint32_t min_tf, min_docs, min_df, max_df; };         // min_tf and min_docs already >= 1

__device__ __forceinline__ uint64_t ta_key(uint32_t t, uint32_t fg, const uint32_t* __restrict__ df, const float* __restrict__ idf, TaRule r) {
    const uint32_t d = df[t];
    const float f = idf[t];
    const bool ok = d >= 1u && d >= r.min_df && d <= r.max_df && f > 0.0f && f <= 3.402823466e+38f;
    const float w = (float)fg * f;
    return ok ? ((uint64_t)__float_as_uint(w) << 32) | (uint32_t)~t : 0ull;
}

// docs[row_first[row] .. row_first[row + 1]): the row's distinct documents; order[]: the rows, heaviest first
template <uint32_t LOG2W>
__global__ void __launch_bounds__(256) k_ta_count(const uint2* __restrict__ pairs, const uint32_t* __restrict__ doc_off,
                                                  const uint32_t* __restrict__ df, const float* __restrict__ idf, uint32_t n_terms,
                                                  const uint32_t* __restrict__ docs, const uint32_t* __restrict__ row_first,
                                                  const uint32_t* __restrict__ order, TaRule r, uint32_t T, uint32_t* __restrict__ term_out,
                                                  uint32_t* __restrict__ docs_out, uint32_t* __restrict__ w_out, uint32_t* __restrict__ count_out) {
    constexpr uint32_t W = 1u << LOG2W, kWords = W / 4u;
    __shared__ uint32_t s_tab[kWords];
    __shared__ uint32_t s_lo[256], s_hi[256];
    __shared__ uint64_t s_kept[4][64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, v = tid >> 6;
    const uint32_t row = order[blockIdx.x];
    const uint32_t first = row_first[row];
    const uint32_t nd = min(row_first[row + 1] - first, 255u);         // (the plan's cap, once more)
    for (uint32_t i = tid; i < kWords; i += 256u) s_tab[i] = 0u;
    uint32_t cur = 0, end = 0, nxt = 0xFFFFFFFFu;                      // this thread's document: the pairs not yet counted, the next termId
    if (tid < nd) {
        const uint32_t d = docs[first + tid];
        cur = doc_off[d];
        end = doc_off[d + 1];
        if (cur < end) nxt = pairs[cur].x;
    }
    uint64_t kept = 0;
    uint32_t dropped = 0;
    (void)dropped;
    __syncthreads();
    if (tid == 0) NS_TACNT(7, 1);
    for (uint32_t base = 0; nd != 0u && base < n_terms; base += W) {   // (n_terms < 2^31: base + W does not wrap)
        const uint32_t lim = n_terms - base > W ? base + W : n_terms;
        if (!__syncthreads_or(nxt < lim)) {                            // nobody's next pair lies in the window
            if (tid == 0) NS_TACNT(0, 1);
            continue;
        }
        if (tid == 0) NS_TACNT(1, 1);
        uint32_t hi = cur;
        if (nxt < lim) {                                               // the first pair at or past lim: gallop from the cursor, then bisect
            uint32_t a = cur, b = end, step = 1;                       // pairs[a].x < lim;  b == end or pairs[b].x >= lim
            while (step < end - a) {
                if (pairs[a + step].x >= lim) { b = a + step; break; }
                a += step;
                if (step < 0x40000000u) step <<= 1;
            }
            while (b - a > 1u) {
                const uint32_t m = a + (b - a) / 2u;
                if (pairs[m].x < lim) a = m; else b = m;
            }
            hi = b;
        }
        s_lo[tid] = cur;
        s_hi[tid] = hi;
        if (hi != cur) { cur = hi; nxt = hi < end ? pairs[hi].x : 0xFFFFFFFFu; }
        __syncthreads();
        for (uint32_t j = tid >> 4; j < nd; j += 16u) {                // 16 groups of 16 lanes, a document's slice each
            const uint32_t lo = s_lo[j], h = s_hi[j];
            for (uint32_t i = lo + (tid & 15u); i < h; i += 16u) {    // (i < h <= n_pairs < 2^32 - 4096: no wrap)
                const uint2 p = pairs[i];
                const uint32_t rel = p.x - base;
                if (rel >= W) continue;                                // (never in a handle k_ta_order has passed)
                if (p.y >= r.min_tf) atomicAdd(&s_tab[rel >> 2], 1u << (8u * (rel & 3u)));
                else dropped++;
            }
        }
        __syncthreads();
        for (uint32_t blk = v; blk < kWords / 64u; blk += 4u) {        // the sweep: wave v takes words blk * 64 + lane
            const uint32_t wi = blk * 64u + lane;
            const uint32_t word = s_tab[wi];
            if (__ballot(word != 0u) == 0ull) {
                if (lane == 0) NS_TACNT(2, 4);
                continue;
            }
            s_tab[wi] = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t fg = (word >> (8u * j)) & 0xFFu, t = base + wi * 4u + j;
                const bool cand = fg >= r.min_docs && t < n_terms;
                if (__ballot(cand) == 0ull) {                          // before any df / idf gather
                    if (lane == 0) NS_TACNT(2, 1);
                    continue;
                }
                const uint64_t key = cand ? ta_key(t, fg, df, idf, r) : 0ull;
                const uint64_t thr = ml_shfl(kept, T - 1u);            // the current T-th key (0 while fewer are kept)
                if (__ballot(key > thr) == 0ull) {                     // (wave-uniform)
                    if (lane == 0) NS_TACNT(3, 1);
                    continue;
                }
                if (lane == 0) NS_TACNT(4, 1);
                kept = ml_join(kept, ml_sort_up(key, lane), lane);
            }
        }
        // (the next window's first barrier stands between these clears and its atomics)
    }
#ifdef NS_COUNT
    if (dropped) NS_TACNT(6, dropped);
#endif
    s_kept[v][lane] = kept;
    __syncthreads();
    if (v != 0) return;
#pragma unroll
    for (uint32_t o = 1; o < 4; o++) kept = ml_join(kept, s_kept[o][63u - lane], lane);   // read backwards: ascending
    const bool have = kept != 0ull && lane < T;
    uint32_t fg = 0;
    if (have) {
        const uint32_t t = ~(uint32_t)kept, wb = (uint32_t)(kept >> 32);
        if (wb != 0x7F800000u) {                                       // the least fg in 1..255 whose product reaches w
            const float f = idf[t];
            uint32_t a = 1, b = 255;
            while (a < b) {
                const uint32_t m = (a + b) / 2u;
                if (__float_as_uint((float)m * f) < wb) a = m + 1u; else b = m;
            }
            fg = a;
        } else {                                                       // w overflowed: count again, a bisection per document
            for (uint32_t j = 0; j < nd; j++) {
                const uint32_t d = docs[first + j];
                uint32_t a = doc_off[d], b = doc_off[d + 1];
                const uint32_t e = b;
                while (a < b) {
                    const uint32_t m = a + (b - a) / 2u;
                    if (pairs[m].x < t) a = m + 1u; else b = m;
                }
                if (a < e) { const uint2 p = pairs[a]; fg += (p.x == t && p.y >= r.min_tf) ? 1u : 0u; }
            }
        }
    }
    const unsigned long long n_have = __ballot(have);
    if (lane < T) {
        term_out[(size_t)row * T + lane] = ~(uint32_t)kept;            // nothing: ~0u
        docs_out[(size_t)row * T + lane] = fg;
        w_out[(size_t)row * T + lane] = (uint32_t)(kept >> 32);       // nothing: the bits of 0.0f
    }
    if (lane == 0) count_out[row] = (uint32_t)__popcll(n_have);
}

}  // namespace ns
