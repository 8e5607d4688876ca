// SPDX-License-Identifier: MIT
// Spelling correction on the device: the best L dictionary terms within a bounded edit distance of a query term, answered
// from autocomplete's sorted table (csrc/ns_suggest.hip).
//
//   candidates   the table's entries with score != 0 that do not repeat their predecessor's bytes
//   distance     optimal string alignment over bytes (Levenshtein + transposition of two adjacent bytes, no substring
//                edited twice), bounded by e = max_edits in {0, 1, 2}
//   prefix       the candidate shares its first min(prefix_len, |query|) bytes with the query: one index range [lo, hi)
//   order        distance, then score descending, then index ascending: ONE u64 key, (dist << 62) | (~score << 30) | index
//                (the table has fewer than 2^30 entries), smallest = best; the order is strict, so the answer does not
//                depend on how the work was cut
//
// Side structures (k_fz_build_*, once per table): the candidates in a LENGTH-ORDERED permutation (a counting sort by term
// length, stable in index), with a signature each: bits 0..35 = which of [0-9a-z] occur, bit 36 = some other byte occurs,
// bits 40..47 = the length.  A query of n bytes can only match lengths n - e .. n + e: one contiguous piece of the
// permutation; inside one length the permutation ascends in index, so [lo, hi) is one piece per length (k_fz_plan).
// The scan (k_fz_scan), one workgroup per (query, slice of its pieces): a lane takes a candidate and tests the signature
// (one edit moves the symmetric difference of the byte sets by at most 2); the lanes that pass are queued in LDS and the
// banded DP runs on full waves of them.  The DP's rows go over the QUERY's bytes, so its trip count is uniform whatever
// the candidates' lengths; band (2e + 1 cells), three rows and the sliding window of candidate bytes are registers with
// compile-time indices (templated on e).  Survivors better than the wave's current L-th key are appended to a per-wave
// LDS buffer that is reduced to its best L when it fills.  k_fz_select merges a query's slices.
//
// Typo-tolerant completion (k_fp_plan, k_fp_scan) is a second scan over the same structures with another
// end condition: the distance is the PREFIX distance pd(q, c) = min over j of osa(q, c[0, j)), so a candidate may be any
// length from n - e upwards (the bucket of terms past 66 bytes included: signature 0, length from the offsets), the plan
// has one piece per length bucket (FpPlan) and the signature test is one-sided (a byte class of the query that the
// candidate lacks costs an edit of its own).  DP rows, queue, keep buffer, merges and k_fz_select are the ones above.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ns {

constexpr int kFzMaxLen = 64;                  // NS_FUZZY_MAX_LEN: longer query terms never reach the device
constexpr int kFzMaxEdits = 2;
constexpr int kFzBuckets = kFzMaxLen + kFzMaxEdits + 2;   // lengths 0..66 and one bucket for everything longer (k_fp_scan only)
constexpr uint32_t kFzChunk = 4096;            // entries per wave of the build kernels
constexpr uint64_t kFzSigBits = (1ull << 37) - 1;
constexpr uint32_t kFzIdxBits = 30;
constexpr uint32_t kFzIdxMask = (1u << kFzIdxBits) - 1;
constexpr int kFzQueue = 128;                  // per wave: signature survivors waiting for the DP
constexpr int kFzKeep = 128;                   // per wave: DP survivors waiting for a reduction

#ifdef NS_COUNT
// Counting build only: events of the fuzzy kernels since the last reset (ns_debug_fuzzy_counters; tests/fuzzy_shapes.py names
// them).  0 candidates given to the signature test, 1 of those rejected, 2 DP calls on a full wave of the queue, 3 of those
// that left entries waiting, 4 DP calls on the queue's remainder, 5 DP waves that left the row loop early, 6 DP rows in which
// a lane was past the bound while another kept the wave going, 7 fz_load4 lanes that funnelled two dwords, 8 fz_load4 lanes
// whose second dword holds no byte of the term, 9 DP lanes in which the transposition lowered a cell, 10 reductions of a full
// keep buffer, 11 slices past a query's candidates, 12 queries with several slices, 13 DP lanes on the bucket past 66 bytes,
// 14 entries dropped for score 0, 15 entries dropped as repeats (both in k_fz_build_count), 16 waves of k_fz_build_scatter
// with more than one length round.
constexpr int kNsZcnt = 17;
__device__ unsigned long long g_ns_zcnt[kNsZcnt];
// one atomic per wave, by its first active lane (the DP runs with the queue's idle lanes masked off)
__device__ __forceinline__ void fz_count_wave(int i, unsigned long long v) {
    const uint64_t act = __builtin_amdgcn_ballot_w64(true);
    if (v && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(act)) atomicAdd(&g_ns_zcnt[i], v);
}
__device__ __forceinline__ void fz_count_lanes(int i, bool on) {
    fz_count_wave(i, (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(on)));
}
#endif

struct FzPlan {            // one query's pieces of the permutation, one per length n - e + t
    uint32_t start[5];
    uint32_t cum[5];       // inclusive running counts; cum[4] = the query's candidates
    uint32_t pad[2];
};

struct FpPlan {            // completion: one piece per length bucket (a bucket below n - e is empty)
    uint32_t start[kFzBuckets];
    uint32_t cum[kFzBuckets];   // inclusive running counts; cum[kFzBuckets - 1] = the query's candidates
};

struct FpPieces {          // a query's FpPlan, copied to LDS by the scanning workgroup
    const uint32_t* start;
    const uint32_t* cum;
};

__device__ __forceinline__ uint64_t fz_sig_bit(uint32_t c) {
    if (c >= '0' && c <= '9') return 1ull << (c - '0');
    if (c >= 'a' && c <= 'z') return 1ull << (10 + c - 'a');
    return 1ull << 36;
}

// Entry i: candidate or not, its length bucket and (for a length that a query can reach) its signature.
__device__ __forceinline__ bool fz_classify(uint32_t i, const uint64_t* __restrict__ heads, const uint32_t* __restrict__ offs,
                                            const uint8_t* __restrict__ pool, const uint64_t* __restrict__ keys, uint32_t& bucket,
                                            uint64_t& sig) {
    const uint32_t o = offs[i], len = offs[i + 1] - o;
    const uint64_t h = heads[i];
    bucket = len < (uint32_t)kFzBuckets - 1 ? len : (uint32_t)kFzBuckets - 1;
    sig = 0;
#ifdef NS_COUNT
    if ((uint32_t)(keys[i] >> 32) == ~0u) sig = 1;        // the reason, for k_fz_build_count (a caller ignores sig of a non-candidate)
#endif
    if ((uint32_t)(keys[i] >> 32) == ~0u) return false;   // ~score: score 0, no document carries the term
    if (i > 0) {                                           // equal to the predecessor: not the first of its run
        const uint32_t po = offs[i - 1];
        if (o - po == len && heads[i - 1] == h) {
            bool same = true;
            for (uint32_t j = 8; j < len && same; j++) same = pool[(uint64_t)po + j] == pool[(uint64_t)o + j];
#ifdef NS_COUNT
            if (same) sig = 2;
#endif
            if (same) return false;
        }
    }
    if (bucket == (uint32_t)kFzBuckets - 1) return true;
    for (uint32_t j = 0; j < len; j++) sig |= fz_sig_bit(j < 8 ? (uint32_t)(h >> (56 - 8 * j)) & 0xffu : pool[(uint64_t)o + j]);
    sig |= (uint64_t)len << 40;
    return true;
}

// ghist[bucket * n_blocks + block] = candidates of that length in the block's chunk.  One wave per chunk.
__global__ void __launch_bounds__(64) k_fz_build_count(const uint64_t* __restrict__ heads, const uint32_t* __restrict__ offs,
                                                       const uint8_t* __restrict__ pool, const uint64_t* __restrict__ keys, uint32_t n,
                                                       uint32_t* __restrict__ ghist, uint32_t n_blocks) {
    __shared__ uint32_t hist[kFzBuckets];
    const uint32_t lane = threadIdx.x;
    for (uint32_t b = lane; b < (uint32_t)kFzBuckets; b += 64) hist[b] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kFzChunk;
    for (uint32_t g = 0; g < kFzChunk; g += 64) {
        const uint64_t i = base + g + lane;
        uint32_t bucket = 0;
        uint64_t sig = 0;
        if (i < n && fz_classify((uint32_t)i, heads, offs, pool, keys, bucket, sig)) atomicAdd(&hist[bucket], 1u);
#ifdef NS_COUNT
        fz_count_lanes(14, sig == 1);   // (a candidate's signature carries its length from bit 40 up, or is 0)
        fz_count_lanes(15, sig == 2);
#endif
    }
    __syncthreads();
    for (uint32_t b = lane; b < (uint32_t)kFzBuckets; b += 64) ghist[(uint64_t)b * n_blocks + blockIdx.x] = hist[b];
}

// ghist -> exclusive running counts per length over the blocks; len_start[b] = first permutation slot of length b
// (kFzBuckets + 1 entries).  One workgroup.
__global__ void __launch_bounds__(128) k_fz_build_scan(uint32_t* __restrict__ ghist, uint32_t n_blocks, uint32_t* __restrict__ len_start) {
    __shared__ uint32_t tot[kFzBuckets];
    const uint32_t b = threadIdx.x;
    if (b < (uint32_t)kFzBuckets) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < n_blocks; k++) {
            const uint32_t t = ghist[(uint64_t)b * n_blocks + k];
            ghist[(uint64_t)b * n_blocks + k] = run;
            run += t;
        }
        tot[b] = run;
    }
    __syncthreads();
    if (b == 0) {
        uint32_t run = 0;
        for (int k = 0; k < kFzBuckets; k++) { len_start[k] = run; run += tot[k]; }
        len_start[kFzBuckets] = run;
    }
}

// The stable scatter: candidate i of length b goes to slot len_start[b] + (candidates of length b before i).
__global__ void __launch_bounds__(64) k_fz_build_scatter(const uint64_t* __restrict__ heads, const uint32_t* __restrict__ offs,
                                                         const uint8_t* __restrict__ pool, const uint64_t* __restrict__ keys, uint32_t n,
                                                         const uint32_t* __restrict__ ghist, uint32_t n_blocks,
                                                         const uint32_t* __restrict__ len_start, uint32_t* __restrict__ perm,
                                                         uint64_t* __restrict__ psig) {
    __shared__ uint32_t next[kFzBuckets];
    const uint32_t lane = threadIdx.x;
    for (uint32_t b = lane; b < (uint32_t)kFzBuckets; b += 64) next[b] = len_start[b] + ghist[(uint64_t)b * n_blocks + blockIdx.x];
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kFzChunk;
    for (uint32_t g = 0; g < kFzChunk; g += 64) {
        if (base + g >= n) break;   // uniform
        const uint64_t i = base + g + lane;
        uint32_t bucket = 0;
        uint64_t sig = 0;
        const bool cand = i < n && fz_classify((uint32_t)i, heads, offs, pool, keys, bucket, sig);
        uint64_t todo = __builtin_amdgcn_ballot_w64(cand);
#ifdef NS_COUNT
        uint32_t zc_rounds = 0;
#endif
        while (todo) {              // one round per distinct length among the wave's candidates
            const uint32_t lb = (uint32_t)__shfl((int)bucket, (int)__builtin_ctzll(todo), 64);
            const uint64_t same = __builtin_amdgcn_ballot_w64(cand && bucket == lb);
            const uint32_t at = next[lb];
            __builtin_amdgcn_wave_barrier();
            if (cand && bucket == lb) {
                const uint32_t slot = at + (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1));
                perm[slot] = (uint32_t)i;
                psig[slot] = sig;
            }
            if (lane == 0) next[lb] = at + (uint32_t)__builtin_popcountll(same);
            __builtin_amdgcn_wave_barrier();
            todo &= ~same;
#ifdef NS_COUNT
            zc_rounds++;
#endif
        }
#ifdef NS_COUNT
        fz_count_wave(16, zc_rounds > 1 ? 1 : 0);
#endif
    }
}

// One wave per query: the prefix's index range [lo, hi), then for each length of the window the slots of that length
// whose index lies in it (the permutation ascends in index inside one length).
__global__ void __launch_bounds__(256) k_fz_plan(const uint64_t* __restrict__ heads, const uint32_t* __restrict__ offs,
                                                 const uint8_t* __restrict__ pool, uint32_t n, const uint32_t* __restrict__ perm,
                                                 const uint32_t* __restrict__ len_start, const uint8_t* __restrict__ qbytes,
                                                 const uint32_t* __restrict__ qoffs, const uint8_t* __restrict__ qedits, uint32_t n_q,
                                                 uint32_t prefix_len, FzPlan* __restrict__ plans) {
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (q >= n_q) return;   // wave-uniform
    const uint8_t* p = qbytes + qoffs[q];
    const uint32_t qlen = qoffs[q + 1] - qoffs[q];
    const uint32_t e = qedits[q];
    const uint32_t plen = prefix_len < qlen ? prefix_len : qlen;
    uint32_t lo = 0, hi = n;
    if (plen) {
        const uint32_t hlen = plen < 8 ? plen : 8;
        uint64_t ph = 0;
        for (uint32_t j = 0; j < hlen; j++) ph |= (uint64_t)p[j] << (56 - 8 * j);
        ac_prefix_range(n, lane, heads, offs, pool, p, plen, ph, ~0ull << (64 - 8 * hlen), lo, hi);
    }
    uint32_t start = 0, count = 0;
    const int len = (int)qlen - (int)e + (int)lane;
    if (lane < 2 * e + 1 && len >= 0) {   // len <= 66 < kFzBuckets - 1
        const uint32_t a = len_start[len], b = len_start[len + 1];
        uint32_t x = a, y = b;             // first slot with perm >= lo
        while (x < y) { const uint32_t m = x + (y - x) / 2; if (perm[m] < lo) x = m + 1; else y = m; }
        start = x;
        y = b;                             // first slot with perm >= hi
        while (x < y) { const uint32_t m = x + (y - x) / 2; if (perm[m] < hi) x = m + 1; else y = m; }
        count = x - start;
    }
    uint32_t cum = count;
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)cum, d, 64);
        if (lane >= (uint32_t)d) cum += o;
    }
    if (lane < 5) {
        plans[q].start[lane] = start;
        plans[q].cum[lane] = cum;
    }
}

// The 4 candidate bytes c[k .. k + 4) of the term at pool[o, end): two aligned dwords, funnelled.  Bytes at or past `end`
// are whatever follows (never used by a cell that counts); a dword is only read if it holds a byte of the term.
__device__ __forceinline__ uint32_t fz_load4(const uint8_t* __restrict__ pool, uint32_t a, uint32_t end) {
    if (a >= end) return 0;
    const uint32_t* w = (const uint32_t*)(pool + (a & ~3u));
    const uint32_t sh = (a & 3u) * 8;
    const uint32_t lo = w[0];
    if (sh == 0) return lo;
#ifdef NS_COUNT
    fz_count_lanes(7, (a & ~3u) + 4 < end);
    fz_count_lanes(8, (a & ~3u) + 4 >= end);
#endif
    const uint32_t hi = (a & ~3u) + 4 < end ? w[1] : 0u;
    return (lo >> sh) | (hi << (32 - sh));
}

// Banded optimal string alignment of the query qs[0, n) (LDS, uniform) against one candidate per lane: first 8 bytes in
// `head` (big-endian), the rest at pool[o + 8, o + m).  Row i covers the cells j = i - E .. i + E; returns D[n][m], or a
// value above E once no cell of two consecutive rows is within E for any lane of the wave.
// kPrefix: returns min over j of D[n][j] instead, over the band's columns j = n - E + t that lie in [0, m].  A cell only
// depends on cells of smaller or equal j, so the cells with j <= m are exact whatever follows the term in the pool; the
// cells with j > m were computed from those bytes and are masked here, where they would be read.
template <int E, bool kPrefix = false>
__device__ __forceinline__ uint32_t fz_osa(const uint8_t* qs, uint32_t n, uint64_t head, uint32_t o, uint32_t m,
                                           const uint8_t* __restrict__ pool) {
    constexpr int B = 2 * E + 1;
    constexpr uint32_t kInf = 255;
    uint32_t p1[B], p2[B], cur[B];
#pragma unroll
    for (int t = 0; t < B; t++) {
        p1[t] = t >= E ? (uint32_t)(t - E) : kInf;
        p2[t] = kInf;
        cur[t] = kInf;
    }
    // w: the bytes c[i - E - 2 .. i + E - 1] of row i, byte s = c[i - E - 2 + s]; one byte enters per row
    uint64_t w = 0;
#pragma unroll
    for (int k = 0; k < E; k++) w = (w >> 8) | (((head >> (56 - 8 * k)) & 0xffull) << (8 * (2 * E + 1)));
    uint32_t cw = 0, qp = 0;
    bool done = true;
#ifdef NS_COUNT
    bool zc_tr = false;
#endif
    for (uint32_t i = 1; i <= n; i++) {
        const uint32_t k = i + E - 1;
        uint32_t b;
        if (k < 8) {
            b = (uint32_t)(head >> (56 - 8 * k)) & 0xffu;
        } else {
            if ((k & 3u) == 0) cw = fz_load4(pool, o + k, o + m);
            b = (cw >> (8 * (k & 3u))) & 0xffu;
        }
        w = (w >> 8) | ((uint64_t)b << (8 * (2 * E + 1)));
        const uint32_t qc = qs[i - 1];
        uint32_t before = kInf, now = kInf;
#pragma unroll
        for (int t = 0; t < B; t++) {
            const int j = (int)i + t - E;
            const uint32_t c1 = (uint32_t)(w >> (8 * (t + 1))) & 0xffu;   // c[j - 1]
            const uint32_t c2 = (uint32_t)(w >> (8 * t)) & 0xffu;         // c[j - 2]
            uint32_t v = p1[t] + (qc != c1 ? 1u : 0u);
            if (t + 1 < B) v = min(v, p1[t + 1] + 1);
            if (t >= 1) v = min(v, cur[t - 1] + 1);
#ifdef NS_COUNT
            zc_tr = zc_tr || (i >= 2 && j >= 2 && qc == c2 && qp == c1 && p2[t] + 1 < v);
#endif
            if (i >= 2 && j >= 2 && qc == c2 && qp == c1) v = min(v, p2[t] + 1);
            if (j == 0) v = i;
            if (j < 0) v = kInf;
            cur[t] = v;
            before = min(before, p1[t]);
            now = min(now, v);
        }
#pragma unroll
        for (int t = 0; t < B; t++) { p2[t] = p1[t]; p1[t] = cur[t]; }
        qp = qc;
#ifdef NS_COUNT
        if (__builtin_amdgcn_ballot_w64(min(before, now) <= (uint32_t)E)) fz_count_wave(6, __builtin_amdgcn_ballot_w64(min(before, now) > (uint32_t)E) ? 1 : 0);
        else fz_count_wave(5, i < n ? 1 : 0);
#endif
        if (!__builtin_amdgcn_ballot_w64(min(before, now) <= (uint32_t)E)) { done = i == n; break; }
    }
#ifdef NS_COUNT
    fz_count_lanes(9, zc_tr);
#endif
    uint32_t d = kInf;
    if constexpr (kPrefix) {
        const int last = (int)min(m, n + (uint32_t)E) - (int)n + E;   // the band cell of column min(m, n + E); >= 0 as m >= n - E
#pragma unroll
        for (int t = 0; t < B; t++) d = t <= last ? min(d, p1[t]) : d;   // a cell of column j < 0 holds kInf
    } else {
        const int dd = (int)m - (int)n + E;
#pragma unroll
        for (int t = 0; t < B; t++) d = dd == t ? p1[t] : d;
    }
    return done ? d : kInf;
}

// The wave's kept keys keep[0, cnt) -> their best L at keep[0, L) (kAcEmpty-padded), cnt = L; returns the L-th.
__device__ __forceinline__ uint64_t fz_reduce(uint64_t* keep, uint32_t& cnt, uint32_t lane, uint32_t L) {
    uint64_t k[kAcTop];
#pragma unroll
    for (int i = 0; i < kAcTop; i++) k[i] = kAcEmpty;
    const uint64_t a = lane < cnt ? keep[lane] : kAcEmpty, b = lane + 64 < cnt ? keep[lane + 64] : kAcEmpty;
    k[0] = a < b ? a : b;
    k[1] = a < b ? b : a;
    uint64_t best[kAcTop], worst = kAcEmpty;
#pragma unroll
    for (int i = 0; i < kAcTop; i++) best[i] = kAcEmpty;
    ac_merge(k, L, best, worst);
    __builtin_amdgcn_wave_barrier();
    if (lane < L) {
        uint64_t v = best[0];
#pragma unroll
        for (int i = 1; i < kAcTop; i++) v = lane == (uint32_t)i ? best[i] : v;
        keep[lane] = v;
    }
    __builtin_amdgcn_wave_barrier();
    cnt = L;
    return worst;
}

// The DP on one wave of queued candidates (slot < 0: idle lane), survivors appended to the wave's keep buffer.
// kPrefix: the prefix distance; a slot with signature 0 (the bucket past 66 bytes) has its length in the offsets.
template <int E, bool kPrefix = false>
__device__ __forceinline__ void fz_verify(int64_t slot, const uint8_t* qs, uint32_t n, const uint32_t* __restrict__ perm,
                                          const uint64_t* __restrict__ psig, const uint64_t* __restrict__ heads,
                                          const uint32_t* __restrict__ offs, const uint8_t* __restrict__ pool,
                                          const uint64_t* __restrict__ keys, uint64_t* keep, uint32_t& cnt, uint64_t& worst,
                                          uint32_t lane, uint32_t L) {
    uint64_t key = kAcEmpty;
    if (slot >= 0) {
        const uint32_t idx = perm[slot];
        uint32_t m = (uint32_t)(psig[slot] >> 40) & 0xffu;
        if constexpr (kPrefix) m = psig[slot] ? m : offs[idx + 1] - offs[idx];
#ifdef NS_COUNT
        if constexpr (kPrefix) fz_count_lanes(13, psig[slot] == 0);
#endif
        const uint32_t o = m > 8 ? offs[idx] : 0u;
        const uint32_t d = fz_osa<E, kPrefix>(qs, n, heads[idx], o, m, pool);
        if (d <= (uint32_t)E) key = ((uint64_t)d << 62) | ((keys[idx] >> 32) << kFzIdxBits) | idx;
    }
    const bool take = key < worst;   // kAcEmpty is never below worst
    const uint64_t bal = __builtin_amdgcn_ballot_w64(take);
    if (!bal) return;
    const uint32_t add = (uint32_t)__builtin_popcountll(bal);
#ifdef NS_COUNT
    fz_count_wave(10, cnt + add > (uint32_t)kFzKeep ? 1 : 0);
#endif
    if (cnt + add > (uint32_t)kFzKeep) worst = fz_reduce(keep, cnt, lane, L);   // cnt = L <= 10 afterwards: 64 more fit
    if (take) keep[cnt + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1))] = key;
    __builtin_amdgcn_wave_barrier();
    cnt += add;
}

// x -> the slot of position x of a query's candidates: the piece with cum[t - 1] <= x < cum[t] (x below the last cum)
__device__ __forceinline__ uint32_t fp_slot(const FpPieces& pl, uint32_t x) {
    uint32_t a = 0, b = (uint32_t)kFzBuckets - 1;   // the first t with x < cum[t]
    while (a < b) {
        const uint32_t t = (a + b) / 2;
        if (x < pl.cum[t]) b = t; else a = t + 1;
    }
    return pl.start[a] + (x - (a ? pl.cum[a - 1] : 0u));
}

// Positions [p0, p1) of a query's candidates, dealt to the workgroup's four waves 64 at a time.  kPrefix (Plan =
// FpPieces): completion's pieces, signature test and distance.
template <int E, bool kPrefix = false, class Plan>
__device__ __forceinline__ void fz_scan_body(const Plan& pl, uint64_t p0, uint64_t p1, uint64_t qsig, const uint8_t* qs, uint32_t n,
                                             const uint32_t* __restrict__ perm, const uint64_t* __restrict__ psig,
                                             const uint64_t* __restrict__ heads, const uint32_t* __restrict__ offs,
                                             const uint8_t* __restrict__ pool, const uint64_t* __restrict__ keys, uint32_t* queue,
                                             uint64_t* keep, uint32_t& cnt, uint64_t& worst, uint32_t wave, uint32_t lane, uint32_t L,
                                             bool use_sig) {
    uint32_t queued = 0;
    for (uint64_t base = p0 + wave * 64; base < p1; base += 256) {   // wave-uniform
        const uint64_t p = base + lane;
        bool pass = false;
        uint32_t slot = 0;
        if (p < p1) {
            const uint32_t x = (uint32_t)p;
            // the piece that holds position x of the query's candidates
            if constexpr (kPrefix) {
                slot = fp_slot(pl, x);
                const uint64_t cs = psig[slot];   // 0: the bucket past 66 bytes, which has no byte set
                pass = !use_sig || cs == 0 || __builtin_popcountll(qsig & ~cs & kFzSigBits) <= E;
            } else {
                slot = pl.start[0] + x;
#pragma unroll
                for (int t = 1; t < 2 * E + 1; t++) slot = x >= pl.cum[t - 1] ? pl.start[t] + (x - pl.cum[t - 1]) : slot;
                pass = !use_sig || __builtin_popcountll((psig[slot] ^ qsig) & kFzSigBits) <= 2 * E;
            }
        }
#ifdef NS_COUNT
        fz_count_lanes(0, p < p1);
        fz_count_lanes(1, p < p1 && !pass);
#endif
        const uint64_t bal = __builtin_amdgcn_ballot_w64(pass);
        if (pass) queue[queued + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1))] = slot;
        __builtin_amdgcn_wave_barrier();
        queued += (uint32_t)__builtin_popcountll(bal);
        if (queued >= 64) {   // a full wave of work for the DP, taken from the top
            queued -= 64;
#ifdef NS_COUNT
            fz_count_wave(2, 1);
            fz_count_wave(3, queued ? 1 : 0);
#endif
            const uint32_t s = queue[queued + lane];
            __builtin_amdgcn_wave_barrier();
            fz_verify<E, kPrefix>((int64_t)s, qs, n, perm, psig, heads, offs, pool, keys, keep, cnt, worst, lane, L);
        }
    }
    if (queued) {
#ifdef NS_COUNT
        fz_count_wave(4, 1);
#endif
        const int64_t s = lane < queued ? (int64_t)queue[lane] : -1;
        __builtin_amdgcn_wave_barrier();
        fz_verify<E, kPrefix>(s, qs, n, perm, psig, heads, offs, pool, keys, keep, cnt, worst, lane, L);
    }
}

// The end of a slice: each wave's keep buffer reduced to its best L, the four lists merged by wave 0 into part[b * kAcTop ..].
// k_fp_scan's; k_fz_scan keeps the same lines in its own body (calling this from there reorders a few of its scalar
// instructions, and that kernel stays the code object it was).
__device__ __forceinline__ void fz_finish_slice(uint64_t (*keep_all)[kFzKeep], uint64_t* keep, uint32_t& cnt, uint32_t wave, uint32_t lane,
                                                uint32_t L, uint32_t b, uint64_t* __restrict__ part) {
    fz_reduce(keep, cnt, lane, L);   // keep[0, L): the wave's best
    __syncthreads();
    if (wave == 0) {                 // the four waves' lists, one per lane
        uint64_t k[kAcTop];
#pragma unroll
        for (int i = 0; i < kAcTop; i++) k[i] = (lane < 4 && (uint32_t)i < L) ? keep_all[lane][i] : kAcEmpty;
        uint64_t best[kAcTop], w2 = kAcEmpty;
#pragma unroll
        for (int i = 0; i < kAcTop; i++) best[i] = kAcEmpty;
        ac_merge(k, L, best, w2);
        if (lane < (uint32_t)kAcTop) {
            uint64_t v = best[0];
#pragma unroll
            for (int i = 1; i < kAcTop; i++) v = lane == (uint32_t)i ? best[i] : v;
            part[(uint64_t)b * kAcTop + lane] = v;
        }
    }
}

// One workgroup per (query, slice): positions [s * slice, (s + 1) * slice) of the query's candidates.  Workgroup b belongs
// to the query q with slice_base[q] <= b < slice_base[q + 1] (the host sizes a query's slices from the length window
// alone; the slices that the prefix range leaves empty return at once).  part[b * kAcTop ..]: the slice's best L keys.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4)))
k_fz_scan(const uint64_t* __restrict__ heads, const uint32_t* __restrict__ offs, const uint8_t* __restrict__ pool,
          const uint64_t* __restrict__ keys, const uint32_t* __restrict__ perm, const uint64_t* __restrict__ psig,
          const uint8_t* __restrict__ qbytes, const uint32_t* __restrict__ qoffs, const uint8_t* __restrict__ qedits,
          const uint64_t* __restrict__ qsigs, const uint32_t* __restrict__ slice_base, uint32_t n_q, uint32_t slice,
          const FzPlan* __restrict__ plans, uint32_t L, uint32_t use_sig, uint64_t* __restrict__ part) {
    __shared__ uint8_t qs[kFzMaxLen];
    __shared__ uint32_t queue_all[4][kFzQueue];
    __shared__ uint64_t keep_all[4][kFzKeep];
    const uint32_t b = blockIdx.x;
    uint32_t q = 0, hi = n_q;   // the last q with slice_base[q] <= b
    while (hi - q > 1) {
        const uint32_t m = q + (hi - q) / 2;
        if (slice_base[m] <= b) q = m; else hi = m;
    }
    const FzPlan pl = plans[q];
    const uint64_t p0 = (uint64_t)(b - slice_base[q]) * slice;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (p0 >= pl.cum[4]) {   // uniform: nothing of the query falls into this slice
#ifdef NS_COUNT
        if (threadIdx.x == 0) atomicAdd(&g_ns_zcnt[11], 1ull);
#endif
        if (threadIdx.x < (uint32_t)kAcTop) part[(uint64_t)b * kAcTop + threadIdx.x] = kAcEmpty;
        return;
    }
    const uint64_t p1 = p0 + slice < pl.cum[4] ? p0 + slice : (uint64_t)pl.cum[4];
    const uint32_t qo = qoffs[q], n = qoffs[q + 1] - qo, e = qedits[q];
    if (threadIdx.x < n) qs[threadIdx.x] = qbytes[qo + threadIdx.x];
    __syncthreads();
    const uint64_t qsig = qsigs[q];
    uint32_t cnt = 0;
    uint64_t worst = kAcEmpty;
    uint32_t* queue = queue_all[wave];
    uint64_t* keep = keep_all[wave];
    if (e == 0) fz_scan_body<0>(pl, p0, p1, qsig, qs, n, perm, psig, heads, offs, pool, keys, queue, keep, cnt, worst, wave, lane, L, use_sig != 0);
    else if (e == 1) fz_scan_body<1>(pl, p0, p1, qsig, qs, n, perm, psig, heads, offs, pool, keys, queue, keep, cnt, worst, wave, lane, L, use_sig != 0);
    else fz_scan_body<2>(pl, p0, p1, qsig, qs, n, perm, psig, heads, offs, pool, keys, queue, keep, cnt, worst, wave, lane, L, use_sig != 0);
    fz_reduce(keep, cnt, lane, L);   // keep[0, L): the wave's best
    __syncthreads();
    if (wave == 0) {                 // the four waves' lists, one per lane
        uint64_t k[kAcTop];
#pragma unroll
        for (int i = 0; i < kAcTop; i++) k[i] = (lane < 4 && (uint32_t)i < L) ? keep_all[lane][i] : kAcEmpty;
        uint64_t best[kAcTop], w2 = kAcEmpty;
#pragma unroll
        for (int i = 0; i < kAcTop; i++) best[i] = kAcEmpty;
        ac_merge(k, L, best, w2);
        if (lane < (uint32_t)kAcTop) {
            uint64_t v = best[0];
#pragma unroll
            for (int i = 1; i < kAcTop; i++) v = lane == (uint32_t)i ? best[i] : v;
            part[(uint64_t)b * kAcTop + lane] = v;
        }
    }
}

// Completion's plan.  One wave per query: the fixed prefix's index range [lo, hi), then for every length bucket from
// n - e upwards (the one past 66 bytes included) the slots of that bucket whose index lies in it.  Lane l has the buckets
// 2l and 2l + 1.
__global__ void __launch_bounds__(256) k_fp_plan(const uint64_t* __restrict__ heads, const uint32_t* __restrict__ offs,
                                                 const uint8_t* __restrict__ pool, uint32_t n, const uint32_t* __restrict__ perm,
                                                 const uint32_t* __restrict__ len_start, const uint8_t* __restrict__ qbytes,
                                                 const uint32_t* __restrict__ qoffs, const uint8_t* __restrict__ qedits, uint32_t n_q,
                                                 uint32_t prefix_len, FpPlan* __restrict__ plans) {
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (q >= n_q) return;   // wave-uniform
    const uint8_t* p = qbytes + qoffs[q];
    const uint32_t qlen = qoffs[q + 1] - qoffs[q];
    const uint32_t e = qedits[q];
    const uint32_t plen = prefix_len < qlen ? prefix_len : qlen;
    uint32_t lo = 0, hi = n;
    if (plen) {
        const uint32_t hlen = plen < 8 ? plen : 8;
        uint64_t ph = 0;
        for (uint32_t j = 0; j < hlen; j++) ph |= (uint64_t)p[j] << (56 - 8 * j);
        ac_prefix_range(n, lane, heads, offs, pool, p, plen, ph, ~0ull << (64 - 8 * hlen), lo, hi);
    }
    const uint32_t first = qlen > e ? qlen - e : 0u;   // the shortest candidate
    uint32_t start[2] = {0, 0}, count[2] = {0, 0};
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint32_t bk = 2 * lane + h;
        if (bk < (uint32_t)kFzBuckets && bk >= first) {
            const uint32_t a = len_start[bk], b = len_start[bk + 1];
            uint32_t x = a, y = b;             // first slot with perm >= lo
            while (x < y) { const uint32_t m = x + (y - x) / 2; if (perm[m] < lo) x = m + 1; else y = m; }
            start[h] = x;
            y = b;                             // first slot with perm >= hi
            while (x < y) { const uint32_t m = x + (y - x) / 2; if (perm[m] < hi) x = m + 1; else y = m; }
            count[h] = x - start[h];
        }
    }
    uint32_t cum = count[0] + count[1];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)cum, d, 64);
        if (lane >= (uint32_t)d) cum += o;
    }
    if (2 * lane + 1 < (uint32_t)kFzBuckets) {   // kFzBuckets is even
        plans[q].start[2 * lane] = start[0];
        plans[q].start[2 * lane + 1] = start[1];
        plans[q].cum[2 * lane] = cum - count[1];
        plans[q].cum[2 * lane + 1] = cum;
    }
}

// hist[b] += the candidates whose first byte is b (a candidate of 0 bytes counts under 0); hist has 256 zeroed entries.  Once per
// table: with a fixed prefix the host sizes a query's slices from min(length window, candidates that start with its first byte).
__global__ void __launch_bounds__(256) k_fp_first_bytes(const uint64_t* __restrict__ heads, const uint32_t* __restrict__ perm, uint32_t cands,
                                                        uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < cands; s += (uint64_t)gridDim.x * 256)
        atomicAdd(&h[(uint32_t)(heads[perm[s]] >> 56)], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// Completion's scan: k_fz_scan with the plan of k_fp_plan in LDS.  How a query's slices were sized (slice_base) decides
// nothing but the work's cut: a slice past the query's candidates returns at once.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4)))
k_fp_scan(const uint64_t* __restrict__ heads, const uint32_t* __restrict__ offs, const uint8_t* __restrict__ pool,
          const uint64_t* __restrict__ keys, const uint32_t* __restrict__ perm, const uint64_t* __restrict__ psig,
          const uint8_t* __restrict__ qbytes, const uint32_t* __restrict__ qoffs, const uint8_t* __restrict__ qedits,
          const uint64_t* __restrict__ qsigs, const uint32_t* __restrict__ slice_base, uint32_t n_q, uint32_t slice,
          const FpPlan* __restrict__ plans, uint32_t L, uint32_t use_sig, uint64_t* __restrict__ part) {
    __shared__ uint8_t qs[kFzMaxLen];
    __shared__ uint32_t pstart[kFzBuckets], pcum[kFzBuckets];
    __shared__ uint32_t queue_all[4][kFzQueue];
    __shared__ uint64_t keep_all[4][kFzKeep];
    const uint32_t b = blockIdx.x;
    uint32_t q = 0, hi = n_q;   // the last q with slice_base[q] <= b
    while (hi - q > 1) {
        const uint32_t m = q + (hi - q) / 2;
        if (slice_base[m] <= b) q = m; else hi = m;
    }
    const uint32_t total = plans[q].cum[kFzBuckets - 1];
    const uint64_t p0 = (uint64_t)(b - slice_base[q]) * slice;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (p0 >= total) {   // uniform: nothing of the query falls into this slice
#ifdef NS_COUNT
        if (threadIdx.x == 0) atomicAdd(&g_ns_zcnt[11], 1ull);
#endif
        if (threadIdx.x < (uint32_t)kAcTop) part[(uint64_t)b * kAcTop + threadIdx.x] = kAcEmpty;
        return;
    }
    const uint64_t p1 = p0 + slice < total ? p0 + slice : (uint64_t)total;
    const uint32_t qo = qoffs[q], n = qoffs[q + 1] - qo, e = qedits[q];
    if (threadIdx.x < n) qs[threadIdx.x] = qbytes[qo + threadIdx.x];
    if (threadIdx.x < (uint32_t)kFzBuckets) {
        pstart[threadIdx.x] = plans[q].start[threadIdx.x];
        pcum[threadIdx.x] = plans[q].cum[threadIdx.x];
    }
    __syncthreads();
    const FpPieces pl{pstart, pcum};
    const uint64_t qsig = qsigs[q];
    uint32_t cnt = 0;
    uint64_t worst = kAcEmpty;
    uint32_t* queue = queue_all[wave];
    uint64_t* keep = keep_all[wave];
    if (e == 0) fz_scan_body<0, true>(pl, p0, p1, qsig, qs, n, perm, psig, heads, offs, pool, keys, queue, keep, cnt, worst, wave, lane, L, use_sig != 0);
    else if (e == 1) fz_scan_body<1, true>(pl, p0, p1, qsig, qs, n, perm, psig, heads, offs, pool, keys, queue, keep, cnt, worst, wave, lane, L, use_sig != 0);
    else fz_scan_body<2, true>(pl, p0, p1, qsig, qs, n, perm, psig, heads, offs, pool, keys, queue, keep, cnt, worst, wave, lane, L, use_sig != 0);
    fz_finish_slice(keep_all, keep, cnt, wave, lane, L, b, part);
}

// One wave per query: the best L over its slices' lists.
__global__ void __launch_bounds__(256) k_fz_select(const uint64_t* __restrict__ part, const uint32_t* __restrict__ slice_base, uint32_t n_q,
                                                   uint32_t L, uint32_t* __restrict__ idx_out, uint8_t* __restrict__ dist_out,
                                                   uint32_t* __restrict__ count_out) {
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (q >= n_q) return;   // wave-uniform
#ifdef NS_COUNT
    fz_count_wave(12, slice_base[q + 1] - slice_base[q] > 1 ? 1 : 0);
#endif
    uint64_t best[kAcTop], worst = kAcEmpty;
#pragma unroll
    for (int i = 0; i < kAcTop; i++) best[i] = kAcEmpty;
    ac_offer(part, kAcTop, L, slice_base[q], slice_base[q + 1], lane, L, best, worst);
    if (lane < L) {
        uint64_t v = best[0];
#pragma unroll
        for (int i = 1; i < kAcTop; i++) v = lane == (uint32_t)i ? best[i] : v;
        idx_out[(uint64_t)q * L + lane] = v == kAcEmpty ? ~0u : (uint32_t)v & kFzIdxMask;
        dist_out[(uint64_t)q * L + lane] = v == kAcEmpty ? (uint8_t)0xff : (uint8_t)(v >> 62);
    }
    if (lane == 0) {
        uint32_t cnt = 0;
#pragma unroll
        for (int i = 0; i < kAcTop; i++) cnt += ((uint32_t)i < L && best[i] != kAcEmpty) ? 1u : 0u;
        count_out[q] = cnt;
    }
}

}  // namespace ns
