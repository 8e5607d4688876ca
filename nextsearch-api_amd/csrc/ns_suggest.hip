// SPDX-License-Identifier: MIT
// Autocomplete on the device: the reference's AutocompleteIndex (src/api_autocomplete.cpp) answered from a sorted
// dictionary instead of a trie.
//
// The terms are sorted by their bytes, so the terms that start with a prefix are ONE index range [lo, hi), and inside
// the dictionary "term ascending" is "index ascending".  A term's ranking key is the u64 (~score << 32) | index: the
// smallest key is the best suggestion (score descending, then term ascending), exactly the trie's order.  A request is
//   1. lo / hi by a 64-ary search (each lane compares one pivot, a ballot narrows the range 64x per round), on the
//      terms' first 8 bytes packed big-endian (one load), with the term pool read only for prefixes longer than 8 bytes;
//   2. the L smallest keys of [lo, hi) from a range top-10 tree: level 0 holds the 10 smallest keys of every block of 64
//      terms, level j the 10 smallest of every 64 nodes of level j - 1 (~0 = empty slot).  The range splits into at most
//      two partial blocks of raw terms plus at most 63 whole nodes per side per level, so the work per request is bounded
//      whatever the range's size.
// Lists (a node's sorted keys, or one raw term's key) are merged in chunks of 63, one list per lane; lane 63 carries the
// best keys found so far.  A merge is L rounds of a wave-wide minimum: the lane that holds it shifts its list by one.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ns {

constexpr int kAcTop = 10;          // keys per tree node (the reference's max_top_, src/api_engine.cpp:104)
constexpr int kAcFan = 64;          // terms per level-0 block, nodes per parent
constexpr int kAcMaxLevels = 6;     // 64^6 > 2^32 terms
constexpr uint64_t kAcEmpty = ~0ull;

struct AcLevels {
    uint64_t off[kAcMaxLevels];     // first key of level j inside the tree array
    uint32_t nodes[kAcMaxLevels];
    uint32_t n_levels;              // the top level has <= 64 nodes
};

__device__ __forceinline__ uint64_t ac_wave_min(uint64_t k) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = __shfl_xor(k, d, 64);
        k = o < k ? o : k;
    }
    return k;
}

// One merge: every lane holds a sorted list k[0..10) (kAcEmpty-padded).  The L smallest keys over all lanes go to
// best[0..L) (uniform); `worst` = best[L - 1].  Keys are unique across lanes except kAcEmpty, which is never taken twice
// usefully (a lane whose head is kAcEmpty shifts kAcEmpty in).
__device__ __forceinline__ void ac_merge(uint64_t (&k)[kAcTop], uint32_t L, uint64_t (&best)[kAcTop], uint64_t& worst) {
#pragma unroll
    for (int r = 0; r < kAcTop; r++) {
        if ((uint32_t)r >= L) break;
        const uint64_t m = ac_wave_min(k[0]);
        best[r] = m;
        worst = m;
        if (k[0] == m) {
#pragma unroll
            for (int i = 0; i + 1 < kAcTop; i++) k[i] = k[i + 1];
            k[kAcTop - 1] = kAcEmpty;
        }
    }
}

// Builds one tree level: node = 64 children (level 0: raw keys, stride 1, one key each; level j: nodes of level j - 1,
// stride 10, ten keys each) -> its 10 smallest keys.  One wave per node.
__global__ void __launch_bounds__(256) k_ac_build(const uint64_t* __restrict__ src, uint32_t n_src, uint32_t stride, uint32_t len,
                                                  uint64_t* __restrict__ dst, uint32_t n_nodes) {
    const uint32_t node = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (node >= n_nodes) return;   // wave-uniform
    const uint64_t child = (uint64_t)node * kAcFan + lane;
    uint64_t k[kAcTop];
#pragma unroll
    for (int i = 0; i < kAcTop; i++) k[i] = (child < n_src && (uint32_t)i < len) ? src[child * stride + i] : kAcEmpty;
    uint64_t best[kAcTop], worst = kAcEmpty;
    ac_merge(k, kAcTop, best, worst);
    if (lane < (uint32_t)kAcTop) {
        uint64_t v = best[0];
#pragma unroll
        for (int i = 1; i < kAcTop; i++) v = lane == (uint32_t)i ? best[i] : v;
        dst[(uint64_t)node * kAcTop + lane] = v;
    }
}

// c(i): the sign of compare(term_i truncated to |p| bytes, p) — -1, 0 (term_i starts with p), +1.  Monotone over the
// sorted dictionary.  ph / mask: p's first min(|p|, 8) bytes, big-endian, and the mask of those bytes.
__device__ __forceinline__ int ac_cmp(uint32_t i, const uint64_t* __restrict__ heads, const uint32_t* __restrict__ offs,
                                      const uint8_t* __restrict__ pool, const uint8_t* __restrict__ p, uint32_t plen,
                                      uint64_t ph, uint64_t mask) {
    const uint64_t th = heads[i] & mask;
    if (th != ph) return th < ph ? -1 : 1;
    const uint32_t o = offs[i], tlen = offs[i + 1] - o;
    if (plen > 8) {
        const uint32_t m = tlen < plen ? tlen : plen;
        for (uint32_t j = 8; j < m; j++) {
            const uint8_t a = pool[(uint64_t)o + j], b = p[j];
            if (a != b) return a < b ? -1 : 1;
        }
    }
    return tlen >= plen ? 0 : -1;   // equal on the shorter length: a term shorter than p sorts before it
}

// One round of the 64-ary search on [a, b): lanes test the pivots a + (l + 1) s - 1; m = the number of leading lanes whose
// pivot is false.  The first true index of [a, b) (b if none) then lies in [a + m s, min(b, a + (m + 1) s - 1)].
__device__ __forceinline__ void ac_narrow(uint32_t& a, uint32_t& b, uint32_t s, uint32_t m) {
    const uint64_t na = (uint64_t)a + (uint64_t)m * s, nb = (uint64_t)a + (uint64_t)(m + 1) * s - 1;
    a = (uint32_t)(na < b ? na : b);
    b = (uint32_t)(nb < b ? nb : b);
}

__device__ __forceinline__ uint32_t ac_first_false_count(bool t) {   // leading lanes with t == false
    const uint64_t bal = __builtin_amdgcn_ballot_w64(t);
    return bal ? (uint32_t)__builtin_ctzll(bal) : 64u;
}

// first index of [a, b) with c(i) >= thr (b if none)
__device__ __forceinline__ uint32_t ac_search(uint32_t a, uint32_t b, int thr, uint32_t lane, const uint64_t* heads, const uint32_t* offs,
                                              const uint8_t* pool, const uint8_t* p, uint32_t plen, uint64_t ph, uint64_t mask) {
    while (b > a) {
        const uint32_t s = (b - a + 63) / 64;
        const uint64_t piv = (uint64_t)a + (uint64_t)(lane + 1) * s - 1;
        const bool t = piv < b ? ac_cmp((uint32_t)piv, heads, offs, pool, p, plen, ph, mask) >= thr : true;
        ac_narrow(a, b, s, ac_first_false_count(t));
    }
    return a;
}

// [lo, hi): the index range of the terms that start with p (one wave; every lane gets both ends).  One search for both
// ends while their ranges coincide, then one each.  Shared by k_ac_suggest and the spelling corrector's k_fz_plan.
__device__ __forceinline__ void ac_prefix_range(uint32_t n, uint32_t lane, const uint64_t* __restrict__ heads,
                                                const uint32_t* __restrict__ offs, const uint8_t* __restrict__ pool,
                                                const uint8_t* __restrict__ p, uint32_t plen, uint64_t ph, uint64_t mask,
                                                uint32_t& lo, uint32_t& hi) {
    uint32_t a = 0, b = n;
    bool split = false;
    uint32_t alo = 0, blo = 0, ahi = 0, bhi = 0;
    while (b > a) {
        const uint32_t s = (b - a + 63) / 64;
        const uint64_t piv = (uint64_t)a + (uint64_t)(lane + 1) * s - 1;
        const int c = piv < b ? ac_cmp((uint32_t)piv, heads, offs, pool, p, plen, ph, mask) : 1;
        const uint32_t mlo = ac_first_false_count(c >= 0), mhi = ac_first_false_count(c > 0);
        if (mlo != mhi) {
            alo = a; blo = b; ac_narrow(alo, blo, s, mlo);
            ahi = a; bhi = b; ac_narrow(ahi, bhi, s, mhi);
            split = true;
            break;
        }
        ac_narrow(a, b, s, mlo);
    }
    if (split) {
        lo = ac_search(alo, blo, 0, lane, heads, offs, pool, p, plen, ph, mask);
        hi = ac_search(ahi, bhi, 1, lane, heads, offs, pool, p, plen, ph, mask);
    } else {
        lo = hi = a;
    }
}

// The lists [x, y) of one level (level < 0: raw terms, one key each; else nodes, L keys each) offered in chunks of 63.
__device__ __forceinline__ void ac_offer(const uint64_t* __restrict__ base, uint32_t stride, uint32_t len, uint32_t x, uint32_t y,
                                         uint32_t lane, uint32_t L, uint64_t (&best)[kAcTop], uint64_t& worst) {
    for (uint32_t c0 = x; c0 < y; c0 += 63) {
        const uint32_t cnt = (y - c0) < 63u ? (y - c0) : 63u;
        uint64_t k[kAcTop];
        if (lane < cnt) {
            const uint64_t* src = base + (uint64_t)(c0 + lane) * stride;
#pragma unroll
            for (int i = 0; i < kAcTop; i++) k[i] = (uint32_t)i < len ? src[i] : kAcEmpty;
        } else {
#pragma unroll
            for (int i = 0; i < kAcTop; i++) k[i] = lane == 63 ? best[i] : kAcEmpty;
        }
        // nothing of this chunk can enter the best L: skip the merge
        if (worst != kAcEmpty && ac_wave_min(lane < cnt ? k[0] : kAcEmpty) > worst) continue;
        ac_merge(k, L, best, worst);
    }
}

// One wave per request.  idx_out[q * L + r] = dictionary index of the r-th suggestion (~0u past count_out[q]).
__global__ void __launch_bounds__(256) k_ac_suggest(const uint64_t* __restrict__ heads, const uint32_t* __restrict__ offs,
                                                    const uint8_t* __restrict__ pool, const uint64_t* __restrict__ keys,
                                                    const uint64_t* __restrict__ tree, AcLevels lv, uint32_t n,
                                                    const uint8_t* __restrict__ qbytes, const uint32_t* __restrict__ qoffs, uint32_t n_q,
                                                    uint32_t L, uint32_t* __restrict__ idx_out, uint32_t* __restrict__ count_out) {
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (q >= n_q) return;   // wave-uniform
    const uint8_t* p = qbytes + qoffs[q];
    const uint32_t plen = qoffs[q + 1] - qoffs[q];
    const uint32_t hlen = plen < 8 ? plen : 8;
    uint64_t ph = 0;
    for (uint32_t j = 0; j < hlen; j++) ph |= (uint64_t)p[j] << (56 - 8 * j);
    const uint64_t mask = hlen ? ~0ull << (64 - 8 * hlen) : 0ull;

    uint32_t lo = 0, hi = 0;
    ac_prefix_range(n, lane, heads, offs, pool, p, plen, ph, mask, lo, hi);

    uint64_t best[kAcTop], worst = kAcEmpty;
#pragma unroll
    for (int i = 0; i < kAcTop; i++) best[i] = kAcEmpty;
    if (lo < hi) {
        const uint32_t bl = (lo + kAcFan - 1) / kAcFan, bh = hi / kAcFan;   // whole level-0 blocks [bl, bh)
        if (bl >= bh) {
            ac_offer(keys, 1, 1, lo, hi, lane, L, best, worst);
        } else {
            ac_offer(keys, 1, 1, lo, bl * kAcFan, lane, L, best, worst);
            ac_offer(keys, 1, 1, bh * kAcFan, hi, lane, L, best, worst);
            uint32_t x = bl, y = bh;
            for (uint32_t j = 0; j < lv.n_levels; j++) {
                const uint64_t* nodes = tree + lv.off[j];
                const uint32_t gx = (x + kAcFan - 1) / kAcFan, gy = y / kAcFan;
                if (j + 1 == lv.n_levels || gx >= gy) {
                    ac_offer(nodes, kAcTop, L, x, y, lane, L, best, worst);
                    break;
                }
                ac_offer(nodes, kAcTop, L, x, gx * kAcFan, lane, L, best, worst);
                ac_offer(nodes, kAcTop, L, gy * kAcFan, y, lane, L, best, worst);
                x = gx;
                y = gy;
            }
        }
    }
    if (lane < L) {
        uint64_t v = best[0];
#pragma unroll
        for (int i = 1; i < kAcTop; i++) v = lane == (uint32_t)i ? best[i] : v;
        idx_out[(uint64_t)q * L + lane] = v == kAcEmpty ? ~0u : (uint32_t)v;
    }
    if (lane == 0) {
        uint32_t cnt = 0;
#pragma unroll
        for (int i = 0; i < kAcTop; i++) cnt += ((uint32_t)i < L && best[i] != kAcEmpty) ? 1u : 0u;
        count_out[q] = cnt;
    }
}

}  // namespace ns
