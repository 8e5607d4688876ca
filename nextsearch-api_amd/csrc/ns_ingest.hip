// SPDX-License-Identifier: MIT
// Indexing on the device: document texts -> forward index, the step in front of ns_invert_forward.
// The reference does it per document on one core (src/ForwardIndex.cpp:139-179 with include/textutil.hpp:13-37):
// tokenize, drop tokens shorter than 2 bytes and the 24 stop words, count tf in a hash map, hand out term ids.
//
// Here, over the texts of all documents back to back (n bytes, < 4 GiB):
//   k_ig_docmark      one bit per byte: a document starts here (a document boundary separates tokens)
//   k_ig_text<false>  16 bytes per thread: alnum mask, token STARTS and token ENDS counted per 4096-byte tile
//   k_ig_text<true>   the same masks after the scan of the tile counts: token t's start and end positions are written
//                     (the t-th start and the t-th end belong together, so a token of any length — across tiles, 70 000
//                     bytes — costs what two marks cost), and the text is lower-cased in place
//   k_ig_keep         length >= 2 and not a stop word; scan -> the kept tokens, compacted in input order
//   k_ig_kept         per kept token: start, length, document (binary search in the offsets), 64-bit polynomial hash;
//                     tokens longer than kIgLong bytes are hashed by a workgroup each (k_ig_hash_long: chunk hashes
//                     joined by h(AB) = h(A) * P^|B| + h(B))
//   k_ig_insert       open-addressing table of token indices: the hash routes, the BYTES decide; a slot holds the
//                     smallest token index of its term (atomicMin), i.e. the term's first kept occurrence
//   k_ig_first / k_ig_termid   term id = rank of that first occurrence among all first occurrences (a scan)
//   k_ig_term_bytes   the dictionary's bytes in term id order
//   sort 1 (k_iv_pass, stable) by term id; equal (doc, term) are then neighbours: k_ig_runflag / k_ig_runemit / k_ig_tf
//   sort 2 (k_iv_pass, stable) of the (doc, term, tf) runs by document: forward.bin's order, term ids ascending per document
//   k_iv_runs         pairs per document, kept tokens per document (doc_len); k_ig_docemit compacts the surviving documents
//
// Which slot of the table a term lands in depends on the order the atomics arrive in; nothing that leaves the table does:
// a lookup yields the term's smallest token index whatever the slot.  Everything else is scans and stable sorts.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ns_ingest_text.hpp"

namespace ns {

__global__ void __launch_bounds__(256) k_ig_docmark(const uint32_t* __restrict__ offs, uint32_t n_docs, uint32_t n, uint32_t* __restrict__ docbits) {
    const uint32_t d = blockIdx.x * 256 + threadIdx.x;
    if (d >= n_docs) return;
    const uint32_t o = offs[d];
    if (o < n) atomicOr(&docbits[o >> 5], 1u << (o & 31u));   // OR commutes: the bitmap does not depend on arrival order
}

// WRITE == false: tile_s / tile_e receive the tile's number of token starts / ends.
// WRITE == true : they hold the exclusive scans of those; tok_start / tok_end are filled and the text is lower-cased in place
//                 (a neighbour reading a byte before or after it is lower-cased sees the same alnum class either way).
template <bool WRITE>
__global__ void __launch_bounds__(256) k_ig_text(uint8_t* __restrict__ text, uint32_t n, const uint32_t* __restrict__ docbits,
                                                 uint32_t* __restrict__ tile_s, uint32_t* __restrict__ tile_e,
                                                 uint32_t* __restrict__ tok_start, uint32_t* __restrict__ tok_end) {
    __shared__ uint32_t wsum[4];
    const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * 16u;   // n < 2^32 - 65536: no wrap
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    const bool full = i0 < n && n - i0 >= 16u;
    if (full) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + i0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else if (i0 < n) {
        for (uint32_t j = 0; i0 + j < n; j++) w[j >> 2] |= (uint32_t)text[i0 + j] << (8 * (j & 3u));   // (a zero byte is a separator)
    }
    uint32_t A = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) A |= (uint32_t)ig_alnum((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) << j;
    uint32_t S = 0, E = 0;
    if (i0 < n && A) {
        const uint32_t dw = docbits[i0 >> 5];
        const uint32_t sh = i0 & 31u;                                   // 0 or 16
        const uint32_t D = (dw >> sh) & 0xFFFFu;
        const uint32_t nextD = sh ? (docbits[(i0 >> 5) + 1] & 1u) : ((dw >> 16) & 1u);   // the bitmap has a word past the text's last
        const uint32_t prevA = (i0 > 0 && ig_alnum(text[i0 - 1])) ? 1u : 0u;
        const uint32_t nextA = (n - i0 > 16u && ig_alnum(text[i0 + 16])) ? 1u : 0u;
        S = A & (~((A << 1) | prevA) | D) & 0xFFFFu;
        E = A & (~((A >> 1) | (nextA << 15)) | ((D >> 1) | (nextD << 15))) & 0xFFFFu;
    }
    const uint32_t c = (uint32_t)__popc(S) | ((uint32_t)__popc(E) << 16);   // a tile holds at most 4096 of each
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x == 0) {
            const uint32_t t = wsum[0] + wsum[1] + wsum[2] + wsum[3];
            tile_s[blockIdx.x] = t & 0xFFFFu;
            tile_e[blockIdx.x] = t >> 16;
        }
        return;
    }
    uint32_t ex = inc - c;
    for (int j = 0; j < wv; j++) ex += wsum[j];
    uint32_t rs = tile_s[blockIdx.x] + (ex & 0xFFFFu), re = tile_e[blockIdx.x] + (ex >> 16);
    for (uint32_t m = S; m; m &= m - 1) tok_start[rs++] = i0 + (uint32_t)__ffs(m) - 1u;
    for (uint32_t m = E; m; m &= m - 1) tok_end[re++] = i0 + (uint32_t)__ffs(m);          // one past the token's last byte
    if (A) {   // lower-case: only alnum bytes can be upper-case letters
        bool changed = false;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t ch = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            if (ch - 'A' < 26u) { w[j >> 2] |= 0x20u << (8 * (j & 3)); changed = true; }
        }
        if (changed) {
            if (full) *reinterpret_cast<uint4*>(text + i0) = make_uint4(w[0], w[1], w[2], w[3]);
            else for (uint32_t j = 0; i0 + j < n; j++) text[i0 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3u)));
        }
    }
}

// (the text is lower case by now)
__global__ void __launch_bounds__(256) k_ig_keep(const uint8_t* __restrict__ text, const uint32_t* __restrict__ tok_start,
                                                 const uint32_t* __restrict__ tok_end, uint32_t n_tok, uint32_t* __restrict__ keep) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tok) return;
    const uint32_t s = tok_start[t], len = tok_end[t] - s;
    bool k = len >= 2;                                   // src/ForwardIndex.cpp:146
    if (k && len <= 4) {                                 // :147
        uint32_t w = 0;
        for (uint32_t j = 0; j < len; j++) w |= (uint32_t)text[s + j] << (8 * j);
        k = !ig_stop(w);
    }
    keep[t] = k ? 1u : 0u;
}

// kidx = exclusive scan of keep; n_kept_dev = its total
__global__ void __launch_bounds__(256) k_ig_kept(const uint8_t* __restrict__ text, const uint32_t* __restrict__ tok_start,
                                                 const uint32_t* __restrict__ tok_end, uint32_t n_tok, const uint32_t* __restrict__ kidx,
                                                 const uint32_t* __restrict__ n_kept_dev, const uint32_t* __restrict__ offs, uint32_t n_docs,
                                                 uint64_t hash_mask, uint32_t* __restrict__ kstart, uint32_t* __restrict__ klen,
                                                 uint32_t* __restrict__ kdoc, uint64_t* __restrict__ khash,
                                                 uint32_t* __restrict__ long_list, uint32_t* __restrict__ long_count) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tok) return;
    const uint32_t k = kidx[t];
    if ((t + 1 < n_tok ? kidx[t + 1] : *n_kept_dev) == k) return;   // not kept
    const uint32_t s = tok_start[t], len = tok_end[t] - s;
    // the document that holds byte s: the last d with offs[d] <= s (empty documents share their offset with the next one)
    uint32_t lo = 0, hi = n_docs;                                     // offs[lo] <= s < offs[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (offs[mid] <= s) lo = mid; else hi = mid;
    }
    kstart[k] = s; klen[k] = len; kdoc[k] = lo;
    if (len > kIgLong) {
        long_list[atomicAdd(long_count, 1u)] = k;                     // (the list's order is never read: each entry writes its own khash)
        return;
    }
    khash[k] = ig_hash_bytes(text + s, len) & hash_mask;
}

__global__ void __launch_bounds__(256) k_ig_hash_long(const uint8_t* __restrict__ text, const uint32_t* __restrict__ kstart,
                                                      const uint32_t* __restrict__ klen, const uint32_t* __restrict__ long_list,
                                                      const uint32_t* __restrict__ long_count, uint64_t hash_mask, uint64_t* __restrict__ khash) {
    __shared__ uint64_t part[256];
    const uint32_t n_long = *long_count;
    for (uint32_t i = blockIdx.x; i < n_long; i += gridDim.x) {
        const uint32_t k = long_list[i], s = kstart[k], len = klen[k];
        const uint32_t chunk = (len + 255u) / 256u;
        const uint32_t b = min(len, threadIdx.x * chunk), e = min(len, b + chunk);
        uint64_t h = 0;
        for (uint32_t j = b; j < e; j++) h = h * kIgP + (uint64_t)(text[s + j] + 1u);
        part[threadIdx.x] = h;
        __syncthreads();
        if (threadIdx.x == 0) khash[k] = ig_hash_join(part, len) & hash_mask;
        __syncthreads();
    }
}

__device__ __forceinline__ bool ig_same(const uint8_t* __restrict__ text, uint32_t a, uint32_t b, uint32_t len) {
    if (a == b) return true;
    for (uint32_t j = 0; j < len; j++)
        if (text[a + j] != text[b + j]) return false;
    return true;
}

// table: `mask + 1` slots (a power of two, at least twice the kept tokens: an empty slot always ends a probe)
__global__ void __launch_bounds__(256) k_ig_insert(const uint8_t* __restrict__ text, const uint32_t* __restrict__ kstart,
                                                   const uint32_t* __restrict__ klen, const uint64_t* __restrict__ khash, uint32_t n_kept,
                                                   uint32_t* __restrict__ table, uint32_t mask, uint32_t* __restrict__ kslot) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_kept) return;
    const uint64_t h = khash[k];
    const uint32_t s = kstart[k], len = klen[k];
    uint32_t slot = (uint32_t)h & mask;
    for (;;) {
        uint32_t cur = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kIgEmpty) {
            cur = atomicCAS(&table[slot], kIgEmpty, k);
            if (cur == kIgEmpty) break;
        }
        // a slot only ever changes from one token of a term to another token of the same term
        if (cur == k || (khash[cur] == h && klen[cur] == len && ig_same(text, kstart[cur], s, len))) {
            if (k < cur) atomicMin(&table[slot], k);
            break;
        }
        slot = (slot + 1u) & mask;
    }
    kslot[k] = slot;
}

__global__ void __launch_bounds__(256) k_ig_first(const uint32_t* __restrict__ table, const uint32_t* __restrict__ kslot, uint32_t n_kept,
                                                  uint32_t* __restrict__ krep, uint32_t* __restrict__ isfirst) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_kept) return;
    const uint32_t rep = table[kslot[k]];
    krep[k] = rep;
    isfirst[k] = rep == k ? 1u : 0u;
}

// fid = exclusive scan of isfirst: at a term's first occurrence, the term's id
__global__ void __launch_bounds__(256) k_ig_termid(const uint32_t* __restrict__ krep, const uint32_t* __restrict__ fid,
                                                   const uint32_t* __restrict__ kdoc, const uint32_t* __restrict__ kstart,
                                                   const uint32_t* __restrict__ klen, uint32_t n_kept, uint32_t* __restrict__ keys,
                                                   uint2* __restrict__ vals, uint32_t* __restrict__ tlen, uint32_t* __restrict__ tsrc) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_kept) return;
    const uint32_t rep = krep[k], tid = fid[rep];
    keys[k] = tid;
    vals[k] = make_uint2(kdoc[k], tid);
    if (rep == k) { tlen[tid] = klen[k]; tsrc[tid] = kstart[k]; }
}

// one wave per term; toff = exclusive scan of tlen (n_terms + 1 entries)
__global__ void __launch_bounds__(256) k_ig_term_bytes(const uint8_t* __restrict__ text, const uint32_t* __restrict__ tsrc,
                                                       const uint32_t* __restrict__ toff, uint32_t n_terms, uint8_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= n_terms) return;
    const uint32_t o = toff[t], len = toff[t + 1] - o, s = tsrc[t];
    for (uint32_t j = threadIdx.x & 63; j < len; j += 64) out[o + j] = text[s + j];
}

// vals sorted by (term, doc): a run of equal values is one (doc, term) pair, its length the tf
__global__ void __launch_bounds__(256) k_ig_runflag(const uint2* __restrict__ vals, uint32_t n, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool f = i == 0;
    if (!f) { const uint2 a = vals[i - 1], b = vals[i]; f = a.x != b.x || a.y != b.y; }
    flag[i] = f ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_ig_runemit(const uint2* __restrict__ vals, uint32_t n, const uint32_t* __restrict__ ridx,
                                                    uint32_t* __restrict__ rdoc, uint32_t* __restrict__ rterm, uint32_t* __restrict__ rpos) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint2 b = vals[i];
    if (i) { const uint2 a = vals[i - 1]; if (a.x == b.x && a.y == b.y) return; }
    const uint32_t r = ridx[i];
    rdoc[r] = b.x; rterm[r] = b.y; rpos[r] = i;
}
__global__ void __launch_bounds__(256) k_ig_tf(const uint32_t* __restrict__ rterm, const uint32_t* __restrict__ rpos, uint32_t n_runs,
                                               uint32_t n, uint2* __restrict__ pvals) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_runs) return;
    pvals[r] = make_uint2(rterm[r], (r + 1 < n_runs ? rpos[r + 1] : n) - rpos[r]);
}

__global__ void __launch_bounds__(256) k_ig_docflag(const uint32_t* __restrict__ dfirst, uint32_t n_docs, uint32_t* __restrict__ flag) {
    const uint32_t d = blockIdx.x * 256 + threadIdx.x;
    if (d < n_docs) flag[d] = dfirst[d] != kIgEmpty ? 1u : 0u;
}
// the documents with doc_len > 0 move up (src/ForwardIndex.cpp:152-155): didx = exclusive scan of the flags
__global__ void __launch_bounds__(256) k_ig_docemit(const uint32_t* __restrict__ dfirst, const uint32_t* __restrict__ dlast,
                                                    const uint32_t* __restrict__ pfirst, const uint32_t* __restrict__ plast,
                                                    const uint32_t* __restrict__ didx, uint32_t n_docs, uint32_t* __restrict__ out_map,
                                                    uint32_t* __restrict__ out_len, uint32_t* __restrict__ out_cnt) {
    const uint32_t d = blockIdx.x * 256 + threadIdx.x;
    if (d >= n_docs || dfirst[d] == kIgEmpty) return;
    const uint32_t j = didx[d];
    out_map[j] = d;
    out_len[j] = dlast[d] - dfirst[d] + 1u;
    out_cnt[j] = plast[d] - pfirst[d] + 1u;
}

}  // namespace ns
