// SPDX-License-Identifier: MIT
// Search sorted by a per-document key: for a batch of queries the first K documents of each query's matched
// set in the order (rank key, position of the segment in the call's list ascending, docId ascending), with their BM25
// scores.  The matched set is ns_facet_count's; the work items are fc_plan's (ns_facet_plan.hpp), the sub-batches
// ns_sorted_plan.hpp's.  rank key t = key (newest first) or key ? ~key : 0 (oldest first): larger t first, key 0 last in
// both directions (0xFFFFFFFF is refused at upload, so ~key is never 0 for a dated document).
//   k_sd_check    at upload: does a key hold the reserved value?
//   k_sd_select   one workgroup of 256 threads per item.  Cut and mark as k_fc_count does (fc_cut, fc_mark: the tile's
//                 matched set as a bitmap in LDS; AND through a second bitmap).  Sweep: a wave takes 64 bitmap words at a
//                 time, one per lane; every lane pops its lowest set bit, gathers that document's key (4 B) and offers
//                     (t << 32) | ~(docId - doc_lo)         distinct per document of the tile, never 0
//                 to the wave's kept set: the 128 best keys so far, SORTED in two registers per lane (§5n's ml_sort_up /
//                 ml_merge_down network, twice).  A chunk of 64 in which no lane beats the current K-th key is skipped on one
//                 ballot.  The four waves' sets meet in LDS, wave 0 joins them and writes the item's row of K candidates
//                 (0 = none).  The item's matched count goes into found[query] with one integer atomic.
//                 A group of ONE list needs no bitmap: its in-tile postings are its documents.
//   k_sd_join     one wave per query over the rows of the query's items, which are contiguous in plan order (segment
//                 position, then tile).  (t << 32) | ~(item index relative to the query * 128 + slot) is again distinct and
//                 realises the total order, because a row is docId-ascending among equal t.  Writes the final row (segment
//                 id, docId, the key as uploaded), nhits and the pad.
//   k_sd_score    one wave per (query, hit): for each ref of the query in the hit's segment, in query order, a wave-wide
//                 lower bound over the list (fc_lower_bound); on an exact docId match
//                     acc += qweight * ((idf * (tf * 2.2f)) / (tf + norm[doc]))      every operation rounds to fp32
//                 Lane 0 stores the score with a plain vector store.
// Every docId read from a list is tested against the tile before it indexes the bitmap or the key table; a list that is
// not ascending may lose hits but reads and writes nothing out of bounds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ns_sorted_plan.hpp"
#include "ns_after.hip"

namespace ns {

struct DevSdSeg {
    const uint32_t* keys;   // per document
    const float* norm;      // per document (ns_seg::d_norm)
    uint32_t seg_id;        // the id the refs use for this segment
    uint32_t pad;
};

#ifdef NS_COUNT
// Counting build only: events of the three kernels since the last reset (ns_debug_sorted_counters).  0 items, 1 AND items that
// intersected two bitmaps, 2 single-list items, 3 AND items ended by a list without a posting in the tile, 4 chunks skipped
// on the threshold ballot, 5 chunks that inserted, 6 rows joined, 7 score lookups that found the document, 8 those that did not.
constexpr int kNsScnt = 9;
__device__ unsigned long long g_ns_scnt[kNsScnt];
#define NS_SCNT(i, v) do { if (threadIdx.x == 0) atomicAdd(&g_ns_scnt[(i)], (unsigned long long)(v)); } while (0)
#define NS_SCNT_WAVE(i, v) do { if ((threadIdx.x & 63u) == 0) atomicAdd(&g_ns_scnt[(i)], (unsigned long long)(v)); } while (0)
#else
#define NS_SCNT(i, v)
#define NS_SCNT_WAVE(i, v)
#endif

__global__ void __launch_bounds__(256) k_sd_check(const uint32_t* __restrict__ keys, uint32_t n_docs, uint32_t* __restrict__ bad) {
    bool b = false;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_docs; i += gridDim.x * 256u) b = b || keys[i] == 0xFFFFFFFFu;
    if (b) atomicOr(bad, 1u);
}

// A wave's kept set: the 128 largest keys offered so far, descending over (hi lane 0 .. 63, lo lane 0 .. 63); 0 = none.
struct SdSet {
    uint64_t hi, lo;
};

__device__ __forceinline__ uint64_t sd_key(uint32_t key, uint32_t low, bool asc) {
    const uint32_t t = asc ? (key ? ~key : 0u) : key;
    return ((uint64_t)t << 32) | (uint32_t)~low;
}

// Offers one key per lane (any order, 0 = none).  All 64 lanes call it together.  K <= 64 keeps hi alone.
__device__ __forceinline__ void sd_insert(SdSet& s, uint64_t key, uint32_t K, uint32_t lane) {
    const uint64_t thr = K <= 64u ? ml_shfl(s.hi, K - 1u) : ml_shfl(s.lo, K - 65u);   // the current K-th key (0 while fewer are kept)
    if (__ballot(key > thr) == 0ull) { NS_SCNT_WAVE(4, 1); return; }                  // (wave-uniform)
    NS_SCNT_WAVE(5, 1);
    const uint64_t up = ml_sort_up(key, lane);
    // hi descending against up ascending: lane by lane the larger ones are the 64 largest of the 128, the smaller ones the
    // rest, each a bitonic sequence.  Everything in lo is below everything in hi, so the new hi is final.
    const uint64_t big = s.hi < up ? up : s.hi, small = s.hi < up ? s.hi : up;
    s.hi = ml_merge_down(big, lane);
    if (K > 64u) {
        const uint64_t rest = ml_merge_down(small, lane);                             // descending
        s.lo = ml_join(s.lo, ml_shfl(rest, 63u - lane), lane);
    }
}

// AFTER (§5s, ns_after.hip): last[blockIdx.x] bounds the keys that may enter, and the item's count of such keys goes into
// rest[query].  Wave 0's own slot of s_rows is never read back, so under AFTER it is not written and its first word holds the
// item's count instead.  With AFTER = false neither pointer is read and the code is what it was without the parameter.
template <bool AND, bool AFTER>
__global__ void __launch_bounds__(256) k_sd_select(const FcItem* __restrict__ items, const FcRef* __restrict__ refs,
                                                   const DevFcSeg* __restrict__ segs, const DevSdSeg* __restrict__ sds, uint32_t K,
                                                   uint32_t asc, uint64_t* __restrict__ cand, unsigned long long* __restrict__ found,
                                                   const uint64_t* __restrict__ last_of, unsigned long long* __restrict__ rest) {
    __shared__ uint32_t s_bm[kFcTileDocs / 32u];
    __shared__ uint32_t s_and[AND ? kFcTileDocs / 32u : 1u];
    __shared__ uint64_t s_rows[4][128];
    __shared__ uint32_t s_cnt;
    const FcItem it = items[blockIdx.x];
    const DevFcSeg sg = segs[it.seg];
    const uint32_t* __restrict__ keys = sds[it.seg].keys;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, v = tid >> 6;
    const uint32_t n_words = (it.doc_hi - it.doc_lo + 31u) / 32u;   // <= kFcTileDocs / 32: the tile is the host's, at most the product's
    NS_SCNT(0, 1);
    if (tid == 0) s_cnt = 0u;
    uint32_t* const s_rest = reinterpret_cast<uint32_t*>(&s_rows[0][0]);
    uint64_t last = kAfterAll;
    uint32_t kept = 0;
    if (AFTER) {
        last = last_of[blockIdx.x];
        if (tid == 0) *s_rest = 0u;
        af_count_item(last);
    }
    SdSet set{0ull, 0ull};
    uint32_t cnt = 0;
    if (it.ref_count == 1u) {
        uint64_t lo, hi;
        fc_cut(sg, refs[it.ref_begin], it.doc_lo, it.doc_hi, lane, lo, hi);
        NS_SCNT(2, 1);
        for (uint64_t base = lo + v * 64u; base < hi; base += 256u) {   // (wave-uniform)
            const uint64_t i = base + lane;
            uint64_t key = 0;
            if (i < hi) {
                const uint32_t d = sg.postings[i].x;
                if (d >= it.doc_lo && d < it.doc_hi) { cnt++; key = sd_key(keys[d], d - it.doc_lo, asc != 0u); }
            }
            if (AFTER) key = af_clip(key, last, kept);
            sd_insert(set, key, K, lane);
        }
    } else {
        bool any = true;   // the same in every thread: the cuts depend on the item alone
        for (uint32_t w = tid; w < n_words; w += 256u) {
            s_bm[w] = 0u;
            if (AND) s_and[w] = 0u;
        }
        __syncthreads();
        for (uint32_t r = 0; r < it.ref_count; r++) {
            uint64_t lo, hi;
            fc_cut(sg, refs[it.ref_begin + r], it.doc_lo, it.doc_hi, lane, lo, hi);
            if (AND) {
                if (lo == hi) { any = false; NS_SCNT(3, 1); break; }
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
                    if (r == 1u) NS_SCNT(1, 1);
                }
            } else {
                fc_mark(sg.postings, lo, hi, it.doc_lo, it.doc_hi, s_bm);
            }
        }
        __syncthreads();
        if (any)
            for (uint32_t wb = v * 64u; wb < n_words; wb += 256u) {   // (wave-uniform)
                const uint32_t w = wb + lane;
                uint32_t bits = w < n_words ? s_bm[w] : 0u;
                cnt += (uint32_t)__popc(bits);
                while (__ballot(bits != 0u) != 0ull) {
                    uint64_t key = 0;
                    if (bits) {
                        const uint32_t rel = w * 32u + (uint32_t)__builtin_ctz(bits);   // < doc_hi - doc_lo: only such bits are set
                        bits &= bits - 1u;
                        key = sd_key(keys[it.doc_lo + rel], rel, asc != 0u);
                    }
                    if (AFTER) key = af_clip(key, last, kept);
                    sd_insert(set, key, K, lane);
                }
            }
    }
    __syncthreads();   // (s_cnt is zero)
    if (cnt) atomicAdd(&s_cnt, cnt);
    if (AFTER && kept) atomicAdd(s_rest, kept);
    if (!AFTER || v != 0u) {
        s_rows[v][lane] = set.hi;
        s_rows[v][64u + lane] = set.lo;
    }
    __syncthreads();
    if (v != 0u) return;
    if (tid == 0 && s_cnt) atomicAdd(&found[it.query], (unsigned long long)s_cnt);
    if (AFTER && tid == 0 && *s_rest) atomicAdd(&rest[it.query], (unsigned long long)*s_rest);
#pragma unroll 1
    for (uint32_t o = 1; o < 4u; o++) {
        sd_insert(set, s_rows[o][lane], K, lane);
        if (K > 64u) sd_insert(set, s_rows[o][64u + lane], K, lane);
    }
    uint64_t* __restrict__ row = cand + (size_t)blockIdx.x * K;
    if (lane < K) row[lane] = set.hi;
    if (64u + lane < K) row[64u + lane] = set.lo;
}

// items / q_off index the whole call's items; cand holds the rows of the items from item_begin on.
__global__ void __launch_bounds__(256) k_sd_join(const FcItem* __restrict__ items, const uint32_t* __restrict__ q_off, uint32_t q_begin,
                                                 uint32_t q_end, uint32_t item_begin, const DevSdSeg* __restrict__ sds,
                                                 const uint64_t* __restrict__ cand, uint32_t K, uint32_t asc, uint32_t* __restrict__ hits,
                                                 uint32_t* __restrict__ keys_out, uint32_t* __restrict__ pos_out, uint32_t* __restrict__ nhits) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = q_begin + blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= q_end) return;                                            // (wave-uniform; no barrier in this kernel)
    const uint32_t ib = q_off[q], ie = q_off[q + 1u];
    SdSet set{0ull, 0ull};
    for (uint32_t i = ib; i < ie; i++) {
        const uint64_t* __restrict__ row = cand + (size_t)(i - item_begin) * K;
        if (row[0] == 0ull) continue;                                  // an item that matched nothing (wave-uniform)
        NS_SCNT_WAVE(6, 1);
        const uint32_t base = (i - ib) * kSdRowSlots;
#pragma unroll 1
        for (uint32_t slot = lane; slot < kSdRowSlots && slot - lane < K; slot += 64u) {   // (wave-uniform: slot - lane is 0 or 64)
            const uint64_t c = slot < K ? row[slot] : 0ull;
            sd_insert(set, c ? ((c >> 32) << 32) | (uint32_t)~(base + slot) : 0ull, K, lane);
        }
    }
    uint32_t n = 0;
#pragma unroll 1
    for (uint32_t r = lane; r - lane < K; r += 64u) {                  // (r - lane is 0 or 64; K <= 128)
        const uint64_t jk = r < 64u ? set.hi : set.lo;
        const bool have = r < K && jk != 0ull;
        n += (uint32_t)__popcll(__ballot(have));
        if (r >= K) continue;
        const size_t at = (size_t)q * K + r;
        if (have) {
            const uint32_t low = ~(uint32_t)jk, rel = low / kSdRowSlots, slot = low % kSdRowSlots;
            const FcItem it = items[ib + rel];
            const uint64_t c = cand[(size_t)(ib + rel - item_begin) * K + slot];
            const uint32_t t = (uint32_t)(c >> 32);
            hits[at * 3u + 0u] = 0u;                                  // k_sd_score's
            hits[at * 3u + 1u] = sds[it.seg].seg_id;
            hits[at * 3u + 2u] = it.doc_lo + ~(uint32_t)c;
            keys_out[at] = asc ? (t ? ~t : 0u) : t;
            pos_out[at] = it.seg;
        } else {
            hits[at * 3u + 0u] = 0xFF800000u;                         // -inf
            hits[at * 3u + 1u] = 0xFFFFFFFFu;
            hits[at * 3u + 2u] = 0xFFFFFFFFu;
            keys_out[at] = 0u;
            pos_out[at] = 0xFFFFFFFFu;
        }
    }
    if (lane == 0) nhits[q] = n;
}

__global__ void __launch_bounds__(256) k_sd_score(const ns_query_desc* __restrict__ queries, const ns_term_ref* __restrict__ terms,
                                                  uint32_t q_begin, uint32_t q_end, const DevFcSeg* __restrict__ segs,
                                                  const DevSdSeg* __restrict__ sds, uint32_t K, const uint32_t* __restrict__ pos_out,
                                                  const uint32_t* __restrict__ nhits, uint32_t* __restrict__ hits) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint64_t qq = q_begin + w / K;
    if (qq >= q_end) return;                                           // (wave-uniform; no barrier in this kernel)
    const uint32_t q = (uint32_t)qq, r = (uint32_t)(w % K);
    if (r >= nhits[q]) return;
    const size_t at = (size_t)q * K + r;
    const uint32_t pos = pos_out[at], doc = hits[at * 3u + 2u];
    const DevFcSeg sg = segs[pos];
    const DevSdSeg sd = sds[pos];
    const ns_query_desc qd = queries[q];
    const float norm = sd.norm[doc];                                   // doc < n_docs: it came out of the tile
    float acc = 0.0f;
    for (uint32_t j = qd.term_begin; j < qd.term_begin + qd.term_count; j++) {
        const ns_term_ref t = terms[j];
        if (t.seg_id != sd.seg_id || !t.count) continue;
        const uint64_t first = t.byte_off / 8u, end = first + t.count;
        const uint64_t i = fc_lower_bound(sg.postings, first, end, doc, lane);
        bool hit = false;
        if (i < end) {
            const uint2 p = sg.postings[i];
            if (p.x == doc) {
                const float tf = (float)p.y;
                const float s = (t.idf * (tf * (1.2f + 1.0f))) / (tf + norm);
                acc = acc + t.qweight * s;
                hit = true;
            }
        }
        if (hit) NS_SCNT_WAVE(7, 1); else NS_SCNT_WAVE(8, 1);
    }
    if (lane == 0) hits[at * 3u + 0u] = __float_as_uint(acc);
}

}  // namespace ns
