// SPDX-License-Identifier: MIT
// Facet counts and date order for boolean queries: the matched set of ns_search_boolean, role by role, for a
// whole tile of kFcTileDocs documents at once, swept into a bucket histogram (ns_facet_count_boolean) or into the
// date-ordered kept set (ns_search_sorted_boolean).  No score table: the boolean score is looked up for the K survivors only.
// The work items are bq_plan's (ns_boolean_plan.hpp), the sub-batches ns_sorted_plan.hpp's, the cursor bounds
// ns_after_plan.hpp's.  k_fc_count, k_sd_select, k_sd_score, k_bq_select and k_bq_join are not touched; k_sd_join is reused.
//   bs_matched    the matched bitmap of one item's tile from its BqRefs, in two bitmaps of kFcTileDocs / 32 words:
//                   MUST lists: the first marks the matched bitmap, every further one the scratch bitmap, which is AND-ed in
//                   and cleared; a MUST list without a posting in the tile ends the item (workgroup-uniform).  No MUST ref: the
//                   SHOULD lists mark the matched bitmap.  NOT lists mark the scratch bitmap, which is clear at that point
//                   (never used, or cleared by the last intersection); matched &= ~scratch.  No third bitmap.
//   k_bs_count    bs_matched -> sweep (per set bit one gather of bucket_of_doc, 2 B, and one LDS atomic add) -> flush of the
//                 nonzero histogram entries with global integer atomics, as k_fc_count: no dependence on the item order.
//   k_bs_select   bs_matched -> sweep (per set bit one gather of the key, 4 B) into §5q's SdSet with sd_key, under AFTER through
//                 af_clip; the four waves' sets meet in LDS, wave 0 joins them and writes the item's row of K candidates;
//                 found / rest get one integer atomic each, as k_sd_select.
//   k_bs_score    k_sd_score's lookup with a role per ref: NOT refs are skipped.
// The GROUPED instantiations of k_bs_count and k_bs_select (§5u) differ in bs_matched's required stage alone; k_bs_score serves
// them as it is: a clause member that does not hold the document adds nothing.
// An item of ONE ref needs no bitmap (bq_plan emits it only when the ref is MUST or SHOULD): its in-tile postings are its
// documents.  Every docId read from a list is tested against the tile before it indexes LDS, the bucket table or the key table.
// Static LDS: 36 KiB per workgroup in both kernels (2 x 16 KiB bitmaps + 4 KiB histogram or row exchange).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ns_boolean_plan.hpp"

namespace ns {

#ifdef NS_COUNT
// Counting build only: events of the three kernels since the last reset (ns_debug_boolean_sets_counters).  0 items, 1 single-list
// items, 2 further MUST lists intersected, 3 items ended by a MUST list without a posting in the tile, 4 items in which an
// exclusion cleared a bit, 5 items whose matched set is empty after an exclusion ran, 6 histogram entries flushed, 7 chunks
// skipped on the threshold ballot, 8 chunks that inserted, 9 score lookups that found the document, 10 those that did not,
// 11 NOT refs the score kernel skipped.
constexpr int kNsBscnt = 12;
__device__ unsigned long long g_ns_bscnt[kNsBscnt];
#define NS_BSCNT(i, v) do { if (threadIdx.x == 0) atomicAdd(&g_ns_bscnt[(i)], (unsigned long long)(v)); } while (0)
#define NS_BSCNT_WAVE(i, v) do { if ((threadIdx.x & 63u) == 0) atomicAdd(&g_ns_bscnt[(i)], (unsigned long long)(v)); } while (0)
#else
#define NS_BSCNT(i, v)
#define NS_BSCNT_WAVE(i, v)
#endif

// sd_insert, counting into this file's counters (the sorted search's stay its own)
__device__ __forceinline__ void bs_insert(SdSet& s, uint64_t key, uint32_t K, uint32_t lane) {
#ifdef NS_COUNT
    const uint64_t thr = K <= 64u ? ml_shfl(s.hi, K - 1u) : ml_shfl(s.lo, K - 65u);
    if (__ballot(key > thr) == 0ull) { NS_BSCNT_WAVE(7, 1); return; }   // (wave-uniform; sd_insert would return here too)
    NS_BSCNT_WAVE(8, 1);
    const uint64_t up = ml_sort_up(key, lane);
    const uint64_t big = s.hi < up ? up : s.hi, small = s.hi < up ? s.hi : up;
    s.hi = ml_merge_down(big, lane);
    if (K > 64u) {
        const uint64_t rest = ml_merge_down(small, lane);
        s.lo = ml_join(s.lo, ml_shfl(rest, 63u - lane), lane);
    }
#else
    sd_insert(s, key, K, lane);
#endif
}

// The matched set of item `it` (ref_count >= 2) as bits of s_bm; s_tmp is the scratch bitmap.  Both hold at least
// n_words = ceil((doc_hi - doc_lo) / 32) <= kFcTileDocs / 32 words.  Called by all 256 threads; ends behind a barrier.  False
// (in every thread) when a MUST list has no posting in the tile: the item matches nothing and s_bm is not to be read.
// GROUPED (§5u): the required stage is ns_boolean.hip's bq_mark_clauses over the tile, as k_bq_select<., true>'s is over a window;
// false when a clause has no posting in the tile.  The scratch bitmap is clear when the NOT lists arrive, as before.
// QUORUM (§5w; implies GROUPED): the required stage is bq_count_clauses over the tile; s_pl: the counter planes, kFcTileDocs / 32
// words each (dynamic LDS behind the static bitmaps; NULL-like and never touched when the launch's needs are all 1).
template <bool GROUPED, bool QUORUM = false>
__device__ __forceinline__ bool bs_matched(const FcItem& it, const DevFcSeg& sg, const BqRef* __restrict__ rf, uint32_t n_words,
                                           uint32_t* s_bm, uint32_t* s_tmp, uint32_t* s_pl = nullptr) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t w = tid; w < n_words; w += 256u) {
        s_bm[w] = 0u;
        s_tmp[w] = 0u;
    }
    uint32_t n_must = 0, n_not = 0;   // the same in every thread: they depend on the item alone
    uint32_t n_clauses = 0;           // GROUPED: 1 + the largest clause index of a MUST ref
    for (uint32_t r = 0; r < it.ref_count; r++) {
        const uint32_t role = rf[r].role;
        n_must += role == kBqMust;
        n_not += role == kBqNot;
        if (GROUPED && role == kBqMust) n_clauses = max(n_clauses, (QUORUM ? bq_clause_index(rf[r].clause) : rf[r].clause) + 1u);
    }
    const uint32_t my_clause = GROUPED ? bq_clause_of_lane(rf, it.ref_count, lane) : 0u;
    __syncthreads();
    if (QUORUM && n_must) {
        if (!bq_count_clauses<7>(sg, rf, it.ref_count, n_clauses, my_clause, it.doc_lo, it.doc_hi, n_words, s_bm, s_tmp, s_pl, kFcTileDocs / 32u)) return false;
    } else if (GROUPED && n_must) {
        if (!bq_mark_clauses<6>(sg, rf, it.ref_count, n_clauses, my_clause, it.doc_lo, it.doc_hi, n_words, s_bm, s_tmp)) return false;
    } else if (n_must) {
        uint32_t seen = 0;
        for (uint32_t r = 0; r < it.ref_count; r++) {
            const BqRef b = rf[r];
            if (b.role != kBqMust) continue;
            uint64_t lo, hi;
            fc_cut(sg, b.list, it.doc_lo, it.doc_hi, lane, lo, hi);
            if (lo == hi) { NS_BSCNT(3, 1); return false; }   // (workgroup-uniform: the cut depends on the item alone)
            if (seen == 0u) {
                fc_mark(sg.postings, lo, hi, it.doc_lo, it.doc_hi, s_bm);
                __syncthreads();
            } else {
                fc_mark(sg.postings, lo, hi, it.doc_lo, it.doc_hi, s_tmp);
                __syncthreads();
                for (uint32_t w = tid; w < n_words; w += 256u) {
                    s_bm[w] &= s_tmp[w];
                    s_tmp[w] = 0u;
                }
                __syncthreads();
                NS_BSCNT(2, 1);
            }
            seen++;
        }
    } else {
        for (uint32_t r = 0; r < it.ref_count; r++) {
            const BqRef b = rf[r];
            if (b.role != kBqShould) continue;
            uint64_t lo, hi;
            fc_cut(sg, b.list, it.doc_lo, it.doc_hi, lane, lo, hi);
            fc_mark(sg.postings, lo, hi, it.doc_lo, it.doc_hi, s_bm);
        }
        __syncthreads();
    }
    if (n_not) {
        for (uint32_t r = 0; r < it.ref_count; r++) {
            const BqRef b = rf[r];
            if (b.role != kBqNot) continue;
            uint64_t lo, hi;
            fc_cut(sg, b.list, it.doc_lo, it.doc_hi, lane, lo, hi);
            fc_mark(sg.postings, lo, hi, it.doc_lo, it.doc_hi, s_tmp);
        }
        __syncthreads();
        bool cleared = false, left = false;
        for (uint32_t w = tid; w < n_words; w += 256u) {
            const uint32_t m = s_bm[w], x = s_tmp[w];
            cleared = cleared || (m & x) != 0u;
            left = left || (m & ~x) != 0u;
            s_bm[w] = m & ~x;
        }
#ifdef NS_COUNT
        if (__syncthreads_or(cleared ? 1 : 0)) NS_BSCNT(4, 1);
        if (!__syncthreads_or(left ? 1 : 0)) NS_BSCNT(5, 1);
#else
        (void)cleared;
        (void)left;
        __syncthreads();
#endif
    }
    return true;
}

template <bool GROUPED = false, bool QUORUM = false>
__global__ void __launch_bounds__(256) k_bs_count(const FcItem* __restrict__ items, const BqRef* __restrict__ refs,
                                                  const DevFcSeg* __restrict__ segs, uint32_t n_buckets, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_hist[kFcMaxBuckets];
    __shared__ uint32_t s_bm[kFcTileDocs / 32u];
    __shared__ uint32_t s_tmp[kFcTileDocs / 32u];
    extern __shared__ __attribute__((aligned(16))) uint32_t s_bs_planes[];   // QUORUM: 16 KiB per plane of the launch, else none
    const FcItem it = items[blockIdx.x];
    const DevFcSeg sg = segs[it.seg];
    const BqRef* __restrict__ rf = refs + it.ref_begin;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t n_words = (it.doc_hi - it.doc_lo + 31u) / 32u;   // <= kFcTileDocs / 32: the tile is the host's, at most the product's
    NS_BSCNT(0, 1);
    NS_BGCNT(5, 1);
    if (QUORUM) NS_BQCNT(6, 1);
    for (uint32_t b = tid; b < n_buckets; b += 256u) s_hist[b] = 0u;
    if (it.ref_count == 1u) {
        uint64_t lo, hi;
        fc_cut(sg, rf[0].list, it.doc_lo, it.doc_hi, lane, lo, hi);
        NS_BSCNT(1, 1);
        NS_BGCNT(10, 1);
        __syncthreads();
        for (uint64_t i = lo + tid; i < hi; i += 256u) {
            const uint32_t d = sg.postings[i].x;
            if (d >= it.doc_lo && d < it.doc_hi) atomicAdd(&s_hist[sg.buckets[d]], 1u);
        }
    } else {
        if (!bs_matched<GROUPED, QUORUM>(it, sg, rf, n_words, s_bm, s_tmp, QUORUM ? s_bs_planes : nullptr)) return;   // (workgroup-uniform; the histogram is all zero)
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
    uint32_t* __restrict__ row = counts + (size_t)it.query * n_buckets;
    for (uint32_t b = tid; b < n_buckets; b += 256u) {
        const uint32_t c = s_hist[b];
        if (c) {
            atomicAdd(&row[b], c);
#ifdef NS_COUNT
            atomicAdd(&g_ns_bscnt[6], 1ull);
#endif
        }
    }
}

// AFTER as in k_sd_select: last[blockIdx.x] bounds the keys that may enter, and the item's count of such keys goes into
// rest[query].  Wave 0's own slot of s_rows is never read back, so under AFTER it is not written and its first word holds the
// item's count instead.  With AFTER = false neither pointer is read.
template <bool AFTER, bool GROUPED = false, bool QUORUM = false>
__global__ void __launch_bounds__(256) k_bs_select(const FcItem* __restrict__ items, const BqRef* __restrict__ refs,
                                                   const DevFcSeg* __restrict__ segs, const DevSdSeg* __restrict__ sds, uint32_t K,
                                                   uint32_t asc, uint64_t* __restrict__ cand, unsigned long long* __restrict__ found,
                                                   const uint64_t* __restrict__ last_of, unsigned long long* __restrict__ rest) {
    __shared__ uint32_t s_bm[kFcTileDocs / 32u];
    __shared__ uint32_t s_tmp[kFcTileDocs / 32u];
    __shared__ uint64_t s_rows[4][128];
    __shared__ uint32_t s_cnt;
    extern __shared__ __attribute__((aligned(16))) uint32_t s_bs_planes[];   // QUORUM: 16 KiB per plane of the launch, else none
    const FcItem it = items[blockIdx.x];
    const DevFcSeg sg = segs[it.seg];
    const BqRef* __restrict__ rf = refs + it.ref_begin;
    const uint32_t* __restrict__ keys = sds[it.seg].keys;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, v = tid >> 6;
    const uint32_t n_words = (it.doc_hi - it.doc_lo + 31u) / 32u;   // <= kFcTileDocs / 32: the tile is the host's, at most the product's
    NS_BSCNT(0, 1);
    NS_BGCNT(5, 1);
    if (QUORUM) NS_BQCNT(6, 1);
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
        fc_cut(sg, rf[0].list, it.doc_lo, it.doc_hi, lane, lo, hi);
        NS_BSCNT(1, 1);
        NS_BGCNT(10, 1);
        for (uint64_t base = lo + v * 64u; base < hi; base += 256u) {   // (wave-uniform)
            const uint64_t i = base + lane;
            uint64_t key = 0;
            if (i < hi) {
                const uint32_t d = sg.postings[i].x;
                if (d >= it.doc_lo && d < it.doc_hi) { cnt++; key = sd_key(keys[d], d - it.doc_lo, asc != 0u); }
            }
            if (AFTER) key = af_clip(key, last, kept);
            bs_insert(set, key, K, lane);
        }
    } else if (bs_matched<GROUPED, QUORUM>(it, sg, rf, n_words, s_bm, s_tmp, QUORUM ? s_bs_planes : nullptr)) { // (workgroup-uniform)
        for (uint32_t wb = v * 64u; wb < n_words; wb += 256u) {         // (wave-uniform)
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
                bs_insert(set, key, K, lane);
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
        bs_insert(set, s_rows[o][lane], K, lane);
        if (K > 64u) bs_insert(set, s_rows[o][64u + lane], K, lane);
    }
    uint64_t* __restrict__ row = cand + (size_t)blockIdx.x * K;
    if (lane < K) row[lane] = set.hi;
    if (64u + lane < K) row[64u + lane] = set.lo;
}

// One wave per (query, hit), as k_sd_score; roles is parallel to terms (nullptr: all SHOULD).  The refs of the hit's segment
// whose role is not NOT add in query order, duplicates included: ns_search_boolean's score, bit for bit.
__global__ void __launch_bounds__(256) k_bs_score(const ns_query_desc* __restrict__ queries, const ns_term_ref* __restrict__ terms,
                                                  const uint8_t* __restrict__ roles, uint32_t q_begin, uint32_t q_end,
                                                  const DevFcSeg* __restrict__ segs, const DevSdSeg* __restrict__ sds, uint32_t K,
                                                  const uint32_t* __restrict__ pos_out, const uint32_t* __restrict__ nhits,
                                                  uint32_t* __restrict__ hits) {
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
        if (roles && roles[j] == kBqNot) { NS_BSCNT_WAVE(11, 1); continue; }
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
        if (hit) NS_BSCNT_WAVE(9, 1); else NS_BSCNT_WAVE(10, 1);
    }
    if (lane == 0) hits[at * 3u + 0u] = __float_as_uint(acc);
}

}  // namespace ns
