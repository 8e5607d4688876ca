// SPDX-License-Identifier: MIT
// Boolean queries: every term ref has a role (SHOULD, MUST, NOT); per query the K best documents of the
// matched set by BM25 score, in the search's canonical order (score descending, position of the segment in the call's list
// ascending, docId ascending).  The work items are bq_plan's (ns_boolean_plan.hpp): one (query, segment) group over one
// tile of the facet tile size; the sub-batches are ns_sorted_plan.hpp's.  The scoring launch (k_uscore) is not involved.
//   k_bq_select   one workgroup of 256 threads per item.  The tile is walked in windows of `win` documents (kBqWinDocs in
//                 the product); per window, in LDS: an fp32 accumulator per document, the matched bitmap, a scratch bitmap
//                 and the excluded bitmap.
//                   cut     every list to the window (fc_cut), once per pass that reads it
//                   mark    MUST lists: the first marks the matched bitmap, every further one the scratch bitmap, which is
//                           AND-ed in and cleared (as k_sd_select<true>); a MUST list without a posting in the window ends
//                           the window.  No MUST ref: SHOULD lists mark the matched bitmap.  NOT lists mark the excluded
//                           bitmap; matched &= ~excluded.  A window without a matched bit ends here (workgroup-uniform).
//                           GROUPED (§5u): a required clause is a SET of MUST lists; the lists of a clause are OR-ed into one
//                           bitmap before the AND (see the template parameter below).
//                   score   the MUST and SHOULD refs in query order, one at a time, a barrier in between: every posting of
//                           the window whose document is matched does a plain LDS read-add-write
//                               acc[doc] = acc[doc] + qweight * ((idf * (tf * 2.2f)) / (tf + norm[doc]))   each op rounds to fp32
//                           docIds are unique within a list, so no two threads meet on a document; term by term is the
//                           scoring path's fp32 order; a list named twice adds twice.
//                   sweep   a wave takes 64 bitmap words at a time, one per lane; every lane pops its lowest set bit and offers
//                               (ord(score) << 32) | ~(docId - doc_lo)        distinct per document of the tile, never 0
//                           to the wave's kept set (§5q's SdSet / sd_insert), which lives across the windows of the item.
//                 The four waves' sets meet in LDS, wave 0 joins them and writes the item's row of K candidates (0 = none).
//                 The item's matched count goes into found[query] with one integer atomic.
//   k_bq_join     one wave per query over the rows of its items (contiguous, in plan order: segment position, then tile):
//                 k_sd_join's scheme, with the score taken back out of the key.  Writes the final row, nhits and the pad.
// ord is the order-preserving map of fp32 bits: negative -> ~bits, else bits | 0x80000000.  The accumulator starts at +0.0f
// and x + y is -0.0f only for x = y = -0.0f, so no score is a negative zero and ord orders as floats compare.
// Every docId read from a list is tested against the window before it indexes LDS; a list that is not ascending may lose
// hits but reads and writes nothing out of bounds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ns_boolean_plan.hpp"
#include "ns_collapse_plan.hpp"   // cl_others_seed (host and device)

namespace ns {

struct DevBqSeg {
    const float* norm;   // per document (ns_seg::d_norm)
    uint32_t seg_id;     // the id the refs use for this segment
    uint32_t boost_at;   // BOOST launches (§5z): entry boost_at of this array, read as a DevBqBoost, is segment 0's; else 0
};
// Per-document factors (§5z, ns_docboost): a sibling of DevBqSeg of the same size, so that the array of a BOOST launch carries
// n_segs DevBqSeg and then n_segs DevBqBoost, and DevBqSeg keeps its 16 bytes for every other launch.
struct DevBqBoost {
    const float* boost;  // per document: at least the segment's n_docs finite factors without a sign bit
    uint64_t pad;
};
static_assert(sizeof(DevBqBoost) == sizeof(DevBqSeg), "the two share one array");
// Per-document groups (§5ac, ns_search_collapsed): a third sibling.  The array of a COLLAPSE launch carries n_segs DevBqSeg, n_segs
// DevBqBoost (read by its BOOST instantiations alone) and n_segs DevBqGroup; boost_at = n_segs in every entry, so segment s's
// group table is entry 2 * boost_at + s.
struct DevBqGroup {
    const uint32_t* group;  // per document: the segment's n_docs keys of an ns_dockeys table (0 = stands alone)
    uint64_t pad;
};
static_assert(sizeof(DevBqGroup) == sizeof(DevBqSeg), "the three share one array");
__device__ __forceinline__ const uint32_t* bq_group_table(const DevBqSeg* __restrict__ bqs, uint32_t seg) {
    return reinterpret_cast<const DevBqGroup*>(bqs)[2u * bqs[seg].boost_at + seg].group;
}

#ifdef NS_COUNT
// Counting build only: events of the two kernels since the last reset (ns_debug_boolean_counters).  0 items, 1 windows,
// 2 windows left early for an empty matched set, 3 MUST intersections (a further MUST list AND-ed in), 4 windows in which an
// exclusion cleared a bit, 5 chunks skipped on the threshold ballot, 6 chunks that inserted, 7 rows joined.
constexpr int kNsBcnt = 8;
__device__ unsigned long long g_ns_bcnt[kNsBcnt];
#define NS_BCNT(i, v) do { if (threadIdx.x == 0) atomicAdd(&g_ns_bcnt[(i)], (unsigned long long)(v)); } while (0)
#define NS_BCNT_WAVE(i, v) do { if ((threadIdx.x & 63u) == 0) atomicAdd(&g_ns_bcnt[(i)], (unsigned long long)(v)); } while (0)
// Grouped clauses (§5u; ns_debug_boolean_groups_counters), the GROUPED instantiations only.  k_bq_select<., true>: 0 work items
// (one per workgroup); then, counted per window, 1 clauses marked from two or more lists with a posting in the window, 2 clause
// intersections, 3 windows ended by a clause without a posting, 4 clause members that missed a window their clause still hit.
// The set kernels (ns_boolean_sets.hip): 5 work items; 6..9 as 1..4, counted per tile (= per item); 10 items on the single-list path.
constexpr int kNsBgcnt = 11;
__device__ unsigned long long g_ns_bgcnt[kNsBgcnt];
#define NS_BGCNT(i, v) do { if (GROUPED && threadIdx.x == 0) atomicAdd(&g_ns_bgcnt[(i)], (unsigned long long)(v)); } while (0)
// At-least-m-of-n clauses (§5w; ns_debug_boolean_quorum_counters), the QUORUM instantiations only.  k_bq_select<., ., true>: 0 work
// items; then, counted per window, 1 clauses counted (need > 1), 2 list additions into the planes, 3 additions that saturated a
// bit, 4 windows ended because fewer lists of a clause hit than it needs, 5 non-counting duplicates skipped.  The set kernels
// (ns_boolean_sets.hip): 6 work items; 7..11 as 1..5, counted per tile (= per item).
constexpr int kNsBqcnt = 12;
__device__ unsigned long long g_ns_bqcnt[kNsBqcnt];
#define NS_BQCNT(i, v) do { if (threadIdx.x == 0) atomicAdd(&g_ns_bqcnt[(i)], (unsigned long long)(v)); } while (0)
// Per-document factors (§5z; ns_debug_boolean_boost_counters), the BOOST instantiations of k_bq_select only: 0 work items, 1 items
// swept (at least one window reached the sweep), 2 documents whose score was multiplied, 3 boosted keys a cursor clipped, 4 swept
// windows in which every matched document's factor is 0.0f, 5..7 the work items of <true, false, false, true>, <true, true, false,
// true> and <true, true, true, true>.
constexpr int kNsBbcnt = 8;
__device__ unsigned long long g_ns_bbcnt[kNsBbcnt];
#define NS_BBCNT(i, v) do { if (BOOST && threadIdx.x == 0) atomicAdd(&g_ns_bbcnt[(i)], (unsigned long long)(v)); } while (0)
// One hit per group (§5ac; ns_debug_collapse_counters), the COLLAPSE instantiations of k_bq_select, k_bq_join_collapsed and
// ns_collapse.hip's k_cl_count.  Counted per wave: 0 rounds of 64 skipped on the threshold ballot, 1 candidates dropped because their
// group's kept entry is better, 2 replacements, 3 replacements or evictions that moved an entry across the hi / lo register
// boundary, 4 fresh insertions, 5 key-0 candidates that beat the threshold, 6 rounds in which two survivors carry one group,
// 7 duplicates met while the four waves' sets are merged, 8 join duplicates from two tiles of one segment, 9 join duplicates
// from two segments.  10 documents the count pass counted, 11 work items it skipped (no grouped hit), 12 work items of the
// collapsing select, 13 work items of the count pass.
constexpr int kNsClcnt = 14;
__device__ unsigned long long g_ns_clcnt[kNsClcnt];
#define NS_CLCNT(i, v) do { if (threadIdx.x == 0) atomicAdd(&g_ns_clcnt[(i)], (unsigned long long)(v)); } while (0)
#define NS_CLCNT_WAVE(i, v) do { if ((threadIdx.x & 63u) == 0) atomicAdd(&g_ns_clcnt[(i)], (unsigned long long)(v)); } while (0)
#else
#define NS_BCNT(i, v)
#define NS_BCNT_WAVE(i, v)
#define NS_BGCNT(i, v)
#define NS_BQCNT(i, v)
#define NS_BBCNT(i, v)
#define NS_CLCNT(i, v)
#define NS_CLCNT_WAVE(i, v)
#endif

__device__ __forceinline__ uint32_t bq_ord(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ uint32_t bq_unord(uint32_t o) { return (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o; }

// sd_insert, counting into this file's counters (the sorted search's stay its own)
__device__ __forceinline__ void bq_insert(SdSet& s, uint64_t key, uint32_t K, uint32_t lane) {
#ifdef NS_COUNT
    const uint64_t thr = K <= 64u ? ml_shfl(s.hi, K - 1u) : ml_shfl(s.lo, K - 65u);
    if (__ballot(key > thr) == 0ull) { NS_BCNT_WAVE(5, 1); return; }   // (wave-uniform; sd_insert would return here too)
    NS_BCNT_WAVE(6, 1);
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

// The collapsing kept set (§5ac): SdSet with a 32-bit group next to each key.  INVARIANT: slots 0 .. K - 1 (hi lane 0 .. 63, then lo
// lane 0 .. 63) hold distinct keys, descending, 0 = none and then nothing behind it; no two of them carry the same non-zero
// group; slots K .. 127 are empty.  Group 0 stands alone: it never equals a kept group.
struct CgSet {
    uint64_t hi, lo;
    uint32_t ghi, glo;
};
__device__ __forceinline__ uint64_t cg_shfl_up1(uint64_t key) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)key, 1u, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(key >> 32), 1u, 64);
    return ((uint64_t)hi << 32) | lo;
}
// One candidate, the same in all 64 lanes (key != 0).  p: the slot of the group's kept entry, or K - 1, the slot a fresh entry
// pushes out.  ins: how many kept keys are larger, the slot the candidate would take.  ins > p: the group's entry is better, or K
// kept keys are; nothing changes.  Else the candidate takes slot ins, the entries of [ins, p) move down by one, and what was in
// slot p (the group's worse entry, or the K-th key) is gone: one group less or the same groups, still sorted.
// STAGE (the counting build's): 0 the sweep, 1 the merge of the four waves' sets, 2 the join; dup_low: the low word of the kept
// entry a duplicate met, else untouched.  Returns whether the candidate's group was kept already.
template <int STAGE>
__device__ __forceinline__ bool cg_insert_one(CgSet& s, uint64_t key, uint32_t g, uint32_t K, uint32_t lane, uint32_t& dup_low) {
    const unsigned long long mh = __ballot(g != 0u && s.hi != 0ull && s.ghi == g);
    const unsigned long long ml = K > 64u ? __ballot(g != 0u && s.lo != 0ull && s.glo == g) : 0ull;
    const bool dup = (mh | ml) != 0ull;
    const uint32_t p = mh ? (uint32_t)__builtin_ctzll(mh) : ml ? 64u + (uint32_t)__builtin_ctzll(ml) : K - 1u;
    uint32_t ins = (uint32_t)__popcll(__ballot(s.hi > key));
    if (K > 64u) ins += (uint32_t)__popcll(__ballot(s.lo > key));
#ifdef NS_COUNT
    if (dup) dup_low = p < 64u ? (uint32_t)ml_shfl(s.hi, p) : (uint32_t)ml_shfl(s.lo, p - 64u);
    if (g == 0u) NS_CLCNT_WAVE(5, 1);
    if (dup && STAGE == 1) NS_CLCNT_WAVE(7, 1);
    if (dup && ins > p) NS_CLCNT_WAVE(1, 1);
    if (dup && ins <= p) NS_CLCNT_WAVE(2, 1);
    if (!dup && ins <= p) NS_CLCNT_WAVE(4, 1);
    if (ins < 64u && p >= 64u) NS_CLCNT_WAVE(3, 1);   // (ins <= p: what was in hi lane 63 is in lo lane 0 afterwards)
#else
    (void)dup_low;
#endif
    if (ins > p) return dup;                            // (wave-uniform)
    if (K > 64u && p >= 64u) {                          // lo first: it takes hi's last entry as it still is
        const uint32_t i = 64u + lane;
        const uint64_t from_hi = ml_shfl(s.hi, 63u), up = cg_shfl_up1(s.lo);
        const uint32_t g_from_hi = (uint32_t)__shfl((int)s.ghi, 63, 64), g_up = (uint32_t)__shfl_up((int)s.glo, 1u, 64);
        if (i == ins) { s.lo = key; s.glo = g; }
        else if (i > ins && i <= p) { s.lo = lane ? up : from_hi; s.glo = lane ? g_up : g_from_hi; }
    }
    if (ins < 64u) {
        const uint64_t up = cg_shfl_up1(s.hi);
        const uint32_t g_up = (uint32_t)__shfl_up((int)s.ghi, 1u, 64);
        if (lane == ins) { s.hi = key; s.ghi = g; }
        else if (lane > ins && lane <= p) { s.hi = up; s.ghi = g_up; }
    }
    return dup;
}
// Offers one (key, group) per lane (any order, key 0 = none).  All 64 lanes call it together.  The threshold skip is sd_insert's:
// a key at or below the K-th kept key cannot enter on its own and cannot be its group's best among the kept, whose keys are all
// above it.  The survivors of the ballot are taken one at a time in lane order, so a second member of a group finds the first in
// the set; a survivor the growing threshold has overtaken meanwhile drops out at ins > p.
// on_dup(low): called (wave-uniformly) for every survivor whose group was kept already, with the low word of the kept entry it met;
// the counting build's join tells the two kinds of duplicate apart with it, every other caller passes nothing (CgNoDup).
struct CgNoDup { __device__ __forceinline__ void operator()(uint32_t) const {} };
template <int STAGE, class OnDup = CgNoDup>
__device__ __forceinline__ void cg_insert(CgSet& s, uint64_t key, uint32_t g, uint32_t K, uint32_t lane, OnDup on_dup = OnDup()) {
    const uint64_t thr = K <= 64u ? ml_shfl(s.hi, K - 1u) : ml_shfl(s.lo, K - 65u);   // the current K-th key (0 while fewer are kept)
    unsigned long long live = __ballot(key > thr);
    if (live == 0ull) { NS_CLCNT_WAVE(0, 1); return; }                                // (wave-uniform)
#ifdef NS_COUNT
    bool pair = false;
    const unsigned long long all = live;
#endif
    while (live) {
        const uint32_t l = (uint32_t)__builtin_ctzll(live);
        live &= live - 1ull;
        const uint64_t k1 = ml_shfl(key, l);
        const uint32_t g1 = (uint32_t)__shfl((int)g, (int)l, 64);
#ifdef NS_COUNT
        pair = pair || (g1 != 0u && (__ballot(g == g1 && lane > l) & all) != 0ull);
#endif
        uint32_t low = 0;
        if (cg_insert_one<STAGE>(s, k1, g1, K, lane, low)) on_dup(low);
    }
#ifdef NS_COUNT
    if (pair) NS_CLCNT_WAVE(6, 1);
#endif
}

// The grouped required stage (§5u) over the documents [doc_lo, doc_hi) (a window of k_bq_select, a tile of bs_matched), called by
// all 256 threads in workgroup-uniform control flow.  For clause c = 0, 1, ... every list of the clause with a posting in the range
// marks one bitmap (s_bm for c = 0, s_tmp after it) with fc_mark's atomic ORs, no barrier between the lists; then one barrier, and
// for c > 0 the AND, the clearing of s_tmp and a second barrier.  False (in every thread) when a clause has no posting in the range:
// nothing was marked for it, s_tmp is clear, and s_bm is not to be read.  A list that misses while another of its clause hits
// does not end it.  The members of a clause need not be neighbours (the refs stay in query order, which is the score's):
//   at most 64 refs   `mine` holds, per lane, the clause index of ref `lane` (bq_clause_of_lane: read ONCE per item), and a ballot
//                     names the members of clause c; the loop then reads the refs it cuts and no other
//   more than 64      the refs are scanned from the clause's first ref on; the numbering by first appearance puts the first ref
//                     of clause c + 1 behind it
// BASE: the first of the four counters (ns_debug_boolean_groups_counters) of the caller.
constexpr uint32_t kBqNoClause = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t bq_clause_of_lane(const BqRef* __restrict__ rf, uint32_t ref_count, uint32_t lane) {
    return (lane < ref_count && rf[lane].role == kBqMust) ? rf[lane].clause : kBqNoClause;
}
template <int BASE>
__device__ __forceinline__ bool bq_mark_clauses(const DevFcSeg& sg, const BqRef* __restrict__ rf, uint32_t ref_count, uint32_t n_clauses,
                                                uint32_t mine, uint32_t doc_lo, uint32_t doc_hi, uint32_t n_words, uint32_t* s_bm,
                                                uint32_t* s_tmp) {
    constexpr bool GROUPED = true;   // (NS_BGCNT counts in the grouped instantiations only)
    (void)GROUPED;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t from = 0;
    for (uint32_t c = 0; c < n_clauses; c++) {
        uint32_t hit = 0, missed = 0;   // lists of the clause with / without a posting in the range
        uint32_t* const bm = c == 0u ? s_bm : s_tmp;
        if (ref_count <= 64u) {
            unsigned long long members = __ballot(mine == c);   // (wave-uniform, and the same in all four waves)
            while (members) {
                const uint32_t r = (uint32_t)__builtin_ctzll(members);
                members &= members - 1ull;
                uint64_t lo, hi;
                fc_cut(sg, rf[r].list, doc_lo, doc_hi, lane, lo, hi);
                if (lo == hi) { missed++; continue; }
                fc_mark(sg.postings, lo, hi, doc_lo, doc_hi, bm);
                hit++;
            }
        } else {
            uint32_t next = ref_count;
            for (uint32_t r = from; r < ref_count; r++) {
                const BqRef b = rf[r];
                if (b.role != kBqMust) continue;
                if (b.clause != c) { if (b.clause == c + 1u && next == ref_count) next = r; continue; }
                uint64_t lo, hi;
                fc_cut(sg, b.list, doc_lo, doc_hi, lane, lo, hi);
                if (lo == hi) { missed++; continue; }
                fc_mark(sg.postings, lo, hi, doc_lo, doc_hi, bm);
                hit++;
            }
            from = next;
        }
        if (!hit) { NS_BGCNT(BASE + 2, 1); return false; }   // (workgroup-uniform: the cuts depend on the item and the range alone)
        if (hit > 1u) NS_BGCNT(BASE, 1);
        if (missed) NS_BGCNT(BASE + 3, missed);
        __syncthreads();
        if (c) {
            for (uint32_t w = tid; w < n_words; w += 256u) {
                s_bm[w] &= s_tmp[w];
                s_tmp[w] = 0u;
            }
            __syncthreads();
            NS_BGCNT(BASE + 1, 1);
        }
    }
    return true;
}

// The quorum required stage (§5w): bq_mark_clauses with a need per clause (bq_clause_need of the members' BqRef::clause, the same in
// all of them: bq_plan_quorum), over the same range, with the same callers' contract: workgroup-uniform, false (in every thread)
// when a clause cannot hold in the range, s_tmp clear on return either way.  `mine` holds the lane's whole clause word.
//   need 1   bq_mark_clauses' path: the clause's lists mark its bitmap directly
//   need m   every counting list with a posting in the range is marked into s_tmp with fc_mark; a barrier; a word-wise pass adds
//            the scratch word into the p = bq_need_planes(m) bit-sliced counter planes (plane i holds bit i of every document's
//            count) with a ripple-carry add that SATURATES: a carry out of the top plane sets all planes for those bits, so a count
//            stays at 2^p - 1 >= m; the pass clears the scratch word; a second barrier.  After the last list a word-wise compare
//            of the planes against m gives the clause's set, which becomes s_bm for c = 0 and is AND-ed into it afterwards.
// A ref with kBqDupBit is skipped: an earlier ref of the clause named its list.  Fewer than m counting lists with a posting in the
// range end it (m = 1: "no list hits").  The planes (s_pl: p arrays, `stride` words apart) are cleared before a clause counts into
// them, so nothing is assumed about what an earlier clause, window or early exit left there; words past n_words are never touched.
// BASE: the first of the five counters (ns_debug_boolean_quorum_counters) of the caller.
template <int BASE>
__device__ __forceinline__ bool bq_count_clauses(const DevFcSeg& sg, const BqRef* __restrict__ rf, uint32_t ref_count, uint32_t n_clauses,
                                                 uint32_t mine, uint32_t doc_lo, uint32_t doc_hi, uint32_t n_words, uint32_t* s_bm,
                                                 uint32_t* s_tmp, uint32_t* s_pl, uint32_t stride) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t from = 0;
    for (uint32_t c = 0; c < n_clauses; c++) {
        unsigned long long members = 0ull;   // at most 64 refs: the clause's refs (wave-uniform, and the same in all four waves)
        uint32_t need = 1u;
        if (ref_count <= 64u) {
            members = __ballot(mine != kBqNoClause && bq_clause_index(mine) == c);
            if (!members) return false;      // (never: the indices are dense)
            need = bq_clause_need(rf[(uint32_t)__builtin_ctzll(members)].clause);
        } else {
            while (from < ref_count && !(rf[from].role == kBqMust && bq_clause_index(rf[from].clause) == c)) from++;
            if (from == ref_count) return false;   // (never)
            need = bq_clause_need(rf[from].clause);
        }
        const uint32_t planes = bq_need_planes(need);   // 0, 2 or 3 (workgroup-uniform, as `need`)
        uint32_t* const bm = c == 0u ? s_bm : s_tmp;
        uint32_t hit = 0, skipped = 0;
        if (planes) {
            for (uint32_t i = 0; i < planes; i++)
                for (uint32_t w = tid; w < n_words; w += 256u) s_pl[i * stride + w] = 0u;
            NS_BQCNT(BASE, 1);
        }
        // one list of the clause (workgroup-uniform)
        auto take = [&](const BqRef& b) {
            if (b.clause & kBqDupBit) { skipped++; return; }
            uint64_t lo, hi;
            fc_cut(sg, b.list, doc_lo, doc_hi, lane, lo, hi);
            if (lo == hi) return;
            hit++;
            if (!planes) { fc_mark(sg.postings, lo, hi, doc_lo, doc_hi, bm); return; }
            fc_mark(sg.postings, lo, hi, doc_lo, doc_hi, s_tmp);
            __syncthreads();
            bool full = false;
            for (uint32_t w = tid; w < n_words; w += 256u) {
                uint32_t carry = s_tmp[w];
                if (!carry) continue;
                s_tmp[w] = 0u;
                for (uint32_t i = 0; i < planes; i++) {
                    const uint32_t x = s_pl[i * stride + w];
                    s_pl[i * stride + w] = x ^ carry;
                    carry &= x;
                }
                if (carry) {   // these documents were at 2^p - 1: they stay there
                    full = true;
                    for (uint32_t i = 0; i < planes; i++) s_pl[i * stride + w] |= carry;
                }
            }
#ifdef NS_COUNT
            if (__syncthreads_or(full ? 1 : 0)) NS_BQCNT(BASE + 2, 1);
            NS_BQCNT(BASE + 1, 1);
#else
            (void)full;
            __syncthreads();
#endif
        };
        if (ref_count <= 64u) {
            while (members) {
                const uint32_t r = (uint32_t)__builtin_ctzll(members);
                members &= members - 1ull;
                take(rf[r]);
            }
        } else {
            uint32_t next = ref_count;
            for (uint32_t r = from; r < ref_count; r++) {
                const BqRef b = rf[r];
                if (b.role != kBqMust) continue;
                const uint32_t at = bq_clause_index(b.clause);
                if (at != c) { if (at == c + 1u && next == ref_count) next = r; continue; }
                take(b);
            }
            from = next;
        }
        if (skipped) NS_BQCNT(BASE + 4, skipped);
        if (hit < need) { NS_BQCNT(BASE + 3, 1); return false; }   // (workgroup-uniform: the cuts depend on the item and the range alone)
        if (planes) {
            for (uint32_t w = tid; w < n_words; w += 256u) {
                uint32_t ge = 0xFFFFFFFFu;   // count >= need, from the lowest bit up
                for (uint32_t i = 0; i < planes; i++) {
                    const uint32_t x = s_pl[i * stride + w];
                    ge = ((need >> i) & 1u) ? (x & ge) : (x | ge);
                }
                s_bm[w] = c ? (s_bm[w] & ge) : ge;
            }
            __syncthreads();
        } else {
            __syncthreads();
            if (c) {
                for (uint32_t w = tid; w < n_words; w += 256u) {
                    s_bm[w] &= s_tmp[w];
                    s_tmp[w] = 0u;
                }
                __syncthreads();
            }
        }
    }
    return true;
}

// Dynamic LDS, and no static LDS in front of it, so that the 8-byte rows stay aligned: 4 KiB row exchange, then win x 4 B
// accumulators, then three bitmaps of win / 8 B, then the item's matched count.
__host__ __device__ inline size_t bq_lds_bytes(uint32_t win) { return 4096u + (size_t)win * 4u + 3u * (size_t)(win / 8u) + 16u; }
// QUORUM (§5w): the counter planes follow, win / 8 B each, as many as the launch's largest need asks for (none when it is 1)
__host__ __device__ inline size_t bq_quorum_lds_bytes(uint32_t win, uint32_t planes) { return bq_lds_bytes(win) + (size_t)planes * (win / 8u); }

// AFTER (§5s, ns_after.hip): last[blockIdx.x] bounds the keys that may enter, and the item's count of such keys goes into
// rest[query] through the word behind s_cnt.  With AFTER = false neither pointer is read and the code is what it was without
// the parameter.
// GROUPED (§5u): the MUST refs carry a clause index (BqRef::clause, dense per group: bq_plan_grouped), and the required stage
// of a window is bq_mark_clauses: a clause NONE of whose lists has a posting in the window ends the window.  With GROUPED = false
// the code is what it was without the parameter.
// QUORUM (§5w; implies GROUPED): BqRef::clause is bq_plan_quorum's word, and the required stage of a window is bq_count_clauses
// over the counter planes behind bq_lds_bytes(win).  With QUORUM = false the code is what it was without the parameter.
// BOOST (§5z; instantiated with AFTER alone, a call without a cursor passes kAfterAll for every item): in the sweep the lane that
// owns a set bit gathers its document's factor from the segment's DevBqBoost (one dependent 4-byte global load per matched
// document, as k_sd_select gathers its key) and the key carries ord(fp32(score * factor)).  The score is the FINISHED sum: the
// score stage stored it to LDS and a barrier lies in between, so the multiply is one rounding of its own and cannot be contracted
// into the last accumulation (it is written __fmul_rn all the same).  A negative score times 0.0f is -0.0f, which ord puts just
// below +0.0f.  With BOOST = false the code is what it was without the parameter.
// COLLAPSE (§5ac, ns_search_collapsed; instantiated without AFTER: the call has no cursor): in the sweep the lane that owns a set bit
// gathers its document's group from the segment's DevBqGroup, 4 bytes next to the factor, and the keys go through the collapsing
// set (CgSet / cg_insert) in place of SdSet.  The four waves' sets meet in s_rows as keys alone: wave 0 gathers a key's group again
// by the docId in its low word, so the LDS is what it was.  The item's row holds the tile's best K groups by their tile-best
// document, keys alone.  With COLLAPSE = false the code is what it was without the parameter.
template <bool AFTER, bool GROUPED = false, bool QUORUM = false, bool BOOST = false, bool COLLAPSE = false>
__global__ void __launch_bounds__(256) k_bq_select(const FcItem* __restrict__ items, const BqRef* __restrict__ refs,
                                                   const DevFcSeg* __restrict__ segs, const DevBqSeg* __restrict__ bqs, uint32_t K,
                                                   uint32_t win, uint64_t* __restrict__ cand, unsigned long long* __restrict__ found,
                                                   const uint64_t* __restrict__ last_of, unsigned long long* __restrict__ rest) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    uint64_t (*s_rows)[128] = reinterpret_cast<uint64_t (*)[128]>(s_raw);
    float* s_acc = reinterpret_cast<float*>(s_raw + 4096u);
    uint32_t* s_bm = reinterpret_cast<uint32_t*>(s_raw + 4096u + (size_t)win * 4u);
    uint32_t* s_tmp = s_bm + win / 32u;
    uint32_t* s_ex = s_tmp + win / 32u;
    uint32_t& s_cnt = s_ex[win / 32u];
    uint32_t& s_rest = s_ex[win / 32u + 1u];   // (inside bq_lds_bytes' last 16 bytes)
    uint32_t* const s_pl = reinterpret_cast<uint32_t*>(s_raw + bq_lds_bytes(win));   // QUORUM: the planes, if the launch has any
    const FcItem it = items[blockIdx.x];
    const DevFcSeg sg = segs[it.seg];
    const float* __restrict__ norm = bqs[it.seg].norm;
    const float* __restrict__ boost = BOOST ? reinterpret_cast<const DevBqBoost*>(bqs)[bqs[it.seg].boost_at + it.seg].boost : nullptr;
    static_assert(!(COLLAPSE && AFTER), "the collapsed call has no cursor");
    const uint32_t* __restrict__ grp = COLLAPSE ? bq_group_table(bqs, it.seg) : nullptr;
    const BqRef* __restrict__ rf = refs + it.ref_begin;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, v = tid >> 6;
    NS_BCNT(0, 1);
    if (COLLAPSE) NS_CLCNT(12, 1);
    NS_BBCNT(0, 1);
    NS_BBCNT(QUORUM ? 7 : GROUPED ? 6 : 5, 1);
    if (tid == 0) s_cnt = 0u;
    uint64_t last = kAfterAll;
    uint32_t kept = 0;
    if (AFTER) {
        last = last_of[blockIdx.x];
        if (tid == 0) s_rest = 0u;
        af_count_item(last);
    }
    uint32_t n_must = 0, n_not = 0;   // the same in every thread: they depend on the item alone
    uint32_t n_clauses = 0;           // GROUPED: 1 + the largest clause index of a MUST ref
    for (uint32_t r = 0; r < it.ref_count; r++) {
        const uint32_t role = rf[r].role;
        n_must += role == kBqMust;
        n_not += role == kBqNot;
        if (GROUPED && role == kBqMust) n_clauses = max(n_clauses, (QUORUM ? bq_clause_index(rf[r].clause) : rf[r].clause) + 1u);
    }
    const uint32_t my_clause = GROUPED ? bq_clause_of_lane(rf, it.ref_count, lane) : 0u;   // (once per item, not per window)
    NS_BGCNT(0, 1);
    if (QUORUM) NS_BQCNT(0, 1);
    SdSet set{0ull, 0ull};
    CgSet cset{0ull, 0ull, 0u, 0u};   // COLLAPSE: in place of `set`
    uint32_t cnt = 0;
#ifdef NS_COUNT
    bool swept = false;   // BOOST: a window of the item reached the sweep (workgroup-uniform)
#endif
    const uint32_t tile_n = it.doc_hi - it.doc_lo;   // <= kFcTileDocs: the tile is the host's
    for (uint32_t tile_rel = 0; tile_rel < tile_n; tile_rel += win) {   // (tile_rel + win <= 2^17 + 2^15: no wrap)
        const uint32_t w_lo = it.doc_lo + tile_rel;
        const uint32_t w_hi = tile_n - tile_rel > win ? w_lo + win : it.doc_hi;
        const uint32_t n = w_hi - w_lo, n_words = (n + 31u) / 32u;      // n <= win
        __syncthreads();   // the sweep of the window before is through
        for (uint32_t i = tid; i < n; i += 256u) s_acc[i] = 0.0f;
        for (uint32_t w = tid; w < n_words; w += 256u) {
            s_bm[w] = 0u;
            s_tmp[w] = 0u;
            s_ex[w] = 0u;
        }
        __syncthreads();
        NS_BCNT(1, 1);
        bool alive = true;   // workgroup-uniform: the cuts depend on the item and the window alone
        if (QUORUM && n_must) {
            alive = bq_count_clauses<1>(sg, rf, it.ref_count, n_clauses, my_clause, w_lo, w_hi, n_words, s_bm, s_tmp, s_pl, win / 32u);
        } else if (GROUPED && n_must) {
            alive = bq_mark_clauses<1>(sg, rf, it.ref_count, n_clauses, my_clause, w_lo, w_hi, n_words, s_bm, s_tmp);
        } else if (n_must) {
            uint32_t seen = 0;
            for (uint32_t r = 0; r < it.ref_count; r++) {
                const BqRef b = rf[r];
                if (b.role != kBqMust) continue;
                uint64_t lo, hi;
                fc_cut(sg, b.list, w_lo, w_hi, lane, lo, hi);
                if (lo == hi) { alive = false; break; }
                if (seen == 0u) {
                    fc_mark(sg.postings, lo, hi, w_lo, w_hi, s_bm);
                    __syncthreads();
                } else {
                    fc_mark(sg.postings, lo, hi, w_lo, w_hi, s_tmp);
                    __syncthreads();
                    for (uint32_t w = tid; w < n_words; w += 256u) {
                        s_bm[w] &= s_tmp[w];
                        s_tmp[w] = 0u;
                    }
                    __syncthreads();
                    NS_BCNT(3, 1);
                }
                seen++;
            }
        } else {
            for (uint32_t r = 0; r < it.ref_count; r++) {
                const BqRef b = rf[r];
                if (b.role != kBqShould) continue;
                uint64_t lo, hi;
                fc_cut(sg, b.list, w_lo, w_hi, lane, lo, hi);
                fc_mark(sg.postings, lo, hi, w_lo, w_hi, s_bm);
            }
            __syncthreads();
        }
        if (alive && n_not) {
            for (uint32_t r = 0; r < it.ref_count; r++) {
                const BqRef b = rf[r];
                if (b.role != kBqNot) continue;
                uint64_t lo, hi;
                fc_cut(sg, b.list, w_lo, w_hi, lane, lo, hi);
                fc_mark(sg.postings, lo, hi, w_lo, w_hi, s_ex);
            }
            __syncthreads();
            bool cleared = false;
            for (uint32_t w = tid; w < n_words; w += 256u) {
                const uint32_t m = s_bm[w], x = s_ex[w];
                cleared = cleared || (m & x) != 0u;
                s_bm[w] = m & ~x;
            }
#ifdef NS_COUNT
            if (__syncthreads_or(cleared ? 1 : 0)) NS_BCNT(4, 1);
#else
            (void)cleared;
#endif
        }
        int mine = 0;   // a thread tests the words it wrote last itself
        if (alive)
            for (uint32_t w = tid; w < n_words; w += 256u) mine |= s_bm[w] != 0u;
        if (!__syncthreads_or(mine)) { NS_BCNT(2, 1); continue; }   // (workgroup-uniform)
        for (uint32_t r = 0; r < it.ref_count; r++) {
            const BqRef b = rf[r];
            if (b.role == kBqNot) continue;
            uint64_t lo, hi;
            fc_cut(sg, b.list, w_lo, w_hi, lane, lo, hi);
            for (uint64_t i = lo + tid; i < hi; i += 256u) {
                const uint2 p = sg.postings[i];
                if (p.x < w_lo || p.x >= w_hi) continue;
                const uint32_t rel = p.x - w_lo;
                if (!((s_bm[rel >> 5] >> (rel & 31u)) & 1u)) continue;
                const float tf = (float)p.y;
                const float s = (b.idf * (tf * (1.2f + 1.0f))) / (tf + norm[p.x]);   // p.x < w_hi <= n_docs
                s_acc[rel] = s_acc[rel] + b.qweight * s;
            }
            __syncthreads();
        }
#ifdef NS_COUNT
        uint32_t multiplied = 0, clipped = 0;
        bool nonzero = false;   // BOOST: a factor of this thread's documents is not 0.0f
#endif
        for (uint32_t wb = v * 64u; wb < n_words; wb += 256u) {   // (wave-uniform)
            const uint32_t w = wb + lane;
            uint32_t bits = w < n_words ? s_bm[w] : 0u;
            cnt += (uint32_t)__popc(bits);
            while (__ballot(bits != 0u) != 0ull) {
                uint64_t key = 0;
                uint32_t g = 0;
                if (bits) {
                    const uint32_t rel = w * 32u + (uint32_t)__builtin_ctz(bits);   // < n: only such bits are set
                    bits &= bits - 1u;
                    if (COLLAPSE) g = grp[w_lo + rel];   // w_lo + rel < w_hi <= n_docs = the table's length (the call checked)
                    float score = s_acc[rel];
                    if (BOOST) {
                        const float f = boost[w_lo + rel];   // w_lo + rel < w_hi <= n_docs <= the table's length (the call checked)
                        score = __fmul_rn(score, f);
#ifdef NS_COUNT
                        multiplied++;
                        nonzero = nonzero || f != 0.0f;
#endif
                    }
                    key = ((uint64_t)bq_ord(__float_as_uint(score)) << 32) | (uint32_t)~(tile_rel + rel);
                }
#ifdef NS_COUNT
                if (BOOST && key != 0ull && key > last) clipped++;
#endif
                if (AFTER) key = af_clip(key, last, kept);
                if (COLLAPSE) cg_insert<0>(cset, key, g, K, lane);
                else bq_insert(set, key, K, lane);
            }
        }
#ifdef NS_COUNT
        if (BOOST) {   // (every thread of the workgroup is here: what leaves a window early leaves it above, uniformly)
            if (multiplied) atomicAdd(&g_ns_bbcnt[2], (unsigned long long)multiplied);
            if (clipped) atomicAdd(&g_ns_bbcnt[3], (unsigned long long)clipped);
            if (!__syncthreads_or(nonzero ? 1 : 0)) NS_BBCNT(4, 1);
            swept = true;
        }
#endif
    }
#ifdef NS_COUNT
    if (BOOST && swept) NS_BBCNT(1, 1);
#endif
    __syncthreads();   // (s_cnt is zero; nobody reads the accumulators any more)
    if (cnt) atomicAdd(&s_cnt, cnt);
    if (AFTER && kept) atomicAdd(&s_rest, kept);
    s_rows[v][lane] = COLLAPSE ? cset.hi : set.hi;
    s_rows[v][64u + lane] = COLLAPSE ? cset.lo : set.lo;
    __syncthreads();
    if (v != 0u) return;
    if (tid == 0 && s_cnt) atomicAdd(&found[it.query], (unsigned long long)s_cnt);
    if (AFTER && tid == 0 && s_rest) atomicAdd(&rest[it.query], (unsigned long long)s_rest);
    uint64_t* __restrict__ row = cand + (size_t)blockIdx.x * K;
    if (COLLAPSE) {
#pragma unroll 1
        for (uint32_t o = 1; o < 4u; o++)
#pragma unroll 1
            for (uint32_t half = 0; half < (K > 64u ? 2u : 1u); half++) {
                const uint64_t key = s_rows[o][half * 64u + lane];
                // the key's document is it.doc_lo + ~low < it.doc_hi <= n_docs: the sweep made it from such a document
                const uint32_t g = key ? grp[it.doc_lo + ~(uint32_t)key] : 0u;
                cg_insert<1>(cset, key, g, K, lane);
            }
        if (lane < K) row[lane] = cset.hi;
        if (64u + lane < K) row[64u + lane] = cset.lo;
        return;
    }
#pragma unroll 1
    for (uint32_t o = 1; o < 4u; o++) {
        bq_insert(set, s_rows[o][lane], K, lane);
        if (K > 64u) bq_insert(set, s_rows[o][64u + lane], K, lane);
    }
    if (lane < K) row[lane] = set.hi;
    if (64u + lane < K) row[64u + lane] = set.lo;
}

// At the upload of a factor table (ns_docboost_upload; as k_sd_check): is a factor not finite, or is its sign bit set (-0.0f too)?
__global__ void __launch_bounds__(256) k_bq_boost_check(const float* __restrict__ boost, uint32_t n_docs, uint32_t* __restrict__ bad) {
    bool any = false;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_docs; i += gridDim.x * 256u) {
        const uint32_t b = __float_as_uint(boost[i]);
        any = any || (b & 0x80000000u) != 0u || (b & 0x7F800000u) == 0x7F800000u;
    }
    if (any) atomicOr(bad, 1u);
}

// items / q_off index the whole call's items; cand holds the rows of the items from item_begin on.
__global__ void __launch_bounds__(256) k_bq_join(const FcItem* __restrict__ items, const uint32_t* __restrict__ q_off, uint32_t q_begin,
                                                 uint32_t q_end, uint32_t item_begin, const DevBqSeg* __restrict__ bqs,
                                                 const uint64_t* __restrict__ cand, uint32_t K, uint32_t* __restrict__ hits,
                                                 uint32_t* __restrict__ nhits) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = q_begin + blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= q_end) return;                                            // (wave-uniform; no barrier in this kernel)
    const uint32_t ib = q_off[q], ie = q_off[q + 1u];
    SdSet set{0ull, 0ull};
    for (uint32_t i = ib; i < ie; i++) {
        const uint64_t* __restrict__ row = cand + (size_t)(i - item_begin) * K;
        if (row[0] == 0ull) continue;                                  // an item that matched nothing (wave-uniform)
        NS_BCNT_WAVE(7, 1);
        const uint32_t base = (i - ib) * kSdRowSlots;
#pragma unroll 1
        for (uint32_t slot = lane; slot < kSdRowSlots && slot - lane < K; slot += 64u) {   // (wave-uniform: slot - lane is 0 or 64)
            const uint64_t c = slot < K ? row[slot] : 0ull;
            bq_insert(set, c ? ((c >> 32) << 32) | (uint32_t)~(base + slot) : 0ull, K, lane);
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
            hits[at * 3u + 0u] = bq_unord((uint32_t)(c >> 32));
            hits[at * 3u + 1u] = bqs[it.seg].seg_id;
            hits[at * 3u + 2u] = it.doc_lo + ~(uint32_t)c;
        } else {
            hits[at * 3u + 0u] = 0xFF800000u;                         // -inf
            hits[at * 3u + 1u] = 0xFFFFFFFFu;
            hits[at * 3u + 2u] = 0xFFFFFFFFu;
        }
    }
    if (lane == 0) nhits[q] = n;
}

// k_bq_join for ns_search_collapsed (§5ac), a kernel of its own so that k_bq_join keeps its name and its figures.  The rows of a
// query's items are joined through the collapsing set; a candidate's group is gathered from its item's segment table by its
// docId.  EXACT: a row holds its tile's best K groups by their tile-best document.  A group of the global first K has its
// global best in some tile; the groups that beat it there beat it globally too, so there are fewer than K of them and it is in
// that tile's row; of two rows' entries of one group the insertion keeps the better.  Writes the hits and the pad as k_bq_join
// does, groups[q * K + r] = the hit's group (0 in the pad) and, with others != NULL, others[q * K + r] = 0xFFFFFFFF for a hit
// with a group and 0 otherwise: k_cl_count adds the group's matched documents, the hit among them, and the sum is "others".
__global__ void __launch_bounds__(256) k_bq_join_collapsed(const FcItem* __restrict__ items, const uint32_t* __restrict__ q_off, uint32_t q_begin,
                                                           uint32_t q_end, uint32_t item_begin, const DevBqSeg* __restrict__ bqs,
                                                           const uint64_t* __restrict__ cand, uint32_t K, uint32_t* __restrict__ hits,
                                                           uint32_t* __restrict__ nhits, uint32_t* __restrict__ groups,
                                                           uint32_t* __restrict__ others) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = q_begin + blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= q_end) return;                                            // (wave-uniform; no barrier in this kernel)
    const uint32_t ib = q_off[q], ie = q_off[q + 1u];
    CgSet set{0ull, 0ull, 0u, 0u};
    for (uint32_t i = ib; i < ie; i++) {
        const uint64_t* __restrict__ row = cand + (size_t)(i - item_begin) * K;
        if (row[0] == 0ull) continue;                                  // an item that matched nothing (wave-uniform)
        const FcItem it = items[i];
        const uint32_t* __restrict__ grp = bq_group_table(bqs, it.seg);
        const uint32_t base = (i - ib) * kSdRowSlots;
#pragma unroll 1
        for (uint32_t slot = lane; slot < kSdRowSlots && slot - lane < K; slot += 64u) {   // (wave-uniform: slot - lane is 0 or 64)
            const uint64_t c = slot < K ? row[slot] : 0ull;
            const uint64_t key = c ? ((c >> 32) << 32) | (uint32_t)~(base + slot) : 0ull;
            const uint32_t g = c ? grp[it.doc_lo + ~(uint32_t)c] : 0u;   // a document of the tile: < doc_hi <= n_docs
#ifdef NS_COUNT
            cg_insert<2>(set, key, g, K, lane, [&](uint32_t low) { NS_CLCNT_WAVE(items[ib + ~low / kSdRowSlots].seg == it.seg ? 8 : 9, 1); });
#else
            cg_insert<2>(set, key, g, K, lane);
#endif
        }
    }
    uint32_t n = 0;
#pragma unroll 1
    for (uint32_t r = lane; r - lane < K; r += 64u) {                  // (r - lane is 0 or 64; K <= 128)
        const uint64_t jk = r < 64u ? set.hi : set.lo;
        const uint32_t g = r < 64u ? set.ghi : set.glo;
        const bool have = r < K && jk != 0ull;
        n += (uint32_t)__popcll(__ballot(have));
        if (r >= K) continue;
        const size_t at = (size_t)q * K + r;
        if (have) {
            const uint32_t low = ~(uint32_t)jk, rel = low / kSdRowSlots, slot = low % kSdRowSlots;
            const FcItem it = items[ib + rel];
            const uint64_t c = cand[(size_t)(ib + rel - item_begin) * K + slot];
            hits[at * 3u + 0u] = bq_unord((uint32_t)(c >> 32));
            hits[at * 3u + 1u] = bqs[it.seg].seg_id;
            hits[at * 3u + 2u] = it.doc_lo + ~(uint32_t)c;
        } else {
            hits[at * 3u + 0u] = 0xFF800000u;                         // -inf
            hits[at * 3u + 1u] = 0xFFFFFFFFu;
            hits[at * 3u + 2u] = 0xFFFFFFFFu;
        }
        groups[at] = have ? g : 0u;
        if (others) others[at] = cl_others_seed(g, have);
    }
    if (lane == 0) nhits[q] = n;
}

}  // namespace ns
