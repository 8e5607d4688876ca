// Batch planning: term refs -> (query, segment) term groups -> work items in launch order -> the descriptor image that
// ns_batch_prepare (ns_api.hip) uploads.  Host code only: no HIP runtime call and no device pointer.  The segments are seen
// through SegView (sizes and list registries), the settings and the shared-score registry are passed in.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/nextsearch_hip.h"
#include "ns_forkjoin.hpp"
#include "ns_internal.h"

namespace ns {

// Kernel variants (DESIGN.md "kernel variants").
//   wave variants: hb = table entries per wave (k_dscore) or docs per tile (k_tscore)
//   workgroup variants (k_score, the >64-terms fallback and the round-1 baseline): threads per
//   workgroup, slots per thread, postings per thread per round; tile_docs = nt * spt.
struct VariantDesc { uint32_t hb; uint32_t nt, spt, u; uint32_t d; };
static const VariantDesc kVariants[] = {
    {512, 512, 12, 4, 0},       // 0: default = AUTO: k_uscore, per (query, segment) group the driver-stream body (64 or 192 foreign postings per super-batch) or 1024-doc tiles, by its mix of lists
    {0, 1024, 12, 4, 0},        // 1: workgroup kernel, 12288-doc tiles
    {0, 512, 12, 4, 0},         // 2: workgroup kernel,  6144-doc tiles
    {0, 256, 16, 4, 0},         // 3: workgroup kernel,  4096-doc tiles
    {0, 512, 16, 8, 0},         // 4: workgroup kernel,  8192-doc tiles
    {0, 0, 0, 0, 0},            // 5..11: retired in round 2 (the wave-private batch kernel k_wscore); ns_set_tuning rejects them
    {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0},
    {512, 512, 12, 4, 0},       // 12: driver-stream kernel (k_dscore), 512 slots, 128 foreign postings per super-batch   [d == 0 marks k_dscore]
    {256, 512, 12, 4, 0},       // 13: k_dscore  256 slots /  64 foreign
    {1024, 512, 12, 4, 0},      // 14: k_dscore 1024 slots / 256 foreign
    {512, 512, 12, 4, 0},       // 15: k_dscore  512 slots /  64 foreign
    {512, 512, 12, 4, 0},       // 16: k_dscore  512 slots / 256 foreign
    {1024, 512, 12, 4, 0},      // 17: k_dscore 1024 slots / 128 foreign
    {512, 512, 12, 4, 1},       // 18: doc-tile kernel k_tscore for every group, 512-doc tiles   [d == 1 marks k_tscore]
    {1024, 512, 12, 4, 1},      // 19: k_tscore, 1024-doc tiles
    {2048, 512, 12, 4, 1},      // 20: k_tscore, 2048-doc tiles
};
static constexpr uint32_t kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);
static constexpr uint32_t kWaveMaxTerms = 64;
static constexpr uint32_t kDefaultSplitPostings = 32768;   // forced variants: postings per work item
// auto mode: work units per item (one unit = one streamed driver posting).  Every item pays for its own
// top-K warm-up and its K-row partial result, so large K wants fewer, longer items (sweeps: profiles/r01).
static constexpr uint32_t kSplitWorkSmallK = 98304, kSplitWorkLargeK = 131072;
static constexpr uint64_t kWorkForeign = 8, kWorkTile = 2, kWorkMerge = 4;   // merge: fitted on two-list laws (profiles/r03): 1.0 ps per unit, like the general class
// Class model (ns_ctx_class_model; DESIGN.md §4 "Choosing the body by modelled cost"): what the doc-tile body costs a group, in
// sixteenths of a work unit: 250 units per 1024-doc tile of the segment (header, top-K read-back, and the latency of a tile
// in the item's chain), 40 per (term, tile) visit and 0.6 per posting.  The visits of a list of c postings over t tiles are
// t * (1 - exp(-c / t)), from the table below (c / t in eighths, value in 1/256).  A class-0 group is promoted to doc tiles
// when kClassMarginPct per cent of that cost is at most its general (or merge) cost: no margin, because the whole-batch A/B
// that chose the constants (profiles/class_model/README.md) ran faster without one at every per-tile price tried.
static constexpr uint32_t kTileCostTile16 = 4000, kTileCostVisit16 = 640, kTileCostPosting16 = 10;
static constexpr uint32_t kClassMarginPct = 100;
static constexpr uint16_t kTileOcc256[65] = {
    0, 30, 57, 80, 101, 119, 135, 149, 162, 173, 183, 191, 199, 206, 212, 217, 221, 225, 229, 232, 235, 237, 240, 242, 243, 245,
    246, 247, 248, 249, 250, 251, 251, 252, 252, 253, 253, 253, 254, 254, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256};
static constexpr uint32_t kSkipMinCount = 64;   // shorter lists are never looked up in the skip registry (ns_segment_build_skips)
// per-item, per-term constants of the launch-order key (fitted to per-item timestamps, tools/dbg/item_times.py)
static constexpr uint64_t kItemTermGeneral = 4000, kItemTermThin = 3000, kItemTermTile = 8000;   // general re-fitted in round 2 (10000 -> 4000: ab16)
// Shared top rows (ns_ctx_share_rows; BatchPlan::cut "shared top rows"): a hot list gets rows when at least kRowMinUsers
// thin groups of the batch name it with the same idf and weight; its doc space is cut into the smallest power-of-two
// number of cells that leaves at most kRowCellPostings of its postings per cell on average.
static constexpr uint32_t kRowMinUsers = 4, kRowCellPostings = 65536;
static constexpr uint32_t kRowMaxTerms = 16;   // k_rscore has the 16-entry term tables only

inline std::string vformat(const char* fmt, va_list ap) {
    char buf[512];
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    return buf;
}

// ---- list tables ---------------------------------------------------------------------------------------------------
// Open-addressed table of posting lists keyed by the list's first posting (or by (segment << 32) | first posting): linear
// probing over a power-of-two number of slots (at least 16), doubled at half load.  Every lookup is by exact key.
template <class V>
class ListTable {
public:
    bool empty() const { return n_ == 0; }
    size_t slot_of(uint64_t key) const { return (size_t)((key * 0x9E3779B97F4A7C15ull) >> 20) & (slots_.size() - 1); }
    void prefetch(uint64_t key) const { if (!slots_.empty()) __builtin_prefetch(&slots_[slot_of(key)]); }
    const V* find(uint64_t key) const {
        if (slots_.empty()) return nullptr;
        for (size_t h = slot_of(key);; h = (h + 1) & (slots_.size() - 1)) {
            if (slots_[h].key == key) return &slots_[h].v;
            if (slots_[h].key == kFree) return nullptr;
        }
    }
    // the entry of `key`: found, or made with a value-initialised V (then *fresh is true)
    V& insert(uint64_t key, bool* fresh) {
        if (2 * n_ >= slots_.size()) rebuild(std::max<size_t>(16, slots_.size() * 2));
        for (size_t h = slot_of(key);; h = (h + 1) & (slots_.size() - 1)) {
            Slot& s = slots_[h];
            if (s.key == key) { *fresh = false; return s.v; }
            if (s.key == kFree) { s.key = key; n_++; *fresh = true; return s.v; }
        }
    }
    void put(uint64_t key, const V& v) { bool fresh; insert(key, &fresh) = v; }   // insert or replace
    template <class F> void for_each(F fn) { for (Slot& s : slots_) if (s.key != kFree) fn(s.key, s.v); }
    template <class F> void erase_if(F pred) { refill(slots_.size(), pred); }
    void clear() { slots_.clear(); n_ = 0; }

private:
    static constexpr uint64_t kFree = ~0ull;
    struct Slot { uint64_t key = kFree; V v{}; };
    void rebuild(size_t cap) { refill(cap, [](uint64_t, const V&) { return false; }); }
    template <class F> void refill(size_t cap, F drop) {
        std::vector<Slot> old(cap);
        old.swap(slots_);
        n_ = 0;
        for (const Slot& s : old) if (s.key != kFree && !drop(s.key, s.v)) put(s.key, s.v);
    }
    std::vector<Slot> slots_;
    size_t n_ = 0;
};

// The host side of a segment's optional per-list data, keyed by the list's first posting index.
struct SegLists {
    struct Imp { uint32_t count, idf_bits; };          // ns_segment_build_impacts: the impact stream holds this list with this idf
    struct Skip { uint32_t count, entry; };            // ns_segment_build_skips: index of the list's first entry in DevSeg::skips
    struct Bmx { uint32_t count, idf_bits, entry; };   // ns_segment_build_blockmax: index of its first block maximum
    ListTable<Imp> imp;
    ListTable<Skip> skip;
    ListTable<Bmx> bmx;
    // Shared term scores (ns_ctx_share_scores): every list a sharing batch ever built into d_impacts, first -> count.  Lists
    // that overlap another one are refused (two builders would write the same postings with different values).
    std::map<uint32_t, uint32_t> share_lists;
    bool share_admit(uint32_t first, uint32_t count) {
        auto it = share_lists.lower_bound(first);
        if (it != share_lists.end() && (it->first == first ? it->second != count : (uint64_t)first + count > it->first)) return false;
        if (it != share_lists.begin() && (it == share_lists.end() || it->first != first)) {
            auto pv = std::prev(it);
            if ((uint64_t)pv->first + pv->second > first) return false;
        }
        share_lists.emplace(first, count);
        return true;
    }
    bool imp_has(uint32_t first, uint32_t count, uint32_t idf_bits) const {
        const Imp* e = imp.find(first);
        return e && e->count == count && e->idf_bits == idf_bits;
    }
    // 1 + index of the first table entry of the list [first, first + count), or 0
    uint32_t skip_of(uint32_t first, uint32_t count) const {
        const Skip* e = skip.find(first);
        return e && e->count == count ? e->entry + 1u : 0u;
    }
    // 1 + index of the first block maximum of the list [first, first + count) built with this idf, or 0
    uint32_t bmx_of(uint32_t first, uint32_t count, uint32_t idf_bits) const {
        const Bmx* e = bmx.find(first);
        return e && e->count == count && e->idf_bits == idf_bits ? e->entry + 1u : 0u;
    }
};

// What planning knows of a segment.  `lists` is null when no segment has this id.
struct SegView {
    uint32_t n_docs = 0, n_tiles = 0;   // n_tiles: ceil(n_docs / tile_docs) of the workgroup-kernel variant
    uint64_t n_postings = 0;
    bool norm_safe = false;   // every norm lies in [2^-20, 2^30]: the BM25 division may take its short form (ns_div_short)
    bool packed = false;      // the packed posting stream exists
    SegLists* lists = nullptr;
};

// The shared-score registry of a ctx: (segment, first posting) -> the list's count and idf and the last batch that listed
// it; `live` counts the sharing batches alive: an idf may only change while it is 0.
struct ShareRegistry {
    struct Ent { uint32_t count, idf_bits, epoch; bool bad; };
    ListTable<Ent> tab;
    uint32_t epoch = 0;
    uint32_t live = 0;
};

// The tuning of a ctx that planning reads (ns_set_tuning, ns_ctx_use_*, ns_ctx_share_scores, ns_ctx_set_host_threads and
// the sweep knobs that ns_ctx_create reads from the environment).
struct PlanSettings {
    uint32_t variant = 0;
    uint32_t min_items = 0;
    uint32_t split_postings = 0;
    int n_cus = 0;
    bool use_impacts = true;   // batches take the impact stream when every list they touch has one (ns_ctx_use_impacts)
    int use_packed = 1;        // 0 off; 1, 2: batches read the packed stream when every segment they touch has one (ns_ctx_use_packed)
    bool use_skips = true;     // doc-tile groups walk the skip grid when their lists have skip tables (ns_ctx_use_skips)
    bool use_merge = true;     // general-class groups of exactly two term refs take the two-list merge body (ns_ctx_use_merge)
    uint32_t merge_ratio = 8;  // ... when the longer list is at most this many times the shorter (NS_MERGE_RATIO: sweeps)
    bool use_pruning = false;  // single-term groups whose list has block maxima skip the blocks that cannot enter the top-K (ns_ctx_use_pruning)
    // Shared term scores (ns_ctx_share_scores): 0 off; 1 a batch whose term refs name each distinct list often enough computes
    // every list's BM25 term scores ONCE (k_share_scores, in front of the scoring kernel, on every run) and scores from
    // {docId, score}; 2 every batch that can (tests).
    int share_mode = 1;
    uint32_t share_ratio = 48;           // share when postings >= share_ratio x distinct postings (below ~50 uses per posting the extra kernel costs what it saves) ...
    uint64_t share_min_postings = 4u << 20;   // ... and the batch scans at least this many postings
    unsigned prep_threads = 0; // 0 = automatic (up to 8); 1 = prepare on the calling thread only (ns_ctx_set_host_threads)
    // Launch order inside coarse run-time classes (see "XCD dealing" in BatchPlan::write): 1 = on.  The environment variables
    // NS_ORDER_MODE (0 = off) / NS_ORDER_COARSE (log2 of the fine buckets per class) override it for experiments; read at
    // ns_ctx_create.
    int order_mode = 1, order_coarse = 3;
    bool order_coarse_forced = false;   // NS_ORDER_COARSE given: no automatic choice
    uint32_t key_pct[4] = {100, 100, 100, 100};   // launch-order key of general / thin / tile / merge items in per cent (NS_KEY_PCT=g,t,d,m: sweeps)
    uint32_t tile_dens64 = 16;   // doc-tile class from this many postings per 64 docs (0.25 per doc); NS_TILE_DENS64 overrides (sweeps)
    // Shared top rows (ns_ctx_share_rows): 0 off; 1 thin groups whose hot list is named by at least row_min_users of them
    // take the list's top row per cell instead of streaming it; 2 every thin group that can (tests).  A ctx starts with 1
    // (ns_ctx_create; NS_SHARE_ROWS, NS_ROW_MIN_USERS and NS_ROW_CELL override the three for sweeps and tests).
    int row_mode = 0;
    uint32_t row_min_users = kRowMinUsers;
    uint32_t row_cell_postings = kRowCellPostings;
    // Class model (ns_ctx_class_model): 0 the density rule alone; 1 in a batch that fills the chip (no finer cut under the old
    // classes) a class-0 group whose modelled doc-tile cost undercuts its general cost becomes a tile group, and every tile
    // group is estimated by the model; 2 in every batch (tests, sweeps).  A ctx starts with 1 (ns_ctx_create; NS_CLASS_MODEL,
    // NS_CLASS_MARGIN and NS_TILE_COST=tile,visit,posting override mode, margin and constants for sweeps).
    int class_model = 0;
    uint32_t class_margin_pct = kClassMarginPct;
    uint32_t tile_cost16[3] = {kTileCostTile16, kTileCostVisit16, kTileCostPosting16};
    // sweeps only (ns_ctx_class_force; tools/class_fit.py): class-0 groups of three or more terms whose foreign share
    // rest / cost lies in tenth number force_share10 and whose postings per 64 docs lie in [force_dens_lo, force_dens_hi)
    // take the doc-tile body (force_body 1) or keep the general one whatever the model says (2); 0 = no forcing
    uint32_t force_body = 0, force_share10 = 0, force_dens_lo = 0, force_dens_hi = 0;
};

// A batch's device block is laid out in 256-byte aligned arrays: the offset of the next one of `bytes` bytes
inline size_t place_at(size_t& off, size_t bytes) {
    const size_t o = off;
    off = (off + std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
    return o;
}

// The class model's doc-tile cost of a group in work units (integers only: the same on every host thread)
inline uint64_t tile_model_cost(const uint32_t cost16[3], const DevTerm* dt, uint32_t n_terms, uint32_t n_docs) {
    const uint64_t tiles = ((uint64_t)n_docs + kSkipDocs - 1) / kSkipDocs;
    if (!tiles) return 0;
    uint64_t occ = 0, postings = 0;   // occ: the sum over the lists of the share of the tiles they visit, in 1/256
    for (uint32_t i = 0; i < n_terms; i++) {
        occ += kTileOcc256[std::min<uint64_t>((uint64_t)dt[i].count * 8 / tiles, 64)];
        postings += dt[i].count;
    }
    const uint64_t c16 = cost16[0] * tiles + cost16[1] * (tiles * occ / 256) + cost16[2] * postings;
    return (c16 + 15) / 16;
}

// ---- the planner ---------------------------------------------------------------------------------------------------
// A batch is planned in three fork-join phases over contiguous slices of the queries (the reference's requests are
// independent, src/api_engine.cpp:369): A regroup + classify, B cut into work items, C write the descriptors into the
// caller's buffer in launch order.  Between the phases only prefix sums over the slices run serially.  Every result
// (descriptor bytes, launch order) is independent of the number of threads.

struct HostGroup { DevGroup g; uint32_t query; uint64_t cost; uint64_t cmax; uint64_t work; bool wave; uint8_t cls; bool fast_div; bool signed_in; bool grid; bool merge2;
                   bool promoted;     // class model: a class-0 group by the density rule that the model made a tile group
                   uint32_t rkey1; };   // shared top rows: 0, or 1 + the group's entry in BatchPlan::rkeys (its items are consumers)

// Shared top rows: a hot list as its users score it — the list, its idf and its weight, bit for bit
struct RowKey {
    uint32_t seg, first, count, idf_bits, w_bits;
    bool operator==(const RowKey& o) const { return seg == o.seg && first == o.first && count == o.count && idf_bits == o.idf_bits && w_bits == o.w_bits; }
};
struct RowKeyHash {
    size_t operator()(const RowKey& k) const {
        uint64_t h = ((uint64_t)k.seg << 32 | k.first) * 0x9E3779B97F4A7C15ull;
        h ^= ((uint64_t)k.idf_bits << 32 | k.w_bits) * 0xC2B2AE3D27D4EB4Full;
        return (size_t)(h ^ (h >> 29));
    }
};
struct RowKeyEnt { RowKey key; uint32_t users, skip, cells, prod_begin, rank; bool on; };
struct RowCand { uint32_t group, dterm, skip, key; };   // a thin group that could take rows: its hot term and that list's skip table

constexpr uint32_t kOrderBuckets = 2048;   // launch-order key: 6 bits of exponent x 5 bits of mantissa of the estimated run time
inline uint32_t order_bucket(uint64_t c) {  // descending: bucket 0 holds the longest items
    if (c < 32) return kOrderBuckets - 1 - (uint32_t)c;
    const int b = 63 - __builtin_clzll(c);
    const uint32_t key = (uint32_t)b * 32u + (uint32_t)((c >> (b - 5)) & 31u);
    return kOrderBuckets - 1 - std::min(key, kOrderBuckets - 1);
}

struct PrepSlice {
    uint32_t q0 = 0, q1 = 0;
    std::vector<DevTerm> dterms;
    std::vector<HostGroup> groups;
    std::vector<uint32_t> qgroup_begin;   // q1 - q0 + 1 entries, local group indices
    std::vector<uint32_t> seg_ids;
    std::vector<RowCand> rcand;           // shared top rows: the slice's candidate groups, in group order
    uint64_t bounds_total = 0, postings_total = 0, total_work = 0;
    bool all_imp = true, all_pk = true, any_pruned = false;
    int err_code = NS_OK;
    uint32_t err_query = 0xFFFFFFFFu;
    std::string err_msg;
    // phase B
    std::vector<DevWItem> witems;
    std::vector<uint16_t> wbucket;        // launch-order bucket of each wave item; bit 15: > 16 terms (the "wide" instantiation)
    std::vector<uint32_t> wshare;         // locality key of the item: segment (6 bits) | doc range on the 4096-grid (12) | hash of its largest list (14) -> XCD dealing
    std::vector<DevRItem> ritems;         // shared top rows: consumer items (their own launch) ...
    std::vector<uint16_t> rbucket;        // ... and their launch-order buckets
    std::vector<DevItem> items;
    std::vector<uint64_t> item_cost;
    std::vector<DevGroup> bgroups;
    uint32_t n_rows = 0;
    bool direct = true;
    std::vector<uint32_t> hist;           // [3][kOrderBuckets]: narrow, wide, row consumers
    // offsets handed down by the serial steps
    uint32_t term_off = 0, row_off = 0, bgroup_off = 0;
    uint64_t bounds_off = 0;
    std::vector<uint32_t> start;          // [3][kOrderBuckets]: this slice's first position in each bucket of the sorted item array (row consumers: of theirs)
    void reset(uint32_t a, uint32_t b) {
        q0 = a; q1 = b;
        dterms.clear(); groups.clear(); qgroup_begin.clear(); seg_ids.clear(); rcand.clear();
        bounds_total = postings_total = total_work = 0; all_imp = true; all_pk = true; any_pruned = false;
        err_code = NS_OK; err_query = 0xFFFFFFFFu; err_msg.clear();
        witems.clear(); wbucket.clear(); wshare.clear(); ritems.clear(); rbucket.clear(); items.clear(); item_cost.clear(); bgroups.clear();
        n_rows = 0; direct = true;
        hist.assign(3 * kOrderBuckets, 0u);
        start.assign(3 * kOrderBuckets, 0u);
        term_off = row_off = bgroup_off = 0; bounds_off = 0;
    }
    void fail_at(uint32_t q, int code, const char* fmt, ...) {
        if (err_code != NS_OK) return;   // the first failing query of the slice is reported
        va_list ap;
        va_start(ap, fmt);
        err_msg = vformat(fmt, ap);
        va_end(ap);
        err_code = code; err_query = q;
    }
};

// Plans one batch after the other; keeps its host threads and per-thread scratch from batch to batch.  Use:
//   group()  phase A and the choice of shared term scores (the caller then makes the score buffers, or sets shared = false)
//   cut()    phase B and the launch order; sets the sizes and the layout of the descriptor image
//   write()  phase C and the XCD dealing: the image, except the DevSeg table at layout.segs, which is the caller's
struct BatchPlan {
    // ---- results (valid until the next group()) ----
    std::string err;                    // the message of a failing step
    uint32_t n_dterms = 0, n_rows = 0, n_witems = 0, n_items = 0, n_bgroups = 0;
    uint32_t n_class[3] = {0, 0, 0};    // auto mode: narrow wave items (<= 16 terms), then wide ones; contiguous in launch order
    uint64_t bounds_total = 0, postings_total = 0;
    bool direct = false;                // every query has exactly one work item: the scoring kernel writes final rows
    uint32_t class_stats[4] = {0, 0, 0, 0};   // auto mode: groups of class 0 (general and merge), 1 (thin), 2 (tile) after the rule; groups the class model promoted
    bool all_imp = false, all_pk = false, pruned = false;
    // shared term scores: the distinct lists the batch builds, in build order, and their postings
    bool shared = false;
    std::vector<DevShare> share_build;
    uint64_t share_postings = 0;
    std::vector<uint32_t> wide_q;       // queries cut into many partial rows: joined by k_merge_wide, one workgroup each
    // shared top rows: consumer items (k_rscore), producer items (single-term items over the cells of the hot lists, one row
    // of the row buffer each) and the producers' term entries, which follow the batch's own in the term array
    uint32_t n_ritems = 0, n_pitems = 0, n_pterms = 0;
    std::vector<RowKeyEnt> rkeys;
    std::vector<DevWItem> pitems;
    std::vector<DevTerm> pterms;
    struct Layout { size_t items, witems, terms, groups, queries, segs, wideq, share, ritems, pitems, rstats, bytes; } layout{};
    bool deal = false;                  // write() deals the coarse classes over the XCDs ...
    uint32_t deal_shift = 0;            // ... classes of 2^deal_shift fine buckets
    std::vector<uint32_t> bucket_pos;   // launch position at which each fine bucket of the narrow half starts (+ the end)

    // ---- inputs of the batch being planned ----
    const PlanSettings* cfg = nullptr;
    const std::vector<SegView>* segs = nullptr;
    const ns_query_desc* queries = nullptr;
    const ns_term_ref* terms = nullptr;
    uint32_t n_queries = 0, k = 0, flags = 0;
    bool auto_mode = false, want_imp = false, row_try = false;
    // ---- scratch ----
    unsigned width = 1;
    uint32_t G = 0;
    uint64_t total_work = 0;
    std::vector<PrepSlice> slices;
    std::vector<DevQuery> dq;
    std::vector<DevItem> sorted_items;
    std::vector<uint32_t> share_at;       // per launch position: the item's locality key (XCD dealing)
    std::vector<std::vector<DevWItem>> deal_tmp;   // per host thread
    std::vector<std::vector<uint64_t>> deal_key, deal_alt;
    std::vector<std::vector<uint32_t>> deal_bins;
    std::unique_ptr<ForkJoin> pool;

    int failed(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        err = vformat(fmt, ap);
        va_end(ap);
        return code;
    }
    void fork(const std::function<void(unsigned)>& fn) {
        if (width == 1) fn(0); else pool->run(width, fn);
    }

    int group(const PlanSettings& C, const std::vector<SegView>& SV, ShareRegistry& reg, const ns_query_desc* queries_,
              const ns_term_ref* terms_, uint32_t n_queries_, uint32_t k_, uint32_t flags_) {
        cfg = &C; segs = &SV; queries = queries_; terms = terms_; n_queries = n_queries_; k = k_; flags = flags_;
        const bool wave_path = kVariants[C.variant].hb != 0;
        auto_mode = C.variant == 0;

        // ---- slices: one per host thread for large batches (below ~1500 queries per thread the hand-over costs more than it saves) ----
        width = 1;
        if (n_queries >= 3000 && C.prep_threads != 1) {
            unsigned want = C.prep_threads ? C.prep_threads : std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 8u);
            // one thread per ~1500 queries or ~6000 term refs, whichever asks for more (a query over 8 segments carries 8x the refs)
            uint64_t n_refs = 0;
            for (uint32_t q = 0; q < n_queries; q++) n_refs += queries[q].term_count;
            width = std::max(1u, std::min<unsigned>(want, std::max<unsigned>(n_queries / 1500, (unsigned)std::min<uint64_t>(n_refs / 6000, 64))));
        }
        if (width > 1 && (!pool || pool->width() < width)) pool.reset(new ForkJoin(width));
        if (slices.size() < width) slices.resize(width);
        for (unsigned s = 0; s < width; s++) slices[s].reset((uint32_t)((uint64_t)n_queries * s / width), (uint32_t)((uint64_t)n_queries * (s + 1) / width));
        want_imp = C.use_impacts && auto_mode;
        // shared top rows: worth looking for candidates only in a batch that may share its term scores, in OR mode, at K <= 32
        // (the proof at the end of a consumer item needs kRowLen - K spare row entries)
        row_try = want_imp && C.row_mode != 0 && C.share_mode != 0 && C.use_skips && !(flags & NS_FLAG_AND) && k <= 32;

        // ---- phase A: regroup term refs by (query, segment), keeping query-term order inside each group; classify ----
        fork([&](unsigned si) {
            PrepSlice& S = slices[si];
            S.all_imp = want_imp;   // stays true while every list met so far has an impact stream built with this idf
            S.qgroup_begin.reserve(S.q1 - S.q0 + 1);
            for (uint32_t q = S.q0; q < S.q1; q++) {
                S.qgroup_begin.push_back((uint32_t)S.groups.size());
                const ns_query_desc qd = queries[q];
                if (qd.term_count && !terms) { S.fail_at(q, NS_E_INVAL, "terms is NULL"); break; }
                S.seg_ids.clear();
                bool bad = false;
                for (uint32_t i = 0; i < qd.term_count && !bad; i++) {
                    const ns_term_ref& r = terms[qd.term_begin + i];
                    if (r.seg_id >= SV.size() || !SV[r.seg_id].lists) { S.fail_at(q, NS_E_INVAL, "query %u term %u: unknown segment %u", q, i, r.seg_id); bad = true; break; }
                    const SegView& s = SV[r.seg_id];
                    if (r.byte_off % 8 != 0) { S.fail_at(q, NS_E_INVAL, "query %u term %u: byte_off %llu not a multiple of 8", q, i, (unsigned long long)r.byte_off); bad = true; break; }
                    if (r.byte_off / 8 + r.count > s.n_postings) { S.fail_at(q, NS_E_INVAL, "query %u term %u: list [%llu,+%u) outside segment %u (%llu postings)", q, i, (unsigned long long)(r.byte_off / 8), r.count, r.seg_id, (unsigned long long)s.n_postings); bad = true; break; }
                    if (std::find(S.seg_ids.begin(), S.seg_ids.end(), r.seg_id) == S.seg_ids.end()) S.seg_ids.push_back(r.seg_id);
                }
                if (bad) break;
                std::sort(S.seg_ids.begin(), S.seg_ids.end());   // segments in manifest (id) order, api_engine.cpp:441
                for (uint32_t sid : S.seg_ids) {
                    const SegView& sv = SV[sid];
                    HostGroup hg{};
                    hg.fast_div = sv.norm_safe;
                    if (!sv.packed) S.all_pk = false;
                    hg.g.term_begin = (uint32_t)S.dterms.size();   // local to the slice until phase B
                    hg.g.seg = sid;
                    hg.query = q;
                    for (uint32_t i = 0; i < qd.term_count; i++) {
                        const ns_term_ref& r = terms[qd.term_begin + i];
                        if (r.seg_id != sid) continue;
                        DevTerm t{};
                        t.list_off = r.byte_off / 8;
                        t.count = r.count;
                        t.idf = r.idf;
                        t.weight = r.qweight;
                        t.seg = sid;
                        S.dterms.push_back(t);
                        hg.cost += r.count;
                        hg.cmax = std::max<uint64_t>(hg.cmax, r.count);
                        if (S.all_imp) {
                            uint32_t ib; std::memcpy(&ib, &r.idf, 4);
                            S.all_imp = sv.lists->imp_has((uint32_t)(r.byte_off / 8), r.count, ib);
                        }
                        // 2^-30 <= idf <= 2^30 (and finite): see ns_div_short
                        if (!(r.idf >= 9.313225746154785e-10f && r.idf <= 1073741824.0f)) hg.fast_div = false;
                        if (std::signbit(r.idf) || std::signbit(r.qweight)) hg.signed_in = true;   // a contribution may be -0.0f (see dscore_body)
                    }
                    hg.g.term_count = (uint32_t)S.dterms.size() - hg.g.term_begin;
                    if ((flags & NS_FLAG_AND) && hg.g.term_count > 255) { S.fail_at(q, NS_E_INVAL, "AND mode supports at most 255 term refs per (query, segment)"); bad = true; break; }
                    hg.wave = wave_path && hg.g.term_count <= kWaveMaxTerms;
                    // class of the group (auto mode only): which scoring body suits its mix of lists (sweeps on
                    // MI355X, profiles/r01): 1 = one list dominates (the others hold <= 1/32 of its postings): driver
                    // stream with the 64-posting foreign budget; 2 = dense (>= 0.25 postings per doc over >= 2
                    // lists): doc tiles; 0 = driver stream with the 192-posting budget.
                    {
                        const uint64_t rest = hg.cost - hg.cmax;
                        const uint32_t nd = std::max<uint32_t>(sv.n_docs, 1);
                        if (rest * 32 <= hg.cmax) hg.cls = 1;
                        else if (hg.g.term_count >= 2 && hg.cost * 64 >= (uint64_t)nd * C.tile_dens64) hg.cls = 2;
                        else hg.cls = 0;
                        // work estimate in units of one streamed driver posting (measured, profiles/r01): a foreign
                        // posting (claim, accumulate, read back) costs ~8x, a doc-tile posting ~2x
                        hg.work = !auto_mode ? hg.cost : (hg.cls == 2 ? hg.cost * kWorkTile : hg.cmax + rest * kWorkForeign);
                        // two lists, general class: the merge body (no table): both lists cost about alike per posting
                        // (two COMPARABLE lists: when one is more than 8x the other, a window of the short one per round of the long
                        // one is mostly padding and the table path is as good: r8 + r300, 37 : 1, measured 3 % slower with the merge)
                        hg.merge2 = auto_mode && C.use_merge && hg.cls == 0 && hg.g.term_count == 2 && rest * C.merge_ratio >= hg.cmax;
                        if (hg.merge2) hg.work = hg.cmax + rest * kWorkMerge;
                    }
                    // shared top rows: a thin group whose hot list (its first largest one) has a skip table is a candidate
                    if (row_try && hg.wave && hg.cls == 1 && !hg.signed_in && hg.g.term_count <= kRowMaxTerms && hg.cmax >= kSkipMinCount &&
                        sv.n_docs > 0 && !sv.lists->skip.empty() && !(C.use_pruning && hg.g.term_count == 1)) {
                        const DevTerm* dt = S.dterms.data() + hg.g.term_begin;
                        uint32_t d = 0;
                        while (dt[d].count != hg.cmax) d++;
                        const uint32_t sk = sv.lists->skip_of((uint32_t)dt[d].list_off, dt[d].count);
                        if (sk) S.rcand.push_back(RowCand{(uint32_t)S.groups.size(), d, sk, 0u});
                    }
                    if (!hg.wave) {
                        hg.g.bounds_off = S.bounds_total;   // local; the slice's base is added in phase B
                        S.bounds_total += (uint64_t)(sv.n_tiles + 1) * hg.g.term_count;
                    }
                    S.postings_total += hg.cost;
                    S.total_work += hg.work;
                    S.groups.push_back(hg);
                }
                if (bad) break;
            }
            S.qgroup_begin.resize(S.q1 - S.q0 + 1, (uint32_t)S.groups.size());
        });
        {
            const PrepSlice* first = nullptr;
            for (unsigned s = 0; s < width; s++)
                if (slices[s].err_code != NS_OK && (!first || slices[s].err_query < first->err_query)) first = &slices[s];
            if (first) return failed(first->err_code, "%s", first->err_msg.c_str());
        }
        bounds_total = postings_total = total_work = 0;
        n_dterms = G = 0;
        all_imp = want_imp; all_pk = C.use_packed != 0 && auto_mode;
        for (unsigned s = 0; s < width; s++) {
            PrepSlice& S = slices[s];
            S.term_off = n_dterms; S.bounds_off = bounds_total;
            n_dterms += (uint32_t)S.dterms.size(); G += (uint32_t)S.groups.size();
            bounds_total += S.bounds_total; postings_total += S.postings_total; total_work += S.total_work;
            all_imp = all_imp && S.all_imp;
            all_pk = all_pk && S.all_pk;
        }
        // ---- class model (ns_ctx_class_model), between phases A and B as the row pass is: whether the batch fills the chip is
        // known only now.  It does when cut() would not cut it finer than the default share under the classes of the density
        // rule (cut()'s fine_cut, restated); a batch that leaves wave slots idle is bound by its longest chain, where the fitted
        // costs do not hold.  Then every tile group is estimated by the model — the estimate cuts it into ranges and orders its
        // items — and a class-0 group whose modelled tile cost undercuts its general or merge cost by the margin joins them.
        if (auto_mode && (C.class_model != 0 || C.force_body != 0)) {
            const uint64_t share0 = k <= 32 ? kSplitWorkSmallK : kSplitWorkLargeK;
            const bool fills = !C.split_postings && total_work / ((uint64_t)std::max(C.n_cus, 1) * 96u) >= share0;
            const bool model_on = C.class_model == 2 || (C.class_model == 1 && fills);
            if (model_on || C.force_body != 0) {
                fork([&](unsigned si) {
                    PrepSlice& S = slices[si];
                    for (HostGroup& hg : S.groups) {
                        const uint32_t nd = SV[hg.g.seg].n_docs;
                        if (!hg.wave || hg.g.term_count < 2 || hg.cls == 1 || nd == 0) continue;
                        const uint64_t tc = tile_model_cost(C.tile_cost16, S.dterms.data() + hg.g.term_begin, hg.g.term_count, nd);
                        const uint64_t old = hg.work;
                        if (hg.cls == 2) {
                            if (model_on) hg.work = tc;
                        } else {
                            bool promote = model_on && tc * C.class_margin_pct <= hg.work * 100;
                            if (C.force_body != 0 && hg.g.term_count >= 3 && (hg.cost - hg.cmax) * 10 / hg.cost == C.force_share10) {
                                const uint64_t d64 = hg.cost * 64 / nd;
                                if (d64 >= C.force_dens_lo && d64 < C.force_dens_hi) promote = C.force_body == 1;
                            }
                            if (promote) { hg.cls = 2; hg.merge2 = false; hg.promoted = true; hg.work = tc; }
                        }
                        S.total_work += hg.work - old;   // (modulo 2^64: the sum stays exact)
                    }
                });
                total_work = 0;
                for (unsigned s = 0; s < width; s++) total_work += slices[s].total_work;
            }
        }
        class_stats[0] = class_stats[1] = class_stats[2] = class_stats[3] = 0;
        if (auto_mode)
            for (unsigned s = 0; s < width; s++)
                for (const HostGroup& hg : slices[s].groups) { class_stats[hg.cls]++; class_stats[3] += hg.promoted ? 1u : 0u; }
        if (bounds_total >= (1ull << 32)) return failed(NS_E_INVAL, "batch too large: %llu boundary entries; split the batch", (unsigned long long)bounds_total);

        // ---- shared term scores (ns_ctx_share_scores; k_share_scores): the batch's distinct lists, each listed once, in the
        // order the term refs name them.  A list is refused — and the batch then scores every posting in place, as it
        // always did — when it overlaps another list ever shared in its segment (two builders, one posting), when the segment
        // carries an optional impact stream that does not hold exactly this list with this idf (the stream is not the batch's
        // to overwrite), or when its idf differs from the one a LIVE sharing batch built it with (that batch may run again).
        share_build.clear();
        share_postings = 0;
        shared = false;
        if (!all_imp && want_imp && C.share_mode != 0 && !all_pk && postings_total > 0 &&
            (C.share_mode == 2 || postings_total >= C.share_min_postings)) {
            shared = true;
            if (++reg.epoch == 0) {   // the batch counter wrapped: no entry may look like this batch's
                reg.tab.for_each([](uint64_t, ShareRegistry::Ent& en) { en.epoch = 0; });
                reg.epoch = 1;
            }
            const uint32_t epoch = reg.epoch;
            for (unsigned sl = 0; sl < width && shared; sl++) {
                const std::vector<DevTerm>& dts = slices[sl].dterms;
                for (size_t ti = 0; ti < dts.size(); ti++) {
                    // the registry is a few MB and every probe of it a cache miss: the probe of the term 8 ahead is requested now
                    if (ti + 8 < dts.size()) reg.tab.prefetch(((uint64_t)dts[ti + 8].seg << 32) | (uint32_t)dts[ti + 8].list_off);
                    const DevTerm& t = dts[ti];
                    if (!t.count) continue;
                    SegLists* sg = SV[t.seg].lists;
                    uint32_t ib; std::memcpy(&ib, &t.idf, 4);
                    const uint32_t first = (uint32_t)t.list_off;
                    if (!sg->imp.empty()) {
                        if (sg->imp_has(first, t.count, ib)) continue;   // the optional stream holds this list already
                        shared = false; break;
                    }
                    bool fresh = false;
                    ShareRegistry::Ent& en = reg.tab.insert(((uint64_t)t.seg << 32) | first, &fresh);
                    if (fresh) { en.count = t.count; en.idf_bits = ib; en.epoch = 0; en.bad = !sg->share_admit(first, t.count); }
                    if (en.bad || en.count != t.count) { shared = false; break; }
                    if (en.idf_bits != ib) {
                        if (reg.live || en.epoch == epoch) { shared = false; break; }
                        en.idf_bits = ib;
                    }
                    if (en.epoch != epoch) {
                        en.epoch = epoch;
                        if (share_postings + t.count >= (1ull << 32)) { shared = false; break; }
                        share_build.push_back(DevShare{first, t.count, t.idf, t.seg, (uint32_t)share_postings});
                        share_postings += t.count;
                        // (a batch that cannot reach the ratio gives up here: the frequent lists come early, and with them the verdict)
                        if (C.share_mode == 1 && share_postings * C.share_ratio > postings_total) { shared = false; break; }
                    }
                }
            }
            if (shared && C.share_mode == 1 && postings_total < (uint64_t)C.share_ratio * share_postings) shared = false;
        }
        return NS_OK;
    }

    // cell i of `cells` (a power of two, at most n_docs / kSkipDocs) of a segment's doc space: the nested grid of the range
    // cut, on the skip grid
    static void row_cell(uint32_t n_docs, uint32_t cells, uint32_t i, uint32_t& lo, uint32_t& hi) {
        lo = (uint32_t)((uint64_t)n_docs * i / cells);
        hi = (uint32_t)((uint64_t)n_docs * (i + 1) / cells);
        lo -= lo % kSkipDocs;
        if (i + 1 < cells) hi -= hi % kSkipDocs;
    }

    int cut() {
        const PlanSettings& C = *cfg;
        const std::vector<SegView>& SV = *segs;
        if (shared) all_imp = true;
        else { share_build.clear(); share_postings = 0; }

        // ---- work items.  A group is split into doc ranges (a) so that no single worker carries more
        // than ~split_postings units of estimated work (the longest item bounds the batch's tail; launch
        // order is longest-estimated-work first), and (b) so that a small batch still fills the chip.  Partial rows of one query are contiguous; k_merge joins them.
        const uint32_t min_items = C.min_items ? C.min_items : (uint32_t)std::max(C.n_cus, 1) * 24u;
        int small_mode = 0;   // thin / tile items: 0 = double share, 1 = plain share, 2 = half share (see below)
        uint64_t split_postings = C.split_postings ? C.split_postings
                                  : (!auto_mode ? kDefaultSplitPostings : (k <= 32 ? kSplitWorkSmallK : kSplitWorkLargeK));
        bool fine_cut = false;   // the batch is cut finer than the default share: it does not fill the chip for long
        if (!C.split_postings && auto_mode) {
            // a small batch: cut finer so that the chip still sees ~100 items per CU (an item of the default size
            // runs 0.3-1.3 ms: with fewer items than wave slots that would be the whole batch's time), but not
            // below ~16 K units, where an item's fixed cost takes over
            const uint64_t fine = total_work / ((uint64_t)std::max(C.n_cus, 1) * 96u);
            fine_cut = fine < split_postings;
            split_postings = std::min<uint64_t>(split_postings, std::max<uint64_t>(fine, 16384));
            // A batch that leaves wave slots idle is bound by its LONGEST item, and a streaming item is a chain of dependent
            // round trips (one 256-posting round in flight per wave).  When the double share of a thin or tile item would
            // exceed what a wave slot gets on average, those items lose it; when even a plain share does, they are halved
            // (profiles/r02/small_batch_split_modes.txt: 256 / 512 / 1024 queries of the cfg5 law run 36 / 27 / 14 % faster;
            // batches that fill the chip — all thin groups of cfg5 alone, 4096 single-term queries — are left as they were).
            const uint64_t per_slot = total_work / ((uint64_t)std::max(C.n_cus, 1) * 24u);
            small_mode = per_slot >= 2 * split_postings ? 0 : (per_slot >= split_postings ? 1 : 2);
        }
        uint32_t chunks_per_group = 1;
        if (G > 0 && G < min_items) chunks_per_group = std::min<uint32_t>((min_items + G - 1) / G, 1024u);   // one query alone: 1024 ranges are plenty
        dq.assign(n_queries, DevQuery{});

        // ---- shared top rows (ns_ctx_share_rows; k_rscore, ns_row_kernel.hip).  A thin group is one hot list H plus tail lists.
        // A doc that no tail holds scores 0.0f + w * s_H(d): what a single-term query on H gives it, bit for bit, whichever
        // query asks.  So the batch ranks H once per cell of its doc space (a PRODUCER item: a plain single-term item with
        // K' = kRowLen whose result row lies in the batch's row buffer), and the thin groups that name H with this idf and this
        // weight are cut into exactly those cells; their items (CONSUMERS) leave the scoring launch for one of their own, in
        // which H is looked up by docId for the tails' docs and otherwise taken from the row.  Serial: the users of a key are
        // counted over the whole batch, keys are numbered in the order the queries name them.
        rkeys.clear(); pitems.clear(); pterms.clear();
        n_ritems = n_pitems = n_pterms = 0;
        if (shared && row_try) {
            std::unordered_map<RowKey, uint32_t, RowKeyHash> index;
            for (unsigned s = 0; s < width; s++) {
                PrepSlice& S = slices[s];
                for (RowCand& c : S.rcand) {
                    const DevTerm& t = S.dterms[S.groups[c.group].g.term_begin + c.dterm];
                    RowKey key{t.seg, (uint32_t)t.list_off, t.count, 0u, 0u};
                    std::memcpy(&key.idf_bits, &t.idf, 4); std::memcpy(&key.w_bits, &t.weight, 4);
                    auto ins = index.emplace(key, (uint32_t)rkeys.size());
                    if (ins.second) rkeys.push_back(RowKeyEnt{key, 0u, c.skip, 0u, 0u, 0u, false});
                    c.key = ins.first->second;
                    rkeys[c.key].users++;
                }
            }
            for (RowKeyEnt& e : rkeys) {
                if (C.row_mode != 2 && e.users < C.row_min_users) continue;
                const SegView& sg = SV[e.key.seg];
                // every cell holds at least one cell of the skip grid (the ranges start and end on it)
                uint32_t cells = 1;
                while ((uint64_t)cells * std::max<uint32_t>(C.row_cell_postings, 1u) < e.key.count && cells * 2 <= sg.n_docs / kSkipDocs && cells < 4096) cells <<= 1;
                e.on = true; e.cells = cells; e.prod_begin = n_pitems; e.rank = n_pterms++;
                DevTerm t{};
                t.list_off = e.key.first; t.count = e.key.count; t.seg = e.key.seg; t.skip = e.skip;
                std::memcpy(&t.idf, &e.key.idf_bits, 4); std::memcpy(&t.weight, &e.key.w_bits, 4);
                pterms.push_back(t);
                for (uint32_t i = 0; i < cells; i++) {
                    DevWItem it{};
                    it.seg = e.key.seg;
                    it.term_begin = n_dterms + e.rank;
                    it.term_count = 1;
                    row_cell(sg.n_docs, cells, i, it.doc_lo, it.doc_hi);
                    it.out_slot = n_pitems++;
                    it.whole = (cells == 1 ? 1u : 0u) | 4u | 64u;   // thin body (no foreign list at all), range ends from the skip table
                    pitems.push_back(it);
                }
            }
            for (unsigned s = 0; s < width; s++) {
                PrepSlice& S = slices[s];
                for (const RowCand& c : S.rcand)
                    if (rkeys[c.key].on) S.groups[c.group].rkey1 = c.key + 1u;
            }
        }

        // ---- phase B: cut the groups into work items (rows numbered inside the slice) ----
        fork([&](unsigned si) {
            PrepSlice& S = slices[si];
            for (uint32_t q = S.q0; q < S.q1; q++) {
                dq[q].part_begin = S.n_rows;
                for (uint32_t gi = S.qgroup_begin[q - S.q0]; gi < S.qgroup_begin[q - S.q0 + 1]; gi++) {
                    HostGroup& hg = S.groups[gi];
                    hg.g.term_begin += S.term_off;          // global from here on
                    const SegView& sg = SV[hg.g.seg];
                    if (sg.n_docs == 0) continue;   // empty segment: nothing to score
                    if (hg.wave) {
                        DevTerm* dt = S.dterms.data() + (hg.g.term_begin - S.term_off);
                        // thin and tile groups run at a steady rate per posting: fewer, longer items (less per-item set-up,
                        // same balance); groups with dense foreign lists vary more per posting and stay finer
                        uint64_t sp_ = (auto_mode && hg.cls != 0) ? split_postings * 2 : split_postings;
                        if (auto_mode && hg.cls != 0 && small_mode) sp_ = small_mode == 2 ? split_postings / 2 : split_postings;
                        const uint64_t want = std::max<uint64_t>((hg.work + sp_ - 1) / sp_, chunks_per_group);
                        uint32_t ns = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(want, 1), std::min<uint32_t>(sg.n_docs, 4096));
                        // The number of ranges is a POWER OF TWO (the nearest in ratio; the next one up for a small batch): range boundaries then come from one
                        // nested grid, so the items of different queries cover IDENTICAL doc ranges of the lists they share, and
                        // items of one range — equal size, adjacent in the launch order — read the same bytes at about the same
                        // time: L2 / Infinity-Cache hits instead of misses (same number of items on average; cfg3 -5 %, cfg5's
                        // tile groups -7 %, a 2048-query batch -4 %; profiles/r02/ab/ab14_range_grid.txt).
                        if (auto_mode && ns > 1) {
                            uint32_t p2 = 1;
                            while (p2 < ns) p2 <<= 1;
                            if (!small_mode && (uint64_t)ns * ns * 2 < (uint64_t)p2 * p2) p2 >>= 1;   // a batch that leaves wave slots idle never gets fewer items
                            // K > 32: a group that is cut at all is cut into at least 8 ranges (cfg3 -7 %, at K = 64 -7 %, another seed
                            // -7 %; 16 is too many; at K <= 32 the same rule costs 2 %: ab14 / ab19)
                            if (k > 32 && p2 < 8) p2 = 8;
                            ns = std::min<uint32_t>(p2, std::min<uint32_t>(sg.n_docs, 4096));
                        }
                        // shared top rows: a consumer group is cut into exactly the cells of its hot list's rows
                        const RowKeyEnt* rk = hg.rkey1 ? &rkeys[hg.rkey1 - 1u] : nullptr;
                        if (rk) ns = rk->cells;
                        // Skip tables (ns_segment_build_skips): a doc-tile group walks the grid of its lists' tables; a group of the
                        // driver-stream bodies that is cut into ranges takes the ranges' ends of its frequent lists from their
                        // tables instead of searching for them (the searches of a hot list are a dozen dependent loads: 4-20 % of
                        // an item's time, most in small batches).  Either way the ranges start and end on the grid.
                        if (auto_mode && C.use_skips && (hg.cls == 2 || ns > 1 || rk) && !sg.lists->skip.empty()) {
                            for (uint32_t ti = 0; ti < hg.g.term_count; ti++) {
                                if (dt[ti].count < kSkipMinCount) continue;
                                dt[ti].skip = sg.lists->skip_of((uint32_t)dt[ti].list_off, dt[ti].count);
                                if (dt[ti].skip) hg.grid = true;
                            }
                        }
                        // Block-max pruning (ns_ctx_use_pruning): a group of ONE list whose block maxima were built with this idf, scored
                        // with a positive weight — the fp32 product w * s is then monotone in s and never a negative zero
                        bool pruned_ = false;
                        if (auto_mode && C.use_pruning && hg.g.term_count == 1 && !sg.lists->bmx.empty()) {
                            uint32_t ib; std::memcpy(&ib, &dt[0].idf, 4);
                            if (dt[0].idf > 0.0f && std::isfinite(dt[0].idf) && dt[0].weight > 0.0f && std::isfinite(dt[0].weight)) {
                                dt[0].bmx = sg.lists->bmx_of((uint32_t)dt[0].list_off, dt[0].count, ib);
                                pruned_ = dt[0].bmx != 0;
                            }
                            if (pruned_) S.any_pruned = true;
                        }
                        // launch-order key = estimated run time of the ITEM: its share of the group's work plus what
                        // every item pays per term regardless of size (window planning, range searches, table set-up)
                        const uint64_t per_term = hg.cls == 2 ? kItemTermTile : (hg.cls == 1 ? kItemTermThin : kItemTermGeneral);
                        uint64_t key = hg.work / ns + 1 + (auto_mode ? per_term * hg.g.term_count : 0);
                        // In a batch cut finer than the default share the streaming items (thin, tile) are chains of round trips that
                        // a less loaded chip does not shorten, while the issue-bound general items do run faster: those start
                        // later (2048 queries of the cfg5 law -11 %, 4096 -5 %, 512 -4 %; ab16_order_key_small_batches.txt).
                        if (fine_cut && hg.cls == 0) key = key * 5 / 8;
                        // K > 32: the streaming items pay more per posting than the work units (fitted at K = 10) say — fewer waves
                        // per CU, larger candidate buffers — so the general items start later there too (cfg3 -2.6 %, at K = 64 -2.3 %)
                        else if (auto_mode && k > 32 && hg.cls == 0) key = key * 3 / 4;
                        if (auto_mode) key = key * C.key_pct[hg.merge2 ? 3 : hg.cls] / 100;   // sweeps (NS_KEY_PCT); 100 each by default
                        // a consumer pays for its foreign postings and per term; its hot list costs it a look-up per foreign doc
                        if (rk) key = (hg.cost - hg.cmax) * kWorkForeign / ns + 1 + kItemTermThin * hg.g.term_count;
                        const bool wide = auto_mode && hg.g.term_count > 16;
                        const uint32_t bucket = order_bucket(key);
                        // what the group's items read most of: its largest list (the driver of a driver-stream item)
                        uint64_t big_off = 0;
                        for (uint32_t ti = 0, cm = 0; ti < hg.g.term_count; ti++)
                            if (dt[ti].count >= cm) { cm = dt[ti].count; big_off = dt[ti].list_off; }
                        for (uint32_t i = 0; i < ns; i++) {
                            DevWItem it{};
                            it.query = q;
                            it.seg = hg.g.seg;
                            it.term_begin = hg.g.term_begin;
                            it.term_count = hg.g.term_count;
                            it.doc_lo = (uint32_t)((uint64_t)sg.n_docs * i / ns);
                            it.doc_hi = (uint32_t)((uint64_t)sg.n_docs * (i + 1) / ns);
                            if (hg.grid) {   // ranges of a skip-grid group start and end on the grid
                                it.doc_lo -= it.doc_lo % kSkipDocs;
                                if (i + 1 < ns) it.doc_hi -= it.doc_hi % kSkipDocs;
                            }
                            if (rk) row_cell(sg.n_docs, ns, i, it.doc_lo, it.doc_hi);   // (the same range; spelled by the rule the producers use)
                            if (it.doc_hi <= it.doc_lo) continue;
                            it.out_slot = S.n_rows++;
                            it.whole = (ns == 1 ? 1u : 0u) | (hg.fast_div ? 8u : 0u) | (hg.signed_in ? 16u : 0u) | (hg.grid ? (hg.cls == 2 ? 32u : 64u) : 0u);
                            // auto mode: very dense groups take the doc-tile body (bit 1), groups with thin non-driver lists the small foreign budget (bit 2)
                            if (auto_mode) it.whole |= (hg.cls == 2 ? 2u : 0u) | (hg.cls == 1 ? 4u : 0u) | (pruned_ ? 128u : 0u) | (hg.merge2 && hg.wave ? 256u : 0u);
                            if (rk) {   // a consumer: k_rscore's, with the row of its cell and the place of the hot list in its term order
                                uint32_t d = 0;
                                while (dt[d].count != hg.cmax) d++;
                                S.ritems.push_back(DevRItem{it, rk->prod_begin + i, d});
                                S.rbucket.push_back((uint16_t)bucket);
                                S.hist[2 * kOrderBuckets + bucket]++;
                                continue;
                            }
                            S.witems.push_back(it);
                            S.wbucket.push_back((uint16_t)(bucket | (wide ? 0x8000u : 0u)));
                            {
                                uint64_t h = big_off * 0x9E3779B97F4A7C15ull;
                                h ^= h >> 29;
                                const uint32_t r12 = (uint32_t)(((uint64_t)it.doc_lo << 12) / std::max<uint32_t>(sg.n_docs, 1u)) & 4095u;
                                S.wshare.push_back(((it.seg & 63u) << 26) | (r12 << 14) | (uint32_t)((h >> 40) & 0x3FFFu));
                            }
                            S.hist[(wide ? kOrderBuckets : 0) + bucket]++;
                        }
                    } else {
                        DevGroup g = hg.g;
                        g.bounds_off += S.bounds_off;
                        S.bgroups.push_back(g);
                        const uint32_t nt = sg.n_tiles;
                        const uint32_t chunks = std::min(chunks_per_group, nt);
                        const uint32_t per = (nt + chunks - 1) / chunks;
                        for (uint32_t tb = 0; tb < nt; tb += per) {
                            DevItem it{};
                            it.bounds_off = g.bounds_off;
                            it.query = q;
                            it.seg = g.seg;
                            it.term_begin = g.term_begin;
                            it.term_count = g.term_count;
                            it.tile_begin = tb;
                            it.tile_end = std::min(nt, tb + per);
                            it.out_slot = S.n_rows++;
                            S.item_cost.push_back(hg.cost * (it.tile_end - it.tile_begin) / nt + 1);
                            S.items.push_back(it);
                        }
                    }
                }
                dq[q].part_count = S.n_rows - dq[q].part_begin;
                if (dq[q].part_count != 1) S.direct = false;
            }
        });
        n_rows = n_witems = n_items = n_bgroups = 0;
        direct = n_queries > 0;
        pruned = false;
        for (unsigned s = 0; s < width; s++) {
            PrepSlice& S = slices[s];
            S.row_off = n_rows; S.bgroup_off = n_bgroups;
            n_rows += S.n_rows; n_witems += (uint32_t)S.witems.size(); n_ritems += (uint32_t)S.ritems.size(); n_items += (uint32_t)S.items.size(); n_bgroups += (uint32_t)S.bgroups.size();
            direct = direct && S.direct;
            pruned = pruned || S.any_pruned;
        }
        // launch order of the wave items: narrow (<= 16 terms) before wide, longest estimated run time first, ties in query order
        n_class[0] = n_class[1] = n_class[2] = 0;
        {
            uint32_t pos = 0;
            bucket_pos.assign(kOrderBuckets + 1, 0u);
            for (uint32_t half = 0; half < 2; half++) {
                for (uint32_t bkt = 0; bkt < kOrderBuckets; bkt++) {
                    if (half == 0) bucket_pos[bkt] = pos;
                    for (unsigned s = 0; s < width; s++) {
                        slices[s].start[half * kOrderBuckets + bkt] = pos;
                        pos += slices[s].hist[half * kOrderBuckets + bkt];
                    }
                }
                if (half == 0) { n_class[0] = pos; bucket_pos[kOrderBuckets] = pos; }
            }
            n_class[1] = pos - n_class[0];
            // every wave item has exactly one launch position (the kernels trust the item array: an item lost or doubled here
            // would be a wild descriptor on the device)
            if (pos != n_witems) return failed(NS_E_STATE, "internal: launch order holds %u of %u work items", pos, n_witems);
            if (!auto_mode) { n_class[0] = n_class[1] = 0; }
            // the consumers of shared top rows: a launch of their own, longest estimated run time first, ties in query order
            uint32_t rpos = 0;
            for (uint32_t bkt = 0; bkt < kOrderBuckets; bkt++)
                for (unsigned s = 0; s < width; s++) {
                    slices[s].start[2 * kOrderBuckets + bkt] = rpos;
                    rpos += slices[s].hist[2 * kOrderBuckets + bkt];
                }
            if (rpos != n_ritems) return failed(NS_E_STATE, "internal: launch order holds %u of %u row consumers", rpos, n_ritems);
        }
        // the workgroup-kernel items (fallback path: few): longest first, serially
        sorted_items.clear();
        if (n_items) {
            struct Cost { uint64_t c; uint32_t slice, idx; };
            std::vector<Cost> ic;
            ic.reserve(n_items);
            for (unsigned s = 0; s < width; s++)
                for (uint32_t i = 0; i < slices[s].items.size(); i++) ic.push_back({slices[s].item_cost[i], s, i});
            std::stable_sort(ic.begin(), ic.end(), [](const Cost& a, const Cost& b) { return a.c > b.c; });
            sorted_items.resize(n_items);
            for (uint32_t i = 0; i < n_items; i++) {
                DevItem it = slices[ic[i].slice].items[ic[i].idx];
                it.out_slot = direct ? it.query : it.out_slot + slices[ic[i].slice].row_off;
                sorted_items[i] = it;
            }
        }
        wide_q.clear();
        if (!direct)
            for (uint32_t q = 0; q < n_queries; q++)
                if (merge_is_wide(dq[q].part_count, k)) wide_q.push_back(q);

        // the descriptor image: the head of the batch's device block, uploaded in one copy
        size_t off = 0;
        layout.items = place_at(off, (size_t)n_items * sizeof(DevItem));
        layout.witems = place_at(off, (size_t)n_witems * sizeof(DevWItem));
        layout.terms = place_at(off, (size_t)(n_dterms + n_pterms) * sizeof(DevTerm));
        layout.groups = place_at(off, (size_t)n_bgroups * sizeof(DevGroup));
        layout.queries = place_at(off, dq.size() * sizeof(DevQuery));
        layout.segs = place_at(off, SV.size() * sizeof(DevSeg));
        layout.wideq = place_at(off, wide_q.size() * 4);
        layout.share = place_at(off, shared ? (share_build.size() + 1) * sizeof(DevShare) : 0);
        layout.ritems = n_ritems ? place_at(off, (size_t)n_ritems * sizeof(DevRItem)) : off;   // (a batch without rows keeps its image byte for byte)
        layout.pitems = n_pitems ? place_at(off, (size_t)n_pitems * sizeof(DevWItem)) : off;
        layout.rstats = n_pitems ? place_at(off, 8) : off;   // k_rscore's two counters: zero in the image, so zeroed by the upload
        layout.bytes = off;

        // The dealing costs host time (a sort per class: +0.2 ms for cfg5's 16384 queries on 8 prepare threads).  A batch small
        // enough to be prepared by fewer than 4 threads over a cache-resident index gains ~1 % of kernel time from it and would
        // pay 0.3 ms of single-threaded sorting per 2048 queries — more than the batch's kernel — so it keeps the plain order
        // (2048-query batches pipelined: 0.71 ms per batch with the dealing, 0.44 without; profiles/r03/final_e2e_*.txt).
        uint64_t resident_bytes = 0;
        for (const SegView& sv : SV) resident_bytes += sv.n_postings * 12ull;
        deal = C.order_mode >= 1 && auto_mode && n_class[0] >= 64 && (width >= 4 || resident_bytes > (256ull << 20) || C.order_mode >= 2);
        // classes of 8 fine buckets while the index fits the 256 MiB Infinity Cache (an L2 miss is cheap there and the
        // longest-first order matters more), of 16 when it does not (20 x 1M docs: L2-miss traffic 31.6 -> 28.6 GB at
        // the same launch time; the 1M-doc index loses 3 % with 32, profiles/r03)
        deal_shift = C.order_coarse_forced ? (uint32_t)C.order_coarse : (resident_bytes > (256ull << 20) ? 4u : 3u);
        return NS_OK;
    }

    // ---- phase C: the descriptors go into `hb` (layout.bytes bytes), wave items at their place in the launch order ----
    void write(char* hb) {
        if (deal && share_at.size() < n_witems) share_at.resize(n_witems);
        fork([&](unsigned si) {
            PrepSlice& S = slices[si];
            DevWItem* wdst = (DevWItem*)(hb + layout.witems);
            for (size_t i = 0; i < S.witems.size(); i++) {
                DevWItem it = S.witems[i];
                it.out_slot = direct ? it.query : it.out_slot + S.row_off;
                const uint32_t bk = S.wbucket[i];
                const uint32_t at = S.start[((bk & 0x8000u) ? kOrderBuckets : 0) + (bk & 0x7FFFu)]++;
                wdst[at] = it;
                if (deal) share_at[at] = S.wshare[i];
            }
            DevRItem* rdst = (DevRItem*)(hb + layout.ritems);
            for (size_t i = 0; i < S.ritems.size(); i++) {
                DevRItem ri = S.ritems[i];
                ri.it.out_slot = direct ? ri.it.query : ri.it.out_slot + S.row_off;
                rdst[S.start[2 * kOrderBuckets + S.rbucket[i]]++] = ri;
            }
            if (!S.dterms.empty()) std::memcpy(hb + layout.terms + (size_t)S.term_off * sizeof(DevTerm), S.dterms.data(), S.dterms.size() * sizeof(DevTerm));
            if (!S.bgroups.empty()) std::memcpy(hb + layout.groups + (size_t)S.bgroup_off * sizeof(DevGroup), S.bgroups.data(), S.bgroups.size() * sizeof(DevGroup));
            for (uint32_t q = S.q0; q < S.q1; q++) dq[q].part_begin += S.row_off;
            if (S.q1 > S.q0) std::memcpy(hb + layout.queries + (size_t)S.q0 * sizeof(DevQuery), dq.data() + S.q0, (size_t)(S.q1 - S.q0) * sizeof(DevQuery));
        });
        // ---- XCD dealing.  The launch order is longest-estimated-run-time first (2048 fine buckets).  Inside a coarse class of
        // 8 fine buckets (run times within ~19 % of each other) the order is free, and it is used for locality: workgroup i
        // runs on XCD i % 8, each XCD has its own 4 MB L2, and items that read the same bytes — same segment, same doc range
        // of the grid, same largest list: the shards of a hot list that dozens of queries of a batch share — should meet
        // in ONE L2 at about the same time, so that one of them pulls a line from HBM and the others hit it.  The items of a
        // class are sorted by their locality key (segment, then doc range, then a hash of the largest list), the sorted
        // sequence is cut into eight equal parts, and XCD x — the launch positions p with p % 8 == x — takes part x in
        // order: one L2 per part of the doc space, neighbours in time share lists.
        // Measured (profiles/r03): 20 x 1M-doc index, L2-miss traffic of the cfg5 launch 44.2 -> 31 GB, 7.05 -> 6.70 ms; the
        // 1M-doc index 2.61 -> 2.56 ms.  (A key quantised to eighths of the doc space lost 3 % there: the exact range matters.)
        // The classes are spread over the prepare threads; a class of n items costs one sort of n 64-bit words.
        if (deal) {
            DevWItem* wd = (DevWItem*)(hb + layout.witems);
            const uint32_t shift = deal_shift, n_cls = kOrderBuckets >> shift;
            if (deal_tmp.size() < width) { deal_tmp.resize(width); deal_key.resize(width); deal_alt.resize(width); deal_bins.resize(width); }
            fork([&](unsigned si) {
                std::vector<DevWItem>& tmp = deal_tmp[si];
                std::vector<uint64_t>& ord = deal_key[si];   // (key << 32 | index in the class): sorted = stable by key
                for (uint32_t c = si; c < n_cls; c += width) {
                    const uint32_t p0 = bucket_pos[c << shift], p1 = bucket_pos[(c + 1) << shift];
                    const uint32_t n = p1 - p0;
                    if (n < 16) continue;
                    ord.resize(n);
                    for (uint32_t i = 0; i < n; i++) ord[i] = ((uint64_t)share_at[p0 + i] << 32) | i;
                    if (n <= 4096) {
                        std::sort(ord.begin(), ord.end());
                    } else {
                        // a large class (all thin items of a batch have about the same run time: 17 000 items in one class of
                        // cfg5) would keep ONE prepare thread in a comparison sort for ~1 ms: two stable counting passes over
                        // the key's halves instead (the index in the low word is ascending already)
                        std::vector<uint64_t>& alt = deal_alt[si];
                        std::vector<uint32_t>& bins = deal_bins[si];
                        alt.resize(n);
                        bins.resize(65537);
                        for (int pass = 0; pass < 2; pass++) {
                            const int sh = 32 + 16 * pass;
                            std::fill(bins.begin(), bins.end(), 0u);
                            const uint64_t* src = pass ? alt.data() : ord.data();
                            uint64_t* dst = pass ? ord.data() : alt.data();
                            for (uint32_t i = 0; i < n; i++) bins[((src[i] >> sh) & 0xFFFFu) + 1u]++;
                            for (uint32_t b2 = 0; b2 < 65536; b2++) bins[b2 + 1] += bins[b2];
                            for (uint32_t i = 0; i < n; i++) dst[bins[(src[i] >> sh) & 0xFFFFu]++] = src[i];
                        }
                    }
                    tmp.assign(wd + p0, wd + p1);
                    uint32_t cur[8], end[8];
                    for (uint32_t x = 0; x < 8; x++) { cur[x] = (uint32_t)((uint64_t)n * x / 8); end[x] = (uint32_t)((uint64_t)n * (x + 1) / 8); }
                    for (uint32_t p = 0; p < n; p++) {
                        uint32_t x = (p0 + p) & 7u;
                        for (uint32_t tr = 0; tr < 8 && cur[x] >= end[x]; tr++) x = (x + 1) & 7u;   // a part one item short of its slots
                        wd[p0 + p] = tmp[(uint32_t)ord[cur[x]++]];
                    }
                }
            });
        }
        if (n_pterms) std::memcpy(hb + layout.terms + (size_t)n_dterms * sizeof(DevTerm), pterms.data(), (size_t)n_pterms * sizeof(DevTerm));
        if (n_pitems) std::memcpy(hb + layout.pitems, pitems.data(), (size_t)n_pitems * sizeof(DevWItem));
        if (n_pitems) std::memset(hb + layout.rstats, 0, 8);
        if (n_items) std::memcpy(hb + layout.items, sorted_items.data(), (size_t)n_items * sizeof(DevItem));
        if (!wide_q.empty()) std::memcpy(hb + layout.wideq, wide_q.data(), wide_q.size() * 4);
        if (shared) {
            std::memcpy(hb + layout.share, share_build.data(), share_build.size() * sizeof(DevShare));
            const DevShare sentinel{0u, 0u, 0.0f, 0u, (uint32_t)share_postings};
            std::memcpy(hb + layout.share + share_build.size() * sizeof(DevShare), &sentinel, sizeof(DevShare));
        }
    }
};

}  // namespace ns
