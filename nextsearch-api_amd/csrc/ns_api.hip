// C-ABI implementation of include/nextsearch_hip.h: context, segment upload (pinned staging),
// batch preparation (term groups -> work items), kernel launches and result fetch.
// No CPU fallback exists in this library: every compute entry point needs a live HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nextsearch_hip.h"
#include "ns_internal.h"
#include "ns_plan.hpp"
#include "ns_kernels.hip"
#include "ns_wave_kernel.hip"
#include "ns_driver_kernel.hip"
#include "ns_prune_kernel.hip"
#include "ns_merge_kernel.hip"
#include "ns_tile_kernel.hip"
#include "ns_row_kernel.hip"   // after ns_tile_kernel.hip (kUscoreWavesPerBlock: the producers are items of k_uscore)
#include "ns_invert.hip"
#include "ns_ingest.hip"
#include "ns_compact.hip"
#include "ns_delete.hip"
#include "ns_filter.hip"
#include "ns_union.hip"    // includes ns_union_plan.hpp (host only: what ns_segment_union plans before it touches the device)
#include "ns_facet.hip"
#include "ns_similar.hip"
#include "ns_terms.hip"     // after ns_similar.hip (ml_shfl, ml_sort_up, ml_join)
#include "ns_terms_plan.hpp"
#include "ns_sorted.hip"   // after ns_facet.hip (fc_cut, fc_mark, fc_lower_bound) and ns_similar.hip (ml_sort_up, ml_merge_down, ml_join)
#include "ns_boolean.hip"  // after ns_sorted.hip (SdSet, sd_insert) and ns_facet.hip (fc_cut, fc_mark)
#include "ns_boolean_sets.hip"  // after ns_boolean.hip (BqRef), ns_sorted.hip (SdSet, sd_key, sd_insert, DevSdSeg, af_clip) and ns_facet.hip
#include "ns_collapse.hip"   // after ns_boolean.hip (CgSet, DevBqGroup) and ns_boolean_sets.hip (bs_matched); includes ns_collapse_plan.hpp (host only)
#include "ns_sem.hip"
#include "ns_suggest.hip"
#include "ns_fuzzy.hip"
#include "ns_call_plan.hpp"   // host only: what a ranked call plans on top of ns_sorted_plan.hpp and ns_after_plan.hpp
#include "ns_radix_plan.hpp"  // host only: the digits of the radix sort in ns_invert.hip, and what the inversion plans
#include "ns_merge_plan.hpp"  // host only: what the merge plans before it touches the device

using namespace ns;

static_assert(sizeof(ns_hit) == sizeof(Hit), "ns_hit layout");


// ------------------------------------------------------------------------------------------------
struct ns_seg {
    ns_ctx* ctx = nullptr;
    uint32_t id = 0;
    uint32_t n_docs = 0;
    uint64_t n_postings = 0;
    uint2* d_postings = nullptr;
    float* d_norm = nullptr;    // per doc
    float* d_pnorm = nullptr;   // per posting
    bool norm_safe = false;     // every norm lies in [2^-20, 2^30]: the BM25 division may take its short form (ns_div_short)
    float avgdl = 0.0f;
    // upload in progress (ns_segment_upload_begin .. _end): payload bytes received so far, doc_len on the device, pinned staging
    bool pending = false;
    uint64_t filled = 0;
    uint32_t* d_len = nullptr;
    void* pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    int stage_k = 0;
    // packed posting stream (ns_segment_build_packed; ns_internal.h kPk*): blocks, per-block headers; the norm index per
    // doc and the table of distinct norms are made at upload (they only exist when the segment has <= 65536 distinct doc lengths)
    uint32_t* d_packed = nullptr;
    uint2* d_pk_hdr = nullptr;
    float* d_pk_scores = nullptr;   // per posting: the impact stream's score alone (built when both streams exist)
    uint16_t* d_nidx = nullptr;
    float* d_ntab = nullptr;
    uint32_t n_norms = 0;
    // Optional impact stream (ns_segment_build_impacts): {docId, term score bits} per posting of the registered lists
    // (lists.imp), index-aligned with d_postings.
    uint2* d_impacts = nullptr;
    // Optional skip tables (ns_segment_build_skips; DevSeg::skips): every registered list (lists.skip) has skip_entries() entries.
    uint32_t* d_skips = nullptr;
    std::vector<uint32_t*> skip_retired;    // outgrown blocks: batches prepared before the growth still point into them
    uint64_t skip_cap = 0, skip_used = 0;   // entries allocated / in use
    uint32_t skip_entries() const { return (n_docs + kSkipDocs - 1) / kSkipDocs + 2; }
    // Optional block maxima (ns_segment_build_blockmax; DevSeg::blockmax): per registered list (lists.bmx) ceil(count / 256) fp32 values.
    float* d_blockmax = nullptr;
    std::vector<float*> bmx_retired;         // outgrown blocks: batches prepared before the growth still point into them
    uint64_t bmx_cap = 0, bmx_used = 0;      // entries allocated / in use
    SegLists lists;   // the host side of the three above and of the shared term scores (ns_plan.hpp)
};

struct ns_ctx {
    // Device blocks of destroyed batches are kept for the next batch (a serving loop prepares batch after batch
    // of similar shape; 14 hipMalloc + 14 hipFree per batch cost more than the descriptors' upload).
    struct Block { void* p; size_t n; };
    std::vector<Block> pool;
    size_t pool_bytes = 0;
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // Batches alternate between the ctx's stream and this second one when overlap is on (ns_ctx_set_overlap): the
    // head of batch i+1 then fills the wave slots that the draining tail of batch i leaves idle.
    hipStream_t alt_stream = nullptr;
    // Large descriptor uploads are pulled by a kernel on a stream of their own (highest priority), so that batch i+1's upload
    // runs NEXT TO batch i's scoring kernel instead of behind it on the batch's stream or in the shared DMA queue.
    hipStream_t pull_stream = nullptr;
    bool overlap = false, flip = false;
    // shared top rows: the producers and consumers of a batch run here, next to its scoring launch (fork after k_share_scores,
    // join in front of k_merge: two events of the batch); without it they run in front of and behind the scoring launch on
    // the batch's stream
    hipStream_t row_stream = nullptr;
    std::string err;
    std::string devname;
    std::vector<ns_seg*> segs;   // indexed by seg_id
    std::vector<ns_seg*> pending_uploads;   // begun (ns_segment_upload_begin), not yet ended or released: freed with the ctx
    // Pinned staging: a batch's descriptor arrays go up in ONE copy and its three result arrays come down in
    // ONE copy (a lone query is otherwise dominated by ten small pageable copies and the syncs they imply).
    void* h_up = nullptr;
    size_t h_up_cap = 0;
    hipEvent_t up_done = nullptr;   // recorded after the upload that reads h_up; waited on before h_up is rewritten
    bool up_busy = false;
    void* h_down = nullptr;
    size_t h_down_cap = 0;
    // A small batch has its result arrays IN h_down (pinned host memory is device-addressable): the kernels
    // write the few hits over PCIe themselves and fetch is a stream sync + memcpy.  One batch at a time owns it.
    struct ns_batch* down_owner = nullptr;
    // pinned result buffers for batches in flight (NS_RUN_FETCH): one per batch between its run and its fetch
    struct DownSlot { void* p = nullptr; size_t cap = 0; bool busy = false; };
    std::vector<DownSlot> down_slots;
    PlanSettings cfg;      // what ns_batch_prepare's planner reads: ns_set_tuning, ns_ctx_use_*, ns_ctx_share_scores, the sweep knobs
    ShareRegistry share;   // every list a sharing batch built (ns_ctx_share_scores) and the sharing batches alive
    BatchPlan plan;        // ns_batch_prepare's host threads and per-thread scratch, kept from batch to batch
    std::vector<ns_ac*> acs;   // autocomplete tables (ns_ac_upload): owned by the ctx, freed by ns_ac_release or ns_ctx_destroy
    std::vector<ns_forward*> fwds;   // live forward-index handles (ns_forward_build, ns_forward_merge): orphaned, not freed, by ns_ctx_destroy
    bool cp_inplace = true;          // ns_forward_merge sorts documents up to kCpDocCut pairs where they lie (ns_ctx_use_docsort)
    std::vector<ns_docterms*> dts;   // live ns_docterms handles (ns_docterms_upload): orphaned, not freed, by ns_ctx_destroy
    uint64_t union_scratch = kUnDefaultScratch;   // table bytes per round of ns_segment_union (ns_ctx_union_scratch)
};

static thread_local std::string g_create_err;
static void ac_free_fwd(ns_ac* ac);
static void forward_orphan_fwd(ns_forward* f);
static void docterms_orphan_fwd(ns_docterms* h);
static void seg_free_device_fwd(ns_seg* s);
static void seg_free_staging_fwd(ns_seg* s);

static int fail(ns_ctx* ctx, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    (ctx ? ctx->err : g_create_err) = vformat(fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail((ctx), NS_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// k_uscore, the unified scoring kernel, over n_items work items of one class (one wave each)
template <int CB, int TMAX, bool IMP, int PK>
static void launch_uscore(bool and_mode, uint32_t n_items, hipStream_t st, const DevWItem* items, const DevTerm* terms,
                          const DevSeg* segs, Hit* hits, uint32_t* nhits, uint64_t* found, uint32_t K) {
    dim3 grid((n_items + kUscoreWavesPerBlock - 1) / kUscoreWavesPerBlock), block(64 * kUscoreWavesPerBlock);
    if (and_mode)
        hipLaunchKernelGGL((k_uscore<512, 192, true, CB, TMAX, IMP, PK>), grid, block, 0, st, items, n_items, terms, segs, hits, nhits, found, K);
    else
        hipLaunchKernelGGL((k_uscore<512, 192, false, CB, TMAX, IMP, PK>), grid, block, 0, st, items, n_items, terms, segs, hits, nhits, found, K);
}
// ... in the instantiation for the streams the batch reads: term scores precomputed (imp) and / or packed blocks (pk)
template <int CB, int TMAX>
static void launch_uscore(bool and_mode, bool imp, int pk, uint32_t n_items, hipStream_t st, const DevWItem* items,
                          const DevTerm* terms, const DevSeg* segs, Hit* hits, uint32_t* nhits, uint64_t* found, uint32_t K) {
    if (imp && pk) launch_uscore<CB, TMAX, true, 1>(and_mode, n_items, st, items, terms, segs, hits, nhits, found, K);   // scores come with the block: no norms at all
    else if (imp) launch_uscore<CB, TMAX, true, 0>(and_mode, n_items, st, items, terms, segs, hits, nhits, found, K);
    else if (pk == 2) launch_uscore<CB, TMAX, false, 2>(and_mode, n_items, st, items, terms, segs, hits, nhits, found, K);
    else if (pk == 1) launch_uscore<CB, TMAX, false, 1>(and_mode, n_items, st, items, terms, segs, hits, nhits, found, K);
    else launch_uscore<CB, TMAX, false, 0>(and_mode, n_items, st, items, terms, segs, hits, nhits, found, K);
}

template <int HK, int FB>
static void launch_dscore(bool and_mode, uint32_t n_items, hipStream_t st, const DevWItem* items, const DevTerm* terms,
                          const DevSeg* segs, Hit* hits, uint32_t* nhits, uint64_t* found, uint32_t K) {
    dim3 grid((n_items + 3) / 4), block(256);
    if (and_mode)
        hipLaunchKernelGGL((k_dscore<HK, FB, true>), grid, block, 0, st, items, n_items, terms, segs, hits, nhits, found, K);
    else
        hipLaunchKernelGGL((k_dscore<HK, FB, false>), grid, block, 0, st, items, n_items, terms, segs, hits, nhits, found, K);
}

template <int TD>
static void launch_tscore(bool and_mode, uint32_t n_items, hipStream_t st, const DevWItem* items, const DevTerm* terms,
                          const DevSeg* segs, Hit* hits, uint32_t* nhits, uint64_t* found, uint32_t K) {
    dim3 grid((n_items + 3) / 4), block(256);
    if (and_mode)
        hipLaunchKernelGGL((k_tscore<TD, true>), grid, block, 0, st, items, n_items, terms, segs, hits, nhits, found, K);
    else
        hipLaunchKernelGGL((k_tscore<TD, false>), grid, block, 0, st, items, n_items, terms, segs, hits, nhits, found, K);
}

template <int NT, int SPT, int U>
static void launch_score(bool and_mode, uint32_t n_items, hipStream_t st, const DevItem* items, const DevTerm* terms,
                         const DevSeg* segs, const uint32_t* bounds, Hit* hits, uint32_t* nhits, uint64_t* found,
                         uint32_t K) {
    if (and_mode)
        hipLaunchKernelGGL((k_score<NT, SPT, U, true>), dim3(n_items), dim3(NT), 0, st, items, terms, segs, bounds, hits, nhits, found, K);
    else
        hipLaunchKernelGGL((k_score<NT, SPT, U, false>), dim3(n_items), dim3(NT), 0, st, items, terms, segs, bounds, hits, nhits, found, K);
}

// ------------------------------------------------------------------------------------------------
extern "C" int ns_ctx_create(int device, ns_ctx** out) {
    if (!out) return fail(nullptr, NS_E_INVAL, "ns_ctx_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, NS_E_NODEVICE, "no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(nullptr, NS_E_INVAL, "device %d out of range [0,%d)", device, ndev);
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, NS_E_NODEVICE, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail(nullptr, NS_E_NODEVICE, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    ns_ctx* ctx = new ns_ctx();
    ctx->device = device;
    ctx->devname = std::string(prop.gcnArchName) + " " + prop.name;
    ctx->cfg.n_cus = prop.multiProcessorCount;
    e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        int rc = fail(nullptr, NS_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
        delete ctx;
        return rc;
    }
    ctx->stream = ctx->own_stream;
    if (const char* om = std::getenv("NS_ORDER_MODE")) ctx->cfg.order_mode = std::atoi(om);
    if (const char* kp = std::getenv("NS_KEY_PCT")) {
        unsigned a = 100, b = 100, c = 100, d = 100;
        if (std::sscanf(kp, "%u,%u,%u,%u", &a, &b, &c, &d) >= 1) { ctx->cfg.key_pct[0] = a; ctx->cfg.key_pct[1] = b; ctx->cfg.key_pct[2] = c; ctx->cfg.key_pct[3] = d; }
    }
    if (const char* td = std::getenv("NS_TILE_DENS64")) ctx->cfg.tile_dens64 = (uint32_t)std::max(1, std::atoi(td));
    if (const char* um = std::getenv("NS_MERGE")) ctx->cfg.use_merge = std::atoi(um) != 0;
    if (const char* mr = std::getenv("NS_MERGE_RATIO")) ctx->cfg.merge_ratio = (uint32_t)std::max(1, std::atoi(mr));
    if (const char* sm = std::getenv("NS_SHARE")) ctx->cfg.share_mode = std::max(0, std::min(2, std::atoi(sm)));
    if (const char* sr = std::getenv("NS_SHARE_RATIO")) ctx->cfg.share_ratio = (uint32_t)std::max(1, std::atoi(sr));
    if (const char* sp = std::getenv("NS_SHARE_MIN")) ctx->cfg.share_min_postings = (uint64_t)std::max(0ll, std::atoll(sp));
    ctx->cfg.row_mode = 1;
    if (const char* rm = std::getenv("NS_SHARE_ROWS")) ctx->cfg.row_mode = std::max(0, std::min(2, std::atoi(rm)));
    if (const char* ru = std::getenv("NS_ROW_MIN_USERS")) ctx->cfg.row_min_users = (uint32_t)std::max(1, std::atoi(ru));
    if (const char* rc = std::getenv("NS_ROW_CELL")) ctx->cfg.row_cell_postings = (uint32_t)std::max(1, std::atoi(rc));
    {
        const char* rf = std::getenv("NS_ROW_FORK");   // 0: the producers stay on the batch's stream (measurements)
        if ((!rf || std::atoi(rf) != 0) && hipStreamCreateWithFlags(&ctx->row_stream, hipStreamNonBlocking) != hipSuccess) { ctx->row_stream = nullptr; (void)hipGetLastError(); }
    }
    ctx->cfg.class_model = 1;
    if (const char* cm = std::getenv("NS_CLASS_MODEL")) ctx->cfg.class_model = std::max(0, std::min(2, std::atoi(cm)));
    if (const char* mg = std::getenv("NS_CLASS_MARGIN")) ctx->cfg.class_margin_pct = (uint32_t)std::max(1, std::atoi(mg));
    if (const char* tc = std::getenv("NS_TILE_COST")) {
        unsigned a = kTileCostTile16, v = kTileCostVisit16, p = kTileCostPosting16;
        if (std::sscanf(tc, "%u,%u,%u", &a, &v, &p) >= 1) { ctx->cfg.tile_cost16[0] = a; ctx->cfg.tile_cost16[1] = v; ctx->cfg.tile_cost16[2] = p; }
    }
    if (const char* oc = std::getenv("NS_ORDER_COARSE")) { ctx->cfg.order_coarse = std::max(0, std::min(11, std::atoi(oc))); ctx->cfg.order_coarse_forced = true; }
    if (hipStreamCreateWithFlags(&ctx->alt_stream, hipStreamNonBlocking) != hipSuccess) { ctx->alt_stream = nullptr; (void)hipGetLastError(); }
    {
        int lo_pri = 0, hi_pri = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri);
        if (hipStreamCreateWithPriority(&ctx->pull_stream, hipStreamNonBlocking, hi_pri) != hipSuccess) { ctx->pull_stream = nullptr; (void)hipGetLastError(); }
    }
    *out = ctx;
    return NS_OK;
}

extern "C" void ns_ctx_destroy(ns_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->alt_stream) (void)hipStreamSynchronize(ctx->alt_stream);
    if (ctx->pull_stream) (void)hipStreamSynchronize(ctx->pull_stream);
    if (ctx->row_stream) (void)hipStreamSynchronize(ctx->row_stream);
    for (ns_seg* s : ctx->segs) {
        if (!s) continue;
        seg_free_device_fwd(s);
        delete s;
    }
    for (ns_seg* s : ctx->pending_uploads) {   // uploads begun and never ended: their HBM, pinned staging and events go with the ctx
        seg_free_staging_fwd(s);
        seg_free_device_fwd(s);
        delete s;
    }
    for (ns_ac* ac : ctx->acs) ac_free_fwd(ac);   // tables still held: their handles die with the ctx
    for (ns_forward* f : ctx->fwds) forward_orphan_fwd(f);   // their device memory goes; the handles stay valid for ns_forward_destroy
    for (ns_docterms* h : ctx->dts) docterms_orphan_fwd(h);  // the same for ns_docterms handles
    for (auto& blk : ctx->pool) (void)hipFree(blk.p);
    if (ctx->h_up) (void)hipHostFree(ctx->h_up);
    if (ctx->h_down) (void)hipHostFree(ctx->h_down);
    for (auto& ds : ctx->down_slots) if (ds.p) (void)hipHostFree(ds.p);
    if (ctx->up_done) (void)hipEventDestroy(ctx->up_done);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    if (ctx->alt_stream) (void)hipStreamDestroy(ctx->alt_stream);
    if (ctx->pull_stream) (void)hipStreamDestroy(ctx->pull_stream);
    if (ctx->row_stream) (void)hipStreamDestroy(ctx->row_stream);
    delete ctx;
}

extern "C" int ns_ctx_set_stream(ns_ctx* ctx, void* hip_stream) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_ctx_set_stream: ctx is NULL");
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return NS_OK;
}

extern "C" const char* ns_last_error(ns_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }
extern "C" const char* ns_device_name(ns_ctx* ctx) { return ctx ? ctx->devname.c_str() : ""; }

extern "C" int ns_set_tuning(ns_ctx* ctx, uint32_t variant, uint32_t min_items, uint32_t split_postings) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_set_tuning: ctx is NULL");
    if (variant >= kNumVariants || kVariants[variant].nt == 0) return fail(ctx, NS_E_INVAL, "unknown kernel variant %u", variant);
#ifndef NS_VARIANTS
    // The product library holds ONE scoring kernel (k_uscore, variant 0) plus k_score as the fallback for term groups of more
    // than 64 terms.  The forced variants — each body as a kernel of its own, other table / tile sizes — exist for the
    // parity tests and for sweeps: `make -C nextsearch-api_amd variants` builds libnextsearch_hip_variants.so with them.
    if (variant != 0) return fail(ctx, NS_E_INVAL, "kernel variant %u exists only in the variants build (make -C nextsearch-api_amd variants)", variant);
#endif
    ctx->cfg.variant = variant;
    ctx->cfg.min_items = min_items;
    ctx->cfg.split_postings = split_postings;
    return NS_OK;
}

// ------------------------------------------------------------------------------------------------
// slack behind the payload: the driver stream loads whole rounds of 256 postings (and their norms) from a list's
// cursor, i.e. up to 255 entries past the end of the last list
static constexpr size_t kPadPostings = 256;
static constexpr size_t kStageChunk = 32u << 20;   // pinned, double-buffered: the host memcpy of chunk i+1 overlaps the DMA of chunk i

static void seg_free_staging(ns_seg* s) {
    for (int i = 0; i < 2; i++) {
        if (s->pin[i]) (void)hipHostFree(s->pin[i]);
        if (s->ev[i]) (void)hipEventDestroy(s->ev[i]);
        s->pin[i] = nullptr; s->ev[i] = nullptr;
    }
    if (s->d_len) (void)hipFree(s->d_len);
    s->d_len = nullptr;
}
static void seg_free_device(ns_seg* s);
static void seg_free_device_fwd(ns_seg* s) { seg_free_device(s); }
static void seg_free_staging_fwd(ns_seg* s) { seg_free_staging(s); }
static void seg_free_device(ns_seg* s) {
    (void)hipFree(s->d_postings);
    (void)hipFree(s->d_norm);
    (void)hipFree(s->d_pnorm);
    (void)hipFree(s->d_impacts);
    (void)hipFree(s->d_packed);
    (void)hipFree(s->d_pk_hdr);
    (void)hipFree(s->d_pk_scores);
    (void)hipFree(s->d_nidx);
    (void)hipFree(s->d_ntab);
    (void)hipFree(s->d_skips);
    for (uint32_t* p : s->skip_retired) (void)hipFree(p);
    s->skip_retired.clear();
    (void)hipFree(s->d_blockmax);
    for (float* p : s->bmx_retired) (void)hipFree(p);
    s->bmx_retired.clear();
    s->d_blockmax = nullptr; s->bmx_cap = s->bmx_used = 0; s->lists.bmx.clear();
    s->d_skips = nullptr; s->skip_cap = s->skip_used = 0; s->lists.skip.clear();
    s->d_postings = nullptr; s->d_norm = nullptr; s->d_pnorm = nullptr; s->d_impacts = nullptr; s->d_packed = nullptr;
    s->d_pk_hdr = nullptr; s->d_pk_scores = nullptr; s->d_nidx = nullptr; s->d_ntab = nullptr;
}
// host bytes -> device through the segment's two pinned buffers
static hipError_t seg_stage(ns_ctx* ctx, ns_seg* s, void* dst, const void* src, size_t n) {
    size_t off = 0;
    while (off < n) {
        const size_t c = std::min(kStageChunk, n - off);
        const int k = s->stage_k;
        hipError_t r = hipEventSynchronize(s->ev[k]);
        if (r != hipSuccess) return r;
        std::memcpy(s->pin[k], (const char*)src + off, c);
        r = hipMemcpyAsync((char*)dst + off, s->pin[k], c, hipMemcpyHostToDevice, ctx->stream);
        if (r != hipSuccess) return r;
        r = hipEventRecord(s->ev[k], ctx->stream);
        if (r != hipSuccess) return r;
        off += c;
        s->stage_k ^= 1;
    }
    return hipSuccess;
}

extern "C" int ns_segment_upload_begin(ns_ctx* ctx, uint32_t seg_id, uint32_t n_docs, float avgdl, const uint32_t* doc_len,
                                       uint64_t nbytes, ns_seg** out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_segment_upload: ctx is NULL");
    if (!out) return fail(ctx, NS_E_INVAL, "ns_segment_upload_begin: out is NULL");
    *out = nullptr;
    if (seg_id >= (1u << 20)) return fail(ctx, NS_E_INVAL, "seg_id %u too large", seg_id);
    if (nbytes % 8 != 0) return fail(ctx, NS_E_INVAL, "posting payload of %llu bytes is not a whole number of {u32,u32} pairs", (unsigned long long)nbytes);
    if (nbytes / 8 >= (1ull << 32)) return fail(ctx, NS_E_INVAL, "segment has %llu postings; this build indexes postings with 32 bits (split the segment)", (unsigned long long)(nbytes / 8));
    if (n_docs && !doc_len) return fail(ctx, NS_E_INVAL, "null doc_len/postings");
    if (seg_id < ctx->segs.size() && ctx->segs[seg_id]) return fail(ctx, NS_E_INVAL, "segment %u already uploaded", seg_id);
    HIPCHK(ctx, hipSetDevice(ctx->device));

    ns_seg* s = new ns_seg();
    s->ctx = ctx;
    s->id = seg_id;
    s->n_docs = n_docs;
    s->n_postings = nbytes / 8;
    s->avgdl = avgdl;
    s->pending = true;
    auto cleanup = [&]() { seg_free_staging(s); seg_free_device(s); delete s; };

    hipError_t e;
    if ((e = hipMalloc((void**)&s->d_postings, nbytes + kPadPostings * 8)) != hipSuccess) { cleanup(); return fail(ctx, NS_E_NOMEM, "hipMalloc postings (%llu B): %s", (unsigned long long)nbytes, hipGetErrorString(e)); }
    if ((e = hipMalloc((void**)&s->d_norm, (size_t)std::max<uint32_t>(n_docs, 1) * 4)) != hipSuccess) { cleanup(); return fail(ctx, NS_E_NOMEM, "hipMalloc norm: %s", hipGetErrorString(e)); }
    if ((e = hipMalloc((void**)&s->d_pnorm, nbytes / 2 + kPadPostings * 4)) != hipSuccess) { cleanup(); return fail(ctx, NS_E_NOMEM, "hipMalloc per-posting norms (%llu B): %s", (unsigned long long)(nbytes / 2), hipGetErrorString(e)); }
    if ((e = hipMalloc((void**)&s->d_len, (size_t)std::max<uint32_t>(n_docs, 1) * 4)) != hipSuccess) { cleanup(); return fail(ctx, NS_E_NOMEM, "hipMalloc doc_len: %s", hipGetErrorString(e)); }
    for (int i = 0; i < 2; i++)
        if (hipHostMalloc(&s->pin[i], kStageChunk, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&s->ev[i], hipEventDisableTiming) != hipSuccess) {
            cleanup();
            return fail(ctx, NS_E_NOMEM, "pinned staging allocation failed");
        }
    e = hipMemsetAsync((char*)s->d_postings + nbytes, 0xFF, kPadPostings * 8, ctx->stream);   // docId ~0: never taken
    if (e == hipSuccess) e = hipMemsetAsync((char*)s->d_pnorm + nbytes / 2, 0, kPadPostings * 4, ctx->stream);
    if (e == hipSuccess && n_docs) e = seg_stage(ctx, s, s->d_len, doc_len, (size_t)n_docs * 4);
    if (e == hipSuccess && n_docs) {
        hipLaunchKernelGGL(k_norm, dim3((n_docs + 255) / 256), dim3(256), 0, ctx->stream, s->d_len, s->d_norm, n_docs, avgdl);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n_docs) {
        // The packed stream's norm plane: a posting carries a 16-bit index into the table of the segment's DISTINCT norms
        // (norm is a function of doc_len alone) instead of the fp32 norm — no quantisation, 2 B instead of 4.  The table is
        // k_norm over the distinct lengths: the same expression on the same inputs, the same bits.  Segments with more
        // than 65536 distinct lengths get no table (and no packed stream).
        uint32_t max_len = 0;
        for (uint32_t i = 0; i < n_docs; i++) max_len = std::max(max_len, doc_len[i]);
        std::vector<uint32_t> uniq;
        std::vector<uint16_t> nidx;
        if (max_len < (1u << 24)) {
            std::vector<uint32_t> rank((size_t)max_len + 1, 0u);
            for (uint32_t i = 0; i < n_docs; i++) rank[doc_len[i]] = 1u;
            for (uint32_t v = 0; v <= max_len; v++)
                if (rank[v]) { rank[v] = (uint32_t)uniq.size(); uniq.push_back(v); }
            if (uniq.size() <= 65536) {
                nidx.resize(n_docs);
                for (uint32_t i = 0; i < n_docs; i++) nidx[i] = (uint16_t)rank[doc_len[i]];
            }
        } else {
            uniq.assign(doc_len, doc_len + n_docs);
            std::sort(uniq.begin(), uniq.end());
            uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
            if (uniq.size() <= 65536) {
                nidx.resize(n_docs);
                for (uint32_t i = 0; i < n_docs; i++) nidx[i] = (uint16_t)(std::lower_bound(uniq.begin(), uniq.end(), doc_len[i]) - uniq.begin());
            }
        }
        if (!nidx.empty()) {
            uint32_t* d_ulen = nullptr;
            const size_t D = uniq.size();
            e = hipMalloc((void**)&s->d_nidx, (size_t)n_docs * 2);
            if (e == hipSuccess) e = hipMalloc((void**)&s->d_ntab, D * 4);
            if (e == hipSuccess) e = hipMalloc((void**)&d_ulen, D * 4);
            if (e == hipSuccess) e = seg_stage(ctx, s, s->d_nidx, nidx.data(), (size_t)n_docs * 2);
            if (e == hipSuccess) e = seg_stage(ctx, s, d_ulen, uniq.data(), D * 4);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_norm, dim3((uint32_t)((D + 255) / 256)), dim3(256), 0, ctx->stream, d_ulen, s->d_ntab, (uint32_t)D, avgdl);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // d_ulen and the host vectors die here
            (void)hipFree(d_ulen);
            s->n_norms = (uint32_t)D;
        }
    }
    if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); cleanup(); return fail(ctx, NS_E_HIP, "segment upload: %s", hipGetErrorString(e)); }
    {
        // norms are monotone in doc_len (k_norm's expression, evaluated here the same way): the extremes bound them all
        uint32_t dl_min = 0xFFFFFFFFu, dl_max = 0;
        for (uint32_t i = 0; i < n_docs; i++) { dl_min = std::min(dl_min, doc_len[i]); dl_max = std::max(dl_max, doc_len[i]); }
        auto norm_of = [&](uint32_t dl) { return 1.2f * ((1.0f - 0.75f) + 0.75f * ((float)dl / avgdl)); };
        const float lo_ok = 9.5367431640625e-07f /* 2^-20 */, hi_ok = 1073741824.0f /* 2^30 */;
        s->norm_safe = n_docs > 0 && std::isfinite(avgdl) && avgdl > 0.0f && norm_of(dl_min) >= lo_ok && norm_of(dl_min) <= hi_ok &&
                       norm_of(dl_max) >= lo_ok && norm_of(dl_max) <= hi_ok;
    }
    ctx->pending_uploads.push_back(s);
    *out = s;
    return NS_OK;
}

extern "C" int ns_segment_upload_append(ns_ctx* ctx, ns_seg* s, const void* bytes, uint64_t nbytes) {
    if (!ctx || !s || s->ctx != ctx || !s->pending) return fail(ctx, NS_E_STATE, "ns_segment_upload_append: no upload in progress for this segment");
    if (nbytes % 8 != 0) return fail(ctx, NS_E_INVAL, "chunk of %llu bytes is not a whole number of {u32,u32} pairs", (unsigned long long)nbytes);
    if (s->filled + nbytes > s->n_postings * 8) return fail(ctx, NS_E_INVAL, "chunk runs past the %llu payload bytes announced at begin", (unsigned long long)(s->n_postings * 8));
    if (nbytes && !bytes) return fail(ctx, NS_E_INVAL, "null doc_len/postings");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const hipError_t e = seg_stage(ctx, s, (char*)s->d_postings + s->filled, bytes, nbytes);
    if (e != hipSuccess) return fail(ctx, NS_E_HIP, "segment upload: %s", hipGetErrorString(e));
    s->filled += nbytes;
    return NS_OK;
}

extern "C" int ns_segment_upload_end(ns_ctx* ctx, ns_seg* s) {
    if (!ctx || !s || s->ctx != ctx || !s->pending) return fail(ctx, NS_E_STATE, "ns_segment_upload_end: no upload in progress for this segment");
    if (s->filled != s->n_postings * 8) return fail(ctx, NS_E_STATE, "ns_segment_upload_end: %llu of %llu payload bytes received", (unsigned long long)s->filled, (unsigned long long)(s->n_postings * 8));
    if (s->id < ctx->segs.size() && ctx->segs[s->id]) return fail(ctx, NS_E_INVAL, "segment %u already uploaded", s->id);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipSuccess;
    if (s->n_postings) {
        uint32_t blocks = (uint32_t)std::min<uint64_t>((s->n_postings + 255) / 256, 65536);
        hipLaunchKernelGGL(k_pnorm, dim3(blocks), dim3(256), 0, ctx->stream, s->d_postings, s->d_norm, s->d_pnorm, s->n_postings, s->n_docs);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, NS_E_HIP, "segment upload: %s", hipGetErrorString(e));
    seg_free_staging(s);
    s->pending = false;
    ctx->pending_uploads.erase(std::remove(ctx->pending_uploads.begin(), ctx->pending_uploads.end(), s), ctx->pending_uploads.end());
    if (ctx->segs.size() <= s->id) ctx->segs.resize(s->id + 1, nullptr);
    ctx->segs[s->id] = s;
    return NS_OK;
}

extern "C" int ns_segment_upload(ns_ctx* ctx, uint32_t seg_id, uint32_t n_docs, float avgdl, const uint32_t* doc_len,
                                 const void* postings, uint64_t nbytes, ns_seg** out) {
    if (out) *out = nullptr;
    if (ctx && nbytes && !postings) return fail(ctx, NS_E_INVAL, "null doc_len/postings");
    ns_seg* s = nullptr;
    int rc = ns_segment_upload_begin(ctx, seg_id, n_docs, avgdl, doc_len, nbytes, &s);
    if (rc != NS_OK) return rc;
    rc = ns_segment_upload_append(ctx, s, postings, nbytes);
    if (rc == NS_OK) rc = ns_segment_upload_end(ctx, s);
    if (rc != NS_OK) { const std::string keep = ctx->err; (void)ns_segment_release(ctx, s); ctx->err = keep; return rc; }
    if (out) *out = s;
    return NS_OK;
}

extern "C" int ns_segment_release(ns_ctx* ctx, ns_seg* seg) {
    if (!ctx || !seg) return fail(ctx, NS_E_INVAL, "ns_segment_release: null argument");
    if (seg->ctx != ctx) return fail(ctx, NS_E_INVAL, "segment does not belong to this ctx");
    if (!seg->pending && (seg->id >= ctx->segs.size() || ctx->segs[seg->id] != seg)) return fail(ctx, NS_E_INVAL, "segment does not belong to this ctx");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->alt_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->alt_stream));
    if (ctx->pull_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->pull_stream));
    seg_free_staging(seg);
    seg_free_device(seg);
    // the shared-score registry forgets the segment's lists: a later segment under the same id starts with an empty interval map
    // and must see every one of its lists as new (that is when overlaps are checked)
    if (!seg->pending) ctx->share.tab.erase_if([&](uint64_t key, const ShareRegistry::Ent&) { return (uint32_t)(key >> 32) == seg->id; });
    if (!seg->pending) ctx->segs[seg->id] = nullptr;
    else ctx->pending_uploads.erase(std::remove(ctx->pending_uploads.begin(), ctx->pending_uploads.end(), seg), ctx->pending_uploads.end());
    delete seg;
    return NS_OK;
}

__global__ void __launch_bounds__(256) k_pk_scores(const uint2* __restrict__ impacts, float* __restrict__ scores, uint64_t n) {
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) scores[p] = __uint_as_float(impacts[p].y);
}
// the packed form of the impact stream = the scores alone, per posting (the docIds come from the packed doc plane)
static hipError_t seg_fill_pk_scores(ns_ctx* ctx, ns_seg* seg) {
    if (!seg->d_packed || !seg->d_impacts || !seg->n_postings) return hipSuccess;
    const uint64_t n = seg->n_postings + kPadPostings;
    hipError_t e = hipSuccess;
    if (!seg->d_pk_scores) e = hipMalloc((void**)&seg->d_pk_scores, n * 4);
    if (e != hipSuccess) { seg->d_pk_scores = nullptr; return e; }
    hipLaunchKernelGGL(k_pk_scores, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 16)), dim3(256), 0, ctx->stream, seg->d_impacts, seg->d_pk_scores, n);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e;
}

// One thread per posting: the list that holds it is found by binary search over the (sorted) list starts.
// The arithmetic is src/api_engine.cpp:477-479 operation for operation with the compiler's IEEE division —
// the expression the scoring kernels evaluate per posting per query when no impact stream exists.
__global__ void __launch_bounds__(256) k_build_impacts(const uint2* __restrict__ postings, const float* __restrict__ pnorm,
                                                       uint2* __restrict__ impacts, const uint32_t* __restrict__ starts,
                                                       const uint32_t* __restrict__ counts, const float* __restrict__ idfs,
                                                       uint32_t n_lists, uint64_t n_postings) {
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n_postings; p += (uint64_t)gridDim.x * 256) {
        uint32_t lo = 0, hi = n_lists;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if ((uint64_t)starts[mid] <= p) lo = mid + 1; else hi = mid;
        }
        if (lo == 0) continue;
        const uint32_t l = lo - 1;
        if (p - starts[l] >= counts[l]) continue;
        const uint2 pv = postings[p];
        const float tf = (float)pv.y;
        const float den = tf + pnorm[p];
        const float num = idfs[l] * (tf * (1.2f + 1.0f));
        impacts[p] = make_uint2(pv.x, __float_as_uint(num / den));
    }
}

// the lists [byte_off / 8, + count) given to a ns_segment_build_* call: byte offsets a multiple of 8, lists inside the segment
static int check_lists(ns_ctx* ctx, const ns_seg* seg, const uint64_t* byte_off, const uint32_t* counts, uint32_t n_lists) {
    for (uint32_t i = 0; i < n_lists; i++) {
        if (byte_off[i] % 8 != 0) return fail(ctx, NS_E_INVAL, "list %u: byte offset %llu is not a multiple of 8", i, (unsigned long long)byte_off[i]);
        if (byte_off[i] / 8 + counts[i] > seg->n_postings) return fail(ctx, NS_E_INVAL, "list %u runs past the segment's postings", i);
    }
    return NS_OK;
}

extern "C" int ns_segment_build_impacts(ns_ctx* ctx, ns_seg* seg, const uint64_t* byte_off, const uint32_t* counts,
                                        const float* idfs, uint32_t n_lists) {
    if (!ctx || !seg) return fail(ctx, NS_E_INVAL, "ns_segment_build_impacts: null argument");
    if (seg->id >= ctx->segs.size() || ctx->segs[seg->id] != seg) return fail(ctx, NS_E_INVAL, "segment does not belong to this ctx");
    if (n_lists && (!byte_off || !counts || !idfs)) return fail(ctx, NS_E_INVAL, "null list arrays");
    if (!n_lists || !seg->n_postings) return NS_OK;
    if (ctx->share.live) return fail(ctx, NS_E_STATE, "ns_segment_build_impacts: %u batch(es) that compute shared term scores into the same buffer are alive; destroy them first", ctx->share.live);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = check_lists(ctx, seg, byte_off, counts, n_lists)) return rc;
    struct L { uint32_t first, count; float idf; };
    std::vector<L> lists;
    lists.reserve(n_lists);
    for (uint32_t i = 0; i < n_lists; i++)
        if (counts[i]) lists.push_back({(uint32_t)(byte_off[i] / 8), counts[i], idfs[i]});
    std::sort(lists.begin(), lists.end(), [](const L& a, const L& b) { return a.first < b.first; });
    for (size_t i = 1; i < lists.size(); i++)
        if (lists[i - 1].first + (uint64_t)lists[i - 1].count > lists[i].first) return fail(ctx, NS_E_INVAL, "lists overlap at posting %u", lists[i].first);
    if (lists.empty()) return NS_OK;
    hipError_t e = hipSuccess;
    if (!seg->d_impacts) {
        e = hipMalloc((void**)&seg->d_impacts, (seg->n_postings + kPadPostings) * 8);
        if (e != hipSuccess) { seg->d_impacts = nullptr; return fail(ctx, NS_E_NOMEM, "hipMalloc impact stream (%llu B): %s", (unsigned long long)(seg->n_postings * 8), hipGetErrorString(e)); }
        e = hipMemsetAsync(seg->d_impacts, 0xFF, (seg->n_postings + kPadPostings) * 8, ctx->stream);   // docId ~0: never taken
    }
    const size_t n = lists.size();
    std::vector<uint32_t> h_starts(n), h_counts(n);
    std::vector<float> h_idfs(n);
    for (size_t i = 0; i < n; i++) { h_starts[i] = lists[i].first; h_counts[i] = lists[i].count; h_idfs[i] = lists[i].idf; }
    uint32_t* d_tmp = nullptr;
    if (e == hipSuccess) e = hipMalloc((void**)&d_tmp, n * 12);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tmp, h_starts.data(), n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tmp + n, h_counts.data(), n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tmp + 2 * n, h_idfs.data(), n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((seg->n_postings + 255) / 256, 1u << 16);
        hipLaunchKernelGGL(k_build_impacts, dim3(blocks), dim3(256), 0, ctx->stream, seg->d_postings, seg->d_pnorm, seg->d_impacts,
                           d_tmp, d_tmp + n, (const float*)(d_tmp + 2 * n), (uint32_t)n, seg->n_postings);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_tmp);
    if (e == hipSuccess) e = seg_fill_pk_scores(ctx, seg);
    if (e != hipSuccess) return fail(ctx, NS_E_HIP, "ns_segment_build_impacts: %s", hipGetErrorString(e));
    for (const auto& l : lists) {   // a list given again replaces its entry
        uint32_t ib; std::memcpy(&ib, &l.idf, 4);
        seg->lists.imp.put(l.first, {l.count, ib});
    }
    return NS_OK;
}

// ---- shared term scores -------------------------------------------------------------------------------------------
// A batch names the same posting list many times (cfg5: 16384 queries draw ~50 000 term refs from ~40 000 distinct lists, and
// the 32 hot lists ~460 times each): the BM25 term score of a posting, src/api_engine.cpp:477-479, depends on the list and on
// the list's idf, not on the query.  A sharing batch therefore computes the scores of every DISTINCT list it names once, in
// this kernel, in front of its scoring kernel and on every run (nothing is kept from one batch for the next: a later batch
// finds the buffer as if it had never been written), and the scoring bodies read {docId, score bits} — their IMP form, the one
// that serves the optional impact stream — instead of {docId, tf} + norm.  Same operations, same order, same bits: the
// division below is the compiler's correctly rounded one, which ns_div_short reproduces exactly where it is used.
// 1024 consecutive postings of the batch's build order per workgroup; a thread finds the list of each of its postings by
// binary search between the lists that hold the workgroup's first and last posting.
__global__ void __launch_bounds__(256) k_share_scores(const DevShare* __restrict__ sh, uint32_t n_lists, const DevSeg* __restrict__ segs) {
    const uint32_t total = sh[n_lists].before;
    const uint32_t base = blockIdx.x * 1024u;
    if (base >= total) return;
    const uint32_t last = min(base + 1023u, total - 1u);
    __shared__ uint32_t s_lo, s_hi;
    if (threadIdx.x < 2) {
        const uint32_t want = threadIdx.x == 0 ? base : last;   // the list l with sh[l].before <= want < sh[l + 1].before
        uint32_t lo = 0, hi = n_lists;
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (sh[mid].before <= want) lo = mid; else hi = mid;
        }
        if (threadIdx.x == 0) s_lo = lo; else s_hi = lo;
    }
    __syncthreads();
    const uint32_t l0 = s_lo, l1 = s_hi;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t p = base + (uint32_t)j * 256u + threadIdx.x;
        if (p > last) continue;
        uint32_t lo = l0, hi = l1 + 1u;
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (sh[mid].before <= p) lo = mid; else hi = mid;
        }
        const DevShare L = sh[lo];
        const DevSeg& sg = segs[L.seg];
        const uint64_t at = (uint64_t)L.first + (p - L.before);
        const uint2 pv = sg.postings[at];
        const float tf = (float)pv.y;
        const float den = tf + sg.pnorm[at];
        const float num = L.idf * (tf * (1.2f + 1.0f));
        const_cast<uint2*>(sg.impacts)[at] = make_uint2(pv.x, __float_as_uint(num / den));
    }
}

extern "C" int ns_ctx_share_scores(ns_ctx* ctx, int mode) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_ctx_share_scores: ctx is NULL");
    if (mode < 0 || mode > 2) return fail(ctx, NS_E_INVAL, "ns_ctx_share_scores: mode %d outside [0, 2]", mode);
    ctx->cfg.share_mode = mode;
    return NS_OK;
}

extern "C" int ns_ctx_share_rows(ns_ctx* ctx, int mode) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_ctx_share_rows: ctx is NULL");
    if (mode < 0 || mode > 2) return fail(ctx, NS_E_INVAL, "ns_ctx_share_rows: mode %d outside [0, 2]", mode);
    ctx->cfg.row_mode = mode;
    return NS_OK;
}

extern "C" int ns_ctx_class_model(ns_ctx* ctx, int mode) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_ctx_class_model: ctx is NULL");
    if (mode < 0 || mode > 2) return fail(ctx, NS_E_INVAL, "ns_ctx_class_model: mode %d outside [0, 2]", mode);
    ctx->cfg.class_model = mode;
    return NS_OK;
}

// sweeps only (tools/class_fit.py): see PlanSettings::force_body
extern "C" int ns_ctx_class_force(ns_ctx* ctx, uint32_t body, uint32_t share10, uint32_t dens64_lo, uint32_t dens64_hi) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_ctx_class_force: ctx is NULL");
    if (body > 2 || share10 > 9 || dens64_lo > dens64_hi) return fail(ctx, NS_E_INVAL, "ns_ctx_class_force: body %u, share tenth %u, density [%u, %u)", body, share10, dens64_lo, dens64_hi);
    ctx->cfg.force_body = body; ctx->cfg.force_share10 = share10; ctx->cfg.force_dens_lo = dens64_lo; ctx->cfg.force_dens_hi = dens64_hi;
    return NS_OK;
}

extern "C" int ns_segment_build_packed(ns_ctx* ctx, ns_seg* seg) {
    if (!ctx || !seg) return fail(ctx, NS_E_INVAL, "ns_segment_build_packed: null argument");
    if (seg->pending || seg->id >= ctx->segs.size() || ctx->segs[seg->id] != seg) return fail(ctx, NS_E_INVAL, "segment does not belong to this ctx");
    if (seg->d_packed || !seg->n_postings) return NS_OK;
    if (!seg->d_nidx) return fail(ctx, NS_E_INVAL, "ns_segment_build_packed: segment %u has more than 65536 distinct document lengths; its norms do not fit a 16-bit index", seg->id);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t n_blocks = (seg->n_postings + kPkBlock - 1) / kPkBlock;
    hipError_t e = hipMalloc((void**)&seg->d_packed, (n_blocks + 2) * kPkStrideDwords * 4);   // + slack: a round may be planned one block past the end
    if (e == hipSuccess) e = hipMalloc((void**)&seg->d_pk_hdr, (n_blocks + 2) * sizeof(uint2));
    if (e == hipSuccess) e = hipMemsetAsync(seg->d_packed + n_blocks * kPkStrideDwords, 0, 2 * kPkStrideDwords * 4, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(seg->d_pk_hdr + n_blocks, 0, 2 * sizeof(uint2), ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_pack, dim3((uint32_t)n_blocks), dim3(64), 0, ctx->stream, seg->d_postings, seg->d_nidx, seg->d_packed, seg->d_pk_hdr,
                           seg->n_postings, seg->n_docs, (uint32_t)n_blocks);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = seg_fill_pk_scores(ctx, seg);
    if (e != hipSuccess) {
        (void)hipFree(seg->d_packed); (void)hipFree(seg->d_pk_hdr);
        seg->d_packed = nullptr; seg->d_pk_hdr = nullptr;
        return fail(ctx, e == hipErrorOutOfMemory ? NS_E_NOMEM : NS_E_HIP, "ns_segment_build_packed: %s", hipGetErrorString(e));
    }
    return NS_OK;
}

// ---- skip tables (block metadata next to the reference's posting format) --------------------------------
// entry[l][i] = index of list l's first posting with docId >= i * kSkipDocs.  k_skip_fill: every entry = the list's end;
// k_skip_build: one thread per posting p of a registered list — the grid cells after the previous posting's, up to its own,
// start at p (docIds ascend inside a list, so every cell is written at most once); k_skip_check: a table is usable when
// it starts at the list's first posting, never decreases and ends at the list's end (an unsorted list fails here and
// simply keeps no table: its groups take the cursor path, which tolerates any order).
__global__ void __launch_bounds__(256) k_skip_fill(uint32_t* __restrict__ sk, const uint32_t* __restrict__ starts, const uint32_t* __restrict__ counts,
                                                   uint32_t per_list) {
    const uint32_t l = blockIdx.y;
    const uint32_t endp = starts[l] + counts[l];
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < per_list; i += gridDim.x * 256) sk[(uint64_t)l * per_list + i] = endp;
}
__global__ void __launch_bounds__(256) k_skip_build(const uint2* __restrict__ postings, uint32_t* __restrict__ sk, const uint32_t* __restrict__ starts,
                                                    const uint32_t* __restrict__ counts, uint32_t per_list) {
    const uint32_t l = blockIdx.y;
    const uint32_t first = starts[l], n = counts[l];
    uint32_t* row = sk + (uint64_t)l * per_list;
    const uint32_t cells = per_list - 2;   // entries 0 .. cells are cell starts (cells = one past the last doc's), + 1 spare
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t d = postings[first + i].x / kSkipDocs;
        uint32_t c0 = 0;
        if (i) {
            const uint32_t dp = postings[first + i - 1].x / kSkipDocs;
            c0 = dp + 1;
        }
        for (uint32_t c = c0; c <= d && c <= cells; c++) row[c] = first + i;
    }
}
__global__ void __launch_bounds__(256) k_skip_check(const uint2* __restrict__ postings, const uint32_t* __restrict__ sk, const uint32_t* __restrict__ starts,
                                                    const uint32_t* __restrict__ counts, uint32_t per_list, uint32_t* __restrict__ bad) {
    const uint32_t l = blockIdx.y;
    const uint32_t first = starts[l], endp = first + counts[l];
    const uint32_t* row = sk + (uint64_t)l * per_list;
    bool b = false;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i + 1 < per_list; i += gridDim.x * 256) {
        const uint32_t a = row[i], z = row[i + 1];
        if (a > z || a < first || z > endp) b = true;
        if (i == 0 && a != first) b = true;
        if (i + 2 == per_list && (z != endp || a != endp)) b = true;
        // the postings of cell i really are inside it (first and last suffice: the list ascends between table entries
        // or the next cell's check fails)
        if (i + 2 < per_list && a < z) {
            if (postings[a].x / kSkipDocs != i || postings[z - 1].x / kSkipDocs != i) b = true;
        }
    }
    if (b) bad[l] = 1u;
}

extern "C" int ns_segment_build_skips(ns_ctx* ctx, ns_seg* seg, const uint64_t* byte_off, const uint32_t* counts, uint32_t n_lists) {
    if (!ctx || !seg) return fail(ctx, NS_E_INVAL, "ns_segment_build_skips: null argument");
    if (seg->pending || seg->id >= ctx->segs.size() || ctx->segs[seg->id] != seg) return fail(ctx, NS_E_INVAL, "segment does not belong to this ctx");
    if (n_lists && (!byte_off || !counts)) return fail(ctx, NS_E_INVAL, "null list arrays");
    if (!n_lists || !seg->n_postings || !seg->n_docs) return NS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = check_lists(ctx, seg, byte_off, counts, n_lists)) return rc;
    struct L { uint32_t first, count; };
    std::vector<L> lists;
    lists.reserve(n_lists);
    for (uint32_t i = 0; i < n_lists; i++)
        if (counts[i] && !seg->lists.skip_of((uint32_t)(byte_off[i] / 8), counts[i])) lists.push_back({(uint32_t)(byte_off[i] / 8), counts[i]});
    std::sort(lists.begin(), lists.end(), [](const L& a, const L& b) { return a.first < b.first || (a.first == b.first && a.count < b.count); });
    lists.erase(std::unique(lists.begin(), lists.end(), [](const L& a, const L& b) { return a.first == b.first; }), lists.end());
    if (lists.empty()) return NS_OK;
    const uint32_t per_list = seg->skip_entries();
    const size_t n = lists.size();
    const uint64_t need = seg->skip_used + (uint64_t)n * per_list;
    if (need >= (1ull << 32) - 1) return fail(ctx, NS_E_INVAL, "ns_segment_build_skips: %llu table entries do not fit 32 bits", (unsigned long long)need);
    hipError_t e = hipSuccess;
    if (need > seg->skip_cap) {   // grow (tables already built are kept: batches prepared earlier hold indices into them)
        uint32_t* bigger = nullptr;
        const uint64_t cap = std::max<uint64_t>(need, seg->skip_cap * 2);
        e = hipMalloc((void**)&bigger, cap * 4);
        if (e != hipSuccess) return fail(ctx, NS_E_NOMEM, "hipMalloc skip tables (%llu B): %s", (unsigned long long)(cap * 4), hipGetErrorString(e));
        if (seg->d_skips) {   // the old block stays until the segment goes: earlier batches point into it
            e = hipMemcpyAsync(bigger, seg->d_skips, seg->skip_used * 4, hipMemcpyDeviceToDevice, ctx->stream);
            seg->skip_retired.push_back(seg->d_skips);
        }
        seg->d_skips = bigger;
        seg->skip_cap = cap;
        if (e != hipSuccess) return fail(ctx, NS_E_HIP, "ns_segment_build_skips: %s", hipGetErrorString(e));
    }
    std::vector<uint32_t> h(n * 3, 0u);
    for (size_t i = 0; i < n; i++) { h[i] = lists[i].first; h[n + i] = lists[i].count; }
    uint32_t* d_tmp = nullptr;
    e = hipMalloc((void**)&d_tmp, n * 12);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tmp, h.data(), n * 12, hipMemcpyHostToDevice, ctx->stream);
    uint32_t* base = seg->d_skips + seg->skip_used;
    if (e == hipSuccess) {
        const dim3 g1((per_list + 255) / 256 > 64 ? 64 : (per_list + 255) / 256, (uint32_t)n);
        hipLaunchKernelGGL(k_skip_fill, g1, dim3(256), 0, ctx->stream, base, d_tmp, d_tmp + n, per_list);
        uint32_t cmax = 0;
        for (const auto& l : lists) cmax = std::max(cmax, l.count);
        const dim3 g2(std::min<uint32_t>((cmax + 255) / 256, 1024u), (uint32_t)n);
        hipLaunchKernelGGL(k_skip_build, g2, dim3(256), 0, ctx->stream, seg->d_postings, base, d_tmp, d_tmp + n, per_list);
        hipLaunchKernelGGL(k_skip_check, g1, dim3(256), 0, ctx->stream, seg->d_postings, base, d_tmp, d_tmp + n, per_list, d_tmp + 2 * n);
        e = hipGetLastError();
    }
    std::vector<uint32_t> bad(n, 1u);
    if (e == hipSuccess) e = hipMemcpyAsync(bad.data(), d_tmp + 2 * n, n * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_tmp);
    if (e != hipSuccess) return fail(ctx, NS_E_HIP, "ns_segment_build_skips: %s", hipGetErrorString(e));
    // registry (a list that is not ascending gets no table; a list registered already, under another count, keeps its entry)
    for (size_t i = 0; i < n; i++)
        if (!bad[i] && !seg->lists.skip.find(lists[i].first)) seg->lists.skip.put(lists[i].first, {lists[i].count, (uint32_t)(seg->skip_used + i * per_list)});
    seg->skip_used = need;
    return NS_OK;
}

// Block maxima of the given lists (DevSeg::blockmax; ns_prune_kernel.hip): per 256 postings of a list the largest BM25 term
// score with the given idf.  Lists given again (same first posting) are rebuilt with the new idf; tables already built stay
// where they are (batches prepared earlier hold indices into them).
extern "C" int ns_segment_build_blockmax(ns_ctx* ctx, ns_seg* seg, const uint64_t* byte_off, const uint32_t* counts, const float* idfs, uint32_t n_lists) {
    if (!ctx || !seg) return fail(ctx, NS_E_INVAL, "ns_segment_build_blockmax: null argument");
    if (seg->pending || seg->id >= ctx->segs.size() || ctx->segs[seg->id] != seg) return fail(ctx, NS_E_INVAL, "segment does not belong to this ctx");
    if (n_lists && (!byte_off || !counts || !idfs)) return fail(ctx, NS_E_INVAL, "null list arrays");
    if (!n_lists || !seg->n_postings) return NS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = check_lists(ctx, seg, byte_off, counts, n_lists)) return rc;
    struct L { uint32_t first, count; float idf; uint32_t entry; };
    std::vector<L> lists;
    lists.reserve(n_lists);
    for (uint32_t i = 0; i < n_lists; i++) {
        uint32_t ib; std::memcpy(&ib, &idfs[i], 4);
        if (counts[i] && !seg->lists.bmx_of((uint32_t)(byte_off[i] / 8), counts[i], ib)) lists.push_back({(uint32_t)(byte_off[i] / 8), counts[i], idfs[i], 0u});
    }
    std::sort(lists.begin(), lists.end(), [](const L& a, const L& b) { return a.first < b.first; });
    lists.erase(std::unique(lists.begin(), lists.end(), [](const L& a, const L& b) { return a.first == b.first; }), lists.end());
    if (lists.empty()) return NS_OK;
    uint64_t need = seg->bmx_used;
    uint32_t bmax_blocks = 0;
    for (auto& l : lists) {
        const uint32_t nb = (l.count + kBmxBlock - 1) / kBmxBlock;
        l.entry = (uint32_t)need;
        need += nb;
        bmax_blocks = std::max(bmax_blocks, nb);
    }
    if (need + 64 >= (1ull << 32) - 1) return fail(ctx, NS_E_INVAL, "ns_segment_build_blockmax: %llu entries do not fit 32 bits", (unsigned long long)need);
    hipError_t e = hipSuccess;
    if (need + 64 > seg->bmx_cap) {   // +64: a wave reads 64 maxima at a time, possibly past a list's last block
        float* bigger = nullptr;
        const uint64_t cap = std::max<uint64_t>(need + 64, seg->bmx_cap * 2);
        e = hipMalloc((void**)&bigger, cap * 4);
        if (e != hipSuccess) return fail(ctx, NS_E_NOMEM, "hipMalloc block maxima (%llu B): %s", (unsigned long long)(cap * 4), hipGetErrorString(e));
        e = hipMemsetAsync(bigger, 0, cap * 4, ctx->stream);
        if (e == hipSuccess && seg->d_blockmax) {
            e = hipMemcpyAsync(bigger, seg->d_blockmax, seg->bmx_used * 4, hipMemcpyDeviceToDevice, ctx->stream);
            seg->bmx_retired.push_back(seg->d_blockmax);
        }
        seg->d_blockmax = bigger;
        seg->bmx_cap = cap;
        if (e != hipSuccess) return fail(ctx, NS_E_HIP, "ns_segment_build_blockmax: %s", hipGetErrorString(e));
    }
    const size_t n = lists.size();
    std::vector<uint32_t> h(n * 4);
    for (size_t i = 0; i < n; i++) {
        h[i] = lists[i].first; h[n + i] = lists[i].count;
        std::memcpy(&h[2 * n + i], &lists[i].idf, 4);
        h[3 * n + i] = lists[i].entry;
    }
    uint32_t* d_tmp = nullptr;
    e = hipMalloc((void**)&d_tmp, n * 16);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tmp, h.data(), n * 16, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        for (size_t l0 = 0; l0 < n; l0 += 32768) {   // grid.y is limited to 65535
            const uint32_t ny = (uint32_t)std::min<size_t>(32768, n - l0);
            hipLaunchKernelGGL(k_blockmax, dim3(std::min<uint32_t>(std::max<uint32_t>(bmax_blocks, 1u), 256u), ny), dim3(64), 0, ctx->stream,
                               seg->d_postings, seg->d_pnorm, seg->d_blockmax, d_tmp + l0, d_tmp + n + l0, (const float*)(d_tmp + 2 * n + l0), d_tmp + 3 * n + l0);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_tmp);
    if (e != hipSuccess) return fail(ctx, NS_E_HIP, "ns_segment_build_blockmax: %s", hipGetErrorString(e));
    seg->bmx_used = need;
    for (const auto& l : lists) {   // a list given again: the later table wins
        uint32_t ib; std::memcpy(&ib, &l.idf, 4);
        seg->lists.bmx.put(l.first, {l.count, ib, l.entry});
    }
    return NS_OK;
}

extern "C" int ns_ctx_use_merge(ns_ctx* ctx, int on) {
    if (!ctx) return NS_E_INVAL;
    ctx->cfg.use_merge = on != 0;
    return NS_OK;
}

extern "C" int ns_ctx_use_pruning(ns_ctx* ctx, int on) {
    if (!ctx) return NS_E_INVAL;
    ctx->cfg.use_pruning = on != 0;
    return NS_OK;
}

extern "C" int ns_ctx_use_skips(ns_ctx* ctx, int on) {
    if (!ctx) return NS_E_INVAL;
    ctx->cfg.use_skips = on != 0;
    return NS_OK;
}

extern "C" int ns_ctx_use_packed(ns_ctx* ctx, int on) {
    if (!ctx) return NS_E_INVAL;
    if (on < 0 || on > 2) return fail(ctx, NS_E_INVAL, "ns_ctx_use_packed: mode %d (0, 1 or 2)", on);
    ctx->cfg.use_packed = on;
    return NS_OK;
}

extern "C" int ns_ctx_set_overlap(ns_ctx* ctx, int on) {
    if (!ctx) return NS_E_INVAL;
    if (on && !ctx->alt_stream) return fail(ctx, NS_E_HIP, "ns_ctx_set_overlap: the second stream could not be created");
    ctx->overlap = on != 0;
    return NS_OK;
}

extern "C" int ns_ctx_set_host_threads(ns_ctx* ctx, uint32_t n) {
    if (!ctx) return NS_E_INVAL;
    if (n > 64) return fail(ctx, NS_E_INVAL, "ns_ctx_set_host_threads: %u threads (at most 64)", n);
    ctx->cfg.prep_threads = n;
    return NS_OK;
}

extern "C" int ns_ctx_use_impacts(ns_ctx* ctx, int on) {
    if (!ctx) return NS_E_INVAL;
    ctx->cfg.use_impacts = on != 0;
    return NS_OK;
}

// ------------------------------------------------------------------------------------------------
struct ns_batch {
    ns_ctx* ctx = nullptr;
    uint32_t Q = 0, K = 0, flags = 0;
    uint32_t variant = 0, tile_docs = 0, hb = 0;
    uint32_t n_items = 0;      // workgroup-kernel items (k_score)
    uint32_t n_witems = 0;     // wave-kernel items
    uint32_t n_class[3] = {0, 0, 0};   // auto mode: items of class S (thin foreign lists), D (dense foreign), T (very dense: doc tiles); contiguous in d_witems
    uint32_t n_bgroups = 0;    // term groups that need the boundary prepass (k_score path only)
    uint32_t n_terms = 0, n_parts = 0;
    uint64_t postings = 0;
    bool direct = false;   // every query has exactly one work item: the scoring kernel writes final rows
    int pk = 0;            // every segment of the batch has a packed posting stream and the ctx wants it: 1 = packed docIds + tf, norms from the fp32 norm stream; 2 = norms through the 16-bit norm index (ns_ctx_use_packed)
    bool pruned = false;   // some single-term items take the block-max pruned body (ns_ctx_use_pruning)
    bool imp = false;      // every list of the batch has an impact stream: the kernels read {docId, score} instead of {docId, tf} + norm
    bool shared = false;   // ... because the batch computes them itself, once per distinct list and run (k_share_scores; ns_ctx_share_scores)
    uint32_t n_share = 0;          // distinct lists the batch builds
    uint64_t share_postings = 0;   // their postings
    DevShare* d_share = nullptr;   // n_share + 1 entries
    // shared top rows (ns_ctx_share_rows): producer items (k_uscore with K' = kRowLen into the row buffer), consumer items (k_rscore)
    uint32_t n_pitems = 0, n_ritems = 0;
    uint32_t class_stats[4] = {0, 0, 0, 0};   // ns_batch_class_stats
    DevWItem* d_pitems = nullptr;
    DevRItem* d_ritems = nullptr;
    Hit* d_row_hits = nullptr;         // kRowLen entries per producer item
    uint32_t* d_row_nhits = nullptr;
    uint64_t* d_row_found = nullptr;
    uint32_t* d_row_stats = nullptr;   // over the batch's runs: fallbacks, row entries that hit the table
    hipEvent_t row_fork = nullptr, row_join = nullptr;
    // device
    DevItem* d_items = nullptr;
    DevWItem* d_witems = nullptr;
    DevTerm* d_terms = nullptr;
    DevGroup* d_groups = nullptr;
    DevQuery* d_queries = nullptr;
    DevSeg* d_segs = nullptr;
    uint32_t* d_bounds = nullptr;
    Hit* d_part_hits = nullptr;
    uint32_t* d_part_nhits = nullptr;
    uint64_t* d_part_found = nullptr;
    uint32_t* d_heads = nullptr;
    Hit* d_hits = nullptr;
    uint32_t* d_nhits = nullptr;
    uint64_t* d_found = nullptr;
    // active output pointers (own or bound)
    Hit* o_hits = nullptr;
    uint32_t* o_nhits = nullptr;
    uint64_t* o_found = nullptr;
    // timed runs: four events per run (start, before scoring, after scoring, end), read back at sync
    std::vector<hipEvent_t> ev_pool;
    size_t ev_pending = 0;          // events recorded since the last sync
    bool ran = false;
    float last_score_ms = -1.0f, last_total_ms = -1.0f;
    double sum_score_ms = 0.0, sum_total_ms = 0.0;
    uint32_t timed_runs = 0;
    uint32_t* d_wide_q = nullptr;
    uint32_t n_wide_q = 0;
    size_t out_span = 0, off_nhits = 0, off_found = 0;   // [d_hits .. d_found end) is one contiguous span of the block
    std::vector<std::pair<void*, size_t>> blocks;   // every device block of this batch (returned to the ctx pool on destroy)
    // pipelined use (NS_RUN_FETCH): the results' D2H copy into a pinned slot of the ctx is enqueued right behind the
    // kernels and `done` is recorded after it, so that fetch / destroy wait for THIS batch only, not for the stream
    hipStream_t st = nullptr;  // the stream all of this batch's work goes to (the ctx's, or its second one when overlap is on)
    hipEvent_t done = nullptr;
    bool done_recorded = false;
    bool fetch_enqueued = false;   // the last run carried NS_RUN_FETCH
    int down_slot = -1;        // index into ns_ctx::down_slots while a D2H copy is pending or unread
};

static constexpr size_t kPoolMaxBytes = 1ull << 30;   // cached blocks beyond this are released
static constexpr size_t kStageMaxBytes = 256ull << 20;   // larger batches upload/fetch array by array
static constexpr size_t kPullUploadBytes = 256 << 10;     // uploads up to this size are pulled by a kernel instead of the DMA engine
static constexpr size_t kHostResultBytes = 64 << 10;      // result arrays up to this size live in pinned host memory

// Block sizes are quantised (powers of two from 64 KB to 64 MB, multiples of 16 MB above) so that a serving loop's
// batches of slightly different shape reuse each other's blocks instead of going to hipMalloc.
static size_t pool_quantise(size_t n) {
    if (n <= (64u << 10)) return 64u << 10;
    if (n <= (64u << 20)) { size_t q = 64u << 10; while (q < n) q <<= 1; return q; }
    return (n + (16u << 20) - 1) & ~(size_t)((16u << 20) - 1);
}
static hipError_t pool_alloc(ns_ctx* ctx, void** out, size_t n) {
    n = pool_quantise(n);
    size_t best = (size_t)-1;
    for (size_t i = 0; i < ctx->pool.size(); i++)
        if (ctx->pool[i].n >= n && ctx->pool[i].n <= 2 * n + 4096 && (best == (size_t)-1 || ctx->pool[i].n < ctx->pool[best].n)) best = i;
    if (best != (size_t)-1) {
        *out = ctx->pool[best].p;
        ctx->pool_bytes -= ctx->pool[best].n;
        ctx->pool[best] = ctx->pool.back();
        ctx->pool.pop_back();
        return hipSuccess;
    }
    hipError_t e = hipMalloc(out, n);
    if (e == hipErrorOutOfMemory && !ctx->pool.empty()) {   // give the cache back and try once more
        for (auto& b : ctx->pool) (void)hipFree(b.p);
        ctx->pool.clear(); ctx->pool_bytes = 0;
        e = hipMalloc(out, n);
    }
    return e;
}
// caller has synchronised the stream: nothing in flight uses the block
static void pool_free(ns_ctx* ctx, void* p, size_t n) {
    if (!p) return;
    n = pool_quantise(n);
    if (ctx->pool_bytes + n > kPoolMaxBytes || ctx->pool.size() >= 64) { (void)hipFree(p); return; }
    ctx->pool.push_back({p, n});
    ctx->pool_bytes += n;
}

// ------------------------------------------------------------------------------------------------
// The scaffold of a pooled one-shot call.
// The device blocks of one call: regions laid out with place_at, pooled allocations, the call's events and the first HIP
// error.  reserve() everything, alloc(), then work on the stream only while ok(); finish() on every path after alloc().
// A call that sizes a further block by what it read back from an earlier one goes on with open(), reserve() and alloc():
// at(off), upload(), zero() and fetch() address the newest block, at(off, b) the one that alloc() numbered b.
struct CallBlock {
    struct Held { char* p; size_t n; };
    ns_ctx* ctx;
    hipStream_t st;
    size_t bytes = 0;              // the layout cursor of the block being laid out
    char* blk = nullptr;           // the newest block
    std::vector<Held> held;        // every block the call holds, in order of allocation
    std::vector<hipEvent_t> evs;   // none in a call that times nothing
    hipError_t e = hipSuccess;

    explicit CallBlock(ns_ctx* c) : ctx(c), st(c->stream) {}
    void chk(hipError_t r) { if (e == hipSuccess) e = r; }
    bool ok() const { return e == hipSuccess; }
    size_t reserve(size_t n) { return place_at(bytes, n); }   // (a region of no bytes still takes a place)
    void open() { bytes = 0; }
    size_t alloc(size_t n_events) {
        blk = nullptr;
        const hipError_t r = pool_alloc(ctx, (void**)&blk, bytes);
        chk(r);
        if (r != hipSuccess) { blk = nullptr; return held.size(); }   // no block, no events: the call is not ok() from here on
        held.push_back({blk, bytes});
        for (size_t i = 0; i < n_events; i++) { hipEvent_t ev = nullptr; chk(hipEventCreate(&ev)); evs.push_back(ev); }
        return held.size() - 1;   // the block's number for at(off, b)
    }
    template <class T> T* at(size_t off) const { return (T*)(blk + off); }
    template <class T> T* at(size_t off, size_t b) const { return (T*)(held[b].p + off); }
    size_t held_bytes() const { size_t n = 0; for (auto& h : held) n += h.n; return n; }
    void upload(size_t off, const void* src, size_t n) { if (n) chk(hipMemcpyAsync(blk + off, src, n, hipMemcpyHostToDevice, st)); }
    void zero(size_t off, size_t n) { chk(hipMemsetAsync(blk + off, 0, n, st)); }
    void fetch(void* dst, size_t off, size_t n) { chk(hipMemcpyAsync(dst, blk + off, n, hipMemcpyDeviceToHost, st)); }
    void record(size_t ev) { if (ev < evs.size()) chk(hipEventRecord(evs[ev], st)); }
    void launched() { chk(hipGetLastError()); }
    void sync() { chk(hipStreamSynchronize(st)); }
    // the interval between two recorded events, once the call has synchronised without an error
    bool elapsed_ms(size_t first, size_t second, float* ms) const {
        return ok() && first < evs.size() && second < evs.size() && hipEventElapsedTime(ms, evs[first], evs[second]) == hipSuccess;
    }
    // the blocks go back to the pool, newest first, only once nothing in flight uses them, whatever failed before;
    // `what` replaces the error's own text in the message
    int finish(const char* fn, const char* what = nullptr) {
        if (!held.empty()) (void)hipStreamSynchronize(st);
        for (size_t b = held.size(); b-- > 0;) pool_free(ctx, held[b].p, held[b].n);
        for (auto& ev : evs) if (ev) (void)hipEventDestroy(ev);
        if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? NS_E_NOMEM : NS_E_HIP, "%s: %s", fn, what ? what : hipGetErrorString(e));
        return NS_OK;
    }
};

// Host memory for one call's upload image (`up` bytes) and, with down != 0, its result image: the ctx's pinned staging
// buffers where they are free and hold the image (grown to n + n / 2, at least 64 KiB; nothing above kStageMaxBytes is
// pinned, and h_down is a batch's while it has an owner), pageable memory of the call's own otherwise.
struct Staged {
    char *up = nullptr, *down = nullptr;
    bool up_pinned = false;
    std::vector<char> up_own, down_own;
};
static hipError_t stage_host(ns_ctx* ctx, size_t up, size_t down, Staged& s) {
    if (ctx->up_busy) {   // a batch's upload may still be reading the staging buffer
        const hipError_t e = hipEventSynchronize(ctx->up_done);
        ctx->up_busy = false;
        if (e != hipSuccess) return e;
    }
    if (up <= kStageMaxBytes && ctx->h_up_cap < up) {
        if (ctx->h_up) (void)hipHostFree(ctx->h_up);
        ctx->h_up = nullptr; ctx->h_up_cap = 0;
        const size_t cap = std::max<size_t>(up + up / 2, 1 << 16);
        if (hipHostMalloc(&ctx->h_up, cap, hipHostMallocDefault) == hipSuccess) ctx->h_up_cap = cap;
        else { ctx->h_up = nullptr; (void)hipGetLastError(); }
    }
    s.up_pinned = ctx->h_up_cap >= up;
    s.up = s.up_pinned ? (char*)ctx->h_up : (s.up_own.resize(up), s.up_own.data());
    if (!down) return hipSuccess;
    const bool down_free = !ctx->down_owner && down <= kStageMaxBytes;
    if (down_free && ctx->h_down_cap < down) {
        if (ctx->h_down) (void)hipHostFree(ctx->h_down);
        ctx->h_down = nullptr; ctx->h_down_cap = 0;
        const size_t cap = std::max<size_t>(down + down / 2, 1 << 16);
        if (hipHostMalloc(&ctx->h_down, cap, hipHostMallocDefault) == hipSuccess) ctx->h_down_cap = cap;
        else { ctx->h_down = nullptr; (void)hipGetLastError(); }
    }
    s.down = (down_free && ctx->h_down_cap >= down) ? (char*)ctx->h_down : (s.down_own.resize(down), s.down_own.data());
    return hipSuccess;
}

__global__ void __launch_bounds__(256) k_pull(uint4* __restrict__ dst, const uint4* __restrict__ src, uint32_t n16) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}

extern "C" void ns_batch_destroy(ns_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    // nothing of THIS batch may still be in flight when its blocks go back to the pool; later batches on the same
    // stream are none of its business (a pipelined caller destroys batch i while batch i+1 runs)
    if (b->done_recorded) (void)hipEventSynchronize(b->done);
    else (void)hipStreamSynchronize(b->st);
    if (b->ctx->down_owner == b) b->ctx->down_owner = nullptr;
    if (b->down_slot >= 0) b->ctx->down_slots[(size_t)b->down_slot].busy = false;
    if (b->shared && b->ctx->share.live) b->ctx->share.live--;
    for (auto& blk : b->blocks) pool_free(b->ctx, blk.first, blk.second);
    for (auto& e : b->ev_pool) if (e) (void)hipEventDestroy(e);
    if (b->done) (void)hipEventDestroy(b->done);
    if (b->row_fork) (void)hipEventDestroy(b->row_fork);
    if (b->row_join) (void)hipEventDestroy(b->row_join);
    delete b;
}

static hipError_t batch_alloc(ns_batch* b, void** dptr, size_t n) {
    hipError_t e = pool_alloc(b->ctx, dptr, n);
    if (e == hipSuccess) b->blocks.push_back({*dptr, n});
    return e;
}
// ---- a batch: planned on the host (ns_plan.hpp), then one device block, the descriptor image staged and uploaded --------
extern "C" int ns_batch_prepare(ns_ctx* ctx, const ns_query_desc* queries, const ns_term_ref* terms, uint32_t n_queries,
                                uint32_t k, uint32_t flags, ns_batch** out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_batch_prepare: ctx is NULL");
    if (!out) return fail(ctx, NS_E_INVAL, "ns_batch_prepare: out is NULL");
    *out = nullptr;
    if (k < 1 || k > NS_MAX_K) return fail(ctx, NS_E_INVAL, "k=%u outside [1,%u]", k, NS_MAX_K);
    if (n_queries && !queries) return fail(ctx, NS_E_INVAL, "queries is NULL");
    if (flags & ~NS_FLAG_AND) return fail(ctx, NS_E_INVAL, "unknown flags 0x%x", flags);
    HIPCHK(ctx, hipSetDevice(ctx->device));

    // the segments as the planner sees them, and the per-batch segment table (n_tiles depends on the workgroup-kernel variant)
    const VariantDesc vd = kVariants[ctx->cfg.variant];
    const uint32_t tile_docs = vd.nt * vd.spt;
    std::vector<SegView> views(ctx->segs.size());
    std::vector<DevSeg> segs(ctx->segs.size());
    for (size_t i = 0; i < ctx->segs.size(); i++) {
        DevSeg d{};
        if (ns_seg* s = ctx->segs[i]) {
            d.postings = s->d_postings;
            d.pnorm = s->d_pnorm;
            d.impacts = s->d_impacts;
            d.packed = s->d_packed;
            d.pk_hdr = s->d_pk_hdr;
            d.ntab = s->d_ntab;
            d.pk_scores = s->d_pk_scores;
            d.skips = s->d_skips;
            d.blockmax = s->d_blockmax;
            d.norm = s->d_norm;
            d.n_postings = s->n_postings;
            d.n_docs = s->n_docs;
            d.n_tiles = (s->n_docs + tile_docs - 1) / tile_docs;
            views[i] = SegView{s->n_docs, d.n_tiles, s->n_postings, s->norm_safe, s->d_packed != nullptr, &s->lists};
        }
        segs[i] = d;
    }

    BatchPlan& P = ctx->plan;
    int rc = P.group(ctx->cfg, views, ctx->share, queries, terms, n_queries, k, flags);
    if (rc != NS_OK) return fail(ctx, rc, "%s", P.err.c_str());
    for (size_t i = 0; P.shared && i < P.share_build.size(); i++) {   // the score buffers of the segments the batch builds into
        ns_seg* sg = ctx->segs[P.share_build[i].seg];
        if (!sg->d_impacts) {
            const size_t nb = (size_t)(sg->n_postings + kPadPostings) * 8;
            hipError_t ea = hipMalloc((void**)&sg->d_impacts, nb);
            if (ea == hipSuccess) ea = hipMemsetAsync(sg->d_impacts, 0xFF, nb, ctx->stream);   // docId ~0: never taken
            if (ea == hipSuccess) ea = hipStreamSynchronize(ctx->stream);
            if (ea != hipSuccess) {   // no room for the scores: the batch scores in place
                if (sg->d_impacts) (void)hipFree(sg->d_impacts);
                sg->d_impacts = nullptr; (void)hipGetLastError();
                P.shared = false;
            }
        }
        if (P.shared) segs[P.share_build[i].seg].impacts = sg->d_impacts;
    }
    rc = P.cut();
    if (rc != NS_OK) return fail(ctx, rc, "%s", P.err.c_str());

    ns_batch* b = new ns_batch();
    b->ctx = ctx;
    b->st = ctx->stream;
    if (ctx->overlap && ctx->stream == ctx->own_stream && ctx->alt_stream) {   // (an externally owned stream is never second-guessed)
        ctx->flip = !ctx->flip;
        if (ctx->flip) b->st = ctx->alt_stream;
    }
    b->Q = n_queries; b->K = k; b->flags = flags;
    b->variant = ctx->cfg.variant; b->tile_docs = tile_docs; b->hb = vd.hb;
    b->n_items = P.n_items; b->n_witems = P.n_witems;
    b->n_bgroups = P.n_bgroups; b->n_terms = P.n_dterms;
    for (int c = 0; c < 3; c++) b->n_class[c] = P.n_class[c];
    b->n_parts = P.direct ? 0 : P.n_rows;
    b->postings = P.postings_total;
    b->direct = P.direct;
    b->imp = P.all_imp && P.postings_total > 0;
    if (P.shared) {
        b->shared = true;
        b->n_share = (uint32_t)P.share_build.size();
        b->share_postings = P.share_postings;
        ctx->share.live++;
    }
    b->pk = (P.all_pk && P.postings_total > 0) ? ctx->cfg.use_packed : 0;
    b->pruned = P.pruned;
    b->n_wide_q = (uint32_t)P.wide_q.size();
    b->n_pitems = P.n_pitems; b->n_ritems = P.n_ritems;
    std::memcpy(b->class_stats, P.class_stats, sizeof(b->class_stats));

    // One device block per batch: [descriptors, uploaded in one copy][scratch][hits | nhits | found, fetched in one copy]
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    const BatchPlan::Layout& L = P.layout;   // the descriptor image ...
    const size_t up_bytes = L.bytes;
    size_t off = up_bytes;                   // ... and behind it
    auto place = [&](size_t bytes) { return place_at(off, bytes); };
    const size_t Qn = std::max<uint32_t>(n_queries, 1), Pn = std::max<uint32_t>(b->n_parts, 1);
    const size_t o_bounds = place(P.bounds_total * 4);
    size_t o_phits = 0, o_pnhits = 0, o_pfound = 0, o_heads = 0;
    if (!P.direct) {
        o_phits = place(Pn * k * sizeof(Hit));
        o_pnhits = place(Pn * 4);
        o_pfound = place(Pn * 8);
        o_heads = place(Pn * 4);
    }
    size_t o_rhits = 0, o_rnhits = 0, o_rfound = 0;
    if (b->n_pitems) {   // the row buffer: one row of kRowLen hits per producer item
        o_rhits = place((size_t)b->n_pitems * kRowLen * sizeof(Hit));
        o_rnhits = place((size_t)b->n_pitems * 4);
        o_rfound = place((size_t)b->n_pitems * 8);
    }
    const size_t o_hits = place(Qn * k * sizeof(Hit));
    const size_t o_nhits = place(Qn * 4);
    const size_t o_found = place(Qn * 8);
    char* base = nullptr;
    chk(batch_alloc(b, (void**)&base, off));
    if (e == hipSuccess) {
        b->d_items = (decltype(b->d_items))(base + L.items);
        b->d_witems = (decltype(b->d_witems))(base + L.witems);
        b->d_terms = (decltype(b->d_terms))(base + L.terms);
        b->d_groups = (decltype(b->d_groups))(base + L.groups);
        b->d_queries = (decltype(b->d_queries))(base + L.queries);
        b->d_segs = (decltype(b->d_segs))(base + L.segs);
        b->d_wide_q = (uint32_t*)(base + L.wideq);
        b->d_share = (DevShare*)(base + L.share);
        b->d_bounds = (uint32_t*)(base + o_bounds);
        if (b->n_pitems) {
            b->d_pitems = (DevWItem*)(base + L.pitems);
            b->d_ritems = (DevRItem*)(base + L.ritems);
            b->d_row_hits = (Hit*)(base + o_rhits);
            b->d_row_nhits = (uint32_t*)(base + o_rnhits);
            b->d_row_found = (uint64_t*)(base + o_rfound);
            b->d_row_stats = (uint32_t*)(base + L.rstats);   // zero in the descriptor image
        }
        if (!P.direct) {
            b->d_part_hits = (Hit*)(base + o_phits);
            b->d_part_nhits = (uint32_t*)(base + o_pnhits);
            b->d_part_found = (uint64_t*)(base + o_pfound);
            b->d_heads = (uint32_t*)(base + o_heads);
        }
        b->d_hits = (Hit*)(base + o_hits);
        b->d_nhits = (uint32_t*)(base + o_nhits);
        b->d_found = (uint64_t*)(base + o_found);
        b->out_span = o_found + Qn * 8 - o_hits;
        b->off_nhits = o_nhits - o_hits;
        b->off_found = o_found - o_hits;
        if (b->out_span <= kHostResultBytes && !ctx->down_owner) {
            if (ctx->h_down_cap < b->out_span) {
                if (ctx->h_down) (void)hipHostFree(ctx->h_down);
                ctx->h_down = nullptr; ctx->h_down_cap = 0;
                if (hipHostMalloc(&ctx->h_down, kHostResultBytes, hipHostMallocDefault) == hipSuccess) ctx->h_down_cap = kHostResultBytes;
                else { ctx->h_down = nullptr; (void)hipGetLastError(); }
            }
            if (ctx->h_down_cap >= b->out_span) {
                ctx->down_owner = b;
                b->d_hits = (Hit*)ctx->h_down;
                b->d_nhits = (uint32_t*)((char*)ctx->h_down + b->off_nhits);
                b->d_found = (uint64_t*)((char*)ctx->h_down + b->off_found);
            }
        }
    }
    Staged stage;   // (the previous batch's upload may still be reading the staging buffer: stage_host waits for it)
    if (e == hipSuccess) chk(stage_host(ctx, up_bytes, 0, stage));
    if (e == hipSuccess && !ctx->up_done) chk(hipEventCreateWithFlags(&ctx->up_done, hipEventDisableTiming));
    if (e == hipSuccess) {
        // ---- the descriptors go straight into the pinned staging buffer (or, for a batch too large for it, into a host
        // vector that is copied array by array) ----
        const bool staged = stage.up_pinned;
        char* hb = stage.up;
        P.write(hb);
        if (!segs.empty()) std::memcpy(hb + L.segs, segs.data(), segs.size() * sizeof(segs[0]));
        if (staged) {
            // a small upload is pulled by a kernel (the pinned buffer is device-addressable): a DMA-engine copy
            // followed by a kernel costs ~11 us of cross-engine hand-over, more than the copy itself
            // ... and with batches alternating between two streams (ns_ctx_set_overlap) EVERY upload is pulled: copies of all
            // streams go through one in-order DMA queue, where batch i+1's upload would sit behind batch i's result copy
            // — i.e. wait for batch i's kernels — and batch i+1's kernels with it (measured: 0.12 ms between consecutive
            // batches on two streams, as much as on one)
            // A LARGE upload (a 16384-query batch: 2.7 MB; 4096 queries over 8 segments: 6.5 MB = 0.2-0.25 ms) is pulled on the
            // ctx's pull stream and the batch's stream waits for it: it then runs next to the previous batch's scoring kernel
            // on one stream as on two.
            if (up_bytes > kPullUploadBytes && ctx->pull_stream) {
                hipLaunchKernelGGL(k_pull, dim3((uint32_t)((up_bytes / 16 + 255) / 256)), dim3(256), 0, ctx->pull_stream,
                                   (uint4*)base, (const uint4*)hb, (uint32_t)(up_bytes / 16));
                chk(hipEventRecord(ctx->up_done, ctx->pull_stream));
                chk(hipStreamWaitEvent(b->st, ctx->up_done, 0));
            } else {
                if (up_bytes <= kPullUploadBytes || ctx->overlap)
                    hipLaunchKernelGGL(k_pull, dim3((uint32_t)((up_bytes / 16 + 255) / 256)), dim3(256), 0, b->st,
                                       (uint4*)base, (const uint4*)hb, (uint32_t)(up_bytes / 16));
                else
                    chk(hipMemcpyAsync(base, hb, up_bytes, hipMemcpyHostToDevice, b->st));
                chk(hipEventRecord(ctx->up_done, b->st));
            }
            if (e == hipSuccess) ctx->up_busy = true;
        } else {
            chk(hipMemcpyAsync(base, hb, up_bytes, hipMemcpyHostToDevice, b->st));
            chk(hipStreamSynchronize(b->st));   // the copy reads a host vector that dies with this call
        }
    }
    if (e != hipSuccess) {
        rc = fail(ctx, e == hipErrorOutOfMemory ? NS_E_NOMEM : NS_E_HIP, "ns_batch_prepare: %s", hipGetErrorString(e));
        ns_batch_destroy(b);
        return rc;
    }
    b->o_hits = b->d_hits; b->o_nhits = b->d_nhits; b->o_found = b->d_found;
    *out = b;
    return NS_OK;
}

extern "C" int ns_batch_bind_outputs(ns_batch* b, void* d_hits, void* d_nhits, void* d_found) {
    if (!b) return NS_E_INVAL;
    b->o_hits = d_hits ? (Hit*)d_hits : b->d_hits;
    b->o_nhits = d_nhits ? (uint32_t*)d_nhits : b->d_nhits;
    b->o_found = d_found ? (uint64_t*)d_found : b->d_found;
    return NS_OK;
}

extern "C" int ns_batch_run(ns_batch* b, int run_flags) {
    if (!b) return NS_E_INVAL;
    ns_ctx* ctx = b->ctx;
    const int timed = run_flags & NS_RUN_TIMED;
    // preconditions are checked BEFORE anything is enqueued, and the previous run's completion event stops counting from
    // here on: whatever early return follows, ns_batch_destroy then falls back to synchronising the batch's stream instead
    // of trusting an event that lies before kernels of this run
    if (run_flags & NS_RUN_FETCH) {
        const bool own_outputs = b->o_hits == b->d_hits && b->o_nhits == b->d_nhits && b->o_found == b->d_found;
        if (!own_outputs) return fail(ctx, NS_E_STATE, "NS_RUN_FETCH: the batch writes into caller-bound device buffers (ns_batch_bind_outputs); there is nothing to fetch");
    }
    b->done_recorded = false;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = b->st;
    const bool and_mode = (b->flags & NS_FLAG_AND) != 0;
    hipEvent_t* ev = nullptr;
    if (timed) {
        while (b->ev_pool.size() < b->ev_pending + 4) {
            hipEvent_t e = nullptr;
            HIPCHK(ctx, hipEventCreate(&e));
            b->ev_pool.push_back(e);
        }
        ev = b->ev_pool.data() + b->ev_pending;
        b->ev_pending += 4;
    }
    if (timed) HIPCHK(ctx, hipEventRecord(ev[0], st));
    if (b->n_bgroups)
        hipLaunchKernelGGL(k_bounds, dim3(b->n_bgroups), dim3(128), 0, st, b->d_groups, b->d_terms, b->d_segs, b->d_bounds, b->tile_docs);
    if (timed) HIPCHK(ctx, hipEventRecord(ev[1], st));
    // shared term scores: every distinct list of the batch once, on every run, inside the scoring kernel's timed span
    if (b->shared && b->n_share)
        hipLaunchKernelGGL(k_share_scores, dim3((uint32_t)((b->share_postings + 1023) / 1024)), dim3(256), 0, st, b->d_share, b->n_share, b->d_segs);
    Hit* sh = b->direct ? b->o_hits : b->d_part_hits;
    uint32_t* sn = b->direct ? b->o_nhits : b->d_part_nhits;
    uint64_t* sf = b->direct ? b->o_found : b->d_part_found;
    // shared top rows, producers: the hot lists' cells as single-term items of the scoring kernel's own instantiation with
    // K' = kRowLen (CB = 128 holds K' + 64), into the row buffer; next to the scoring launch when the ctx has the side stream
    const bool rows = b->n_pitems && b->n_ritems && b->variant == 0;
    bool row_forked = false;
    if (rows) {
        hipStream_t ps = st;
        if (ctx->row_stream) {
            if (!b->row_fork) HIPCHK(ctx, hipEventCreateWithFlags(&b->row_fork, hipEventDisableTiming));
            if (!b->row_join) HIPCHK(ctx, hipEventCreateWithFlags(&b->row_join, hipEventDisableTiming));
            HIPCHK(ctx, hipEventRecord(b->row_fork, st));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->row_stream, b->row_fork, 0));
            ps = ctx->row_stream;
            row_forked = true;
        }
        launch_uscore<128, 16>(false, true, 0, b->n_pitems, ps, b->d_pitems, b->d_terms, b->d_segs, b->d_row_hits, b->d_row_nhits, b->d_row_found, kRowLen);
        // ... and the consumers right behind them: they wait for the producers alone (stream order), not for the scoring launch,
        // whose wave slots they fill as it drains — launched after it they were a serial tail of 0.3 ms (profiles/row_share)
        if (row_forked) {
            hipLaunchKernelGGL((k_rscore<512, 128, 16>), dim3(b->n_ritems), dim3(64), 0, ps, b->d_ritems, b->n_ritems, b->d_terms, b->d_segs,
                               b->d_row_hits, b->d_row_nhits, sh, sn, sf, b->K, b->d_row_stats);
            HIPCHK(ctx, hipEventRecord(b->row_join, ps));
        }
    }
    if (b->n_witems && b->variant == 0) {
        // auto mode: ONE launch; each wave picks the body that suits its item (DevWItem::whole bit 1)
        // K <= 64: a 128-entry candidate buffer is enough (K + 64 appended per step at most) and its
        // smaller LDS footprint admits more workgroups per CU.  Groups of <= 16 terms (all but exotic
        // queries) run in the instantiation with 16-entry term tables; the rest in the 64-entry one.
        const uint32_t n_narrow = b->n_class[0], n_wide = b->n_witems - b->n_class[0];
        const DevWItem* wide = b->d_witems + n_narrow;
        if (b->K <= 32) {   // the buffer is shrunk to K when it holds more than CB - 64 entries: CB = 128 needs K well below 64
            if (n_narrow) launch_uscore<128, 16>(and_mode, b->imp, b->pk, n_narrow, st, b->d_witems, b->d_terms, b->d_segs, sh, sn, sf, b->K);
            if (n_wide) launch_uscore<128, 64>(and_mode, b->imp, b->pk, n_wide, st, wide, b->d_terms, b->d_segs, sh, sn, sf, b->K);
        } else {
            if (n_narrow) launch_uscore<256, 16>(and_mode, b->imp, b->pk, n_narrow, st, b->d_witems, b->d_terms, b->d_segs, sh, sn, sf, b->K);
            if (n_wide) launch_uscore<256, 64>(and_mode, b->imp, b->pk, n_wide, st, wide, b->d_terms, b->d_segs, sh, sn, sf, b->K);
        }
    }
#ifdef NS_VARIANTS
    else if (b->n_witems) {
        const VariantDesc wv = kVariants[b->variant];
#define NS_D(HH, FF) launch_dscore<HH, FF>(and_mode, b->n_witems, st, b->d_witems, b->d_terms, b->d_segs, sh, sn, sf, b->K)
        if (wv.d == 1) {
            if (wv.hb == 512) launch_tscore<512>(and_mode, b->n_witems, st, b->d_witems, b->d_terms, b->d_segs, sh, sn, sf, b->K);
            else if (wv.hb == 2048) launch_tscore<2048>(and_mode, b->n_witems, st, b->d_witems, b->d_terms, b->d_segs, sh, sn, sf, b->K);
            else launch_tscore<1024>(and_mode, b->n_witems, st, b->d_witems, b->d_terms, b->d_segs, sh, sn, sf, b->K);
        } else if (wv.d == 0) {
            switch (b->variant) {
                case 13: NS_D(256, 64); break;
                case 14: NS_D(1024, 256); break;
                case 15: NS_D(512, 64); break;
                case 16: NS_D(512, 256); break;
                case 17: NS_D(1024, 128); break;
                default: NS_D(512, 128); break;
            }
        }
#undef NS_D
    }
#endif
    if (rows) {   // shared top rows: the side stream joins in front of the row join of the queries; without it the consumers run here
        if (row_forked) HIPCHK(ctx, hipStreamWaitEvent(st, b->row_join, 0));
        else hipLaunchKernelGGL((k_rscore<512, 128, 16>), dim3(b->n_ritems), dim3(64), 0, st, b->d_ritems, b->n_ritems, b->d_terms, b->d_segs,
                                b->d_row_hits, b->d_row_nhits, sh, sn, sf, b->K, b->d_row_stats);
    }
    if (b->n_items) {   // term groups of more than 64 terms (and, in the variants build, every group of variants 1-4): the workgroup-tile kernel
#ifdef NS_VARIANTS
        const VariantDesc vd = kVariants[b->variant];
        if (vd.nt == 1024) launch_score<1024, 12, 4>(and_mode, b->n_items, st, b->d_items, b->d_terms, b->d_segs, b->d_bounds, sh, sn, sf, b->K);
        else if (vd.nt == 256) launch_score<256, 16, 4>(and_mode, b->n_items, st, b->d_items, b->d_terms, b->d_segs, b->d_bounds, sh, sn, sf, b->K);
        else if (vd.spt == 16) launch_score<512, 16, 8>(and_mode, b->n_items, st, b->d_items, b->d_terms, b->d_segs, b->d_bounds, sh, sn, sf, b->K);
        else
#endif
        launch_score<512, 12, 4>(and_mode, b->n_items, st, b->d_items, b->d_terms, b->d_segs, b->d_bounds, sh, sn, sf, b->K);
    }
    if (timed) HIPCHK(ctx, hipEventRecord(ev[2], st));
    if (!b->direct && b->Q > b->n_wide_q)
        hipLaunchKernelGGL(k_merge, dim3((b->Q + 3) / 4), dim3(256), 0, st, b->d_queries, b->Q, b->d_part_hits, b->d_part_nhits,
                           b->d_part_found, b->o_hits, b->o_nhits, b->o_found, b->K, b->d_heads);
    if (!b->direct && b->n_wide_q)
        hipLaunchKernelGGL(k_merge_wide, dim3(b->n_wide_q), dim3(256), 0, st, b->d_queries, b->d_wide_q, b->d_part_hits, b->d_part_nhits,
                           b->d_part_found, b->o_hits, b->o_nhits, b->o_found, b->K, b->d_heads);
    if (timed) HIPCHK(ctx, hipEventRecord(ev[3], st));
    HIPCHK(ctx, hipGetLastError());
    b->ran = true;
    if (run_flags & NS_RUN_FETCH) {
        if (b->Q && ctx->down_owner != b) {   // (a small batch that owns h_down already has its results in host memory)
            if (b->down_slot < 0) {
                int slot = -1;
                for (size_t i = 0; i < ctx->down_slots.size(); i++)
                    if (!ctx->down_slots[i].busy && ctx->down_slots[i].cap >= b->out_span) { slot = (int)i; break; }
                if (slot < 0) {
                    for (size_t i = 0; i < ctx->down_slots.size() && slot < 0; i++)
                        if (!ctx->down_slots[i].busy) {   // grow an idle slot
                            if (ctx->down_slots[i].p) (void)hipHostFree(ctx->down_slots[i].p);
                            ctx->down_slots[i] = ns_ctx::DownSlot{};
                            slot = (int)i;
                        }
                    if (slot < 0) {
                        if (ctx->down_slots.size() >= 8) return fail(ctx, NS_E_STATE, "NS_RUN_FETCH: more than 8 batches between run and fetch");
                        ctx->down_slots.emplace_back();
                        slot = (int)ctx->down_slots.size() - 1;
                    }
                    const size_t cap = std::max<size_t>(b->out_span + b->out_span / 4, 1 << 16);
                    if (hipHostMalloc(&ctx->down_slots[(size_t)slot].p, cap, hipHostMallocDefault) != hipSuccess) {
                        ctx->down_slots[(size_t)slot].p = nullptr;
                        (void)hipGetLastError();
                        return fail(ctx, NS_E_NOMEM, "NS_RUN_FETCH: pinned result buffer of %zu bytes", cap);
                    }
                    ctx->down_slots[(size_t)slot].cap = cap;
                }
                ctx->down_slots[(size_t)slot].busy = true;
                b->down_slot = slot;
            }
            HIPCHK(ctx, hipMemcpyAsync(ctx->down_slots[(size_t)b->down_slot].p, b->d_hits, b->out_span, hipMemcpyDeviceToHost, st));
        }
    }
    // completion event of THIS run: destroy (and a NS_RUN_FETCH fetch) wait for it instead of for the whole stream
    if (!b->done) HIPCHK(ctx, hipEventCreateWithFlags(&b->done, hipEventDisableTiming));
    HIPCHK(ctx, hipEventRecord(b->done, st));
    b->done_recorded = true;
    b->fetch_enqueued = (run_flags & NS_RUN_FETCH) != 0;
    return NS_OK;
}

extern "C" void* ns_batch_stream(ns_batch* b) { return b ? (void*)b->st : nullptr; }

// Diagnostic: device time between the END of `prev`'s last timed run (after its last kernel) and the START of `next`'s
// (before its first kernel) — the idle or overlapped time between two batches of a pipelined loop.  Both must have been
// run with NS_RUN_TIMED and must still exist; NS_E_STATE while `next` has not started yet.
extern "C" int ns_batch_gap_ms(ns_batch* prev, ns_batch* next, float* ms) {
    if (!prev || !next || !ms) return NS_E_INVAL;
    if (prev->ev_pool.size() < 4 || next->ev_pool.size() < 4) return fail(next->ctx, NS_E_STATE, "ns_batch_gap_ms: both batches need a timed run");
    const hipError_t e = hipEventElapsedTime(ms, prev->ev_pool[3], next->ev_pool[0]);
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return NS_E_STATE; }
    if (e != hipSuccess) return fail(next->ctx, NS_E_HIP, "ns_batch_gap_ms: %s", hipGetErrorString(e));
    return NS_OK;
}


// reads the HIP-event timings of the runs since the last call (all of them lie before the point the caller has waited for)
static int batch_collect_timings(ns_batch* b) {
    ns_ctx* ctx = b->ctx;
    for (size_t i = 0; i + 4 <= b->ev_pending; i += 4) {
        HIPCHK(ctx, hipEventElapsedTime(&b->last_score_ms, b->ev_pool[i + 1], b->ev_pool[i + 2]));
        HIPCHK(ctx, hipEventElapsedTime(&b->last_total_ms, b->ev_pool[i], b->ev_pool[i + 3]));
        b->sum_score_ms += b->last_score_ms;
        b->sum_total_ms += b->last_total_ms;
        b->timed_runs++;
    }
    b->ev_pending = 0;
    return NS_OK;
}

extern "C" int ns_batch_sync(ns_batch* b) {
    if (!b) return NS_E_INVAL;
    ns_ctx* ctx = b->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(b->st));
    return batch_collect_timings(b);
}

extern "C" int ns_batch_fetch(ns_batch* b, ns_hit* hits_out, uint32_t* nhits_out, uint64_t* found_out) {
    if (!b) return NS_E_INVAL;
    ns_ctx* ctx = b->ctx;
    if (!b->ran) return fail(ctx, NS_E_STATE, "ns_batch_fetch before ns_batch_run");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = b->st;
    const bool own_outputs = b->o_hits == b->d_hits && b->o_nhits == b->d_nhits && b->o_found == b->d_found;
    if (b->fetch_enqueued && b->done_recorded && own_outputs) {   // NS_RUN_FETCH: wait for this batch alone; its results are in (or on their way to) pinned host memory
        HIPCHK(ctx, hipEventSynchronize(b->done));
        int rc = batch_collect_timings(b);
        if (rc != NS_OK) return rc;
        if (b->Q) {
            const char* h = (ctx->down_owner == b) ? (const char*)ctx->h_down : (const char*)ctx->down_slots[(size_t)b->down_slot].p;
            if (hits_out) std::memcpy(hits_out, h, (size_t)b->Q * b->K * sizeof(Hit));
            if (nhits_out) std::memcpy(nhits_out, h + b->off_nhits, (size_t)b->Q * 4);
            if (found_out) std::memcpy(found_out, h + b->off_found, (size_t)b->Q * 8);
        }
        // the pinned slot goes back to the ctx with the fetch (not only at destroy): a serving loop that fetches promptly may
        // keep any number of batches alive.  A second fetch of this run takes the ordinary path (the device buffers still
        // hold the results); the next NS_RUN_FETCH run acquires a slot again.
        if (b->down_slot >= 0) { ctx->down_slots[(size_t)b->down_slot].busy = false; b->down_slot = -1; }
        b->fetch_enqueued = false;
        return NS_OK;
    }
    if (b->Q && own_outputs && ctx->down_owner == b) {   // the results are already in host memory
        int rc = ns_batch_sync(b);
        if (rc != NS_OK) return rc;
        const char* h = (const char*)ctx->h_down;
        if (hits_out) std::memcpy(hits_out, h, (size_t)b->Q * b->K * sizeof(Hit));
        if (nhits_out) std::memcpy(nhits_out, h + b->off_nhits, (size_t)b->Q * 4);
        if (found_out) std::memcpy(found_out, h + b->off_found, (size_t)b->Q * 8);
        return NS_OK;
    }
    if (b->Q && own_outputs && !ctx->down_owner && b->out_span <= kStageMaxBytes) {
        if (ctx->h_down_cap < b->out_span) {
            if (ctx->h_down) (void)hipHostFree(ctx->h_down);
            ctx->h_down = nullptr; ctx->h_down_cap = 0;
            const size_t cap = std::max<size_t>(b->out_span + b->out_span / 2, 1 << 16);
            if (hipHostMalloc(&ctx->h_down, cap, hipHostMallocDefault) == hipSuccess) ctx->h_down_cap = cap;
            else { ctx->h_down = nullptr; (void)hipGetLastError(); }
        }
        if (ctx->h_down_cap >= b->out_span) {
            HIPCHK(ctx, hipMemcpyAsync(ctx->h_down, b->d_hits, b->out_span, hipMemcpyDeviceToHost, st));
            int rc = ns_batch_sync(b);
            if (rc != NS_OK) return rc;
            const char* h = (const char*)ctx->h_down;
            if (hits_out) std::memcpy(hits_out, h, (size_t)b->Q * b->K * sizeof(Hit));
            if (nhits_out) std::memcpy(nhits_out, h + b->off_nhits, (size_t)b->Q * 4);
            if (found_out) std::memcpy(found_out, h + b->off_found, (size_t)b->Q * 8);
            return NS_OK;
        }
    }
    if (b->Q) {
        if (hits_out) HIPCHK(ctx, hipMemcpyAsync(hits_out, b->o_hits, (size_t)b->Q * b->K * sizeof(Hit), hipMemcpyDeviceToHost, st));
        if (nhits_out) HIPCHK(ctx, hipMemcpyAsync(nhits_out, b->o_nhits, (size_t)b->Q * 4, hipMemcpyDeviceToHost, st));
        if (found_out) HIPCHK(ctx, hipMemcpyAsync(found_out, b->o_found, (size_t)b->Q * 8, hipMemcpyDeviceToHost, st));
    }
    return ns_batch_sync(b);
}

extern "C" int ns_batch_get_info(ns_batch* b, ns_batch_info* info) {
    if (!b || !info) return NS_E_INVAL;
    info->postings = b->postings;
    info->algo_bytes = b->postings * 8;
    info->n_queries = b->Q;
    info->n_items = b->n_items + b->n_witems + b->n_ritems + b->n_pitems;
    info->n_term_refs = b->n_terms;
    info->tile_docs = b->tile_docs;
    info->k = b->K;
    info->flags = b->flags | (b->imp ? NS_INFO_IMPACTS : 0u) | (b->pk ? NS_INFO_PACKED : 0u) | (b->pruned ? NS_INFO_PRUNED : 0u) |
                  (b->shared ? NS_INFO_SHARED : 0u);
    info->shared_lists = b->n_share;
    info->shared_postings = b->share_postings;
    info->last_score_kernel_ms = b->last_score_ms;
    info->last_total_ms = b->last_total_ms;
    info->timed_runs = b->timed_runs;
    info->sum_score_kernel_ms = b->sum_score_ms;
    info->sum_total_ms = b->sum_total_ms;
    return NS_OK;
}

// shared top rows of the batch: producer items, consumer items, and over its runs so far (waited for here) the consumer
// items that fell back to the streaming body and the row entries that hit a table
extern "C" int ns_batch_row_stats(ns_batch* b, uint32_t out[4]) {
    if (!b || !out) return NS_E_INVAL;
    ns_ctx* ctx = b->ctx;
    const bool rows = b->n_pitems && b->n_ritems && b->variant == 0;
    out[0] = rows ? b->n_pitems : 0u; out[1] = rows ? b->n_ritems : 0u; out[2] = 0u; out[3] = 0u;
    if (rows && b->ran) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, hipMemcpyAsync(out + 2, b->d_row_stats, 8, hipMemcpyDeviceToHost, b->st));
        HIPCHK(ctx, hipStreamSynchronize(b->st));
    }
    return NS_OK;
}

// the batch's (query, segment) groups by scoring body after the class rule, and those the class model promoted
extern "C" int ns_batch_class_stats(ns_batch* b, uint32_t out[4]) {
    if (!b || !out) return NS_E_INVAL;
    std::memcpy(out, b->class_stats, sizeof(b->class_stats));
    return NS_OK;
}

extern "C" int ns_search_batch(ns_ctx* ctx, const ns_query_desc* queries, const ns_term_ref* terms, uint32_t n_queries,
                               uint32_t k, ns_hit* hits_out, uint32_t* nhits_out, uint64_t* found_out, uint32_t flags) {
    ns_batch* b = nullptr;
    int rc = ns_batch_prepare(ctx, queries, terms, n_queries, k, flags, &b);
    if (rc != NS_OK) return rc;
    rc = ns_batch_run(b, 0);
    if (rc == NS_OK) rc = ns_batch_fetch(b, hits_out, nhits_out, found_out);
    ns_batch_destroy(b);
    return rc;
}


// ------------------------------------------------------------------------------------------------
// The scan and the radix sort that the index-building calls share (csrc/ns_invert.hip)
// exclusive scan of a[0 .. m) in place; the sum of all goes to *d_total (device, may be NULL); d_sums: ceil(m / 1024) words
static void ig_scan(hipStream_t st, uint32_t* d_a, uint32_t m, uint32_t* d_sums, uint32_t* d_total) {
    const uint32_t blocks = (m + 1023) / 1024;
    hipLaunchKernelGGL(k_iv_scan_sums, dim3(blocks), dim3(256), 0, st, d_a, m, d_sums);
    hipLaunchKernelGGL(k_iv_scan_top, dim3(1), dim3(1024), 0, st, d_sums, blocks, d_total);
    hipLaunchKernelGGL(k_iv_scan_apply, dim3(blocks), dim3(256), 0, st, d_a, m, d_sums);
}

// What the inversion's first pass reads instead of buffer *cur: the pairs, the documents' pair prefix and each tile's first and
// last document.  d_kept receives the number of items that survive the first pass; the later passes read their n from it.
// All NULL: a sort of buffer *cur (ig_sort).
struct IvFirst {
    const uint2* d_pairs = nullptr;
    const uint64_t* d_prefix = nullptr;
    const uint2* d_tile_docs = nullptr;
    uint32_t* d_kept = nullptr;
};
using IvHistKernel = void (*)(const uint32_t*, const uint2*, uint32_t, const uint32_t*, uint32_t, uint32_t, uint32_t*, uint32_t);
using IvPassKernel = void (*)(const uint2*, const uint64_t*, const uint2*, uint32_t, const uint32_t*, const uint2*, uint32_t*, uint2*, uint32_t, const uint32_t*,
                              uint32_t, const uint32_t*, uint32_t);

// The stable LSD radix sort of ns_invert.hip over the keys below key_range, digit plan from key_range alone
// (ns_radix_plan.hpp): per pass a histogram, its scan and the scatter from buffer *cur into the other one; the result is
// buffer *cur afterwards.  With from.d_pairs the first pass reads the pairs and writes buffer 0 (*cur need not be set).
// last_is_final: the last pass is the LAST instantiation of k_iv_pass.  d_hist: 2048 * ceil(n / kIvTile) words at most
static void iv_sort(hipStream_t st, uint32_t n, uint32_t key_range, uint32_t* d_keys[2], uint2* d_vals[2], int* cur, uint32_t* d_hist, uint32_t* d_sums,
                    const IvFirst& from, bool last_is_final) {
    static const IvHistKernel kHist[4] = {k_iv_hist_w<8>, k_iv_hist_w<9>, k_iv_hist_w<10>, k_iv_hist_w<11>};   // [digit width - 8]
    static const IvPassKernel kPass[4][2][2] = {   // [digit width - 8][first][last]
        {{k_iv_pass<8, false, false>, k_iv_pass<8, false, true>}, {k_iv_pass<8, true, false>, k_iv_pass<8, true, true>}},
        {{k_iv_pass<9, false, false>, k_iv_pass<9, false, true>}, {k_iv_pass<9, true, false>, k_iv_pass<9, true, true>}},
        {{k_iv_pass<10, false, false>, k_iv_pass<10, false, true>}, {k_iv_pass<10, true, false>, k_iv_pass<10, true, true>}},
        {{k_iv_pass<11, false, false>, k_iv_pass<11, false, true>}, {k_iv_pass<11, true, false>, k_iv_pass<11, true, true>}}};
    const uint32_t n_tiles = (n + kIvTile - 1) / kIvTile;
    const RadixPlan rp = radix_plan(key_range);
    uint32_t shift = 0;
    for (int p = 0; p < rp.passes; p++) {
        const bool first = from.d_pairs && p == 0, last = last_is_final && p == rp.passes - 1;
        const int w = rp.pbits[p] - 8;                                 // 8 .. 11 bits: 0 .. 3
        const int nxt = first ? 0 : (*cur ^ 1);
        const uint32_t m = ((uint32_t)1 << rp.pbits[p]) * n_tiles;     // < 2^31: fewer than 2^20 tiles of at most 2^11 bins
        const uint32_t* kin = first ? nullptr : d_keys[*cur];
        const uint2* vin = first ? nullptr : d_vals[*cur];
        const uint32_t* n_dev = first ? nullptr : from.d_kept;
        hipLaunchKernelGGL(kHist[w], dim3(n_tiles), dim3(256), 0, st, kin, first ? from.d_pairs : (const uint2*)nullptr, n, n_dev, key_range, shift, d_hist, n_tiles);
        ig_scan(st, d_hist, m, d_sums, first ? from.d_kept : (uint32_t*)nullptr);
        hipLaunchKernelGGL(kPass[w][first][last], dim3(n_tiles), dim3(256), 0, st, from.d_pairs, from.d_prefix, from.d_tile_docs, key_range, kin, vin, d_keys[nxt],
                           d_vals[nxt], n, n_dev, shift, (const uint32_t*)d_hist, n_tiles);
        shift += (uint32_t)rp.pbits[p];
        *cur = nxt;
    }
}

// the sort of n (key, value) items in buffer *cur, for text ingest and compaction: every pass is k_iv_pass<B, false, false>
static void ig_sort(hipStream_t st, uint32_t n, uint32_t key_range, uint32_t* d_keys[2], uint2* d_vals[2], int* cur, uint32_t* d_hist, uint32_t* d_sums) {
    iv_sort(st, n, key_range, d_keys, d_vals, cur, d_hist, d_sums, IvFirst{}, false);
}

// ------------------------------------------------------------------------------------------------
// f3: forward.bin -> inverted lists (csrc/ns_invert.hip)
// `adopt` != nullptr: the inverted lists also become the posting stream of that segment (an upload in progress whose announced
// payload is n_pairs postings) by a device-to-device copy; postings_out may then be NULL.
// `dev_pairs` != nullptr: the pairs are on the device already (ns_forward_invert); `pairs` is not read and nothing is uploaded for them.
static int invert_run(ns_ctx* ctx, const uint32_t* doc_term_counts, uint32_t n_docs, const uint32_t* pairs,
                      uint64_t n_pairs, uint32_t n_terms, uint32_t* df_out, void* postings_out, uint64_t* kept_out,
                      float* device_ms_out, ns_seg* adopt, const uint2* dev_pairs = nullptr) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_invert_forward: ctx is NULL");
    if ((n_docs && !doc_term_counts) || (n_pairs && !pairs && !dev_pairs) || (n_terms && !df_out) || !kept_out) return fail(ctx, NS_E_INVAL, "ns_invert_forward: null argument");
    if (n_pairs >= (1ull << 32) - kIvTile) return fail(ctx, NS_E_INVAL, "ns_invert_forward: %llu pairs; this build indexes pairs with 32 bits (split the segment)", (unsigned long long)n_pairs);
    if (n_terms == 0xFFFFFFFFu) return fail(ctx, NS_E_INVAL, "ns_invert_forward: n_terms too large");
    *kept_out = 0;
    if (device_ms_out) *device_ms_out = 0.0f;
    InvertPlan plan;
    std::string why;
    if (!invert_plan(doc_term_counts, n_docs, n_pairs, n_terms, plan, why)) return fail(ctx, NS_E_INVAL, "ns_invert_forward: %s", why.c_str());
    if (n_terms) std::memset(df_out, 0, (size_t)n_terms * 4);
    if (!n_pairs) return NS_OK;
    if (!postings_out && !adopt) return fail(ctx, NS_E_INVAL, "ns_invert_forward: postings_out is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)n_pairs, n_tiles = plan.n_tiles;
    // Digit plan, from n_terms alone (no device -> host sync decides it): the keys are the termIds below n_terms — a pair with
    // any other termId is dropped by the reference (src/lexicon.cpp:69-70) and leaves the sort in the first pass — so
    // the width of n_terms - 1 is sorted in ceil(bits / 11) passes of 8 .. 11 bits, as even as possible (ns_radix_plan.hpp).
    const int passes = plan.rp.passes;

    // one block from the ctx pool for all scratch arrays (a build loop inverts segment after segment of similar size;
    // ten hipMalloc + hipFree per call cost more than the device work)
    CallBlock blk(ctx);
    const size_t nt1 = (size_t)std::max<uint32_t>(n_terms, 1);
    const size_t o_pairs = blk.reserve(dev_pairs ? 1 : (size_t)n * 8), o_v0 = blk.reserve((size_t)n * 8), o_v1 = blk.reserve(passes > 1 ? (size_t)n * 8 : 1);
    const size_t o_k0 = blk.reserve((size_t)n * 4), o_k1 = blk.reserve(passes > 1 ? (size_t)n * 4 : 1);
    const size_t o_df = blk.reserve(nt1 * 4), o_first = blk.reserve(nt1 * 4), o_hist = blk.reserve(plan.m_max * 4), o_sums = blk.reserve((size_t)plan.scan_blocks_max * 4),
                 o_kept = blk.reserve(4), o_prefix = blk.reserve(plan.prefix.size() * 8), o_tdocs = blk.reserve((size_t)n_tiles * 8);
    blk.alloc(2);
    if (blk.ok()) {
        uint2* d_pairs = dev_pairs ? const_cast<uint2*>(dev_pairs) : blk.at<uint2>(o_pairs);
        uint2* d_vals[2] = {blk.at<uint2>(o_v0), blk.at<uint2>(o_v1)};
        uint32_t* d_keys[2] = {blk.at<uint32_t>(o_k0), blk.at<uint32_t>(o_k1)};
        uint32_t *d_df = blk.at<uint32_t>(o_df), *d_first = blk.at<uint32_t>(o_first), *d_hist = blk.at<uint32_t>(o_hist), *d_sums = blk.at<uint32_t>(o_sums),
                 *d_kept = blk.at<uint32_t>(o_kept);
        if (!dev_pairs) blk.upload(o_pairs, pairs, (size_t)n * 8);
        blk.upload(o_prefix, plan.prefix.data(), plan.prefix.size() * 8);
        blk.upload(o_tdocs, plan.tile_docs.data(), plan.tile_docs.size() * 4);
        blk.zero(o_df, nt1 * 4);
        blk.chk(hipMemsetAsync(d_first, 0xFF, nt1 * 4, st));
        blk.record(0);
        // The first pass reads the pairs and writes buffer 0.  The number of items that survive it (the kept pairs) stays on
        // the device: the first scan leaves it in d_kept, later kernels read it.
        int cur = -1;
        const IvFirst from_pairs{d_pairs, blk.at<uint64_t>(o_prefix), blk.at<uint2>(o_tdocs), d_kept};
        iv_sort(st, n, n_terms, d_keys, d_vals, &cur, d_hist, d_sums, from_pairs, true);
        const uint2* d_final = d_vals[cur];
        // df from the sorted keys: a run's first pair records where it starts, its last pair where it ends (d_df holds the ends)
        if (n_terms) hipLaunchKernelGGL(k_iv_runs, dim3((n + 1023) / 1024), dim3(256), 0, st, d_keys[cur], n, n_terms, d_first, d_df, d_kept);
        blk.record(1);
        blk.launched();
        std::vector<uint32_t> h_first(n_terms);
        if (n_terms) blk.fetch(df_out, o_df, (size_t)n_terms * 4);
        if (n_terms) blk.fetch(h_first.data(), o_first, (size_t)n_terms * 4);
        blk.sync();
        if (blk.ok()) {
            uint64_t kept = 0;
            for (uint32_t t = 0; t < n_terms; t++) df_out[t] = (h_first[t] == 0xFFFFFFFFu) ? 0u : df_out[t] - h_first[t] + 1u;
            for (uint32_t t = 0; t < n_terms; t++) kept += df_out[t];
            *kept_out = kept;   // the dropped pairs left the sort in the first pass
            if (kept && postings_out) blk.chk(hipMemcpy(postings_out, d_final, (size_t)kept * 8, hipMemcpyDeviceToHost));
            if (adopt) {   // the lists stay on the device: they ARE the segment's posting stream
                if (kept) blk.chk(hipMemcpyAsync(adopt->d_postings, d_final, (size_t)kept * 8, hipMemcpyDeviceToDevice, st));
                if (kept != adopt->n_postings) {   // dropped pairs: the stream is shorter than announced; move the padding
                    blk.chk(hipMemsetAsync((char*)adopt->d_postings + kept * 8, 0xFF, kPadPostings * 8, st));
                    blk.chk(hipMemsetAsync((char*)adopt->d_pnorm + kept * 4, 0, kPadPostings * 4, st));
                }
                blk.sync();
                if (blk.ok()) { adopt->n_postings = kept; adopt->filled = kept * 8; }
            }
            float ms = 0.0f;
            if (blk.elapsed_ms(0, 1, &ms) && device_ms_out) *device_ms_out = ms;
        }
    }
    return blk.finish("ns_invert_forward");
}

extern "C" int ns_invert_forward(ns_ctx* ctx, const uint32_t* doc_term_counts, uint32_t n_docs, const uint32_t* pairs,
                                 uint64_t n_pairs, uint32_t n_terms, uint32_t* df_out, void* postings_out, uint64_t* kept_out,
                                 float* device_ms_out) {
    return invert_run(ctx, doc_term_counts, n_docs, pairs, n_pairs, n_terms, df_out, postings_out, kept_out, device_ms_out, nullptr);
}

extern "C" int ns_segment_upload_inverted(ns_ctx* ctx, ns_seg* seg, const uint32_t* doc_term_counts, const uint32_t* pairs,
                                          uint64_t n_pairs, uint32_t n_terms, uint32_t* df_out, void* postings_out,
                                          uint64_t* kept_out, float* device_ms_out) {
    if (!ctx || !seg || seg->ctx != ctx || !seg->pending) return fail(ctx, NS_E_STATE, "ns_segment_upload_inverted: no upload in progress for this segment");
    if (seg->filled != 0) return fail(ctx, NS_E_STATE, "ns_segment_upload_inverted: the segment already received %llu payload bytes", (unsigned long long)seg->filled);
    if (seg->n_postings != n_pairs) return fail(ctx, NS_E_INVAL, "ns_segment_upload_inverted: %llu pairs, but ns_segment_upload_begin announced %llu postings", (unsigned long long)n_pairs, (unsigned long long)seg->n_postings);
    return invert_run(ctx, doc_term_counts, seg->n_docs, pairs, n_pairs, n_terms, df_out, postings_out, kept_out, device_ms_out, seg);
}

// ------------------------------------------------------------------------------------------------
// Indexing: document texts -> forward index (csrc/ns_ingest.hip)
struct ns_forward {
    ns_ctx* ctx = nullptr;          // nullptr: orphaned by ns_ctx_destroy (the device arrays below are gone)
    ns_forward_info info{};
    uint32_t* d_map = nullptr;      // kept_docs
    uint32_t* d_len = nullptr;      // kept_docs
    uint32_t* d_cnt = nullptr;      // kept_docs
    uint2* d_pairs = nullptr;       // n_pairs {termId, tf}
    uint8_t* d_terms = nullptr;     // term_bytes
    uint32_t* d_toff = nullptr;     // n_terms + 1
};

static void forward_free_device(ns_forward* f) {
    (void)hipFree(f->d_map); (void)hipFree(f->d_len); (void)hipFree(f->d_cnt);
    (void)hipFree(f->d_pairs); (void)hipFree(f->d_terms); (void)hipFree(f->d_toff);
    f->d_map = f->d_len = f->d_cnt = f->d_toff = nullptr; f->d_pairs = nullptr; f->d_terms = nullptr;
}
static void forward_orphan_fwd(ns_forward* f) { forward_free_device(f); f->ctx = nullptr; }

// ------------------------------------------------------------------------------------------------
// Filtered copy of a segment (csrc/ns_filter.hip)
extern "C" int ns_segment_filter(ns_ctx* ctx, ns_seg* src, uint32_t new_seg_id, const uint32_t* keep_bits, const uint64_t* byte_off,
                                 const uint32_t* counts, uint32_t n_lists, uint64_t* new_byte_off_out, uint32_t* new_counts_out,
                                 void* postings_out, uint64_t* kept_postings_out, float* device_ms_out, ns_seg** out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_segment_filter: ctx is NULL");
    if (!out) return fail(ctx, NS_E_INVAL, "ns_segment_filter: out is NULL");
    *out = nullptr;
    if (!src) return fail(ctx, NS_E_INVAL, "ns_segment_filter: src is NULL");
    if (src->ctx != ctx) return fail(ctx, NS_E_INVAL, "ns_segment_filter: the source does not belong to this ctx");
    if (src->pending) return fail(ctx, NS_E_INVAL, "ns_segment_filter: the source's upload has not ended");
    if (src->id >= ctx->segs.size() || ctx->segs[src->id] != src) return fail(ctx, NS_E_INVAL, "ns_segment_filter: the source does not belong to this ctx");
    if (src->n_docs && !keep_bits) return fail(ctx, NS_E_INVAL, "ns_segment_filter: keep_bits is NULL");
    if (n_lists && (!byte_off || !counts || !new_byte_off_out || !new_counts_out)) return fail(ctx, NS_E_INVAL, "ns_segment_filter: null list arrays");
    if (new_seg_id >= (1u << 20)) return fail(ctx, NS_E_INVAL, "seg_id %u too large", new_seg_id);
    if (new_seg_id < ctx->segs.size() && ctx->segs[new_seg_id]) return fail(ctx, NS_E_INVAL, "segment %u already uploaded", new_seg_id);
    for (const ns_seg* p : ctx->pending_uploads)
        if (p->id == new_seg_id) return fail(ctx, NS_E_INVAL, "segment %u is being uploaded", new_seg_id);
    if (src->n_postings >= (1ull << 32) - 2 * kFlChunk) return fail(ctx, NS_E_INVAL, "ns_segment_filter: the source has too many postings");
    if (int rc = check_lists(ctx, src, byte_off, counts, n_lists)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));

    const uint32_t n = (uint32_t)src->n_postings, n_docs = src->n_docs;
    const uint32_t n_chunks = (n + kFlChunk - 1) / kFlChunk, m = n_chunks + 1;
    const uint32_t n_words = (n_docs + 31) / 32;
    hipStream_t st = ctx->stream;
    // the scratch of the call in one block from the ctx pool; the new segment's own arrays are hipMallocs, like a forward handle's
    CallBlock blk(ctx);
    const size_t o_bits = blk.reserve((size_t)std::max<uint32_t>(n_words, 1) * 4), o_mask = blk.reserve((size_t)m * 8), o_base = blk.reserve((size_t)m * 4),
                 o_sums = blk.reserve((size_t)((m + 1023) / 1024) * 4), o_total = blk.reserve(4);
    const size_t o_starts = blk.reserve((size_t)n_lists * 4), o_counts = blk.reserve((size_t)n_lists * 4), o_ncnt = blk.reserve((size_t)n_lists * 4),
                 o_noff = blk.reserve((size_t)n_lists * 8);
    blk.alloc(4);
    ns_seg* s = new ns_seg();
    s->ctx = ctx;
    s->id = new_seg_id;
    s->n_docs = n_docs;
    s->avgdl = src->avgdl;
    s->norm_safe = src->norm_safe;
    uint32_t kept = 0;
    if (blk.ok()) {
        uint32_t *d_bits = blk.at<uint32_t>(o_bits), *d_base = blk.at<uint32_t>(o_base), *d_sums = blk.at<uint32_t>(o_sums), *d_total = blk.at<uint32_t>(o_total);
        uint32_t *d_starts = blk.at<uint32_t>(o_starts), *d_counts = blk.at<uint32_t>(o_counts), *d_ncnt = blk.at<uint32_t>(o_ncnt);
        uint64_t *d_mask = blk.at<uint64_t>(o_mask), *d_noff = blk.at<uint64_t>(o_noff);
        std::vector<uint32_t> starts(n_lists);
        for (uint32_t i = 0; i < n_lists; i++) starts[i] = (uint32_t)(byte_off[i] / 8);
        blk.upload(o_bits, keep_bits, (size_t)n_words * 4);
        blk.upload(o_starts, starts.data(), (size_t)n_lists * 4);
        blk.upload(o_counts, counts, (size_t)n_lists * 4);

        // mark + scan, then the one number the host needs before it can size the copy
        const uint32_t grid = std::min<uint32_t>((m + 3) / 4, 1u << 16);
        blk.record(0);
        hipLaunchKernelGGL(k_fl_mark, dim3(grid), dim3(256), 0, st, src->d_postings, n, d_bits, n_docs, d_mask, d_base);
        ig_scan(st, d_base, m, d_sums, d_total);
        blk.record(1);
        blk.launched();
        if (blk.ok()) blk.fetch(&kept, o_total, 4);
        if (blk.ok()) blk.sync();
        if (blk.ok() && kept > n) blk.chk(hipErrorUnknown);

        if (blk.ok()) {
            s->n_postings = kept;
            blk.chk(hipMalloc((void**)&s->d_postings, ((size_t)kept + kPadPostings) * 8));
            blk.chk(hipMalloc((void**)&s->d_pnorm, ((size_t)kept + kPadPostings) * 4));
            blk.chk(hipMalloc((void**)&s->d_norm, (size_t)std::max<uint32_t>(n_docs, 1) * 4));
        }
        if (blk.ok()) {
            blk.chk(hipMemsetAsync(s->d_postings + kept, 0xFF, kPadPostings * 8, st));   // docId ~0: never taken
            blk.chk(hipMemsetAsync(s->d_pnorm + kept, 0, kPadPostings * 4, st));
            if (n_docs) blk.chk(hipMemcpyAsync(s->d_norm, src->d_norm, (size_t)n_docs * 4, hipMemcpyDeviceToDevice, st));
        }
        if (blk.ok()) {
            blk.record(2);
            if (n_chunks) hipLaunchKernelGGL(k_fl_scatter, dim3(std::min<uint32_t>((n_chunks + 3) / 4, 1u << 16)), dim3(256), 0, st, src->d_postings, src->d_pnorm, n, d_mask, d_base, s->d_postings, s->d_pnorm);
            if (n_lists) hipLaunchKernelGGL(k_fl_lists, dim3((n_lists + 255) / 256), dim3(256), 0, st, d_starts, d_counts, n_lists, d_mask, d_base, d_noff, d_ncnt);
            blk.record(3);
            blk.launched();
        }
        if (blk.ok() && n_lists) {
            blk.fetch(new_byte_off_out, o_noff, (size_t)n_lists * 8);
            blk.fetch(new_counts_out, o_ncnt, (size_t)n_lists * 4);
        }
        if (blk.ok() && postings_out && kept) blk.chk(hipMemcpyAsync(postings_out, s->d_postings, (size_t)kept * 8, hipMemcpyDeviceToHost, st));
        if (blk.ok()) blk.sync();
        float a = 0.0f, b = 0.0f;
        if (blk.elapsed_ms(0, 1, &a) && blk.elapsed_ms(2, 3, &b) && device_ms_out) *device_ms_out = a + b;
    }
    const int rc = blk.finish("ns_segment_filter");
    if (rc != NS_OK) {
        seg_free_device(s);
        delete s;
        return rc;
    }
    if (kept_postings_out) *kept_postings_out = kept;
    if (ctx->segs.size() <= new_seg_id) ctx->segs.resize(new_seg_id + 1, nullptr);
    ctx->segs[new_seg_id] = s;
    *out = s;
    return NS_OK;
}

// ------------------------------------------------------------------------------------------------
// A derived segment of copied lists and union lists (csrc/ns_union.hip, csrc/ns_union_plan.hpp)
extern "C" int ns_ctx_union_scratch(ns_ctx* ctx, uint64_t bytes) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_ctx_union_scratch: ctx is NULL");
    if (bytes > kUnMaxScratch) return fail(ctx, NS_E_INVAL, "ns_ctx_union_scratch: %llu bytes (at most %llu)", (unsigned long long)bytes, (unsigned long long)kUnMaxScratch);
    ctx->union_scratch = bytes ? bytes : kUnDefaultScratch;
    return NS_OK;
}

extern "C" int ns_segment_union(ns_ctx* ctx, ns_seg* src, uint32_t new_seg_id, const uint64_t* member_off, const uint32_t* member_cnt,
                                const uint32_t* group_begin, uint32_t n_groups, uint64_t* new_byte_off_out, uint32_t* new_counts_out,
                                void* postings_out, uint64_t* n_postings_out, uint32_t* rounds_out, float* device_ms_out, ns_seg** out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_segment_union: ctx is NULL");
    if (!out) return fail(ctx, NS_E_INVAL, "ns_segment_union: out is NULL");
    *out = nullptr;
    if (!src) return fail(ctx, NS_E_INVAL, "ns_segment_union: src is NULL");
    if (src->ctx != ctx) return fail(ctx, NS_E_INVAL, "ns_segment_union: the source does not belong to this ctx");
    if (src->pending) return fail(ctx, NS_E_INVAL, "ns_segment_union: the source's upload has not ended");
    if (src->id >= ctx->segs.size() || ctx->segs[src->id] != src) return fail(ctx, NS_E_INVAL, "ns_segment_union: the source does not belong to this ctx");
    if (!group_begin) return fail(ctx, NS_E_INVAL, "ns_segment_union: group_begin is NULL");
    if (n_groups && (!new_byte_off_out || !new_counts_out)) return fail(ctx, NS_E_INVAL, "ns_segment_union: null list arrays");
    if (postings_out && !n_postings_out) return fail(ctx, NS_E_INVAL, "ns_segment_union: postings_out without n_postings_out");
    if (group_begin[0] != 0) return fail(ctx, NS_E_INVAL, "ns_segment_union: group_begin[0] is %u, not 0", group_begin[0]);
    for (uint32_t g = 0; g < n_groups; g++)
        if (group_begin[g + 1] < group_begin[g]) return fail(ctx, NS_E_INVAL, "ns_segment_union: group_begin decreases at group %u", g);
    const uint32_t n_members = group_begin[n_groups];
    if (n_members && (!member_off || !member_cnt)) return fail(ctx, NS_E_INVAL, "ns_segment_union: null list arrays");
    if (new_seg_id >= (1u << 20)) return fail(ctx, NS_E_INVAL, "seg_id %u too large", new_seg_id);
    if (new_seg_id < ctx->segs.size() && ctx->segs[new_seg_id]) return fail(ctx, NS_E_INVAL, "segment %u already uploaded", new_seg_id);
    for (const ns_seg* p : ctx->pending_uploads)
        if (p->id == new_seg_id) return fail(ctx, NS_E_INVAL, "segment %u is being uploaded", new_seg_id);
    if (src->n_postings >= (1ull << 32) - 2 * kUnChunk) return fail(ctx, NS_E_INVAL, "ns_segment_union: the source has too many postings");
    if (int rc = check_lists(ctx, src, member_off, member_cnt, n_members)) return rc;
    uint64_t named = 0;
    for (uint32_t i = 0; i < n_members; i++) named += member_cnt[i];
    if (named >= (1ull << 32) - 2 * kUnChunk) return fail(ctx, NS_E_INVAL, "ns_segment_union: the members have too many postings");
    HIPCHK(ctx, hipSetDevice(ctx->device));

    const uint32_t n_docs = src->n_docs, cpt = (n_docs + kUnChunk - 1) / kUnChunk;
    std::vector<uint32_t> firsts(n_members);
    for (uint32_t i = 0; i < n_members; i++) firsts[i] = (uint32_t)(member_off[i] / 8);
    const UnionPlan plan = union_plan(firsts.data(), member_cnt, group_begin, n_groups, n_docs, ctx->union_scratch);
    const uint32_t n_rounds = (uint32_t)plan.rounds.size(), n_tabled = (uint32_t)plan.tabled.size();
    const uint32_t R = std::min<uint32_t>(plan.tables_per_round, std::max<uint32_t>(n_tabled, 1));   // tables the call holds
    const uint32_t m = R * cpt + 1;
    const size_t n_copy = plan.copy_items.size(), n_add = plan.add_items.size();
    // what the host knows of the answers: the single groups' places; k_un_lists stores the tabled groups' over the zeros
    std::vector<uint64_t> noff(n_groups, 0);
    std::vector<uint32_t> ncnt(n_groups, 0);
    for (uint32_t g = 0; g < n_groups; g++)
        if (group_begin[g + 1] - group_begin[g] == 1) { noff[g] = (uint64_t)plan.single_off[g] * 8; ncnt[g] = member_cnt[group_begin[g]]; }
    std::vector<uint32_t> run(n_rounds + 1, 0);
    run[0] = (uint32_t)plan.single_postings;

    hipStream_t st = ctx->stream;
    // the scratch of the call in one block from the ctx pool; the new segment's own arrays are hipMallocs, like a filtered copy's
    CallBlock blk(ctx);
    const size_t o_tables = blk.reserve(n_tabled ? (size_t)R * std::max<uint32_t>(n_docs, 1) * 4 : 4), o_mask = blk.reserve((size_t)m * 8),
                 o_base = blk.reserve((size_t)m * 4), o_sums = blk.reserve((size_t)((m + 1023) / 1024) * 4), o_run = blk.reserve((size_t)(n_rounds + 1) * 4);
    const size_t o_copy = blk.reserve(n_copy * sizeof(UnCopyItem)), o_add = blk.reserve(n_add * sizeof(UnAddItem)), o_tabled = blk.reserve((size_t)n_tabled * 4),
                 o_ncnt = blk.reserve((size_t)n_groups * 4), o_noff = blk.reserve((size_t)n_groups * 8);
    blk.alloc(2);
    ns_seg* s = new ns_seg();
    s->ctx = ctx;
    s->id = new_seg_id;
    s->n_docs = n_docs;
    s->avgdl = src->avgdl;
    s->norm_safe = src->norm_safe;
    uint32_t written = 0;
    if (blk.ok()) {
        uint32_t *d_tables = blk.at<uint32_t>(o_tables), *d_base = blk.at<uint32_t>(o_base), *d_sums = blk.at<uint32_t>(o_sums), *d_run = blk.at<uint32_t>(o_run);
        uint32_t *d_tabled = blk.at<uint32_t>(o_tabled), *d_ncnt = blk.at<uint32_t>(o_ncnt);
        uint64_t *d_mask = blk.at<uint64_t>(o_mask), *d_noff = blk.at<uint64_t>(o_noff);
        const UnCopyItem* d_copy = blk.at<UnCopyItem>(o_copy);
        const UnAddItem* d_add = blk.at<UnAddItem>(o_add);
        blk.chk(hipMalloc((void**)&s->d_postings, ((size_t)plan.bound + kPadPostings) * 8));
        blk.chk(hipMalloc((void**)&s->d_pnorm, ((size_t)plan.bound + kPadPostings) * 4));
        blk.chk(hipMalloc((void**)&s->d_norm, (size_t)std::max<uint32_t>(n_docs, 1) * 4));
        if (blk.ok()) {
            blk.upload(o_run, run.data(), (size_t)(n_rounds + 1) * 4);
            blk.upload(o_copy, plan.copy_items.data(), n_copy * sizeof(UnCopyItem));
            blk.upload(o_add, plan.add_items.data(), n_add * sizeof(UnAddItem));
            blk.upload(o_tabled, plan.tabled.data(), (size_t)n_tabled * 4);
            blk.upload(o_ncnt, ncnt.data(), (size_t)n_groups * 4);
            blk.upload(o_noff, noff.data(), (size_t)n_groups * 8);
            if (n_docs) blk.chk(hipMemcpyAsync(s->d_norm, src->d_norm, (size_t)n_docs * 4, hipMemcpyDeviceToDevice, st));
        }
        if (blk.ok()) {
            blk.record(0);
            if (n_copy) hipLaunchKernelGGL(k_un_copy, dim3(std::min<uint32_t>(((uint32_t)n_copy + 3) / 4, 1u << 16)), dim3(256), 0, st, src->d_postings, src->d_pnorm, d_copy, (uint32_t)n_copy, s->d_postings, s->d_pnorm);
            for (uint32_t r = 0; r < n_rounds && blk.ok(); r++) {
                const UnRound& rd = plan.rounds[r];
                const uint32_t chunks = rd.n_tables * cpt, mr = chunks + 1;
                blk.chk(hipMemsetAsync(d_tables, 0, (size_t)rd.n_tables * n_docs * 4, st));
                if (rd.n_items) hipLaunchKernelGGL(k_un_add, dim3(std::min<uint32_t>((rd.n_items + 3) / 4, 1u << 16)), dim3(256), 0, st, src->d_postings, d_add + rd.first_item, rd.n_items, n_docs, d_tables);
                hipLaunchKernelGGL(k_un_mark, dim3(std::min<uint32_t>((mr + 3) / 4, 1u << 16)), dim3(256), 0, st, d_tables, rd.n_tables, n_docs, cpt, d_mask, d_base);
                ig_scan(st, d_base, mr, d_sums, (uint32_t*)nullptr);
                if (chunks) hipLaunchKernelGGL(k_un_scatter, dim3(std::min<uint32_t>((chunks + 3) / 4, 1u << 16)), dim3(256), 0, st, d_tables, rd.n_tables, n_docs, cpt, d_mask, d_base, d_run + r, src->d_norm, s->d_postings, s->d_pnorm);
                hipLaunchKernelGGL(k_un_lists, dim3((rd.n_tables + 255) / 256), dim3(256), 0, st, d_tabled + rd.first_table, rd.n_tables, cpt, d_base, d_run + r, d_noff, d_ncnt);
                blk.launched();
            }
            hipLaunchKernelGGL(k_un_pad, dim3((kPadPostings + 255) / 256), dim3(256), 0, st, d_run + n_rounds, (uint32_t)kPadPostings, s->d_postings, s->d_pnorm);
            blk.record(1);
            blk.launched();
        }
        // the one synchronisation: how many postings were written, and the groups' places
        if (blk.ok()) blk.chk(hipMemcpyAsync(&written, d_run + n_rounds, 4, hipMemcpyDeviceToHost, st));
        if (blk.ok() && n_groups) {
            blk.fetch(new_byte_off_out, o_noff, (size_t)n_groups * 8);
            blk.fetch(new_counts_out, o_ncnt, (size_t)n_groups * 4);
        }
        if (blk.ok()) blk.sync();
        if (blk.ok() && written > plan.bound) blk.chk(hipErrorUnknown);
        float ms = 0.0f;
        if (blk.elapsed_ms(0, 1, &ms) && device_ms_out) *device_ms_out = ms;
        // the payload for tests and tools: its size is known only now
        if (blk.ok() && postings_out && written) {
            blk.chk(hipMemcpyAsync(postings_out, s->d_postings, (size_t)written * 8, hipMemcpyDeviceToHost, st));
            blk.sync();
        }
    }
    const int rc = blk.finish("ns_segment_union");
    if (rc != NS_OK) {
        seg_free_device(s);
        delete s;
        return rc;
    }
    s->n_postings = written;
    if (n_postings_out) *n_postings_out = written;
    if (rounds_out) *rounds_out = n_rounds;
    if (ctx->segs.size() <= new_seg_id) ctx->segs.resize(new_seg_id + 1, nullptr);
    ctx->segs[new_seg_id] = s;
    *out = s;
    return NS_OK;
}

// The eight counters of ns_forward_build and of the merge, once everything launched so far is done.  Both reserve them
// first in their first block (o_cnt == 0 in block 0).
static void read_counts(CallBlock& blk, uint32_t (&h_cnt)[8]) {
    blk.launched();
    if (blk.ok()) blk.chk(hipMemcpyAsync(h_cnt, blk.at<uint32_t>(0, 0), sizeof(h_cnt), hipMemcpyDeviceToHost, blk.st));
    if (blk.ok()) blk.sync();
}

// The dictionary stage that text ingest runs over its kept tokens and the merge over its source terms:
// K "tokens" (start, length, hash) of d_text, the table of `cap` slots (filled with 0xFF by the caller), and what the stage
// writes per token.  d_owner: a token's document (ingest) or source (merge).
struct DictStage {
    const uint8_t* d_text;
    const uint32_t *d_kstart, *d_klen, *d_owner;
    const uint64_t* d_khash;
    uint32_t K;
    uint32_t* d_table;
    uint64_t cap;
    uint32_t *d_kslot, *d_krep, *d_fid, *d_tsrc, *d_sums;
};
// the distinct byte strings: k_ig_insert, k_ig_first, their number scanned into *d_n_terms; then the counters are read
static void dict_count_terms(CallBlock& blk, const DictStage& D, uint32_t* d_n_terms, uint32_t (&h_cnt)[8]) {
    const uint32_t g = (D.K + 255) / 256;
    hipLaunchKernelGGL(k_ig_insert, dim3(g), dim3(256), 0, blk.st, D.d_text, D.d_kstart, D.d_klen, D.d_khash, D.K, D.d_table, (uint32_t)(D.cap - 1), D.d_kslot);
    hipLaunchKernelGGL(k_ig_first, dim3(g), dim3(256), 0, blk.st, D.d_table, D.d_kslot, D.K, D.d_krep, D.d_fid);
    ig_scan(blk.st, D.d_fid, D.K, D.d_sums, d_n_terms);
    read_counts(blk, h_cnt);
}
// the handle's term offsets: allocated and zeroed; with tokens, k_ig_termid (the tokens' term ids into d_ids, {owner, term} into
// d_vals, the terms' lengths into d_toff) and the lengths scanned, their sum into *d_term_bytes
static void dict_term_ids(CallBlock& blk, const DictStage& D, ns_forward* f, uint32_t n_terms, uint32_t* d_ids, uint2* d_vals, uint32_t* d_term_bytes) {
    if (blk.ok()) blk.chk(hipMalloc((void**)&f->d_toff, ((size_t)n_terms + 1) * 4));
    if (!blk.ok()) return;
    blk.chk(hipMemsetAsync(f->d_toff, 0, ((size_t)n_terms + 1) * 4, blk.st));
    if (!D.K) return;
    hipLaunchKernelGGL(k_ig_termid, dim3((D.K + 255) / 256), dim3(256), 0, blk.st, D.d_krep, D.d_fid, D.d_owner, D.d_kstart, D.d_klen, D.K, d_ids, d_vals, f->d_toff, D.d_tsrc);
    ig_scan(blk.st, f->d_toff, n_terms + 1, D.d_sums, d_term_bytes);
}

// ---- the frame around a forward handle (ns_forward_build and the merge) ----
// test knob (variants build only): narrow the term hash so that every probe collides and the byte comparison decides
static uint64_t ingest_hash_mask() {
#ifdef NS_VARIANTS
    if (const char* hb = std::getenv("NS_INGEST_HASH_BITS")) { const int b = std::atoi(hb); if (b >= 0 && b < 64) return (1ull << b) - 1ull; }
#endif
    return ~0ull;
}
static ns_forward* forward_new(ns_ctx* ctx) {
    ns_forward* f = new ns_forward();
    f->ctx = ctx;
    f->info.struct_size = (uint32_t)sizeof(ns_forward_info);
    return f;
}
static int forward_publish(ns_ctx* ctx, ns_forward* f, ns_forward** out) {
    ctx->fwds.push_back(f);
    *out = f;
    return NS_OK;
}
// the end of a call that built f with `scratch_bytes` of pooled blocks: rc != NS_OK discards the half-built handle
static int forward_finish(ns_ctx* ctx, ns_forward* f, ns_forward** out, size_t scratch_bytes, int rc) {
    f->info.device_bytes = (uint64_t)scratch_bytes + ((uint64_t)f->info.n_terms + 1) * 4 + (uint64_t)f->info.kept_docs * 12 + f->info.n_pairs * 8 + f->info.term_bytes;
    if (rc == NS_OK) return forward_publish(ctx, f, out);
    forward_free_device(f);
    delete f;
    (void)hipGetLastError();
    return rc;
}

extern "C" int ns_forward_build(ns_ctx* ctx, const uint8_t* text, uint64_t text_bytes, const uint64_t* offsets, uint32_t n_docs, ns_forward** out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_forward_build: ctx is NULL");
    if (!out) return fail(ctx, NS_E_INVAL, "ns_forward_build: out is NULL");
    *out = nullptr;
    if (n_docs == 0xFFFFFFFFu) return fail(ctx, NS_E_INVAL, "ns_forward_build: n_docs too large");
    if (n_docs && !offsets) return fail(ctx, NS_E_INVAL, "ns_forward_build: offsets is NULL");
    if (n_docs && offsets[0] != 0) return fail(ctx, NS_E_INVAL, "ns_forward_build: offsets[0] = %llu, not 0", (unsigned long long)offsets[0]);
    for (uint32_t d = 0; d < n_docs; d++)
        if (offsets[d + 1] < offsets[d]) return fail(ctx, NS_E_INVAL, "ns_forward_build: offsets decrease at document %u", d);
    const uint64_t n64 = n_docs ? offsets[n_docs] : 0;
    if (n64 > text_bytes) return fail(ctx, NS_E_INVAL, "ns_forward_build: offsets[n_docs] = %llu lies past the %llu bytes of text", (unsigned long long)n64, (unsigned long long)text_bytes);
    if (n64 >= (1ull << 32) - 65536) return fail(ctx, NS_E_INVAL, "ns_forward_build: %llu bytes of text; this build addresses text with 32 bits (below 4 GiB - 64 KiB per call: split the batch)", (unsigned long long)n64);
    if (n64 && !text) return fail(ctx, NS_E_INVAL, "ns_forward_build: text is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ns_forward* f = forward_new(ctx);
    f->info.n_docs = n_docs;
    if (n64 == 0) return forward_publish(ctx, f, out);   // no text: no token, no document survives
    const uint32_t n = (uint32_t)n64;
    hipStream_t st = ctx->stream;
    const uint64_t hash_mask = ingest_hash_mask();
    CallBlock blk(ctx);
    uint32_t h_cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    enum { C_TOK = 0, C_TOKE = 1, C_KEPT = 2, C_LONG = 3, C_KD = 4, C_TERMS = 5, C_TBYTES = 6, C_PAIRS = 7 };
    const uint32_t nd1 = n_docs + 1, n_tiles = (n + kIgTile - 1) / kIgTile;
    const uint32_t g_docs = (n_docs + 255) / 256;
    std::vector<uint32_t> offs32(nd1);
    for (uint32_t d = 0; d <= n_docs; d++) offs32[d] = (uint32_t)offsets[d];

    // ---- block A: what the text and the documents size ----
    const size_t o_cnt = blk.reserve(sizeof(h_cnt)), o_text = blk.reserve((size_t)n + 16), o_bits = blk.reserve(((size_t)(n >> 5) + 2) * 4), o_offs = blk.reserve((size_t)nd1 * 4);
    const size_t o_ts = blk.reserve((size_t)n_tiles * 4), o_te = blk.reserve((size_t)n_tiles * 4), o_sumsA = blk.reserve(((size_t)std::max(n_tiles, n_docs) / 1024 + 2) * 4);
    const size_t o_long = blk.reserve(((size_t)n / kIgLong + 1) * 4);
    const size_t o_df = blk.reserve((size_t)n_docs * 4), o_dl = blk.reserve((size_t)n_docs * 4), o_pf = blk.reserve((size_t)n_docs * 4), o_pl = blk.reserve((size_t)n_docs * 4),
                 o_dx = blk.reserve((size_t)n_docs * 4);
    blk.alloc(2);
    uint32_t n_tok = 0, n_kept = 0;
    if (blk.ok()) {
        uint32_t* d_cntv = blk.at<uint32_t>(o_cnt);
        uint8_t* d_text = blk.at<uint8_t>(o_text);
        uint32_t *d_bits = blk.at<uint32_t>(o_bits), *d_offs = blk.at<uint32_t>(o_offs), *d_ts = blk.at<uint32_t>(o_ts), *d_te = blk.at<uint32_t>(o_te);
        uint32_t *d_sumsA = blk.at<uint32_t>(o_sumsA), *d_long = blk.at<uint32_t>(o_long);
        uint32_t *d_dfirst = blk.at<uint32_t>(o_df), *d_dlast = blk.at<uint32_t>(o_dl), *d_pfirst = blk.at<uint32_t>(o_pf), *d_plast = blk.at<uint32_t>(o_pl),
                 *d_didx = blk.at<uint32_t>(o_dx);
        blk.upload(o_text, text, n);
        blk.upload(o_offs, offs32.data(), (size_t)nd1 * 4);
        blk.record(0);
        blk.zero(o_cnt, sizeof(h_cnt));
        blk.zero(o_bits, ((size_t)(n >> 5) + 2) * 4);
        blk.chk(hipMemsetAsync(d_dfirst, 0xFF, (size_t)n_docs * 4, st));
        blk.chk(hipMemsetAsync(d_pfirst, 0xFF, (size_t)n_docs * 4, st));
        hipLaunchKernelGGL(k_ig_docmark, dim3(g_docs), dim3(256), 0, st, d_offs, n_docs, n, d_bits);
        hipLaunchKernelGGL((k_ig_text<false>), dim3(n_tiles), dim3(256), 0, st, d_text, n, d_bits, d_ts, d_te, (uint32_t*)nullptr, (uint32_t*)nullptr);
        ig_scan(st, d_ts, n_tiles, d_sumsA, d_cntv + C_TOK);
        ig_scan(st, d_te, n_tiles, d_sumsA, d_cntv + C_TOKE);
        read_counts(blk, h_cnt);
        n_tok = h_cnt[C_TOK];
        if (blk.ok() && h_cnt[C_TOKE] != n_tok) blk.chk(hipErrorUnknown);   // every token has one start and one end
        f->info.n_tokens = n_tok;

        // ---- block B: what the tokens size ----
        uint32_t *d_tstart = nullptr, *d_tend = nullptr, *d_kidx = nullptr, *d_sums = nullptr;
        if (blk.ok() && n_tok) {
            blk.open();
            const size_t o_a = blk.reserve((size_t)n_tok * 4), o_b = blk.reserve((size_t)n_tok * 4), o_c = blk.reserve((size_t)n_tok * 4);
            const size_t scan_max = std::max<size_t>((size_t)n_tok + 1, (size_t)2048 * ((n_tok + kIvTile - 1) / kIvTile));
            const size_t o_s = blk.reserve((scan_max / 1024 + 2) * 4);
            blk.alloc(0);
            if (blk.ok()) {
                d_tstart = blk.at<uint32_t>(o_a); d_tend = blk.at<uint32_t>(o_b); d_kidx = blk.at<uint32_t>(o_c); d_sums = blk.at<uint32_t>(o_s);
                hipLaunchKernelGGL((k_ig_text<true>), dim3(n_tiles), dim3(256), 0, st, d_text, n, d_bits, d_ts, d_te, d_tstart, d_tend);
                hipLaunchKernelGGL(k_ig_keep, dim3((n_tok + 255) / 256), dim3(256), 0, st, d_text, d_tstart, d_tend, n_tok, d_kidx);
                ig_scan(st, d_kidx, n_tok, d_sums, d_cntv + C_KEPT);
                read_counts(blk, h_cnt);
                n_kept = h_cnt[C_KEPT];
                f->info.kept_tokens = n_kept;
            }
        }
        // ---- block C: what the kept tokens size ----
        if (blk.ok() && n_kept) {
            const uint32_t K = n_kept, gK = (K + 255) / 256, kt = (K + kIvTile - 1) / kIvTile;
            const uint64_t cap = ig_table_slots(K);                // K <= n / 2 < 2^31: cap <= 2^32, its mask fits 32 bits
            blk.open();
            const size_t o_ks = blk.reserve((size_t)K * 4), o_kl = blk.reserve((size_t)K * 4), o_kd = blk.reserve((size_t)K * 4), o_kh = blk.reserve((size_t)K * 8);
            const size_t o_sl = blk.reserve((size_t)K * 4), o_kr = blk.reserve((size_t)K * 4), o_fi = blk.reserve((size_t)K * 4), o_tsrc = blk.reserve((size_t)K * 4);
            const size_t o_tab = blk.reserve((size_t)cap * 4), o_k0 = blk.reserve((size_t)K * 4), o_k1 = blk.reserve((size_t)K * 4), o_v0 = blk.reserve((size_t)K * 8),
                         o_v1 = blk.reserve((size_t)K * 8);
            const size_t o_hist = blk.reserve((size_t)2048 * kt * 4);
            blk.alloc(0);
            if (blk.ok()) {
                uint32_t *d_kstart = blk.at<uint32_t>(o_ks), *d_klen = blk.at<uint32_t>(o_kl), *d_kdoc = blk.at<uint32_t>(o_kd);
                uint64_t* d_khash = blk.at<uint64_t>(o_kh);
                uint32_t *d_kslot = blk.at<uint32_t>(o_sl), *d_krep = blk.at<uint32_t>(o_kr), *d_fid = blk.at<uint32_t>(o_fi), *d_tsrc = blk.at<uint32_t>(o_tsrc);
                uint32_t* d_table = blk.at<uint32_t>(o_tab);
                uint32_t* d_keys[2] = {blk.at<uint32_t>(o_k0), blk.at<uint32_t>(o_k1)};
                uint2* d_vals[2] = {blk.at<uint2>(o_v0), blk.at<uint2>(o_v1)};
                uint32_t* d_hist = blk.at<uint32_t>(o_hist);
                blk.chk(hipMemsetAsync(d_table, 0xFF, (size_t)cap * 4, st));
                hipLaunchKernelGGL(k_ig_kept, dim3((n_tok + 255) / 256), dim3(256), 0, st, d_text, d_tstart, d_tend, n_tok, d_kidx, d_cntv + C_KEPT, d_offs, n_docs,
                                   hash_mask, d_kstart, d_klen, d_kdoc, d_khash, d_long, d_cntv + C_LONG);
                hipLaunchKernelGGL(k_ig_hash_long, dim3(1024), dim3(256), 0, st, d_text, d_kstart, d_klen, d_long, d_cntv + C_LONG, hash_mask, d_khash);
                // doc_len: the kept tokens are in document order, a document's tokens are one run of kdoc
                hipLaunchKernelGGL(k_iv_runs, dim3((K + 1023) / 1024), dim3(256), 0, st, d_kdoc, K, n_docs, d_dfirst, d_dlast, (const uint32_t*)nullptr);
                hipLaunchKernelGGL(k_ig_docflag, dim3(g_docs), dim3(256), 0, st, d_dfirst, n_docs, d_didx);
                ig_scan(st, d_didx, n_docs, d_sumsA, d_cntv + C_KD);
                const DictStage dict{d_text, d_kstart, d_klen, d_kdoc, d_khash, K, d_table, cap, d_kslot, d_krep, d_fid, d_tsrc, d_sums};
                dict_count_terms(blk, dict, d_cntv + C_TERMS, h_cnt);
                const uint32_t n_terms = h_cnt[C_TERMS], n_kd = h_cnt[C_KD];
                f->info.n_terms = n_terms; f->info.kept_docs = n_kd;
                if (blk.ok()) {
                    blk.chk(hipMalloc((void**)&f->d_map, (size_t)n_kd * 4));
                    blk.chk(hipMalloc((void**)&f->d_len, (size_t)n_kd * 4));
                    blk.chk(hipMalloc((void**)&f->d_cnt, (size_t)n_kd * 4));
                }
                int cur = 0;
                dict_term_ids(blk, dict, f, n_terms, d_keys[0], d_vals[0], d_cntv + C_TBYTES);
                if (blk.ok()) {
                    ig_sort(st, K, n_terms, d_keys, d_vals, &cur, d_hist, d_sums);
                    hipLaunchKernelGGL(k_ig_runflag, dim3(gK), dim3(256), 0, st, d_vals[cur], K, d_kslot);
                    ig_scan(st, d_kslot, K, d_sums, d_cntv + C_PAIRS);
                    read_counts(blk, h_cnt);
                }
                const uint32_t n_pairs = h_cnt[C_PAIRS], tbytes = h_cnt[C_TBYTES];
                f->info.n_pairs = n_pairs; f->info.term_bytes = tbytes;
                if (blk.ok()) {
                    blk.chk(hipMalloc((void**)&f->d_terms, std::max<size_t>(tbytes, 1)));
                    blk.chk(hipMalloc((void**)&f->d_pairs, (size_t)n_pairs * 8));
                }
                if (blk.ok()) {
                    hipLaunchKernelGGL(k_ig_term_bytes, dim3((n_terms + 3) / 4), dim3(256), 0, st, d_text, d_tsrc, f->d_toff, n_terms, f->d_terms);
                    // the runs, (term, doc)-ordered: keys = doc, values = {term, tf}, into the buffer the first sort left free
                    const int in = cur ^ 1;
                    uint32_t *d_rterm = d_krep, *d_rpos = d_kstart;   // (dead since k_ig_termid)
                    hipLaunchKernelGGL(k_ig_runemit, dim3(gK), dim3(256), 0, st, d_vals[cur], K, d_kslot, d_keys[in], d_rterm, d_rpos);
                    hipLaunchKernelGGL(k_ig_tf, dim3((n_pairs + 255) / 256), dim3(256), 0, st, d_rterm, d_rpos, n_pairs, K, d_vals[in]);
                    cur = in;
                    ig_sort(st, n_pairs, n_docs, d_keys, d_vals, &cur, d_hist, d_sums);
                    hipLaunchKernelGGL(k_iv_runs, dim3((n_pairs + 1023) / 1024), dim3(256), 0, st, d_keys[cur], n_pairs, n_docs, d_pfirst, d_plast, (const uint32_t*)nullptr);
                    hipLaunchKernelGGL(k_ig_docemit, dim3(g_docs), dim3(256), 0, st, d_dfirst, d_dlast, d_pfirst, d_plast, d_didx, n_docs, f->d_map, f->d_len, f->d_cnt);
                    blk.chk(hipMemcpyAsync(f->d_pairs, d_vals[cur], (size_t)n_pairs * 8, hipMemcpyDeviceToDevice, st));
                    blk.launched();
                }
            }
        }
        if (blk.ok()) blk.record(1);
        if (blk.ok()) blk.sync();
        float ms = 0.0f;
        if (blk.elapsed_ms(0, 1, &ms)) f->info.device_ms = ms;
    }
    const int rc = blk.finish("ns_forward_build", blk.e == hipErrorUnknown ? "token starts and ends disagree (internal error)" : nullptr);
    return forward_finish(ctx, f, out, blk.held_bytes(), rc);
}

extern "C" int ns_forward_get_info(const ns_forward* fwd, ns_forward_info* info) {
    ns_ctx* ctx = fwd ? fwd->ctx : nullptr;
    if (!fwd || !info) return fail(ctx, NS_E_INVAL, "ns_forward_get_info: null argument");
    if (info->struct_size < 4) return fail(ctx, NS_E_INVAL, "ns_forward_get_info: struct_size = %u (the caller sets it to sizeof(ns_forward_info))", info->struct_size);
    const uint32_t sz = std::min<uint32_t>(info->struct_size, (uint32_t)sizeof(ns_forward_info));
    ns_forward_info tmp = fwd->info;
    tmp.struct_size = sz;
    std::memcpy(info, &tmp, sz);
    return NS_OK;
}

extern "C" int ns_forward_fetch(ns_forward* fwd, uint32_t* kept_docs_out, uint32_t* doc_len_out, uint32_t* counts_out,
                                uint32_t* pairs_out, uint8_t* term_bytes_out, uint64_t* term_offsets_out) {
    if (!fwd) return fail(nullptr, NS_E_INVAL, "ns_forward_fetch: handle is NULL");
    ns_ctx* ctx = fwd->ctx;
    if (!ctx) return fail(nullptr, NS_E_STATE, "ns_forward_fetch: the handle's ctx has been destroyed");
    const ns_forward_info& in = fwd->info;
    if (in.kept_docs == 0) {   // empty result: nothing on the device
        if (term_offsets_out) term_offsets_out[0] = 0;
        return NS_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (kept_docs_out) HIPCHK(ctx, hipMemcpy(kept_docs_out, fwd->d_map, (size_t)in.kept_docs * 4, hipMemcpyDeviceToHost));
    if (doc_len_out) HIPCHK(ctx, hipMemcpy(doc_len_out, fwd->d_len, (size_t)in.kept_docs * 4, hipMemcpyDeviceToHost));
    if (counts_out) HIPCHK(ctx, hipMemcpy(counts_out, fwd->d_cnt, (size_t)in.kept_docs * 4, hipMemcpyDeviceToHost));
    if (pairs_out && in.n_pairs) HIPCHK(ctx, hipMemcpy(pairs_out, fwd->d_pairs, (size_t)in.n_pairs * 8, hipMemcpyDeviceToHost));
    if (term_bytes_out && in.term_bytes) HIPCHK(ctx, hipMemcpy(term_bytes_out, fwd->d_terms, (size_t)in.term_bytes, hipMemcpyDeviceToHost));
    if (term_offsets_out) {
        std::vector<uint32_t> t32((size_t)in.n_terms + 1);
        HIPCHK(ctx, hipMemcpy(t32.data(), fwd->d_toff, t32.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < t32.size(); i++) term_offsets_out[i] = t32[i];
    }
    return NS_OK;
}

extern "C" void ns_forward_destroy(ns_forward* fwd) {
    if (!fwd) return;
    if (ns_ctx* ctx = fwd->ctx) {
        (void)hipSetDevice(ctx->device);
        auto it = std::find(ctx->fwds.begin(), ctx->fwds.end(), fwd);
        if (it != ctx->fwds.end()) ctx->fwds.erase(it);
        forward_free_device(fwd);
    }
    delete fwd;
}

// ------------------------------------------------------------------------------------------------
// Compaction: the forward indexes of several segments -> one (csrc/ns_compact.hip)
extern "C" uint32_t ns_compact_doc_cut(void) { return kCpDocCut; }
extern "C" uint32_t ns_radix_plan(uint32_t key_range, uint32_t pbits_out[3]) {
    const RadixPlan rp = radix_plan(key_range);
    for (int p = 0; pbits_out && p < 3; p++) pbits_out[p] = (uint32_t)rp.pbits[p];
    return (uint32_t)rp.passes;
}
extern "C" uint32_t ns_radix_tile(void) { return (uint32_t)kIvTile; }

extern "C" int ns_ctx_use_docsort(ns_ctx* ctx, int on) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_ctx_use_docsort: ctx is NULL");
    ctx->cp_inplace = on != 0;
    return NS_OK;
}

// The body of ns_forward_merge and ns_forward_merge_keep (fn: the entry point's name for the messages).  keep == NULL, or
// every keep[s] NULL: the plain merge, launch for launch what it always was.  Otherwise the filter stages of
// csrc/ns_delete.hip run first and hand the dictionary, remap and docsort stages their input in device memory.
static int forward_merge_run(ns_ctx* ctx, const char* fn, const ns_forward_src* src, const uint32_t* const* keep, uint32_t n_src, ns_forward** out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "%s: ctx is NULL", fn);
    if (!out) return fail(ctx, NS_E_INVAL, "%s: out is NULL", fn);
    *out = nullptr;
    if (n_src && !src) return fail(ctx, NS_E_INVAL, "%s: src is NULL", fn);
    MergePlan plan;                                                    // everything the host derives from the sources (ns_merge_plan.hpp)
    std::string why;
    if (!merge_plan(src, keep, n_src, ctx->cp_inplace, plan, why)) return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    const bool filtered = plan.filtered;
    const uint32_t raw_pairs = plan.raw_pairs, T = plan.T, n = plan.text_bytes, n_docs = plan.n_docs, n_pairs = plan.n_pairs;
    const uint32_t n_wave = plan.n_wave, n_lds = plan.n_lds, n_bigdocs = plan.n_bigdocs, n_big = plan.n_big;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ns_forward* f = forward_new(ctx);
    if (n_docs == 0) return forward_publish(ctx, f, out);   // no document: an empty result, whatever the term lists hold
    f->info.n_docs = f->info.kept_docs = n_docs;
    f->info.n_tokens = f->info.kept_tokens = plan.total_len;
    f->info.n_pairs = n_pairs;
    hipStream_t st = ctx->stream;
    const uint64_t hash_mask = ingest_hash_mask();

    CallBlock blk(ctx);
    uint32_t h_cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    enum { C_TERMS = 0, C_TBYTES = 1, C_LONG = 2, C_LIVE = 3, C_DUP = 4, C_BAD = 5 };   // C_DUP / C_BAD: the smallest refused source, ~0 for none; C_LIVE: the terms that stay (filtered)
    const uint64_t cap = ig_table_slots(T);                            // T < 2^31: cap <= 2^32, its mask fits 32 bits
    const uint32_t big_tiles = (n_big + kIvTile - 1) / kIvTile;
    const size_t scan_max = std::max<size_t>({(size_t)T + 1, (size_t)2048 * big_tiles, (size_t)1});

    // ---- block A: the dictionary stage, sized by the source terms; the per-source bases, the document prefix, the lists ----
    const size_t T1 = std::max<uint32_t>(T, 1);
    const size_t o_cnt = blk.reserve(sizeof(h_cnt)), o_text = blk.reserve((size_t)n + 16), o_ks = blk.reserve(T1 * 4), o_kl = blk.reserve(T1 * 4), o_src = blk.reserve(T1 * 4),
                 o_kh = blk.reserve(T1 * 8);
    const size_t o_sl = blk.reserve(T1 * 4), o_kr = blk.reserve(T1 * 4), o_fi = blk.reserve(T1 * 4), o_tsrc = blk.reserve(T1 * 4), o_map = blk.reserve(T1 * 4),
                 o_vals = blk.reserve(T1 * 8);
    const size_t o_tab = blk.reserve((size_t)cap * 4), o_dtab = blk.reserve((size_t)cap * 8), o_long = blk.reserve(((size_t)n / kIgLong + 1) * 4),
                 o_sums = blk.reserve((scan_max / 1024 + 2) * 4);
    const size_t o_tb = blk.reserve(plan.term_base.size() * 4), o_pb = blk.reserve(plan.pair_base.size() * 4), o_prefix = blk.reserve(plan.prefix.size() * 4),
                 o_lists = blk.reserve(plan.lists.size() * 4);
    const size_t A = blk.alloc(2);
    // ---- block F (filtered only): the pairs as uploaded, the live flags and their scan, the source terms' (start, length),
    // the surviving terms' per-source base, the (source, old id) -> new id map, the surviving documents' places in the upload ----
    blk.open();
    const size_t o_raw = blk.reserve((size_t)raw_pairs * 8), o_live = blk.reserve(((size_t)T + 1) * 4), o_rank = blk.reserve(((size_t)T + 1) * 4), o_ks0 = blk.reserve(T1 * 4),
                 o_kl0 = blk.reserve(T1 * 4);
    const size_t o_tbl = blk.reserve(plan.term_base.size() * 4), o_omap = blk.reserve(T1 * 4), o_spos = blk.reserve((size_t)n_docs * 4);
    const size_t F = filtered ? blk.alloc(0) : A;
    blk.chk(hipMalloc((void**)&f->d_pairs, (size_t)n_pairs * 8));
    blk.chk(hipMalloc((void**)&f->d_map, (size_t)n_docs * 4));
    blk.chk(hipMalloc((void**)&f->d_len, (size_t)n_docs * 4));
    blk.chk(hipMalloc((void**)&f->d_cnt, (size_t)n_docs * 4));
    uint32_t n_terms = 0, tbytes = 0;
    int refused_src = -1;
    const char* refused_why = "";
    if (blk.ok()) {
        uint32_t* d_cntv = blk.at<uint32_t>(o_cnt, A);
        uint8_t* d_text = blk.at<uint8_t>(o_text, A);
        uint32_t *d_kstart = blk.at<uint32_t>(o_ks, A), *d_klen = blk.at<uint32_t>(o_kl, A), *d_ksrc = blk.at<uint32_t>(o_src, A);
        uint64_t* d_khash = blk.at<uint64_t>(o_kh, A);
        uint32_t *d_kslot = blk.at<uint32_t>(o_sl, A), *d_krep = blk.at<uint32_t>(o_kr, A), *d_fid = blk.at<uint32_t>(o_fi, A), *d_tsrc = blk.at<uint32_t>(o_tsrc, A);
        uint32_t* d_newid = blk.at<uint32_t>(o_map, A);
        uint2* d_tvals = blk.at<uint2>(o_vals, A);                     // k_ig_termid's {source, new id} per source term: written, not read
        uint32_t* d_table = blk.at<uint32_t>(o_tab, A);
        unsigned long long* d_dtab = blk.at<unsigned long long>(o_dtab, A);
        uint32_t *d_long = blk.at<uint32_t>(o_long, A), *d_sums = blk.at<uint32_t>(o_sums, A);
        uint32_t *d_tb = blk.at<uint32_t>(o_tb, A), *d_pb = blk.at<uint32_t>(o_pb, A), *d_prefix = blk.at<uint32_t>(o_prefix, A), *d_lists = blk.at<uint32_t>(o_lists, A);
        uint2* d_raw = filtered ? blk.at<uint2>(o_raw, F) : nullptr;
        uint32_t *d_live = filtered ? blk.at<uint32_t>(o_live, F) : nullptr, *d_rank = filtered ? blk.at<uint32_t>(o_rank, F) : nullptr;
        uint32_t *d_ks0 = filtered ? blk.at<uint32_t>(o_ks0, F) : d_kstart, *d_kl0 = filtered ? blk.at<uint32_t>(o_kl0, F) : d_klen;   // where the host's (start, length) go
        uint32_t *d_tbl = filtered ? blk.at<uint32_t>(o_tbl, F) : d_tb, *d_omap = filtered ? blk.at<uint32_t>(o_omap, F) : d_newid, *d_spos = filtered ? blk.at<uint32_t>(o_spos, F) : nullptr;
        const uint32_t *d_lwave = d_lists, *d_llds = d_lists + n_wave, *d_lbig = d_lists + n_wave + n_lds, *d_bigpre = d_lists + n_wave + n_lds + n_bigdocs;
        // uploads: term bytes, pairs, counts and doc_len source by source; the host-made arrays
        {
            uint32_t at = 0, d = 0;
            for (uint32_t s = 0; s < n_src; s++) {
                const ns_forward_src& S = src[s];
                const uint32_t nb = S.n_terms ? (uint32_t)(S.term_offsets[S.n_terms] - S.term_offsets[0]) : 0u;
                if (nb) blk.chk(hipMemcpyAsync(d_text + at, S.term_bytes + S.term_offsets[0], nb, hipMemcpyHostToDevice, st));
                if (filtered) {   // (a source without a surviving pair is not uploaded: nothing reads it)
                    if (plan.pair_base[s + 1] != plan.pair_base[s]) blk.chk(hipMemcpyAsync(d_raw + plan.raw_base[s], S.pairs, (size_t)S.n_pairs * 8, hipMemcpyHostToDevice, st));
                } else if (S.n_pairs) blk.chk(hipMemcpyAsync(f->d_pairs + plan.pair_base[s], S.pairs, (size_t)S.n_pairs * 8, hipMemcpyHostToDevice, st));
                if (S.n_docs && !filtered) {
                    blk.chk(hipMemcpyAsync(f->d_len + d, S.doc_len, (size_t)S.n_docs * 4, hipMemcpyHostToDevice, st));
                    blk.chk(hipMemcpyAsync(f->d_cnt + d, S.counts, (size_t)S.n_docs * 4, hipMemcpyHostToDevice, st));
                }
                at += nb; d += S.n_docs;
            }
        }
        std::vector<uint32_t> iota(n_docs);
        for (uint32_t d = 0; d < n_docs; d++) iota[d] = d;
        blk.chk(hipMemcpyAsync(f->d_map, iota.data(), (size_t)n_docs * 4, hipMemcpyHostToDevice, st));
        if (T) {
            blk.chk(hipMemcpyAsync(d_ks0, plan.kstart.data(), (size_t)T * 4, hipMemcpyHostToDevice, st));
            blk.chk(hipMemcpyAsync(d_kl0, plan.klen.data(), (size_t)T * 4, hipMemcpyHostToDevice, st));
        }
        if (filtered) {
            blk.chk(hipMemcpyAsync(f->d_len, plan.kept_len.data(), (size_t)n_docs * 4, hipMemcpyHostToDevice, st));
            blk.chk(hipMemcpyAsync(f->d_cnt, plan.kept_cnt.data(), (size_t)n_docs * 4, hipMemcpyHostToDevice, st));
            blk.chk(hipMemcpyAsync(d_spos, plan.srcpos.data(), (size_t)n_docs * 4, hipMemcpyHostToDevice, st));
            blk.chk(hipMemcpyAsync(d_live, plan.live0.data(), ((size_t)T + 1) * 4, hipMemcpyHostToDevice, st));
        }
        blk.chk(hipMemcpyAsync(d_tb, plan.term_base.data(), plan.term_base.size() * 4, hipMemcpyHostToDevice, st));
        blk.chk(hipMemcpyAsync(d_pb, plan.pair_base.data(), plan.pair_base.size() * 4, hipMemcpyHostToDevice, st));
        blk.chk(hipMemcpyAsync(d_prefix, plan.prefix.data(), plan.prefix.size() * 4, hipMemcpyHostToDevice, st));
        blk.chk(hipMemcpyAsync(d_lists, plan.lists.data(), plan.lists.size() * 4, hipMemcpyHostToDevice, st));
        blk.record(0);
        h_cnt[C_DUP] = h_cnt[C_BAD] = 0xFFFFFFFFu;
        blk.chk(hipMemcpyAsync(d_cntv, h_cnt, sizeof(h_cnt), hipMemcpyHostToDevice, st));
        // ---- the filter (csrc/ns_delete.hip): afterwards Td "tokens" in d_kstart / d_klen with their bases in d_tbl, the
        // surviving pairs in f->d_pairs under the sources' OLD term ids ----
        uint32_t Td = T;                                               // the dictionary stage's tokens: the source terms that stay
        if (blk.ok() && filtered) {
            if (n_pairs) {
                const uint32_t gK = (n_pairs + kCpKeepTile - 1) / kCpKeepTile;
#ifdef NS_VARIANTS
                // test and A/B knob (variants build only): every pair searches the whole document prefix; same bytes
                if (std::getenv("NS_KEEP_FULL_SEARCH")) hipLaunchKernelGGL((k_cp_keep_gather<false>), dim3(gK), dim3(256), 0, st, d_raw, d_prefix, d_spos, n_docs, n_pairs, d_pb, d_tb, n_src, f->d_pairs, d_live);
                else
#endif
                hipLaunchKernelGGL((k_cp_keep_gather<true>), dim3(gK), dim3(256), 0, st, d_raw, d_prefix, d_spos, n_docs, n_pairs, d_pb, d_tb, n_src, f->d_pairs, d_live);
            }
            blk.chk(hipMemcpyAsync(d_rank, d_live, ((size_t)T + 1) * 4, hipMemcpyDeviceToDevice, st));
            ig_scan(st, d_rank, T + 1, d_sums, d_cntv + C_LIVE);       // (entry T is 0: the total is rank[T] as well)
            hipLaunchKernelGGL(k_cp_keep_terms, dim3((std::max(T, n_src + 1) + 255) / 256), dim3(256), 0, st, d_live, d_rank, T, d_ks0, d_kl0, d_tb, n_src, d_kstart, d_klen, d_tbl);
            read_counts(blk, h_cnt);
            Td = h_cnt[C_LIVE];
        }
        const uint64_t capd = ig_table_slots(Td);                      // == cap unless terms were dropped
        const uint32_t gT = (Td + 255) / 256;
        const DictStage dict{d_text, d_kstart, d_klen, d_ksrc, d_khash, Td, d_table, capd, d_kslot, d_krep, d_fid, d_tsrc, d_sums};
        if (blk.ok() && Td) {
            blk.chk(hipMemsetAsync(d_table, 0xFF, (size_t)capd * 4, st));
            blk.chk(hipMemsetAsync(d_dtab, 0xFF, (size_t)capd * 8, st));
            hipLaunchKernelGGL(k_cp_hash, dim3(gT), dim3(256), 0, st, d_text, d_kstart, d_klen, Td, d_tbl, n_src, hash_mask, d_ksrc, d_khash, d_long, d_cntv + C_LONG);
            hipLaunchKernelGGL(k_ig_hash_long, dim3(1024), dim3(256), 0, st, d_text, d_kstart, d_klen, d_long, d_cntv + C_LONG, hash_mask, d_khash);
            dict_count_terms(blk, dict, d_cntv + C_TERMS, h_cnt);
            n_terms = h_cnt[C_TERMS];
        }
        f->info.n_terms = n_terms;
        dict_term_ids(blk, dict, f, n_terms, d_newid, d_tvals, d_cntv + C_TBYTES);
        if (blk.ok()) {
            if (Td) hipLaunchKernelGGL(k_cp_dup, dim3(gT), dim3(256), 0, st, d_newid, d_ksrc, Td, d_dtab, (uint32_t)(capd - 1), d_cntv + C_DUP);
            // d_omap: the map over the sources' own term ids (filtered: through the ranks; otherwise d_newid itself)
            if (filtered && T) hipLaunchKernelGGL(k_cp_keep_map, dim3((T + 255) / 256), dim3(256), 0, st, d_live, d_rank, T, d_newid, d_omap);
            if (n_pairs) hipLaunchKernelGGL(k_cp_remap, dim3((n_pairs + 255) / 256), dim3(256), 0, st, f->d_pairs, n_pairs, d_pb, d_tb, n_src, d_omap, d_cntv + C_BAD);
            read_counts(blk, h_cnt);
            tbytes = h_cnt[C_TBYTES];
            f->info.term_bytes = tbytes;
            if (blk.ok() && h_cnt[C_DUP] != 0xFFFFFFFFu) { refused_src = (int)h_cnt[C_DUP]; refused_why = "one byte string occurs twice in its term list"; }
            else if (blk.ok() && h_cnt[C_BAD] != 0xFFFFFFFFu) { refused_src = (int)h_cnt[C_BAD]; refused_why = "a pair's termId is not below the source's n_terms"; }
        }
        if (blk.ok() && refused_src < 0) blk.chk(hipMalloc((void**)&f->d_terms, std::max<size_t>(tbytes, 1)));
        if (blk.ok() && refused_src < 0) {
            if (n_terms) hipLaunchKernelGGL(k_ig_term_bytes, dim3((n_terms + 3) / 4), dim3(256), 0, st, d_text, d_tsrc, f->d_toff, n_terms, f->d_terms);
            // ---- the order inside each document ----
            if (n_wave) hipLaunchKernelGGL(k_cp_docsort_wave, dim3((n_wave + 3) / 4), dim3(256), 0, st, f->d_pairs, d_prefix, d_lwave, n_wave);
            if (n_lds) hipLaunchKernelGGL(k_cp_docsort_lds, dim3(n_lds), dim3(256), 0, st, f->d_pairs, d_prefix, d_llds);
            if (n_big) {
                blk.open();
                const size_t o_k0 = blk.reserve((size_t)n_big * 4), o_k1 = blk.reserve((size_t)n_big * 4), o_v0 = blk.reserve((size_t)n_big * 8),
                             o_v1 = blk.reserve((size_t)n_big * 8);
                const size_t o_hist = blk.reserve((size_t)2048 * big_tiles * 4);
                blk.alloc(0);
                if (blk.ok()) {
                    uint32_t* d_keys[2] = {blk.at<uint32_t>(o_k0), blk.at<uint32_t>(o_k1)};
                    uint2* d_vals[2] = {blk.at<uint2>(o_v0), blk.at<uint2>(o_v1)};
                    uint32_t* d_hist = blk.at<uint32_t>(o_hist);
                    const uint32_t gB = (n_big + 255) / 256;
                    int cur = 0;
                    hipLaunchKernelGGL(k_cp_big_gather, dim3(gB), dim3(256), 0, st, f->d_pairs, d_prefix, d_lbig, d_bigpre, n_bigdocs, n_big, d_keys[0], d_vals[0]);
                    ig_sort(st, n_big, n_terms, d_keys, d_vals, &cur, d_hist, d_sums);
                    hipLaunchKernelGGL(k_cp_big_rekey, dim3(gB), dim3(256), 0, st, d_keys[cur], d_vals[cur], n_big, d_keys[cur ^ 1], d_vals[cur ^ 1]);
                    cur ^= 1;
                    ig_sort(st, n_big, n_bigdocs, d_keys, d_vals, &cur, d_hist, d_sums);
                    hipLaunchKernelGGL(k_cp_big_scatter, dim3(gB), dim3(256), 0, st, d_keys[cur], d_vals[cur], n_big, d_prefix, d_lbig, d_bigpre, f->d_pairs);
                }
            }
            blk.launched();
        }
        if (blk.ok()) blk.record(1);
        if (blk.ok()) blk.sync();
        float ms = 0.0f;
        if (blk.elapsed_ms(0, 1, &ms)) f->info.device_ms = ms;
    }
    int rc = blk.finish(fn);
    if (refused_src >= 0) rc = fail(ctx, NS_E_INVAL, "%s: source %d: %s", fn, refused_src, refused_why);   // (the refusal is what the caller hears of)
    return forward_finish(ctx, f, out, blk.held_bytes(), rc);
}

extern "C" int ns_forward_merge(ns_ctx* ctx, const ns_forward_src* src, uint32_t n_src, ns_forward** out) {
    return forward_merge_run(ctx, "ns_forward_merge", src, nullptr, n_src, out);
}

// ------------------------------------------------------------------------------------------------
// Deleting documents: the merge over filtered sources (csrc/ns_delete.hip)
extern "C" int ns_forward_merge_keep(ns_ctx* ctx, const ns_forward_src* src, const uint32_t* const* keep, uint32_t n_src, ns_forward** out) {
    return forward_merge_run(ctx, "ns_forward_merge_keep", src, keep, n_src, out);
}

extern "C" int ns_forward_invert(ns_forward* fwd, uint32_t* df_out, void* postings_out, uint64_t* kept_out, float* device_ms_out) {
    if (!fwd) return fail(nullptr, NS_E_INVAL, "ns_forward_invert: handle is NULL");
    ns_ctx* ctx = fwd->ctx;
    if (!ctx) return fail(nullptr, NS_E_STATE, "ns_forward_invert: the handle's ctx has been destroyed");
    const ns_forward_info& in = fwd->info;
    if (!kept_out || (in.n_terms && !df_out) || (in.n_pairs && !postings_out)) return fail(ctx, NS_E_INVAL, "ns_forward_invert: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> counts(in.kept_docs);                       // the host keeps the prefix sums (the tiles' first and last documents)
    if (in.kept_docs) HIPCHK(ctx, hipMemcpy(counts.data(), fwd->d_cnt, (size_t)in.kept_docs * 4, hipMemcpyDeviceToHost));
    return invert_run(ctx, counts.data(), in.kept_docs, nullptr, in.n_pairs, in.n_terms, df_out, postings_out, kept_out, device_ms_out, nullptr,
                      in.n_pairs ? fwd->d_pairs : nullptr);
}

// ------------------------------------------------------------------------------------------------
// "More like this": the most telling terms of a batch of documents (csrc/ns_similar.hip)
struct ns_docterms {
    ns_ctx* ctx = nullptr;          // nullptr: orphaned by ns_ctx_destroy (the device arrays below are gone)
    uint32_t n_docs = 0, n_terms = 0, n_pairs = 0;
    std::vector<uint32_t> doc_off;  // n_docs + 1: the host keeps the offsets too (the size class of a listed document)
    uint2* d_pairs = nullptr;       // n_pairs {termId, tf}
    uint32_t* d_off = nullptr;      // n_docs + 1
    uint32_t* d_df = nullptr;       // n_terms
    float* d_idf = nullptr;         // n_terms
    int ordered = -1;               // ns_docterms_aggregate: -1 not looked at yet, 1 every document's term ids ascend, 0 one does not (k_ta_order)
};

static void docterms_free_device(ns_docterms* h) {
    (void)hipFree(h->d_pairs); (void)hipFree(h->d_off); (void)hipFree(h->d_df); (void)hipFree(h->d_idf);
    h->d_pairs = nullptr; h->d_off = h->d_df = nullptr; h->d_idf = nullptr;
}
static void docterms_orphan_fwd(ns_docterms* h) { docterms_free_device(h); h->ctx = nullptr; }

extern "C" uint32_t ns_docterms_doc_cut(void) { return kMlDocCut; }

extern "C" int ns_docterms_upload(ns_ctx* ctx, const ns_forward_src* src, const uint32_t* df, const float* idf, ns_docterms** out) {
    const char* fn = "ns_docterms_upload";
    if (!ctx) return fail(nullptr, NS_E_INVAL, "%s: ctx is NULL", fn);
    if (!out) return fail(ctx, NS_E_INVAL, "%s: out is NULL", fn);
    *out = nullptr;
    if (!src) return fail(ctx, NS_E_INVAL, "%s: src is NULL", fn);
    const ns_forward_src& S = *src;
    // the structural checks and limits of ns_forward_merge (the term bytes are not needed here)
    if (S.n_pairs >= (1ull << 32) - kIvTile) return fail(ctx, NS_E_INVAL, "%s: more than %llu pairs; this build indexes pairs with 32 bits", fn, (unsigned long long)((1ull << 32) - kIvTile - 1));
    if (S.n_docs == 0xFFFFFFFFu) return fail(ctx, NS_E_INVAL, "%s: %u documents; docIds are 32 bits wide (below 2^32 - 1)", fn, S.n_docs);
    if (S.n_terms >= (1u << 31)) return fail(ctx, NS_E_INVAL, "%s: %u terms; the dictionary holds fewer than 2^31", fn, S.n_terms);
    if ((S.n_docs && !S.counts) || (S.n_pairs && !S.pairs) || (S.n_terms && (!df || !idf))) return fail(ctx, NS_E_INVAL, "%s: null array", fn);
    ns_docterms* h = new ns_docterms();
    h->doc_off.assign((size_t)S.n_docs + 1, 0u);
    uint64_t sum = 0;
    for (uint32_t j = 0; j < S.n_docs; j++) {
        sum += S.counts[j];
        if (sum > S.n_pairs) break;
        h->doc_off[j + 1] = (uint32_t)sum;
    }
    if (sum != S.n_pairs) { delete h; return fail(ctx, NS_E_INVAL, "%s: the per-document counts do not sum to n_pairs = %llu", fn, (unsigned long long)S.n_pairs); }
    h->n_docs = S.n_docs; h->n_terms = S.n_terms; h->n_pairs = (uint32_t)S.n_pairs;
    hipError_t e = hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    uint32_t* d_bad = nullptr;
    uint32_t bad = 0;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    if (e == hipSuccess) chk(hipMalloc((void**)&h->d_off, h->doc_off.size() * 4));
    if (h->n_pairs) chk(hipMalloc((void**)&h->d_pairs, (size_t)h->n_pairs * 8));
    if (h->n_terms) { chk(hipMalloc((void**)&h->d_df, (size_t)h->n_terms * 4)); chk(hipMalloc((void**)&h->d_idf, (size_t)h->n_terms * 4)); }
    chk(hipMalloc((void**)&d_bad, 4));
    if (e == hipSuccess) {
        chk(hipMemcpyAsync(h->d_off, h->doc_off.data(), h->doc_off.size() * 4, hipMemcpyHostToDevice, st));
        if (h->n_pairs) chk(hipMemcpyAsync(h->d_pairs, S.pairs, (size_t)h->n_pairs * 8, hipMemcpyHostToDevice, st));
        if (h->n_terms) {
            chk(hipMemcpyAsync(h->d_df, df, (size_t)h->n_terms * 4, hipMemcpyHostToDevice, st));
            chk(hipMemcpyAsync(h->d_idf, idf, (size_t)h->n_terms * 4, hipMemcpyHostToDevice, st));
        }
        chk(hipMemsetAsync(d_bad, 0, 4, st));
        if (e == hipSuccess && h->n_pairs) {
            hipLaunchKernelGGL(k_ml_check, dim3((h->n_pairs + 255) / 256), dim3(256), 0, st, h->d_pairs, h->n_pairs, h->n_terms, d_bad);
            chk(hipGetLastError());
        }
        chk(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    }
    if (e == hipSuccess || d_bad) { const hipError_t s2 = hipStreamSynchronize(st); chk(s2); }   // (the host arrays are the caller's: nothing may still read them)
    (void)hipFree(d_bad);
    if (e != hipSuccess || bad) {
        docterms_free_device(h);
        delete h;
        if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? NS_E_NOMEM : NS_E_HIP, "%s: %s", fn, hipGetErrorString(e));
        return fail(ctx, NS_E_INVAL, "%s: a pair names a termId >= n_terms = %u", fn, S.n_terms);
    }
    h->ctx = ctx;
    ctx->dts.push_back(h);
    *out = h;
    return NS_OK;
}

extern "C" void ns_docterms_destroy(ns_docterms* h) {
    if (!h) return;
    if (ns_ctx* ctx = h->ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        auto it = std::find(ctx->dts.begin(), ctx->dts.end(), h);
        if (it != ctx->dts.end()) ctx->dts.erase(it);
        docterms_free_device(h);
    }
    delete h;
}

extern "C" int ns_docterms_select(ns_docterms* h, const uint32_t* doc_ids, uint32_t n, uint32_t max_terms, uint32_t min_tf, uint32_t min_df,
                                  uint32_t max_df, uint32_t* term_out, float* w_out, uint32_t* count_out, float* device_ms_out) {
    const char* fn = "ns_docterms_select";
    if (!h) return fail(nullptr, NS_E_INVAL, "%s: handle is NULL", fn);
    ns_ctx* ctx = h->ctx;
    if (!ctx) return fail(nullptr, NS_E_STATE, "%s: the handle's ctx has been destroyed", fn);
    if (device_ms_out) *device_ms_out = 0.0f;
    if (n == 0) return NS_OK;
    if (!doc_ids || !term_out || !w_out || !count_out) return fail(ctx, NS_E_INVAL, "%s: null argument", fn);
    const uint32_t T = std::max(1u, std::min(max_terms, kMlMaxTerms));
    const MlRule rule{std::max(1u, min_tf), min_df, max_df};
    // the rows by size class; nothing is launched before every doc id has been checked
    std::vector<uint32_t> lists(n);
    uint32_t n_wave = 0, n_block = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t d = doc_ids[i];
        if (d >= h->n_docs) return fail(ctx, NS_E_INVAL, "%s: doc_ids[%u] = %u, the handle holds %u documents", fn, i, d, h->n_docs);
        if (h->doc_off[d + 1] - h->doc_off[d] <= kMlDocCut) lists[n_wave++] = i; else lists[n - 1 - n_block++] = i;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    CallBlock blk(ctx);
    const size_t o_ids = blk.reserve((size_t)n * 4), o_list = blk.reserve((size_t)n * 4), o_term = blk.reserve((size_t)n * T * 4), o_w = blk.reserve((size_t)n * T * 4),
                 o_cnt = blk.reserve((size_t)n * 4);
    blk.alloc(2);
    if (blk.ok()) {
        const uint32_t *d_ids = blk.at<uint32_t>(o_ids), *d_list = blk.at<uint32_t>(o_list);
        uint32_t *d_term = blk.at<uint32_t>(o_term), *d_w = blk.at<uint32_t>(o_w), *d_cnt = blk.at<uint32_t>(o_cnt);
        blk.upload(o_ids, doc_ids, (size_t)n * 4);
        blk.upload(o_list, lists.data(), (size_t)n * 4);
        blk.record(0);
        if (blk.ok() && n_wave)
            hipLaunchKernelGGL(k_ml_wave, dim3((n_wave + 3) / 4), dim3(256), 0, st, h->d_pairs, h->d_off, h->d_df, h->d_idf, d_ids, d_list, n_wave, rule, T, d_term, d_w, d_cnt);
        if (blk.ok() && n_block)
            hipLaunchKernelGGL(k_ml_block, dim3(n_block), dim3(256), 0, st, h->d_pairs, h->d_off, h->d_df, h->d_idf, d_ids, d_list + (n - n_block), rule, T, d_term, d_w, d_cnt);
        blk.launched();
        blk.record(1);
        blk.fetch(term_out, o_term, (size_t)n * T * 4);
        blk.fetch(w_out, o_w, (size_t)n * T * 4);
        blk.fetch(count_out, o_cnt, (size_t)n * 4);
        blk.sync();
        float ms = 0.0f;
        if (device_ms_out && blk.elapsed_ms(0, 1, &ms)) *device_ms_out = ms;
    }
    return blk.finish(fn);
}

// ------------------------------------------------------------------------------------------------
// Related terms: what a set of documents is about (csrc/ns_terms.hip, csrc/ns_terms_plan.hpp)
extern "C" uint32_t ns_docterms_window(void) {
#ifdef NS_VARIANTS
    if (std::getenv("NS_TERMS_WINDOW_15")) return 1u << 15;             // the A/B knob below (variants build only)
#endif
    return 1u << kTaWindowLog2;
}
extern "C" uint32_t ns_docterms_max_row_docs(void) { return kTaMaxRowDocs; }
#ifdef NS_COUNT
static unsigned long long g_ta_rows_refused = 0;   // rows over the cap (they never reach the device)
#endif

extern "C" int ns_docterms_aggregate(ns_docterms* h, const uint32_t* doc_ids, const uint64_t* row_off, uint32_t n_rows, uint32_t max_terms,
                                     uint32_t min_tf, uint32_t min_docs, uint32_t min_df, uint32_t max_df, uint32_t* term_out,
                                     uint32_t* docs_out, float* w_out, uint32_t* count_out, uint32_t* ndocs_out, float* device_ms_out) {
    const char* fn = "ns_docterms_aggregate";
    if (!h) return fail(nullptr, NS_E_INVAL, "%s: handle is NULL", fn);
    ns_ctx* ctx = h->ctx;
    if (!ctx) return fail(nullptr, NS_E_STATE, "%s: the handle's ctx has been destroyed", fn);
    if (device_ms_out) *device_ms_out = 0.0f;
    if (n_rows == 0) return NS_OK;
    if (!row_off || !term_out || !docs_out || !w_out || !count_out || !ndocs_out) return fail(ctx, NS_E_INVAL, "%s: null argument", fn);
    // nothing is launched before row_off and every doc id have been checked and every row fits the byte counters
    TermsPlan plan;
    std::string why;
    bool planned = false;
    if (row_off[0] == 0 && row_off[n_rows] != 0 && !doc_ids) why = "null argument";
    else planned = terms_plan(doc_ids, row_off, n_rows, h->doc_off.data(), h->n_docs, plan, why);
#ifdef NS_COUNT
    g_ta_rows_refused += plan.over_cap;
#endif
    if (!planned) return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    const uint32_t T = std::max(1u, std::min(max_terms, kTaMaxTerms));
    const TaRule rule{std::max(1u, min_tf), std::max(1u, min_docs), min_df, max_df};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (h->ordered < 0) {   // once per handle: do the term ids of every document ascend?
        CallBlock chk(ctx);
        const size_t o_bad = chk.reserve(4);
        chk.alloc(0);
        uint32_t bad = 0;
        if (chk.ok()) {
            chk.zero(o_bad, 4);
            if (chk.ok() && h->n_pairs > 1) hipLaunchKernelGGL(k_ta_order, dim3((h->n_pairs + 255) / 256), dim3(256), 0, st, h->d_pairs, h->n_pairs, h->d_off, h->n_docs, chk.at<uint32_t>(o_bad));
            chk.launched();
            chk.fetch(&bad, o_bad, 4);
            chk.sync();
        }
        const bool ok = chk.ok();
        const int rc = chk.finish(fn);
        if (rc != NS_OK) return rc;
        if (ok) h->ordered = bad ? 0 : 1;
    }
    if (h->ordered != 1)
        return fail(ctx, NS_E_INVAL, "%s: a document of this handle does not hold its term ids in strictly ascending order (the order ns_forward_fetch gives); the counting needs it", fn);
    const size_t n_docs_all = plan.docs.size();
    CallBlock blk(ctx);
    const size_t o_docs = blk.reserve(std::max<size_t>(n_docs_all, 1) * 4), o_first = blk.reserve(((size_t)n_rows + 1) * 4), o_order = blk.reserve((size_t)n_rows * 4),
                 o_term = blk.reserve((size_t)n_rows * T * 4), o_fg = blk.reserve((size_t)n_rows * T * 4), o_w = blk.reserve((size_t)n_rows * T * 4),
                 o_cnt = blk.reserve((size_t)n_rows * 4);
    blk.alloc(2);
    if (blk.ok()) {
        blk.upload(o_docs, plan.docs.data(), n_docs_all * 4);
        blk.upload(o_first, plan.first.data(), ((size_t)n_rows + 1) * 4);
        blk.upload(o_order, plan.order.data(), (size_t)n_rows * 4);
        blk.record(0);
        if (blk.ok()) {
            const uint32_t *d_docs = blk.at<uint32_t>(o_docs), *d_first = blk.at<uint32_t>(o_first), *d_order = blk.at<uint32_t>(o_order);
            uint32_t *d_term = blk.at<uint32_t>(o_term), *d_fg = blk.at<uint32_t>(o_fg), *d_w = blk.at<uint32_t>(o_w), *d_cnt = blk.at<uint32_t>(o_cnt);
#ifdef NS_VARIANTS
            // A/B knob (variants build only): the other window size; same rows
            if (std::getenv("NS_TERMS_WINDOW_15"))
                hipLaunchKernelGGL((k_ta_count<15>), dim3(n_rows), dim3(256), 0, st, h->d_pairs, h->d_off, h->d_df, h->d_idf, h->n_terms, d_docs, d_first, d_order, rule, T, d_term, d_fg, d_w, d_cnt);
            else
#endif
            hipLaunchKernelGGL((k_ta_count<kTaWindowLog2>), dim3(n_rows), dim3(256), 0, st, h->d_pairs, h->d_off, h->d_df, h->d_idf, h->n_terms, d_docs, d_first, d_order, rule, T, d_term, d_fg, d_w, d_cnt);
        }
        blk.launched();
        blk.record(1);
        blk.fetch(term_out, o_term, (size_t)n_rows * T * 4);
        blk.fetch(docs_out, o_fg, (size_t)n_rows * T * 4);
        blk.fetch(w_out, o_w, (size_t)n_rows * T * 4);
        blk.fetch(count_out, o_cnt, (size_t)n_rows * 4);
        blk.sync();
        float ms = 0.0f;
        if (device_ms_out && blk.elapsed_ms(0, 1, &ms)) *device_ms_out = ms;
        if (blk.ok()) for (uint32_t i = 0; i < n_rows; i++) ndocs_out[i] = plan.first[i + 1] - plan.first[i];
    }
    return blk.finish(fn);
}

// ------------------------------------------------------------------------------------------------
// What the facet, date-order and boolean entry points share above CallBlock (the host-only part of a ranked
// call's planning is csrc/ns_call_plan.hpp).  A call validates its own arguments, binds its segments (bind_segments), runs
// its planner and hands the work items to run_count or run_ranked, which own the device block.  (CallBlock itself, behind
// pool_free, also carries the indexing, merge, similar-terms, semantic and autocomplete calls.)

// A per-document table checked by a kernel at upload (ns_facet_upload, ns_dockeys_upload): n_docs values go up to a fresh
// allocation, launch_check(d_table, d_bad, grid, stream) starts the kernel that sets *d_bad for a value the call refuses.
// On an error or a refused value nothing stays allocated and *d_out is NULL.
template <class T, class Check>
static hipError_t upload_checked(ns_ctx* ctx, const T* src, uint32_t n_docs, T** d_out, bool* refused, Check launch_check) {
    hipStream_t st = ctx->stream;
    uint32_t* d_bad = nullptr;
    uint32_t bad = 0;
    hipError_t e = hipSetDevice(ctx->device);
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    if (e == hipSuccess) chk(hipMalloc((void**)d_out, (size_t)std::max<uint32_t>(n_docs, 1) * sizeof(T)));
    chk(hipMalloc((void**)&d_bad, 4));
    if (e == hipSuccess) {
        if (n_docs) chk(hipMemcpyAsync(*d_out, src, (size_t)n_docs * sizeof(T), hipMemcpyHostToDevice, st));
        chk(hipMemsetAsync(d_bad, 0, 4, st));
        if (e == hipSuccess && n_docs) {
            launch_check(*d_out, d_bad, dim3(std::min<uint32_t>((n_docs + 255) / 256, 1024u)), st);
            chk(hipGetLastError());
        }
        chk(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    }
    { const hipError_t s2 = hipStreamSynchronize(st); chk(s2); }   // (the host array is the caller's: nothing may still read it)
    (void)hipFree(d_bad);
    if (e != hipSuccess || bad) { (void)hipFree(*d_out); *d_out = nullptr; }
    *refused = bad != 0;
    return e;
}

// The listed segments of a call -> what its planner (views) and its kernels (dsegs) know of them.  `tables` is the call's
// companion table per segment and `noun` its name in the messages; Table = void and both NULL for a call without one.
// per_seg(i, s, t) is the caller's part: it checks the table (a code other than NS_OK, with the message set, ends the call)
// and fills what the call adds per segment.
template <class Table, class PerSeg>
static int bind_segments(ns_ctx* ctx, const char* fn, const uint32_t* seg_ids, ns_seg* const* segs, Table* const* tables, const char* noun,
                         uint32_t n_segs, std::vector<FcSegView>& views, std::vector<DevFcSeg>& dsegs, PerSeg per_seg) {
    if (!seg_ids || !segs || (noun && !tables)) return fail(ctx, NS_E_INVAL, "%s: null segment arrays", fn);
    views.assign(n_segs, FcSegView());
    dsegs.assign(n_segs, DevFcSeg());
    for (uint32_t i = 0; i < n_segs; i++) {
        ns_seg* s = segs[i];
        const Table* t = tables ? tables[i] : nullptr;
        if (noun && (!s || !t)) return fail(ctx, NS_E_INVAL, "%s: segment or %s %u is NULL", fn, noun, i);
        if (!s) return fail(ctx, NS_E_INVAL, "%s: segment %u is NULL", fn, i);
        if (s->ctx != ctx || s->pending || s->id >= ctx->segs.size() || ctx->segs[s->id] != s) return fail(ctx, NS_E_INVAL, "%s: segment %u is not a published segment of this ctx", fn, i);
        views[i].seg_id = seg_ids[i];
        views[i].n_docs = s->n_docs;
        views[i].n_postings = s->n_postings;
        if (s->d_skips && !s->lists.skip.empty()) views[i].skip_of = [s](uint32_t first, uint32_t count) { return s->lists.skip_of(first, count); };
        dsegs[i] = DevFcSeg{s->d_postings, s->d_skips, nullptr, s->n_docs, 0u};
        const int rc = per_seg(i, s, t);
        if (rc != NS_OK) return rc;
    }
    return NS_OK;
}

// Grouped clauses: clauses without roles name no MUST ref, so nothing reads them: the sibling's plan and
// kernels, as for clauses == NULL.
static const uint16_t* bq_live_clauses(const uint16_t* clauses, uint32_t n_terms, const uint8_t* roles) {
    return (clauses && n_terms && !roles) ? nullptr : clauses;
}

// At-least-m-of-n clauses: needs belong to clauses; without live clauses nothing reads them.  False (with `why`):
// needs were given without clauses.
static bool bq_live_needs(const uint16_t* given_clauses, const uint16_t* live_clauses, const uint8_t*& needs, std::string& why) {
    if (needs && !given_clauses) { why = "needs without clauses: a need belongs to a clause"; return false; }
    if (!live_clauses) needs = nullptr;
    return true;
}

// Counter planes of a quorum launch: what its largest need asks for.  Test builds may force three (NS_QUORUM_PLANES=3: the price of
// the LDS alone, tools/quorum_bench.py).
static uint32_t bq_launch_planes(uint32_t max_need) {
    uint32_t planes = bq_need_planes(max_need);
#if defined(NS_VARIANTS) || defined(NS_COUNT)
    if (const char* t = std::getenv("NS_QUORUM_PLANES")) { if (planes && std::atol(t) == 3) planes = 3; }
#endif
    return planes;
}

// The facet-count calls from their work items on: one kernel over the items adds to counts[q * B + b], found = the sum of a
// query's buckets.  time_memset: whether the interval device_ms_out reports starts before the memset of the counts
// (ns_facet_count) or after it (the boolean and grouped counts); ms_acc (may be NULL) also gets the interval.
template <class Ref>
static int run_count(ns_ctx* ctx, const char* fn, const std::vector<FcItem>& items, const std::vector<Ref>& refs, const std::vector<DevFcSeg>& dsegs,
                     void (*kernel)(const FcItem*, const Ref*, const DevFcSeg*, uint32_t, uint32_t*), uint32_t n_queries, uint32_t B,
                     bool time_memset, float* ms_acc, uint32_t* counts_out, uint64_t* found_out, float* device_ms_out, size_t lds = 0) {
    std::string why;
    if (!call_item_limit(items.size(), why)) return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    const size_t n_counts = (size_t)n_queries * B;
    if (!items.empty()) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        CallBlock blk(ctx);
        if (lds) blk.chk(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // (the quorum planes)
        const size_t o_items = blk.reserve(items.size() * sizeof(FcItem)), o_refs = blk.reserve(refs.size() * sizeof(Ref)),
                     o_segs = blk.reserve(dsegs.size() * sizeof(DevFcSeg)), o_counts = blk.reserve(n_counts * 4);
        blk.alloc(2);
        if (blk.ok()) {
            blk.upload(o_items, items.data(), items.size() * sizeof(FcItem));
            blk.upload(o_refs, refs.data(), refs.size() * sizeof(Ref));
            blk.upload(o_segs, dsegs.data(), dsegs.size() * sizeof(DevFcSeg));
            if (time_memset) blk.record(0);
            blk.zero(o_counts, n_counts * 4);
            if (!time_memset) blk.record(0);
            if (blk.ok()) {
                hipLaunchKernelGGL(kernel, dim3((uint32_t)items.size()), dim3(256), lds, blk.st, blk.at<const FcItem>(o_items), blk.at<const Ref>(o_refs),
                                   blk.at<const DevFcSeg>(o_segs), B, blk.at<uint32_t>(o_counts));
                blk.launched();
            }
            blk.record(1);
            blk.fetch(counts_out, o_counts, n_counts * 4);
            blk.sync();
            float ms = 0.0f;
            if (blk.elapsed_ms(0, 1, &ms)) {
                if (ms_acc) *ms_acc += ms;
                if (device_ms_out) *device_ms_out = ms;
            }
        }
        const int rc = blk.finish(fn);
        if (rc != NS_OK) return rc;
    } else {
        std::memset(counts_out, 0, n_counts * 4);
    }
    if (found_out)
        for (uint32_t q = 0; q < n_queries; q++) {
            uint64_t sum = 0;
            for (uint32_t b = 0; b < B; b++) sum += counts_out[(size_t)q * B + b];
            found_out[q] = sum;
        }
    return NS_OK;
}

// k_sd_select, k_bq_select and k_bs_select: (items, refs, segs, aux, K, asc or window, cand, found, last, rest)
template <class Ref, class Aux>
using SelectKernel = void (*)(const FcItem*, const Ref*, const DevFcSeg*, const Aux*, uint32_t, uint32_t, uint64_t*, unsigned long long*, const uint64_t*,
                              unsigned long long*);

// The regions of a ranked call's block as its kernels take them.
template <class Ref, class Aux>
struct RankedDev {
    const FcItem* items;
    const Ref* refs;
    const DevFcSeg* segs;
    const Aux* aux;               // DevSdSeg (date order) or DevBqSeg (ranked by score) per segment
    const uint32_t* q_off;
    const ns_query_desc* qd;      // qd, terms, roles, keys, pos: of the calls with a score stage only
    const ns_term_ref* terms;
    const uint8_t* roles;         // NULL: the call has none
    uint32_t *hits, *keys, *pos, *nhits;
    const uint64_t* cand;
};

// A ranked call from its plan on.  Per cut: the select kernel over the cut's items fills their candidate rows, join(dev, cut)
// launches the kernel that joins them into the queries' rows, and score(dev, cut), in the calls ordered by date, the one
// that looks the hits' scores up; `stages` = 2 or 3 says which, and ms_acc[stage] and device_ms_out get the kernels' times.
template <class Ref, class Aux>
struct RankedCall {
    const std::vector<FcItem>& items;
    const std::vector<Ref>& refs;
    const std::vector<DevFcSeg>& dsegs;
    const std::vector<Aux>& aux;
    const RankedPlan& plan;
    uint32_t n_queries;
    // the select stage: the instantiation (the AFTER = false ones get NULL for last and rest), its scalar after K (asc, or
    // the window) and its dynamic LDS
    SelectKernel<Ref, Aux> select;
    uint32_t select_arg;
    size_t select_lds;
    int stages;
    float* ms_acc;
    // what the score stage reads (stages == 3); roles_region: the block has a region for the roles, used or not
    const ns_query_desc* queries;
    const ns_term_ref* terms;
    uint32_t n_terms;
    const uint8_t* roles;
    bool roles_region;
    hipError_t before;            // the first error of what the caller did on the device before the block
    ns_hit* hits_out;
    uint32_t* keys_out;           // with stages == 3
    uint32_t* nhits_out;
    uint64_t *found_out, *rest_out;
    float* device_ms_out;
};

template <class Ref, class Aux, class Join, class Score>
static int run_ranked(ns_ctx* ctx, const char* fn, const RankedCall<Ref, Aux>& c, Join join, Score score) {
    const RankedPlan& p = c.plan;
    const bool scored = c.stages == 3;
    const uint32_t K = p.K, n_queries = c.n_queries;
    const size_t n_out = (size_t)n_queries * K, n_roles = c.roles ? (size_t)c.n_terms : 0;
    const size_t per_cut = (size_t)c.stages + 1;
    CallBlock blk(ctx);
    blk.chk(c.before);
    const size_t o_last = blk.reserve(p.last.size() * 8), o_rest = blk.reserve(p.paged ? (size_t)n_queries * 8 : 0);
    const size_t o_items = blk.reserve(c.items.size() * sizeof(FcItem)), o_refs = blk.reserve(c.refs.size() * sizeof(Ref)),
                 o_segs = blk.reserve(c.dsegs.size() * sizeof(DevFcSeg)), o_aux = blk.reserve(c.aux.size() * sizeof(Aux)),
                 o_qoff = blk.reserve(p.q_off.size() * 4);
    const size_t o_qd = scored ? blk.reserve((size_t)n_queries * sizeof(ns_query_desc)) : 0,
                 o_terms = scored ? blk.reserve((size_t)c.n_terms * sizeof(ns_term_ref)) : 0, o_roles = c.roles_region ? blk.reserve(n_roles) : 0;
    const size_t o_hits = blk.reserve(n_out * sizeof(ns_hit)), o_keys = scored ? blk.reserve(n_out * 4) : 0, o_pos = scored ? blk.reserve(n_out * 4) : 0,
                 o_nhits = blk.reserve((size_t)n_queries * 4), o_found = blk.reserve((size_t)n_queries * 8),
                 o_cand = blk.reserve((size_t)p.cand_rows * K * 8);   // <= kSdCandBytes
    blk.alloc(p.cuts.size() * per_cut);
    if (blk.ok()) {
        blk.upload(o_items, c.items.data(), c.items.size() * sizeof(FcItem));
        blk.upload(o_refs, c.refs.data(), c.refs.size() * sizeof(Ref));
        blk.upload(o_segs, c.dsegs.data(), c.dsegs.size() * sizeof(DevFcSeg));
        blk.upload(o_aux, c.aux.data(), c.aux.size() * sizeof(Aux));
        blk.upload(o_qoff, p.q_off.data(), p.q_off.size() * 4);
        if (scored) {
            blk.upload(o_qd, c.queries, (size_t)n_queries * sizeof(ns_query_desc));
            blk.upload(o_terms, c.terms, (size_t)c.n_terms * sizeof(ns_term_ref));
            blk.upload(o_roles, c.roles, n_roles);
        }
        blk.zero(o_found, (size_t)n_queries * 8);
        blk.upload(o_last, p.last.data(), p.last.size() * 8);
        if (p.paged) blk.zero(o_rest, (size_t)n_queries * 8);
        const uint64_t* d_last = blk.at<const uint64_t>(o_last);
        uint64_t* d_cand = blk.at<uint64_t>(o_cand);
        const RankedDev<Ref, Aux> dev{blk.at<const FcItem>(o_items), blk.at<const Ref>(o_refs), blk.at<const DevFcSeg>(o_segs), blk.at<const Aux>(o_aux),
                                      blk.at<const uint32_t>(o_qoff), blk.at<const ns_query_desc>(o_qd), blk.at<const ns_term_ref>(o_terms),
                                      n_roles ? blk.at<const uint8_t>(o_roles) : nullptr, blk.at<uint32_t>(o_hits), blk.at<uint32_t>(o_keys),
                                      blk.at<uint32_t>(o_pos), blk.at<uint32_t>(o_nhits), d_cand};
        for (size_t i = 0; i < p.cuts.size() && blk.ok(); i++) {
            const SdBatch& b = p.cuts[i];
            const uint32_t n_it = b.item_end - b.item_begin;
            blk.record(i * per_cut + 0);
            if (n_it) {   // last is indexed by the call's item number, as items: both start at the sub-batch's first
                hipLaunchKernelGGL(c.select, dim3(n_it), dim3(256), c.select_lds, blk.st, dev.items + b.item_begin, dev.refs, dev.segs, dev.aux, K, c.select_arg,
                                   d_cand, blk.at<unsigned long long>(o_found), p.paged ? d_last + b.item_begin : (const uint64_t*)nullptr,
                                   p.paged ? blk.at<unsigned long long>(o_rest) : (unsigned long long*)nullptr);
                blk.launched();
            }
            blk.record(i * per_cut + 1);
            join(dev, b, blk.st);
            blk.launched();
            blk.record(i * per_cut + 2);
            if (scored) {
                score(dev, b, blk.st);
                blk.launched();
                blk.record(i * per_cut + 3);
            }
        }
        blk.fetch(c.hits_out, o_hits, n_out * sizeof(ns_hit));
        if (scored) blk.fetch(c.keys_out, o_keys, n_out * 4);
        blk.fetch(c.nhits_out, o_nhits, (size_t)n_queries * 4);
        if (c.found_out) blk.fetch(c.found_out, o_found, (size_t)n_queries * 8);
        if (c.rest_out) blk.fetch(c.rest_out, p.paged ? o_rest : o_found, (size_t)n_queries * 8);   // no cursor: rest = found
        blk.sync();
        if (blk.ok()) {
            float sum = 0.0f;
            for (size_t i = 0; i < p.cuts.size(); i++)
                for (int j = 0; j < c.stages; j++) {
                    float ms = 0.0f;
                    if (blk.elapsed_ms(i * per_cut + j, i * per_cut + j + 1, &ms)) { c.ms_acc[j] += ms; sum += ms; }
                }
            if (c.device_ms_out) *c.device_ms_out = sum;
        }
    }
    return blk.finish(fn);
}

// ------------------------------------------------------------------------------------------------
// Facet counts (csrc/ns_facet.hip, csrc/ns_facet_plan.hpp)
struct ns_facet {
    ns_ctx* ctx = nullptr;
    uint32_t n_docs = 0, n_buckets = 0;
    uint16_t* d_buckets = nullptr;
};

extern "C" uint32_t ns_facet_tile_docs(void) {
#if defined(NS_VARIANTS) || defined(NS_COUNT)
    // test knob (variants and counting builds only): small tiles, so that a few hundred documents span several
    if (const char* t = std::getenv("NS_FACET_TILE_DOCS")) { const long v = std::atol(t); if (v > 0 && v <= (long)kFcTileDocs && fc_tile_ok((uint32_t)v)) return (uint32_t)v; }
#endif
    return kFcTileDocs;
}

extern "C" int ns_facet_upload(ns_ctx* ctx, uint32_t n_docs, const uint16_t* bucket_of_doc, uint32_t n_buckets, ns_facet** out) {
    const char* fn = "ns_facet_upload";
    if (!ctx) return fail(nullptr, NS_E_INVAL, "%s: ctx is NULL", fn);
    if (!out) return fail(ctx, NS_E_INVAL, "%s: out is NULL", fn);
    *out = nullptr;
    if (n_docs && !bucket_of_doc) return fail(ctx, NS_E_INVAL, "%s: bucket_of_doc is NULL", fn);
    if (n_buckets < 1 || n_buckets > kFcMaxBuckets) return fail(ctx, NS_E_INVAL, "%s: n_buckets = %u outside [1, %u]", fn, n_buckets, kFcMaxBuckets);
    ns_facet* t = new ns_facet();
    t->ctx = ctx; t->n_docs = n_docs; t->n_buckets = n_buckets;
    bool refused = false;
    const hipError_t e = upload_checked(ctx, bucket_of_doc, n_docs, &t->d_buckets, &refused, [&](const uint16_t* d_table, uint32_t* d_bad, dim3 grid, hipStream_t st) {
        hipLaunchKernelGGL(k_fc_check, grid, dim3(256), 0, st, d_table, n_docs, n_buckets, d_bad);
    });
    if (e != hipSuccess || refused) {
        delete t;
        if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? NS_E_NOMEM : NS_E_HIP, "%s: %s", fn, hipGetErrorString(e));
        return fail(ctx, NS_E_INVAL, "%s: a document has a bucket id >= n_buckets = %u", fn, n_buckets);
    }
    *out = t;
    return NS_OK;
}

extern "C" int ns_facet_release(ns_ctx* ctx, ns_facet* table) {
    if (!ctx || !table || table->ctx != ctx) return fail(ctx, NS_E_INVAL, "ns_facet_release: table does not belong to this ctx");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(table->d_buckets);
    delete table;
    return NS_OK;
}

// The facet calls' part of bind_segments: the table buckets the segment's documents, as many buckets as table 0; the
// kernels read it through the segment's DevFcSeg.
static int fc_bind_table(ns_ctx* ctx, const char* fn, uint32_t i, const ns_seg* s, const ns_facet* t, const ns_facet* t0, DevFcSeg& dseg) {
    if (t->ctx != ctx) return fail(ctx, NS_E_INVAL, "%s: table %u does not belong to this ctx", fn, i);
    if (t->n_docs != s->n_docs) return fail(ctx, NS_E_INVAL, "%s: table %u buckets %u documents, its segment has %u", fn, i, t->n_docs, s->n_docs);
    if (t->n_buckets != t0->n_buckets) return fail(ctx, NS_E_INVAL, "%s: table %u has %u buckets, table 0 has %u", fn, i, t->n_buckets, t0->n_buckets);
    dseg.buckets = t->d_buckets;
    return NS_OK;
}

extern "C" int ns_facet_count(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, uint32_t n_terms,
                              uint32_t flags, const uint32_t* seg_ids, ns_seg* const* segs, ns_facet* const* tables, uint32_t n_segs,
                              uint32_t* counts_out, uint64_t* found_out, float* device_ms_out) {
    const char* fn = "ns_facet_count";
    if (!ctx) return fail(nullptr, NS_E_INVAL, "%s: ctx is NULL", fn);
    if (device_ms_out) *device_ms_out = 0.0f;
    if (n_queries == 0) return NS_OK;
    if (!queries || !counts_out || (n_terms && !terms)) return fail(ctx, NS_E_INVAL, "%s: null argument", fn);
    if (!n_segs) return fail(ctx, NS_E_INVAL, "%s: no segment listed (the number of buckets comes from the tables)", fn);
    std::vector<FcSegView> views;
    std::vector<DevFcSeg> dsegs;
    const int rc = bind_segments(ctx, fn, seg_ids, segs, tables, "table", n_segs, views, dsegs,
                                 [&](uint32_t i, const ns_seg* s, const ns_facet* t) { return fc_bind_table(ctx, fn, i, s, t, tables[0], dsegs[i]); });
    if (rc != NS_OK) return rc;
    const bool and_mode = (flags & NS_FLAG_AND) != 0;
    std::vector<FcRef> refs;
    std::vector<FcItem> items;
    std::string why;
    if (fc_plan(queries, n_queries, terms, n_terms, and_mode, views.data(), n_segs, ns_facet_tile_docs(), refs, items, why) != NS_OK)
        return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    return run_count(ctx, fn, items, refs, dsegs, and_mode ? k_fc_count<true> : k_fc_count<false>, n_queries, tables[0]->n_buckets, true, nullptr,
                     counts_out, found_out, device_ms_out);
}

// ------------------------------------------------------------------------------------------------
// Search sorted by a per-document key (csrc/ns_sorted.hip, csrc/ns_sorted_plan.hpp)
struct ns_dockeys {
    ns_ctx* ctx = nullptr;
    uint32_t n_docs = 0;
    uint32_t* d_keys = nullptr;
};
static thread_local float g_sd_ms[3] = {0.0f, 0.0f, 0.0f};   // k_sd_select, k_sd_join, k_sd_score: summed over the thread's ns_search_sorted calls (ns_sorted_kernel_ms)

extern "C" int ns_dockeys_upload(ns_ctx* ctx, uint32_t n_docs, const uint32_t* keys, ns_dockeys** out) {
    const char* fn = "ns_dockeys_upload";
    if (!ctx) return fail(nullptr, NS_E_INVAL, "%s: ctx is NULL", fn);
    if (!out) return fail(ctx, NS_E_INVAL, "%s: out is NULL", fn);
    *out = nullptr;
    if (n_docs && !keys) return fail(ctx, NS_E_INVAL, "%s: keys is NULL", fn);
    ns_dockeys* t = new ns_dockeys();
    t->ctx = ctx; t->n_docs = n_docs;
    bool refused = false;
    const hipError_t e = upload_checked(ctx, keys, n_docs, &t->d_keys, &refused, [&](const uint32_t* d_table, uint32_t* d_bad, dim3 grid, hipStream_t st) {
        hipLaunchKernelGGL(k_sd_check, grid, dim3(256), 0, st, d_table, n_docs, d_bad);
    });
    if (e != hipSuccess || refused) {
        delete t;
        if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? NS_E_NOMEM : NS_E_HIP, "%s: %s", fn, hipGetErrorString(e));
        return fail(ctx, NS_E_INVAL, "%s: a document has the reserved key 0xFFFFFFFF", fn);
    }
    *out = t;
    return NS_OK;
}

extern "C" int ns_dockeys_release(ns_ctx* ctx, ns_dockeys* table) {
    if (!ctx || !table || table->ctx != ctx) return fail(ctx, NS_E_INVAL, "ns_dockeys_release: table does not belong to this ctx");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(table->d_keys);
    delete table;
    return NS_OK;
}

static int sd_search(ns_ctx* ctx, const char* fn, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, uint32_t n_terms,
                     uint32_t k, uint32_t flags, const ns_cursor* after, const uint32_t* seg_ids, ns_seg* const* segs, ns_dockeys* const* keys,
                     uint32_t n_segs, ns_hit* hits_out, uint32_t* keys_out, uint32_t* nhits_out, uint64_t* found_out, uint64_t* rest_out,
                     float* device_ms_out);

extern "C" int ns_sorted_kernel_ms(float* out3, int reset) {
    if (!out3) return NS_E_INVAL;
    for (int i = 0; i < 3; i++) out3[i] = g_sd_ms[i];
    if (reset) g_sd_ms[0] = g_sd_ms[1] = g_sd_ms[2] = 0.0f;
    return NS_OK;
}

// (Pages past the first K, DESIGN.md §5s: ranked_call_plan of csrc/ns_call_plan.hpp turns the cursors of a call into last[item].)
extern "C" int ns_search_sorted(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, uint32_t n_terms,
                                uint32_t k, uint32_t flags, const uint32_t* seg_ids, ns_seg* const* segs, ns_dockeys* const* keys, uint32_t n_segs,
                                ns_hit* hits_out, uint32_t* keys_out, uint32_t* nhits_out, uint64_t* found_out, float* device_ms_out) {
    return sd_search(ctx, "ns_search_sorted", queries, n_queries, terms, n_terms, k, flags, nullptr, seg_ids, segs, keys, n_segs, hits_out, keys_out, nhits_out,
                     found_out, nullptr, device_ms_out);
}

extern "C" int ns_search_sorted_after(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, uint32_t n_terms,
                                      uint32_t k, uint32_t flags, const ns_cursor* after, const uint32_t* seg_ids, ns_seg* const* segs,
                                      ns_dockeys* const* keys, uint32_t n_segs, ns_hit* hits_out, uint32_t* keys_out, uint32_t* nhits_out,
                                      uint64_t* found_out, uint64_t* rest_out, float* device_ms_out) {
    return sd_search(ctx, "ns_search_sorted_after", queries, n_queries, terms, n_terms, k, flags, after, seg_ids, segs, keys, n_segs, hits_out, keys_out,
                     nhits_out, found_out, rest_out, device_ms_out);
}

// The date-ordered calls' part of bind_segments (ns_search_sorted*, ns_search_sorted_boolean, ns_search_sorted_grouped): the
// table keys the segment's documents; the kernels read it, the norms and the segment's id through a DevSdSeg.
static int sd_bind_table(ns_ctx* ctx, const char* fn, uint32_t i, const ns_seg* s, const ns_dockeys* t, uint32_t seg_id, DevSdSeg& sd) {
    if (t->ctx != ctx) return fail(ctx, NS_E_INVAL, "%s: key table %u does not belong to this ctx", fn, i);
    if (t->n_docs != s->n_docs) return fail(ctx, NS_E_INVAL, "%s: key table %u keys %u documents, its segment has %u", fn, i, t->n_docs, s->n_docs);
    sd = DevSdSeg{t->d_keys, s->d_norm, seg_id, 0u};
    return NS_OK;
}

// the join stage of the date-ordered calls
template <class Ref>
static void sd_launch_join(const RankedDev<Ref, DevSdSeg>& d, const SdBatch& b, uint32_t K, uint32_t asc, hipStream_t st) {
    hipLaunchKernelGGL(k_sd_join, dim3((b.q_end - b.q_begin + 3) / 4), dim3(256), 0, st, d.items, d.q_off, b.q_begin, b.q_end, b.item_begin, d.aux, d.cand, K, asc,
                       d.hits, d.keys, d.pos, d.nhits);
}
// a score stage has one wave per hit of the cut's queries, four to a block
static dim3 sd_score_grid(const SdBatch& b, uint32_t K) { return dim3((uint32_t)(((uint64_t)(b.q_end - b.q_begin) * K + 3) / 4)); }

static int sd_search(ns_ctx* ctx, const char* fn, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, uint32_t n_terms,
                     uint32_t k, uint32_t flags, const ns_cursor* after, const uint32_t* seg_ids, ns_seg* const* segs, ns_dockeys* const* keys,
                     uint32_t n_segs, ns_hit* hits_out, uint32_t* keys_out, uint32_t* nhits_out, uint64_t* found_out, uint64_t* rest_out,
                     float* device_ms_out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "%s: ctx is NULL", fn);
    if (device_ms_out) *device_ms_out = 0.0f;
    if (n_queries == 0) return NS_OK;
    if (!queries || !hits_out || !keys_out || !nhits_out || (n_terms && !terms)) return fail(ctx, NS_E_INVAL, "%s: null argument", fn);
    if (flags & ~(NS_FLAG_AND | NS_SORT_ASC)) return fail(ctx, NS_E_INVAL, "%s: flags 0x%x: only NS_FLAG_AND and NS_SORT_ASC are known", fn, flags);
    if (!n_segs) return fail(ctx, NS_E_INVAL, "%s: no segment listed", fn);
    std::vector<FcSegView> views;
    std::vector<DevFcSeg> dsegs;
    std::vector<DevSdSeg> sds(n_segs);
    const int rc = bind_segments(ctx, fn, seg_ids, segs, keys, "key table", n_segs, views, dsegs,
                                 [&](uint32_t i, const ns_seg* s, const ns_dockeys* t) { return sd_bind_table(ctx, fn, i, s, t, seg_ids[i], sds[i]); });
    if (rc != NS_OK) return rc;
    const bool and_mode = (flags & NS_FLAG_AND) != 0;
    const uint32_t asc = (flags & NS_SORT_ASC) ? 1u : 0u;
    std::vector<FcRef> refs;
    std::vector<FcItem> items;
    RankedPlan plan;
    std::string why;
    if (fc_plan(queries, n_queries, terms, n_terms, and_mode, views.data(), n_segs, ns_facet_tile_docs(), refs, items, why) != NS_OK)
        return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    if (!ranked_call_plan(items, n_queries, k, after, views, [asc](uint32_t key) { return after_sort_rank(key, asc != 0u); }, true, kSdCandBytes, plan, why))
        return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    HIPCHK(ctx, hipSetDevice(ctx->device));
    static const SelectKernel<FcRef, DevSdSeg> kSelect[2][2] = {{k_sd_select<false, false>, k_sd_select<false, true>},
                                                                {k_sd_select<true, false>, k_sd_select<true, true>}};   // [and][paged]
    const uint32_t K = plan.K;
    RankedCall<FcRef, DevSdSeg> c{items, refs, dsegs, sds, plan, n_queries};
    c.select = kSelect[and_mode][plan.paged];
    c.select_arg = asc;
    c.stages = 3;
    c.ms_acc = g_sd_ms;
    c.queries = queries; c.terms = terms; c.n_terms = n_terms;
    c.hits_out = hits_out; c.keys_out = keys_out; c.nhits_out = nhits_out; c.found_out = found_out; c.rest_out = rest_out; c.device_ms_out = device_ms_out;
    return run_ranked(ctx, fn, c, [=](const RankedDev<FcRef, DevSdSeg>& d, const SdBatch& b, hipStream_t st) { sd_launch_join(d, b, K, asc, st); },
                      [=](const RankedDev<FcRef, DevSdSeg>& d, const SdBatch& b, hipStream_t st) {
                          hipLaunchKernelGGL(k_sd_score, sd_score_grid(b, K), dim3(256), 0, st, d.qd, d.terms, b.q_begin, b.q_end, d.segs, d.aux, K, d.pos, d.nhits, d.hits);
                      });
}

// ------------------------------------------------------------------------------------------------
// Boolean queries (csrc/ns_boolean.hip, csrc/ns_boolean_plan.hpp)
static thread_local float g_bq_ms[2] = {0.0f, 0.0f};   // k_bq_select, k_bq_join: summed over the thread's ns_search_boolean calls (ns_boolean_kernel_ms)

// documents per window of k_bq_select: never more than the tile
static uint32_t bq_win_docs(uint32_t tile_docs) {
    uint32_t win = kBqWinDocs;
#if defined(NS_VARIANTS) || defined(NS_COUNT)
    // test knob (variants and counting builds only), next to NS_FACET_TILE_DOCS: small windows, so that a few hundred documents span several
    if (const char* t = std::getenv("NS_BOOL_WIN_DOCS")) { const long v = std::atol(t); if (v > 0 && v <= (long)kBqMaxWinDocs && bq_win_ok((uint32_t)v)) win = (uint32_t)v; }
#endif
    return std::min(win, tile_docs);
}

extern "C" int ns_boolean_kernel_ms(float* out2, int reset) {
    if (!out2) return NS_E_INVAL;
    for (int i = 0; i < 2; i++) out2[i] = g_bq_ms[i];
    if (reset) g_bq_ms[0] = g_bq_ms[1] = 0.0f;
    return NS_OK;
}

struct ns_docboost;
static int bq_search(ns_ctx* ctx, const char* fn, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                     const uint16_t* clauses, const uint8_t* needs, uint32_t n_terms, uint32_t k, const ns_cursor* after, const uint32_t* seg_ids, ns_seg* const* segs, uint32_t n_segs, ns_hit* hits_out,
                     uint32_t* nhits_out, uint64_t* found_out, uint64_t* rest_out, float* device_ms_out, ns_docboost* const* boosts = nullptr);

extern "C" int ns_search_boolean(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                                 uint32_t n_terms, uint32_t k, const uint32_t* seg_ids, ns_seg* const* segs, uint32_t n_segs, ns_hit* hits_out,
                                 uint32_t* nhits_out, uint64_t* found_out, float* device_ms_out) {
    return bq_search(ctx, "ns_search_boolean", queries, n_queries, terms, roles, nullptr, nullptr, n_terms, k, nullptr, seg_ids, segs, n_segs, hits_out, nhits_out, found_out,
                     nullptr, device_ms_out);
}

extern "C" int ns_search_boolean_after(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                                       uint32_t n_terms, uint32_t k, const ns_cursor* after, const uint32_t* seg_ids, ns_seg* const* segs,
                                       uint32_t n_segs, ns_hit* hits_out, uint32_t* nhits_out, uint64_t* found_out, uint64_t* rest_out,
                                       float* device_ms_out) {
    return bq_search(ctx, "ns_search_boolean_after", queries, n_queries, terms, roles, nullptr, nullptr, n_terms, k, after, seg_ids, segs, n_segs, hits_out, nhits_out,
                     found_out, rest_out, device_ms_out);
}

// Grouped clauses: clauses == NULL is the sibling, plan and kernels; otherwise bq_plan_grouped and the GROUPED
// instantiations of the same kernels.  The joins and the score lookup are the siblings'.
static thread_local float g_gq_ms[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // of the calls with clauses: k_bq_select, k_bq_join, k_bs_count, k_bs_select, k_sd_join, k_bs_score (ns_grouped_kernel_ms)

extern "C" int ns_grouped_kernel_ms(float* out6, int reset) {
    if (!out6) return NS_E_INVAL;
    for (int i = 0; i < 6; i++) out6[i] = g_gq_ms[i];
    if (reset) for (int i = 0; i < 6; i++) g_gq_ms[i] = 0.0f;
    return NS_OK;
}

extern "C" int ns_search_grouped_after(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                                       const uint16_t* clauses, uint32_t n_terms, uint32_t k, const ns_cursor* after, const uint32_t* seg_ids,
                                       ns_seg* const* segs, uint32_t n_segs, ns_hit* hits_out, uint32_t* nhits_out, uint64_t* found_out,
                                       uint64_t* rest_out, float* device_ms_out) {
    return bq_search(ctx, "ns_search_grouped_after", queries, n_queries, terms, roles, clauses, nullptr, n_terms, k, after, seg_ids, segs, n_segs, hits_out, nhits_out,
                     found_out, rest_out, device_ms_out);
}

// At-least-m-of-n clauses: needs == NULL is the grouped sibling, plan and kernels; otherwise bq_plan_quorum and the
// QUORUM instantiations of the same kernels, with counter planes in dynamic LDS when a need of the launch is above 1.
static thread_local float g_qq_ms[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // of the calls with needs: k_bq_select, k_bq_join, k_bs_count, k_bs_select, k_sd_join, k_bs_score (ns_quorum_kernel_ms)

extern "C" int ns_quorum_kernel_ms(float* out6, int reset) {
    if (!out6) return NS_E_INVAL;
    for (int i = 0; i < 6; i++) out6[i] = g_qq_ms[i];
    if (reset) for (int i = 0; i < 6; i++) g_qq_ms[i] = 0.0f;
    return NS_OK;
}

extern "C" int ns_search_quorum_after(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                                      const uint16_t* clauses, const uint8_t* needs, uint32_t n_terms, uint32_t k, const ns_cursor* after,
                                      const uint32_t* seg_ids, ns_seg* const* segs, uint32_t n_segs, ns_hit* hits_out, uint32_t* nhits_out,
                                      uint64_t* found_out, uint64_t* rest_out, float* device_ms_out) {
    return bq_search(ctx, "ns_search_quorum_after", queries, n_queries, terms, roles, clauses, needs, n_terms, k, after, seg_ids, segs, n_segs, hits_out, nhits_out,
                     found_out, rest_out, device_ms_out);
}

// Per-document boost factors (csrc/ns_boolean.hip k_bq_select<true, ., ., true>)
struct ns_docboost {
    ns_ctx* ctx = nullptr;
    uint32_t n_docs = 0;
    float* d_boost = nullptr;
};
static thread_local float g_bb_ms[2] = {0.0f, 0.0f};   // k_bq_select, k_bq_join: summed over the thread's ns_search_boosted_after calls with tables (ns_boosted_kernel_ms)

extern "C" int ns_docboost_upload(ns_ctx* ctx, uint32_t n_docs, const float* boost, ns_docboost** out) {
    const char* fn = "ns_docboost_upload";
    if (!ctx) return fail(nullptr, NS_E_INVAL, "%s: ctx is NULL", fn);
    if (!out) return fail(ctx, NS_E_INVAL, "%s: out is NULL", fn);
    *out = nullptr;
    if (n_docs && !boost) return fail(ctx, NS_E_INVAL, "%s: boost is NULL", fn);
    ns_docboost* t = new ns_docboost();
    t->ctx = ctx; t->n_docs = n_docs;
    bool refused = false;
    const hipError_t e = upload_checked(ctx, boost, n_docs, &t->d_boost, &refused, [&](const float* d_table, uint32_t* d_bad, dim3 grid, hipStream_t st) {
        hipLaunchKernelGGL(k_bq_boost_check, grid, dim3(256), 0, st, d_table, n_docs, d_bad);
    });
    if (e != hipSuccess || refused) {
        delete t;
        if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? NS_E_NOMEM : NS_E_HIP, "%s: %s", fn, hipGetErrorString(e));
        return fail(ctx, NS_E_INVAL, "%s: a document has a factor that is not finite or has its sign bit set", fn);
    }
    *out = t;
    return NS_OK;
}

extern "C" int ns_docboost_release(ns_ctx* ctx, ns_docboost* table) {
    if (!ctx || !table || table->ctx != ctx) return fail(ctx, NS_E_INVAL, "ns_docboost_release: table does not belong to this ctx");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(table->d_boost);
    delete table;
    return NS_OK;
}

extern "C" int ns_boosted_kernel_ms(float* out2, int reset) {
    if (!out2) return NS_E_INVAL;
    for (int i = 0; i < 2; i++) out2[i] = g_bb_ms[i];
    if (reset) g_bb_ms[0] = g_bb_ms[1] = 0.0f;
    return NS_OK;
}

// boosts == NULL is the quorum sibling, plan and kernels; otherwise the sibling's plan, every item given a bound (kAfterAll
// without a cursor), and the BOOST instantiations of k_bq_select.  The join is the sibling's: it carries key bits.
extern "C" int ns_search_boosted_after(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                                       const uint16_t* clauses, const uint8_t* needs, uint32_t n_terms, uint32_t k, const ns_cursor* after,
                                       const uint32_t* seg_ids, ns_seg* const* segs, ns_docboost* const* boosts, uint32_t n_segs, ns_hit* hits_out,
                                       uint32_t* nhits_out, uint64_t* found_out, uint64_t* rest_out, float* device_ms_out) {
    return bq_search(ctx, "ns_search_boosted_after", queries, n_queries, terms, roles, clauses, needs, n_terms, k, after, seg_ids, segs, n_segs, hits_out, nhits_out,
                     found_out, rest_out, device_ms_out, boosts);
}

static int bq_search(ns_ctx* ctx, const char* fn, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                     const uint16_t* clauses, const uint8_t* needs, uint32_t n_terms, uint32_t k, const ns_cursor* after, const uint32_t* seg_ids, ns_seg* const* segs, uint32_t n_segs, ns_hit* hits_out,
                     uint32_t* nhits_out, uint64_t* found_out, uint64_t* rest_out, float* device_ms_out, ns_docboost* const* boosts) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "%s: ctx is NULL", fn);
    if (device_ms_out) *device_ms_out = 0.0f;
    if (n_queries == 0) return NS_OK;
    if (!queries || !hits_out || !nhits_out || (n_terms && !terms)) return fail(ctx, NS_E_INVAL, "%s: null argument", fn);
    if (!n_segs) return fail(ctx, NS_E_INVAL, "%s: no segment listed", fn);
    std::vector<FcSegView> views;
    std::vector<DevFcSeg> dsegs;
    std::vector<DevBqSeg> bqs(boosts ? 2 * (size_t)n_segs : (size_t)n_segs);   // with tables: n_segs DevBqBoost behind
    const int rc = bind_segments<void>(ctx, fn, seg_ids, segs, nullptr, nullptr, n_segs, views, dsegs, [&](uint32_t i, const ns_seg* s, const void*) {
        bqs[i] = DevBqSeg{s->d_norm, seg_ids[i], boosts ? n_segs : 0u};
        if (boosts) {
            const ns_docboost* t = boosts[i];
            if (!t) return fail(ctx, NS_E_INVAL, "%s: segment or boost table %u is NULL", fn, i);
            if (t->ctx != ctx) return fail(ctx, NS_E_INVAL, "%s: boost table %u does not belong to this ctx", fn, i);
            if (t->n_docs < s->n_docs) return fail(ctx, NS_E_INVAL, "%s: boost table %u has %u factors, its segment has %u documents", fn, i, t->n_docs, s->n_docs);
            const DevBqBoost b{t->d_boost, 0ull};
            std::memcpy(&bqs[(size_t)n_segs + i], &b, sizeof(b));
        }
        return (int)NS_OK;
    });
    if (rc != NS_OK) return rc;
    std::vector<BqRef> refs;
    std::vector<FcItem> items;
    RankedPlan plan;
    std::string why;
    const uint32_t tile = ns_facet_tile_docs(), win = bq_win_docs(tile);
    const uint16_t* const given = clauses;
    clauses = bq_live_clauses(clauses, n_terms, roles);
    if (!bq_live_needs(given, clauses, needs, why)) return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    const bool grouped = clauses != nullptr, quorum = needs != nullptr;
    uint32_t max_need = 0;
    if (bq_plan_quorum(queries, n_queries, terms, roles, clauses, needs, n_terms, views.data(), n_segs, tile, refs, items, max_need, why) != NS_OK)
        return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    if (!ranked_call_plan(items, n_queries, k, after, views, [](uint32_t bits) { return after_ord(bits); }, false, kSdCandBytes, plan, why))
        return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    if (boosts) ranked_plan_bound_all(items.size(), plan);   // (the BOOST kernels exist with AFTER alone)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    static const SelectKernel<BqRef, DevBqSeg> kBoosted[3] = {k_bq_select<true, false, false, true>, k_bq_select<true, true, false, true>,
                                                              k_bq_select<true, true, true, true>};   // [boolean, grouped, quorum]
    static const SelectKernel<BqRef, DevBqSeg> kSelect[3][2] = {{k_bq_select<false, false>, k_bq_select<true, false>},
                                                                {k_bq_select<false, true>, k_bq_select<true, true>},
                                                                {k_bq_select<false, true, true>, k_bq_select<true, true, true>}};   // [boolean, grouped, quorum][paged]
    const uint32_t K = plan.K;
    RankedCall<BqRef, DevBqSeg> c{items, refs, dsegs, bqs, plan, n_queries};
    c.select = boosts ? kBoosted[quorum ? 2 : grouped] : kSelect[quorum ? 2 : grouped][plan.paged];
    c.select_arg = win;
    c.select_lds = quorum ? bq_quorum_lds_bytes(win, bq_launch_planes(max_need)) : bq_lds_bytes(win);   // (the product's: at most 42 KiB)
#if defined(NS_VARIANTS) || defined(NS_COUNT)
    if (c.select_lds > (48u << 10))   // (the test windows only: the product's fits the default)
        c.before = hipFuncSetAttribute(reinterpret_cast<const void*>(c.select), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.select_lds);
#endif
    c.stages = 2;
    c.ms_acc = boosts ? g_bb_ms : quorum ? g_qq_ms : grouped ? g_gq_ms : g_bq_ms;
    c.hits_out = hits_out; c.nhits_out = nhits_out; c.found_out = found_out; c.rest_out = rest_out; c.device_ms_out = device_ms_out;
    return run_ranked(ctx, fn, c, [=](const RankedDev<BqRef, DevBqSeg>& d, const SdBatch& b, hipStream_t st) {
        hipLaunchKernelGGL(k_bq_join, dim3((b.q_end - b.q_begin + 3) / 4), dim3(256), 0, st, d.items, d.q_off, b.q_begin, b.q_end, b.item_begin, d.aux, d.cand, K, d.hits, d.nhits);
    }, [](const RankedDev<BqRef, DevBqSeg>&, const SdBatch&, hipStream_t) {});
}

// ------------------------------------------------------------------------------------------------
// One hit per group (csrc/ns_boolean.hip k_bq_select<false, ., ., ., true> and k_bq_join_collapsed, csrc/ns_collapse.hip k_cl_count,
// csrc/ns_collapse_plan.hpp)
static thread_local float g_cl_ms[3] = {0.0f, 0.0f, 0.0f};   // k_bq_select, k_bq_join_collapsed, k_cl_count: summed over the thread's ns_search_collapsed calls (ns_collapsed_kernel_ms)

extern "C" int ns_collapsed_kernel_ms(float* out3, int reset) {
    if (!out3) return NS_E_INVAL;
    for (int i = 0; i < 3; i++) out3[i] = g_cl_ms[i];
    if (reset) g_cl_ms[0] = g_cl_ms[1] = g_cl_ms[2] = 0.0f;
    return NS_OK;
}

// ns_search_boosted_after's validation and plan without a cursor; the block is run_ranked's plus the groups and others rows, and
// per cut the count kernel runs behind the join when others are asked for.
extern "C" int ns_search_collapsed(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                                   const uint16_t* clauses, const uint8_t* needs, uint32_t n_terms, uint32_t k, const uint32_t* seg_ids,
                                   ns_seg* const* segs, ns_docboost* const* boosts, ns_dockeys* const* groups, uint32_t n_segs, ns_hit* hits_out,
                                   uint32_t* groups_out, uint32_t* others_out, uint32_t* nhits_out, uint64_t* found_out, float* device_ms_out) {
    const char* fn = "ns_search_collapsed";
    if (!ctx) return fail(nullptr, NS_E_INVAL, "%s: ctx is NULL", fn);
    if (device_ms_out) *device_ms_out = 0.0f;
    if (n_queries == 0) return NS_OK;
    if (!queries || !hits_out || !groups_out || !nhits_out || (n_terms && !terms)) return fail(ctx, NS_E_INVAL, "%s: null argument", fn);
    if (!n_segs) return fail(ctx, NS_E_INVAL, "%s: no segment listed", fn);
    if (!groups) return fail(ctx, NS_E_INVAL, "%s: null group tables", fn);
    std::vector<FcSegView> views;
    std::vector<DevFcSeg> dsegs;
    std::vector<DevBqSeg> bqs(3 * (size_t)n_segs);   // n_segs DevBqSeg, n_segs DevBqBoost (zero without boosts), n_segs DevBqGroup
    std::memset(bqs.data(), 0, bqs.size() * sizeof(DevBqSeg));
    const int rc = bind_segments<void>(ctx, fn, seg_ids, segs, nullptr, nullptr, n_segs, views, dsegs, [&](uint32_t i, const ns_seg* s, const void*) {
        bqs[i] = DevBqSeg{s->d_norm, seg_ids[i], n_segs};
        if (boosts) {
            const ns_docboost* t = boosts[i];
            if (!t) return fail(ctx, NS_E_INVAL, "%s: segment or boost table %u is NULL", fn, i);
            if (t->ctx != ctx) return fail(ctx, NS_E_INVAL, "%s: boost table %u does not belong to this ctx", fn, i);
            if (t->n_docs < s->n_docs) return fail(ctx, NS_E_INVAL, "%s: boost table %u has %u factors, its segment has %u documents", fn, i, t->n_docs, s->n_docs);
            const DevBqBoost b{t->d_boost, 0ull};
            std::memcpy(&bqs[(size_t)n_segs + i], &b, sizeof(b));
        }
        const ns_dockeys* g = groups[i];
        if (!g) return fail(ctx, NS_E_INVAL, "%s: segment or group table %u is NULL", fn, i);
        if (g->ctx != ctx) return fail(ctx, NS_E_INVAL, "%s: group table %u does not belong to this ctx", fn, i);
        if (g->n_docs != s->n_docs) return fail(ctx, NS_E_INVAL, "%s: group table %u keys %u documents, its segment has %u", fn, i, g->n_docs, s->n_docs);
        const DevBqGroup dg{g->d_keys, 0ull};
        std::memcpy(&bqs[2 * (size_t)n_segs + i], &dg, sizeof(dg));
        return (int)NS_OK;
    });
    if (rc != NS_OK) return rc;
    std::vector<BqRef> refs;
    std::vector<FcItem> items;
    RankedPlan plan;
    CollapsePlan cp;
    std::string why;
    const uint32_t tile = ns_facet_tile_docs(), win = bq_win_docs(tile);
    const uint16_t* const given = clauses;
    clauses = bq_live_clauses(clauses, n_terms, roles);
    if (!bq_live_needs(given, clauses, needs, why)) return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    const bool grouped = clauses != nullptr;   // (with clauses the QUORUM kernels run: a call without needs plans need 1 everywhere)
    uint32_t max_need = 0;
    if (bq_plan_quorum(queries, n_queries, terms, roles, clauses, needs, n_terms, views.data(), n_segs, tile, refs, items, max_need, why) != NS_OK)
        return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    if (!ranked_call_plan(items, n_queries, k, nullptr, views, [](uint32_t bits) { return after_ord(bits); }, false, kSdCandBytes, plan, why))
        return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    const uint32_t planes = grouped ? bq_launch_planes(max_need) : 0u;
    if (!collapse_plan(plan, n_queries, others_out != nullptr, planes, cp, why)) return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    HIPCHK(ctx, hipSetDevice(ctx->device));
    static const SelectKernel<BqRef, DevBqSeg> kSelect[2][2] = {{k_bq_select<false, false, false, false, true>, k_bq_select<false, false, false, true, true>},
                                                                {k_bq_select<false, true, true, false, true>, k_bq_select<false, true, true, true, true>}};   // [clauses][boosts]
    using CountKernel = void (*)(const FcItem*, const BqRef*, const DevFcSeg*, const DevBqSeg*, uint32_t, const uint32_t*, const uint32_t*, uint32_t*);
    static const CountKernel kCount[2] = {k_cl_count<false, false>, k_cl_count<true, true>};
    const SelectKernel<BqRef, DevBqSeg> select = kSelect[grouped][boosts != nullptr];
    const CountKernel count = kCount[grouped];
    const size_t select_lds = grouped ? bq_quorum_lds_bytes(win, planes) : bq_lds_bytes(win);
    const uint32_t K = plan.K;
    const size_t n_out = cp.out_slots;
    CallBlock blk(ctx);
#if defined(NS_VARIANTS) || defined(NS_COUNT)
    if (select_lds > (48u << 10))   // (the test windows only: the product's fits the default)
        blk.chk(hipFuncSetAttribute(reinterpret_cast<const void*>(select), hipFuncAttributeMaxDynamicSharedMemorySize, (int)select_lds));
#endif
    if (cp.count_lds) blk.chk(hipFuncSetAttribute(reinterpret_cast<const void*>(count), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cp.count_lds));
    const size_t per_cut = (size_t)cp.stages + 1;
    const size_t o_items = blk.reserve(items.size() * sizeof(FcItem)), o_refs = blk.reserve(refs.size() * sizeof(BqRef)),
                 o_segs = blk.reserve(dsegs.size() * sizeof(DevFcSeg)), o_aux = blk.reserve(bqs.size() * sizeof(DevBqSeg)),
                 o_qoff = blk.reserve(plan.q_off.size() * 4), o_hits = blk.reserve(n_out * sizeof(ns_hit)), o_groups = blk.reserve(n_out * 4),
                 o_others = blk.reserve(cp.count ? n_out * 4 : 0), o_nhits = blk.reserve((size_t)n_queries * 4),
                 o_found = blk.reserve((size_t)n_queries * 8), o_cand = blk.reserve((size_t)plan.cand_rows * K * 8);   // <= kSdCandBytes
    blk.alloc(plan.cuts.size() * per_cut);
    if (blk.ok()) {
        blk.upload(o_items, items.data(), items.size() * sizeof(FcItem));
        blk.upload(o_refs, refs.data(), refs.size() * sizeof(BqRef));
        blk.upload(o_segs, dsegs.data(), dsegs.size() * sizeof(DevFcSeg));
        blk.upload(o_aux, bqs.data(), bqs.size() * sizeof(DevBqSeg));
        blk.upload(o_qoff, plan.q_off.data(), plan.q_off.size() * 4);
        blk.zero(o_found, (size_t)n_queries * 8);
        const FcItem* d_items = blk.at<const FcItem>(o_items);
        const BqRef* d_refs = blk.at<const BqRef>(o_refs);
        const DevFcSeg* d_segs = blk.at<const DevFcSeg>(o_segs);
        const DevBqSeg* d_aux = blk.at<const DevBqSeg>(o_aux);
        uint32_t* d_others = cp.count ? blk.at<uint32_t>(o_others) : nullptr;
        for (size_t i = 0; i < plan.cuts.size() && blk.ok(); i++) {
            const SdBatch& b = plan.cuts[i];
            const uint32_t n_it = b.item_end - b.item_begin;
            blk.record(i * per_cut + 0);
            if (n_it) {
                hipLaunchKernelGGL(select, dim3(n_it), dim3(256), select_lds, blk.st, d_items + b.item_begin, d_refs, d_segs, d_aux, K, win, blk.at<uint64_t>(o_cand),
                                   blk.at<unsigned long long>(o_found), (const uint64_t*)nullptr, (unsigned long long*)nullptr);
                blk.launched();
            }
            blk.record(i * per_cut + 1);
            hipLaunchKernelGGL(k_bq_join_collapsed, dim3((b.q_end - b.q_begin + 3) / 4), dim3(256), 0, blk.st, d_items, blk.at<const uint32_t>(o_qoff), b.q_begin,
                               b.q_end, b.item_begin, d_aux, blk.at<const uint64_t>(o_cand), K, blk.at<uint32_t>(o_hits), blk.at<uint32_t>(o_nhits),
                               blk.at<uint32_t>(o_groups), d_others);
            blk.launched();
            blk.record(i * per_cut + 2);
            if (cp.count) {
                if (n_it) {
                    hipLaunchKernelGGL(count, dim3(n_it), dim3(256), cp.count_lds, blk.st, d_items + b.item_begin, d_refs, d_segs, d_aux, K,
                                       blk.at<const uint32_t>(o_nhits), blk.at<const uint32_t>(o_groups), d_others);
                    blk.launched();
                }
                blk.record(i * per_cut + 3);
            }
        }
        blk.fetch(hits_out, o_hits, n_out * sizeof(ns_hit));
        blk.fetch(groups_out, o_groups, n_out * 4);
        if (cp.count) blk.fetch(others_out, o_others, n_out * 4);
        blk.fetch(nhits_out, o_nhits, (size_t)n_queries * 4);
        if (found_out) blk.fetch(found_out, o_found, (size_t)n_queries * 8);
        blk.sync();
        if (blk.ok()) {
            float sum = 0.0f;
            for (size_t i = 0; i < plan.cuts.size(); i++)
                for (uint32_t j = 0; j < cp.stages; j++) {
                    float ms = 0.0f;
                    if (blk.elapsed_ms(i * per_cut + j, i * per_cut + j + 1, &ms)) { g_cl_ms[j] += ms; sum += ms; }
                }
            if (device_ms_out) *device_ms_out = sum;
        }
    }
    return blk.finish(fn);
}

// ------------------------------------------------------------------------------------------------
// Facet counts and date order for boolean queries (csrc/ns_boolean_sets.hip)
static thread_local float g_bs_ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // k_bs_count, k_bs_select, k_sd_join, k_bs_score: summed over the thread's calls (ns_boolean_sets_kernel_ms)

extern "C" int ns_boolean_sets_kernel_ms(float* out4, int reset) {
    if (!out4) return NS_E_INVAL;
    for (int i = 0; i < 4; i++) out4[i] = g_bs_ms[i];
    if (reset) g_bs_ms[0] = g_bs_ms[1] = g_bs_ms[2] = g_bs_ms[3] = 0.0f;
    return NS_OK;
}

static int bs_facet(ns_ctx* ctx, const char* fn, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                    const uint16_t* clauses, const uint8_t* needs, uint32_t n_terms, const uint32_t* seg_ids, ns_seg* const* segs, ns_facet* const* tables, uint32_t n_segs,
                    uint32_t* counts_out, uint64_t* found_out, float* device_ms_out);
static int bs_sorted(ns_ctx* ctx, const char* fn, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                     const uint16_t* clauses, const uint8_t* needs, uint32_t n_terms, uint32_t k, uint32_t flags, const ns_cursor* after, const uint32_t* seg_ids,
                     ns_seg* const* segs, ns_dockeys* const* keys, uint32_t n_segs, ns_hit* hits_out, uint32_t* keys_out,
                     uint32_t* nhits_out, uint64_t* found_out, uint64_t* rest_out, float* device_ms_out);

extern "C" int ns_facet_count_boolean(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                                      uint32_t n_terms, const uint32_t* seg_ids, ns_seg* const* segs, ns_facet* const* tables, uint32_t n_segs,
                                      uint32_t* counts_out, uint64_t* found_out, float* device_ms_out) {
    return bs_facet(ctx, "ns_facet_count_boolean", queries, n_queries, terms, roles, nullptr, nullptr, n_terms, seg_ids, segs, tables, n_segs, counts_out, found_out, device_ms_out);
}

extern "C" int ns_facet_count_grouped(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                                      const uint16_t* clauses, uint32_t n_terms, const uint32_t* seg_ids, ns_seg* const* segs, ns_facet* const* tables,
                                      uint32_t n_segs, uint32_t* counts_out, uint64_t* found_out, float* device_ms_out) {
    return bs_facet(ctx, "ns_facet_count_grouped", queries, n_queries, terms, roles, clauses, nullptr, n_terms, seg_ids, segs, tables, n_segs, counts_out, found_out, device_ms_out);
}

extern "C" int ns_search_sorted_boolean(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                                        uint32_t n_terms, uint32_t k, uint32_t flags, const ns_cursor* after, const uint32_t* seg_ids,
                                        ns_seg* const* segs, ns_dockeys* const* keys, uint32_t n_segs, ns_hit* hits_out, uint32_t* keys_out,
                                        uint32_t* nhits_out, uint64_t* found_out, uint64_t* rest_out, float* device_ms_out) {
    return bs_sorted(ctx, "ns_search_sorted_boolean", queries, n_queries, terms, roles, nullptr, nullptr, n_terms, k, flags, after, seg_ids, segs, keys, n_segs, hits_out,
                     keys_out, nhits_out, found_out, rest_out, device_ms_out);
}

extern "C" int ns_search_sorted_grouped(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                                        const uint16_t* clauses, uint32_t n_terms, uint32_t k, uint32_t flags, const ns_cursor* after,
                                        const uint32_t* seg_ids, ns_seg* const* segs, ns_dockeys* const* keys, uint32_t n_segs, ns_hit* hits_out,
                                        uint32_t* keys_out, uint32_t* nhits_out, uint64_t* found_out, uint64_t* rest_out, float* device_ms_out) {
    return bs_sorted(ctx, "ns_search_sorted_grouped", queries, n_queries, terms, roles, clauses, nullptr, n_terms, k, flags, after, seg_ids, segs, keys, n_segs, hits_out,
                     keys_out, nhits_out, found_out, rest_out, device_ms_out);
}

extern "C" int ns_facet_count_quorum(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                                     const uint16_t* clauses, const uint8_t* needs, uint32_t n_terms, const uint32_t* seg_ids, ns_seg* const* segs,
                                     ns_facet* const* tables, uint32_t n_segs, uint32_t* counts_out, uint64_t* found_out, float* device_ms_out) {
    return bs_facet(ctx, "ns_facet_count_quorum", queries, n_queries, terms, roles, clauses, needs, n_terms, seg_ids, segs, tables, n_segs, counts_out, found_out, device_ms_out);
}

extern "C" int ns_search_sorted_quorum(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                                       const uint16_t* clauses, const uint8_t* needs, uint32_t n_terms, uint32_t k, uint32_t flags,
                                       const ns_cursor* after, const uint32_t* seg_ids, ns_seg* const* segs, ns_dockeys* const* keys, uint32_t n_segs,
                                       ns_hit* hits_out, uint32_t* keys_out, uint32_t* nhits_out, uint64_t* found_out, uint64_t* rest_out,
                                       float* device_ms_out) {
    return bs_sorted(ctx, "ns_search_sorted_quorum", queries, n_queries, terms, roles, clauses, needs, n_terms, k, flags, after, seg_ids, segs, keys, n_segs, hits_out,
                     keys_out, nhits_out, found_out, rest_out, device_ms_out);
}

static int bs_facet(ns_ctx* ctx, const char* fn, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                    const uint16_t* clauses, const uint8_t* needs, uint32_t n_terms, const uint32_t* seg_ids, ns_seg* const* segs, ns_facet* const* tables, uint32_t n_segs,
                    uint32_t* counts_out, uint64_t* found_out, float* device_ms_out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "%s: ctx is NULL", fn);
    if (device_ms_out) *device_ms_out = 0.0f;
    if (n_queries == 0) return NS_OK;
    if (!queries || !counts_out || (n_terms && !terms)) return fail(ctx, NS_E_INVAL, "%s: null argument", fn);
    if (!n_segs) return fail(ctx, NS_E_INVAL, "%s: no segment listed (the number of buckets comes from the tables)", fn);
    std::vector<FcSegView> views;
    std::vector<DevFcSeg> dsegs;
    const int rc = bind_segments(ctx, fn, seg_ids, segs, tables, "table", n_segs, views, dsegs,
                                 [&](uint32_t i, const ns_seg* s, const ns_facet* t) { return fc_bind_table(ctx, fn, i, s, t, tables[0], dsegs[i]); });
    if (rc != NS_OK) return rc;
    std::vector<BqRef> refs;
    std::vector<FcItem> items;
    std::string why;
    const uint16_t* const given = clauses;
    clauses = bq_live_clauses(clauses, n_terms, roles);
    if (!bq_live_needs(given, clauses, needs, why)) return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    const bool grouped = clauses != nullptr, quorum = needs != nullptr;
    uint32_t max_need = 0;
    if (bq_plan_quorum(queries, n_queries, terms, roles, clauses, needs, n_terms, views.data(), n_segs, ns_facet_tile_docs(), refs, items, max_need, why) != NS_OK)
        return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    if (quorum)
        return run_count(ctx, fn, items, refs, dsegs, k_bs_count<true, true>, n_queries, tables[0]->n_buckets, false, &g_qq_ms[2], counts_out, found_out,
                         device_ms_out, (size_t)bq_launch_planes(max_need) * (kFcTileDocs / 8u));
    return run_count(ctx, fn, items, refs, dsegs, grouped ? k_bs_count<true> : k_bs_count<false>, n_queries, tables[0]->n_buckets, false,
                     grouped ? &g_gq_ms[2] : &g_bs_ms[0], counts_out, found_out, device_ms_out);
}

static int bs_sorted(ns_ctx* ctx, const char* fn, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, const uint8_t* roles,
                     const uint16_t* clauses, const uint8_t* needs, uint32_t n_terms, uint32_t k, uint32_t flags, const ns_cursor* after, const uint32_t* seg_ids,
                     ns_seg* const* segs, ns_dockeys* const* keys, uint32_t n_segs, ns_hit* hits_out, uint32_t* keys_out,
                     uint32_t* nhits_out, uint64_t* found_out, uint64_t* rest_out, float* device_ms_out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "%s: ctx is NULL", fn);
    if (device_ms_out) *device_ms_out = 0.0f;
    if (n_queries == 0) return NS_OK;
    if (!queries || !hits_out || !keys_out || !nhits_out || (n_terms && !terms)) return fail(ctx, NS_E_INVAL, "%s: null argument", fn);
    if (flags & ~NS_SORT_ASC) return fail(ctx, NS_E_INVAL, "%s: flags 0x%x: only NS_SORT_ASC is known (the roles say what matches)", fn, flags);
    if (!n_segs) return fail(ctx, NS_E_INVAL, "%s: no segment listed", fn);
    std::vector<FcSegView> views;
    std::vector<DevFcSeg> dsegs;
    std::vector<DevSdSeg> sds(n_segs);
    const int rc = bind_segments(ctx, fn, seg_ids, segs, keys, "key table", n_segs, views, dsegs,
                                 [&](uint32_t i, const ns_seg* s, const ns_dockeys* t) { return sd_bind_table(ctx, fn, i, s, t, seg_ids[i], sds[i]); });
    if (rc != NS_OK) return rc;
    const uint32_t asc = (flags & NS_SORT_ASC) ? 1u : 0u;
    std::vector<BqRef> refs;
    std::vector<FcItem> items;
    RankedPlan plan;
    std::string why;
    const uint16_t* const given = clauses;
    clauses = bq_live_clauses(clauses, n_terms, roles);
    if (!bq_live_needs(given, clauses, needs, why)) return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    const bool grouped = clauses != nullptr, quorum = needs != nullptr;
    uint32_t max_need = 0;
    if (bq_plan_quorum(queries, n_queries, terms, roles, clauses, needs, n_terms, views.data(), n_segs, ns_facet_tile_docs(), refs, items, max_need, why) != NS_OK)
        return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    if (!ranked_call_plan(items, n_queries, k, after, views, [asc](uint32_t key) { return after_sort_rank(key, asc != 0u); }, true, kSdCandBytes, plan, why))
        return fail(ctx, NS_E_INVAL, "%s: %s", fn, why.c_str());
    HIPCHK(ctx, hipSetDevice(ctx->device));
    static const SelectKernel<BqRef, DevSdSeg> kSelect[3][2] = {{k_bs_select<false, false>, k_bs_select<true, false>},
                                                                {k_bs_select<false, true>, k_bs_select<true, true>},
                                                                {k_bs_select<false, true, true>, k_bs_select<true, true, true>}};   // [boolean, grouped, quorum][paged]
    const uint32_t K = plan.K;
    RankedCall<BqRef, DevSdSeg> c{items, refs, dsegs, sds, plan, n_queries};
    c.select = kSelect[quorum ? 2 : grouped][plan.paged];
    c.select_arg = asc;
    if (quorum && (c.select_lds = (size_t)bq_launch_planes(max_need) * (kFcTileDocs / 8u)) != 0)   // (the quorum planes: past the default with the static 36 KiB)
        c.before = hipFuncSetAttribute(reinterpret_cast<const void*>(c.select), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.select_lds);
    c.stages = 3;
    c.ms_acc = quorum ? g_qq_ms + 3 : grouped ? g_gq_ms + 3 : g_bs_ms + 1;
    c.queries = queries; c.terms = terms; c.n_terms = n_terms; c.roles = roles; c.roles_region = true;
    c.hits_out = hits_out; c.keys_out = keys_out; c.nhits_out = nhits_out; c.found_out = found_out; c.rest_out = rest_out; c.device_ms_out = device_ms_out;
    return run_ranked(ctx, fn, c, [=](const RankedDev<BqRef, DevSdSeg>& d, const SdBatch& b, hipStream_t st) { sd_launch_join(d, b, K, asc, st); },
                      [=](const RankedDev<BqRef, DevSdSeg>& d, const SdBatch& b, hipStream_t st) {
                          hipLaunchKernelGGL(k_bs_score, sd_score_grid(b, K), dim3(256), 0, st, d.qd, d.terms, d.roles, b.q_begin, b.q_end, d.segs, d.aux, K, d.pos, d.nhits, d.hits);
                      });
}

// ------------------------------------------------------------------------------------------------
// Segment-sharded multi-GPU: join the all-gathered per-rank rows (k_merge_ranks).  Device pointers; asynchronous on the ctx stream.
extern "C" int ns_merge_rank_rows(ns_ctx* ctx, const void* d_hits, const void* d_nhits, const void* d_found, uint32_t n_ranks,
                                  uint32_t n_queries, uint32_t k, const uint32_t* d_seg_map, uint32_t seg_map_stride,
                                  void* d_out_hits, void* d_out_nhits, void* d_out_found) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_merge_rank_rows: ctx is NULL");
    if (n_ranks < 1 || n_ranks > 64) return fail(ctx, NS_E_INVAL, "ns_merge_rank_rows: %u ranks (1..64 supported)", n_ranks);
    if (k < 1 || k > NS_MAX_K) return fail(ctx, NS_E_INVAL, "k=%u outside [1,%u]", k, NS_MAX_K);
    if (!n_queries) return NS_OK;
    if (!d_hits || !d_nhits || !d_found || !d_out_hits || !d_out_nhits || !d_out_found) return fail(ctx, NS_E_INVAL, "ns_merge_rank_rows: null buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_merge_ranks, dim3((n_queries + 3) / 4), dim3(256), 0, ctx->stream, (const Hit*)d_hits, (const uint32_t*)d_nhits,
                       (const uint64_t*)d_found, n_ranks, n_queries, k, d_seg_map, seg_map_stride, (Hit*)d_out_hits, (uint32_t*)d_out_nhits,
                       (uint64_t*)d_out_found);
    HIPCHK(ctx, hipGetLastError());
    return NS_OK;
}

// ------------------------------------------------------------------------------------------------
// f4: semantic expansion's similarity search (csrc/ns_sem.hip)
struct ns_sem {
    ns_ctx* ctx = nullptr;
    uint32_t rows = 0, dim = 0, rows_pad = 0;
    float* d_vt = nullptr;   // [dim][rows_pad]
};

extern "C" int ns_sem_upload(ns_ctx* ctx, const float* vecs, uint32_t n_rows, uint32_t dim, ns_sem** out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_sem_upload: ctx is NULL");
    if (!out || !vecs || !n_rows || !dim) return fail(ctx, NS_E_INVAL, "ns_sem_upload: empty table or null argument");
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ns_sem* s = new ns_sem();
    s->ctx = ctx; s->rows = n_rows; s->dim = dim; s->rows_pad = (n_rows + 63u) & ~63u;
    float* d_in = nullptr;
    hipError_t e = hipMalloc((void**)&s->d_vt, (size_t)dim * s->rows_pad * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d_in, (size_t)n_rows * dim * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, vecs, (size_t)n_rows * dim * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_sem_transpose, dim3((s->rows_pad + 31) / 32, (dim + 31) / 32), dim3(256), 0, ctx->stream, d_in, s->d_vt, n_rows, dim, s->rows_pad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_in);
    if (e != hipSuccess) {
        (void)hipFree(s->d_vt);
        delete s;
        return fail(ctx, e == hipErrorOutOfMemory ? NS_E_NOMEM : NS_E_HIP, "ns_sem_upload: %s", hipGetErrorString(e));
    }
    *out = s;
    return NS_OK;
}

extern "C" int ns_sem_release(ns_ctx* ctx, ns_sem* sem) {
    if (!ctx || !sem || sem->ctx != ctx) return fail(ctx, NS_E_INVAL, "ns_sem_release: table does not belong to this ctx");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(sem->d_vt);
    delete sem;
    return NS_OK;
}

extern "C" int ns_sem_topk(ns_ctx* ctx, ns_sem* sem, const float* qvecs, uint32_t n_q, uint32_t topk, float min_sim,
                           const uint32_t* ban_off, const uint32_t* ban_rows, uint32_t* rows_out, float* sims_out,
                           uint32_t* counts_out, float* device_ms_out) {
    if (!ctx || !sem || sem->ctx != ctx) return fail(ctx, NS_E_INVAL, "ns_sem_topk: table does not belong to this ctx");
    if (topk < 1 || topk > (uint32_t)kSemMaxK) return fail(ctx, NS_E_INVAL, "ns_sem_topk: topk=%u outside [1,%d]", topk, kSemMaxK);
    if (device_ms_out) *device_ms_out = 0.0f;
    if (!n_q) return NS_OK;
    if (!qvecs || !rows_out || !sims_out || !counts_out) return fail(ctx, NS_E_INVAL, "ns_sem_topk: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t dim = sem->dim, rows = sem->rows, rp = sem->rows_pad;
    const uint32_t cap = ((rows + 63) / 64) * topk;   // keys a query's scan can leave: topk per wave of 64 rows
    const uint32_t n_groups = (n_q + kSemB - 1) / kSemB;
    const uint32_t n_ban = ban_off ? ban_off[n_q] : 0;
    // per-group ban offsets, rebased
    std::vector<uint32_t> goff((size_t)n_groups * (kSemB + 1), 0), grows(std::max<uint32_t>(n_ban, 1), 0);
    if (n_ban && !ban_rows) return fail(ctx, NS_E_INVAL, "ns_sem_topk: ban_rows is NULL");
    if (n_ban) std::memcpy(grows.data(), ban_rows, (size_t)n_ban * 4);
    for (uint32_t g = 0; g < n_groups; g++)
        for (uint32_t b = 0; b <= (uint32_t)kSemB; b++) {
            const uint32_t qi = std::min(g * kSemB + b, n_q);
            goff[(size_t)g * (kSemB + 1) + b] = ban_off ? ban_off[qi] : 0;
        }
    std::vector<float> qpad((size_t)n_groups * kSemB * dim, 0.0f);
    std::memcpy(qpad.data(), qvecs, (size_t)n_q * dim * 4);

    const size_t n_pad = (size_t)n_groups * kSemB;
    // one block from the ctx pool for all scratch arrays (every search of a serving loop expands its query)
    CallBlock blk(ctx);
    const size_t o_q = blk.reserve(qpad.size() * 4), o_cand = blk.reserve((size_t)kSemB * cap * 8), o_goff = blk.reserve(goff.size() * 4), o_count = blk.reserve((size_t)kSemB * 4),
                 o_grows = blk.reserve(grows.size() * 4), o_orows = blk.reserve(n_pad * topk * 4), o_osims = blk.reserve(n_pad * topk * 4), o_ocnt = blk.reserve(n_pad * 4);
    blk.alloc(2);
    if (blk.ok()) {
        const float* d_q = blk.at<float>(o_q);
        float* d_osims = blk.at<float>(o_osims);
        const uint32_t *d_goff = blk.at<uint32_t>(o_goff), *d_grows = blk.at<uint32_t>(o_grows);
        uint32_t *d_orows = blk.at<uint32_t>(o_orows), *d_ocnt = blk.at<uint32_t>(o_ocnt), *d_count = blk.at<uint32_t>(o_count);
        uint64_t* d_cand = blk.at<uint64_t>(o_cand);
        blk.upload(o_q, qpad.data(), qpad.size() * 4);
        blk.upload(o_goff, goff.data(), goff.size() * 4);
        blk.upload(o_grows, grows.data(), grows.size() * 4);
        blk.zero(o_count, (size_t)kSemB * 4);   // k_sem_final_topk leaves it zero for the next group
        blk.record(0);
        for (uint32_t g = 0; g < n_groups; g++) {
            hipLaunchKernelGGL(k_sem_scan_topk, dim3((rows + 255) / 256), dim3(256), 0, st, sem->d_vt, rows, rp, dim, d_q + (size_t)g * kSemB * dim, min_sim,
                               d_goff + (size_t)g * (kSemB + 1), d_grows, topk, cap, d_cand, d_count);
            hipLaunchKernelGGL(k_sem_final_topk, dim3(kSemB), dim3(256), 0, st, d_cand, cap, d_count, topk, d_orows + (size_t)g * kSemB * topk, d_osims + (size_t)g * kSemB * topk, d_ocnt + (size_t)g * kSemB);
        }
        blk.record(1);
        blk.launched();
        blk.fetch(rows_out, o_orows, (size_t)n_q * topk * 4);
        blk.fetch(sims_out, o_osims, (size_t)n_q * topk * 4);
        blk.fetch(counts_out, o_ocnt, (size_t)n_q * 4);
        blk.sync();
        float ms = 0.0f;
        if (device_ms_out && blk.elapsed_ms(0, 1, &ms)) *device_ms_out = ms;
    }
    return blk.finish("ns_sem_topk");
}

// ------------------------------------------------------------------------------------------------
// Autocomplete (csrc/ns_suggest.hip): the sorted dictionary, its range top-10 tree, and the batched prefix top-L.
struct ns_ac {
    ns_ctx* ctx = nullptr;
    uint32_t n = 0;
    AcLevels lv{};
    uint8_t* d_pool = nullptr;     // term bytes back to back
    uint32_t* d_offs = nullptr;    // n + 1
    uint64_t* d_heads = nullptr;   // first 8 bytes of each term, big-endian, zero-padded
    uint64_t* d_keys = nullptr;    // (~score << 32) | index: the scores live here
    uint64_t* d_tree = nullptr;    // levels back to back, kAcTop keys per node
    // the spelling corrector's side structures (ns_ac_build_fuzzy, csrc/ns_fuzzy.hip); absent until asked for
    bool fz_built = false;
    uint32_t fz_cands = 0;                       // candidates = slots of the permutation
    uint32_t* d_fz_perm = nullptr;               // candidates ordered by (length, index)
    uint64_t* d_fz_sig = nullptr;                // their signatures, in the same order
    uint32_t* d_fz_len_start = nullptr;          // kFzBuckets + 1: first slot of each length
    uint32_t fz_len_start[kFzBuckets + 1] = {};  // the same on the host: sizes a query's slices
    // completion with a fixed prefix (ns_ac_fuzzy_prefix, prefix_len >= 1): candidates per first byte, counted by the first such call
    bool fp_first_built = false;
    uint32_t fp_first[256] = {};
};

static void ac_free(ns_ac* ac) {
    if (!ac) return;
    (void)hipFree(ac->d_pool);
    (void)hipFree(ac->d_offs);
    (void)hipFree(ac->d_heads);
    (void)hipFree(ac->d_keys);
    (void)hipFree(ac->d_tree);
    (void)hipFree(ac->d_fz_perm);
    (void)hipFree(ac->d_fz_sig);
    (void)hipFree(ac->d_fz_len_start);
    delete ac;
}
static void ac_free_fwd(ns_ac* ac) { ac_free(ac); }

extern "C" int ns_ac_upload(ns_ctx* ctx, const uint8_t* pool, const uint64_t* offsets, const uint32_t* scores, uint32_t n_terms, ns_ac** out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_ac_upload: ctx is NULL");
    if (!out) return fail(ctx, NS_E_INVAL, "ns_ac_upload: out is NULL");
    *out = nullptr;
    if (n_terms && (!offsets || !scores)) return fail(ctx, NS_E_INVAL, "ns_ac_upload: null argument");
    if (n_terms == ~0u) return fail(ctx, NS_E_INVAL, "ns_ac_upload: %u terms (the index ~0 is reserved)", n_terms);
    const uint64_t pool_bytes = n_terms ? offsets[n_terms] : 0;
    if (n_terms && offsets[0] != 0) return fail(ctx, NS_E_INVAL, "ns_ac_upload: offsets[0] = %llu, not 0", (unsigned long long)offsets[0]);
    if (pool_bytes >= (1ull << 32)) return fail(ctx, NS_E_INVAL, "ns_ac_upload: a pool of %llu bytes (>= 4 GiB)", (unsigned long long)pool_bytes);
    if (pool_bytes && !pool) return fail(ctx, NS_E_INVAL, "ns_ac_upload: pool is NULL");
    for (uint32_t i = 0; i < n_terms; i++) {
        if (offsets[i + 1] < offsets[i]) return fail(ctx, NS_E_INVAL, "ns_ac_upload: offsets decrease at term %u", i);
        if (i == 0) continue;
        const uint64_t la = offsets[i] - offsets[i - 1], lb = offsets[i + 1] - offsets[i];
        const int c = std::memcmp(pool + offsets[i - 1], pool + offsets[i], (size_t)std::min(la, lb));
        if (c > 0 || (c == 0 && la > lb)) return fail(ctx, NS_E_INVAL, "ns_ac_upload: terms %u and %u are not in byte order", i - 1, i);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ns_ac* ac = new ns_ac();
    ac->ctx = ctx;
    ac->n = n_terms;
    if (n_terms == 0) {   // an empty table answers every prefix with nothing, on the host
        ctx->acs.push_back(ac);
        *out = ac;
        return NS_OK;
    }
    std::vector<uint32_t> offs32(n_terms + 1);
    std::vector<uint64_t> heads(n_terms), keys(n_terms);
    for (uint32_t i = 0; i <= n_terms; i++) offs32[i] = (uint32_t)offsets[i];
    for (uint32_t i = 0; i < n_terms; i++) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        uint64_t h = 0;
        for (uint64_t j = 0; j < len && j < 8; j++) h |= (uint64_t)pool[offsets[i] + j] << (56 - 8 * j);
        heads[i] = h;
        keys[i] = ((uint64_t)(~scores[i]) << 32) | i;
    }
    uint32_t nodes = (n_terms + kAcFan - 1) / kAcFan;
    uint64_t tree_keys = 0;
    for (;;) {
        ac->lv.off[ac->lv.n_levels] = tree_keys;
        ac->lv.nodes[ac->lv.n_levels] = nodes;
        tree_keys += (uint64_t)nodes * kAcTop;
        ac->lv.n_levels++;
        if (nodes <= (uint32_t)kAcFan) break;
        nodes = (nodes + kAcFan - 1) / kAcFan;
    }
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    chk(hipMalloc((void**)&ac->d_pool, std::max<uint64_t>(pool_bytes, 1)));
    chk(hipMalloc((void**)&ac->d_offs, (size_t)(n_terms + 1) * 4));
    chk(hipMalloc((void**)&ac->d_heads, (size_t)n_terms * 8));
    chk(hipMalloc((void**)&ac->d_keys, (size_t)n_terms * 8));
    chk(hipMalloc((void**)&ac->d_tree, (size_t)tree_keys * 8));
    if (e == hipSuccess) {
        if (pool_bytes) chk(hipMemcpyAsync(ac->d_pool, pool, pool_bytes, hipMemcpyHostToDevice, st));
        chk(hipMemcpyAsync(ac->d_offs, offs32.data(), offs32.size() * 4, hipMemcpyHostToDevice, st));
        chk(hipMemcpyAsync(ac->d_heads, heads.data(), heads.size() * 8, hipMemcpyHostToDevice, st));
        chk(hipMemcpyAsync(ac->d_keys, keys.data(), keys.size() * 8, hipMemcpyHostToDevice, st));
    }
    for (uint32_t j = 0; j < ac->lv.n_levels && e == hipSuccess; j++) {
        const uint64_t* src = j == 0 ? ac->d_keys : ac->d_tree + ac->lv.off[j - 1];
        const uint32_t n_src = j == 0 ? n_terms : ac->lv.nodes[j - 1];
        hipLaunchKernelGGL(k_ac_build, dim3((ac->lv.nodes[j] + 3) / 4), dim3(256), 0, st, src, n_src, j == 0 ? 1u : (uint32_t)kAcTop,
                           j == 0 ? 1u : (uint32_t)kAcTop, ac->d_tree + ac->lv.off[j], ac->lv.nodes[j]);
        chk(hipGetLastError());
    }
    chk(hipStreamSynchronize(st));   // the host arrays above are pageable and die here
    if (e != hipSuccess) {
        ac_free(ac);
        return fail(ctx, e == hipErrorOutOfMemory ? NS_E_NOMEM : NS_E_HIP, "ns_ac_upload: %s", hipGetErrorString(e));
    }
    ctx->acs.push_back(ac);
    *out = ac;
    return NS_OK;
}

extern "C" int ns_ac_release(ns_ctx* ctx, ns_ac* ac) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_ac_release: ctx is NULL");
    auto it = std::find(ctx->acs.begin(), ctx->acs.end(), ac);
    if (!ac || it == ctx->acs.end()) return fail(ctx, NS_E_INVAL, "ns_ac_release: table does not belong to this ctx");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->acs.erase(it);
    ac_free(ac);
    return NS_OK;
}

extern "C" int ns_ac_suggest(ns_ctx* ctx, ns_ac* ac, const uint8_t* prefix_bytes, const uint32_t* prefix_offsets, uint32_t n_q, uint32_t L,
                             uint32_t* idx_out, uint32_t* count_out, float* device_ms_out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_ac_suggest: ctx is NULL");
    if (!ac || std::find(ctx->acs.begin(), ctx->acs.end(), ac) == ctx->acs.end())
        return fail(ctx, NS_E_INVAL, "ns_ac_suggest: table does not belong to this ctx");
    if (L < 1 || L > (uint32_t)kAcTop) return fail(ctx, NS_E_INVAL, "ns_ac_suggest: L=%u outside [1,%d]", L, kAcTop);
    if (device_ms_out) *device_ms_out = 0.0f;
    if (!n_q) return NS_OK;
    if (!prefix_offsets || !idx_out || !count_out) return fail(ctx, NS_E_INVAL, "ns_ac_suggest: null argument");
    for (uint32_t q = 0; q < n_q; q++)
        if (prefix_offsets[q + 1] < prefix_offsets[q]) return fail(ctx, NS_E_INVAL, "ns_ac_suggest: prefix offsets decrease at %u", q);
    const uint32_t b0 = prefix_offsets[0], n_bytes = prefix_offsets[n_q] - b0;
    if (n_bytes && !prefix_bytes) return fail(ctx, NS_E_INVAL, "ns_ac_suggest: prefix_bytes is NULL");
    if (ac->n == 0) {   // nothing starts with anything
        std::fill(idx_out, idx_out + (size_t)n_q * L, ~0u);
        std::fill(count_out, count_out + n_q, 0u);
        return NS_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // device block: [offsets (n_q + 1) | prefix bytes | idx n_q x L | counts n_q]; the first two go up in one copy through the
    // ctx's pinned upload buffer, the last two come down in one copy through its pinned result buffer
    const size_t o_bytes = ((size_t)(n_q + 1) * 4 + 7) & ~(size_t)7;
    const size_t up = o_bytes + n_bytes;
    const size_t o_idx = (up + 255) & ~(size_t)255;
    const size_t down = (size_t)n_q * L * 4 + (size_t)n_q * 4;
    CallBlock blk(ctx);
    blk.reserve(o_idx + down);   // the image above is what the kernel indexes: one region
    Staged h;
    blk.chk(stage_host(ctx, up, down, h));
    if (!blk.ok()) return blk.finish("ns_ac_suggest");
    for (uint32_t q = 0; q <= n_q; q++) ((uint32_t*)h.up)[q] = prefix_offsets[q] - b0;
    if (n_bytes) std::memcpy(h.up + o_bytes, prefix_bytes + b0, n_bytes);
    blk.alloc(device_ms_out ? 2 : 0);
    if (blk.ok()) {
        blk.upload(0, h.up, up);
        blk.record(0);
        hipLaunchKernelGGL(k_ac_suggest, dim3((n_q + 3) / 4), dim3(256), 0, st, ac->d_heads, ac->d_offs, ac->d_pool, ac->d_keys, ac->d_tree, ac->lv,
                           ac->n, blk.at<const uint8_t>(o_bytes), blk.at<const uint32_t>(0), n_q, L, blk.at<uint32_t>(o_idx),
                           blk.at<uint32_t>(o_idx + (size_t)n_q * L * 4));
        blk.launched();
        blk.record(1);
        blk.fetch(h.down, o_idx, down);
        blk.sync();
    }
    if (blk.ok()) {
        std::memcpy(idx_out, h.down, (size_t)n_q * L * 4);
        std::memcpy(count_out, h.down + (size_t)n_q * L * 4, (size_t)n_q * 4);
        float ms = 0.0f;
        if (blk.elapsed_ms(0, 1, &ms)) *device_ms_out = ms;
    }
    return blk.finish("ns_ac_suggest");
}

// ------------------------------------------------------------------------------------------------
// Spelling correction (csrc/ns_fuzzy.hip): the side structures of a table, and the batched bounded-distance top-L.
extern "C" int ns_ac_build_fuzzy(ns_ctx* ctx, ns_ac* ac, float* device_ms_out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "ns_ac_build_fuzzy: ctx is NULL");
    if (!ac || std::find(ctx->acs.begin(), ctx->acs.end(), ac) == ctx->acs.end())
        return fail(ctx, NS_E_INVAL, "ns_ac_build_fuzzy: table does not belong to this ctx");
    if (device_ms_out) *device_ms_out = 0.0f;
    if (ac->fz_built) return NS_OK;
    if (ac->n >= (1u << kFzIdxBits)) return fail(ctx, NS_E_INVAL, "ns_ac_build_fuzzy: %u terms (the ranking key holds 30 index bits)", ac->n);
    if (ac->n == 0) { ac->fz_built = true; return NS_OK; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t n = ac->n, n_blocks = (n + kFzChunk - 1) / kFzChunk;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    uint32_t* d_hist = nullptr;
    uint32_t *d_perm = nullptr, *d_len_start = nullptr;
    uint64_t* d_sig = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint32_t len_start[kFzBuckets + 1] = {};
    chk(hipMalloc((void**)&d_hist, (size_t)kFzBuckets * n_blocks * 4));
    chk(hipMalloc((void**)&d_len_start, sizeof(len_start)));
    if (e == hipSuccess && device_ms_out) { chk(hipEventCreate(&ev0)); chk(hipEventCreate(&ev1)); }
    if (e == hipSuccess) {
        if (ev0) chk(hipEventRecord(ev0, st));
        hipLaunchKernelGGL(k_fz_build_count, dim3(n_blocks), dim3(64), 0, st, ac->d_heads, ac->d_offs, ac->d_pool, ac->d_keys, n, d_hist, n_blocks);
        chk(hipGetLastError());
        hipLaunchKernelGGL(k_fz_build_scan, dim3(1), dim3(128), 0, st, d_hist, n_blocks, d_len_start);
        chk(hipGetLastError());
        chk(hipMemcpyAsync(len_start, d_len_start, sizeof(len_start), hipMemcpyDeviceToHost, st));
        chk(hipStreamSynchronize(st));   // the number of candidates sizes the permutation
    }
    const uint32_t cands = len_start[kFzBuckets];
    if (e == hipSuccess && cands > n) e = hipErrorUnknown;
    if (e == hipSuccess) {
        chk(hipMalloc((void**)&d_perm, std::max<size_t>((size_t)cands * 4, 4)));
        chk(hipMalloc((void**)&d_sig, std::max<size_t>((size_t)cands * 8, 8)));
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_fz_build_scatter, dim3(n_blocks), dim3(64), 0, st, ac->d_heads, ac->d_offs, ac->d_pool, ac->d_keys, n, d_hist, n_blocks,
                           d_len_start, d_perm, d_sig);
        chk(hipGetLastError());
        if (ev1) chk(hipEventRecord(ev1, st));
        chk(hipStreamSynchronize(st));
    }
    if (e == hipSuccess) {
        float ms = 0.0f;
        if (ev0 && ev1 && hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) *device_ms_out = ms;
    }
    (void)hipFree(d_hist);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (e != hipSuccess) {
        (void)hipFree(d_perm);
        (void)hipFree(d_sig);
        (void)hipFree(d_len_start);
        return fail(ctx, e == hipErrorOutOfMemory ? NS_E_NOMEM : NS_E_HIP, "ns_ac_build_fuzzy: %s", hipGetErrorString(e));
    }
    ac->d_fz_perm = d_perm;
    ac->d_fz_sig = d_sig;
    ac->d_fz_len_start = d_len_start;
    std::memcpy(ac->fz_len_start, len_start, sizeof(len_start));
    ac->fz_cands = cands;
    ac->fz_built = true;
    return NS_OK;
}

// Measurement knobs of ns_ac_fuzzy and ns_ac_fuzzy_prefix (the A/B of tools/correct_bench.py and tools/complete_bench.py; process-wide,
// never set by the product):
//   NS_FUZZY_NO_SIG=1    the signature filter passes everything
static bool fz_env_flag(const char* name) {
    const char* v = std::getenv(name);
    return v && v[0] == '1';
}

// The two host loops of ac_fuzzy_call over the rows of a call (a batch of 16384 queries walks some 10^5 query bytes here).
// They are functions of their own, never inlined, so that the code the compiler makes for them does not change with the
// function around them.
// The staged upload image of the rows: per row its offset into the term bytes, its first slice, its edits, the signature
// of its bytes ([0-9] -> bits 0..9, [a-z] -> bits 10..35, anything else bit 36), then the bytes; entry R closes both prefix sums.
__attribute__((noinline)) static void fz_fill_image(const uint32_t* rows, const uint32_t* window, uint32_t R, uint32_t slice, const uint8_t* term_bytes,
                                                    const uint32_t* term_offsets, const uint8_t* max_edits, uint32_t* h_offs, uint32_t* h_base,
                                                    uint64_t* h_sig, uint8_t* h_ed, uint8_t* h_bytes) {
    uint32_t at = 0, sl = 0;
    for (uint32_t r = 0; r < R; r++) {
        const uint32_t q = rows[r], len = term_offsets[q + 1] - term_offsets[q];
        const uint8_t* t = term_bytes + term_offsets[q];
        h_offs[r] = at;
        h_base[r] = sl;
        h_ed[r] = max_edits[q];
        uint64_t sig = 0;
        for (uint32_t j = 0; j < len; j++) {
            const uint8_t c = t[j];
            h_bytes[at + j] = c;
            sig |= (c >= '0' && c <= '9') ? 1ull << (c - '0') : (c >= 'a' && c <= 'z') ? 1ull << (10 + c - 'a') : 1ull << 36;
        }
        h_sig[r] = sig;
        at += len;
        sl += (window[r] + slice - 1) / slice;
    }
    h_offs[R] = at;
    h_base[R] = sl;
}
// The staged result image [idx R x L | counts R | dist R x L] -> the rows' queries in the caller's arrays.
__attribute__((noinline)) static void fz_read_image(const uint32_t* rows, uint32_t R, uint32_t L, const char* h_down, uint32_t* idx_out, uint8_t* dist_out,
                                                    uint32_t* count_out) {
    const uint32_t* h_idx = (const uint32_t*)h_down;
    const uint32_t* h_cnt = h_idx + (size_t)R * L;
    const uint8_t* h_dist = (const uint8_t*)(h_cnt + R);
    for (uint32_t r = 0; r < R; r++) {
        const size_t q = rows[r];
        count_out[q] = h_cnt[r];
        std::memcpy(idx_out + q * L, h_idx + (size_t)r * L, (size_t)L * 4);
        std::memcpy(dist_out + q * L, h_dist + (size_t)r * L, L);
    }
}

// ns_ac_fuzzy (fn = its name, complete = false) and ns_ac_fuzzy_prefix (complete = true): the same arguments, refusals, staging
// and three launches.  They differ in a query's length window (n - e .. n + e, or n - e and everything longer), in the plan
// (FzPlan / FpPlan) and in the plan and scan kernels.
static int ac_fuzzy_call(const char* fn, bool complete, ns_ctx* ctx, ns_ac* ac, const uint8_t* term_bytes, const uint32_t* term_offsets,
                         uint32_t n_q, const uint8_t* max_edits, uint32_t prefix_len, uint32_t L, uint32_t* idx_out, uint8_t* dist_out,
                         uint32_t* count_out, float* device_ms_out) {
    if (!ctx) return fail(nullptr, NS_E_INVAL, "%s: ctx is NULL", fn);
    if (!ac || std::find(ctx->acs.begin(), ctx->acs.end(), ac) == ctx->acs.end())
        return fail(ctx, NS_E_INVAL, "%s: table does not belong to this ctx", fn);
    if (!ac->fz_built) return fail(ctx, NS_E_STATE, "%s: ns_ac_build_fuzzy has not been called on this table", fn);
    L = std::max(1u, std::min(L, (uint32_t)kAcTop));
    if (device_ms_out) *device_ms_out = 0.0f;
    if (!n_q) return NS_OK;
    if (!term_offsets || !max_edits || !idx_out || !dist_out || !count_out) return fail(ctx, NS_E_INVAL, "%s: null argument", fn);
    for (uint32_t q = 0; q < n_q; q++) {
        if (term_offsets[q + 1] < term_offsets[q]) return fail(ctx, NS_E_INVAL, "%s: term offsets decrease at %u", fn, q);
        if (max_edits[q] > kFzMaxEdits) return fail(ctx, NS_E_INVAL, "%s: max_edits[%u] = %u above %d", fn, q, max_edits[q], kFzMaxEdits);
    }
    if (term_offsets[n_q] != term_offsets[0] && !term_bytes) return fail(ctx, NS_E_INVAL, "%s: term_bytes is NULL", fn);
    std::fill(idx_out, idx_out + (size_t)n_q * L, ~0u);
    std::fill(dist_out, dist_out + (size_t)n_q * L, (uint8_t)0xff);
    std::fill(count_out, count_out + n_q, 0u);
    const bool by_first = complete && prefix_len >= 1;
    if (by_first && ac->fz_cands && !ac->fp_first_built) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        uint32_t* d_hist = nullptr;
        HIPCHK(ctx, hipMalloc((void**)&d_hist, sizeof(ac->fp_first)));
        hipError_t e = hipMemsetAsync(d_hist, 0, sizeof(ac->fp_first), ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_fp_first_bytes, dim3(std::min(1024u, (ac->fz_cands + 4095) / 4096)), dim3(256), 0, ctx->stream, ac->d_heads,
                               ac->d_fz_perm, ac->fz_cands, d_hist);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(ac->fp_first, d_hist, sizeof(ac->fp_first), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_hist);
        if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? NS_E_NOMEM : NS_E_HIP, "%s: %s", fn, hipGetErrorString(e));
        ac->fp_first_built = true;
    }
    // the terms that can match something: 1..64 bytes, and some candidate inside the length window (completion with a fixed
    // prefix: and some candidate that starts with the term's first byte; the smaller of the two counts bounds its candidates)
    std::vector<uint32_t> rows, window;
    size_t n_bytes = 0;
    for (uint32_t q = 0; q < n_q && ac->fz_cands; q++) {
        const uint32_t len = term_offsets[q + 1] - term_offsets[q], e = max_edits[q];
        if (len == 0 || len > (uint32_t)kFzMaxLen) continue;
        uint32_t w = ac->fz_len_start[complete ? (uint32_t)kFzBuckets : len + e + 1] - ac->fz_len_start[len > e ? len - e : 0];
        if (by_first) w = std::min(w, ac->fp_first[term_bytes[term_offsets[q]]]);
        if (!w) continue;
        rows.push_back(q);
        window.push_back(w);
        n_bytes += len;
    }
    const uint32_t R = (uint32_t)rows.size();
    if (!R) return NS_OK;
    // slice size: 1024 candidates per workgroup, doubled while the launch would exceed 65536 workgroups (a query's slices
    // are sized from an upper bound of its candidates; the ones that the prefix range leaves empty return at once)
    uint32_t slice = 1024;
    uint64_t n_slices = 0;
    for (;; slice *= 2) {
        n_slices = 0;
        for (uint32_t w : window) n_slices += (w + slice - 1) / slice;
        if (n_slices <= 65536 || slice >= (1u << 30)) break;
    }
    if (n_slices >= (1ull << 31)) return fail(ctx, NS_E_INVAL, "%s: %llu slices in one call", fn, (unsigned long long)n_slices);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // device block: [term offsets (R + 1) | slice bases (R + 1) | signatures R | edits R | term bytes] go up in one copy through
    // the ctx's pinned upload buffer; [plans | slice lists] stay on the device; [idx R x L | counts R | dist R x L] come
    // down in one copy through its pinned result buffer
    auto al8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
    const size_t o_base = al8((size_t)(R + 1) * 4), o_sig = o_base + al8((size_t)(R + 1) * 4), o_ed = o_sig + (size_t)R * 8;
    const size_t o_bytes = o_ed + al8(R);
    const size_t up = o_bytes + n_bytes;
    const size_t o_plan = (up + 255) & ~(size_t)255;
    const size_t o_part = o_plan + (((size_t)R * (complete ? sizeof(FpPlan) : sizeof(FzPlan)) + 255) & ~(size_t)255);
    const size_t o_idx = o_part + (size_t)n_slices * kAcTop * 8;
    const size_t down = (size_t)R * L * 4 + (size_t)R * 4 + (size_t)R * L;
    CallBlock blk(ctx);
    blk.reserve(o_idx + down);   // the image above is what the kernels index: one region
    Staged h;
    blk.chk(stage_host(ctx, up, down, h));
    if (!blk.ok()) return blk.finish(fn);
    fz_fill_image(rows.data(), window.data(), R, slice, term_bytes, term_offsets, max_edits, (uint32_t*)h.up, (uint32_t*)(h.up + o_base),
                  (uint64_t*)(h.up + o_sig), (uint8_t*)(h.up + o_ed), (uint8_t*)(h.up + o_bytes));
    blk.alloc(device_ms_out ? 2 : 0);
    if (blk.ok()) {
        const uint32_t use_sig = fz_env_flag("NS_FUZZY_NO_SIG") ? 0u : 1u;
        const uint32_t *d_offs = blk.at<const uint32_t>(0), *d_base = blk.at<const uint32_t>(o_base);
        const uint8_t *d_ed = blk.at<const uint8_t>(o_ed), *d_bytes = blk.at<const uint8_t>(o_bytes);
        const uint64_t* d_sig = blk.at<const uint64_t>(o_sig);
        uint64_t* d_part = blk.at<uint64_t>(o_part);
        uint32_t* d_idx = blk.at<uint32_t>(o_idx);
        uint32_t* d_cnt = d_idx + (size_t)R * L;
        uint8_t* d_dist = (uint8_t*)(d_cnt + R);
        blk.upload(0, h.up, up);
        blk.record(0);
        if (complete) {
            hipLaunchKernelGGL(k_fp_plan, dim3((R + 3) / 4), dim3(256), 0, st, ac->d_heads, ac->d_offs, ac->d_pool, ac->n, ac->d_fz_perm,
                               ac->d_fz_len_start, d_bytes, d_offs, d_ed, R, prefix_len, blk.at<FpPlan>(o_plan));
            blk.launched();
            hipLaunchKernelGGL(k_fp_scan, dim3((uint32_t)n_slices), dim3(256), 0, st, ac->d_heads, ac->d_offs, ac->d_pool, ac->d_keys, ac->d_fz_perm,
                               ac->d_fz_sig, d_bytes, d_offs, d_ed, d_sig, d_base, R, slice, blk.at<const FpPlan>(o_plan), L, use_sig, d_part);
            blk.launched();
        } else {
            hipLaunchKernelGGL(k_fz_plan, dim3((R + 3) / 4), dim3(256), 0, st, ac->d_heads, ac->d_offs, ac->d_pool, ac->n, ac->d_fz_perm,
                               ac->d_fz_len_start, d_bytes, d_offs, d_ed, R, prefix_len, blk.at<FzPlan>(o_plan));
            blk.launched();
            hipLaunchKernelGGL(k_fz_scan, dim3((uint32_t)n_slices), dim3(256), 0, st, ac->d_heads, ac->d_offs, ac->d_pool, ac->d_keys, ac->d_fz_perm,
                               ac->d_fz_sig, d_bytes, d_offs, d_ed, d_sig, d_base, R, slice, blk.at<const FzPlan>(o_plan), L, use_sig, d_part);
            blk.launched();
        }
        hipLaunchKernelGGL(k_fz_select, dim3((R + 3) / 4), dim3(256), 0, st, (const uint64_t*)d_part, d_base, R, L, d_idx, d_dist, d_cnt);
        blk.launched();
        blk.record(1);
        blk.fetch(h.down, o_idx, down);
        blk.sync();
    }
    if (blk.ok()) {
        fz_read_image(rows.data(), R, L, h.down, idx_out, dist_out, count_out);
        float ms = 0.0f;
        if (blk.elapsed_ms(0, 1, &ms)) *device_ms_out = ms;
    }
    return blk.finish(fn);
}

extern "C" int ns_ac_fuzzy(ns_ctx* ctx, ns_ac* ac, const uint8_t* term_bytes, const uint32_t* term_offsets, uint32_t n_q,
                           const uint8_t* max_edits, uint32_t prefix_len, uint32_t L, uint32_t* idx_out, uint8_t* dist_out,
                           uint32_t* count_out, float* device_ms_out) {
    return ac_fuzzy_call("ns_ac_fuzzy", false, ctx, ac, term_bytes, term_offsets, n_q, max_edits, prefix_len, L, idx_out, dist_out, count_out,
                         device_ms_out);
}

// Typo-tolerant completion: the best L candidates whose PREFIX distance to the query is within max_edits.
extern "C" int ns_ac_fuzzy_prefix(ns_ctx* ctx, ns_ac* ac, const uint8_t* prefix_bytes, const uint32_t* prefix_offsets, uint32_t n_q,
                                  const uint8_t* max_edits, uint32_t prefix_len, uint32_t L, uint32_t* idx_out, uint8_t* dist_out,
                                  uint32_t* count_out, float* device_ms_out) {
    return ac_fuzzy_call("ns_ac_fuzzy_prefix", true, ctx, ac, prefix_bytes, prefix_offsets, n_q, max_edits, prefix_len, L, idx_out, dist_out,
                         count_out, device_ms_out);
}

#ifdef NS_COUNT
// Counting build only: the N event counters of one device symbol, read after a device synchronize and optionally reset.
template <size_t N, class Sym>
static int debug_counters(const Sym& sym, unsigned long long* out, int reset) {
    unsigned long long h[N];
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(h, sym, sizeof(h)) != hipSuccess) return -1;
    if (out) std::memcpy(out, h, sizeof(h));
    if (reset) { std::memset(h, 0, sizeof(h)); if (hipMemcpyToSymbol(sym, h, sizeof(h)) != hipSuccess) return -1; }
    return 0;
}
// the driver-stream body's event counters (ns_driver_kernel.hip; 32 values)
extern "C" int ns_debug_counters(unsigned long long* out, int reset) { return debug_counters<ns::kNsCnt>(HIP_SYMBOL(ns::g_ns_cnt), out, reset); }
extern "C" int ns_debug_tile_counters(unsigned long long* out, int reset) { return debug_counters<12>(HIP_SYMBOL(ns::g_ns_tcnt), out, reset); }
// the merge body's counters (ns_merge_kernel.hip): 16 values
extern "C" int ns_debug_merge_counters(unsigned long long* out, int reset) { return debug_counters<ns::kNsMcnt>(HIP_SYMBOL(ns::g_ns_mcnt), out, reset); }
// the candidate buffer's shrinks over all wave bodies (ns_wave_kernel.hip WaveTopK): 4 values
extern "C" int ns_debug_topk_counters(unsigned long long* out, int reset) { return debug_counters<4>(HIP_SYMBOL(ns::g_ns_kcnt), out, reset); }
// the row join's paths and tie rounds (ns_kernels.hip k_merge, k_merge_wide, k_merge_ranks): 16 values
extern "C" int ns_debug_join_counters(unsigned long long* out, int reset) { return debug_counters<16>(HIP_SYMBOL(ns::g_ns_jcnt), out, reset); }
// the facet kernel's paths (ns_facet.hip k_fc_count): 8 values
extern "C" int ns_debug_facet_counters(unsigned long long* out, int reset) { return debug_counters<ns::kNsFcnt>(HIP_SYMBOL(ns::g_ns_fcnt), out, reset); }
// the sorted search's paths (ns_sorted.hip k_sd_select, k_sd_join, k_sd_score): 9 values
extern "C" int ns_debug_sorted_counters(unsigned long long* out, int reset) { return debug_counters<ns::kNsScnt>(HIP_SYMBOL(ns::g_ns_scnt), out, reset); }
// the cursor bound in k_sd_select<., true> and k_bq_select<true> (ns_after.hip): 5 values
extern "C" int ns_debug_after_counters(unsigned long long* out, int reset) { return debug_counters<ns::kNsAcnt>(HIP_SYMBOL(ns::g_ns_acnt), out, reset); }
// the boolean search's paths (ns_boolean.hip k_bq_select, k_bq_join): 8 values
extern "C" int ns_debug_boolean_counters(unsigned long long* out, int reset) { return debug_counters<ns::kNsBcnt>(HIP_SYMBOL(ns::g_ns_bcnt), out, reset); }
// the grouped required stage (ns_boolean.hip k_bq_select<., true>; ns_boolean_sets.hip bs_matched<true>): 11 values
extern "C" int ns_debug_boolean_groups_counters(unsigned long long* out, int reset) { return debug_counters<ns::kNsBgcnt>(HIP_SYMBOL(ns::g_ns_bgcnt), out, reset); }
// the quorum required stage (ns_boolean.hip k_bq_select<., ., true>; ns_boolean_sets.hip bs_matched<., true>): 12 values
extern "C" int ns_debug_boolean_quorum_counters(unsigned long long* out, int reset) { return debug_counters<ns::kNsBqcnt>(HIP_SYMBOL(ns::g_ns_bqcnt), out, reset); }
// per-document factors (ns_boolean.hip k_bq_select<true, ., ., true>): 8 values
extern "C" int ns_debug_boolean_boost_counters(unsigned long long* out, int reset) { return debug_counters<ns::kNsBbcnt>(HIP_SYMBOL(ns::g_ns_bbcnt), out, reset); }
// one hit per group (ns_boolean.hip k_bq_select<false, ., ., ., true>, k_bq_join_collapsed; ns_collapse.hip k_cl_count): 14 values
extern "C" int ns_debug_collapse_counters(unsigned long long* out, int reset) { return debug_counters<ns::kNsClcnt>(HIP_SYMBOL(ns::g_ns_clcnt), out, reset); }
// facets and date order of boolean queries (ns_boolean_sets.hip k_bs_count, k_bs_select, k_bs_score): 12 values
extern "C" int ns_debug_boolean_sets_counters(unsigned long long* out, int reset) { return debug_counters<ns::kNsBscnt>(HIP_SYMBOL(ns::g_ns_bscnt), out, reset); }
// the corrector's and completion's build, scan and select kernels (ns_fuzzy.hip): 17 values
extern "C" int ns_debug_fuzzy_counters(unsigned long long* out, int reset) { return debug_counters<ns::kNsZcnt>(HIP_SYMBOL(ns::g_ns_zcnt), out, reset); }
// related terms (ns_terms.hip k_ta_count): 8 values; value 5, the rows refused over the cap, is counted on the host
extern "C" int ns_debug_terms_counters(unsigned long long* out, int reset) {
    const int rc = debug_counters<ns::kNsTacnt>(HIP_SYMBOL(ns::g_ns_tacnt), out, reset);
    if (rc == 0 && out) out[5] = g_ta_rows_refused;
    if (rc == 0 && reset) g_ta_rows_refused = 0;
    return rc;
}
#endif
