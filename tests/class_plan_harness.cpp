// CPU harness of the batch planner's class model (nextsearch-api_amd/csrc/ns_plan.hpp, "class model") for
// tests/test_class_model_cpu.py: tests/plan_harness.cpp with the class settings behind the others, and per group the class, the
// work estimate and whether the model promoted it among the results.  Built by the test with the host compiler; not part of
// the product.
#include <hip/hip_runtime.h>

#include "ns_plan.hpp"

using namespace ns;

struct HarnessSeg { uint32_t n_docs, norm_safe, packed, pad; uint64_t n_postings; };
struct HarnessList { uint32_t seg, kind, first, count, idf_bits, entry; };   // kind: 0 impact stream, 1 skip table, 2 block maxima
struct HarnessGroup { uint32_t query, seg, term_count, cls, promoted, merge2; uint64_t cost, cmax, work; };

// settings: the PlanSettings fields in the order of test_batch_plan.py SETTINGS, then class_model, class_margin_pct (0: the
// default), force_body, force_share10, force_dens_lo, force_dens_hi.
// out: layout.bytes, .witems, .terms, .queries, .segs, n_witems, n_dterms, n_rows, width, groups, class_stats[0..3], the default
// margin and the three default cost constants.  groups_out: one entry per (query, segment) group in query order (at most groups_cap).
extern "C" int plan_classes(const uint64_t* settings, const HarnessSeg* hsegs, uint32_t n_segs, const HarnessList* lists,
                            uint32_t n_lists, const ns_query_desc* queries, const ns_term_ref* terms, uint32_t n_queries,
                            uint32_t k, uint32_t flags, char* image, uint64_t image_cap, uint64_t* out, HarnessGroup* groups_out,
                            uint64_t groups_cap, char* err, uint32_t err_cap) {
    PlanSettings c;
    const uint64_t* v = settings;
    c.variant = (uint32_t)*v++; c.min_items = (uint32_t)*v++; c.split_postings = (uint32_t)*v++; c.n_cus = (int)*v++;
    c.use_impacts = *v++ != 0; c.use_packed = (int)*v++; c.use_skips = *v++ != 0; c.use_merge = *v++ != 0;
    c.merge_ratio = (uint32_t)*v++; c.use_pruning = *v++ != 0; c.share_mode = (int)*v++; c.share_ratio = (uint32_t)*v++;
    c.share_min_postings = *v++; c.prep_threads = (unsigned)*v++; c.order_mode = (int)*v++; c.order_coarse = (int)*v++;
    c.order_coarse_forced = *v++ != 0;
    for (int i = 0; i < 4; i++) c.key_pct[i] = (uint32_t)*v++;
    c.tile_dens64 = (uint32_t)*v++;
    c.class_model = (int)*v++;
    if (*v) c.class_margin_pct = (uint32_t)*v;
    v++;
    c.force_body = (uint32_t)*v++; c.force_share10 = (uint32_t)*v++; c.force_dens_lo = (uint32_t)*v++; c.force_dens_hi = (uint32_t)*v++;

    const uint32_t tile_docs = kVariants[c.variant].nt * kVariants[c.variant].spt;
    std::vector<SegLists> seg_lists(n_segs);
    std::vector<SegView> views(n_segs);
    std::vector<DevSeg> dsegs(n_segs);
    auto fake = [](uint32_t seg, uint32_t field) { return (uintptr_t)(seg + 1) << 32 | (uintptr_t)field << 12; };
    for (uint32_t i = 0; i < n_lists; i++) {
        const HarnessList& l = lists[i];
        if (l.kind == 0) seg_lists[l.seg].imp.put(l.first, {l.count, l.idf_bits});
        else if (l.kind == 1) seg_lists[l.seg].skip.put(l.first, {l.count, l.entry});
        else seg_lists[l.seg].bmx.put(l.first, {l.count, l.idf_bits, l.entry});
    }
    for (uint32_t s = 0; s < n_segs; s++) {
        const HarnessSeg& h = hsegs[s];
        const uint32_t n_tiles = (h.n_docs + tile_docs - 1) / tile_docs;
        views[s] = SegView{h.n_docs, n_tiles, h.n_postings, h.norm_safe != 0, h.packed != 0, &seg_lists[s]};
        DevSeg& d = dsegs[s];
        d.postings = (const uint2*)fake(s, 1); d.pnorm = (const float*)fake(s, 2); d.norm = (const float*)fake(s, 3);
        d.impacts = seg_lists[s].imp.empty() ? nullptr : (const uint2*)fake(s, 4);
        d.packed = h.packed ? (const uint32_t*)fake(s, 5) : nullptr;
        d.skips = seg_lists[s].skip.empty() ? nullptr : (const uint32_t*)fake(s, 6);
        d.blockmax = seg_lists[s].bmx.empty() ? nullptr : (const float*)fake(s, 7);
        d.n_postings = h.n_postings; d.n_docs = h.n_docs; d.n_tiles = n_tiles;
    }

    BatchPlan P;
    ShareRegistry reg;
    int rc = P.group(c, views, reg, queries, terms, n_queries, k, flags);
    if (rc == NS_OK) {
        for (const DevShare& sh : P.share_build) dsegs[sh.seg].impacts = (const uint2*)fake(sh.seg, 4);   // the score buffers
        rc = P.cut();
    }
    if (rc != NS_OK) { std::snprintf(err, err_cap, "%s", P.err.c_str()); return rc; }
    if (P.layout.bytes > image_cap) return -100;
    std::memset(image, 0, P.layout.bytes);
    P.write(image);
    std::memcpy(image + P.layout.segs, dsegs.data(), dsegs.size() * sizeof(DevSeg));

    uint64_t n_groups = 0;
    for (unsigned s = 0; s < P.width; s++)
        for (const HostGroup& g : P.slices[s].groups) {
            if (n_groups < groups_cap)
                groups_out[n_groups] = HarnessGroup{g.query, g.g.seg, g.g.term_count, g.cls, g.promoted, g.merge2, g.cost, g.cmax, g.work};
            n_groups++;
        }
    const BatchPlan::Layout& L = P.layout;
    const uint64_t o[] = {L.bytes, L.witems, L.terms, L.queries, L.segs, P.n_witems, P.n_dterms, P.n_rows, P.width, n_groups,
                          P.class_stats[0], P.class_stats[1], P.class_stats[2], P.class_stats[3],
                          kClassMarginPct, kTileCostTile16, kTileCostVisit16, kTileCostPosting16};
    std::memcpy(out, o, sizeof(o));
    return NS_OK;
}
