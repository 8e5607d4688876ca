// CPU harness of the batch planner (nextsearch-api_amd/csrc/ns_plan.hpp) for tests/test_batch_plan.py: plans one batch
// over segments described by the caller and writes the descriptor image a device would receive, with fixed stand-ins for
// the device pointers of the DevSeg table.  Built by the test with the host compiler; not part of the product.
#include <hip/hip_runtime.h>

#include "ns_plan.hpp"

using namespace ns;

struct HarnessSeg { uint32_t n_docs, norm_safe, packed, pad; uint64_t n_postings; };
struct HarnessList { uint32_t seg, kind, first, count, idf_bits, entry; };   // kind: 0 impact stream, 1 skip table, 2 block maxima

// settings: the PlanSettings fields in the order of test_batch_plan.py SETTINGS.  out: see test_batch_plan.py OUT.
// bucket_pos: kOrderBuckets + 1 launch positions.  Returns the planner's status, or -100 when `image` is too small.
extern "C" int plan_batch(const uint64_t* settings, const HarnessSeg* hsegs, uint32_t n_segs, const HarnessList* lists,
                          uint32_t n_lists, const ns_query_desc* queries, const ns_term_ref* terms, uint32_t n_queries,
                          uint32_t k, uint32_t flags, char* image, uint64_t image_cap, uint64_t* out, uint32_t* bucket_pos,
                          char* err, uint32_t err_cap) {
    PlanSettings c;
    const uint64_t* v = settings;
    c.variant = (uint32_t)*v++; c.min_items = (uint32_t)*v++; c.split_postings = (uint32_t)*v++; c.n_cus = (int)*v++;
    c.use_impacts = *v++ != 0; c.use_packed = (int)*v++; c.use_skips = *v++ != 0; c.use_merge = *v++ != 0;
    c.merge_ratio = (uint32_t)*v++; c.use_pruning = *v++ != 0; c.share_mode = (int)*v++; c.share_ratio = (uint32_t)*v++;
    c.share_min_postings = *v++; c.prep_threads = (unsigned)*v++; c.order_mode = (int)*v++; c.order_coarse = (int)*v++;
    c.order_coarse_forced = *v++ != 0;
    for (int i = 0; i < 4; i++) c.key_pct[i] = (uint32_t)*v++;
    c.tile_dens64 = (uint32_t)*v++;

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

    uint64_t refused = 0, empty_groups = 0, largest_dealt = 0;
    reg.tab.for_each([&](uint64_t, const ShareRegistry::Ent& e) { refused += e.bad; });
    for (unsigned s = 0; s < P.width; s++)
        for (const HostGroup& g : P.slices[s].groups) empty_groups += views[g.g.seg].n_docs == 0;
    if (P.deal)
        for (uint32_t cl = 0; cl < (kOrderBuckets >> P.deal_shift); cl++)
            largest_dealt = std::max<uint64_t>(largest_dealt, P.bucket_pos[(cl + 1) << P.deal_shift] - P.bucket_pos[cl << P.deal_shift]);
    const BatchPlan::Layout& L = P.layout;
    const uint64_t o[] = {L.bytes, L.items, L.witems, L.terms, L.groups, L.queries, L.segs, L.wideq, L.share,
                          P.n_items, P.n_witems, P.n_dterms, P.n_bgroups, P.n_rows, P.n_class[0], P.n_class[1], P.direct,
                          P.shared, P.share_build.size(), P.share_postings, P.all_imp, P.all_pk, P.pruned, P.deal,
                          P.deal_shift, P.width, P.postings_total, P.wide_q.size(), refused, empty_groups, largest_dealt};
    std::memcpy(out, o, sizeof(o));
    std::memcpy(bucket_pos, P.bucket_pos.data(), (kOrderBuckets + 1) * 4);
    return NS_OK;
}
