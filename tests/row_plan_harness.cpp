// CPU harness of the batch planner's shared top rows (nextsearch-api_amd/csrc/ns_plan.hpp, "shared top rows") for
// tests/test_row_plan_cpu.py: tests/plan_harness.cpp with the three row settings in front of the others and the row arrays
// among the results.  Built by the test with the host compiler; not part of the product.
#include <hip/hip_runtime.h>

#include "ns_plan.hpp"

using namespace ns;

struct HarnessSeg { uint32_t n_docs, norm_safe, packed, pad; uint64_t n_postings; };
struct HarnessList { uint32_t seg, kind, first, count, idf_bits, entry; };   // kind: 0 impact stream, 1 skip table, 2 block maxima

// settings: row_mode, row_min_users, row_cell_postings, share_mode, use_skips, prep_threads, use_pruning, order_mode.
// out: layout.bytes, .witems, .terms, .ritems, .pitems, n_witems, n_dterms, n_ritems, n_pitems, n_pterms, n_rows, direct, shared, width.
extern "C" int plan_rows(const uint64_t* settings, const HarnessSeg* hsegs, uint32_t n_segs, const HarnessList* lists,
                         uint32_t n_lists, const ns_query_desc* queries, const ns_term_ref* terms, uint32_t n_queries,
                         uint32_t k, uint32_t flags, char* image, uint64_t image_cap, uint64_t* out, char* err, uint32_t err_cap) {
    PlanSettings c;
    c.n_cus = 256;
    c.row_mode = (int)settings[0]; c.row_min_users = (uint32_t)settings[1]; c.row_cell_postings = (uint32_t)settings[2];
    c.share_mode = (int)settings[3]; c.use_skips = settings[4] != 0; c.prep_threads = (unsigned)settings[5];
    c.use_pruning = settings[6] != 0; c.order_mode = (int)settings[7];

    std::vector<SegLists> seg_lists(n_segs);
    std::vector<SegView> views(n_segs);
    for (uint32_t i = 0; i < n_lists; i++) {
        const HarnessList& l = lists[i];
        if (l.kind == 0) seg_lists[l.seg].imp.put(l.first, {l.count, l.idf_bits});
        else if (l.kind == 1) seg_lists[l.seg].skip.put(l.first, {l.count, l.entry});
        else seg_lists[l.seg].bmx.put(l.first, {l.count, l.idf_bits, l.entry});
    }
    const uint32_t tile_docs = kVariants[0].nt * kVariants[0].spt;
    for (uint32_t s = 0; s < n_segs; s++) {
        const HarnessSeg& h = hsegs[s];
        views[s] = SegView{h.n_docs, (h.n_docs + tile_docs - 1) / tile_docs, h.n_postings, h.norm_safe != 0, h.packed != 0, &seg_lists[s]};
    }

    BatchPlan P;
    ShareRegistry reg;
    int rc = P.group(c, views, reg, queries, terms, n_queries, k, flags);
    if (rc == NS_OK) rc = P.cut();
    if (rc != NS_OK) { std::snprintf(err, err_cap, "%s", P.err.c_str()); return rc; }
    if (P.layout.bytes > image_cap) return -100;
    std::memset(image, 0, P.layout.bytes);
    P.write(image);
    const BatchPlan::Layout& L = P.layout;
    const uint64_t o[] = {L.bytes, L.witems, L.terms, L.ritems, L.pitems, P.n_witems, P.n_dterms, P.n_ritems, P.n_pitems,
                          P.n_pterms, P.n_rows, P.direct, P.shared, P.width};
    std::memcpy(out, o, sizeof(o));
    return NS_OK;
}
