// C entry point of the grouped planner (bq_plan_grouped, nextsearch-api_amd/csrc/ns_boolean_plan.hpp) for
// tests/test_grouped_cpu.py: host code only, compiled with g++ by the test.
#include <cstring>

#include "ns_boolean_plan.hpp"

static_assert(sizeof(ns::BqRef) == 32, "BqRef keeps its size: clause took the place of pad");

// bq_plan_grouped (use_bq_plan != 0: bq_plan, which takes no clauses) over the caller's descriptors (qd: n_queries x {term_begin,
// term_count}; refs: n_refs ns_term_ref; roles: n_refs bytes or NULL; clauses: n_refs uint16 or NULL) and segments (seg_ids /
// seg_docs / seg_postings: n_segs each, in the call's order; no skip tables).  items_out: 6 uint32 per item {query, seg, ref_begin,
// ref_count, doc_lo, doc_hi}; ref_out: 5 uint64 per planned ref {first, count, role, clause, fp32 bits of idf | fp32 bits of
// qweight << 32}; raw_out (may be NULL): the planned refs' bytes as they are, sizeof(BqRef) each.  Returns the planner's code; the
// message goes to err.
extern "C" int grouped_plan(int use_bq_plan, const uint32_t* qd_in, uint32_t n_queries, const void* refs_in, const uint8_t* roles,
                            const uint16_t* clauses, uint32_t n_refs, const uint32_t* seg_ids, const uint32_t* seg_docs,
                            const uint64_t* seg_postings, uint32_t n_segs, uint32_t tile_docs, uint32_t* items_out, uint64_t items_cap,
                            uint64_t* n_items_out, uint64_t* ref_out, uint64_t refs_cap, uint64_t* n_refs_out, unsigned char* raw_out, char* err,
                            uint32_t err_cap) {
    std::vector<ns::FcSegView> segs(n_segs);
    for (uint32_t i = 0; i < n_segs; i++) {
        segs[i].seg_id = seg_ids[i];
        segs[i].n_docs = seg_docs[i];
        segs[i].n_postings = seg_postings[i];
    }
    std::vector<ns_query_desc> qd(n_queries);
    for (uint32_t q = 0; q < n_queries; q++) qd[q] = ns_query_desc{qd_in[2 * q], qd_in[2 * q + 1]};
    std::vector<ns::BqRef> r;
    std::vector<ns::FcItem> it;
    std::string why;
    const int rc = use_bq_plan ? ns::bq_plan(qd.data(), n_queries, (const ns_term_ref*)refs_in, roles, n_refs, segs.data(), n_segs, tile_docs, r, it, why)
                               : ns::bq_plan_grouped(qd.data(), n_queries, (const ns_term_ref*)refs_in, roles, clauses, n_refs, segs.data(), n_segs,
                                                     tile_docs, r, it, why);
    if (err && err_cap) { std::strncpy(err, why.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    *n_items_out = it.size();
    *n_refs_out = r.size();
    for (size_t i = 0; i < it.size() && i < items_cap; i++) {
        const uint32_t v[6] = {it[i].query, it[i].seg, it[i].ref_begin, it[i].ref_count, it[i].doc_lo, it[i].doc_hi};
        std::memcpy(items_out + 6 * i, v, sizeof(v));
    }
    for (size_t i = 0; i < r.size() && i < refs_cap; i++) {
        uint32_t a, b;
        std::memcpy(&a, &r[i].idf, 4);
        std::memcpy(&b, &r[i].qweight, 4);
        const uint64_t v[5] = {r[i].list.first, r[i].list.count, r[i].role, r[i].clause, (uint64_t)a | ((uint64_t)b << 32)};
        std::memcpy(ref_out + 5 * i, v, sizeof(v));
        if (raw_out) std::memcpy(raw_out + sizeof(ns::BqRef) * i, &r[i], sizeof(ns::BqRef));
    }
    return rc;
}
extern "C" uint32_t grouped_ref_bytes(void) { return (uint32_t)sizeof(ns::BqRef); }
