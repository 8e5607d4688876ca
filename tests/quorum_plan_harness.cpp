// C entry point of the quorum planner (bq_plan_quorum, nextsearch-api_amd/csrc/ns_boolean_plan.hpp) for
// tests/test_quorum_cpu.py: host code only, compiled with g++ by the test.
#include <cstring>

#include "ns_boolean_plan.hpp"

static_assert(sizeof(ns::BqRef) == 32, "BqRef keeps its size: need and duplicate flag live in spare bits of clause");
static_assert(ns::bq_clause_index(ns::bq_clause_word(65535u, 7u, true)) == 65535u && ns::bq_clause_need(ns::bq_clause_word(65535u, 7u, true)) == 7u, "packing");
static_assert(ns::bq_clause_need(5u) == 1u && ns::bq_need_planes(1) == 0 && ns::bq_need_planes(2) == 2 && ns::bq_need_planes(3) == 2 &&
                  ns::bq_need_planes(4) == 3 && ns::bq_need_planes(7) == 3, "a word without a need reads as need 1; planes count to 3 and to 7");

// bq_plan_grouped and bq_plan are thin wrappers of bq_plan_quorum, so comparing which = 0 without needs against which = 1 cannot fail by
// itself: what guards their output bytes are the recorded expectations of tests/test_grouped_cpu.py and tests/test_boolean_cpu.py,
// which stay as they are, and tests/test_quorum_cpu.py's recorded items and refs for the call without needs.
// which: 0 = bq_plan_quorum, 1 = bq_plan_grouped (takes no needs), 2 = bq_plan (takes neither).  Descriptors and segments as
// tests/grouped_plan_harness.cpp's; needs: n_refs bytes or NULL.  ref_out: 7 uint64 per planned ref {first, count, role, clause
// index, need as stored (0 = none), duplicate flag, fp32 bits of idf}; raw_out (may be NULL): the planned refs' bytes as they are.
// max_need_out: the planner's (0 for which != 0).  Returns the planner's code; the message goes to err.
extern "C" int quorum_plan(int which, const uint32_t* qd_in, uint32_t n_queries, const void* refs_in, const uint8_t* roles, const uint16_t* clauses,
                           const uint8_t* needs, uint32_t n_refs, const uint32_t* seg_ids, const uint32_t* seg_docs, const uint64_t* seg_postings,
                           uint32_t n_segs, uint32_t tile_docs, uint32_t* items_out, uint64_t items_cap, uint64_t* n_items_out, uint64_t* ref_out,
                           uint64_t refs_cap, uint64_t* n_refs_out, unsigned char* raw_out, uint32_t* max_need_out, char* err, uint32_t err_cap) {
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
    uint32_t max_need = 0;
    const ns_term_ref* refs = (const ns_term_ref*)refs_in;
    const int rc = which == 2   ? ns::bq_plan(qd.data(), n_queries, refs, roles, n_refs, segs.data(), n_segs, tile_docs, r, it, why)
                   : which == 1 ? ns::bq_plan_grouped(qd.data(), n_queries, refs, roles, clauses, n_refs, segs.data(), n_segs, tile_docs, r, it, why)
                                : ns::bq_plan_quorum(qd.data(), n_queries, refs, roles, clauses, needs, n_refs, segs.data(), n_segs, tile_docs, r, it, max_need, why);
    if (err && err_cap) { std::strncpy(err, why.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    *n_items_out = it.size();
    *n_refs_out = r.size();
    *max_need_out = max_need;
    for (size_t i = 0; i < it.size() && i < items_cap; i++) {
        const uint32_t v[6] = {it[i].query, it[i].seg, it[i].ref_begin, it[i].ref_count, it[i].doc_lo, it[i].doc_hi};
        std::memcpy(items_out + 6 * i, v, sizeof(v));
    }
    for (size_t i = 0; i < r.size() && i < refs_cap; i++) {
        uint32_t a;
        std::memcpy(&a, &r[i].idf, 4);
        const uint64_t v[7] = {r[i].list.first, r[i].list.count, r[i].role, ns::bq_clause_index(r[i].clause), (r[i].clause >> ns::kBqNeedShift) & ns::kBqNeedMask,
                               (r[i].clause & ns::kBqDupBit) ? 1u : 0u, a};
        std::memcpy(ref_out + 7 * i, v, sizeof(v));
        if (raw_out) std::memcpy(raw_out + sizeof(ns::BqRef) * i, &r[i], sizeof(ns::BqRef));
    }
    return rc;
}
extern "C" uint32_t quorum_ref_bytes(void) { return (uint32_t)sizeof(ns::BqRef); }
extern "C" uint32_t quorum_max_need(void) { return ns::kBqMaxNeed; }
