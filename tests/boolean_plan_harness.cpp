// C entry point of the boolean search's planner (nextsearch-api_amd/csrc/ns_boolean_plan.hpp) for
// tests/test_boolean_cpu.py: host code only, compiled with g++ by the test.
#include <cstring>

#include "ns_boolean_plan.hpp"

// bq_plan over the caller's descriptors (qd: n_queries x {term_begin, term_count}; refs: n_refs ns_term_ref; roles: n_refs
// bytes or NULL) and segments (seg_ids / seg_docs / seg_postings: n_segs each, in the call's order; no skip tables), then
// sd_query_items.  items_out: 6 uint32 per item {query, seg, ref_begin, ref_count, doc_lo, doc_hi}; ref_out: 4 uint64 per
// planned ref {first, count, role, fp32 bits of idf | fp32 bits of qweight << 32}; q_off_out: n_queries + 1 entries.
// Returns bq_plan's code, or -100 when sd_query_items refuses; the message goes to err.
extern "C" int boolean_plan(const uint32_t* qd_in, uint32_t n_queries, const void* refs_in, const uint8_t* roles, uint32_t n_refs,
                            const uint32_t* seg_ids, const uint32_t* seg_docs, const uint64_t* seg_postings, uint32_t n_segs, uint32_t tile_docs,
                            uint32_t* items_out, uint64_t items_cap, uint64_t* n_items_out, uint64_t* ref_out, uint64_t refs_cap,
                            uint64_t* n_refs_out, uint32_t* q_off_out, char* err, uint32_t err_cap) {
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
    std::vector<uint32_t> q_off;
    std::string why;
    int rc = ns::bq_plan(qd.data(), n_queries, (const ns_term_ref*)refs_in, roles, n_refs, segs.data(), n_segs, tile_docs, r, it, why);
    if (rc == NS_OK && !ns::sd_query_items(it, n_queries, q_off)) { rc = -100; why = "items are not grouped by query"; }
    if (err && err_cap) { std::strncpy(err, why.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    *n_items_out = it.size();
    *n_refs_out = r.size();
    for (size_t i = 0; i < q_off.size(); i++) q_off_out[i] = q_off[i];
    for (size_t i = 0; i < it.size() && i < items_cap; i++) {
        const uint32_t v[6] = {it[i].query, it[i].seg, it[i].ref_begin, it[i].ref_count, it[i].doc_lo, it[i].doc_hi};
        std::memcpy(items_out + 6 * i, v, sizeof(v));
    }
    for (size_t i = 0; i < r.size() && i < refs_cap; i++) {
        uint32_t a, b;
        std::memcpy(&a, &r[i].idf, 4);
        std::memcpy(&b, &r[i].qweight, 4);
        const uint64_t v[4] = {r[i].list.first, r[i].list.count, r[i].role, (uint64_t)a | ((uint64_t)b << 32)};
        std::memcpy(ref_out + 4 * i, v, sizeof(v));
    }
    return rc;
}
extern "C" uint32_t boolean_win_docs(void) { return ns::kBqWinDocs; }
extern "C" uint32_t boolean_max_win_docs(void) { return ns::kBqMaxWinDocs; }
extern "C" uint32_t boolean_tile_docs(void) { return ns::kFcTileDocs; }
extern "C" int boolean_win_ok(uint32_t w) { return ns::bq_win_ok(w) ? 1 : 0; }
extern "C" uint32_t boolean_role(int which) { return which == 0 ? ns::kBqShould : which == 1 ? ns::kBqMust : ns::kBqNot; }
