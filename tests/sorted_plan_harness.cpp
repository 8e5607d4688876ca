// C entry point of the sorted search's planner additions (nextsearch-api_amd/csrc/ns_sorted_plan.hpp) for
// tests/test_sorted_cpu.py: host code only, compiled with g++ by the test.
#include <cstring>

#include "ns_sorted_plan.hpp"

// One (query, segment) group per query over `tiles[q]` tiles of tile_docs documents each (0: the query has no refs), cut by
// fc_plan; then sd_query_items and sd_cut at K and cand_bytes.  q_off_out: n_queries + 1 entries.  batches_out: 4 uint32 per
// sub-batch {q_begin, q_end, item_begin, item_end}.  item_query_out (capacity items_cap): the query of every item.
// Returns fc_plan's / sd_cut's code, or -100 when sd_query_items refuses; the message goes to err.
extern "C" int sorted_plan(const uint32_t* tiles, uint32_t n_queries, uint32_t tile_docs, uint32_t K, uint64_t cand_bytes, uint32_t* q_off_out,
                           uint32_t* batches_out, uint64_t batches_cap, uint64_t* n_batches_out, uint32_t* item_query_out, uint64_t items_cap,
                           uint64_t* n_items_out, char* err, uint32_t err_cap) {
    std::vector<ns::FcSegView> segs(n_queries);
    std::vector<ns_query_desc> qd(n_queries);
    std::vector<ns_term_ref> refs;
    for (uint32_t q = 0; q < n_queries; q++) {   // segment q has tiles[q] tiles (the last one a document short) and 4 postings
        segs[q].seg_id = q;
        segs[q].n_docs = tiles[q] ? tiles[q] * tile_docs - 1 : 0;
        segs[q].n_postings = 4;
        qd[q] = ns_query_desc{(uint32_t)refs.size(), tiles[q] ? 1u : 0u};
        if (tiles[q]) refs.push_back(ns_term_ref{q, 4, 0, 1.0f, 1.0f});
    }
    std::vector<ns::FcRef> r;
    std::vector<ns::FcItem> it;
    std::vector<uint32_t> q_off;
    std::vector<ns::SdBatch> cuts;
    std::string why;
    int rc = ns::fc_plan(qd.data(), n_queries, refs.data(), (uint32_t)refs.size(), false, segs.data(), n_queries, tile_docs, r, it, why);
    if (rc == NS_OK && !ns::sd_query_items(it, n_queries, q_off)) { rc = -100; why = "items are not grouped by query"; }
    if (rc == NS_OK) rc = ns::sd_cut(q_off, n_queries, K, cand_bytes, cuts, why);
    if (err && err_cap) { std::strncpy(err, why.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    *n_items_out = it.size();
    *n_batches_out = cuts.size();
    for (size_t i = 0; i < q_off.size(); i++) q_off_out[i] = q_off[i];
    for (size_t i = 0; i < it.size() && i < items_cap; i++) item_query_out[i] = it[i].query;
    for (size_t i = 0; i < cuts.size() && i < batches_cap; i++) {
        const uint32_t v[4] = {cuts[i].q_begin, cuts[i].q_end, cuts[i].item_begin, cuts[i].item_end};
        std::memcpy(batches_out + 4 * i, v, sizeof(v));
    }
    return rc;
}
// items given out of query order: sd_query_items must say no
extern "C" int sorted_plan_refuses_unordered(void) {
    std::vector<ns::FcItem> it = {ns::FcItem{1, 0, 0, 1, 0, 8}, ns::FcItem{0, 0, 0, 1, 0, 8}};
    std::vector<uint32_t> q_off;
    return ns::sd_query_items(it, 2, q_off) ? 0 : 1;
}
extern "C" uint64_t sorted_cand_bytes(void) { return ns::kSdCandBytes; }
extern "C" uint32_t sorted_asc_flag(void) { return ns::kSdAscFlag; }
