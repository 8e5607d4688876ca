// C entry points over csrc/ns_call_plan.hpp for tests/test_call_plan_cpu.py (built by g++ inside the test; no HIP, no device).
// With -DCALL_PLAN_MAIN it is a program of its own that runs the test's directed shapes against values written out by hand,
// for a run under the host sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ns_call_plan.hpp"

namespace {

std::vector<ns::FcItem> items_of(const uint32_t* rows, uint64_t n) {   // rows[i * 4 ..] = query, segment position, doc_lo, doc_hi
    std::vector<ns::FcItem> it(n);
    for (uint64_t i = 0; i < n; i++) it[i] = ns::FcItem{rows[i * 4], rows[i * 4 + 1], (uint32_t)i, 1u, rows[i * 4 + 2], rows[i * 4 + 3]};
    return it;
}

// rank_map 0: after_ord (the ranked boolean search), 1: after_sort_rank newest first, 2: oldest first
bool plan(const std::vector<ns::FcItem>& items, uint32_t n_queries, uint32_t k, const ns_cursor* after, const std::vector<ns::FcSegView>& views,
          int rank_map, bool reserved_rank, uint64_t cand_bytes, ns::RankedPlan& out, std::string& err) {
    if (rank_map == 0) return ns::ranked_call_plan(items, n_queries, k, after, views, [](uint32_t bits) { return ns::after_ord(bits); }, reserved_rank, cand_bytes, out, err);
    const bool asc = rank_map == 2;
    return ns::ranked_call_plan(items, n_queries, k, after, views, [asc](uint32_t key) { return ns::after_sort_rank(key, asc); }, reserved_rank, cand_bytes, out, err);
}

}  // namespace

extern "C" {

// cursors: NULL, or per query rank, seg_id, doc_id, set.  q_off_out: n_queries + 1 entries; cuts_out: 4 uint32 per cut
// {q_begin, q_end, item_begin, item_end}, cuts_cap of them; last_out: n_items entries.  scalars_out: K, paged, number of cuts,
// entries of last, cand_rows.  Returns 1, or 0 with the refusal's text in err.
int call_plan(const uint32_t* item_rows, uint64_t n_items, uint32_t n_queries, uint32_t k, const uint32_t* cursors, const uint32_t* seg_ids, uint32_t n_segs,
              int rank_map, int reserved_rank, uint64_t cand_bytes, uint32_t* q_off_out, uint32_t* cuts_out, uint64_t cuts_cap, uint64_t* last_out,
              uint64_t* scalars_out, char* err, uint32_t err_cap) {
    const std::vector<ns::FcItem> items = items_of(item_rows, n_items);
    std::vector<ns::FcSegView> views(n_segs);
    for (uint32_t i = 0; i < n_segs; i++) views[i].seg_id = seg_ids[i];
    std::vector<ns_cursor> after;
    for (uint32_t q = 0; cursors && q < n_queries; q++) after.push_back(ns_cursor{cursors[q * 4], cursors[q * 4 + 1], cursors[q * 4 + 2], cursors[q * 4 + 3]});
    ns::RankedPlan p;
    std::string why;
    const bool ok = plan(items, n_queries, k, cursors ? after.data() : nullptr, views, rank_map, reserved_rank != 0, cand_bytes, p, why);
    if (err && err_cap) { std::strncpy(err, why.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    if (!ok) return 0;
    for (size_t i = 0; i < p.q_off.size(); i++) q_off_out[i] = p.q_off[i];
    for (size_t i = 0; i < p.cuts.size() && i < cuts_cap; i++) {
        const uint32_t v[4] = {p.cuts[i].q_begin, p.cuts[i].q_end, p.cuts[i].item_begin, p.cuts[i].item_end};
        std::memcpy(cuts_out + 4 * i, v, sizeof(v));
    }
    for (size_t i = 0; i < p.last.size(); i++) last_out[i] = p.last[i];
    scalars_out[0] = p.K;
    scalars_out[1] = p.paged ? 1 : 0;
    scalars_out[2] = p.cuts.size();
    scalars_out[3] = p.last.size();
    scalars_out[4] = p.cand_rows;
    return 1;
}

// the item limit of every call: 1, or 0 with the text in err
int call_item_limit_c(uint64_t n_items, char* err, uint32_t err_cap) {
    std::string why;
    const bool ok = ns::call_item_limit(n_items, why);
    if (err && err_cap) { std::strncpy(err, why.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    return ok ? 1 : 0;
}

uint64_t call_cand_bytes(void) { return ns::kSdCandBytes; }
uint32_t call_max_k(void) { return NS_MAX_K; }

}  // extern "C"

#ifdef CALL_PLAN_MAIN
// The shapes of tests/test_call_plan_cpu.py: three segments listed as ids {7, 3, 9}, tiles of 32 documents, query 0 with three
// items, query 1 with none, query 2 with three.
static int g_bad = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { std::printf("call_plan_harness: WRONG: %s\n", what); g_bad++; }
}

int main() {
    const uint32_t rows[6 * 4] = {0, 0, 0, 32, 0, 0, 32, 50, 0, 1, 0, 32, 2, 0, 0, 32, 2, 0, 32, 50, 2, 2, 0, 20};
    const std::vector<ns::FcItem> items = items_of(rows, 6);
    std::vector<ns::FcSegView> views(3);
    views[0].seg_id = 7; views[1].seg_id = 3; views[2].seg_id = 9;
    const uint64_t big = ns::kSdCandBytes;
    ns::RankedPlan p;
    std::string why;

    // no cursor at all
    expect(plan(items, 3, 10, nullptr, views, 0, false, big, p, why), "no cursor: accepted");
    expect(p.K == 10 && !p.paged && p.last.empty() && p.cand_rows == 6, "no cursor: K, paged, last, cand_rows");
    expect(p.q_off == std::vector<uint32_t>({0, 3, 3, 6}), "no cursor: q_off with an empty query in the middle");
    expect(p.cuts.size() == 1 && p.cuts[0].q_begin == 0 && p.cuts[0].q_end == 3 && p.cuts[0].item_begin == 0 && p.cuts[0].item_end == 6, "no cursor: one cut");

    // a cursor on query 2 of three: rank 5 newest first, segment 7 (position 0), document 40
    ns_cursor after[3] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {5, 7, 40, 1}};
    expect(plan(items, 3, 10, after, views, 1, true, big, p, why), "one cursor: accepted");
    expect(p.paged && p.last.size() == 6, "one cursor: paged, one bound per item");
    expect(p.last[0] == ns::kAfterAll && p.last[1] == ns::kAfterAll && p.last[2] == ns::kAfterAll, "one cursor: the other query's items take everything");
    expect(p.last[3] == ((4ull << 32) | 0xFFFFFFFFull), "one cursor: the tile before the cursor's takes lower ranks only");
    expect(p.last[4] == ((5ull << 32) | (uint32_t)~9u), "one cursor: the cursor's tile takes ties from document 41 on");
    expect(p.last[5] == ((5ull << 32) | 0xFFFFFFFFull), "one cursor: a later segment takes ties");

    // refusals
    after[2] = ns_cursor{5, 5, 40, 1};
    expect(!plan(items, 3, 10, after, views, 1, true, big, p, why) && why == "query 2: cursor names segment 5, which the call does not list", "unlisted segment");
    after[2] = ns_cursor{5, 7, 40, 1};
    after[0] = ns_cursor{1, 7, 0, 2};
    expect(!plan(items, 3, 10, after, views, 1, true, big, p, why) && why == "query 0: cursor with set = 2 (0 or 1)", "set = 2");
    after[0] = ns_cursor{0, 0, 0, 0};
    after[2] = ns_cursor{0xFFFFFFFFu, 7, 40, 1};
    expect(!plan(items, 3, 10, after, views, 2, true, big, p, why) && why == "query 2: cursor with the reserved key 0xFFFFFFFF", "reserved key refused");
    expect(plan(items, 3, 10, after, views, 0, false, big, p, why) && p.paged, "0xFFFFFFFF is an ordinary score without reserved_rank");
    expect(p.last[3] == 0 && p.last[4] == (uint32_t)~9u && p.last[5] == 0xFFFFFFFFull, "after_ord(0xFFFFFFFF) = 0: nothing below it");

    // k is clamped
    expect(plan(items, 3, 0, nullptr, views, 0, false, big, p, why) && p.K == 1, "k = 0");
    expect(plan(items, 3, 1000, nullptr, views, 0, false, big, p, why) && p.K == NS_MAX_K, "k = 1000");

    // a budget of three rows at K = 10: two cuts; of two rows: query 0 alone does not fit
    expect(plan(items, 3, 10, after, views, 0, false, 240, p, why) && p.cuts.size() == 2 && p.cand_rows == 3, "two cuts");
    expect(p.cuts[0].q_begin == 0 && p.cuts[0].q_end == 2 && p.cuts[0].item_end == 3 && p.cuts[1].q_begin == 2 && p.cuts[1].q_end == 3 && p.cuts[1].item_begin == 3 && p.cuts[1].item_end == 6, "the cuts");
    expect(p.last.size() == 6, "last stays per item of the call");
    expect(!plan(items, 3, 10, nullptr, views, 0, false, 160, p, why) && why == "query 0 alone has 3 work items; the candidate buffer of 160 bytes holds 2 rows at K = 10", "a query too large");

    // items out of query order, and the item limit
    const uint32_t mixed[2 * 4] = {1, 0, 0, 32, 0, 0, 0, 32};
    expect(!plan(items_of(mixed, 2), 2, 10, nullptr, views, 0, false, big, p, why) && why == "the work items are not grouped by query", "not grouped");
    expect(ns::call_item_limit((1ull << 31) - 1, why) && !ns::call_item_limit(1ull << 31, why) && why == "2147483648 work items; cut the batch", "item limit");

    std::printf("call_plan_harness: %d wrong\n", g_bad);
    return g_bad ? 1 : 0;
}
#endif
