// Related terms: the rows of ns_docterms_aggregate -> what k_ta_count reads.  Host code only, like
// ns_facet_plan.hpp and ns_call_plan.hpp: no HIP runtime call and no device pointer; tests/terms_plan_harness.cpp compiles it
// with g++ for the CPU suite.  The rule is host/related.hpp's.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

namespace ns {

// Distinct documents of a row: k_ta_count counts them in one BYTE per term id, which must not carry into its neighbour.
static constexpr uint32_t kTaMaxRowDocs = 255;

struct TermsPlan {
    std::vector<uint32_t> docs;        // every row's distinct doc ids, ascending inside a row, rows in the caller's order
    std::vector<uint32_t> first;       // n_rows + 1: row i is docs[first[i], first[i + 1])
    std::vector<uint64_t> row_pairs;   // n_rows: the forward pairs of the row's documents together
    std::vector<uint32_t> order;       // n_rows: the rows in launch order, heaviest first (ties: the smaller row first)
    uint32_t over_cap = 0;             // rows that named more than kTaMaxRowDocs distinct documents (a refused call)
};

inline std::string ta_format(const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}

// Checks row_off (starting at 0, never descending) and every doc id (< n_docs), sorts and de-duplicates each row, refuses a
// row of more than kTaMaxRowDocs distinct documents.  doc_off[n_docs + 1]: the handle's document offsets.  true, or false
// with `err` set and nothing usable in the plan (over_cap counts the rows over the cap all the same).
inline bool terms_plan(const uint32_t* doc_ids, const uint64_t* row_off, uint32_t n_rows, const uint32_t* doc_off, uint32_t n_docs,
                       TermsPlan& p, std::string& err) {
    p.docs.clear(); p.first.assign((size_t)n_rows + 1, 0u); p.row_pairs.assign(n_rows, 0ull); p.order.clear(); p.over_cap = 0;
    err.clear();
    auto refuse = [&](std::string why) { if (err.empty()) err = std::move(why); };
    if (n_rows && row_off[0] != 0) refuse(ta_format("row_off[0] = %llu, not 0", (unsigned long long)row_off[0]));
    for (uint32_t i = 0; i < n_rows && err.empty(); i++)
        if (row_off[i + 1] < row_off[i])
            refuse(ta_format("row_off[%u] = %llu is below row_off[%u] = %llu", i + 1, (unsigned long long)row_off[i + 1], i, (unsigned long long)row_off[i]));
    if (!err.empty()) return false;
    std::vector<uint32_t> ids;
    for (uint32_t i = 0; i < n_rows; i++) {
        bool bad_id = false;
        for (uint64_t j = row_off[i]; j < row_off[i + 1] && !bad_id; j++)
            if (doc_ids[j] >= n_docs) {
                refuse(ta_format("doc_ids[%llu] = %u (row %u), the handle holds %u documents", (unsigned long long)j, doc_ids[j], i, n_docs));
                bad_id = true;
            }
        if (bad_id) break;                                              // (a bad id ends the planning; rows over the cap are all counted)
        ids.assign(doc_ids + row_off[i], doc_ids + row_off[i + 1]);
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        if (ids.size() > kTaMaxRowDocs) {
            p.over_cap++;
            refuse(ta_format("row %u names %llu distinct documents; a row holds at most %u", i, (unsigned long long)ids.size(), kTaMaxRowDocs));
            continue;
        }
        if (!err.empty()) continue;                                     // (only counting the rows over the cap from here on)
        for (const uint32_t d : ids) p.row_pairs[i] += doc_off[d + 1] - doc_off[d];
        p.docs.insert(p.docs.end(), ids.begin(), ids.end());
        if (p.docs.size() > 0xFFFFFFFFull) { refuse("more than 2^32 - 1 documents in all rows together"); return false; }
        p.first[i + 1] = (uint32_t)p.docs.size();
    }
    if (!err.empty()) { p.docs.clear(); p.first.assign((size_t)n_rows + 1, 0u); p.row_pairs.assign(n_rows, 0ull); return false; }
    p.order.resize(n_rows);
    std::iota(p.order.begin(), p.order.end(), 0u);
    std::stable_sort(p.order.begin(), p.order.end(), [&](uint32_t a, uint32_t b) { return p.row_pairs[a] > p.row_pairs[b]; });
    return true;
}

}  // namespace ns
