// The host-only plan of ns_docterms_aggregate (csrc/ns_terms_plan.hpp) behind a C function for tests/test_related_cpu.py:
// compiled with g++ alone, no HIP header in sight.
#include <cstdint>
#include <cstring>
#include <string>

#include "ns_terms_plan.hpp"

extern "C" uint32_t terms_plan_max_row_docs() { return ns::kTaMaxRowDocs; }

// 1 planned, 0 refused (err holds the message).  docs_out[cap] / *n_docs_out: the flat de-duplicated list; first_out[n_rows + 1],
// row_pairs_out[n_rows], order_out[n_rows]; *over_cap_out: rows over the cap
extern "C" int terms_plan_run(const uint32_t* doc_ids, const uint64_t* row_off, uint32_t n_rows, const uint32_t* doc_off, uint32_t n_docs,
                              uint32_t* docs_out, uint64_t cap, uint64_t* n_docs_out, uint32_t* first_out, uint64_t* row_pairs_out,
                              uint32_t* order_out, uint32_t* over_cap_out, char* err, uint32_t err_cap) {
    ns::TermsPlan p;
    std::string why;
    const bool ok = ns::terms_plan(doc_ids, row_off, n_rows, doc_off, n_docs, p, why);
    if (err && err_cap) { std::strncpy(err, why.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    *over_cap_out = p.over_cap;
    *n_docs_out = p.docs.size();
    if (!ok) return 0;
    if (p.docs.size() > cap) return -1;
    if (!p.docs.empty()) std::memcpy(docs_out, p.docs.data(), p.docs.size() * 4);
    std::memcpy(first_out, p.first.data(), p.first.size() * 4);
    if (n_rows) {
        std::memcpy(row_pairs_out, p.row_pairs.data(), (size_t)n_rows * 8);
        std::memcpy(order_out, p.order.data(), (size_t)n_rows * 4);
    }
    return 1;
}
