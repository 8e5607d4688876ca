// A program of its own for tests/test_related_cpu.py, built with -fsanitize=address,undefined: the plan of
// ns_docterms_aggregate (csrc/ns_terms_plan.hpp) and the host rule (host/related.hpp) over the directed shapes the test writes
// to a file, their answers written back for the test to compare with tests/related_ref.py, and the refusals.
//   related_host_check <shapes.bin> <answers.bin>
// shapes.bin: u64 n_docs, n_pairs, n_terms, n_rows, n_ids; u32 counts[n_docs]; u32 pairs[2 * n_pairs]; u32 df[n_terms];
// f32 idf[n_terms]; u64 row_off[n_rows + 1]; u32 ids[n_ids].  answers.bin, for T = 64 and the default options: u32 term, docs,
// w bits [n_rows * 64 each], count, ndocs [n_rows each].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ns_terms_plan.hpp"
#include "related.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "related_host_check: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

template <class T>
static bool read_vec(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    CHECK(argc == 3);
    std::FILE* f = std::fopen(argv[1], "rb");
    CHECK(f);
    uint64_t hd[5];
    CHECK(std::fread(hd, 8, 5, f) == 5);
    const uint32_t n_docs = (uint32_t)hd[0], n_terms = (uint32_t)hd[2], n_rows = (uint32_t)hd[3];
    std::vector<uint32_t> counts, pairs, df, ids;
    std::vector<float> idf;
    std::vector<uint64_t> row_off;
    CHECK(read_vec(f, counts, n_docs) && read_vec(f, pairs, 2 * hd[1]) && read_vec(f, df, n_terms) && read_vec(f, idf, n_terms) &&
          read_vec(f, row_off, (size_t)n_rows + 1) && read_vec(f, ids, hd[4]));
    std::fclose(f);
    std::vector<uint64_t> off64((size_t)n_docs + 1, 0);
    std::vector<uint32_t> off32((size_t)n_docs + 1, 0);
    for (uint32_t d = 0; d < n_docs; d++) { off64[d + 1] = off64[d] + counts[d]; off32[d + 1] = (uint32_t)off64[d + 1]; }
    CHECK(off64[n_docs] == hd[1]);

    // the plan: every row sorted, without repeats, its pairs summed, the launch order heaviest first
    ns::TermsPlan plan;
    std::string why;
    CHECK(ns::terms_plan(ids.data(), row_off.data(), n_rows, off32.data(), n_docs, plan, why) && why.empty() && plan.over_cap == 0);
    CHECK(plan.first.size() == (size_t)n_rows + 1 && plan.first[0] == 0 && plan.first[n_rows] == plan.docs.size() && plan.order.size() == n_rows);
    std::vector<uint8_t> seen(n_rows, 0);
    for (uint32_t i = 0; i < n_rows; i++) {
        uint64_t sum = 0;
        for (uint32_t j = plan.first[i]; j < plan.first[i + 1]; j++) {
            CHECK(plan.docs[j] < n_docs && (j == plan.first[i] || plan.docs[j - 1] < plan.docs[j]));
            sum += counts[plan.docs[j]];
        }
        CHECK(sum == plan.row_pairs[i] && plan.first[i + 1] - plan.first[i] <= ns::kTaMaxRowDocs);
        CHECK(plan.order[i] < n_rows && !seen[plan.order[i]]);
        seen[plan.order[i]] = 1;
        if (i) CHECK(plan.row_pairs[plan.order[i - 1]] > plan.row_pairs[plan.order[i]] ||
                     (plan.row_pairs[plan.order[i - 1]] == plan.row_pairs[plan.order[i]] && plan.order[i - 1] < plan.order[i]));
    }

    // the rule
    const uint32_t T = 64;
    const nsx::RelatedOptions o;
    std::vector<uint32_t> term((size_t)n_rows * T), docs((size_t)n_rows * T), count(n_rows), ndocs(n_rows);
    std::vector<float> w((size_t)n_rows * T);
    CHECK(nsx::related_aggregate_host(off64.data(), n_docs, pairs.data(), df.data(), idf.data(), n_terms, ids.data(), row_off.data(), n_rows, T, o.min_tf,
                                      o.min_docs, o.min_df, o.max_df, term.data(), docs.data(), w.data(), count.data(), ndocs.data()) == 0);
    for (uint32_t i = 0; i < n_rows; i++) CHECK(ndocs[i] == plan.first[i + 1] - plan.first[i] && count[i] <= T);
    std::FILE* g = std::fopen(argv[2], "wb");
    CHECK(g);
    CHECK(std::fwrite(term.data(), 4, term.size(), g) == term.size() && std::fwrite(docs.data(), 4, docs.size(), g) == docs.size() &&
          std::fwrite(w.data(), 4, w.size(), g) == w.size() && std::fwrite(count.data(), 4, n_rows, g) == n_rows && std::fwrite(ndocs.data(), 4, n_rows, g) == n_rows);
    std::fclose(g);

    // the refusals: 256 distinct documents, 300 ids of 255 documents, a doc id out of range, a bad row_off
    if (n_docs >= 256) {
        std::vector<uint32_t> many(300);
        for (uint32_t i = 0; i < 300; i++) many[i] = i % 255;
        uint64_t ro[3] = {0, 300, 300};
        uint32_t t1[2 * 64], d1[2 * 64], c1[2], n1[2];
        float w1[2 * 64];
        CHECK(ns::terms_plan(many.data(), ro, 2, off32.data(), n_docs, plan, why) && plan.first[1] == 255 && plan.first[2] == 255);
        CHECK(nsx::related_aggregate_host(off64.data(), n_docs, pairs.data(), df.data(), idf.data(), n_terms, many.data(), ro, 2, T, 1, 2, 1, 0xFFFFFFFFu, t1, d1, w1, c1, n1) == 0 &&
              n1[0] == 255 && n1[1] == 0 && c1[1] == 0 && t1[64] == 0xFFFFFFFFu && d1[64] == 0 && w1[64] == 0.0f);
        many[299] = 255;
        CHECK(!ns::terms_plan(many.data(), ro, 2, off32.data(), n_docs, plan, why) && plan.over_cap == 1 && why.find("256 distinct documents") != std::string::npos && plan.docs.empty());
        CHECK(nsx::related_aggregate_host(off64.data(), n_docs, pairs.data(), df.data(), idf.data(), n_terms, many.data(), ro, 2, T, 1, 2, 1, 0xFFFFFFFFu, t1, d1, w1, c1, n1) == -1);
        many[299] = n_docs;
        CHECK(!ns::terms_plan(many.data(), ro, 2, off32.data(), n_docs, plan, why) && why.find("doc_ids[299]") != std::string::npos);
        CHECK(nsx::related_aggregate_host(off64.data(), n_docs, pairs.data(), df.data(), idf.data(), n_terms, many.data(), ro, 2, T, 1, 2, 1, 0xFFFFFFFFu, t1, d1, w1, c1, n1) == -1);
        many[299] = 0;
        uint64_t bad0[3] = {1, 300, 300}, bad1[3] = {0, 300, 299};
        CHECK(!ns::terms_plan(many.data(), bad0, 2, off32.data(), n_docs, plan, why) && why.find("row_off[0]") != std::string::npos);
        CHECK(!ns::terms_plan(many.data(), bad1, 2, off32.data(), n_docs, plan, why) && why.find("row_off[2]") != std::string::npos);
        CHECK(nsx::related_aggregate_host(off64.data(), n_docs, pairs.data(), df.data(), idf.data(), n_terms, many.data(), bad0, 2, T, 1, 2, 1, 0xFFFFFFFFu, t1, d1, w1, c1, n1) == -1);
        CHECK(nsx::related_aggregate_host(off64.data(), n_docs, pairs.data(), df.data(), idf.data(), n_terms, many.data(), bad1, 2, T, 1, 2, 1, 0xFFFFFFFFu, t1, d1, w1, c1, n1) == -1);
    }
    CHECK(ns::terms_plan(nullptr, nullptr, 0, off32.data(), n_docs, plan, why) && plan.first.size() == 1);
    std::printf("related host check OK\n");
    return 0;
}
