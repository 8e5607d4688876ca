// Stand-alone host program (its own main; no HIP, no device): the collapse keys' table builder (host/collapse.hpp) and what
// ns_search_collapsed adds to a ranked call's plan (csrc/ns_collapse_plan.hpp) on the cases of tests/test_collapse_cpu.py, built
// there with -fsanitize=address,undefined and run on the CPU.  Exit status 0 and "collapse host check OK" when every expectation
// holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "collapse.hpp"
#include "ns_boolean_plan.hpp"
#include "ns_call_plan.hpp"
#include "ns_collapse_plan.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static void normalise() {
    EXPECT(nsx::collapse_normalise("The Title: of a PAPER!") == "the title of a paper");
    EXPECT(nsx::collapse_normalise("  the   title of a paper ") == "the title of a paper");
    EXPECT(nsx::collapse_normalise("COVID-19 (SARS/CoV2)") == "covid 19 sars cov2");
    EXPECT(nsx::collapse_normalise("") == "" && nsx::collapse_normalise(" ...!? ") == "" && nsx::collapse_normalise("\xC3\xA9") == "");
    EXPECT(nsx::collapse_normalise("a") == "a" && nsx::collapse_normalise("the") == "the");   // no stop words, no length rule: a title is not a query
    // exact-size heap copies of every prefix: the tokenizer never reads past the end
    const std::string all = "A Long-ish TITLE, with (punctuation) & 123 numbers\xE2\x80\x94" "and bytes above 0x7F";
    for (size_t n = 0; n <= all.size(); n++) {
        const std::string cut(std::vector<char>(all.begin(), all.begin() + n).data(), n);
        const std::string got = nsx::collapse_normalise(cut);
        EXPECT(got.size() <= n && got.find("  ") == std::string::npos && (got.empty() || (got.front() != ' ' && got.back() != ' ')));
    }
}

static void ids() {
    nsx::CollapseIds ids;
    EXPECT(ids.key_of("First title") == 1 && ids.key_of("Second") == 2 && ids.key_of("first TITLE.") == 1 && ids.key_of("") == 0 && ids.key_of("--") == 0);
    EXPECT(ids.key_of("third") == 3 && ids.key_of("second!") == 2 && ids.groups() == 3);
    nsx::CollapseIds many;
    for (uint32_t i = 0; i < 5000; i++) EXPECT(many.key_of("t" + std::to_string(i % 2500)) == 1 + i % 2500);
    EXPECT(many.groups() == 2500);
}

static void custom() {
    std::string err;
    nsx::CollapseSpec s;
    EXPECT(nsx::collapse_check(s, err) && std::strcmp(nsx::collapse_name(s), "title") == 0);
    s.kind = nsx::CollapseSpec::Author;
    EXPECT(std::strcmp(nsx::collapse_name(s), "author") == 0);
    s.kind = (nsx::CollapseSpec::Kind)3;
    EXPECT(!nsx::collapse_check(s, err) && err == "collapse: unknown kind");
    s.kind = nsx::CollapseSpec::Custom;
    EXPECT(std::strcmp(nsx::collapse_name(s), "custom") == 0);
    const std::vector<uint32_t> n_docs{3, 0, 2};
    s.custom = {{1, 0, 0xFFFFFFFEu}, {}, {7, 7}};
    EXPECT(nsx::collapse_custom_check(s, n_docs, err));
    s.custom = {{1, 0, 2}, {}};
    EXPECT(!nsx::collapse_custom_check(s, n_docs, err) && err == "collapse custom: 2 key arrays for 3 segments");
    s.custom = {{1, 0, 2}, {}, {7}};
    EXPECT(!nsx::collapse_custom_check(s, n_docs, err) && err == "collapse custom: the key array of segment 2 has 1 entries, the segment 2 documents");
    s.custom = {{1, 0xFFFFFFFFu, 2}, {}, {7, 7}};
    EXPECT(!nsx::collapse_custom_check(s, n_docs, err) && err == "collapse custom: segment 0 holds the reserved key 0xFFFFFFFF");
}

static std::string first_prefix(const std::string& text) {
    std::vector<char> exact(text.begin(), text.end()), scratch;   // an exact-size heap copy
    return nsx::collapse_first_prefix(exact.data(), exact.size(), scratch);
}

static void prefixes() {
    EXPECT(first_prefix("vaccin*") == "vaccin" && first_prefix("+(covid immun*)~1 vir*^2") == "immun" && first_prefix("-mouse* a1") == "mouse");
    EXPECT(first_prefix("") == "" && first_prefix("vaccine^2 +(a1 b1)~2") == "" && first_prefix("vac*cine x * **") == "" && first_prefix("a*") == "");
    const std::string all = "+(a1 b1*)~2^1.5 -(c1)~3 d1* ~2";
    for (size_t n = 0; n <= all.size(); n++) (void)first_prefix(all.substr(0, n));
}

struct Pair { uint32_t x, y; };

static void plan() {
    // the look-up of the count kernel: every present and absent value around a sorted table of 0, 1, 2 and 128 groups
    for (uint32_t n : {0u, 1u, 2u, 3u, 100u, 128u}) {
        std::vector<Pair> t(n);
        for (uint32_t i = 0; i < n; i++) t[i] = Pair{10u + 3u * i, i};
        for (uint32_t g = 0; g < 10u + 3u * n + 5u; g++) {
            const uint32_t at = ns::cl_lower_bound(t.data(), n, g);
            EXPECT(at <= n && (at == n || t[at].x >= g) && (at == 0 || t[at - 1].x < g));
        }
        EXPECT(ns::cl_lower_bound(t.data(), n, 0xFFFFFFFEu) == n && ns::cl_lower_bound(t.data(), n, 0u) == 0u);
    }
    // the plan: a ranked plan without a cursor, with and without the count pass, over the planes a need can ask for
    std::vector<ns::FcItem> items;
    for (uint32_t q = 0; q < 5; q++)
        for (uint32_t tile = 0; tile < 3; tile++) items.push_back(ns::FcItem{q, 0u, 0u, 1u, tile * 128u, tile * 128u + 128u});
    std::vector<ns::FcSegView> views(1);
    views[0].seg_id = 4; views[0].n_docs = 384; views[0].n_postings = 10;
    ns::RankedPlan rp;
    std::string err;
    EXPECT(ns::ranked_call_plan(items, 5, 1000, nullptr, views, [](uint32_t b) { return b; }, false, 64ull << 20, rp, err) && rp.K == NS_MAX_K && !rp.paged);
    ns::CollapsePlan cp;
    EXPECT(ns::collapse_plan(rp, 5, false, 0, cp, err) && !cp.count && cp.stages == 2 && cp.out_slots == 5u * NS_MAX_K && cp.count_lds == 0);
    EXPECT(ns::collapse_plan(rp, 5, true, 0, cp, err) && cp.count && cp.stages == 3 && cp.count_lds == 0);
    EXPECT(ns::collapse_plan(rp, 5, true, 3, cp, err) && cp.count_lds == 3u * (ns::kFcTileDocs / 8u));
    EXPECT(ns::collapse_plan(rp, 5, false, 3, cp, err) && cp.count_lds == 0);
    EXPECT(!ns::collapse_plan(rp, 5, true, 4, cp, err) && err == "4 counter planes; at most 3");
    ns::ranked_plan_bound_all(items.size(), rp);
    EXPECT(!ns::collapse_plan(rp, 5, true, 0, cp, err) && err == "a collapsed call has no cursor" && !cp.count);
    // the fused subtraction: the join's seed plus the count pass's sum
    EXPECT(ns::cl_others_value(ns::cl_others_seed(9, true), 1) == 0 && ns::cl_others_value(ns::cl_others_seed(9, true), 401) == 400);
    EXPECT(ns::cl_others_value(ns::cl_others_seed(0, true), 0) == 0 && ns::cl_others_seed(9, false) == 0);
}

int main() {
    normalise();
    ids();
    custom();
    prefixes();
    plan();
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::printf("collapse host check OK\n");
    return 0;
}
