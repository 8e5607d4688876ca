// Stand-alone host program (its own main; no HIP, no device): the quorum planner (csrc/ns_boolean_plan.hpp bq_plan_quorum) and parser
// (host/quorum.hpp parse_quorum) on the cases of tests/test_quorum_cpu.py, built there with -fsanitize=address,undefined and run
// on the CPU.  Exit status 0 and "quorum host check OK" when every expectation holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ns_boolean_plan.hpp"
#include "quorum.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

struct In { uint32_t seg, count; uint64_t off; uint8_t role; uint16_t clause; uint8_t need; };

struct Planned {
    int rc;
    std::vector<ns::BqRef> refs;
    std::vector<ns::FcItem> items;
    uint32_t max_need;
    std::string err;
};

static Planned plan(const std::vector<std::vector<In>>& queries, bool with_clauses, bool with_needs, uint32_t tile = 128) {
    const ns::FcSegView proto{};
    std::vector<ns::FcSegView> segs(3, proto);
    const uint32_t ids[3] = {7, 3, 9}, docs[3] = {100, 50, 10};
    for (int i = 0; i < 3; i++) { segs[i].seg_id = ids[i]; segs[i].n_docs = docs[i]; segs[i].n_postings = 1000; }
    std::vector<ns_query_desc> qd;
    std::vector<ns_term_ref> refs;
    std::vector<uint8_t> roles, needs;
    std::vector<uint16_t> clauses;
    for (const auto& q : queries) {
        qd.push_back(ns_query_desc{(uint32_t)refs.size(), (uint32_t)q.size()});
        for (const In& r : q) {
            refs.push_back(ns_term_ref{r.seg, r.count, r.off, 1.0f + (float)refs.size(), 0.5f});
            roles.push_back(r.role);
            clauses.push_back(r.clause);
            needs.push_back(r.need);
        }
    }
    // exact-size heap copies: a read past n_refs is a heap-buffer-overflow
    Planned p;
    p.rc = ns::bq_plan_quorum(qd.data(), (uint32_t)qd.size(), refs.data(), roles.data(), with_clauses ? clauses.data() : nullptr, with_needs ? needs.data() : nullptr,
                              (uint32_t)refs.size(), segs.data(), 3, tile, p.refs, p.items, p.max_need, p.err);
    return p;
}

static void planner() {
    const uint8_t M = ns::kBqMust, S = ns::kBqShould, X = ns::kBqNot;
    // needs == nullptr: bq_plan_grouped's bytes (the wrapper and its callee under the sanitizers; the bytes themselves are pinned by the
    // recorded expectations of the grouped and boolean plan tests)
    const std::vector<std::vector<In>> mixed = {{{3, 5, 80, M, 1, 2}, {7, 6, 0, S, 2, 0}, {9, 2, 160, X, 3, 0}, {3, 4, 240, M, 1, 2}, {7, 6, 0, M, 7, 1}, {3, 2, 0, M, 2, 0}},
                                                {{7, 0, 0, M, 1, 1}, {7, 3, 0, S, 1, 0}, {3, 3, 0, M, 9, 1}}};
    {
        const Planned a = plan(mixed, true, false, 32);
        std::vector<ns::BqRef> r;
        std::vector<ns::FcItem> it;
        std::string why;
        // the same call through bq_plan_grouped
        std::vector<ns_query_desc> qd;
        std::vector<ns_term_ref> refs;
        std::vector<uint8_t> roles;
        std::vector<uint16_t> clauses;
        for (const auto& q : mixed) {
            qd.push_back(ns_query_desc{(uint32_t)refs.size(), (uint32_t)q.size()});
            for (const In& x : q) { refs.push_back(ns_term_ref{x.seg, x.count, x.off, 1.0f + (float)refs.size(), 0.5f}); roles.push_back(x.role); clauses.push_back(x.clause); }
        }
        const ns::FcSegView proto{};
        std::vector<ns::FcSegView> segs(3, proto);
        const uint32_t ids[3] = {7, 3, 9}, docs[3] = {100, 50, 10};
        for (int i = 0; i < 3; i++) { segs[i].seg_id = ids[i]; segs[i].n_docs = docs[i]; segs[i].n_postings = 1000; }
        const int rc = ns::bq_plan_grouped(qd.data(), (uint32_t)qd.size(), refs.data(), roles.data(), clauses.data(), (uint32_t)refs.size(), segs.data(), 3, 32, r, it, why);
        EXPECT(rc == NS_OK && a.rc == NS_OK && a.max_need == 0);
        EXPECT(r.size() == a.refs.size() && it.size() == a.items.size());
        EXPECT(r.size() == a.refs.size() && std::memcmp(r.data(), a.refs.data(), r.size() * sizeof(ns::BqRef)) == 0);
        EXPECT(it.size() == a.items.size() && std::memcmp(it.data(), a.items.data(), it.size() * sizeof(ns::FcItem)) == 0);
    }
    {   // the need and the duplicate bit; the largest need
        const Planned p = plan({{{7, 5, 0, M, 4, 2}, {7, 5, 0, M, 4, 2}, {7, 6, 80, M, 4, 2}, {7, 5, 0, M, 9, 0}, {7, 3, 160, S, 4, 200}}}, true, true);
        EXPECT(p.rc == NS_OK && p.refs.size() == 5 && p.items.size() == 1 && p.max_need == 2);
        if (p.refs.size() == 5) {
            EXPECT(p.refs[0].clause == ns::bq_clause_word(0, 2, false) && p.refs[1].clause == ns::bq_clause_word(0, 2, true) && p.refs[2].clause == ns::bq_clause_word(0, 2, false));
            EXPECT(p.refs[3].clause == ns::bq_clause_word(1, 1, false) && p.refs[4].clause == 0u);
        }
    }
    {   // the dead-group rule: need above the distinct live members, in one segment only
        const Planned p = plan({{{7, 5, 0, M, 1, 2}, {7, 5, 0, M, 1, 2}, {7, 0, 80, M, 1, 2}, {3, 5, 0, M, 1, 2}, {3, 4, 80, M, 1, 2}}}, true, true);
        EXPECT(p.rc == NS_OK && p.items.size() == 1 && p.refs.size() == 2 && p.max_need == 2);
        const Planned one = plan({{{7, 5, 0, M, 1, 2}}, {{7, 5, 0, M, 1, 1}}}, true, true);
        EXPECT(one.rc == NS_OK && one.items.size() == 1 && one.items[0].query == 1 && one.items[0].ref_count == 1 && one.max_need == 1);
    }
    {   // the refusals
        const Planned eight = plan({{{7, 5, 0, M, 1, 8}}}, true, true);
        EXPECT(eight.rc == NS_E_INVAL && eight.refs.empty() && eight.items.empty() && eight.err.find("a need of 8") != std::string::npos);
        const Planned differ = plan({{{7, 5, 0, M, 1, 2}}, {{7, 5, 0, M, 1, 2}, {7, 6, 80, M, 1, 3}}}, true, true);
        EXPECT(differ.rc == NS_E_INVAL && differ.err.find("query 1: the refs of clause 1 carry the needs 2 and 3") != std::string::npos);
        const Planned bare = plan({{{7, 5, 0, M, 1, 2}}}, false, true);
        EXPECT(bare.rc == NS_E_INVAL && bare.err.find("needs without clauses") != std::string::npos);
        const Planned ok = plan({{{7, 5, 0, S, 1, 255}, {7, 5, 0, X, 1, 9}, {7, 5, 0, M, 1, 7}}}, true, true);
        EXPECT(ok.rc == NS_OK && ok.items.empty());   // needs on SHOULD and NOT refs are not read; seven of one list is a dead group, not a refusal
    }
}

static std::string shown(const std::string& text) {
    uint32_t m = 0;
    std::string o;
    for (const nsx::QuorumTerm& t : nsx::parse_quorum(text, &m))
        o += t.text + ":" + "SMX"[t.role] + std::to_string(t.clause) + "/" + std::to_string(t.need) + (t.promoted ? "p " : " ");
    return o + "~" + std::to_string(m);
}

static void parser() {
    EXPECT(shown("+(a1 b1 c1)~2") == "a1:M0/2 b1:M0/2 c1:M0/2 ~0");
    EXPECT(shown("(a1 b1 c1)~2") == "a1:M0/2 b1:M0/2 c1:M0/2 ~0");
    EXPECT(shown("-(a1 b1)~2") == "a1:X0/0 b1:X0/0 ~0");
    EXPECT(shown("a1 b1 c1 ~2") == "a1:M0/2p b1:M0/2p c1:M0/2p ~2");
    EXPECT(shown("a1 b1 ~2 c1 ~0") == "a1:S0/0 b1:S0/0 c1:S0/0 ~0");
    EXPECT(shown("+(a1 b1)~") == "a1:M0/1 b1:M0/1 ~0");
    EXPECT(shown("+(a1 b1)~xy") == "a1:M0/1 b1:M0/1 xy:S0/0 ~0");
    EXPECT(shown("~12 a1") == "a1:M0/12p ~12");
    EXPECT(shown("+d1 a1 (b1 c1)~2 ~1") == "d1:M0/1 a1:M2/1p b1:M1/2 c1:M1/2 ~1");
    EXPECT(shown("~99999999999999999999") == "~1000000");
    for (const char* text : {"+(coronavirus covid sars) +(vaccine vaccination) -mouse safety", "+(alpha beta", "+(", "~", "(", ")~2", "+()~3", "a~2", "+(a1)~2~3", ""}) {
        const std::vector<nsx::GroupedTerm> g = nsx::parse_grouped(text);
        const std::vector<nsx::QuorumTerm> q = nsx::parse_quorum(text);
        if (std::string(text).find('~') != std::string::npos) continue;   // (parsed above for the sanitizers' sake)
        EXPECT(g.size() == q.size());
        for (size_t i = 0; i < g.size() && i < q.size(); i++)
            EXPECT(g[i].text == q[i].text && g[i].role == q[i].role && g[i].clause == q[i].clause && q[i].need == (g[i].role == nsx::kRoleMust ? 1u : 0u) && !q[i].promoted);
    }
    // every prefix of a text with every form: the scanner never reads past the end (the string is an exact-size heap copy)
    const std::string all = "+(a1 b1)~2 -(c1)~3 (d1 e1)~1 f1 ~2 +(g1 h1)~";
    for (size_t n = 0; n <= all.size(); n++) {
        std::vector<char> exact(all.begin(), all.begin() + n), scratch;
        nsx::for_each_quorum_term(exact.data(), exact.size(), scratch, [](const char*, size_t, uint8_t, uint32_t, uint32_t) {});
    }
}

// The one scanner (host/boolean.hpp) in all three dialects over every string of 0 to 5 bytes of the grammar's own alphabet, each
// an exact-size heap copy: it never reads past the end, and the dialects are nested (without '(' Grouped scans as Boolean,
// without '~' Quorum scans as Grouped).
template <nsx::Dialect D>
static std::string scanned(const std::vector<char>& text, bool clauses, bool needs) {
    std::vector<char> scratch;
    std::string o;
    const nsx::QuorumShape shape = nsx::for_each_dialect_term<D>(text.data(), text.size(), scratch, [&](const char* p, size_t n, uint8_t role, uint32_t clause, uint32_t need) {
        o += std::string(p, n) + ":" + std::to_string(role);
        if (clauses) o += "." + std::to_string(clause);
        if (needs) o += "/" + std::to_string(need);
        o += " ";
    });
    if (clauses) o += "#" + std::to_string(shape.n_clauses);
    if (needs) o += "~" + std::to_string(shape.min_should);
    return o;
}

static void scanner() {
    const std::string alphabet = "+-()~ a12";
    size_t n_texts = 0;
    for (size_t len = 0; len <= 5; len++) {
        size_t count = 1;
        for (size_t i = 0; i < len; i++) count *= alphabet.size();
        for (size_t code = 0; code < count; code++) {
            std::vector<char> text(len);
            bool paren = false, tilde = false;
            for (size_t i = 0, c = code; i < len; i++, c /= alphabet.size()) {
                text[i] = alphabet[c % alphabet.size()];
                paren = paren || text[i] == '(';
                tilde = tilde || text[i] == '~';
            }
            n_texts++;
            // every text through every dialect; what a dialect says of a text that its smaller sibling reads alike is compared
            const std::string b = scanned<nsx::Dialect::Boolean>(text, false, false);
            const std::string g = scanned<nsx::Dialect::Grouped>(text, true, false), g_terms = scanned<nsx::Dialect::Grouped>(text, false, false);
            const std::string q = scanned<nsx::Dialect::Quorum>(text, true, true), q_clauses = scanned<nsx::Dialect::Quorum>(text, true, false);
            EXPECT(b.empty() == g_terms.empty() || paren);
            if (!paren) EXPECT(b == g_terms);
            if (!tilde) EXPECT(g == q_clauses && q.size() >= 2 && q.compare(q.size() - 2, 2, "~0") == 0);   // and no `~m` piece
        }
    }
    EXPECT(n_texts == 66430);
}

int main() {
    planner();
    parser();
    scanner();
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("quorum host check OK");
    return 0;
}
