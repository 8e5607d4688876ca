// Stand-alone host program (its own main; no HIP, no device): the boosted parser and the decay rule (host/boost.hpp), the scanner's
// fourth dialect (host/boolean.hpp) and the planner's bound for a call without a cursor (csrc/ns_call_plan.hpp) on the cases of
// tests/test_boost_cpu.py, built there with -fsanitize=address,undefined and run on the CPU.  Exit status 0 and "boost host check OK"
// when every expectation holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "boost.hpp"
#include "ns_boolean_plan.hpp"
#include "ns_call_plan.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static std::string weight_text(float w) {
    char buf[32];
    std::snprintf(buf, sizeof(buf), "%g", (double)w);
    return buf;
}

static std::string shown(const std::string& text) {
    uint32_t m = 0;
    std::string o;
    for (const nsx::BoostedTerm& t : nsx::parse_boosted(text, &m))
        o += t.text + ":" + "SMX"[t.role] + std::to_string(t.clause) + "/" + std::to_string(t.need) + (t.promoted ? "p" : "") + "^" + weight_text(t.weight) + " ";
    return o + "~" + std::to_string(m);
}

static void parser() {
    EXPECT(shown("vaccine^2.5") == "vaccine:S0/0^2.5 ~0");
    EXPECT(shown("+vaccine^2.5 covid") == "vaccine:M0/1^2.5 covid:S0/0^1 ~0");
    EXPECT(shown("+(covid sars)^0.5") == "covid:M0/1^0.5 sars:M0/1^0.5 ~0");
    EXPECT(shown("(a1 b1 c1)~2^3") == "a1:M0/2^3 b1:M0/2^3 c1:M0/2^3 ~0");
    EXPECT(shown("-mouse^4 -(rat hamster)^2 a1") == "mouse:X0/0^1 rat:X0/0^1 hamster:X0/0^1 a1:S0/0^1 ~0");
    EXPECT(shown("a1^2 b1 ~2") == "a1:M0/2p^2 b1:M0/2p^1 ~2");
    EXPECT(shown("a1^.5 b1^5. c1^1000000 d1^007") == "a1:S0/0^0.5 b1:S0/0^5 c1:S0/0^1e+06 d1:S0/0^7 ~0");
    EXPECT(shown("+(a1 b1)~2^1.5 c1^2") == "a1:M0/2^1.5 b1:M0/2^1.5 c1:S0/0^2 ~0");
    EXPECT(shown("a1^b1^4") == "a1:S0/0^4 b1:S0/0^4 ~0");
    // no weight: the '^' is the tokenizer's
    EXPECT(shown("ab^") == "ab:S0/0^1 ~0" && shown("ab^0") == "ab:S0/0^1 ~0" && shown("ab^-1") == "ab:S0/0^1 ~0");
    EXPECT(shown("ab^1e3") == "ab:S0/0^1 1e3:S0/0^1 ~0" && shown("ab^1.2.3") == "ab:S0/0^1 ~0" && shown("ab^1000001") == "ab:S0/0^1 1000001:S0/0^1 ~0");
    EXPECT(shown("+(ab cd)^1e3") == "ab:M0/1^1 cd:M0/1^1 1e3:S0/0^1 ~0" && shown("+(ab cd)^") == "ab:M0/1^1 cd:M0/1^1 ~0");
    // a text without '^' is parse_quorum's
    for (const char* text : {"+(coronavirus covid sars) +(vaccine vaccination) -mouse safety", "+(a1 b1 c1)~2", "a1 b1 c1 ~2", "+d1 a1 (b1 c1)~2 -e1 ~1", "+(alpha beta", "+(",
                             "~", "(", ")~2", "+()~3", "a~2", "+(a1)~2~3", "~99999999999999999999 a1", ""}) {
        uint32_t mq = 0, mb = 0;
        const std::vector<nsx::QuorumTerm> q = nsx::parse_quorum(text, &mq);
        const std::vector<nsx::BoostedTerm> b = nsx::parse_boosted(text, &mb);
        EXPECT(q.size() == b.size() && mq == mb);
        for (size_t i = 0; i < q.size() && i < b.size(); i++)
            EXPECT(q[i].text == b[i].text && q[i].role == b[i].role && q[i].clause == b[i].clause && q[i].need == b[i].need && q[i].promoted == b[i].promoted && b[i].weight == 1.0f);
    }
    // every prefix of a text with every form, each an exact-size heap copy (cap 0, 1, ..., the exact fit): the scanner never reads
    // past the end, whether the cut falls inside a weight, behind a '^' or behind a ')'
    const std::string all = "+(a1 b1)~2^1.5 -(c1)~3^2 (d1 e1)^0.25 f1^3 ~2 +g1^2.5 +(h1 i1)^ j1^1.2.3 k1^";
    for (size_t n = 0; n <= all.size(); n++) {
        std::vector<char> exact(all.begin(), all.begin() + n), scratch;
        size_t terms = 0;
        nsx::for_each_boosted_term(exact.data(), exact.size(), scratch, [&](const char*, size_t, uint8_t, uint32_t, uint32_t, float w) { terms++; EXPECT(w > 0.0f && w <= 1e6f); });
        EXPECT(n < 4 || terms >= 1);
    }
    // boost_weight_at on exact-size copies of the shortest texts
    for (const char* text : {"", "^", "^1", "^.", "^1.", "^.1", "^1.1", "^1..1", "^0", "^00.000", "^1000000", "^1000000.0001", "^9999999999999999999999999999999999999999"}) {
        std::vector<char> exact(text, text + std::strlen(text));
        const float w = nsx::boost_weight_at(exact.data(), exact.size(), 0);
        const std::string t(text);
        const bool valid = t == "^1" || t == "^1." || t == "^.1" || t == "^1.1" || t == "^1000000";
        EXPECT((w > 0.0f) == valid);
    }
}

// The scanner's fourth dialect over every string of 0 to 4 bytes of its alphabet, and of 5 and 6 bytes of the suffix's own, each an
// exact-size heap copy: it never reads past the end, every weight lies in (0, 1e6], and without '^' Boosted scans as Quorum.
template <nsx::Dialect D>
static std::string scanned(const std::vector<char>& text, bool& weighted) {
    std::vector<char> scratch;
    std::string o;
    float w = 1.0f;
    const nsx::QuorumShape shape = nsx::for_each_dialect_term<D>(text.data(), text.size(), scratch, [&](const char* p, size_t n, uint8_t role, uint32_t clause, uint32_t need) {
        o += std::string(p, n) + ":" + std::to_string(role) + "." + std::to_string(clause) + "/" + std::to_string(need) + " ";
        EXPECT(w > 0.0f && w <= 1e6f);
        EXPECT(role != nsx::kRoleNot || w == 1.0f);
        weighted = weighted || w != 1.0f;
    }, D == nsx::Dialect::Boosted ? &w : nullptr);
    return o + "#" + std::to_string(shape.n_clauses) + "~" + std::to_string(shape.min_should);
}

static void scan_all(const std::string& alphabet, size_t min_len, size_t max_len, size_t& n_texts, size_t& n_weighted) {
    for (size_t len = min_len; len <= max_len; len++) {
        size_t count = 1;
        for (size_t i = 0; i < len; i++) count *= alphabet.size();
        for (size_t code = 0; code < count; code++) {
            std::vector<char> text(len);
            bool hat = false;
            for (size_t i = 0, c = code; i < len; i++, c /= alphabet.size()) {
                text[i] = alphabet[c % alphabet.size()];
                hat = hat || text[i] == '^';
            }
            n_texts++;
            bool weighted = false, never = false;
            const std::string b = scanned<nsx::Dialect::Boosted>(text, weighted);
            if (!hat) {
                EXPECT(b == scanned<nsx::Dialect::Quorum>(text, never) && !weighted);
            }
            n_weighted += weighted;
        }
    }
}

static void scanner() {
    size_t n_texts = 0, n_weighted = 0;
    scan_all("+-()~^. a12", 0, 4, n_texts, n_weighted);
    EXPECT(n_texts == 1 + 11 + 121 + 1331 + 14641);
    scan_all("^.1 a)", 5, 6, n_texts, n_weighted);
    EXPECT(n_texts == 16105 + 7776 + 46656 && n_weighted > 100);
}

static void decay() {
    EXPECT(nsx::civil_days(1970, 1, 1) == 0 && nsx::civil_days(1969, 12, 31) == -1 && nsx::civil_days(2000, 3, 1) == 11017);
    EXPECT(nsx::civil_days(2020, 2, 29) + 1 == nsx::civil_days(2020, 3, 1) && nsx::civil_days(2100, 2, 28) + 1 == nsx::civil_days(2100, 3, 1));
    EXPECT(nsx::days_of_key(20200000u) == nsx::days_of_key(20200101u) && nsx::days_of_key(20200300u) == nsx::days_of_key(20200301u));
    EXPECT(nsx::days_of_key(99991231u) > nsx::days_of_key(10000u));   // the whole range of a date key
    nsx::BoostSpec s;
    uint32_t origin = 0;
    std::string err;
    s.origin = " 2021-06-15 ";
    EXPECT(nsx::boost_check(s, origin, err) && origin == 20210615u);
    const int64_t at = nsx::days_of_key(origin);
    s.scale_days = 365.0;
    EXPECT(nsx::boost_decay(s, at, 20210615u) == 1.0f && nsx::boost_decay(s, at, 20200615u) == 0.5f && nsx::boost_decay(s, at, 20220615u) == 0.5f);   // |age|, a half-life
    EXPECT(nsx::boost_decay(s, at, 0u) == 1.0f);
    s.undated = 0.25;
    s.weight = 0.5;
    EXPECT(nsx::boost_decay(s, at, 0u) == 0.625f && nsx::boost_decay(s, at, 20200615u) == 0.75f);
    s.kind = nsx::BoostSpec::Linear;
    s.weight = 1.0;
    s.scale_days = 730.0;
    s.offset_days = 10.0;
    EXPECT(nsx::boost_decay(s, at, 20210620u) == 1.0f && nsx::boost_decay(s, at, 20210625u) == 1.0f && nsx::boost_decay(s, at, 20100101u) == 0.0f);
    EXPECT(nsx::boost_decay(s, at, 20200625u) == (float)(1.0 - 345.0 / 730.0));
    s.weight = 0.0;
    EXPECT(nsx::boost_decay(s, at, 20100101u) == 1.0f && nsx::boost_decay(s, at, 0u) == 1.0f);
    // the refusals
    nsx::BoostSpec bad;
    bad.weight = 1.5;
    EXPECT(!nsx::boost_check(bad, origin, err) && err.find("outside [0, 1]") != std::string::npos);
    bad = nsx::BoostSpec{};
    bad.weight = std::nan("");
    EXPECT(!nsx::boost_check(bad, origin, err));
    bad = nsx::BoostSpec{};
    bad.scale_days = 0.0;
    EXPECT(!nsx::boost_check(bad, origin, err) && err.find("scale_days") != std::string::npos);
    bad = nsx::BoostSpec{};
    bad.origin = "2020-13";
    EXPECT(!nsx::boost_check(bad, origin, err) && err.find("is not YYYY, YYYY-MM or YYYY-MM-DD") != std::string::npos);
    bad = nsx::BoostSpec{};
    bad.undated = -1.0;
    EXPECT(!nsx::boost_check(bad, origin, err));
    EXPECT(nsx::boost_factor_ok(0.0f) && nsx::boost_factor_ok(3.0f) && !nsx::boost_factor_ok(-0.0f) && !nsx::boost_factor_ok(-1.0f) && !nsx::boost_factor_ok(INFINITY) && !nsx::boost_factor_ok(NAN));
}

// A boosted call without a cursor: the quorum plan, then the bound that lets every key pass for every item.
static void planner() {
    const ns::FcSegView proto{};
    std::vector<ns::FcSegView> segs(2, proto);
    segs[0].seg_id = 7; segs[0].n_docs = 300; segs[0].n_postings = 1000;
    segs[1].seg_id = 3; segs[1].n_docs = 50; segs[1].n_postings = 1000;
    const std::vector<ns_query_desc> qd = {{0, 3}, {3, 0}, {3, 1}};
    const std::vector<ns_term_ref> refs = {{7, 5, 0, 1.5f, 2.5f}, {7, 6, 80, 1.25f, 2.5f}, {3, 4, 0, 2.0f, 0.5f}, {7, 9, 160, 1.0f, 1.0f}};
    const std::vector<uint8_t> roles = {ns::kBqMust, ns::kBqMust, ns::kBqShould, ns::kBqShould}, needs = {2, 2, 0, 0};
    const std::vector<uint16_t> clauses = {0, 0, 0, 0};
    std::vector<ns::BqRef> out_refs;
    std::vector<ns::FcItem> items;
    uint32_t max_need = 0;
    std::string err;
    EXPECT(ns::bq_plan_quorum(qd.data(), 3, refs.data(), roles.data(), clauses.data(), needs.data(), 4, segs.data(), 2, 128, out_refs, items, max_need, err) == NS_OK);
    EXPECT(max_need == 2 && !items.empty());
    bool weights_kept = false;
    for (const ns::BqRef& r : out_refs) weights_kept = weights_kept || r.qweight == 2.5f;
    EXPECT(weights_kept);   // the `^w` of a piece reaches the kernel as the ref's qweight
    ns::RankedPlan plan;
    EXPECT(ns::ranked_call_plan(items, 3, 10, nullptr, segs, [](uint32_t bits) { return ns::after_ord(bits); }, false, 1u << 20, plan, err));
    EXPECT(!plan.paged && plan.last.empty());
    ns::ranked_plan_bound_all(items.size(), plan);
    EXPECT(plan.paged && plan.last.size() == items.size());
    for (const uint64_t b : plan.last) EXPECT(b == ns::kAfterAll);
    // with a cursor the plan's own bounds stay
    const std::vector<ns_cursor> cur = {{0x3F800000u, 7, 40, 1}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    ns::RankedPlan paged;
    EXPECT(ns::ranked_call_plan(items, 3, 10, cur.data(), segs, [](uint32_t bits) { return ns::after_ord(bits); }, false, 1u << 20, paged, err));
    const std::vector<uint64_t> before = paged.last;
    ns::ranked_plan_bound_all(items.size(), paged);
    EXPECT(paged.paged && paged.last == before && before.size() == items.size() && before[0] != ns::kAfterAll);
    // no item at all
    ns::RankedPlan none;
    const std::vector<ns::FcItem> no_items;
    EXPECT(ns::ranked_call_plan(no_items, 3, 10, nullptr, segs, [](uint32_t bits) { return ns::after_ord(bits); }, false, 1u << 20, none, err));
    ns::ranked_plan_bound_all(0, none);
    EXPECT(none.paged && none.last.empty());
}

int main() {
    parser();
    scanner();
    decay();
    planner();
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("boost host check OK");
    return 0;
}
