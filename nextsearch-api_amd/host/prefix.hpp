// Prefix terms: what `vaccin*` is on the host.
//
// parse_prefixed reads parse_boosted's dialect (boost.hpp) plus the prefix term:
//     vaccin*   +vaccin*   -mouse*   +(vaccin* immun*)~1   vir*^2.5
// A '*' directly behind a token's last byte marks that token as a PREFIX, provided the next byte is not alphanumeric or the text
// ends there; inside or outside a group, and before a `^w`.  Every other '*' stays a separator (`vac*cine` is vac, cine; `x *`
// and `**` say nothing).  The prefix is lower-cased; shorter than 2 bytes it is dropped like a one-byte token (`a*`); it is NOT
// tested against the stop-word list (`the*` means therapy and thermal: the lexicons hold no stop words anyway).  `covid-19*` is
// the term covid and the prefix 19.  A text without such a '*' parses exactly as parse_boosted parses it.  The parser is total.
//
// A prefix stands for the terms of the autocomplete table (suggest.hpp) that begin with it, itself included: at most
// max_expansions of them, the best by (summed df descending, term bytes ascending), which is suggest's order.  In a segment the
// prefix is ONE blended term: the union of its expansions' lists there, the tf of a document the sum of the members' tf, the df
// the size of the union and the idf bm25_idf(N, that df): the posting list the term would have if every word under the prefix
// had been indexed as one word (ns_segment_union).  With one expansion in a segment it is that term's own list, idf included.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "boost.hpp"

namespace nsx {

static constexpr uint32_t kPrefixDefaultExpansions = 1024, kPrefixMaxExpansions = 65535;

struct PrefixSpec {
    uint32_t max_expansions = kPrefixDefaultExpansions;   // 1 .. kPrefixMaxExpansions
};
inline bool prefix_check(const PrefixSpec& s, std::string& err) {
    if (s.max_expansions >= 1 && s.max_expansions <= kPrefixMaxExpansions) return true;
    err = "prefix: max_expansions " + std::to_string(s.max_expansions) + " is outside [1, " + std::to_string(kPrefixMaxExpansions) + "]";
    return false;
}

// what a call did with one prefix: the terms it stands for in this index, and whether max_expansions cut them
struct PrefixInfo {
    std::string prefix;
    uint32_t expansions;
    bool truncated;
};

struct PrefixedTerm {
    std::string text;   // a prefix without its '*'
    uint8_t role;
    uint32_t clause;    // as QuorumTerm's
    uint32_t need;
    bool promoted;
    float weight;       // as BoostedTerm's
    bool prefix;
};

// Calls fn(ptr, len, role, clause, need, weight, is_prefix) for every term of the query, in order.
template <class Fn>
inline QuorumShape for_each_prefixed_term(const char* text, size_t n, std::vector<char>& scratch, Fn fn) {
    float w = 1.0f;
    bool star = false;
    return for_each_dialect_term<Dialect::Prefixed>(text, n, scratch, [&](const char* p, size_t len, uint8_t role, uint32_t clause, uint32_t need) { fn(p, len, role, clause, need, w, star); }, &w, &star);
}

// -> the terms with the `~m` promotion applied, as parse_boosted does; min_should as parse_quorum's
inline std::vector<PrefixedTerm> parse_prefixed(const std::string& text, uint32_t* min_should = nullptr) {
    std::vector<PrefixedTerm> out;
    std::vector<char> scratch;
    const QuorumShape shape = for_each_prefixed_term(text.data(), text.size(), scratch, [&](const char* p, size_t len, uint8_t role, uint32_t clause, uint32_t need, float w, bool star) {
        out.push_back(PrefixedTerm{std::string(p, len), role, clause, need, false, w, star});
    });
    if (shape.min_should)
        for (PrefixedTerm& t : out)
            if (t.role == kRoleShould) t = PrefixedTerm{t.text, kRoleMust, shape.n_clauses, shape.min_should, true, t.weight, t.prefix};
    if (min_should) *min_should = shape.min_should;
    return out;
}

}  // namespace nsx
