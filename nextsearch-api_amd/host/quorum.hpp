// At-least-m-of-n clauses in boolean queries: parse_grouped's dialect (grouped.hpp) plus two forms,
//     +(fever cough dyspnea fatigue)~2 -mouse          at least two of the four
//     fever cough dyspnea fatigue ~2                   at least two of the optional terms
// A text with neither form parses here as it parses there.
//
// A group's ')' directly followed by '~' and decimal digits sets the group's need m: a `+( )` or a bare `( )` group with m >= 1 is
// a REQUIRED clause of which a document must hold at least m terms (so `(a b c)~2` is `+(a b c)~2`); with m == 0 the suffix says
// nothing; on a `-( )` group it is consumed and ignored.  Scanning resumes behind the digits.  A '~' that no digit follows is no
// suffix: scanning resumes right behind the ')', as in parse_grouped.
// A whole piece `~m` (a '~' and decimal digits, nothing else) makes ALL optional terms of the query ONE required clause of need m;
// the last such piece wins and `~0` is none.  The piece itself is no term.
// MUST and SHOULD terms score alike, so the promoted terms score as they did.  Duplicate tokens stay: the score counts them, and
// the C-ABI counts a list once.  The parser is total: a need is whatever the digits say (saturating at kQuorumNeedCap); the
// engine refuses a need above nsx::kQuorumMaxNeed with a message.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "grouped.hpp"

namespace nsx {

static constexpr uint32_t kQuorumMaxNeed = 7;          // == kBqMaxNeed of csrc/ns_boolean_plan.hpp

struct QuorumTerm {
    std::string text;
    uint8_t role;
    uint32_t clause;   // under kRoleMust: the clause the term belongs to; else 0
    uint32_t need;     // under kRoleMust: the need of its clause (>= 1); else 0
    bool promoted;     // an optional term that a `~m` piece made a member of the query's last clause
};

// Calls fn(ptr, len, role, clause, need) for every term of the query, in order: for_each_grouped_term with a need per MUST term
// (QuorumShape, quorum_digits and the scanner itself are boolean.hpp's).
template <class Fn>
inline QuorumShape for_each_quorum_term(const char* text, size_t n, std::vector<char>& scratch, Fn fn) {
    return for_each_dialect_term<Dialect::Quorum>(text, n, scratch, fn);
}

// -> the terms with the `~m` promotion applied; min_should (may be NULL) gets the piece's m (0: none)
inline std::vector<QuorumTerm> parse_quorum(const std::string& text, uint32_t* min_should = nullptr) {
    std::vector<QuorumTerm> out;
    std::vector<char> scratch;
    const QuorumShape shape = for_each_quorum_term(text.data(), text.size(), scratch, [&](const char* p, size_t len, uint8_t role, uint32_t clause, uint32_t need) {
        out.push_back(QuorumTerm{std::string(p, len), role, clause, need, false});
    });
    if (shape.min_should)
        for (QuorumTerm& t : out)
            if (t.role == kRoleShould) t = QuorumTerm{t.text, kRoleMust, shape.n_clauses, shape.min_should, true};
    if (min_should) *min_should = shape.min_should;
    return out;
}

}  // namespace nsx
