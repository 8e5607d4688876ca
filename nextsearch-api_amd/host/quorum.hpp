// At-least-m-of-n clauses in boolean queries: parse_grouped's dialect (grouped.hpp, untouched) plus two forms,
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
static constexpr uint32_t kQuorumNeedCap = 1000000;    // what a longer run of digits reads as

struct QuorumTerm {
    std::string text;
    uint8_t role;
    uint32_t clause;   // under kRoleMust: the clause the term belongs to; else 0
    uint32_t need;     // under kRoleMust: the need of its clause (>= 1); else 0
    bool promoted;     // an optional term that a `~m` piece made a member of the query's last clause
};

struct QuorumShape {
    uint32_t n_clauses;    // of the terms as fn saw them
    uint32_t min_should;   // the last `~m` piece's m; > 0: the caller makes every SHOULD term a MUST term of clause n_clauses, need m
};

// decimal digits at text[i ..): their value (saturating) and the index behind them; no digit: `end` == i
inline uint32_t quorum_digits(const char* text, size_t n, size_t i, size_t& end) {
    uint64_t v = 0;
    end = i;
    while (end < n && text[end] >= '0' && text[end] <= '9') {
        v = v * 10 + (uint64_t)(text[end] - '0');
        if (v > kQuorumNeedCap) v = kQuorumNeedCap;
        end++;
    }
    return (uint32_t)v;
}

// Calls fn(ptr, len, role, clause, need) for every term of the query, in order: for_each_grouped_term with a need per MUST term.
// The optional terms come as SHOULD terms (clause 0, need 0) whatever min_should says: see QuorumShape.
template <class Fn>
inline QuorumShape for_each_quorum_term(const char* text, size_t n, std::vector<char>& scratch, Fn fn) {
    QuorumShape shape{0, 0};
    size_t i = 0;
    while (i < n) {
        while (i < n && bool_is_space((unsigned char)text[i])) i++;
        if (i >= n) break;
        const uint8_t prefix = text[i] == '+' ? kRoleMust : text[i] == '-' ? kRoleNot : kRoleShould;
        const size_t from = prefix == kRoleShould ? i : i + 1;
        if (from < n && text[from] == '(') {
            size_t end = from + 1;
            while (end < n && text[end] != ')') end++;
            size_t resume = end < n ? end + 1 : n;
            uint32_t need = 0;
            if (end + 1 < n && text[end + 1] == '~') {
                size_t behind;
                const uint32_t m = quorum_digits(text, n, end + 2, behind);
                if (behind > end + 2) { need = m; resume = behind; }
            }
            const uint8_t role = (need >= 1 && prefix == kRoleShould) ? kRoleMust : prefix;
            if (role != kRoleMust) need = 0;
            else if (need == 0) need = 1;
            bool any = false;
            for_each_base_term(text + from + 1, end - (from + 1), scratch, [&](const char* p, size_t len) {
                fn(p, len, role, role == kRoleMust ? shape.n_clauses : 0u, need);
                any = true;
            });
            if (any && role == kRoleMust) shape.n_clauses++;
            i = resume;
            continue;
        }
        size_t j = i;
        while (j < n && !bool_is_space((unsigned char)text[j])) j++;
        if (text[i] == '~' && j > i + 1) {
            size_t behind;
            const uint32_t m = quorum_digits(text, n, i + 1, behind);
            if (behind == j) { shape.min_should = m; i = j; continue; }
        }
        for_each_base_term(text + from, j - from, scratch,
                           [&](const char* p, size_t len) { fn(p, len, prefix, prefix == kRoleMust ? shape.n_clauses++ : 0u, prefix == kRoleMust ? 1u : 0u); });
        i = j;
    }
    return shape;
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
