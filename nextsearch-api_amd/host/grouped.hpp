// Any-of groups in boolean queries: the query box's dialect with one level of parentheses,
//     +(coronavirus covid sars) +(vaccine vaccination) -mouse safety
// A text without '(' parses here as it parses under parse_boolean (boolean.hpp, whose scanner reads all three dialects).
//
// The query is split on whitespace.  A piece whose text, after an optional one-byte '+' or '-', begins with '(' opens a group:
// its body runs to the first ')' (across whitespace), or to the end of the query if there is none, and EVERY token the
// search's tokenizer (for_each_base_term) takes from the body gets the group's role.  The tokens of a MUST group share one
// fresh clause id: a document must hold at least one of them.  A body without a token emits nothing and uses no id.
// Scanning resumes right behind the ')': `+(a b)c` is the clause {a, b} and the optional term c.  Inside a body '+', '-' and
// '(' are the tokenizer's business, as is a ')' without an open group.  Every other piece follows parse_boolean's rule, and
// each of its MUST tokens gets a clause id of its own (`+covid-19` is two clauses).  `(a b)` is `a b`; `-(a b)` is `-a -b`.
// The parser is total.  Clause ids count up from 0 in query order; SHOULD and NOT terms carry 0.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "boolean.hpp"

namespace nsx {

struct GroupedTerm {
    std::string text;
    uint8_t role;
    uint32_t clause;   // under kRoleMust: the clause the term belongs to; else 0
};

// Calls fn(ptr, len, role, clause) for every term of the query, in order; returns the number of clauses.
template <class Fn>
inline uint32_t for_each_grouped_term(const char* text, size_t n, std::vector<char>& scratch, Fn fn) {
    return for_each_dialect_term<Dialect::Grouped>(text, n, scratch, [&](const char* p, size_t len, uint8_t role, uint32_t clause, uint32_t) { fn(p, len, role, clause); }).n_clauses;
}

inline std::vector<GroupedTerm> parse_grouped(const std::string& text) {
    std::vector<GroupedTerm> out;
    std::vector<char> scratch;
    for_each_grouped_term(text.data(), text.size(), scratch,
                          [&](const char* p, size_t len, uint8_t role, uint32_t clause) { out.push_back(GroupedTerm{std::string(p, len), role, clause}); });
    return out;
}

}  // namespace nsx
