// Boolean queries: what the query box's `+word` / `-word` dialect is on the host.
//
// The query is split on whitespace.  A piece that begins with '+' gives the role MUST, one that begins with '-' the role
// NOT, to EVERY token the search's tokenizer takes from the rest of the piece; every other piece is SHOULD.  Only the first
// byte of a piece is a prefix: a '-' inside a piece is the tokenizer's business (`covid-19` is the SHOULD terms covid, 19;
// `+covid-19` the MUST terms covid, 19; `--word` excludes word; a lone `+` or `-` says nothing).  Stop words and one-byte
// tokens are dropped as search drops them (for_each_base_term), under a prefix too; order and duplicates stay.
// No parentheses, no phrases, no nesting.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "term_dict.hpp"

namespace nsx {

static constexpr uint8_t kRoleShould = 0, kRoleMust = 1, kRoleNot = 2;   // == NS_ROLE_* of nextsearch_hip.h

struct BoolTerm {
    std::string text;
    uint8_t role;
};

inline bool bool_is_space(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }

// Calls fn(ptr, len, role) for every term of the query, in order.  `scratch` holds the lowercased bytes.
template <class Fn>
inline void for_each_boolean_term(const char* text, size_t n, std::vector<char>& scratch, Fn fn) {
    size_t i = 0;
    while (i < n) {
        while (i < n && bool_is_space((unsigned char)text[i])) i++;
        size_t j = i;
        while (j < n && !bool_is_space((unsigned char)text[j])) j++;
        if (j > i) {
            const uint8_t role = text[i] == '+' ? kRoleMust : text[i] == '-' ? kRoleNot : kRoleShould;
            const size_t from = role == kRoleShould ? i : i + 1;
            for_each_base_term(text + from, j - from, scratch, [&](const char* p, size_t len) { fn(p, len, role); });
        }
        i = j;
    }
}

inline std::vector<BoolTerm> parse_boolean(const std::string& text) {
    std::vector<BoolTerm> out;
    std::vector<char> scratch;
    for_each_boolean_term(text.data(), text.size(), scratch, [&](const char* p, size_t len, uint8_t role) { out.push_back(BoolTerm{std::string(p, len), role}); });
    return out;
}

}  // namespace nsx
