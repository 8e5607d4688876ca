// Boolean queries: what the query box's `+word` / `-word` dialect is on the host.
//
// The query is split on whitespace.  A piece that begins with '+' gives the role MUST, one that begins with '-' the role
// NOT, to EVERY token the search's tokenizer takes from the rest of the piece; every other piece is SHOULD.  Only the first
// byte of a piece is a prefix: a '-' inside a piece is the tokenizer's business (`covid-19` is the SHOULD terms covid, 19;
// `+covid-19` the MUST terms covid, 19; `--word` excludes word; a lone `+` or `-` says nothing).  Stop words and one-byte
// tokens are dropped as search drops them (for_each_base_term), under a prefix too; order and duplicates stay.
// No parentheses, no phrases, no nesting.
#pragma once

#include <charconv>
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

// The three dialects of the query box.  They are nested: Grouped (grouped.hpp) is Boolean plus one level of parentheses, Quorum
// (quorum.hpp) is Grouped plus the two `~m` forms, Boosted (boost.hpp) is Quorum plus the `^w` suffix, Prefixed (prefix.hpp) is
// Boosted plus the prefix term `word*`.  A further dialect is one more value here and one more branch in the scanner.
enum class Dialect : int { Boolean = 0, Grouped = 1, Quorum = 2, Boosted = 3, Prefixed = 4 };

static constexpr uint32_t kQuorumNeedCap = 1000000;    // what a longer run of digits reads as

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

static constexpr double kBoostMaxWeight = 1e6;         // a `^w` is a weight for 0 < w <= this

// Boosted: `^w` at text[i ..), where the piece ends at `stop`: '^', then digits with at most one '.' and at least one digit, up
// to `stop` exactly, their value in (0, kBoostMaxWeight] and above 0 as an fp32 too.  -> the weight, or 0: no weight stands there
// (an exponent, a sign, a second '.', nothing, zero, too much), and the '^' is the tokenizer's business.
inline float boost_weight_at(const char* text, size_t stop, size_t i) {
    if (i >= stop || text[i] != '^' || i + 1 >= stop) return 0.0f;
    size_t dots = 0, digits = 0;
    for (size_t j = i + 1; j < stop; j++) {
        if (text[j] == '.') dots++;
        else if (text[j] >= '0' && text[j] <= '9') digits++;
        else return 0.0f;
    }
    if (dots > 1 || digits == 0) return 0.0f;
    double v = 0.0;
    const auto r = std::from_chars(text + i + 1, text + stop, v, std::chars_format::fixed);
    if (r.ec != std::errc() || r.ptr != text + stop || !(v > 0.0) || v > kBoostMaxWeight) return 0.0f;
    return (float)v;
}

// The one scanner of the five grammars (the header comments of boolean.hpp, grouped.hpp, quorum.hpp, boost.hpp and prefix.hpp).  Calls
// fn(ptr, len, role, clause, need) for every term of the query, in order; `scratch` holds the lowercased bytes.  Under kRoleMust
// `clause` counts up from 0 (one id per group, one per token outside a group) and `need` is the clause's need (>= 1); else both
// are 0.  The optional terms come as SHOULD terms whatever min_should says: see QuorumShape.  Without groups '(' is the
// tokenizer's business; without needs a '~' is; without weights a '^' is.  Boosted: *weight holds the weight of the piece (1.0f
// without a valid suffix, and on a `-` piece, where the suffix is consumed and ignored) whenever fn is called.  Prefixed:
// *is_prefix says whether the term fn is called with is a prefix term (for_each_star_term), inside a group and before a `^w` too.
template <Dialect D, class Fn>
inline QuorumShape for_each_dialect_term(const char* text, size_t n, std::vector<char>& scratch, Fn fn, float* weight = nullptr, bool* is_prefix = nullptr) {
    constexpr bool kPrefixes = D == Dialect::Prefixed;
    constexpr bool kGroups = D != Dialect::Boolean, kNeeds = D == Dialect::Quorum || D == Dialect::Boosted || kPrefixes, kWeights = D == Dialect::Boosted || kPrefixes;
    float unused = 1.0f;
    float& w_now = weight ? *weight : unused;
    bool unused_star = false;
    bool& star_now = is_prefix ? *is_prefix : unused_star;
    // the tokens of a piece's body: for_each_base_term's, or with prefix terms its sibling's
    auto tokens = [&](const char* p, size_t len, auto emit) {
        if constexpr (kPrefixes) for_each_star_term(p, len, scratch, [&](const char* t, size_t tl, bool star) { star_now = star; emit(t, tl); });
        else for_each_base_term(p, len, scratch, emit);
    };
    QuorumShape shape{0, 0};
    size_t i = 0;
    while (i < n) {
        while (i < n && bool_is_space((unsigned char)text[i])) i++;
        if (i >= n) break;
        const uint8_t prefix = text[i] == '+' ? kRoleMust : text[i] == '-' ? kRoleNot : kRoleShould;
        const size_t from = prefix == kRoleShould ? i : i + 1;
        if (kGroups && from < n && text[from] == '(') {
            size_t end = from + 1;
            while (end < n && text[end] != ')') end++;
            size_t resume = end < n ? end + 1 : n;
            uint32_t need = 0;
            if (kNeeds && end + 1 < n && text[end + 1] == '~') {
                size_t behind;
                const uint32_t m = quorum_digits(text, n, end + 2, behind);
                if (behind > end + 2) { need = m; resume = behind; }
            }
            w_now = 1.0f;
            if (kWeights && resume < n && text[resume] == '^') {   // behind the ')' and the `~m`, up to the next blank
                size_t stop = resume;
                while (stop < n && !bool_is_space((unsigned char)text[stop])) stop++;
                const float w = boost_weight_at(text, stop, resume);
                if (w > 0.0f) { resume = stop; if (prefix != kRoleNot) w_now = w; }
            }
            const uint8_t role = (need >= 1 && prefix == kRoleShould) ? kRoleMust : prefix;
            if (role != kRoleMust) need = 0;
            else if (need == 0) need = 1;
            bool any = false;
            tokens(text + from + 1, end - (from + 1), [&](const char* p, size_t len) {
                fn(p, len, role, role == kRoleMust ? shape.n_clauses : 0u, need);
                any = true;
            });
            if (any && role == kRoleMust) shape.n_clauses++;
            i = resume;
            continue;
        }
        size_t j = i;
        while (j < n && !bool_is_space((unsigned char)text[j])) j++;
        if (kNeeds && text[i] == '~' && j > i + 1) {
            size_t behind;
            const uint32_t m = quorum_digits(text, n, i + 1, behind);
            if (behind == j) { shape.min_should = m; i = j; continue; }
        }
        size_t to = j;
        w_now = 1.0f;
        if (kWeights) {   // the piece's last '^', if a weight and nothing else stands behind it
            size_t hat = j;
            while (hat > from && text[hat - 1] != '^') hat--;
            const float w = hat > from ? boost_weight_at(text, j, hat - 1) : 0.0f;
            if (w > 0.0f) { to = hat - 1; if (prefix != kRoleNot) w_now = w; }
        }
        tokens(text + from, to - from, [&](const char* p, size_t len) { fn(p, len, prefix, prefix == kRoleMust ? shape.n_clauses++ : 0u, prefix == kRoleMust ? 1u : 0u); });
        i = j;
    }
    return shape;
}

// the scanner of a dialect chosen at run time
template <class Fn>
inline QuorumShape for_each_term(Dialect d, const char* text, size_t n, std::vector<char>& scratch, Fn fn, float* weight = nullptr, bool* is_prefix = nullptr) {
    if (weight) *weight = 1.0f;
    if (is_prefix) *is_prefix = false;
    switch (d) {
        case Dialect::Prefixed: return for_each_dialect_term<Dialect::Prefixed>(text, n, scratch, fn, weight, is_prefix);
        case Dialect::Boolean: return for_each_dialect_term<Dialect::Boolean>(text, n, scratch, fn);
        case Dialect::Grouped: return for_each_dialect_term<Dialect::Grouped>(text, n, scratch, fn);
        case Dialect::Quorum: return for_each_dialect_term<Dialect::Quorum>(text, n, scratch, fn);
        default: return for_each_dialect_term<Dialect::Boosted>(text, n, scratch, fn, weight);
    }
}

// Calls fn(ptr, len, role) for every term of the query, in order.
template <class Fn>
inline void for_each_boolean_term(const char* text, size_t n, std::vector<char>& scratch, Fn fn) {
    for_each_dialect_term<Dialect::Boolean>(text, n, scratch, [&](const char* p, size_t len, uint8_t role, uint32_t, uint32_t) { fn(p, len, role); });
}

inline std::vector<BoolTerm> parse_boolean(const std::string& text) {
    std::vector<BoolTerm> out;
    std::vector<char> scratch;
    for_each_boolean_term(text.data(), text.size(), scratch, [&](const char* p, size_t len, uint8_t role) { out.push_back(BoolTerm{std::string(p, len), role}); });
    return out;
}

}  // namespace nsx
