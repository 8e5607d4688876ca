// Boosts: what a per-document factor and a term weight are on the host.
//
// A boost is one fp32 factor per document (per segment in manifest order); the device multiplies a matched document's finished
// BM25 sum by it, once, and ranks by the product (ns_search_boosted_after).  A factor is finite and carries no sign bit.
//   Custom        the caller's arrays as they are.
//   Exponential   f = 2^(-age / scale_days)
//   Linear        f = max(0, 1 - age / scale_days)
// with age = max(0, |days(origin) - days(key)| - offset_days), days() the civil day number of a document's date_key()
// (filter.hpp) with a missing month or day read as 1, and `origin` a date as the filter bounds are (empty: the newest dated
// document of the index).  An undated document takes f = undated.  The factor of the two decays is (1 - weight) + weight * f,
// weight in [0, 1], computed in double and rounded once to fp32: weight 0 gives a table of 1.0f, and x * 1.0f is exact, so the
// answers are then the unboosted call's bit for bit.
//
// Term weights.  parse_boosted reads parse_quorum's dialect (quorum.hpp) plus a suffix `^w`:
//     vaccine^2.5   +vaccine^2.5          on a word or a `+word`: the weight of every token of the piece
//     +(covid sars)^0.5   (a b c)~2^3     on a group, behind its ')' and the optional `~m`, up to the next blank
// w is digits with at most one '.', its value in (0, 1e6]; anything else (`^`, `^0`, `^-1`, `^1e3`, `^1.2.3`, more than 1e6) is
// no suffix and leaves the '^' to the tokenizer as before.  On a `-` piece the suffix is consumed and ignored.  The weight becomes
// the qweight of every term of the piece: the score adds qweight * term score, so `^2` counts the term twice.  A text without
// a valid `^w` parses as parse_quorum parses it.  The parser is total.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "filter.hpp"
#include "quorum.hpp"

namespace nsx {

struct BoostSpec {
    enum Kind { Custom = 0, Exponential = 1, Linear = 2 };
    Kind kind = Exponential;
    double weight = 1.0;        // Exponential, Linear: how much of the factor the decay decides, in [0, 1]
    std::string origin;         // YYYY, YYYY-MM or YYYY-MM-DD; empty: the newest dated document
    double scale_days = 365.0;  // > 0: the half-life (Exponential), the age at which f reaches 0 (Linear)
    double offset_days = 0.0;   // ages up to this count as 0
    double undated = 1.0;       // f of a document without a date
    std::vector<std::vector<float>> custom;   // Custom: per segment, one factor per document
};
inline const char* boost_name(const BoostSpec& s) { return s.kind == BoostSpec::Custom ? "custom" : s.kind == BoostSpec::Exponential ? "exponential" : "linear"; }

// days since 1970-01-01 of a proleptic Gregorian date
inline int64_t civil_days(int64_t y, unsigned m, unsigned d) {
    y -= m <= 2;
    const int64_t era = (y >= 0 ? y : y - 399) / 400;
    const unsigned yoe = (unsigned)(y - era * 400);
    const unsigned doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;
    const unsigned doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + (int64_t)doe - 719468;
}
// the day number of a date key (filter.hpp: Y * 10000 + M * 100 + D, missing parts 0, here read as 1); key != 0
inline int64_t days_of_key(uint32_t key) {
    const unsigned m = key / 100u % 100u, d = key % 100u;
    return civil_days((int64_t)(key / 10000u), m ? m : 1u, d ? d : 1u);
}

inline bool boost_factor_ok(float f) { return std::isfinite(f) && !std::signbit(f); }

// The parameters of a decay; false with `err` for a weight outside [0, 1], a scale that is not above 0, an offset or an undated
// value that would leave the range of a factor, and an origin that is neither empty nor a date.  origin_key: 0 for an empty origin.
inline bool boost_check(const BoostSpec& s, uint32_t& origin_key, std::string& err) {
    origin_key = 0;
    if ((unsigned)s.kind > 2u) { err = "boost: unknown kind"; return false; }
    if (s.kind == BoostSpec::Custom) return true;
    if (!(s.weight >= 0.0 && s.weight <= 1.0)) { err = "boost: weight " + std::to_string(s.weight) + " is outside [0, 1]"; return false; }
    if (!(s.scale_days > 0.0) || !std::isfinite(s.scale_days)) { err = "boost: scale_days must be above 0"; return false; }
    if (!(s.offset_days >= 0.0) || !std::isfinite(s.offset_days)) { err = "boost: offset_days must be 0 or above"; return false; }
    if (!(s.undated >= 0.0) || !std::isfinite(s.undated) || !boost_factor_ok((float)((1.0 - s.weight) + s.weight * s.undated))) { err = "boost: undated must be a finite value that is 0 or above"; return false; }
    const std::string text(detail::strip_blanks(s.origin));
    if (text.empty()) return true;
    origin_key = date_key(text);
    if (!origin_key) { err = "boost: origin \"" + s.origin + "\" is not YYYY, YYYY-MM or YYYY-MM-DD"; return false; }
    return true;
}

// the factor of one document under a decay (boost_check passed): key 0 is undated
inline float boost_decay(const BoostSpec& s, int64_t origin_days, uint32_t key) {
    double f = s.undated;
    if (key) {
        const int64_t apart = origin_days - days_of_key(key);
        const double age = std::max(0.0, (double)(apart < 0 ? -apart : apart) - s.offset_days);
        f = s.kind == BoostSpec::Exponential ? std::exp2(-age / s.scale_days) : std::max(0.0, 1.0 - age / s.scale_days);
    }
    return (float)((1.0 - s.weight) + s.weight * f);
}

struct BoostedTerm {
    std::string text;
    uint8_t role;
    uint32_t clause;   // as QuorumTerm's
    uint32_t need;
    bool promoted;
    float weight;      // the piece's `^w`, 1.0f without one and under kRoleNot
};

// Calls fn(ptr, len, role, clause, need, weight) for every term of the query, in order: for_each_quorum_term with a weight per term.
template <class Fn>
inline QuorumShape for_each_boosted_term(const char* text, size_t n, std::vector<char>& scratch, Fn fn) {
    float w = 1.0f;
    return for_each_dialect_term<Dialect::Boosted>(text, n, scratch, [&](const char* p, size_t len, uint8_t role, uint32_t clause, uint32_t need) { fn(p, len, role, clause, need, w); }, &w);
}

// -> the terms with the `~m` promotion applied (a promoted term keeps its weight); min_should as parse_quorum's
inline std::vector<BoostedTerm> parse_boosted(const std::string& text, uint32_t* min_should = nullptr) {
    std::vector<BoostedTerm> out;
    std::vector<char> scratch;
    const QuorumShape shape = for_each_boosted_term(text.data(), text.size(), scratch, [&](const char* p, size_t len, uint8_t role, uint32_t clause, uint32_t need, float w) {
        out.push_back(BoostedTerm{std::string(p, len), role, clause, need, false, w});
    });
    if (shape.min_should)
        for (BoostedTerm& t : out)
            if (t.role == kRoleShould) t = BoostedTerm{t.text, kRoleMust, shape.n_clauses, shape.min_should, true, t.weight};
    if (min_should) *min_should = shape.min_should;
    return out;
}

}  // namespace nsx
