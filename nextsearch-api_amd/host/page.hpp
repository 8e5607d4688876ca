// Pages past the first K: what a cursor is on the host.
//
// A cursor is a position (rank, segment, docId) in the total order of a ranked call; the call answers with the first K
// matched documents strictly after it (ns_search_boolean_after, ns_search_sorted_after).  `rank` is the fp32 score bits in
// score order and the sort key as uploaded in date order; `seg` is a MANIFEST POSITION, which the engine translates to the
// call's segment id.  A cursor is good until a reload() changes the index.
//
// Its text form is what a result page hands to its "next" button:
//     kind letter  's' (score order) or 'd' (date order)
//     rank         exactly 8 lowercase hex digits
//     '.'  position, decimal    '.'  docId, decimal           (no sign, no leading zero except "0", at most 0xFFFFFFFF)
// e.g. s41a3c28f.0.5121.  The empty string is "no cursor".  parse_cursor takes nothing else.
#pragma once

#include <cstdint>
#include <string>

#include "boolean.hpp"
#include "boost.hpp"
#include "prefix.hpp"
#include "sorted.hpp"

namespace nsx {

struct PageCursor {
    bool set = false;
    uint32_t rank = 0;
    uint32_t seg = 0;   // manifest position
    uint32_t doc = 0;
};

// which call a page is a page of
struct PageSpec {
    enum Mode { SearchOr = 0, SearchAnd = 1, Boolean = 2, Sorted = 3, BooleanSorted = 4, Grouped = 5, GroupedSorted = 6, Quorum = 7, QuorumSorted = 8, Boosted = 9, Prefixed = 10 };   // BooleanSorted: DESIGN.md §5t; Grouped*: §5u; Quorum*: §5w; Boosted: §5z; Prefixed: §5ab
    Mode mode = SearchOr;
    bool use_boost = false;              // Boosted and Prefixed only: false = term weights alone
    BoostSpec boost;
    PrefixSpec prefix;                   // Prefixed only
    SortSpec sort;                       // Sorted, BooleanSorted, GroupedSorted and QuorumSorted only
    bool use_filter = false;
    DocFilter filter;
};
// which call a mode pages: the plain search's (SearchOr, SearchAnd, Sorted) or a boolean dialect's, in score or in date order
struct PageCall { bool plain; Dialect dialect; bool dated; };
inline PageCall page_call(PageSpec::Mode m) {
    switch (m) {
        case PageSpec::Sorted: return {true, Dialect::Boolean, true};
        case PageSpec::Boolean: return {false, Dialect::Boolean, false};
        case PageSpec::BooleanSorted: return {false, Dialect::Boolean, true};
        case PageSpec::Grouped: return {false, Dialect::Grouped, false};
        case PageSpec::GroupedSorted: return {false, Dialect::Grouped, true};
        case PageSpec::Quorum: return {false, Dialect::Quorum, false};
        case PageSpec::QuorumSorted: return {false, Dialect::Quorum, true};
        case PageSpec::Boosted: return {false, Dialect::Boosted, false};
        case PageSpec::Prefixed: return {false, Dialect::Prefixed, false};
        default: return {true, Dialect::Boolean, false};   // SearchOr, SearchAnd
    }
}
inline char page_kind(PageSpec::Mode m) { return page_call(m).dated ? 'd' : 's'; }

inline std::string cursor_text(char kind, const PageCursor& c) {
    if (!c.set) return std::string();
    static const char* hex = "0123456789abcdef";
    std::string o(1, kind);
    for (int sh = 28; sh >= 0; sh -= 4) o.push_back(hex[(c.rank >> sh) & 15u]);
    o.push_back('.');
    o += std::to_string(c.seg);
    o.push_back('.');
    o += std::to_string(c.doc);
    return o;
}

// one decimal field of a cursor from text[at]; stops at the first byte that is no digit
inline bool cursor_field(const std::string& text, size_t& at, uint32_t& out, const char* name, std::string& why) {
    const size_t begin = at;
    uint64_t v = 0;
    while (at < text.size() && text[at] >= '0' && text[at] <= '9') {
        v = v * 10 + (uint64_t)(text[at] - '0');
        if (v > 0xFFFFFFFFull) { why = std::string("cursor: ") + name + " overflows 32 bits"; return false; }
        at++;
    }
    if (at == begin) { why = std::string("cursor: ") + name + " is missing"; return false; }
    if (text[begin] == '0' && at - begin > 1) { why = std::string("cursor: ") + name + " has a leading zero"; return false; }
    out = (uint32_t)v;
    return true;
}

// text -> cursor of the given kind ('s' or 'd').  The empty string is the unset cursor.  False with `why` set for anything
// that cursor_text does not write, or a cursor of the other kind.
inline bool parse_cursor(const std::string& text, char kind, PageCursor& out, std::string& why) {
    out = PageCursor{};
    if (text.empty()) return true;
    if (kind != 's' && kind != 'd') { why = "cursor: unknown kind asked for"; return false; }
    if (text[0] != 's' && text[0] != 'd') { why = "cursor: the kind letter is neither 's' nor 'd'"; return false; }
    if (text[0] != kind) { why = std::string("cursor: a cursor of kind '") + text[0] + "' does not fit this call, which pages in " + (kind == 's' ? "score" : "date") + " order"; return false; }
    if (text.size() < 9) { why = "cursor: rank is not 8 hex digits"; return false; }
    uint32_t rank = 0;
    for (size_t i = 1; i < 9; i++) {
        const char c = text[i];
        uint32_t d;
        if (c >= '0' && c <= '9') d = (uint32_t)(c - '0');
        else if (c >= 'a' && c <= 'f') d = (uint32_t)(c - 'a') + 10u;
        else { why = "cursor: rank is not 8 lowercase hex digits"; return false; }
        rank = (rank << 4) | d;
    }
    size_t at = 9;
    PageCursor c;
    if (at >= text.size() || text[at] != '.') { why = "cursor: '.' expected after the rank"; return false; }
    at++;
    if (!cursor_field(text, at, c.seg, "position", why)) return false;
    if (at >= text.size() || text[at] != '.') { why = "cursor: '.' expected after the position"; return false; }
    at++;
    if (!cursor_field(text, at, c.doc, "docId", why)) return false;
    if (at != text.size()) { why = "cursor: trailing bytes"; return false; }
    c.set = true;
    c.rank = rank;
    out = c;
    return true;
}

}  // namespace nsx
