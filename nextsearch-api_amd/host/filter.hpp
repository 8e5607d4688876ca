// Filtered search: what a filter is on the host.
//
// A filter is one keep-bitmap per segment (bit d % 32 of word d / 32 of segment s: document d is kept).  Engine::open_filter
// turns it into filtered copies of the segments' posting streams on the device (ns_segment_filter) and a table of
// {byte_off', count', idf} rows parallel to TermDict's; the idf is the UNFILTERED bm25_idf(N, df): a filter chooses among
// the results, it does not change a score.
//
// Dates.  metadata.csv's publish_time is free text; date_key() accepts exactly YYYY, YYYY-MM (01..12) and YYYY-MM-DD
// (01..31), surrounding blanks stripped, and gives Y * 10000 + M * 100 + D with the missing parts 0.  Anything else, the
// empty string included, gives 0 = undated; so does a document without a metadata row.
// A DocFilter keeps the documents with from <= key <= to.  A bound is parsed like a date, except that the missing parts of
// date_to count as 99: date_to = "2020" keeps all of 2020.  The missing parts of date_from stay 0, and so do those of a
// DOCUMENT'S date: with date_from = "2020-03" a document dated just "2020" (key 20200000 < 20200300) is NOT kept, while
// date_from = "2020" keeps it.  An empty bound is open.  A bound that is neither empty nor a date fails the call.  Undated
// documents are kept only with keep_undated, whatever the bounds.
#pragma once

#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

#include "term_dict.hpp"

namespace nsx {

namespace detail {
inline std::string_view strip_blanks(std::string_view s) {
    auto blank = [](char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\f' || c == '\v'; };
    while (!s.empty() && blank(s.front())) s.remove_prefix(1);
    while (!s.empty() && blank(s.back())) s.remove_suffix(1);
    return s;
}
// the digits s[at, at + n) as a number, or -1
inline int digits(std::string_view s, size_t at, size_t n) {
    int v = 0;
    for (size_t i = 0; i < n; i++) {
        const char c = s[at + i];
        if (c < '0' || c > '9') return -1;
        v = v * 10 + (c - '0');
    }
    return v;
}
// fill: the value of a missing month / day.  0 = not a date.
inline uint32_t parse_date(std::string_view s, uint32_t fill) {
    s = strip_blanks(s);
    if (s.size() != 4 && s.size() != 7 && s.size() != 10) return 0;
    const int y = digits(s, 0, 4);
    if (y < 0) return 0;
    uint32_t m = fill, d = fill;
    if (s.size() >= 7) {
        const int mm = digits(s, 5, 2);
        if (s[4] != '-' || mm < 1 || mm > 12) return 0;
        m = (uint32_t)mm;
    }
    if (s.size() == 10) {
        const int dd = digits(s, 8, 2);
        if (s[7] != '-' || dd < 1 || dd > 31) return 0;
        d = (uint32_t)dd;
    }
    return (uint32_t)y * 10000u + m * 100u + d;
}
}  // namespace detail

inline uint32_t date_key(std::string_view s) { return detail::parse_date(s, 0u); }

struct DocFilter {
    std::string date_from, date_to;
    bool keep_undated = false;
};

// The bounds of a DocFilter as keys.  false: a bound is neither empty nor a date (which: `err`).
struct DateRange {
    uint32_t from = 0u, to = 0xFFFFFFFFu;
    std::string from_text, to_text;   // the bounds with their blanks stripped: the filter's normalised form
    bool keep_undated = false;
    bool keeps(uint32_t key) const { return key == 0u ? keep_undated : (key >= from && key <= to); }
    std::string cache_key() const { return from_text + "|" + to_text + (keep_undated ? "|1" : "|0"); }
};
inline bool parse_filter(const DocFilter& f, DateRange& out, std::string& err) {
    out = DateRange{};
    out.keep_undated = f.keep_undated;
    out.from_text = std::string(detail::strip_blanks(f.date_from));
    out.to_text = std::string(detail::strip_blanks(f.date_to));
    if (!out.from_text.empty()) {
        out.from = detail::parse_date(out.from_text, 0u);
        if (!out.from) { err = "filter: date_from \"" + f.date_from + "\" is not YYYY, YYYY-MM or YYYY-MM-DD"; return false; }
    }
    if (!out.to_text.empty()) {
        out.to = detail::parse_date(out.to_text, 99u);
        if (!out.to) { err = "filter: date_to \"" + f.date_to + "\" is not YYYY, YYYY-MM or YYYY-MM-DD"; return false; }
    }
    return true;
}

struct FilterStats {
    uint64_t docs_kept = 0, docs_total = 0;
    uint64_t postings_kept = 0, postings_total = 0;
    uint32_t segments_on_device = 0;   // segments with a kept document and a surviving posting
    double device_ms = 0.0;            // ns_segment_filter's passes, summed over the segments
    double total_ms = 0.0;             // the whole open_filter: passes, allocations, row table, skip tables
    uint64_t hbm_bytes = 0;            // postings, per-posting norms and per-document norms of the copies
};

// The term rows a batch is prepared from: the dictionary's own (rows == nullptr), or an open filter's — parallel to
// TermDict's ([term][segment]), kAbsent where the filtered list is empty or the term is absent, device ids id_base + position.
struct RowSource {
    const TermSeg* rows = nullptr;
    uint32_t id_base = 0;
};

}  // namespace nsx
