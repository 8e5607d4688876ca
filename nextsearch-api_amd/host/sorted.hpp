// Search sorted by date: what a sort order is on the host.
//
// A sort order is one uint32 key per document (per segment in manifest order) and a direction; the device returns, per
// query, the first K matched documents in the order (key, segment position ascending, docId ascending) with their BM25
// scores (ns_search_sorted).  Key 0 means "no key" and is LAST IN BOTH DIRECTIONS; 0xFFFFFFFF is reserved.
//
// Date keys are date_key() of metadata.csv's publish_time (filter.hpp): YYYYMMDD with missing parts 0, and 0 for an empty
// or malformed date or a document without a metadata row.  Consequence: under newest-first an article dated just "2020"
// (key 20200000) comes AFTER every dated day of 2020; under oldest-first it comes BEFORE them.
// Custom takes the caller's key arrays as they are.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "filter.hpp"

namespace nsx {

static constexpr uint32_t kSortReservedKey = 0xFFFFFFFFu;   // == the device's (ns_dockeys_upload refuses it)

struct SortSpec {
    enum Kind { Date = 0, Custom = 1 };
    Kind kind = Date;
    bool ascending = false;                            // false: newest (largest key) first
    std::vector<std::vector<uint32_t>> custom_keys;    // Custom: per segment, one key per document
};
inline const char* sort_name(const SortSpec& s) { return s.kind == SortSpec::Custom ? "custom" : s.ascending ? "oldest" : "newest"; }

// the total order of a result page, as the device realises it: true when a comes before b
inline bool sort_before(uint32_t key_a, uint32_t pos_a, uint32_t doc_a, uint32_t key_b, uint32_t pos_b, uint32_t doc_b, bool ascending) {
    const uint32_t ta = ascending ? (key_a ? ~key_a : 0u) : key_a, tb = ascending ? (key_b ? ~key_b : 0u) : key_b;
    if (ta != tb) return ta > tb;
    if (pos_a != pos_b) return pos_a < pos_b;
    return doc_a < doc_b;
}

}  // namespace nsx
