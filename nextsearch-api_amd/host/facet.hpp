// Facet counts: what a facet is on the host.
//
// A facet is one bucket id per document (uint16, per segment in manifest order) plus one label per bucket; the device counts,
// per query, the distinct matched documents of every bucket (ns_facet_count).  At most kMaxFacetBuckets buckets.
//
// Year and Month bucket a document by date_key() of its metadata.csv publish_time (filter.hpp): key / 10000, respectively
// key / 100.  Bucket 0 is always "undated" (key 0: an empty or malformed date, or no metadata row), label "".  The other
// buckets are the distinct values present in the index, ascending; labels "2020", respectively "2020-03".  Under Month a
// document dated only "2020" has the value 202000 and lands in a bucket of its own in front of 2020's months, labelled
// "2020".  More than kMaxFacetBuckets - 1 distinct values fail the call with a message.
// Custom takes the caller's bucket arrays and labels as they are (label 0 included).
//
// Round trip with filtered search: the documents of year bucket "Y" are exactly those that DocFilter{date_from = "Y",
// date_to = "Y"} keeps (from = Y0000 <= key <= Y9999 = to), and bucket 0 is what keep_undated adds to an empty range.  So
// a count shown next to a year is the `found` of the same query under that year's filter.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "filter.hpp"

namespace nsx {

static constexpr uint32_t kMaxFacetBuckets = 1024;   // == the device's limit (ns_facet_upload)

struct FacetSpec {
    enum Kind { Year = 0, Month = 1, Custom = 2 };
    Kind kind = Year;
    std::vector<std::vector<uint16_t>> custom_buckets;   // Custom: per segment, one id per document, each < custom_labels.size()
    std::vector<std::string> custom_labels;
};
inline const char* facet_kind_name(FacetSpec::Kind k) { return k == FacetSpec::Year ? "year" : k == FacetSpec::Month ? "month" : "custom"; }

// a document's facet value under Year / Month; 0 = undated
inline uint32_t facet_value(FacetSpec::Kind kind, uint32_t key) { return kind == FacetSpec::Year ? key / 10000u : key / 100u; }
inline std::string facet_label(FacetSpec::Kind kind, uint32_t value) {
    if (!value) return std::string();
    char buf[16];
    if (kind == FacetSpec::Year) std::snprintf(buf, sizeof(buf), "%04u", value);
    else if (value % 100u == 0u) std::snprintf(buf, sizeof(buf), "%04u", value / 100u);   // dated to the year only
    else std::snprintf(buf, sizeof(buf), "%04u-%02u", value / 100u, value % 100u);
    return buf;
}

// keys[s][d] = date_key of document d of segment s -> bucket tables and labels.  false: too many distinct values.
inline bool facet_from_keys(FacetSpec::Kind kind, const std::vector<std::vector<uint32_t>>& keys, std::vector<std::vector<uint16_t>>& tables,
                            std::vector<std::string>& labels, std::string& err) {
    std::vector<uint32_t> values;
    for (const auto& seg : keys)
        for (const uint32_t k : seg)
            if (const uint32_t v = facet_value(kind, k)) values.push_back(v);
    std::sort(values.begin(), values.end());
    values.erase(std::unique(values.begin(), values.end()), values.end());
    if (values.size() > kMaxFacetBuckets - 1) {
        err = std::string("facet ") + facet_kind_name(kind) + ": " + std::to_string(values.size()) + " distinct values; at most " +
              std::to_string(kMaxFacetBuckets - 1) + " (and the undated bucket) fit a facet";
        return false;
    }
    labels.assign(1, std::string());
    for (const uint32_t v : values) labels.push_back(facet_label(kind, v));
    tables.assign(keys.size(), {});
    for (size_t s = 0; s < keys.size(); s++) {
        tables[s].resize(keys[s].size());
        for (size_t d = 0; d < keys[s].size(); d++) {
            const uint32_t v = facet_value(kind, keys[s][d]);
            tables[s][d] = v ? (uint16_t)(1 + (std::lower_bound(values.begin(), values.end(), v) - values.begin())) : (uint16_t)0;
        }
    }
    return true;
}

}  // namespace nsx
