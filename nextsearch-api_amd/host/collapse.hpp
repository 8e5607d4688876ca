// Collapsing ranked hits by a per-document key: what "one hit per title" is on the host.
//
// A collapse key is one uint32 per document: 0 = no key (the document stands alone), any other value names a group, one key space
// over all segments; 0xFFFFFFFF is reserved, as in ns_dockeys.  The device ranks groups by their best member and reports each once
// (ns_search_collapsed).
//   Title    a dense id, from 1, assigned by first appearance in manifest order (segment by segment, docId ascending) of the
//            document's NORMALISED title: the lower-cased alphanumeric tokens of the query tokenizer (textutil.hpp), joined by
//            one space.  An empty normalised title (no metadata row, no title, punctuation only) is key 0.
//   Author   the same over the author field as MetaFields holds it.
//   Custom   the caller's keys.
// Ids are dense, not hashes: no collisions, and the same index gives the same keys.
#pragma once

#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "prefix.hpp"
#include "textutil.hpp"

namespace nsx {

static constexpr uint32_t kCollapseReservedKey = 0xFFFFFFFFu;

struct CollapseSpec {
    enum Kind : int { Title = 0, Author = 1, Custom = 2 };
    Kind kind = Title;
    std::vector<std::vector<uint32_t>> custom;   // Custom: per segment in manifest order, one key per document
};

inline const char* collapse_name(const CollapseSpec& s) { return s.kind == CollapseSpec::Title ? "title" : s.kind == CollapseSpec::Author ? "author" : "custom"; }

inline bool collapse_check(const CollapseSpec& s, std::string& err) {
    if ((unsigned)s.kind <= 2u) return true;
    err = "collapse: unknown kind";
    return false;
}

// the text two documents must share to be one group
inline std::string collapse_normalise(const std::string& field) {
    std::string out;
    for (const std::string& t : nextsearch::tokenize(field)) {
        if (!out.empty()) out.push_back(' ');
        out += t;
    }
    return out;
}

// dense ids by first appearance; feed the documents in manifest order
class CollapseIds {
public:
    uint32_t key_of(const std::string& field) {
        const std::string n = collapse_normalise(field);
        if (n.empty()) return 0u;
        const auto it = ids_.find(n);
        if (it != ids_.end()) return it->second;
        const uint32_t id = (uint32_t)ids_.size() + 1u;   // (an index holds fewer than 2^32 - 1 documents: never the reserved key)
        ids_.emplace(n, id);
        return id;
    }
    size_t groups() const { return ids_.size(); }

private:
    std::unordered_map<std::string, uint32_t> ids_;
};

// Custom keys against the index: one array per segment, one key per document, none the reserved key.  n_docs: the segments' sizes.
inline bool collapse_custom_check(const CollapseSpec& s, const std::vector<uint32_t>& n_docs, std::string& err) {
    if (s.custom.size() != n_docs.size()) { err = "collapse custom: " + std::to_string(s.custom.size()) + " key arrays for " + std::to_string(n_docs.size()) + " segments"; return false; }
    for (size_t i = 0; i < n_docs.size(); i++) {
        if (s.custom[i].size() != n_docs[i]) {
            err = "collapse custom: the key array of segment " + std::to_string(i) + " has " + std::to_string(s.custom[i].size()) + " entries, the segment " + std::to_string(n_docs[i]) + " documents";
            return false;
        }
        for (const uint32_t k : s.custom[i])
            if (k == kCollapseReservedKey) { err = "collapse custom: segment " + std::to_string(i) + " holds the reserved key 0xFFFFFFFF"; return false; }
    }
    return true;
}

// The collapsed call reads parse_boosted's dialect.  A `*` that parse_prefixed would read as a prefix term is refused there
// (derived segments would need group tables of their own: DESIGN.md §5ac, left out); -> the first such prefix, or "".
inline std::string collapse_first_prefix(const char* text, size_t n, std::vector<char>& scratch) {
    std::string first;
    for_each_prefixed_term(text, n, scratch, [&](const char* p, size_t len, uint8_t, uint32_t, uint32_t, float, bool star) {
        if (star && first.empty()) first.assign(p, len);
    });
    return first;
}

}  // namespace nsx
