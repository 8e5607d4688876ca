// Spelling correction's host side ("did you mean"): the rules that sit in front of ns_ac_fuzzy
// (csrc/ns_fuzzy.hip).  The dictionary is autocomplete's sorted table (suggest.hpp); the device ranks its candidates by
// (distance, score desc, index asc).
//
//   normalising      query terms go through normalize_token like the table's terms (ASCII alnum bytes, lower-cased)
//   max_edits auto   by normalised length: under 3 bytes 0 edits, 3..5 one, above 5 two
//   limits           a term of 0 or more than kFuzzyMaxLen bytes has no answer and never reaches the device
//   did_you_mean     tokens = tokenize()'s alnum runs; stop words and tokens under 2 bytes are skipped; a token the term
//                    dictionary holds is "known" (that is what search can match) and gets no device work
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "textutil.hpp"

namespace nsx {

static constexpr size_t kFuzzyMaxLen = 64;   // NS_FUZZY_MAX_LEN
static constexpr int kFuzzyMaxEdits = 2;     // NS_FUZZY_MAX_EDITS

inline int correct_auto_edits(size_t normalized_len) { return normalized_len < 3 ? 0 : normalized_len <= 5 ? 1 : 2; }

// The alnum runs of a query with their place in it: token = input[at, at + len) lower-cased.
struct QueryToken { size_t at, len; std::string text; };

inline std::vector<QueryToken> correct_tokens(const std::string& input) {
    std::vector<QueryToken> out;
    size_t i = 0;
    while (i < input.size()) {
        while (i < input.size() && !nextsearch::is_alnum_ascii((unsigned char)input[i])) i++;
        const size_t at = i;
        while (i < input.size() && nextsearch::is_alnum_ascii((unsigned char)input[i])) i++;
        if (i == at) break;
        QueryToken t{at, i - at, std::string()};
        for (size_t j = at; j < i; j++) {
            const char c = input[j];
            t.text.push_back((c >= 'A' && c <= 'Z') ? (char)(c - 'A' + 'a') : c);
        }
        out.push_back(std::move(t));
    }
    return out;
}

}  // namespace nsx
