// "More like this" (DESIGN.md §5n): the step in front of the scoring launch.  For a source document pick its most telling
// terms from its forward pairs; the engine then scores them as an ordinary weighted OR query.  The reference has no such
// call.  This file is the authority on the SELECTION RULE; csrc/ns_similar.hip (ns_docterms_select) and
// tests/similar_ref.py restate it and are compared with it bit for bit.
//
// Inputs: document d of segment s has the pairs (t, tf) of forward.bin; per term id t of that segment df[t] / idf[t] come
// from the segment's OWN lexicon entry for the byte string terms.bin[t] (similar_term_stats): idf[t] = bm25_idf(N_s, df[t]),
// the host's glibc logf value, exactly what TermDict holds for search.  A term without a lexicon entry has df = 0.
//
//   qualifying   tf >= max(min_tf, 1)  and  min_df <= df[t] <= max_df  and  df[t] >= 1  and  0 < idf[t] < inf
//   weight       w = (float)tf * idf[t], ONE fp32 multiply.  w > 0, so its bit pattern orders as an unsigned integer
//   selection    the first T = clamp(max_terms, 1, 32) qualifying pairs by (w bits descending, termId ascending):
//                64-bit key = w bits << 32 | ~termId, descending.  A key is never 0 (w bits >= 1): 0 means "no pair"
//   rows         term_out[i * T + r] / w_out[i * T + r], r < count_out[i]; past the count ~0u and 0.0f
//
// df / idf are per SEGMENT: in an index of several segments the same word weighs differently in each; after compact()
// the one segment's numbers are the index's.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "compact.hpp"
#include "index_format.hpp"

namespace nsx {

constexpr uint32_t kSimilarMaxTerms = 32;

struct SimilarOptions {
    uint32_t max_terms = 25;            // Lucene's MoreLikeThis default
    uint32_t min_tf = 1;                // Lucene: 2 — too strict for abstracts
    uint32_t min_df = 1;                // Lucene: 5 — wrong for the small segments add_documents makes
    uint32_t max_df = 0xFFFFFFFFu;
    bool boost = false;                 // qweight = w / w_first instead of 1.0f
};

inline uint32_t similar_clamp_terms(uint32_t max_terms) { return max_terms < 1 ? 1u : (max_terms > kSimilarMaxTerms ? kSimilarMaxTerms : max_terms); }
inline uint32_t similar_clamp_min_tf(uint32_t min_tf) { return min_tf < 1 ? 1u : min_tf; }

inline bool similar_qualifies(uint32_t tf, uint32_t df, float idf, uint32_t min_tf, uint32_t min_df, uint32_t max_df) {
    return tf >= similar_clamp_min_tf(min_tf) && df >= 1 && df >= min_df && df <= max_df && idf > 0.0f && idf <= std::numeric_limits<float>::max();
}

// 0: the pair does not qualify
inline uint64_t similar_key(uint32_t term, uint32_t tf, uint32_t df, float idf, uint32_t min_tf, uint32_t min_df, uint32_t max_df) {
    if (!similar_qualifies(tf, df, idf, min_tf, min_df, max_df)) return 0;
    const float w = (float)tf * idf;
    uint32_t bits;
    std::memcpy(&bits, &w, 4);
    return ((uint64_t)bits << 32) | (uint32_t)~term;
}

// The query weight of a selected term: 1.0f, or with boost w / w_first (one IEEE fp32 division)
inline float similar_qweight(float w, float w_first, bool boost) { return boost ? w / w_first : 1.0f; }

// The selection on one host thread: the CPU tests' subject and the bench's baseline.  doc_off[n_docs + 1]: first pair of
// each document.  Streaming: a sorted array of the T best keys so far, a pair enters only when it beats the last one.
// false for a doc id or a termId out of range (nothing useful is written then).
inline bool similar_select_host(const uint64_t* doc_off, uint32_t n_docs, const uint32_t* pairs, const uint32_t* df, const float* idf,
                                uint32_t n_terms, const uint32_t* doc_ids, uint32_t n, uint32_t max_terms, uint32_t min_tf, uint32_t min_df,
                                uint32_t max_df, uint32_t* term_out, float* w_out, uint32_t* count_out) {
    const uint32_t T = similar_clamp_terms(max_terms);
    for (uint32_t i = 0; i < n; i++) {
        if (doc_ids[i] >= n_docs) return false;
        uint64_t best[kSimilarMaxTerms];
        uint32_t have = 0;
        for (uint64_t p = doc_off[doc_ids[i]]; p < doc_off[doc_ids[i] + 1]; p++) {
            const uint32_t t = pairs[2 * p], tf = pairs[2 * p + 1];
            if (t >= n_terms) return false;
            const uint64_t key = similar_key(t, tf, df[t], idf[t], min_tf, min_df, max_df);
            if (key == 0 || (have == T && key <= best[T - 1])) continue;
            uint32_t at = have < T ? have++ : T - 1;
            while (at > 0 && best[at - 1] < key) { best[at] = best[at - 1]; at--; }
            best[at] = key;
        }
        for (uint32_t r = 0; r < T; r++) {
            const uint64_t key = r < have ? best[r] : 0;
            const uint32_t bits = (uint32_t)(key >> 32);
            term_out[(size_t)i * T + r] = ~(uint32_t)key;          // key 0: ~0u
            std::memcpy(&w_out[(size_t)i * T + r], &bits, 4);     // key 0: 0.0f
        }
        count_out[i] = have;
    }
    return true;
}

// df / idf by term id of a loaded segment: the lexicon entry of the byte string terms.bin[t]; absent: df 0, idf 0
template <class IdfFn>
inline void similar_term_stats(const SegmentData& seg, const SourceSegment& src, IdfFn idf_of, std::vector<uint32_t>& df, std::vector<float>& idf) {
    const size_t n_terms = src.term_offsets.empty() ? 0 : src.term_offsets.size() - 1;
    df.assign(n_terms, 0u);
    idf.assign(n_terms, 0.0f);
    std::string key;
    for (size_t t = 0; t < n_terms; t++) {
        key.assign((const char*)src.term_bytes.data() + src.term_offsets[t], (size_t)(src.term_offsets[t + 1] - src.term_offsets[t]));
        const auto it = seg.lex.find(key);
        if (it == seg.lex.end() || it->second.df == 0) continue;
        df[t] = it->second.df;
        idf[t] = idf_of(seg.N, it->second.df);
    }
}

}  // namespace nsx
