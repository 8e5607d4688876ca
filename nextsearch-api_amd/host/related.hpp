// Related terms: the terms that tell what a SET of documents is about — a result page's "refine your search"
// chips.  The reference has no such call.  This file is the authority on the RULE; csrc/ns_terms.hip (ns_docterms_aggregate)
// and tests/related_ref.py restate it and are compared with it bit for bit.
//
// Inputs: the forward pairs (t, tf) of one segment's documents and df[t] / idf[t] by term id, exactly what §5n's selection
// reads (similar.hpp, similar_term_stats).  A ROW is a set of documents of that segment.
//
//   rows         a row's doc ids are sorted and repeats dropped: a document named twice counts once.  A row keeps at most
//                kRelatedMaxDocs = 255 distinct documents (the device counts in bytes); one with more is refused.  An empty
//                row is valid and gives count 0
//   counting     fg[t] = how many of the row's documents hold a pair (t, tf) with tf >= max(min_tf, 1)
//   qualifying   fg[t] >= max(min_docs, 1)  and  min_df <= df[t] <= max_df  and  df[t] >= 1  and  0 < idf[t] < inf
//   weight       w = (float)fg[t] * idf[t], ONE fp32 multiply; no division, no log
//   selection    the first T = clamp(max_terms, 1, 64) qualifying terms by (w bits descending, termId ascending):
//                64-bit key = w bits << 32 | ~termId, descending.  A key is never 0 (w bits >= 1): 0 means "nothing"
//   outputs      term_out / docs_out (= fg) / w_out [i * T + r], r < count_out[i]; past the count ~0u, 0 and 0.0f;
//                ndocs_out[i] = the distinct documents of row i
//
// Term ids are unique inside a document and ascending (the order ns_forward_fetch documents and every segment writer
// keeps); a document that breaks it is refused here where a row visits it, and by the device for the whole handle.
//
// Across segments (Engine::terms_batch): see related_merge below.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace nsx {

constexpr uint32_t kRelatedMaxDocs = 255;       // distinct documents of a row
constexpr uint32_t kRelatedMaxTerms = 64;       // T of one segment's aggregate (a wave's kept set)
constexpr uint32_t kRelatedMaxOut = 32;         // terms of a merged answer (Engine::terms_batch)

struct RelatedOptions {
    uint32_t max_terms = 10;
    uint32_t min_tf = 1;
    uint32_t min_docs = 2;              // a term of ONE document says nothing about the set
    uint32_t min_df = 1;
    uint32_t max_df = 0xFFFFFFFFu;
    uint32_t sample = 100;              // related_terms: the hits the row is made of, 1..100
};

inline uint32_t related_clamp_terms(uint32_t max_terms) { return max_terms < 1 ? 1u : (max_terms > kRelatedMaxTerms ? kRelatedMaxTerms : max_terms); }
inline uint32_t related_clamp_out(uint32_t max_terms) { return max_terms < 1 ? 1u : (max_terms > kRelatedMaxOut ? kRelatedMaxOut : max_terms); }
inline uint32_t related_clamp_sample(uint32_t sample) { return sample < 1 ? 1u : (sample > 100u ? 100u : sample); }

// 0: the term does not qualify
inline uint64_t related_key(uint32_t term, uint32_t fg, uint32_t df, float idf, uint32_t min_docs, uint32_t min_df, uint32_t max_df) {
    if (fg < (min_docs < 1 ? 1u : min_docs) || df < 1 || df < min_df || df > max_df || !(idf > 0.0f) || !(idf <= std::numeric_limits<float>::max())) return 0;
    const float w = (float)fg * idf;
    uint32_t bits;
    std::memcpy(&bits, &w, 4);
    return ((uint64_t)bits << 32) | (uint32_t)~term;
}

// The rule on one host thread, over the arrays the device call takes: the CPU tests' subject and the bench's baseline.
// doc_off[n_docs + 1]: first pair of each document.  One counter per term id, the touched ids remembered so that a row
// costs its own pairs, not n_terms.  0: done; -1: refused (row_off does not start at 0 or descends, a doc id or termId out
// of range, a row of more than kRelatedMaxDocs distinct documents, a visited document whose ids do not ascend) — nothing
// useful is written then.
inline int related_aggregate_host(const uint64_t* doc_off, uint32_t n_docs, const uint32_t* pairs, const uint32_t* df, const float* idf,
                                  uint32_t n_terms, const uint32_t* doc_ids, const uint64_t* row_off, uint32_t n_rows, uint32_t max_terms,
                                  uint32_t min_tf, uint32_t min_docs, uint32_t min_df, uint32_t max_df, uint32_t* term_out, uint32_t* docs_out,
                                  float* w_out, uint32_t* count_out, uint32_t* ndocs_out) {
    const uint32_t T = related_clamp_terms(max_terms), need_tf = min_tf < 1 ? 1u : min_tf;
    if (n_rows && row_off[0] != 0) return -1;
    std::vector<uint16_t> fg(n_terms, 0);
    std::vector<uint32_t> touched, ids;
    for (uint32_t i = 0; i < n_rows; i++) {
        if (row_off[i + 1] < row_off[i]) return -1;
        ids.assign(doc_ids + row_off[i], doc_ids + row_off[i + 1]);
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        if (ids.size() > kRelatedMaxDocs || (!ids.empty() && ids.back() >= n_docs)) return -1;
        touched.clear();
        for (const uint32_t d : ids) {
            for (uint64_t p = doc_off[d]; p < doc_off[d + 1]; p++) {
                const uint32_t t = pairs[2 * p], tf = pairs[2 * p + 1];
                if (t >= n_terms || (p > doc_off[d] && pairs[2 * (p - 1)] >= t)) return -1;
                if (tf < need_tf) continue;
                if (fg[t]++ == 0) touched.push_back(t);
            }
        }
        uint64_t best[kRelatedMaxTerms];
        uint32_t have = 0;
        for (const uint32_t t : touched) {
            const uint64_t key = related_key(t, fg[t], df[t], idf[t], min_docs, min_df, max_df);
            if (key == 0 || (have == T && key <= best[T - 1])) continue;
            uint32_t at = have < T ? have++ : T - 1;
            while (at > 0 && best[at - 1] < key) { best[at] = best[at - 1]; at--; }
            best[at] = key;
        }
        for (uint32_t r = 0; r < T; r++) {
            const uint64_t key = r < have ? best[r] : 0;
            const uint32_t bits = (uint32_t)(key >> 32), t = ~(uint32_t)key;
            term_out[(size_t)i * T + r] = t;                           // key 0: ~0u
            docs_out[(size_t)i * T + r] = key ? fg[t] : 0u;
            std::memcpy(&w_out[(size_t)i * T + r], &bits, 4);         // key 0: 0.0f
        }
        count_out[i] = have;
        ndocs_out[i] = (uint32_t)ids.size();
        for (const uint32_t t : touched) fg[t] = 0;
    }
    return 0;
}

// ---- across segments (Engine::terms_batch) ------------------------------------------------------------------------------
// A row may name documents of several segments.  Each touched segment answers its part of the row with T = 64
// (ns_docterms_aggregate over that segment's own df / idf); the lists meet here:
//   candidates   the union of the per-segment lists, by byte string
//   docs         the sum of fg over the lists that hold the term
//   df, N        the term's lexicon df summed over ALL loaded segments; N = the sum of their document counts
//   w            (float)docs * idf(N, df), idf the engine's bm25_idf
//   order        w bits descending, then the first manifest position whose list holds the term, then the term id there
//   cut          clamp(max_terms, 1, 32), after the caller has dropped what it wants dropped (related_terms: the query's own terms)
// With one segment this is the device row itself (same df, same N, so the same idf bits) and exact.  With several a term
// that misses one segment's 64 loses that segment's fg: docs is a lower bound.  compact() makes it exact.
struct RelatedCand {
    std::string term;
    uint32_t docs = 0;          // summed fg
    uint64_t df = 0;            // over all loaded segments
    float w = 0.0f;
    uint32_t first_pos = 0;     // first manifest position whose list holds the term
    uint32_t term_id = 0;       // the term's id in that segment
};

inline void related_merge_order(std::vector<RelatedCand>& c) {
    auto bits = [](float w) { uint32_t b; std::memcpy(&b, &w, 4); return b; };
    std::sort(c.begin(), c.end(), [&](const RelatedCand& a, const RelatedCand& b) {
        const uint32_t wa = bits(a.w), wb = bits(b.w);
        if (wa != wb) return wa > wb;
        if (a.first_pos != b.first_pos) return a.first_pos < b.first_pos;
        return a.term_id < b.term_id;
    });
}

}  // namespace nsx
