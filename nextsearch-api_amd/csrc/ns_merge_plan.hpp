// What ns_forward_merge and ns_forward_merge_keep derive from their sources before they touch the
// device: the totals and their limits, the per-source bases, the document prefix, what survives the bitmaps, the source
// terms' (start, length) in the concatenated term bytes and the documents by size class.
// Host code only, like ns_call_plan.hpp: no HIP type and no runtime call; tests/merge_plan_harness.cpp compiles it with g++
// for the CPU suite.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/nextsearch_hip.h"
#include "ns_facet_plan.hpp"     // fc_format
#include "ns_index_consts.hpp"   // kIvTile, kCpWaveMax, kCpDocCut

namespace ns {

struct MergePlan {
    bool filtered = false;          // some source has a bitmap: the stages of ns_delete.hip run
    uint32_t raw_pairs = 0;         // the sources' pairs
    uint32_t T = 0;                 // the sources' terms
    uint32_t text_bytes = 0;        // the sources' term bytes, back to back
    uint32_t n_docs = 0, n_pairs = 0;   // filtered: the survivors'
    uint64_t total_len = 0;         // the sum of the (surviving) documents' doc_len
    std::vector<uint32_t> term_base, pair_base;   // n_src + 1 each; pair_base counts surviving pairs
    std::vector<uint32_t> prefix;                 // n_docs + 1: a document's first pair in the result
    std::vector<uint32_t> kstart, klen;           // T each: a source term's bytes in the concatenated term bytes
    // filtered only: where a source's pairs lie in the upload, per surviving document its first pair there, its doc_len and
    // count, and per source term 1 where the source has no bitmap (its terms all stay)
    std::vector<uint32_t> raw_base, srcpos, kept_len, kept_cnt, live0;
    // the documents by size class: sorted by a wave, by a workgroup in LDS, or by the global radix sort (a document of one
    // pair is in order as it is).  lists: the three lists of documents, then the big list's n_bigdocs + 1 pair prefix
    std::vector<uint32_t> lists;
    uint32_t n_wave = 0, n_lds = 0, n_bigdocs = 0, n_big = 0;
};

// The totals, from the counts alone (no array is read), then what has to hold of every source's arrays before one is walked.
// The loops of this header run once per source, document or term; each is a function of its own that is never inlined, so
// that its code does not depend on the function around it (profiles/call_block/README.md).
__attribute__((noinline)) inline bool merge_totals(const ns_forward_src* src, uint32_t n_src, MergePlan& p, uint64_t& docs64, std::string& err) {
    uint64_t pairs64 = 0, terms64 = 0;
    docs64 = 0;
    for (uint32_t s = 0; s < n_src; s++) {
        docs64 += src[s].n_docs; terms64 += src[s].n_terms;
        if (src[s].n_pairs >= (1ull << 32) || (pairs64 += src[s].n_pairs) >= (1ull << 32) - kIvTile) {
            err = fc_format("more than %llu pairs up to source %u; this build indexes pairs with 32 bits (compact fewer segments)", (unsigned long long)((1ull << 32) - kIvTile - 1), s);
            return false;
        }
    }
    if (docs64 >= 0xFFFFFFFFull) { err = fc_format("%llu documents; docIds are 32 bits wide (below 2^32 - 1: compact fewer segments)", (unsigned long long)docs64); return false; }
    if (terms64 >= (1ull << 31)) { err = fc_format("%llu source terms; the dictionary holds fewer than 2^31 (compact fewer segments)", (unsigned long long)terms64); return false; }
    uint64_t bytes64 = 0;
    for (uint32_t s = 0; s < n_src; s++) {
        const ns_forward_src& S = src[s];
        if ((S.n_docs && (!S.doc_len || !S.counts)) || (S.n_pairs && !S.pairs) || (S.n_terms && !S.term_offsets)) { err = fc_format("source %u: null array", s); return false; }
        if (S.n_terms) {
            if (S.term_offsets[S.n_terms] < S.term_offsets[0]) { err = fc_format("source %u: term offsets decrease", s); return false; }
            bytes64 += S.term_offsets[S.n_terms] - S.term_offsets[0];
            if (bytes64 >= (1ull << 32) - 65536) { err = fc_format("more than 4 GiB - 64 KiB of term bytes up to source %u; this build addresses them with 32 bits (compact fewer segments)", s); return false; }
        }
    }
    p.raw_pairs = (uint32_t)pairs64; p.T = (uint32_t)terms64; p.text_bytes = (uint32_t)bytes64;
    return true;
}

// One walk over the sources' documents and terms: the bases, the prefix, the survivors, the terms' places.
__attribute__((noinline)) inline bool merge_walk(const ns_forward_src* src, const uint32_t* const* keep, uint32_t n_src, MergePlan& p, std::string& err) {
    const bool filtered = p.filtered;
    std::vector<uint32_t>&term_base = p.term_base, &pair_base = p.pair_base, &raw_base = p.raw_base, &prefix = p.prefix;
    uint32_t d = 0, k = 0, at = 0;
    for (uint32_t s = 0; s < n_src; s++) {
        const ns_forward_src& S = src[s];
        uint64_t sum = 0;
        if (!filtered) {
            for (uint32_t j = 0; j < S.n_docs; j++, d++) { sum += S.counts[j]; p.total_len += S.doc_len[j]; prefix[d + 1] = (uint32_t)(pair_base[s] + sum); if (sum > S.n_pairs) break; }
            pair_base[s + 1] = pair_base[s] + (uint32_t)S.n_pairs;
        } else {
            const uint32_t* bits = keep[s];
            uint64_t stay = 0;                                     // pairs of the source's surviving documents so far
            for (uint32_t j = 0; j < S.n_docs; j++) {
                const uint32_t c = S.counts[j];
                if (!bits || ((bits[j >> 5] >> (j & 31u)) & 1u)) {
                    p.srcpos.push_back(raw_base[s] + (uint32_t)sum); p.kept_len.push_back(S.doc_len[j]); p.kept_cnt.push_back(c);
                    p.total_len += S.doc_len[j];
                    stay += c;
                    prefix[++d] = (uint32_t)(pair_base[s] + stay);
                }
                sum += c;
                if (sum > S.n_pairs) break;
            }
            raw_base[s + 1] = raw_base[s] + (uint32_t)S.n_pairs;
            pair_base[s + 1] = pair_base[s] + (uint32_t)stay;
            if (!bits) std::fill(p.live0.begin() + term_base[s], p.live0.begin() + term_base[s] + S.n_terms, 1u);
        }
        if (sum != S.n_pairs) { err = fc_format("source %u: the per-document counts do not sum to n_pairs = %llu", s, (unsigned long long)S.n_pairs); return false; }
        for (uint32_t t = 0; t < S.n_terms; t++, k++) {
            if (S.term_offsets[t + 1] < S.term_offsets[t]) { err = fc_format("source %u: term offsets decrease at term %u", s, t); return false; }
            p.kstart[k] = at + (uint32_t)(S.term_offsets[t] - S.term_offsets[0]);
            p.klen[k] = (uint32_t)(S.term_offsets[t + 1] - S.term_offsets[t]);
        }
        if (S.n_terms && S.term_offsets[S.n_terms] != S.term_offsets[0] && !S.term_bytes) { err = fc_format("source %u: term_bytes is NULL", s); return false; }
        if (S.n_terms) at += (uint32_t)(S.term_offsets[S.n_terms] - S.term_offsets[0]);
        term_base[s + 1] = term_base[s] + S.n_terms;
    }
    if (filtered) { p.n_docs = d; p.n_pairs = pair_base[n_src]; prefix.resize((size_t)p.n_docs + 1); }
    return true;
}

// The documents by size class.  cp_inplace off (ns_ctx_use_docsort): everything of two or more pairs goes to the big list.
__attribute__((noinline)) inline void merge_classes(bool cp_inplace, MergePlan& p) {
    std::vector<uint32_t> l_wave, l_lds, l_big, big_prefix(1, 0);
    for (uint32_t d = 0; d < p.n_docs; d++) {
        const uint32_t c = p.prefix[d + 1] - p.prefix[d];
        if (c < 2) continue;
        if (cp_inplace && c <= kCpWaveMax) l_wave.push_back(d);
        else if (cp_inplace && c <= kCpDocCut) l_lds.push_back(d);
        else { l_big.push_back(d); big_prefix.push_back(big_prefix.back() + c); }
    }
    p.n_wave = (uint32_t)l_wave.size(); p.n_lds = (uint32_t)l_lds.size(); p.n_bigdocs = (uint32_t)l_big.size(); p.n_big = big_prefix.back();
    p.lists.clear();
    p.lists.reserve((size_t)p.n_wave + p.n_lds + 2 * (size_t)p.n_bigdocs + 1);
    p.lists.insert(p.lists.end(), l_wave.begin(), l_wave.end());
    p.lists.insert(p.lists.end(), l_lds.begin(), l_lds.end());
    p.lists.insert(p.lists.end(), l_big.begin(), l_big.end());
    p.lists.insert(p.lists.end(), big_prefix.begin(), big_prefix.end());
}

// keep == NULL, or every keep[s] NULL: the plain merge.  False with `err` set (the caller puts its name in front), and
// nothing usable in `p`.  The checks fire in this order: the totals, every source's arrays, then source by source its counts,
// its term offsets and its term bytes.
inline bool merge_plan(const ns_forward_src* src, const uint32_t* const* keep, uint32_t n_src, bool cp_inplace, MergePlan& p, std::string& err) {
    p = MergePlan();
    uint64_t docs64 = 0;
    if (!merge_totals(src, n_src, p, docs64, err)) return false;
    for (uint32_t s = 0; keep && s < n_src; s++) p.filtered = p.filtered || keep[s] != nullptr;
    p.n_docs = (uint32_t)docs64; p.n_pairs = p.raw_pairs;              // filtered: the survivors', set by the walk
    p.term_base.assign((size_t)n_src + 1, 0); p.pair_base.assign((size_t)n_src + 1, 0);
    p.kstart.resize(p.T); p.klen.resize(p.T);
    p.prefix.assign((size_t)p.n_docs + 1, 0);
    if (p.filtered) { p.raw_base.assign((size_t)n_src + 1, 0); p.srcpos.reserve(p.n_docs); p.kept_len.reserve(p.n_docs); p.kept_cnt.reserve(p.n_docs); p.live0.assign((size_t)p.T + 1, 0); }
    if (!merge_walk(src, keep, n_src, p, err)) return false;
    merge_classes(cp_inplace, p);
    return true;
}

}  // namespace ns
