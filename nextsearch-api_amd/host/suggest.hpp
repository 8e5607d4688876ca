// Autocomplete's host side: the reference's AutocompleteIndex (src/api_autocomplete.cpp, built in Engine::reload at
// src/api_engine.cpp:91-107, queried by Engine::suggest at :164-187) restated as a SORTED TABLE that the device answers
// from (csrc/ns_suggest.hip).
//
//   score(term)        the u32 sum of LexEntry.df over all loaded segments, per RAW lexicon term (:97-103; wraps like
//                      the reference's `uint32_t +=`; a df of 0 still makes an entry)
//   normalize_token    keep the ASCII alnum bytes (C locale isalnum), lower-case them (api_autocomplete.cpp:23-30)
//   < 2 bytes          dropped after normalising (:101); two raw terms that normalise alike stay two entries
//   order              by bytes; the device ranks a prefix's range by (score desc, term asc) == (score desc, index asc)
//   request            the last alnum run of the input is the prefix (trailing non-alnum bytes dropped); the raw bytes
//                      before it are the base; suggestion = base + term (api_autocomplete.cpp:171-200)
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../csrc/ns_forkjoin.hpp"
#include "index_format.hpp"
#include "textutil.hpp"

namespace nsx {

static constexpr int kSuggestMaxLimit = 10;   // src/api_engine.cpp:171: clamp to 1..10

inline int clamp_suggest_limit(int limit) { return std::max(1, std::min(limit, kSuggestMaxLimit)); }

// normalize_token over raw bytes, appended to `out`
inline void normalize_token(const char* p, size_t n, std::string& out) {
    for (size_t i = 0; i < n; i++) {
        const unsigned char c = (unsigned char)p[i];
        if (nextsearch::is_alnum_ascii(c)) out.push_back((c >= 'A' && c <= 'Z') ? (char)(c - 'A' + 'a') : (char)c);
    }
}

// The request split (api_autocomplete.cpp:176-187): the last alnum run of the input is [start, end) — trailing
// non-alnum bytes are skipped — the base is input[0, start), the prefix the run lower-cased (it is all alnum).
inline void suggest_last_run(const char* p, size_t n, size_t& start, size_t& end) {
    end = n;
    while (end > 0 && !nextsearch::is_alnum_ascii((unsigned char)p[end - 1])) end--;
    start = end;
    while (start > 0 && nextsearch::is_alnum_ascii((unsigned char)p[start - 1])) start--;
}

inline void split_suggest_input(const char* p, size_t n, size_t& base_len, std::string& prefix) {
    size_t end = 0;
    suggest_last_run(p, n, base_len, end);
    prefix.clear();
    normalize_token(p + base_len, end - base_len, prefix);
}

// The sorted (term, score) table.  Term i = pool[off[i], off[i + 1]).
struct SuggestTable {
    std::string pool;
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> score;
    size_t max_len = 0;

    size_t size() const { return score.size(); }
    const char* term(size_t i) const { return pool.data() + off[i]; }
    size_t term_len(size_t i) const { return (size_t)(off[i + 1] - off[i]); }

    // `pool`: host threads for the sort (nullptr: the calling thread alone)
    void build(const std::vector<SegmentData>& segments, ForkJoin* fj) {
        // df summed per raw term (the reference's std::unordered_map<std::string, uint32_t> term_to_score)
        std::unordered_map<std::string, uint32_t> raw;
        size_t total = 0;
        for (const auto& seg : segments) total += seg.lex.size();
        raw.reserve(total);
        for (const auto& seg : segments)
            for (const auto& kv : seg.lex) raw[kv.first] += kv.second.df;
        struct Ent { uint64_t off; uint32_t len; uint32_t score; };
        std::string norm;
        std::vector<Ent> ents;
        ents.reserve(raw.size());
        norm.reserve(raw.size() * 8);
        for (const auto& kv : raw) {
            const size_t at = norm.size();
            normalize_token(kv.first.data(), kv.first.size(), norm);
            const size_t len = norm.size() - at;
            if (len < 2) { norm.resize(at); continue; }
            ents.push_back(Ent{(uint64_t)at, (uint32_t)len, kv.second});
        }
        // bytes ascending; equal bytes: score descending (such entries print alike, the order only makes the table canonical)
        const char* base = norm.data();
        auto less = [base](const Ent& a, const Ent& b) {
            const int c = std::memcmp(base + a.off, base + b.off, std::min(a.len, b.len));
            if (c != 0) return c < 0;
            if (a.len != b.len) return a.len < b.len;
            return a.score > b.score;
        };
        const unsigned nt = fj ? std::min<unsigned>(fj->width(), (unsigned)std::max<size_t>(1, ents.size() / 65536)) : 1u;
        if (nt <= 1) {
            std::sort(ents.begin(), ents.end(), less);
        } else {   // slices sorted on the pool, then merged pairwise (every round's merges in parallel)
            std::vector<size_t> cut(nt + 1);
            for (unsigned i = 0; i <= nt; i++) cut[i] = ents.size() * i / nt;
            fj->run(nt, [&](unsigned i) { std::sort(ents.begin() + cut[i], ents.begin() + cut[i + 1], less); });
            for (unsigned step = 1; step < nt; step *= 2) {
                const unsigned pairs = (nt + 2 * step - 1) / (2 * step);
                fj->run(pairs, [&](unsigned p) {
                    const unsigned a = p * 2 * step, m = std::min(a + step, nt), b = std::min(a + 2 * step, nt);
                    if (m < b) std::inplace_merge(ents.begin() + cut[a], ents.begin() + cut[m], ents.begin() + cut[b], less);
                });
            }
        }
        pool.clear();
        pool.reserve(norm.size());
        off.assign(1, 0);
        off.reserve(ents.size() + 1);
        score.clear();
        score.reserve(ents.size());
        max_len = 0;
        for (const Ent& e : ents) {
            pool.append(base + e.off, e.len);
            off.push_back(pool.size());
            score.push_back(e.score);
            max_len = std::max<size_t>(max_len, e.len);
        }
    }
};

}  // namespace nsx
