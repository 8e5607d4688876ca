// The digit plan of the LSD radix sort in csrc/ns_invert.hip, for index inversion (invert_run) and for the sorts of text ingest
// and compaction (ig_sort): a pure function of the key range; and invert_plan, what the inversion derives from its
// per-document counts.  Host code only, like ns_call_plan.hpp: no HIP type and no runtime call; tests/radix_plan_harness.cpp
// and tests/merge_plan_harness.cpp compile it with g++ for the CPU suite.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "ns_facet_plan.hpp"     // fc_format
#include "ns_index_consts.hpp"   // kIvTile

namespace ns {

struct RadixPlan {
    int bits = 1;                   // the width of key_range - 1, at least 1
    int passes = 1;                 // ceil(bits / 11), 1 .. 3
    int pbits[3] = {8, 8, 8};       // the digit of pass p, lowest first: 8 .. 11 bits each, as even as possible
};

// The keys are the values below key_range (nothing else takes part in the sort), so the plan follows from key_range alone:
// no device -> host sync decides it.  The passes' digits cover `bits`; a digit is never narrower than 8 bits, the narrowest
// k_iv_hist_w / k_iv_pass instantiation.
inline RadixPlan radix_plan(uint32_t key_range) {
    RadixPlan r;
    while (r.bits < 32 && key_range > 1 && ((key_range - 1) >> r.bits) != 0) r.bits++;
    r.passes = std::max(1, (r.bits + 10) / 11);
    int left = r.bits;
    for (int p = 0; p < r.passes; p++) {
        const int share = (left + (r.passes - p) - 1) / (r.passes - p);
        r.pbits[p] = std::min(11, std::max(8, share));
        left = std::max(0, left - r.pbits[p]);
    }
    return r;
}

// What ns_invert_forward derives from the per-document counts before it touches the device.
struct InvertPlan {
    RadixPlan rp;                       // of n_terms
    std::vector<uint64_t> prefix;       // n_docs + 1: a document's first pair
    uint32_t n_tiles = 0;               // ceil(n_pairs / kIvTile)
    std::vector<uint32_t> tile_docs;    // per tile {document of its first pair, document of its last pair}
    size_t m_max = 0;                   // the most digit counters of a pass: bins x tiles
    uint32_t scan_blocks_max = 0;       // ceil(m_max / 1024)
};

// n_pairs is below 2^32 - kIvTile (the caller has checked).  False with `err` set where the counts do not sum to n_pairs.
__attribute__((noinline)) inline bool invert_plan(const uint32_t* doc_term_counts, uint32_t n_docs, uint64_t n_pairs, uint32_t n_terms, InvertPlan& out, std::string& err) {
    out = InvertPlan();
    std::vector<uint64_t>& prefix = out.prefix;
    prefix.assign((size_t)n_docs + 1, 0);
    for (uint32_t d = 0; d < n_docs; d++) prefix[d + 1] = prefix[d] + doc_term_counts[d];
    if (prefix[n_docs] != n_pairs) {
        err = fc_format("the per-document counts sum to %llu, not to n_pairs = %llu", (unsigned long long)prefix[n_docs], (unsigned long long)n_pairs);
        return false;
    }
    const uint32_t n = (uint32_t)n_pairs;
    out.n_tiles = (n + kIvTile - 1) / kIvTile;
    out.rp = radix_plan(n_terms);
    for (int p = 0; p < out.rp.passes; p++) out.m_max = std::max(out.m_max, ((size_t)1 << out.rp.pbits[p]) * out.n_tiles);
    out.scan_blocks_max = (uint32_t)((out.m_max + 1023) / 1024);
    // the documents that hold each tile's first and last pair (the first pass marks the documents that start in between):
    // the last d with prefix[d] <= i
    out.tile_docs.resize((size_t)out.n_tiles * 2);
    uint32_t d = 0;
    auto doc_of = [&](uint64_t i) { while (d + 1 < n_docs && prefix[d + 1] <= i) d++; return d; };   // i ascends: one sweep over the documents
    for (uint32_t t = 0; t < out.n_tiles; t++) {
        const uint64_t i0 = (uint64_t)t * kIvTile, i1 = std::min<uint64_t>(i0 + kIvTile, n) - 1;
        out.tile_docs[2 * (size_t)t] = doc_of(i0);
        out.tile_docs[2 * (size_t)t + 1] = doc_of(i1);
    }
    return true;
}

}  // namespace ns
