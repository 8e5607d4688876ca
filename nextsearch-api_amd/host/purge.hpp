// Deleting documents: a segment that loses documents is REWRITTEN from its four forward files — a
// compaction of one source with a filter.  ns_forward_merge_keep drops the documents, their pairs and the terms nobody names
// any more on the device, ns_forward_invert builds the lists; reading and writing are compact.hpp's.  Search is not
// touched: there is no tombstone for a scoring kernel to consult.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "compact.hpp"

namespace nsx {

struct DeleteStats {
    uint32_t segments_rewritten = 0, segments_dropped = 0, docs_deleted = 0, uids_not_found = 0, terms_dropped = 0;
    uint64_t pairs_in = 0, pairs_out = 0, device_bytes = 0;   // pairs of the rewritten segments before and after; the largest rewrite's device memory
    float merge_ms = 0.0f, invert_ms = 0.0f;                  // HIP events around the device parts, summed over the rewritten segments
    double call_s = 0.0;                                      // ns_forward_merge_keep + fetch + ns_forward_invert, copies included, summed
    double total_s = 0.0;                                     // the whole call: files in -> files out, manifest, reload, removals
};

// start of every document's raw record in s.doc_records (n_docs + 1 entries); load_source has checked the layout
inline std::vector<size_t> doc_record_offsets(const SourceSegment& s) {
    const size_t n = s.doc_len.size();
    std::vector<size_t> at(n + 1, 0);
    size_t pos = 0;
    for (size_t d = 0; d < n; d++) {
        at[d] = pos;
        for (int k = 0; k < 3; k++) { uint32_t len; std::memcpy(&len, s.doc_records.data() + pos, 4); pos += 4 + (size_t)len; }
        pos += 4;
    }
    at[n] = pos;
    return at;
}

// The loaded source without the documents whose bit in keep (one bit per document, (n_docs + 31) / 32 words) is clear ->
// the complete segment out_seg.  At least one document must stay.  Nothing is written before the device work has
// succeeded; a directory this call created is removed again when a file cannot be written.
inline bool rewrite_loaded(ns_ctx* ctx, const SourceSegment& source, const std::vector<uint32_t>& keep, const fs::path& out_seg, DeleteStats& st, std::string& err) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    if (!ctx) { err = "rewrite_segment: no device context (deleting runs on the device; there is no CPU path)"; return false; }
    const uint32_t n_docs = (uint32_t)source.doc_len.size();
    if (keep.size() < ((size_t)n_docs + 31) / 32) { err = "rewrite_segment: the bitmap is shorter than the segment's documents"; return false; }
    ns_forward_src src{};
    fill_forward_src(source, src);
    const uint32_t* bits = keep.data();
    ns_forward* fwd = nullptr;
    if (ns_forward_merge_keep(ctx, &src, &bits, 1, &fwd) != NS_OK) { err = std::string(ns_last_error(ctx)) + " (" + source.dir.string() + ")"; return false; }
    MergedSegment m;
    m.info.struct_size = (uint32_t)sizeof(m.info);
    (void)ns_forward_get_info(fwd, &m.info);
    if (m.info.kept_docs == 0) { ns_forward_destroy(fwd); err = "rewrite_segment: no document of " + source.dir.string() + " stays"; return false; }
    float invert_ms = 0.0f;
    if (!fetch_merged(ctx, fwd, m, invert_ms, err)) return false;
    st.call_s += std::chrono::duration<double>(clk::now() - t0).count();
    st.merge_ms += m.info.device_ms; st.invert_ms += invert_ms;
    st.device_bytes = std::max<uint64_t>(st.device_bytes, m.info.device_bytes);
    st.pairs_in += src.n_pairs; st.pairs_out += m.info.n_pairs;
    st.terms_dropped += src.n_terms - m.info.n_terms;
    // docs.bin: the surviving records raw, runs of neighbours as one piece
    const std::vector<size_t> at = doc_record_offsets(source);
    std::vector<std::pair<const uint8_t*, size_t>> records;
    for (uint32_t d = 0; d < n_docs;) {
        if (!((bits[d >> 5] >> (d & 31u)) & 1u)) { d++; continue; }
        uint32_t e = d + 1;
        while (e < n_docs && ((bits[e >> 5] >> (e & 31u)) & 1u)) e++;
        records.emplace_back(source.doc_records.data() + at[d], at[e] - at[d]);
        d = e;
    }
    return write_merged(out_seg, m, records, err);
}

}  // namespace nsx
