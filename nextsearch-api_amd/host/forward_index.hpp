// The reference's `forwardindex` tool (src/ForwardIndex.cpp) from the string it hands to tokenize (:139) onwards, with
// tokenising, tf counting and the term dictionary done on the device (ns_forward_build, csrc/ns_ingest.hip): writes
// docs.bin, stats.bin, forward.bin and terms.bin in the reference's layout (:189-230).  Reading metadata.csv and the
// CORD-19 JSON files (:109-137, cordjson.hpp) stays with the caller: a document arrives as {cord_uid, title,
// json_relpath, text}.
// Term ids are this project's (include/nextsearch_hip.h, ns_forward_build): rank of a term's first kept occurrence.
#pragma once

#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "index_format.hpp"
#include "nextsearch_hip.h"

namespace nsx {

struct DocInput {            // src/ForwardIndex.cpp:26-31 (DocInfo) + the text
    std::string cord_uid, title, json_relpath, text;
};

struct IndexStats {
    uint32_t n_docs_in = 0, n_docs = 0, n_terms = 0;
    uint64_t text_bytes = 0, tokens = 0, kept_tokens = 0, pairs = 0, device_bytes = 0;
    float avgdl = 0.0f;
    float device_ms = 0.0f;   // HIP events around the device part
    double call_s = 0.0;      // ns_forward_build + ns_forward_fetch, copies included
    double total_s = 0.0;     // documents in -> files out
};

// false + err when the device call fails, a file cannot be written, or no document survives (nothing is written then:
// the reference would write a segment with zero documents that no query can hit).
inline bool index_documents(ns_ctx* ctx, const std::vector<DocInput>& docs, const fs::path& segdir, IndexStats& st, std::string& err) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    st = IndexStats{};
    if (!ctx) { err = "index_documents: no device context (indexing runs on the device; there is no CPU path)"; return false; }
    if (docs.size() >= 0xFFFFFFFFull) { err = "index_documents: too many documents"; return false; }
    const uint32_t n_in = (uint32_t)docs.size();
    std::vector<uint64_t> offs((size_t)n_in + 1, 0);
    for (uint32_t d = 0; d < n_in; d++) offs[d + 1] = offs[d] + docs[d].text.size();
    std::string text;
    text.reserve(offs[n_in]);
    for (const auto& d : docs) text += d.text;
    st.n_docs_in = n_in; st.text_bytes = text.size();
    const auto t1 = clk::now();
    ns_forward* fwd = nullptr;
    int rc = ns_forward_build(ctx, (const uint8_t*)text.data(), text.size(), offs.data(), n_in, &fwd);
    if (rc != NS_OK) { err = std::string("ns_forward_build: ") + ns_last_error(ctx); return false; }
    ns_forward_info info{};
    info.struct_size = (uint32_t)sizeof(info);
    (void)ns_forward_get_info(fwd, &info);
    st.n_docs = info.kept_docs; st.n_terms = info.n_terms; st.tokens = info.n_tokens; st.kept_tokens = info.kept_tokens;
    st.pairs = info.n_pairs; st.device_ms = info.device_ms; st.device_bytes = info.device_bytes;
    if (info.kept_docs == 0) {
        ns_forward_destroy(fwd);
        err = "index_documents: no document has a token left after the length and stop-word rules";
        return false;
    }
    std::vector<uint32_t> kept(info.kept_docs), doc_len(info.kept_docs), counts(info.kept_docs), pairs((size_t)info.n_pairs * 2);
    std::vector<uint8_t> tbytes((size_t)info.term_bytes);
    std::vector<uint64_t> toff((size_t)info.n_terms + 1);
    rc = ns_forward_fetch(fwd, kept.data(), doc_len.data(), counts.data(), pairs.data(), tbytes.data(), toff.data());
    if (rc != NS_OK) err = std::string("ns_forward_fetch: ") + ns_last_error(ctx);
    ns_forward_destroy(fwd);
    if (rc != NS_OK) return false;
    st.call_s = std::chrono::duration<double>(clk::now() - t1).count();
    uint64_t total_len = 0;
    for (uint32_t v : doc_len) total_len += v;
    st.avgdl = (float)total_len / (float)info.kept_docs;            // :186
    try {
        std::error_code ec;
        fs::create_directories(segdir, ec);
        {
            FileOut out(segdir / "docs.bin");                          // :189-198
            out.u32(info.kept_docs);
            for (uint32_t j = 0; j < info.kept_docs; j++) {
                const DocInput& d = docs[kept[j]];
                out.str(d.cord_uid); out.str(d.title); out.str(d.json_relpath); out.u32(doc_len[j]);
            }
        }
        { FileOut out(segdir / "stats.bin"); out.u32(info.kept_docs); out.f32(st.avgdl); }   // :201-205
        {
            FileOut out(segdir / "forward.bin");                       // :208-219
            out.u32(info.kept_docs);
            size_t at = 0;
            for (uint32_t j = 0; j < info.kept_docs; j++) {
                out.u32(counts[j]);
                out.raw(pairs.data() + at, (size_t)counts[j] * 8);
                at += (size_t)counts[j] * 2;
            }
        }
        {
            FileOut out(segdir / "terms.bin");                         // :222-227
            out.u32(info.n_terms);
            for (uint32_t t = 0; t < info.n_terms; t++) {
                out.u32((uint32_t)(toff[t + 1] - toff[t]));
                out.raw(tbytes.data() + toff[t], (size_t)(toff[t + 1] - toff[t]));
            }
        }
    } catch (const std::exception& ex) { err = ex.what(); return false; }
    st.total_s = std::chrono::duration<double>(clk::now() - t0).count();
    return true;
}

}  // namespace nsx
