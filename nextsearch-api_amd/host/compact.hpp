// Compaction: several segments -> one, from the four forward files every segment carries (docs.bin,
// stats.bin, forward.bin, terms.bin).  The merge of the term lists, the remap and re-sort of the pairs (ns_forward_merge)
// and the inversion (ns_forward_invert) run on the device; this file reads, cross-checks and writes.  The reference has
// no such tool: its `adddocument` (src/AddDocument.cpp) writes one more segment per call for ever.
// With term ids numbered by ns_forward_build's rule the result is byte for byte the segment that ONE index_documents +
// invert_segment over the sources' documents writes.
#pragma once

#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "index_format.hpp"
#include "invert.hpp"
#include "nextsearch_hip.h"

namespace nsx {

struct CompactStats {
    uint32_t sources = 0, n_docs = 0, n_terms = 0;
    uint64_t terms_in = 0, pairs = 0, device_bytes = 0;
    float merge_ms = 0.0f, invert_ms = 0.0f;   // HIP events around the device parts of ns_forward_merge / ns_forward_invert
    double call_s = 0.0;                       // ns_forward_merge + fetch + ns_forward_invert, copies included
    double total_s = 0.0;                      // files in -> files out
};

struct SourceSegment {                 // one source's forward index as ns_forward_src wants it
    fs::path dir;
    std::vector<uint8_t> doc_records;  // docs.bin without its count: copied raw into the result
    std::vector<uint32_t> doc_len, counts, pairs;
    std::vector<uint8_t> term_bytes;
    std::vector<uint64_t> term_offsets;
};

// false + err (which names the file) for a missing, truncated or inconsistent file
inline bool load_source(const fs::path& dir, SourceSegment& s, std::string& err) {
    s = SourceSegment{};
    s.dir = dir;
    auto rd = [](const std::vector<uint8_t>& b, size_t at) { uint32_t v; std::memcpy(&v, b.data() + at, 4); return v; };
    auto bad = [&](const char* file, const char* what) { err = (dir / file).string() + ": " + what; return false; };
    FileBytes st, docs, fwd, terms;
    if (!st.load(dir / "stats.bin")) return bad("stats.bin", "missing or unreadable");
    if (!docs.load(dir / "docs.bin")) return bad("docs.bin", "missing or unreadable");
    if (!fwd.load(dir / "forward.bin")) return bad("forward.bin", "missing or unreadable");
    if (!terms.load(dir / "terms.bin")) return bad("terms.bin", "missing or unreadable");
    if (st.size() < 8) return bad("stats.bin", "truncated");
    const uint32_t n_docs = st.u32();
    {   // docs.bin: u32 n; n x {string uid, string title, string path, u32 doc_len}
        const std::vector<uint8_t>& b = docs.bytes();
        if (b.size() < 4) return bad("docs.bin", "truncated");
        if (rd(b, 0) != n_docs) return bad("docs.bin", "its document count differs from stats.bin's");
        if ((uint64_t)n_docs * 16 > b.size()) return bad("docs.bin", "truncated");
        s.doc_len.resize(n_docs);
        size_t pos = 4;
        for (uint32_t d = 0; d < n_docs; d++) {
            for (int k = 0; k < 3; k++) {
                if (pos + 4 > b.size()) return bad("docs.bin", "truncated");
                const uint32_t len = rd(b, pos);
                if ((uint64_t)pos + 4 + len > b.size()) return bad("docs.bin", "truncated");
                pos += 4 + (size_t)len;
            }
            if (pos + 4 > b.size()) return bad("docs.bin", "truncated");
            s.doc_len[d] = rd(b, pos);
            pos += 4;
        }
        s.doc_records.assign(b.begin() + 4, b.begin() + pos);
    }
    {   // forward.bin: u32 n; per document u32 cnt + cnt x {u32 termId, u32 tf}
        const std::vector<uint8_t>& b = fwd.bytes();
        if (b.size() < 4) return bad("forward.bin", "truncated");
        if (rd(b, 0) != n_docs) return bad("forward.bin", "its document count differs from stats.bin's");
        if ((uint64_t)n_docs * 4 > b.size()) return bad("forward.bin", "truncated");
        s.counts.resize(n_docs);
        s.pairs.reserve(b.size() / 4);
        size_t pos = 4;
        for (uint32_t d = 0; d < n_docs; d++) {
            if (pos + 4 > b.size()) return bad("forward.bin", "truncated");
            const uint32_t cnt = rd(b, pos);
            pos += 4;
            if ((uint64_t)pos + (uint64_t)cnt * 8 > b.size()) return bad("forward.bin", "truncated");
            s.counts[d] = cnt;
            const size_t at = s.pairs.size();
            s.pairs.resize(at + (size_t)cnt * 2);
            if (cnt) std::memcpy(s.pairs.data() + at, b.data() + pos, (size_t)cnt * 8);
            pos += (size_t)cnt * 8;
        }
    }
    {   // terms.bin: u32 n; n x string
        const std::vector<uint8_t>& b = terms.bytes();
        if (b.size() < 4) return bad("terms.bin", "truncated");
        const uint32_t n_terms = rd(b, 0);
        if ((uint64_t)n_terms * 4 > b.size()) return bad("terms.bin", "truncated");
        s.term_offsets.assign((size_t)n_terms + 1, 0);
        s.term_bytes.reserve(b.size());
        size_t pos = 4;
        for (uint32_t t = 0; t < n_terms; t++) {
            if (pos + 4 > b.size()) return bad("terms.bin", "truncated");
            const uint32_t len = rd(b, pos);
            pos += 4;
            if ((uint64_t)pos + len > b.size()) return bad("terms.bin", "truncated");
            s.term_bytes.insert(s.term_bytes.end(), b.begin() + pos, b.begin() + pos + len);
            pos += len;
            s.term_offsets[t + 1] = s.term_bytes.size();
        }
    }
    return true;
}

inline bool load_sources(const std::vector<fs::path>& dirs, std::vector<SourceSegment>& out, std::string& err) {
    out.clear();
    out.resize(dirs.size());
    for (size_t i = 0; i < dirs.size(); i++)
        if (!load_source(dirs[i], out[i], err)) { out.clear(); return false; }
    return true;
}

// What ns_forward_merge / ns_forward_merge_keep left on the device, on the host: the forward arrays and the inverted lists
struct MergedSegment {
    ns_forward_info info{};
    std::vector<uint32_t> doc_len, counts, pairs, df;
    std::vector<uint8_t> tbytes, postings;
    std::vector<uint64_t> toff;
};

// fetch + ns_forward_invert; fwd is destroyed in every case.  false + err (the C-ABI's message) on failure
inline bool fetch_merged(ns_ctx* ctx, ns_forward* fwd, MergedSegment& m, float& invert_ms, std::string& err) {
    const ns_forward_info& info = m.info;
    m.doc_len.resize(info.kept_docs); m.counts.resize(info.kept_docs); m.pairs.resize((size_t)info.n_pairs * 2); m.df.resize(info.n_terms);
    m.tbytes.resize((size_t)info.term_bytes); m.postings.resize((size_t)info.n_pairs * 8);
    m.toff.resize((size_t)info.n_terms + 1);
    uint64_t kept = 0;
    int rc = ns_forward_fetch(fwd, nullptr, m.doc_len.data(), m.counts.data(), m.pairs.data(), m.tbytes.data(), m.toff.data());
    if (rc == NS_OK) rc = ns_forward_invert(fwd, m.df.data(), m.postings.data(), &kept, &invert_ms);
    if (rc != NS_OK) err = ns_last_error(ctx);
    ns_forward_destroy(fwd);
    return rc == NS_OK;
}

// The complete segment out_seg from m: docs.bin = the count + the raw records in `records` back to back, stats.bin,
// forward.bin, terms.bin, barrels.bin and the barrel files.  A directory this call created is removed again when a file
// cannot be written.
inline bool write_merged(const fs::path& out_seg, const MergedSegment& m, const std::vector<std::pair<const uint8_t*, size_t>>& records, std::string& err) {
    const ns_forward_info& info = m.info;
    uint64_t total_len = 0;
    for (uint32_t v : m.doc_len) total_len += v;
    const float avgdl = (float)total_len / (float)info.kept_docs;       // src/ForwardIndex.cpp:186
    std::error_code ec;
    const bool existed = fs::exists(out_seg, ec);
    try {
        fs::create_directories(out_seg, ec);
        {
            FileOut out(out_seg / "docs.bin");
            out.u32(info.kept_docs);
            for (const auto& r : records) out.raw(r.first, r.second);
        }
        { FileOut out(out_seg / "stats.bin"); out.u32(info.kept_docs); out.f32(avgdl); }
        {
            FileOut out(out_seg / "forward.bin");
            out.u32(info.kept_docs);
            size_t at = 0;
            for (uint32_t j = 0; j < info.kept_docs; j++) {
                out.u32(m.counts[j]);
                out.raw(m.pairs.data() + at, (size_t)m.counts[j] * 8);
                at += (size_t)m.counts[j] * 2;
            }
        }
        {
            FileOut out(out_seg / "terms.bin");
            out.u32(info.n_terms);
            for (uint32_t t = 0; t < info.n_terms; t++) {
                out.u32((uint32_t)(m.toff[t + 1] - m.toff[t]));
                out.raw(m.tbytes.data() + m.toff[t], (size_t)(m.toff[t + 1] - m.toff[t]));
            }
        }
        write_barrels(out_seg, info.n_terms, m.df, m.postings,
                      [&](uint32_t t) { return std::string((const char*)m.tbytes.data() + m.toff[t], (size_t)(m.toff[t + 1] - m.toff[t])); });
    } catch (const std::exception& ex) {
        err = ex.what();
        if (!existed) fs::remove_all(out_seg, ec);
        return false;
    }
    return true;
}

inline void fill_forward_src(const SourceSegment& s, ns_forward_src& out) {
    out.n_docs = (uint32_t)s.doc_len.size(); out.doc_len = s.doc_len.data(); out.counts = s.counts.data();
    out.n_pairs = s.pairs.size() / 2; out.pairs = s.pairs.data();
    out.n_terms = (uint32_t)(s.term_offsets.size() - 1); out.term_bytes = s.term_bytes.data(); out.term_offsets = s.term_offsets.data();
}

// The loaded sources -> out_seg.  Nothing is written before the device work has succeeded; a directory this call created
// is removed again when a file cannot be written.
inline bool merge_loaded(ns_ctx* ctx, const std::vector<SourceSegment>& sources, const fs::path& out_seg, CompactStats& st, std::string& err) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    if (!ctx) { err = "merge_segments: no device context (compaction runs on the device; there is no CPU path)"; return false; }
    std::vector<ns_forward_src> src(sources.size());
    for (size_t i = 0; i < sources.size(); i++) {
        fill_forward_src(sources[i], src[i]);
        st.terms_in += src[i].n_terms;
    }
    st.sources = (uint32_t)sources.size();
    auto name_source = [&](std::string msg) {   // "source 3" of the C-ABI's message -> the segment's directory
        const std::string key = "source ";
        const size_t at = msg.find(key);
        if (at != std::string::npos) {
            const size_t i = (size_t)std::strtoul(msg.c_str() + at + key.size(), nullptr, 10);
            if (i < sources.size()) msg += " (" + sources[i].dir.string() + ")";
        }
        return msg;
    };
    ns_forward* fwd = nullptr;
    int rc = ns_forward_merge(ctx, src.data(), (uint32_t)src.size(), &fwd);
    if (rc != NS_OK) { err = name_source(ns_last_error(ctx)); return false; }
    MergedSegment m;
    m.info.struct_size = (uint32_t)sizeof(m.info);
    (void)ns_forward_get_info(fwd, &m.info);
    const ns_forward_info& info = m.info;
    st.n_docs = info.kept_docs; st.n_terms = info.n_terms; st.pairs = info.n_pairs; st.merge_ms = info.device_ms; st.device_bytes = info.device_bytes;
    if (info.kept_docs == 0) { ns_forward_destroy(fwd); err = "merge_segments: the sources hold no document"; return false; }
    if (!fetch_merged(ctx, fwd, m, st.invert_ms, err)) return false;
    st.call_s = std::chrono::duration<double>(clk::now() - t0).count();
    std::vector<std::pair<const uint8_t*, size_t>> records;
    for (const SourceSegment& s : sources) records.emplace_back(s.doc_records.data(), s.doc_records.size());
    if (!write_merged(out_seg, m, records, err)) return false;
    st.total_s = std::chrono::duration<double>(clk::now() - t0).count();
    return true;
}

inline bool merge_segments(ns_ctx* ctx, const std::vector<fs::path>& sources, const fs::path& out_seg, CompactStats& st, std::string& err) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    st = CompactStats{};
    std::vector<SourceSegment> loaded;
    if (!load_sources(sources, loaded, err)) return false;
    if (!merge_loaded(ctx, loaded, out_seg, st, err)) return false;
    st.total_s = std::chrono::duration<double>(clk::now() - t0).count();
    return true;
}

}  // namespace nsx
