#include "engine.hpp"
#include "invert.hpp"

#include <algorithm>
#include <chrono>
#include <memory>
#include <mutex>
#include <thread>
#include <cmath>
#include <limits>
#include <cstring>

#include "json_writer.hpp"
#include "textutil.hpp"

namespace nextsearch {

// the body of every failure: {"error": why}, dump(2) layout
static std::string error_body(const std::string& why) {
    std::string o = "{\n  \"error\": ";
    json_escape(o, why);
    o += "\n}";
    return o;
}

float bm25_idf(uint32_t N, uint32_t df) {
    // std::log((((N - df + 0.5f) / (df + 0.5f)) + 1.0f))   src/api_engine.cpp:45-47
    float num = (float)(uint32_t)(N - df) + 0.5f;
    float den = (float)df + 0.5f;
    return std::log((num / den) + 1.0f);   // float overload == glibc logf
}

Engine::Engine(int device) : device_(device) {}

Engine::Engine(const std::vector<int>& devices) : device_(devices.empty() ? 0 : devices[0]) {
    for (size_t i = 1; i < devices.size(); i++) { Replica r; r.device = devices[i]; replicas_.push_back(r); }
}

Engine::~Engine() {
    release_device_segments();
    if (ctx_) ns_ctx_destroy(ctx_);
    for (auto& r : replicas_) if (r.ctx) ns_ctx_destroy(r.ctx);   // frees the segments it holds
}

void Engine::release_similar() {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    for (SimilarSeg& s : similar_) if (s.dev) ns_docterms_destroy(s.dev);
    similar_.clear();
}

size_t Engine::similar_segments_on_device() const {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    size_t n = 0;
    for (const SimilarSeg& s : similar_) n += s.dev != nullptr;
    return n;
}

void Engine::release_device_segments() {
    release_similar();
    release_facets();
    release_sorted();
    release_boosts();
    release_collapse();
    close_all_filters();
    if (ctx_)
        for (ns_seg* s : dev_segs_)
            if (s) ns_segment_release(ctx_, s);
    dev_segs_.clear();
    if (ctx_ && sem.dev) ns_sem_release(ctx_, sem.dev);
    sem.dev = nullptr;
    if (ctx_ && ac_) ns_ac_release(ctx_, ac_);
    ac_ = nullptr;
    ac_fuzzy_ = false;
}

// One segment's postings to the device without a host copy: every inverted file is mapped, appended from the mapping
// (the C-ABI stages it through pinned memory) and unmapped again.  What the reference's open ifstreams are to it
// (src/api_segment.cpp:70-102) the device buffer is to this engine.
static bool upload_segment(ns_ctx* ctx, uint32_t seg_id, nsx::SegmentData& s, ns_seg** out, std::string& err) {
    if (s.doc_len.size() < s.N) s.doc_len.resize(s.N, 0);   // stats.bin N larger than docs.bin: treat missing as 0
    ns_seg* dev = nullptr;
    int rc = ns_segment_upload_begin(ctx, seg_id, s.N, s.avgdl, s.doc_len.data(), s.postings_bytes, &dev);
    if (rc != NS_OK) { err = std::string("ns_segment_upload: ") + ns_last_error(ctx); return false; }
    const bool fed = nsx::for_each_inverted_file(s, [&](const uint8_t* p, uint64_t n) {
        rc = ns_segment_upload_append(ctx, dev, p, n);
        return rc == NS_OK;
    });
    if (fed) rc = ns_segment_upload_end(ctx, dev);
    if (!fed || rc != NS_OK) {
        err = rc != NS_OK ? std::string("ns_segment_upload: ") + ns_last_error(ctx)
                          : "cannot map the inverted files of " + s.dir.string() + " (missing, or changed since they were listed)";
        (void)ns_segment_release(ctx, dev);
        return false;
    }
    // skip tables for the segment's frequent lists (ns_segment_build_skips: 4 B per list and 1024-doc cell).  The
    // reference's lists carry no block metadata (src/lexicon.cpp:104-128); this is built from the uploaded postings.
    // The tables are an accelerator, never a load precondition: the reference loads a segment with a damaged lexicon
    // record and only the queries naming that term go wrong (src/api_engine.cpp:464-476), so records that do not
    // describe a whole list inside the payload are left out here, and a refusal of the rest costs the tables, not the
    // segment (queries then take the cursor path; a term ref of a damaged record is rejected at prepare, as before).
    {
        const uint32_t min_count = std::max<uint32_t>(64u, s.N / 512u);
        std::vector<uint64_t> off;
        std::vector<uint32_t> cnt;
        for (const auto& kv : s.lex) {
            const nsx::LexEntry& e = kv.second;
            if (e.df == 0 || e.count < min_count) continue;
            if (s.use_barrels && e.barrelId >= s.barrel_base.size()) continue;
            const uint64_t bo = s.list_byte_offset(e);
            if (bo % 8 != 0 || bo / 8 + e.count > s.postings_bytes / 8) continue;
            off.push_back(bo);
            cnt.push_back(e.count);
        }
        if (!off.empty()) (void)ns_segment_build_skips(ctx, dev, off.data(), cnt.data(), (uint32_t)off.size());
    }
    *out = dev;
    return true;
}

// reload (src/api_engine.cpp:50-160).  Like the reference, the new state replaces the old one only after EVERYTHING
// loaded (:76-90): segments, metadata and embeddings are built aside, the device copy goes into a FRESH context, and
// only then are the old context and the old host state dropped.  A failed reload leaves the engine serving what it
// served before.  (Old and new device copies coexist during the swap: 2 x index size of HBM, against 288 GB.)
bool Engine::reload() {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    err_.clear();
    // manifest, else scan segments/seg_* sorted (src/api_engine.cpp:57-73)
    std::vector<std::string> names = nsx::load_manifest(index_dir / "manifest.bin");
    if (names.empty()) {
        nsx::fs::path segroot = index_dir / "segments";
        std::error_code ec;
        if (nsx::fs::is_directory(segroot, ec)) {
            for (auto it = nsx::fs::directory_iterator(segroot, ec); !ec && it != nsx::fs::directory_iterator(); it.increment(ec)) {
                if (!it->is_directory(ec)) continue;
                auto name = it->path().filename().string();
                if (name.rfind("seg_", 0) == 0) names.push_back(name);
            }
            std::sort(names.begin(), names.end());
        }
    }
    if (names.empty()) { err_ = "no segments found under " + index_dir.string(); return false; }

    std::vector<nsx::SegmentData> loaded(names.size());
    for (size_t i = 0; i < names.size(); i++) {
        nsx::fs::path segdir = index_dir / "segments" / names[i];
        if (!nsx::load_segment(segdir, loaded[i])) { err_ = "failed to load segment: " + segdir.string(); return false; }
    }
    // metadata mapping (src/api_engine.cpp:110-113): absent file = no decoration, not an error
    nsx::MetadataTable fresh_meta;
    fresh_meta.load(index_dir / "metadata.csv", loaded);
    // embeddings (src/api_engine.cpp:115-153): only the terms some lexicon holds; absent or unusable file = no expansion
    nsx::SemanticTable fresh_sem;
    {
        nsx::fs::path emb;
        if (const char* p = std::getenv("EMBEDDINGS_PATH")) {
            emb = nsx::fs::path(p);
        } else {
            for (const char* c : {"embeddings.vec", "embeddings.txt", "glove.txt", "vectors.txt"})
                if (nsx::fs::exists(index_dir / c)) { emb = index_dir / c; break; }
        }
        if (!emb.empty() && nsx::fs::exists(emb)) {
            std::unordered_set<std::string> needed;
            needed.reserve(250000);
            for (const auto& seg : loaded)
                for (const auto& kv : seg.lex) needed.insert(kv.first);
            fresh_sem.load_from_text(emb, needed);
        }
    }

    // autocomplete's table (src/api_engine.cpp:91-107), sorted on the engine's host threads
    nsx::SuggestTable fresh_table;
    const auto t_build = std::chrono::steady_clock::now();
    if (!pool_) pool_.reset(new ForkJoin(std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u)));
    fresh_table.build(loaded, pool_.get());
    const double build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build).count();
    double upload_ms = 0.0;

    ns_ctx* fresh_ctx = nullptr;
    ns_ac* fresh_ac = nullptr;
    std::vector<ns_seg*> fresh_segs;
    std::vector<Replica> fresh_replicas;
    if (device_ >= 0) {
        int rc = ns_ctx_create(device_, &fresh_ctx);
        if (rc != NS_OK) { err_ = std::string("ns_ctx_create: ") + ns_last_error(nullptr); return false; }
        // upload hook: once per segment, after load_segment (src/api_engine.cpp:90)
        fresh_segs.assign(loaded.size(), nullptr);
        bool ok = true;
        for (size_t i = 0; i < loaded.size() && ok; i++) ok = upload_segment(fresh_ctx, (uint32_t)i, loaded[i], &fresh_segs[i], err_);
        if (ok) {   // autocomplete on the primary context only
            const auto t_up = std::chrono::steady_clock::now();
            rc = ns_ac_upload(fresh_ctx, (const uint8_t*)fresh_table.pool.data(), fresh_table.off.data(), fresh_table.score.data(),
                              (uint32_t)fresh_table.size(), &fresh_ac);
            if (rc != NS_OK) { err_ = std::string("ns_ac_upload: ") + ns_last_error(fresh_ctx); ok = false; }
            upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up).count();
        }
        if (ok && fresh_sem.enabled) {
            rc = ns_sem_upload(fresh_ctx, fresh_sem.vecs.data(), (uint32_t)fresh_sem.terms.size(), (uint32_t)fresh_sem.dim, &fresh_sem.dev);
            if (rc != NS_OK) { err_ = std::string("ns_sem_upload: ") + ns_last_error(fresh_ctx); ok = false; }
        }
        // the replicas of a multi-device engine: the same upload into a fresh context on each further device
        for (size_t r = 0; r < replicas_.size() && ok; r++) {
            Replica fr;
            fr.device = replicas_[r].device;
            rc = ns_ctx_create(fr.device, &fr.ctx);
            if (rc != NS_OK) { err_ = std::string("ns_ctx_create (device ") + std::to_string(fr.device) + "): " + ns_last_error(nullptr); ok = false; break; }
            fr.segs.assign(loaded.size(), nullptr);
            for (size_t i = 0; i < loaded.size() && ok; i++) ok = upload_segment(fr.ctx, (uint32_t)i, loaded[i], &fr.segs[i], err_);
            fresh_replicas.push_back(fr);
        }
        if (!ok) {   // the engine keeps serving the previous index
            ns_ctx_destroy(fresh_ctx);   // frees the segments it holds
            for (auto& fr : fresh_replicas) if (fr.ctx) ns_ctx_destroy(fr.ctx);
            return false;
        }
    }
    // ---- commit ----
    release_device_segments();
    if (ctx_) ns_ctx_destroy(ctx_);
    ctx_ = fresh_ctx;
    ac_ = fresh_ac;
    dev_segs_ = std::move(fresh_segs);
    if (device_ >= 0) {
        for (auto& r : replicas_) if (r.ctx) ns_ctx_destroy(r.ctx);
        replicas_ = std::move(fresh_replicas);
    }
    seg_names = std::move(names);
    segments = std::move(loaded);
    meta = std::move(fresh_meta);
    sem = std::move(fresh_sem);
    suggest_table = std::move(fresh_table);
    suggest_build_ms = build_ms;
    suggest_upload_ms = upload_ms;
    correct_build_ms = 0.0;
    dict.build(segments, [](uint32_t N, uint32_t df) { return bm25_idf(N, df); });
    cache_.clear();
    lru_.clear();
    raw_postings_.clear();
    // warm-up: the first requests after a reload otherwise pay for loading the kernels' code objects and for the
    // pinned staging buffers (~60 ms spread over the first few hundred requests).  One lone query over the longest
    // list of the first segment takes the same route (k_pull, k_uscore, k_merge_wide) once, here.
    const char* wu = std::getenv("NS_RELOAD_WARMUP");   // "0": skip (bench.py does, so that a profile of it holds the timed launches only)
    if (ctx_ && !segments.empty() && !(wu && wu[0] == '0')) {
        const nsx::LexEntry* best = nullptr;
        for (const auto& kv : segments[0].lex)
            if (kv.second.df && (!best || kv.second.count > best->count)) best = &kv.second;
        if (best) {
            ns_term_ref r;
            r.seg_id = 0; r.count = best->count; r.byte_off = segments[0].list_byte_offset(*best);
            r.idf = bm25_idf(segments[0].N, best->df); r.qweight = 1.0f;
            ns_query_desc qd{0, 1};
            ns_hit hits[10]; uint32_t nh = 0; uint64_t fd = 0;
            (void)ns_search_batch(ctx_, &qd, &r, 1, 10, hits, &nh, &fd, NS_FLAG_OR);
        }
    }
    return true;
}

bool Engine::add_documents(const std::vector<nsx::DocInput>& docs, nsx::IndexStats* stats) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    err_.clear();
    if (device_ < 0) { err_ = "add_documents: host-only engine (indexing runs on the device; there is no CPU path)"; return false; }
    // an engine that has not loaded anything yet has no context: a context of its own for the two device steps
    ns_ctx* ctx = ctx_;
    ns_ctx* own = nullptr;
    if (!ctx) {
        if (ns_ctx_create(device_, &own) != NS_OK) { err_ = std::string("ns_ctx_create: ") + ns_last_error(nullptr); return false; }
        ctx = own;
    }
    const nsx::fs::path manifest = index_dir / "manifest.bin", segroot = index_dir / "segments";
    std::error_code ec;
    std::vector<std::string> segs = nsx::load_manifest(manifest);                  // src/AddDocument.cpp:54
    uint32_t id = (uint32_t)segs.size();
    while (nsx::fs::exists(segroot / nsx::seg_name(id), ec) || std::find(segs.begin(), segs.end(), nsx::seg_name(id)) != segs.end()) id++;
    const std::string name = nsx::seg_name(id);
    const nsx::fs::path segdir = segroot / name;
    nsx::IndexStats st;
    bool ok = nsx::index_documents(ctx, docs, segdir, st, err_);                    // (creates segdir only when a document survives)
    if (ok) {
        nsx::InvertStats ist;
        ok = nsx::invert_segment(ctx, segdir, ist, err_);
    }
    if (own) ns_ctx_destroy(own);
    if (stats) *stats = st;
    bool had_manifest = false;
    std::vector<uint8_t> old_manifest;
    if (ok) {
        nsx::FileBytes fb;
        had_manifest = nsx::fs::exists(manifest, ec) && fb.load(manifest);
        if (had_manifest) old_manifest = fb.bytes();
        try {
            segs.push_back(name);
            nsx::save_manifest(manifest, segs);                                     // src/AddDocument.cpp:168-169
        } catch (const std::exception& ex) { err_ = ex.what(); ok = false; }
        if (ok && !reload()) ok = false;                                            // (err_ is reload's)
        if (!ok) {   // the manifest as it was
            const std::string keep = err_;
            if (had_manifest) { try { nsx::FileOut out(manifest); out.raw(old_manifest.data(), old_manifest.size()); } catch (...) {} }
            else nsx::fs::remove(manifest, ec);
            err_ = keep;
        }
    }
    if (!ok) nsx::fs::remove_all(segdir, ec);
    return ok;
}

bool Engine::compact(size_t first, size_t count, bool remove_sources, nsx::CompactStats* stats) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    err_.clear();
    if (stats) *stats = nsx::CompactStats{};
    if (device_ < 0) { err_ = "compact: host-only engine (compaction runs on the device; there is no CPU path)"; return false; }
    const nsx::fs::path manifest = index_dir / "manifest.bin", segroot = index_dir / "segments";
    std::error_code ec;
    std::vector<std::string> segs = nsx::load_manifest(manifest);
    first = std::min(first, segs.size());
    count = std::min(count, segs.size() - first);
    if (count < 2) return true;                                                     // nothing to merge
    std::vector<nsx::fs::path> sources;
    for (size_t i = first; i < first + count; i++) sources.push_back(segroot / segs[i]);
    std::vector<nsx::SourceSegment> loaded;
    if (!nsx::load_sources(sources, loaded, err_)) { err_ = "compact: " + err_; return false; }
    ns_ctx* ctx = ctx_;
    ns_ctx* own = nullptr;
    if (!ctx) {
        if (ns_ctx_create(device_, &own) != NS_OK) { err_ = std::string("ns_ctx_create: ") + ns_last_error(nullptr); return false; }
        ctx = own;
    }
    uint32_t id = (uint32_t)segs.size();                                            // the next free name, as add_documents finds it
    while (nsx::fs::exists(segroot / nsx::seg_name(id), ec) || std::find(segs.begin(), segs.end(), nsx::seg_name(id)) != segs.end()) id++;
    const std::string name = nsx::seg_name(id);
    const nsx::fs::path segdir = segroot / name;
    nsx::CompactStats st;
    const auto t0 = std::chrono::steady_clock::now();
    bool ok = nsx::merge_loaded(ctx, loaded, segdir, st, err_);
    if (!ok) err_ = "compact: " + err_;
    loaded.clear();
    if (own) ns_ctx_destroy(own);
    std::vector<std::string> fresh(segs.begin(), segs.begin() + first);
    fresh.push_back(name);
    fresh.insert(fresh.end(), segs.begin() + first + count, segs.end());
    if (ok) {
        nsx::FileBytes fb;
        const bool had_manifest = nsx::fs::exists(manifest, ec) && fb.load(manifest);
        const std::vector<uint8_t> old_manifest = had_manifest ? fb.bytes() : std::vector<uint8_t>();
        try {
            nsx::save_manifest(manifest, fresh);
        } catch (const std::exception& ex) { err_ = ex.what(); ok = false; }
        if (ok && !reload()) ok = false;                                            // (err_ is reload's)
        if (!ok) {   // the manifest as it was
            const std::string keep = err_;
            if (had_manifest) { try { nsx::FileOut out(manifest); out.raw(old_manifest.data(), old_manifest.size()); } catch (...) {} }
            else nsx::fs::remove(manifest, ec);
            err_ = keep;
        }
    }
    if (!ok) { nsx::fs::remove_all(segdir, ec); return false; }
    if (remove_sources) {
        for (size_t i = first; i < first + count; i++) {
            if (std::find(fresh.begin(), fresh.end(), segs[i]) != fresh.end()) continue;   // still named by the manifest
            std::error_code rec;
            nsx::fs::remove_all(segroot / segs[i], rec);
            if (rec) err_ += (err_.empty() ? "compact: could not remove " : "; ") + (segroot / segs[i]).string() + ": " + rec.message();
        }
    }
    st.total_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    return true;
}

bool Engine::find_documents(const std::vector<std::string>& uids, std::vector<std::pair<uint32_t, uint32_t>>& out) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    out.clear();
    const std::unordered_set<std::string> wanted(uids.begin(), uids.end());
    if (wanted.empty()) return true;
    for (size_t i = 0; i < segments.size(); i++)
        for (size_t d = 0; d < segments[i].cord_uid.size(); d++)
            if (wanted.count(segments[i].cord_uid[d])) out.emplace_back((uint32_t)i, (uint32_t)d);
    return true;
}

bool Engine::delete_documents(const std::vector<std::string>& uids, nsx::DeleteStats* stats) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    err_.clear();
    if (stats) *stats = nsx::DeleteStats{};
    if (device_ < 0) { err_ = "delete_documents: host-only engine (deleting runs on the device; there is no CPU path)"; return false; }
    std::vector<std::pair<uint32_t, uint32_t>> hits;
    find_documents(uids, hits);
    std::unordered_set<std::string> missing(uids.begin(), uids.end());
    for (const auto& h : hits) missing.erase(segments[h.first].cord_uid[h.second]);
    nsx::DeleteStats st;
    const bool ok = delete_by_id(hits, &st);
    st.uids_not_found = (uint32_t)missing.size();
    if (stats) *stats = st;
    return ok;
}

bool Engine::delete_by_id(const std::vector<std::pair<uint32_t, uint32_t>>& seg_doc, nsx::DeleteStats* stats) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    const auto t0 = std::chrono::steady_clock::now();
    err_.clear();
    if (stats) *stats = nsx::DeleteStats{};
    if (device_ < 0) { err_ = "delete_documents: host-only engine (deleting runs on the device; there is no CPU path)"; return false; }
    // ---- which documents stay, per touched segment (one bit per document; nothing is touched before this is complete) ----
    std::vector<std::vector<uint32_t>> keep(segments.size());
    std::vector<uint32_t> gone(segments.size(), 0);
    nsx::DeleteStats st;
    for (const auto& sd : seg_doc) {
        if (sd.first >= segments.size() || sd.second >= segments[sd.first].cord_uid.size()) {
            err_ = "delete_documents: (segment " + std::to_string(sd.first) + ", document " + std::to_string(sd.second) + ") is not in the index";
            return false;
        }
        std::vector<uint32_t>& bits = keep[sd.first];
        if (bits.empty()) bits.assign((segments[sd.first].cord_uid.size() + 31) / 32, 0xFFFFFFFFu);
        uint32_t& w = bits[sd.second >> 5];
        const uint32_t b = 1u << (sd.second & 31u);
        if (w & b) { w &= ~b; gone[sd.first]++; st.docs_deleted++; }
    }
    if (st.docs_deleted == 0) return true;                                          // nothing matches: nothing touched
    uint64_t left = 0;
    for (size_t i = 0; i < segments.size(); i++) left += segments[i].cord_uid.size() - gone[i];
    if (left == 0) { err_ = "delete_documents: the call would delete every document of the index (an index without a segment cannot be loaded)"; return false; }
    const nsx::fs::path manifest = index_dir / "manifest.bin", segroot = index_dir / "segments";
    std::error_code ec;
    std::vector<std::string> segs = nsx::load_manifest(manifest);
    if (segs.empty()) segs = seg_names;                                             // (an index without a manifest: the sorted scan reload() made)
    if (segs != seg_names) { err_ = "delete_documents: manifest.bin names other segments than the engine serves (reload first)"; return false; }
    ns_ctx* ctx = ctx_;
    ns_ctx* own = nullptr;
    if (!ctx) {
        if (ns_ctx_create(device_, &own) != NS_OK) { err_ = std::string("ns_ctx_create: ") + ns_last_error(nullptr); return false; }
        ctx = own;
    }
    // ---- every affected segment with a survivor, rewritten on its own into the next free name ----
    std::vector<std::string> fresh, made, old;
    bool ok = true;
    uint32_t id = (uint32_t)segs.size();
    for (size_t i = 0; i < segs.size() && ok; i++) {
        if (!gone[i]) { fresh.push_back(segs[i]); continue; }
        old.push_back(segs[i]);
        if (gone[i] == segments[i].cord_uid.size()) { st.segments_dropped++; continue; }
        nsx::SourceSegment src;
        ok = nsx::load_source(segroot / segs[i], src, err_);
        if (ok && src.doc_len.size() != segments[i].cord_uid.size()) { err_ = (segroot / segs[i]).string() + ": its document count differs from the loaded segment's"; ok = false; }
        if (!ok) break;
        while (nsx::fs::exists(segroot / nsx::seg_name(id), ec) || std::find(segs.begin(), segs.end(), nsx::seg_name(id)) != segs.end()) id++;
        const std::string name = nsx::seg_name(id++);
        made.push_back(name);                                                       // (removed again below if anything fails)
        ok = nsx::rewrite_loaded(ctx, src, keep[i], segroot / name, st, err_);
        if (ok) { fresh.push_back(name); st.segments_rewritten++; }
    }
    if (own) ns_ctx_destroy(own);
    if (!ok) err_ = "delete_documents: " + err_;
    if (ok) {
        nsx::FileBytes fb;
        const bool had_manifest = nsx::fs::exists(manifest, ec) && fb.load(manifest);
        const std::vector<uint8_t> old_manifest = had_manifest ? fb.bytes() : std::vector<uint8_t>();
        try {
            nsx::save_manifest(manifest, fresh);
        } catch (const std::exception& ex) { err_ = ex.what(); ok = false; }
        if (ok && !reload()) ok = false;                                            // (err_ is reload's)
        if (!ok) {   // the manifest as it was
            const std::string why = err_;
            if (had_manifest) { try { nsx::FileOut out(manifest); out.raw(old_manifest.data(), old_manifest.size()); } catch (...) {} }
            else nsx::fs::remove(manifest, ec);
            err_ = why;
        }
    }
    if (!ok) {
        for (const std::string& name : made) nsx::fs::remove_all(segroot / name, ec);
        return false;
    }
    for (const std::string& name : old) {
        std::error_code rec;
        nsx::fs::remove_all(segroot / name, rec);
        if (rec) err_ += (err_.empty() ? "delete_documents: could not remove " : "; ") + (segroot / name).string() + ": " + rec.message();
    }
    st.total_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    return true;
}

const std::vector<uint8_t>* Engine::raw_postings(uint32_t seg) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (seg >= segments.size()) return nullptr;
    if (raw_postings_.size() < segments.size()) raw_postings_.resize(segments.size());
    auto& slot = raw_postings_[seg];
    if (!slot) {
        slot = std::make_unique<std::vector<uint8_t>>();
        if (!nsx::read_postings(segments[seg], *slot)) { slot.reset(); err_ = "cannot read the inverted files of " + segments[seg].dir.string(); return nullptr; }
    }
    return slot.get();
}

bool Engine::build_impacts() {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { err_ = "no device context"; return false; }
    for (size_t sid = 0; sid < segments.size(); sid++) {
        const auto& seg = segments[sid];
        std::vector<uint64_t> off;
        std::vector<uint32_t> cnt;
        std::vector<float> idf;
        off.reserve(seg.lex.size()); cnt.reserve(seg.lex.size()); idf.reserve(seg.lex.size());
        for (const auto& kv : seg.lex) {
            const nsx::LexEntry& e = kv.second;
            if (e.df == 0 || e.count == 0) continue;   // never scored (src/api_engine.cpp:458)
            off.push_back(seg.list_byte_offset(e));
            cnt.push_back(e.count);
            idf.push_back(bm25_idf(seg.N, e.df));   // the idf build_refs_range hands to the device for this list
        }
        int rc = ns_segment_build_impacts(ctx_, dev_segs_[sid], off.data(), cnt.data(), idf.data(), (uint32_t)off.size());
        if (rc != NS_OK) { err_ = std::string("ns_segment_build_impacts: ") + ns_last_error(ctx_); return false; }
        for (auto& r : replicas_) {
            rc = ns_segment_build_impacts(r.ctx, r.segs[sid], off.data(), cnt.data(), idf.data(), (uint32_t)off.size());
            if (rc != NS_OK) { err_ = std::string("ns_segment_build_impacts: ") + ns_last_error(r.ctx); return false; }
        }
    }
    return true;
}

// Optional: the compressed, blocked posting stream of every segment (ns_segment_build_packed).
bool Engine::build_packed() {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { err_ = "no device context"; return false; }
    for (size_t sid = 0; sid < dev_segs_.size(); sid++) {
        int rc = ns_segment_build_packed(ctx_, dev_segs_[sid]);
        if (rc != NS_OK) { err_ = std::string("ns_segment_build_packed: ") + ns_last_error(ctx_); return false; }
        for (auto& r : replicas_) {
            rc = ns_segment_build_packed(r.ctx, r.segs[sid]);
            if (rc != NS_OK) { err_ = std::string("ns_segment_build_packed: ") + ns_last_error(r.ctx); return false; }
        }
    }
    return true;
}

// Optional: block maxima of every list long enough for pruning to pay (ns_segment_build_blockmax).
bool Engine::build_blockmax() {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { err_ = "no device context"; return false; }
    for (size_t sid = 0; sid < segments.size(); sid++) {
        const auto& seg = segments[sid];
        std::vector<uint64_t> off;
        std::vector<uint32_t> cnt;
        std::vector<float> idf;
        for (const auto& kv : seg.lex) {
            const nsx::LexEntry& e = kv.second;
            if (e.df == 0 || e.count < 512) continue;
            if (seg.use_barrels && e.barrelId >= seg.barrel_base.size()) continue;
            const uint64_t bo = seg.list_byte_offset(e);
            if (bo % 8 != 0 || bo / 8 + e.count > seg.postings_bytes / 8) continue;   // a damaged record: never scored either
            off.push_back(bo);
            cnt.push_back(e.count);
            idf.push_back(bm25_idf(seg.N, e.df));   // the idf build_refs hands to the device for this list
        }
        int rc = ns_segment_build_blockmax(ctx_, dev_segs_[sid], off.data(), cnt.data(), idf.data(), (uint32_t)off.size());
        if (rc != NS_OK) { err_ = std::string("ns_segment_build_blockmax: ") + ns_last_error(ctx_); return false; }
        for (auto& r : replicas_) {
            rc = ns_segment_build_blockmax(r.ctx, r.segs[sid], off.data(), cnt.data(), idf.data(), (uint32_t)off.size());
            if (rc != NS_OK) { err_ = std::string("ns_segment_build_blockmax: ") + ns_last_error(r.ctx); return false; }
        }
    }
    return true;
}

void Engine::use_pruning(bool on) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (ctx_) ns_ctx_use_pruning(ctx_, on ? 1 : 0);
    for (auto& r : replicas_) ns_ctx_use_pruning(r.ctx, on ? 1 : 0);
}

void Engine::use_merge(bool on) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (ctx_) ns_ctx_use_merge(ctx_, on ? 1 : 0);
    for (auto& r : replicas_) ns_ctx_use_merge(r.ctx, on ? 1 : 0);
}

void Engine::share_scores(int mode) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (ctx_) ns_ctx_share_scores(ctx_, mode);
    for (auto& r : replicas_) ns_ctx_share_scores(r.ctx, mode);
}

void Engine::use_packed(int mode) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (ctx_) ns_ctx_use_packed(ctx_, mode);
    for (auto& r : replicas_) ns_ctx_use_packed(r.ctx, mode);
}

void Engine::use_skips(bool on) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (ctx_) ns_ctx_use_skips(ctx_, on ? 1 : 0);
    for (auto& r : replicas_) ns_ctx_use_skips(r.ctx, on ? 1 : 0);
}

void Engine::use_impacts(bool on) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (ctx_) ns_ctx_use_impacts(ctx_, on ? 1 : 0);
    for (auto& r : replicas_) ns_ctx_use_impacts(r.ctx, on ? 1 : 0);
}

// Query preparation (tokenise, stop-words, lexicon probes, idf: src/api_engine.cpp:388-397,:454-461) for
// queries [q0, q1) with GIVEN weighted terms (semantic expansion): `refs` receives the term refs of those queries,
// qd[q].term_begin is relative to it.  Terms are probed in the dictionary, once per term for all segments.
void Engine::build_refs_range(const std::vector<std::string>& queries, size_t q0, size_t q1, std::vector<ns_query_desc>& qd,
                              std::vector<ns_term_ref>& refs, std::vector<uint8_t>& usable,
                              const std::vector<nsx::WeightedTerms>* expanded, const nsx::RowSource& rs, bool and_mode) const {
    const uint32_t S = (uint32_t)segments.size();
    std::vector<int64_t> gid;
    for (size_t q = q0; q < q1; q++) {
        nsx::WeightedTerms own;
        if (!expanded)   // weights: 1.0f per base term (src/api_engine.cpp:419-421)
            for (auto& t : base_terms(queries[q])) own.emplace_back(std::move(t), 1.0f);
        const nsx::WeightedTerms& terms = expanded ? (*expanded)[q] : own;
        qd[q].term_begin = (uint32_t)refs.size();
        if (terms.empty() || segments.empty()) continue;   // src/api_engine.cpp:407, :424
        usable[q] = 1;
        gid.clear();
        for (const auto& tw : terms) gid.push_back(dict.find(tw.first.data(), tw.first.size()));
        for (uint32_t sid = 0; sid < segments.size(); sid++) {
            if (rs.rows && and_mode) {   // a list of the group lost all its postings: no kept document of the segment matches
                bool dead = false;
                for (size_t ti = 0; ti < terms.size() && !dead; ti++)
                    dead = gid[ti] >= 0 && dict.row((uint32_t)gid[ti])[sid].byte_off != nsx::kAbsent &&
                           rs.rows[(size_t)gid[ti] * S + sid].byte_off == nsx::kAbsent;
                if (dead) continue;
            }
            for (size_t ti = 0; ti < terms.size(); ti++) {
                if (gid[ti] < 0) continue;                    // :455
                const nsx::TermSeg& e = rs.rows ? rs.rows[(size_t)gid[ti] * S + sid] : dict.row((uint32_t)gid[ti])[sid];
                if (e.byte_off == nsx::kAbsent) continue;     // :455 / :458
                ns_term_ref r;
                r.seg_id = rs.id_base + sid;
                r.count = e.count;
                r.byte_off = e.byte_off;
                r.idf = e.idf;
                r.qweight = terms[ti].second;
                refs.push_back(r);
            }
        }
        qd[q].term_count = (uint32_t)refs.size() - qd[q].term_begin;
    }
}

// The same for plain base terms (weight 1.0f, src/api_engine.cpp:419-421) straight from the query bytes: no std::string
// per token, one dictionary probe per term, the per-segment numbers read from the term's row.
void Engine::build_refs_views(const QueryView* queries, size_t q0, size_t q1, ns_query_desc* qd, std::vector<ns_term_ref>& refs,
                              uint8_t* usable, std::vector<char>& scratch, std::vector<uint32_t>& gids, const nsx::RowSource& rs,
                              bool and_mode) const {
    const uint32_t S = (uint32_t)segments.size();
    for (size_t q = q0; q < q1; q++) {
        ns_query_desc& d = qd[q - q0];
        d.term_begin = (uint32_t)refs.size();
        d.term_count = 0;
        gids.clear();
        size_t n_terms = 0;
        nsx::for_each_base_term(queries[q].p, queries[q].n, scratch, [&](const char* p, size_t n) {
            n_terms++;
            const int64_t g = dict.find(p, n);
            if (g >= 0) gids.push_back((uint32_t)g);
        });
        usable[q - q0] = (n_terms != 0 && S != 0) ? 1 : 0;   // src/api_engine.cpp:407: no base terms (or no segments) -> early return
        if (!usable[q - q0]) continue;
        for (uint32_t sid = 0; sid < S; sid++) {
            if (rs.rows && and_mode) {   // a list of the group lost all its postings: no kept document of the segment matches
                bool dead = false;
                for (const uint32_t g : gids)
                    if (dict.row(g)[sid].byte_off != nsx::kAbsent && rs.rows[(size_t)g * S + sid].byte_off == nsx::kAbsent) { dead = true; break; }
                if (dead) continue;
            }
            for (const uint32_t g : gids) {
                const nsx::TermSeg& e = rs.rows ? rs.rows[(size_t)g * S + sid] : dict.row(g)[sid];
                if (e.byte_off == nsx::kAbsent) continue;
                refs.push_back(ns_term_ref{rs.id_base + sid, e.count, e.byte_off, e.idf, 1.0f});
            }
        }
        d.term_count = (uint32_t)refs.size() - d.term_begin;
    }
}

unsigned Engine::prep_width(size_t Q) const {
    unsigned nt = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
    return (unsigned)std::max<size_t>(1, std::min<size_t>(nt, Q / 256));   // below ~256 queries per thread the hand-over costs more than it saves
}

// queries [q0, q1) on the engine's host threads (contiguous slices; the dictionary is read-only), the slices' term refs
// concatenated in query order.  qd / usable are indexed from q0.
void Engine::build_refs_parallel(const QueryView* queries, size_t q0, size_t q1, std::vector<ns_query_desc>& qd,
                                 std::vector<ns_term_ref>& refs, uint8_t* usable, const nsx::RowSource& rs, bool and_mode) const {
    const size_t Q = q1 - q0;
    qd.resize(Q);
    refs.clear();
    const unsigned nt = prep_width(Q);
    if (scratch_.size() < nt) scratch_.resize(nt);
    if (nt <= 1) {
        build_refs_views(queries, q0, q1, qd.data(), refs, usable, scratch_[0].text, scratch_[0].gids, rs, and_mode);
        return;
    }
    if (!pool_ || pool_->width() < nt) pool_.reset(new ForkJoin(std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u)));
    pool_->run(nt, [&](unsigned i) {
        PrepScratch& sc = scratch_[i];
        sc.refs.clear();
        const size_t a = q0 + Q * i / nt, b = q0 + Q * (i + 1) / nt;
        build_refs_views(queries, a, b, qd.data() + (a - q0), sc.refs, usable + (a - q0), sc.text, sc.gids, rs, and_mode);
    });
    size_t total = 0;
    std::vector<size_t> base(nt);
    for (unsigned i = 0; i < nt; i++) { base[i] = total; total += scratch_[i].refs.size(); }
    refs.resize(total);
    pool_->run(nt, [&](unsigned i) {
        const size_t a = Q * i / nt, b = Q * (i + 1) / nt;
        for (size_t q = a; q < b; q++) qd[q].term_begin += (uint32_t)base[i];
        if (!scratch_[i].refs.empty()) std::memcpy(refs.data() + base[i], scratch_[i].refs.data(), scratch_[i].refs.size() * sizeof(ns_term_ref));
    });
}

// A batch is Q independent searches: large batches are prepared by several host
// threads, each on a contiguous slice of the queries (the lexicons are read-only), and the slices'
// term refs are concatenated in query order.
void Engine::build_refs(const std::vector<std::string>& queries, std::vector<ns_query_desc>& qd,
                        std::vector<ns_term_ref>& refs, std::vector<uint8_t>& usable) const {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    const size_t Q = queries.size();
    qd.assign(Q, ns_query_desc{0, 0});
    usable.assign(Q, 0);
    refs.clear();
    refs_failed_ = false;
    if (sem.enabled) {   // src/api_engine.cpp:409-417: one device call per top-k size for the whole batch
        std::vector<nsx::WeightedTerms> expanded;
        if (!expand_queries(queries, expanded)) { refs_failed_ = true; return; }
        build_refs_range(queries, 0, Q, qd, refs, usable, &expanded);
        return;
    }
    std::vector<QueryView> views(Q);
    for (size_t q = 0; q < Q; q++) views[q] = QueryView{queries[q].data(), queries[q].size()};
    build_refs_parallel(views.data(), 0, Q, qd, refs, usable.data());
}

bool Engine::expand_queries(const std::vector<std::string>& queries, std::vector<nsx::WeightedTerms>& out) const {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    std::vector<std::vector<std::string>> qt(queries.size());
    for (size_t q = 0; q < queries.size(); q++) qt[q] = base_terms(queries[q]);
    if (!sem.enabled) {
        out.assign(queries.size(), {});
        for (size_t q = 0; q < queries.size(); q++)
            for (auto& t : qt[q]) out[q].emplace_back(t, 1.0f);
        return true;
    }
    if (!ctx_ || !sem.dev) { err_ = "embeddings are loaded but there is no device context: the similarity search has no CPU path"; return false; }
    return sem.expand_batch(ctx_, qt, out, err_);
}

bool Engine::prepare(const std::vector<std::string>& queries, int k, uint32_t flags, ns_batch** out) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { err_ = "no device context: this engine has no CPU scoring path"; return false; }
    const int K = std::max(1, std::min(k, 100));   // src/api_engine.cpp:377
    std::vector<ns_query_desc> qd;
    std::vector<ns_term_ref> refs;
    std::vector<uint8_t> usable;
    build_refs(queries, qd, refs, usable);
    if (refs_failed_) return false;
    int rc = ns_batch_prepare(ctx_, qd.data(), refs.data(), (uint32_t)queries.size(), (uint32_t)K, flags, out);
    if (rc != NS_OK) { err_ = std::string("ns_batch_prepare: ") + ns_last_error(ctx_); return false; }
    return true;
}

bool Engine::search_batch(const std::vector<std::string>& queries, int k, uint32_t flags, std::vector<SearchResult>& out) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    return search_batch_locked(queries, k, flags, out);
}

// Sub-batches of a large batch (search_batch_flat): big enough to keep the device near its full-batch rate, small enough
// that preparing the first one — the only host work the device does not hide — is a small part of the call.  Measured on
// cfg5's 16384 queries (profiles/r03, ns_tool facade-bench): sub-batches of 2048 / 4096 / 5462 / 8192 / no cut =
// 8.4 / 5.0 / 4.6 / 3.65 / 3.83 ms per call.
static constexpr size_t kSubBatchDefault = 8192;
static size_t sub_batch_size() {   // NS_SUBBATCH overrides it (experiments)
    static const size_t v = []() {
        const char* e = std::getenv("NS_SUBBATCH");
        const long n = e ? std::atol(e) : 0;
        return n >= 64 ? (size_t)n : kSubBatchDefault;
    }();
    return v;
}

// the sub-batch ranges [a, b) of a batch of Q in order: fn(a, b), until one says false
template <class Fn>
static bool for_each_sub_batch(size_t Q, Fn fn) {
    const size_t kSubBatch = sub_batch_size();
    const size_t n_sub = Q >= 2 * kSubBatch ? (Q + kSubBatch - 1) / kSubBatch : 1;
    for (size_t i = 0; i < n_sub; i++)
        if (!fn(Q * i / n_sub, Q * (i + 1) / n_sub)) return false;
    return true;
}

// One contiguous range [q0, q1) of a batch on one context.  Two or more sub-batches: prepare(i + 1) on the host || kernels(i)
// on the device || results(i - 1) on their way back.  pooled_prep: query preparation on the engine's host threads (the one
// range of a single-device engine); otherwise on the calling thread (a multi-device engine runs one such call per device).
bool Engine::run_range(ns_ctx* ctx, const QueryView* queries, size_t q0, size_t q1, int K, uint32_t flags, ns_hit* hits, uint32_t* nhits,
                       uint64_t* found, uint8_t* usable, bool pooled_prep, std::string& err, const nsx::RowSource& rs) {
    const size_t Q = q1 - q0;
    const bool and_mode = (flags & NS_FLAG_AND) != 0;
    if (Q == 0) return true;
    const size_t kSubBatch = sub_batch_size();
    const size_t n_sub = Q >= 2 * kSubBatch ? (Q + kSubBatch - 1) / kSubBatch : 1;
    const bool piped = n_sub > 1;
    if (piped) (void)ns_ctx_set_overlap(ctx, 1);
    struct InFlight { ns_batch* b = nullptr; size_t q0 = 0, q1 = 0; };
    InFlight prev;
    bool ok = true;
    auto retire = [&](InFlight& f) {
        if (!f.b) return;
        if (ok) {
            const int rc = ns_batch_fetch(f.b, hits + f.q0 * (size_t)K, nhits + f.q0, found + f.q0);
            if (rc != NS_OK) { err = std::string("ns_batch_fetch: ") + ns_last_error(ctx); ok = false; }
            if (ok && rs.rows)   // a filter's device ids back to manifest positions
                for (size_t q = f.q0; q < f.q1; q++)
                    for (uint32_t i = 0; i < nhits[q]; i++) hits[q * (size_t)K + i].seg_id -= rs.id_base;
        }
        ns_batch_destroy(f.b);
        f.b = nullptr;
    };
    std::vector<ns_query_desc> own_qd;
    std::vector<ns_term_ref> own_refs;
    PrepScratch own_sc;
    std::vector<ns_query_desc>& qd = pooled_prep ? flat_qd_ : own_qd;
    std::vector<ns_term_ref>& refs = pooled_prep ? flat_refs_ : own_refs;
    for (size_t i = 0; i < n_sub && ok; i++) {
        const size_t a = q0 + Q * i / n_sub, b = q0 + Q * (i + 1) / n_sub;
        if (pooled_prep) build_refs_parallel(queries, a, b, qd, refs, usable + a, rs, and_mode);
        else {
            qd.resize(b - a);
            refs.clear();
            build_refs_views(queries, a, b, qd.data(), refs, usable + a, own_sc.text, own_sc.gids, rs, and_mode);
        }
        InFlight cur;
        cur.q0 = a;
        cur.q1 = b;
        int rc = ns_batch_prepare(ctx, qd.data(), refs.data(), (uint32_t)(b - a), (uint32_t)K, flags, &cur.b);
        if (rc == NS_OK) rc = ns_batch_run(cur.b, NS_RUN_FETCH);
        if (rc != NS_OK) {
            err = std::string("ns_batch_prepare/run: ") + ns_last_error(ctx);
            ok = false;
            if (cur.b) ns_batch_destroy(cur.b);
            break;
        }
        retire(prev);     // waits for sub-batch i - 1 only; sub-batch i is already queued behind it
        prev = cur;
    }
    retire(prev);
    if (piped) (void)ns_ctx_set_overlap(ctx, 0);
    return ok;
}

bool Engine::search_batch_flat(const QueryView* queries, size_t Q, int k, uint32_t flags, ns_hit* hits, uint32_t* nhits,
                               uint64_t* found, uint8_t* usable) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { err_ = "no device context: this engine has no CPU scoring path"; return false; }
    if (Q && (!queries || !hits || !nhits || !found || !usable)) { err_ = "search_batch_flat: null argument"; return false; }
    const int K = std::max(1, std::min(k, 100));   // src/api_engine.cpp:377
    if (Q == 0) return true;
    const size_t n_dev = num_devices();
    if (sem.enabled) {
        // semantic expansion runs the whole batch through two device calls on the primary context first
        // (src/api_engine.cpp:409-417); the scoring of the expanded terms is then sharded like any other batch
        std::vector<std::string> qs(Q);
        for (size_t q = 0; q < Q; q++) qs[q].assign(queries[q].p, queries[q].n);
        std::vector<ns_query_desc> qd;
        std::vector<ns_term_ref> refs;
        std::vector<uint8_t> us;
        build_refs(qs, qd, refs, us);
        if (refs_failed_) return false;
        std::memcpy(usable, us.data(), Q);
        std::vector<std::string> errs(n_dev);
        std::vector<int> rcs(n_dev, NS_OK);
        auto shard = [&](size_t d) {
            const auto [a, b] = n_dev > 1 ? shard_bounds(Q, d, n_dev) : std::pair<size_t, size_t>{0, Q};
            if (a >= b) return;
            ns_ctx* c = d == 0 ? ctx_ : replicas_[d - 1].ctx;
            // the shard's descriptors: term_begin stays an index into the one refs array
            rcs[d] = ns_search_batch(c, qd.data() + a, refs.data(), (uint32_t)(b - a), (uint32_t)K, hits + a * (size_t)K, nhits + a, found + a, flags);
            if (rcs[d] != NS_OK) errs[d] = std::string("ns_search_batch: ") + ns_last_error(c);
        };
        if (n_dev > 1 && Q >= 2 * n_dev) {
            std::vector<std::thread> th;
            for (size_t d = 1; d < n_dev; d++) th.emplace_back(shard, d);
            shard(0);
            for (auto& t : th) t.join();
        } else {
            const size_t keep = n_dev; (void)keep;
            rcs[0] = ns_search_batch(ctx_, qd.data(), refs.data(), (uint32_t)Q, (uint32_t)K, hits, nhits, found, flags);
            if (rcs[0] != NS_OK) errs[0] = std::string("ns_search_batch: ") + ns_last_error(ctx_);
        }
        for (size_t d = 0; d < n_dev; d++) if (rcs[d] != NS_OK) { err_ = errs[d]; return false; }
        return true;
    }
    if (n_dev > 1 && Q >= 2 * n_dev) {
        // one host thread + context per device, contiguous shards of ceil(Q / N) queries
        std::vector<std::string> errs(n_dev);
        std::vector<char> oks(n_dev, 1);
        auto shard = [&](size_t d) {
            const auto [a, b] = shard_bounds(Q, d, n_dev);
            ns_ctx* c = d == 0 ? ctx_ : replicas_[d - 1].ctx;
            oks[d] = run_range(c, queries, a, b, K, flags, hits, nhits, found, usable, /*pooled_prep*/ false, errs[d]) ? 1 : 0;
        };
        std::vector<std::thread> th;
        for (size_t d = 1; d < n_dev; d++) th.emplace_back(shard, d);
        shard(0);
        for (auto& t : th) t.join();
        for (size_t d = 0; d < n_dev; d++) if (!oks[d]) { err_ = errs[d]; return false; }
        return true;
    }
    return run_range(ctx_, queries, 0, Q, K, flags, hits, nhits, found, usable, /*pooled_prep*/ true, err_);
}

bool Engine::search_batch_locked(const std::vector<std::string>& queries, int k, uint32_t flags, std::vector<SearchResult>& out) {
    out.clear();
    if (!ctx_) { err_ = "no device context: this engine has no CPU scoring path"; return false; }
    const int K = std::max(1, std::min(k, 100));
    const size_t Q = queries.size();
    std::vector<QueryView> views(Q);
    for (size_t q = 0; q < Q; q++) views[q] = QueryView{queries[q].data(), queries[q].size()};
    std::vector<ns_hit> hits(Q * (size_t)K);
    std::vector<uint32_t> nhits(Q);
    std::vector<uint64_t> found(Q);
    std::vector<uint8_t> usable(Q);
    if (!search_batch_flat(views.data(), Q, k, flags, hits.data(), nhits.data(), found.data(), usable.data())) return false;
    out.resize(Q);
    for (size_t q = 0; q < Q; q++) {
        SearchResult& r = out[q];
        r.query = queries[q];
        r.k = K;
        r.segments = (int)segments.size();
        r.has_found = usable[q] != 0;
        if (!r.has_found) continue;
        r.found = found[q];
        r.hits.reserve(nhits[q]);
        for (uint32_t i = 0; i < nhits[q]; i++) {
            const ns_hit& h = hits[q * (size_t)K + i];
            r.hits.push_back(SearchHit{h.score, h.seg_id, h.doc_id});
        }
    }
    return true;
}

bool Engine::search_hits(const std::string& query, int k, uint32_t flags, SearchResult& out) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    return search_hits_locked(query, k, flags, out);
}

bool Engine::search_hits_locked(const std::string& query, int k, uint32_t flags, SearchResult& out) {
    std::vector<SearchResult> v;
    if (!search_batch_locked({query}, k, flags, v)) return false;
    out = std::move(v[0]);
    return true;
}

std::string Engine::to_json(const SearchResult& r) const {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    return to_json_impl(r);
}

// the "results" member of a search body (and of more_like_this's): src/api_engine.cpp:505-536
void Engine::append_results_json(std::string& o, const std::vector<SearchHit>& hits) const {
    if (hits.empty()) {
        o += "  \"results\": [],\n";
    } else {
        o += "  \"results\": [\n";
        for (size_t i = 0; i < hits.size(); i++) {
            const SearchHit& h = hits[i];
            o += "    {\n";
            // result decoration (src/api_engine.cpp:516-531): only non-empty fields; keys in nlohmann's (alphabetical) order
            const nsx::MetaFields* md = meta.get(h.seg, h.doc);
            if (md && !md->author.empty()) { o += "      \"author\": "; json_escape(o, md->author); o += ",\n"; }
            o += "      \"cord_uid\": ";
            const auto& seg = segments[h.seg];
            json_escape(o, h.doc < seg.cord_uid.size() ? seg.cord_uid[h.doc] : std::string());
            o += ",\n";
            o += "      \"docId\": " + std::to_string(h.doc) + ",\n";
            if (md && !md->publish_time.empty()) { o += "      \"publish_time\": "; json_escape(o, md->publish_time); o += ",\n"; }
            o += "      \"score\": ";
            json_number_from_float(o, h.score);
            o += ",\n";
            o += "      \"segment\": ";
            json_escape(o, seg_names[h.seg]);
            if (md && !md->title.empty()) { o += ",\n      \"title\": "; json_escape(o, md->title); }
            if (md && !md->url.empty()) { o += ",\n      \"url\": "; json_escape(o, md->url); }
            o += "\n";
            o += (i + 1 < hits.size()) ? "    },\n" : "    }\n";
        }
        o += "  ],\n";
    }
}

// no lock: search_batch_json runs it on several threads while the calling thread holds the engine lock
std::string Engine::to_json_impl(const SearchResult& r) const {
    std::string o;
    o += "{\n";
    if (r.has_found) o += "  \"found\": " + std::to_string(r.found) + ",\n";
    o += "  \"k\": " + std::to_string(r.k) + ",\n";
    o += "  \"query\": ";
    json_escape(o, r.query);
    o += ",\n";
    append_results_json(o, r.hits);
    o += "  \"segments\": " + std::to_string(r.segments) + "\n";
    o += "}";
    return o;
}

bool Engine::search_batch_json(const std::vector<std::string>& queries, int k, std::vector<std::string>& out) {
    std::vector<SearchResult> res;
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!search_batch_locked(queries, k, NS_FLAG_OR, res)) return false;
    // result assembly reads segments / meta, which only reload() replaces: the lock is held to the end
    const size_t Q = res.size();
    out.assign(Q, std::string());
    unsigned nt = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
    nt = (unsigned)std::min<size_t>(nt, Q / 512);
    if (nt <= 1) {
        for (size_t q = 0; q < Q; q++) out[q] = to_json_impl(res[q]);
        return true;
    }
    std::vector<std::thread> th;
    for (unsigned i = 0; i < nt; i++)
        th.emplace_back([&, i]() { for (size_t q = Q * i / nt; q < Q * (i + 1) / nt; q++) out[q] = to_json_impl(res[q]); });
    for (auto& t : th) t.join();
    return true;
}

// Every engine entry takes the one engine lock, as the reference does (src/api_engine.cpp:372 `std::lock_guard<std::mutex>
// lock(mtx)`; :54, :168): the HTTP layer calls search() from a thread pool, and the result cache, the error string and
// the device context (one stream, one set of pinned staging buffers: include/nextsearch_hip.h) are not re-entrant.
bool Engine::search_text(const std::string& query, int k, std::string& body) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    const int K = std::max(1, std::min(k, 100));
    const std::string key = query + "|" + std::to_string(K);            // make_cache_key (:190-192), K already clamped (:377-380)
    if (cache_on_) {
        auto it = cache_.find(key);
        if (it != cache_.end()) {                                       // get_from_cache (:195-210)
            lru_.erase(it->second.lru);
            lru_.push_front(key);
            it->second.lru = lru_.begin();
            // result["from_cache"] = true: nlohmann keeps keys sorted, so the flag sits right before "k"
            body = it->second.body;
            const size_t at = body.find("  \"k\": ");
            if (at != std::string::npos) body.insert(at, "  \"from_cache\": true,\n");
            return true;
        }
    }
    SearchResult r;
    if (!search_hits_locked(query, k, NS_FLAG_OR, r)) { body = err_; return false; }   // the message, for the caller that has no other way to it
    body = to_json_impl(r);
    if (cache_on_ && r.has_found) {                                     // put_in_cache (:213-250); the early returns (:407,:424) skip it
        if (cache_.size() >= kMaxCacheSize) {
            auto ev = cache_.find(lru_.back());
            if (ev != cache_.end()) { lru_.erase(ev->second.lru); cache_.erase(ev); }
        }
        lru_.push_front(key);
        cache_[key] = CacheEntry{body, lru_.begin()};
    }
    return true;
}

std::string Engine::search(const std::string& query, int k) {
    std::string body;
    return search_text(query, k, body) ? body : error_body(body);
}

// ---- autocomplete (include/api_engine.hpp:67, src/api_engine.cpp:164-187) --------------------------------------------
// One sub-batch's host side: the inputs' split (base / prefix) and the prefixes that can match something, packed for
// ns_ac_suggest.  An input whose prefix is empty or longer than every term, or a table without terms, has no suggestion
// (api_autocomplete.cpp:190-194) and never reaches the device.
namespace {
struct SuggestPrep {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> offs;
    std::vector<uint32_t> rows;          // input (relative to the sub-batch) of each prefix sent
    std::vector<uint32_t> at, len;       // per input: the prefix run's position in the input; len 0 = not sent
    std::vector<uint32_t> idx, cnt;      // the device's answers per prefix sent
};
}  // namespace

static void suggest_prepare(const Engine::QueryView* in, size_t q0, size_t q1, size_t max_len, uint32_t* base_len, SuggestPrep& sp,
                            ForkJoin* fj) {
    const size_t Q = q1 - q0;
    sp.at.assign(Q, 0);
    sp.len.assign(Q, 0);
    // pass 1 (parallel): the split; the prefix is the last alnum run, lower-cased, so its length is the run's length
    auto split = [&](size_t a, size_t b) {
        for (size_t q = a; q < b; q++) {
            size_t start = 0, end = 0;
            nsx::suggest_last_run(in[q0 + q].p, in[q0 + q].n, start, end);
            base_len[q0 + q] = (uint32_t)start;
            sp.at[q] = (uint32_t)start;
            sp.len[q] = (end > start && end - start <= max_len) ? (uint32_t)(end - start) : 0u;
        }
    };
    const unsigned nt = fj ? std::min<unsigned>(fj->width(), (unsigned)std::max<size_t>(1, Q / 2048)) : 1u;
    if (nt <= 1) split(0, Q);
    else fj->run(nt, [&](unsigned i) { split(Q * i / nt, Q * (i + 1) / nt); });
    sp.rows.clear();
    sp.offs.assign(1, 0);
    uint32_t total = 0;
    for (size_t q = 0; q < Q; q++) {
        if (!sp.len[q]) continue;
        sp.rows.push_back((uint32_t)q);
        total += sp.len[q];
        sp.offs.push_back(total);
    }
    sp.bytes.resize(total);
    // pass 2 (parallel): the lower-cased prefix bytes
    const size_t R = sp.rows.size();
    auto fill = [&](size_t a, size_t b) {
        for (size_t r = a; r < b; r++) {
            const uint32_t q = sp.rows[r];
            const unsigned char* s = (const unsigned char*)in[q0 + q].p + sp.at[q];
            uint8_t* d = sp.bytes.data() + sp.offs[r];
            for (uint32_t j = 0; j < sp.len[q]; j++) d[j] = (s[j] >= 'A' && s[j] <= 'Z') ? (uint8_t)(s[j] - 'A' + 'a') : s[j];
        }
    };
    const unsigned nf = fj ? std::min<unsigned>(fj->width(), (unsigned)std::max<size_t>(1, R / 2048)) : 1u;
    if (nf <= 1) fill(0, R);
    else fj->run(nf, [&](unsigned i) { fill(R * i / nf, R * (i + 1) / nf); });
}

bool Engine::suggest_batch(const QueryView* inputs, size_t Q, int limit, uint32_t* term_idx, uint32_t* count, uint32_t* base_len,
                           float* device_ms) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (device_ms) *device_ms = 0.0f;
    if (!ctx_ || !ac_) { err_ = "no device context: this engine has no CPU autocomplete path"; return false; }
    if (Q && (!inputs || !term_idx || !count || !base_len)) { err_ = "suggest_batch: null argument"; return false; }
    const uint32_t L = (uint32_t)nsx::clamp_suggest_limit(limit);
    if (Q == 0) return true;
    if (Q >= 4096 && (!pool_ || pool_->width() < 2)) pool_.reset(new ForkJoin(std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u)));
    ForkJoin* fj = Q >= 4096 ? pool_.get() : nullptr;
    const size_t kSub = sub_batch_size();
    const size_t n_sub = Q >= 2 * kSub ? (Q + kSub - 1) / kSub : 1;
    const size_t max_len = suggest_table.size() ? suggest_table.max_len : 0;
    SuggestPrep sp[2];
    float dev_ms = 0.0f;
    // the device's part of sub-batch i: ns_ac_suggest on the prefixes sent, answers scattered to the caller's rows
    auto device = [&](size_t i, SuggestPrep& p, std::string& err) -> bool {
        const size_t a = Q * i / n_sub, b = Q * (i + 1) / n_sub;
        for (size_t q = a; q < b; q++) count[q] = 0;
        std::fill(term_idx + a * L, term_idx + b * L, ~0u);
        const uint32_t R = (uint32_t)p.rows.size();
        if (!R) return true;
        p.idx.resize((size_t)R * L);
        p.cnt.resize(R);
        float ms = 0.0f;
        const int rc = ns_ac_suggest(ctx_, ac_, p.bytes.data(), p.offs.data(), R, L, p.idx.data(), p.cnt.data(), device_ms ? &ms : nullptr);
        if (rc != NS_OK) { err = std::string("ns_ac_suggest: ") + ns_last_error(ctx_); return false; }
        dev_ms += ms;
        for (uint32_t r = 0; r < R; r++) {
            const size_t q = a + p.rows[r];
            count[q] = p.cnt[r];
            std::memcpy(term_idx + q * L, p.idx.data() + (size_t)r * L, (size_t)L * 4);
        }
        return true;
    };
    suggest_prepare(inputs, 0, Q * 1 / n_sub, max_len, base_len, sp[0], fj);
    bool ok = true;
    for (size_t i = 0; i < n_sub && ok; i++) {
        SuggestPrep& cur = sp[i & 1];
        if (i + 1 < n_sub) {   // prepare(i + 1) on the host threads while the device answers sub-batch i
            std::string err;
            bool dok = true;
            std::thread dev([&]() { dok = device(i, cur, err); });
            suggest_prepare(inputs, Q * (i + 1) / n_sub, Q * (i + 2) / n_sub, max_len, base_len, sp[(i + 1) & 1], fj);
            dev.join();
            if (!dok) { err_ = err; ok = false; }
        } else if (!device(i, cur, err_)) {
            ok = false;
        }
    }
    if (device_ms) *device_ms = dev_ms;
    return ok;
}

bool Engine::suggest_text(const std::string& input, int limit, std::string& body) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    const uint32_t L = (uint32_t)nsx::clamp_suggest_limit(limit);
    const QueryView v{input.data(), input.size()};
    uint32_t idx[nsx::kSuggestMaxLimit], cnt = 0, base_len = 0;
    if (!suggest_batch(&v, 1, limit, idx, &cnt, &base_len)) { body = err_; return false; }
    // out["query"], out["limit"], out["suggestions"] (src/api_engine.cpp:174-177), printed by dump(2): keys sorted
    body.clear();
    body += "{\n  \"limit\": " + std::to_string(L) + ",\n  \"query\": ";
    json_escape(body, input);
    body += ",\n  \"suggestions\": ";
    if (cnt == 0) {
        body += "[]";
    } else {
        body += "[\n";
        std::string s;
        for (uint32_t r = 0; r < cnt; r++) {
            s.assign(input, 0, base_len);
            s.append(suggest_table.term(idx[r]), suggest_table.term_len(idx[r]));
            body += "    ";
            json_escape(body, s);
            body += r + 1 < cnt ? ",\n" : "\n";
        }
        body += "  ]";
    }
    body += "\n}";
    return true;
}

std::string Engine::suggest(const std::string& input, int limit) {
    std::string body;
    return suggest_text(input, limit, body) ? body : error_body(body);
}

// ---- spelling correction (correct.hpp, csrc/ns_fuzzy.hip) --------------------------------------------------------------
bool Engine::ensure_fuzzy() {
    if (ac_fuzzy_) return true;
    const auto t0 = std::chrono::steady_clock::now();
    if (ns_ac_build_fuzzy(ctx_, ac_, nullptr) != NS_OK) { err_ = std::string("ns_ac_build_fuzzy: ") + ns_last_error(ctx_); return false; }
    correct_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ac_fuzzy_ = true;
    return true;
}

namespace {
struct CorrectPrep {
    std::vector<uint8_t> bytes, edits;
    std::vector<uint32_t> offs;
    std::vector<uint32_t> rows;          // term (relative to the sub-batch) of each term sent
    std::vector<uint32_t> idx, cnt;      // the device's answers per term sent
    std::vector<uint8_t> dist;
};
}  // namespace

// One sub-batch's host side: the terms normalised; those of 1..kFuzzyMaxLen bytes packed for ns_ac_fuzzy.  base_len (completion):
// an input is a suggest request, split like suggest_batch's; its prefix is the term and base_len[q] the bytes before it.
static void correct_prepare(const Engine::QueryView* in, size_t q0, size_t q1, int max_edits, uint32_t* base_len, CorrectPrep& cp, ForkJoin* fj) {
    const size_t Q = q1 - q0;
    std::vector<std::string> norm(Q);
    auto run = [&](size_t a, size_t b) {
        for (size_t q = a; q < b; q++) {
            if (!base_len) { nsx::normalize_token(in[q0 + q].p, in[q0 + q].n, norm[q]); continue; }
            size_t base = 0;
            nsx::split_suggest_input(in[q0 + q].p, in[q0 + q].n, base, norm[q]);
            base_len[q0 + q] = (uint32_t)base;
        }
    };
    const unsigned nt = fj ? std::min<unsigned>(fj->width(), (unsigned)std::max<size_t>(1, Q / 2048)) : 1u;
    if (nt <= 1) run(0, Q);
    else fj->run(nt, [&](unsigned i) { run(Q * i / nt, Q * (i + 1) / nt); });
    cp.rows.clear();
    cp.bytes.clear();
    cp.edits.clear();
    cp.offs.assign(1, 0);
    for (size_t q = 0; q < Q; q++) {
        const std::string& t = norm[q];
        if (t.empty() || t.size() > nsx::kFuzzyMaxLen) continue;
        cp.rows.push_back((uint32_t)q);
        cp.bytes.insert(cp.bytes.end(), t.begin(), t.end());
        cp.offs.push_back((uint32_t)cp.bytes.size());
        cp.edits.push_back((uint8_t)(max_edits < 0 ? nsx::correct_auto_edits(t.size()) : max_edits));
    }
}

bool Engine::correct_batch(const QueryView* terms, size_t Q, int limit, int max_edits, int prefix_len, uint32_t* term_idx, uint8_t* dist,
                           uint32_t* count, float* device_ms) {
    return fuzzy_batch("correct_batch", terms, Q, limit, max_edits, prefix_len, term_idx, dist, count, nullptr, device_ms);
}

bool Engine::complete_batch(const QueryView* inputs, size_t Q, int limit, int max_edits, int prefix_len, uint32_t* term_idx, uint8_t* dist,
                            uint32_t* count, uint32_t* base_len, float* device_ms) {
    if (Q && !base_len) { std::lock_guard<std::recursive_mutex> lock(mtx_); err_ = "complete_batch: null argument"; return false; }
    return fuzzy_batch("complete_batch", inputs, Q, limit, max_edits, prefix_len, term_idx, dist, count, base_len, device_ms);
}

// correct_batch (base_len null: ns_ac_fuzzy on the normalised terms) and complete_batch (ns_ac_fuzzy_prefix on the inputs' prefixes).
bool Engine::fuzzy_batch(const char* fn, const QueryView* terms, size_t Q, int limit, int max_edits, int prefix_len, uint32_t* term_idx,
                         uint8_t* dist, uint32_t* count, uint32_t* base_len, float* device_ms) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (device_ms) *device_ms = 0.0f;
    if (!ctx_ || !ac_) {
        err_ = base_len ? "no device context: this engine has no CPU completion path" : "no device context: this engine has no CPU spelling correction path";
        return false;
    }
    if (Q && (!terms || !term_idx || !dist || !count)) { err_ = std::string(fn) + ": null argument"; return false; }
    if (max_edits > nsx::kFuzzyMaxEdits) { err_ = std::string(fn) + ": max_edits " + std::to_string(max_edits) + " above " + std::to_string(nsx::kFuzzyMaxEdits); return false; }
    const uint32_t L = (uint32_t)nsx::clamp_suggest_limit(limit);
    const uint32_t plen = prefix_len > 0 ? (uint32_t)prefix_len : 0u;
    if (Q == 0) return true;
    if (!ensure_fuzzy()) return false;
    if (Q >= 4096 && (!pool_ || pool_->width() < 2)) pool_.reset(new ForkJoin(std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u)));
    ForkJoin* fj = Q >= 4096 ? pool_.get() : nullptr;
    const size_t kSub = sub_batch_size();
    const size_t n_sub = Q >= 2 * kSub ? (Q + kSub - 1) / kSub : 1;
    CorrectPrep cp[2];
    float dev_ms = 0.0f;
    // the device's part of sub-batch i: ns_ac_fuzzy / ns_ac_fuzzy_prefix on the terms sent, answers scattered to the caller's rows
    const char* call = base_len ? "ns_ac_fuzzy_prefix: " : "ns_ac_fuzzy: ";
    auto device = [&](size_t i, CorrectPrep& p, std::string& err) -> bool {
        const size_t a = Q * i / n_sub, b = Q * (i + 1) / n_sub;
        for (size_t q = a; q < b; q++) count[q] = 0;
        std::fill(term_idx + a * L, term_idx + b * L, ~0u);
        std::fill(dist + a * L, dist + b * L, (uint8_t)0xff);
        const uint32_t R = (uint32_t)p.rows.size();
        if (!R) return true;
        p.idx.resize((size_t)R * L);
        p.dist.resize((size_t)R * L);
        p.cnt.resize(R);
        float ms = 0.0f;
        const int rc = (base_len ? ns_ac_fuzzy_prefix : ns_ac_fuzzy)(ctx_, ac_, p.bytes.data(), p.offs.data(), R, p.edits.data(), plen, L, p.idx.data(),
                                                                    p.dist.data(), p.cnt.data(), device_ms ? &ms : nullptr);
        if (rc != NS_OK) { err = std::string(call) + ns_last_error(ctx_); return false; }
        dev_ms += ms;
        for (uint32_t r = 0; r < R; r++) {
            const size_t q = a + p.rows[r];
            count[q] = p.cnt[r];
            std::memcpy(term_idx + q * L, p.idx.data() + (size_t)r * L, (size_t)L * 4);
            std::memcpy(dist + q * L, p.dist.data() + (size_t)r * L, L);
        }
        return true;
    };
    correct_prepare(terms, 0, Q * 1 / n_sub, max_edits, base_len, cp[0], fj);
    bool ok = true;
    for (size_t i = 0; i < n_sub && ok; i++) {
        CorrectPrep& cur = cp[i & 1];
        if (i + 1 < n_sub) {   // prepare(i + 1) on the host threads while the device answers sub-batch i
            std::string err;
            bool dok = true;
            std::thread dev([&]() { dok = device(i, cur, err); });
            correct_prepare(terms, Q * (i + 1) / n_sub, Q * (i + 2) / n_sub, max_edits, base_len, cp[(i + 1) & 1], fj);
            dev.join();
            if (!dok) { err_ = err; ok = false; }
        } else if (!device(i, cur, err_)) {
            ok = false;
        }
    }
    if (device_ms) *device_ms = dev_ms;
    return ok;
}

bool Engine::did_you_mean_text(const std::string& query, int limit, std::string& body) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_ || !ac_) { err_ = "no device context: this engine has no CPU spelling correction path"; body = err_; return false; }
    const uint32_t L = (uint32_t)nsx::clamp_suggest_limit(limit);
    // the tokens search would score (src/api_engine.cpp:391-397), with their place in the query
    std::vector<nsx::QueryToken> toks;
    for (auto& t : nsx::correct_tokens(query))
        if (t.text.size() >= 2 && !is_stopword(t.text)) toks.push_back(std::move(t));
    std::vector<char> known(toks.size(), 0);
    std::vector<QueryView> ask;
    std::vector<size_t> ask_tok;
    for (size_t i = 0; i < toks.size(); i++) {
        known[i] = dict.find(toks[i].text.data(), toks[i].text.size()) >= 0;
        if (!known[i]) { ask.push_back(QueryView{toks[i].text.data(), toks[i].text.size()}); ask_tok.push_back(i); }
    }
    std::vector<uint32_t> idx(ask.size() * L), cnt(ask.size());
    std::vector<uint8_t> dist(ask.size() * L);
    if (!ask.empty() && !correct_batch(ask.data(), ask.size(), limit, -1, 0, idx.data(), dist.data(), cnt.data())) { body = err_; return false; }
    std::vector<size_t> row(toks.size(), SIZE_MAX);
    for (size_t a = 0; a < ask.size(); a++) row[ask_tok[a]] = a;
    // "corrected": every unknown token with a suggestion replaced by its best one, every other byte kept
    std::string corrected;
    bool changed = false;
    size_t at = 0;
    for (size_t i = 0; i < toks.size(); i++) {
        if (row[i] == SIZE_MAX || cnt[row[i]] == 0) continue;
        const uint32_t best = idx[row[i] * L];
        corrected.append(query, at, toks[i].at - at);
        corrected.append(suggest_table.term(best), suggest_table.term_len(best));
        at = toks[i].at + toks[i].len;
        changed = true;
    }
    corrected.append(query, at, std::string::npos);
    body.clear();
    body += std::string("{\n  \"changed\": ") + (changed ? "true" : "false") + ",\n  \"corrected\": ";
    json_escape(body, corrected);
    body += ",\n  \"query\": ";
    json_escape(body, query);
    body += ",\n  \"terms\": ";
    if (toks.empty()) {
        body += "[]";
    } else {
        body += "[\n";
        for (size_t i = 0; i < toks.size(); i++) {
            body += std::string("    {\n      \"known\": ") + (known[i] ? "true" : "false") + ",\n      \"suggestions\": ";
            const uint32_t n = row[i] == SIZE_MAX ? 0u : cnt[row[i]];
            if (n == 0) {
                body += "[]";
            } else {
                body += "[\n";
                for (uint32_t r = 0; r < n; r++) {
                    const uint32_t t = idx[row[i] * L + r];
                    body += "        {\n          \"distance\": " + std::to_string((unsigned)dist[row[i] * L + r]) + ",\n          \"score\": " +
                            std::to_string(suggest_table.score[t]) + ",\n          \"term\": ";
                    json_escape(body, std::string(suggest_table.term(t), suggest_table.term_len(t)));
                    body += r + 1 < n ? "\n        },\n" : "\n        }\n";
                }
                body += "      ]";
            }
            body += ",\n      \"token\": ";
            json_escape(body, toks[i].text);
            body += i + 1 < toks.size() ? "\n    },\n" : "\n    }\n";
        }
        body += "  ]";
    }
    body += "\n}";
    return true;
}

std::string Engine::did_you_mean(const std::string& query, int limit) {
    std::string body;
    return did_you_mean_text(query, limit, body) ? body : error_body(body);
}

// ---- typo-tolerant completion ----------------------------------------------------------------------------
bool Engine::complete_text(const std::string& input, int limit, std::string& body) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    const uint32_t L = (uint32_t)nsx::clamp_suggest_limit(limit);
    const QueryView v{input.data(), input.size()};
    uint32_t idx[nsx::kSuggestMaxLimit], cnt = 0, base_len = 0;
    uint8_t dist[nsx::kSuggestMaxLimit];
    // auto edits; the first typed byte is trusted: one request scans the terms that start with it, not the table
    if (!complete_batch(&v, 1, limit, -1, 1, idx, dist, &cnt, &base_len)) { body = err_; return false; }
    body.clear();
    body += "{\n  \"limit\": " + std::to_string(L) + ",\n  \"query\": ";
    json_escape(body, input);
    body += ",\n  \"suggestions\": ";
    if (cnt == 0) {
        body += "[]";
    } else {
        body += "[\n";
        std::string s;
        for (uint32_t r = 0; r < cnt; r++) {
            const std::string term(suggest_table.term(idx[r]), suggest_table.term_len(idx[r]));
            s.assign(input, 0, base_len);
            s += term;
            body += "    {\n      \"distance\": " + std::to_string((unsigned)dist[r]) + ",\n      \"score\": " + std::to_string(suggest_table.score[idx[r]]) +
                    ",\n      \"suggestion\": ";
            json_escape(body, s);
            body += ",\n      \"term\": ";
            json_escape(body, term);
            body += r + 1 < cnt ? "\n    },\n" : "\n    }\n";
        }
        body += "  ]";
    }
    body += "\n}";
    return true;
}

std::string Engine::complete(const std::string& input, int limit) {
    std::string body;
    return complete_text(input, limit, body) ? body : error_body(body);
}

// ---- more like this -----------------------------------------------------------------------------------------
bool Engine::similar_term_stats(uint32_t seg, std::vector<uint32_t>& df, std::vector<float>& idf) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (seg >= segments.size()) { err_ = "similar_term_stats: segment " + std::to_string(seg) + " is not in the index"; return false; }
    nsx::SourceSegment src;
    std::string why;
    if (!nsx::load_source(segments[seg].dir, src, why)) { err_ = "similar_term_stats: segment " + seg_names[seg] + " carries no forward index: " + why; return false; }
    nsx::similar_term_stats(segments[seg], src, [](uint32_t N, uint32_t d) { return bm25_idf(N, d); }, df, idf);
    return true;
}

// The host side (forward.bin, terms.bin, df / idf by term id) first, so that a segment without forward files is named
// whether or not there is a device; then the upload to the primary context.
bool Engine::ensure_similar(uint32_t seg) {
    if (similar_.size() != segments.size()) similar_.resize(segments.size());
    SimilarSeg& ss = similar_[seg];
    if (ss.dev) return true;
    nsx::SourceSegment src;
    std::string why;
    if (!nsx::load_source(segments[seg].dir, src, why)) {
        err_ = "similar_batch: segment " + seg_names[seg] + " carries no forward index (legacy and generated segments have none): " + why;
        return false;
    }
    if (!ctx_) { err_ = "similar_batch: no device context (the term selection and the scoring run on the device; there is no CPU path)"; return false; }
    std::vector<uint32_t> df;
    std::vector<float> idf;
    nsx::similar_term_stats(segments[seg], src, [](uint32_t N, uint32_t d) { return bm25_idf(N, d); }, df, idf);
    ns_forward_src fs;
    nsx::fill_forward_src(src, fs);
    const int rc = ns_docterms_upload(ctx_, &fs, df.data(), idf.data(), &ss.dev);
    if (rc != NS_OK) { ss.dev = nullptr; err_ = "similar_batch: segment " + seg_names[seg] + ": " + ns_last_error(ctx_); return false; }
    ss.term_bytes = std::move(src.term_bytes);
    ss.term_offsets = std::move(src.term_offsets);
    return true;
}

bool Engine::similar_batch(const std::pair<uint32_t, uint32_t>* seg_doc, size_t Q, int k, const nsx::SimilarOptions& opt, ns_hit* hits,
                           uint32_t* nhits, uint64_t* found, uint8_t* usable, std::vector<nsx::WeightedTerms>* terms_out) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    err_.clear();
    if (terms_out) terms_out->clear();
    if (Q && (!seg_doc || !hits || !nhits || !found || !usable)) { err_ = "similar_batch: null argument"; return false; }
    if (Q >= 0xFFFFFFFFull) { err_ = "similar_batch: too many sources"; return false; }
    const uint32_t K = (uint32_t)std::max(1, std::min(k, 99)), K1 = K + 1;   // the search runs with K + 1 <= NS_MAX_K
    for (size_t q = 0; q < Q; q++)
        if (seg_doc[q].first >= segments.size() || seg_doc[q].second >= segments[seg_doc[q].first].cord_uid.size()) {
            err_ = "similar_batch: (segment " + std::to_string(seg_doc[q].first) + ", document " + std::to_string(seg_doc[q].second) + ") is not in the index";
            return false;
        }
    if (Q == 0) {
        if (!ctx_) { err_ = "similar_batch: no device context (the term selection and the scoring run on the device; there is no CPU path)"; return false; }
        return true;
    }
    // ---- selection: one ns_docterms_select per segment named ----
    const uint32_t T = nsx::similar_clamp_terms(opt.max_terms);
    std::vector<std::vector<uint32_t>> rows_of(segments.size());
    for (size_t q = 0; q < Q; q++) rows_of[seg_doc[q].first].push_back((uint32_t)q);
    for (uint32_t s = 0; s < segments.size(); s++)
        if (!rows_of[s].empty() && !ensure_similar(s)) return false;
    std::vector<uint32_t> sel_term(Q * (size_t)T), sel_cnt(Q);
    std::vector<float> sel_w(Q * (size_t)T);
    {
        std::vector<uint32_t> ids, t_, c_;
        std::vector<float> w_;
        for (uint32_t s = 0; s < segments.size(); s++) {
            const std::vector<uint32_t>& rows = rows_of[s];
            if (rows.empty()) continue;
            ids.resize(rows.size()); t_.resize(rows.size() * (size_t)T); w_.resize(rows.size() * (size_t)T); c_.resize(rows.size());
            for (size_t i = 0; i < rows.size(); i++) ids[i] = seg_doc[rows[i]].second;
            const int rc = ns_docterms_select(similar_[s].dev, ids.data(), (uint32_t)ids.size(), opt.max_terms, opt.min_tf, opt.min_df, opt.max_df,
                                              t_.data(), w_.data(), c_.data(), nullptr);
            if (rc != NS_OK) { err_ = "ns_docterms_select (segment " + seg_names[s] + "): " + ns_last_error(ctx_); return false; }
            for (size_t i = 0; i < rows.size(); i++) {
                std::memcpy(&sel_term[rows[i] * (size_t)T], &t_[i * (size_t)T], (size_t)T * 4);
                std::memcpy(&sel_w[rows[i] * (size_t)T], &w_[i * (size_t)T], (size_t)T * 4);
                sel_cnt[rows[i]] = c_[i];
            }
        }
    }
    if (terms_out) terms_out->assign(Q, {});
    // ---- term refs of sources [a, b): ids -> bytes (terms.bin) -> one dictionary probe -> every segment, selection order ----
    const uint32_t S = (uint32_t)segments.size();
    // sources [a, b) into refs (appended); qd[q - q_base].term_begin counts from refs' start
    auto build_slice = [&](size_t a, size_t b, size_t q_base, ns_query_desc* qd, std::vector<ns_term_ref>& refs, std::vector<uint32_t>& gids) {
        float qw[nsx::kSimilarMaxTerms];
        for (size_t q = a; q < b; q++) {
            const SimilarSeg& ss = similar_[seg_doc[q].first];
            const uint32_t* tid = &sel_term[q * (size_t)T];
            const float* w = &sel_w[q * (size_t)T];
            const uint32_t n = sel_cnt[q];
            ns_query_desc& d = qd[q - q_base];
            d.term_begin = (uint32_t)refs.size();
            usable[q] = n != 0 ? 1 : 0;
            gids.clear();
            uint32_t n_q = 0;
            for (uint32_t r = 0; r < n; r++) {
                const char* tp = (const char*)ss.term_bytes.data() + ss.term_offsets[tid[r]];
                const size_t tn = (size_t)(ss.term_offsets[tid[r] + 1] - ss.term_offsets[tid[r]]);
                if (terms_out) (*terms_out)[q].emplace_back(std::string(tp, tn), w[r]);
                const int64_t g = dict.find(tp, tn);
                if (g < 0) continue;
                gids.push_back((uint32_t)g);
                qw[n_q++] = nsx::similar_qweight(w[r], w[0], opt.boost);
            }
            for (uint32_t sid = 0; sid < S; sid++)
                for (uint32_t i = 0; i < n_q; i++) {
                    const nsx::TermSeg& e = dict.row(gids[i])[sid];
                    if (e.byte_off == nsx::kAbsent) continue;
                    refs.push_back(ns_term_ref{sid, e.count, e.byte_off, e.idf, qw[i]});
                }
            d.term_count = (uint32_t)refs.size() - d.term_begin;
        }
    };
    // ... on the engine's host threads, as build_refs_parallel cuts a text batch (the dictionary is read-only; every source
    // writes its own usable / terms_out entry), the slices' refs concatenated in source order
    auto build = [&](size_t a, size_t b, std::vector<ns_query_desc>& qd, std::vector<ns_term_ref>& refs) {
        const size_t n = b - a;
        qd.assign(n, ns_query_desc{0, 0});
        refs.clear();
        const unsigned nt = prep_width(n);
        if (scratch_.size() < std::max(1u, nt)) scratch_.resize(std::max(1u, nt));
        if (nt <= 1) { build_slice(a, b, a, qd.data(), refs, scratch_[0].gids); return; }
        if (!pool_ || pool_->width() < nt) pool_.reset(new ForkJoin(std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u)));
        pool_->run(nt, [&](unsigned i) {
            PrepScratch& sc = scratch_[i];
            sc.refs.clear();
            const size_t lo = a + n * i / nt, hi = a + n * (i + 1) / nt;
            build_slice(lo, hi, a, qd.data(), sc.refs, sc.gids);
        });
        size_t total = 0;
        std::vector<size_t> base(nt);
        for (unsigned i = 0; i < nt; i++) { base[i] = total; total += scratch_[i].refs.size(); }
        refs.resize(total);
        pool_->run(nt, [&](unsigned i) {
            for (size_t q = n * i / nt; q < n * (i + 1) / nt; q++) qd[q].term_begin += (uint32_t)base[i];
            if (!scratch_[i].refs.empty()) std::memcpy(refs.data() + base[i], scratch_[i].refs.data(), scratch_[i].refs.size() * sizeof(ns_term_ref));
        });
    };
    // ---- the existing batch path with K + 1, sub-batches pipelined as run_range does ----
    std::vector<ns_hit> h1(Q * (size_t)K1);
    std::vector<uint32_t> n1(Q);
    std::vector<uint64_t> f1(Q);
    {
        const size_t kSubBatch = sub_batch_size();
        const size_t n_sub = Q >= 2 * kSubBatch ? (Q + kSubBatch - 1) / kSubBatch : 1;
        const bool piped = n_sub > 1;
        if (piped) (void)ns_ctx_set_overlap(ctx_, 1);
        struct InFlight { ns_batch* b = nullptr; size_t q0 = 0; };
        InFlight prev;
        bool ok = true;
        auto retire = [&](InFlight& f) {
            if (!f.b) return;
            if (ok) {
                const int rc = ns_batch_fetch(f.b, h1.data() + f.q0 * (size_t)K1, n1.data() + f.q0, f1.data() + f.q0);
                if (rc != NS_OK) { err_ = std::string("ns_batch_fetch: ") + ns_last_error(ctx_); ok = false; }
            }
            ns_batch_destroy(f.b);
            f.b = nullptr;
        };
        std::vector<ns_query_desc> qd;
        std::vector<ns_term_ref> refs;
        for (size_t i = 0; i < n_sub && ok; i++) {
            const size_t a = Q * i / n_sub, b = Q * (i + 1) / n_sub;
            build(a, b, qd, refs);
            InFlight cur;
            cur.q0 = a;
            int rc = ns_batch_prepare(ctx_, qd.data(), refs.data(), (uint32_t)(b - a), K1, NS_FLAG_OR, &cur.b);
            if (rc == NS_OK) rc = ns_batch_run(cur.b, NS_RUN_FETCH);
            if (rc != NS_OK) {
                err_ = std::string("ns_batch_prepare/run: ") + ns_last_error(ctx_);
                ok = false;
                if (cur.b) ns_batch_destroy(cur.b);
                break;
            }
            retire(prev);
            prev = cur;
        }
        retire(prev);
        if (piped) (void)ns_ctx_set_overlap(ctx_, 0);
        if (!ok) return false;
    }
    // ---- the source leaves its own row ----
    const ns_hit pad{-std::numeric_limits<float>::infinity(), 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (size_t q = 0; q < Q; q++) {
        ns_hit* out = hits + q * (size_t)K;
        uint32_t n = 0;
        if (usable[q]) {
            const ns_hit* in = h1.data() + q * (size_t)K1;
            for (uint32_t i = 0; i < n1[q] && n < K; i++) {
                if (in[i].seg_id == seg_doc[q].first && in[i].doc_id == seg_doc[q].second) continue;
                out[n++] = in[i];                                       // source absent from the K + 1: the last one is dropped
            }
        }
        nhits[q] = n;
        found[q] = usable[q] && f1[q] ? f1[q] - 1 : 0;
        for (uint32_t i = n; i < K; i++) out[i] = pad;
    }
    return true;
}

bool Engine::more_like_this_text(const std::string& uid, int k, std::string& body) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    const uint32_t K = (uint32_t)std::max(1, std::min(k, 99));
    std::vector<std::pair<uint32_t, uint32_t>> where;
    find_documents({uid}, where);
    if (where.empty()) { err_ = "more_like_this: no document with cord_uid \"" + uid + "\" in the index"; body = err_; return false; }
    const std::pair<uint32_t, uint32_t> src = where[0];                // the first match is the source
    std::vector<ns_hit> hits(K);
    uint32_t nh = 0;
    uint64_t fd = 0;
    uint8_t us = 0;
    std::vector<nsx::WeightedTerms> terms;
    if (!similar_batch(&src, 1, k, nsx::SimilarOptions{}, hits.data(), &nh, &fd, &us, &terms)) { body = err_; return false; }
    std::vector<SearchHit> sh;
    for (uint32_t i = 0; i < nh; i++) sh.push_back(SearchHit{hits[i].score, hits[i].seg_id, hits[i].doc_id});
    std::string& o = body;
    o.clear();
    o += "{\n";
    if (us) o += "  \"found\": " + std::to_string(fd) + ",\n";
    o += "  \"k\": " + std::to_string(K) + ",\n";
    if (terms[0].empty()) {
        o += "  \"query_terms\": [],\n";
    } else {
        o += "  \"query_terms\": [\n";
        for (size_t i = 0; i < terms[0].size(); i++) {
            o += "    {\n      \"term\": ";
            json_escape(o, terms[0][i].first);
            o += ",\n      \"weight\": ";
            json_number_from_float(o, terms[0][i].second);
            o += i + 1 < terms[0].size() ? "\n    },\n" : "\n    }\n";
        }
        o += "  ],\n";
    }
    append_results_json(o, sh);
    o += "  \"segments\": " + std::to_string(segments.size()) + ",\n";
    o += "  \"source\": {\n    \"cord_uid\": ";
    json_escape(o, uid);
    o += ",\n    \"docId\": " + std::to_string(src.second) + ",\n    \"segment\": ";
    json_escape(o, seg_names[src.first]);
    o += "\n  }\n}";
    return true;
}

std::string Engine::more_like_this(const std::string& uid, int k) {
    std::string body;
    return more_like_this_text(uid, k, body) ? body : error_body(body);
}

// ---- related terms (host/related.hpp, csrc/ns_terms.hip) ---------------------------------------------------
bool Engine::related_rows(const std::pair<uint32_t, uint32_t>* seg_doc, const uint64_t* row_off, size_t Q, const nsx::RelatedOptions& opt,
                          std::vector<std::vector<nsx::RelatedCand>>& rows, std::vector<uint32_t>& ndocs, float* device_ms) {
    rows.clear();
    ndocs.clear();
    if (device_ms) *device_ms = 0.0f;
    if (Q && (!row_off || (row_off[Q] && !seg_doc))) { err_ = "terms_batch: null argument"; return false; }
    if (Q >= 0xFFFFFFFFull) { err_ = "terms_batch: too many rows"; return false; }
    if (Q && row_off[0] != 0) { err_ = "terms_batch: row_off[0] is not 0"; return false; }
    for (size_t q = 0; q < Q; q++)
        if (row_off[q + 1] < row_off[q]) { err_ = "terms_batch: row_off[" + std::to_string(q + 1) + "] is below row_off[" + std::to_string(q) + "]"; return false; }
    for (uint64_t j = 0; Q && j < row_off[Q]; j++)
        if (seg_doc[j].first >= segments.size() || seg_doc[j].second >= segments[seg_doc[j].first].cord_uid.size()) {
            err_ = "terms_batch: (segment " + std::to_string(seg_doc[j].first) + ", document " + std::to_string(seg_doc[j].second) + ") is not in the index";
            return false;
        }
    if (!ctx_) { err_ = "terms_batch: no device context (the counting runs on the device; there is no CPU path)"; return false; }
    rows.resize(Q);
    ndocs.assign(Q, 0u);
    if (Q == 0) return true;
    const uint32_t S = (uint32_t)segments.size(), T = nsx::kRelatedMaxTerms;
    const bool one = S == 1;                                           // the options reach the device as they are
    const uint32_t dev_min_docs = one ? opt.min_docs : 1u, dev_min_df = one ? opt.min_df : 1u, dev_max_df = one ? opt.max_df : 0xFFFFFFFFu;
    uint64_t N = 0;
    for (const auto& seg : segments) N += seg.N;
    struct Part { uint32_t docs = 0, first_pos = 0, term_id = 0; };
    std::vector<std::unordered_map<std::string, Part>> acc(Q);
    std::vector<uint32_t> which, ids, t_, g_, c_, n_;
    std::vector<uint64_t> off;
    std::vector<float> w_;
    std::string key;
    for (uint32_t s = 0; s < S; s++) {
        which.clear(); ids.clear(); off.assign(1, 0ull);
        for (size_t q = 0; q < Q; q++) {
            const size_t before = ids.size();
            for (uint64_t j = row_off[q]; j < row_off[q + 1]; j++)
                if (seg_doc[j].first == s) ids.push_back(seg_doc[j].second);
            if (ids.size() == before) continue;
            which.push_back((uint32_t)q);
            off.push_back(ids.size());
        }
        if (which.empty()) continue;
        if (!ensure_similar(s)) return false;
        const size_t R = which.size();
        t_.resize(R * T); g_.resize(R * T); w_.resize(R * T); c_.resize(R); n_.resize(R);
        float ms = 0.0f;
        const int rc = ns_docterms_aggregate(similar_[s].dev, ids.data(), off.data(), (uint32_t)R, T, opt.min_tf, dev_min_docs, dev_min_df, dev_max_df,
                                             t_.data(), g_.data(), w_.data(), c_.data(), n_.data(), &ms);
        if (rc != NS_OK) { err_ = "ns_docterms_aggregate (segment " + seg_names[s] + "): " + ns_last_error(ctx_); return false; }
        if (device_ms) *device_ms += ms;
        const SimilarSeg& ss = similar_[s];
        for (size_t i = 0; i < R; i++) {
            ndocs[which[i]] += n_[i];
            for (uint32_t r = 0; r < c_[i]; r++) {
                const uint32_t t = t_[i * T + r];
                key.assign((const char*)ss.term_bytes.data() + ss.term_offsets[t], (size_t)(ss.term_offsets[t + 1] - ss.term_offsets[t]));
                auto ins = acc[which[i]].emplace(key, Part{0u, s, t});   // segments in manifest order: the first holder stays
                ins.first->second.docs += g_[i * T + r];
            }
        }
    }
    const uint32_t need_docs = std::max(1u, opt.min_docs);
    for (size_t q = 0; q < Q; q++) {
        std::vector<nsx::RelatedCand>& out = rows[q];
        for (const auto& kv : acc[q]) {
            uint64_t df = 0;
            for (const auto& seg : segments) {
                const auto it = seg.lex.find(kv.first);
                if (it != seg.lex.end()) df += it->second.df;
            }
            if (kv.second.docs < need_docs || df < 1 || df < opt.min_df || df > opt.max_df || df > 0xFFFFFFFFull) continue;
            const float idf = bm25_idf((uint32_t)std::min<uint64_t>(N, 0xFFFFFFFFull), (uint32_t)df);
            if (!(idf > 0.0f) || !(idf <= std::numeric_limits<float>::max())) continue;
            nsx::RelatedCand c;
            c.term = kv.first; c.docs = kv.second.docs; c.df = df; c.w = (float)kv.second.docs * idf;
            c.first_pos = kv.second.first_pos; c.term_id = kv.second.term_id;
            out.push_back(std::move(c));
        }
        nsx::related_merge_order(out);
    }
    return true;
}

bool Engine::terms_batch(const std::pair<uint32_t, uint32_t>* seg_doc, const uint64_t* row_off, size_t Q, const nsx::RelatedOptions& opt,
                         uint32_t* docs_out, uint64_t* df_out, float* w_out, uint32_t* count_out, uint32_t* ndocs_out,
                         std::vector<std::vector<std::string>>* terms_out, float* device_ms) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    err_.clear();
    if (terms_out) terms_out->clear();
    if (Q && (!docs_out || !df_out || !w_out || !count_out || !ndocs_out)) { err_ = "terms_batch: null argument"; return false; }
    std::vector<std::vector<nsx::RelatedCand>> rows;
    std::vector<uint32_t> ndocs;
    if (!related_rows(seg_doc, row_off, Q, opt, rows, ndocs, device_ms)) return false;
    const uint32_t To = nsx::related_clamp_out(opt.max_terms);
    if (terms_out) terms_out->assign(Q, {});
    for (size_t q = 0; q < Q; q++) {
        const uint32_t n = (uint32_t)std::min<size_t>(rows[q].size(), To);
        for (uint32_t r = 0; r < To; r++) {
            docs_out[q * To + r] = r < n ? rows[q][r].docs : 0u;
            df_out[q * To + r] = r < n ? rows[q][r].df : 0ull;
            w_out[q * To + r] = r < n ? rows[q][r].w : 0.0f;
            if (terms_out && r < n) (*terms_out)[q].push_back(rows[q][r].term);
        }
        count_out[q] = n;
        ndocs_out[q] = ndocs[q];
    }
    return true;
}

bool Engine::related_terms_text(const std::string& query, const nsx::RelatedOptions& opt, const nsx::DocFilter* f, std::string& body) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    err_.clear();
    if (!ctx_) { body = err_ = "related_terms: no device context (the search and the counting run on the device; there is no CPU path)"; return false; }
    const int K = (int)nsx::related_clamp_sample(opt.sample);
    const QueryView qv{query.data(), query.size()};
    std::vector<ns_hit> hits((size_t)K);
    uint32_t nh = 0;
    uint64_t fd = 0;
    uint8_t us = 0;
    if (f) {
        nsx::DateRange r;
        OpenFilter* of = lru_filter(*f, r);
        if (!of) { body = err_; return false; }
        if (!search_filtered_batch_flat(of->handle, &qv, 1, K, NS_FLAG_OR, hits.data(), &nh, &fd, &us)) { body = err_; return false; }
    } else if (!search_batch_flat(&qv, 1, K, NS_FLAG_OR, hits.data(), &nh, &fd, &us)) { body = err_; return false; }
    if (!us) { nh = 0; fd = 0; }
    std::vector<std::pair<uint32_t, uint32_t>> row(nh);
    for (uint32_t i = 0; i < nh; i++) row[i] = {hits[i].seg_id, hits[i].doc_id};
    const uint64_t off[2] = {0, nh};
    std::vector<std::vector<nsx::RelatedCand>> rows;
    std::vector<uint32_t> ndocs;
    if (!related_rows(row.data(), off, 1, opt, rows, ndocs, nullptr)) { body = err_; return false; }
    const std::vector<std::string> own = base_terms(query);
    const uint32_t To = nsx::related_clamp_out(opt.max_terms);
    std::vector<const nsx::RelatedCand*> keep;
    for (const nsx::RelatedCand& c : rows[0]) {
        if (keep.size() == To) break;
        if (std::find(own.begin(), own.end(), c.term) == own.end()) keep.push_back(&c);
    }
    std::string& o = body;
    o.clear();
    o += "{\n  \"found\": " + std::to_string(fd) + ",\n  \"query\": ";
    json_escape(o, query);
    o += ",\n  \"sample\": " + std::to_string(nh) + ",\n  \"segments\": " + std::to_string(segments.size()) + ",\n";
    if (keep.empty()) {
        o += "  \"terms\": []\n}";
        return true;
    }
    o += "  \"terms\": [\n";
    for (size_t i = 0; i < keep.size(); i++) {
        o += "    {\n      \"df\": " + std::to_string(keep[i]->df) + ",\n      \"docs\": " + std::to_string(keep[i]->docs) + ",\n      \"term\": ";
        json_escape(o, keep[i]->term);
        o += ",\n      \"weight\": ";
        json_number_from_float(o, keep[i]->w);
        o += i + 1 < keep.size() ? "\n    },\n" : "\n    }\n";
    }
    o += "  ]\n}";
    return true;
}

std::string Engine::related_terms(const std::string& query, const nsx::RelatedOptions& opt, const nsx::DocFilter* f) {
    std::string body;
    return related_terms_text(query, opt, f, body) ? body : error_body(body);
}

// ---- filtered search (host/filter.hpp, csrc/ns_filter.hip) ------------------------------------------------
bool Engine::filter_bits(const nsx::DocFilter& f, std::vector<std::vector<uint32_t>>& bits) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    bits.clear();
    nsx::DateRange r;
    if (!nsx::parse_filter(f, r, err_)) return false;
    bits.resize(segments.size());
    for (uint32_t s = 0; s < segments.size(); s++) {
        const uint32_t N = segments[s].N;
        bits[s].assign(((size_t)N + 31) / 32, 0u);
        for (uint32_t d = 0; d < N; d++) {
            const nsx::MetaFields* md = meta.get(s, d);   // nullptr: no metadata row = undated
            if (r.keeps(md ? nsx::date_key(md->publish_time) : 0u)) bits[s][d >> 5] |= 1u << (d & 31u);
        }
    }
    return true;
}

Engine::OpenFilter* Engine::filter_of(uint32_t handle) {
    OpenFilter& f = filters_[handle % kMaxFilters];
    return (f.open && f.handle == handle) ? &f : nullptr;
}

void Engine::close_filter_slot(OpenFilter& f) {
    if (ctx_)
        for (ns_seg* s : f.segs)
            if (s) (void)ns_segment_release(ctx_, s);
    f = OpenFilter{};
}

void Engine::close_all_filters() {
    for (OpenFilter& f : filters_) if (f.open) close_filter_slot(f);
    filter_lru_.clear();
}

size_t Engine::open_filters() const {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    size_t n = 0;
    for (const OpenFilter& f : filters_) n += f.open;
    return n;
}

bool Engine::close_filter(uint32_t handle) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    OpenFilter* f = filter_of(handle);
    if (!f) { err_ = "close_filter: handle " + std::to_string(handle) + " is stale (the filter was closed, or the index was reloaded after it was opened)"; return false; }
    close_filter_slot(*f);
    filter_lru_.remove_if([&](const FilterLruEnt& e) { return e.handle == handle; });
    return true;
}

bool Engine::open_filter(const nsx::DocFilter& f, uint32_t& handle, nsx::FilterStats* stats) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { err_ = "open_filter: no device context: a filter is built on the device, there is no CPU path"; return false; }
    std::vector<std::vector<uint32_t>> bits;
    if (!filter_bits(f, bits)) return false;
    return open_filter(bits, handle, stats);
}

bool Engine::open_filter(const std::vector<std::vector<uint32_t>>& bits, uint32_t& handle, nsx::FilterStats* stats) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    const auto t0 = std::chrono::steady_clock::now();
    if (!ctx_) { err_ = "open_filter: no device context: a filter is built on the device, there is no CPU path"; return false; }
    const uint32_t S = (uint32_t)segments.size();
    if (bits.size() != S) { err_ = "open_filter: " + std::to_string(bits.size()) + " bitmaps for " + std::to_string(S) + " segments"; return false; }
    for (uint32_t s = 0; s < S; s++)
        if (bits[s].size() != ((size_t)segments[s].N + 31) / 32) {
            err_ = "open_filter: the bitmap of segment " + std::to_string(s) + " has " + std::to_string(bits[s].size()) + " words, its " +
                   std::to_string(segments[s].N) + " documents need " + std::to_string(((size_t)segments[s].N + 31) / 32);
            return false;
        }
    size_t slot = kMaxFilters;
    for (size_t i = 0; i < kMaxFilters; i++) if (!filters_[i].open) { slot = i; break; }
    if (slot == kMaxFilters) { err_ = "open_filter: " + std::to_string(kMaxFilters) + " filters are open already; close one first"; return false; }
    if (((uint64_t)slot + 2) * S > (1u << 20)) { err_ = "open_filter: the filter's device segment ids would reach 2^20"; return false; }
    const uint32_t id_base = (uint32_t)(slot + 1) * S;

    OpenFilter fl;
    fl.segs.assign(S, nullptr);
    const size_t T = dict.n_terms();
    fl.rows.assign(T * (size_t)S, nsx::TermSeg{nsx::kAbsent, 0u, 0.0f});
    nsx::FilterStats fs;
    std::vector<uint64_t> off, noff;
    std::vector<uint32_t> cnt, ncnt, gid;
    auto undo = [&]() { for (ns_seg* s : fl.segs) if (s) (void)ns_segment_release(ctx_, s); };
    for (uint32_t sid = 0; sid < S; sid++) {
        const nsx::SegmentData& sd = segments[sid];
        fs.docs_total += sd.N;
        fs.postings_total += sd.postings_bytes / 8;
        uint64_t kept_docs = 0;
        for (uint32_t w = 0; w < bits[sid].size(); w++) {
            uint32_t v = bits[sid][w];
            if (w + 1 == bits[sid].size() && (sd.N & 31u)) v &= (1u << (sd.N & 31u)) - 1u;   // bits past N do not count
            kept_docs += (uint64_t)__builtin_popcount(v);
        }
        fs.docs_kept += kept_docs;
        if (!kept_docs || !dev_segs_[sid]) continue;
        // every list of the dictionary that lies inside the payload (a damaged record stays absent under the filter)
        off.clear(); cnt.clear(); gid.clear();
        for (size_t g = 0; g < T; g++) {
            const nsx::TermSeg& e = dict.row((uint32_t)g)[sid];
            if (e.byte_off == nsx::kAbsent || e.byte_off % 8 != 0 || e.byte_off / 8 + e.count > sd.postings_bytes / 8) continue;
            off.push_back(e.byte_off); cnt.push_back(e.count); gid.push_back((uint32_t)g);
        }
        noff.resize(off.size()); ncnt.resize(off.size());
        uint64_t kept = 0;
        float ms = 0.0f;
        int rc = ns_segment_filter(ctx_, dev_segs_[sid], id_base + sid, bits[sid].data(), off.data(), cnt.data(), (uint32_t)off.size(),
                                   noff.data(), ncnt.data(), nullptr, &kept, &ms, &fl.segs[sid]);
        if (rc != NS_OK) { err_ = std::string("ns_segment_filter: ") + ns_last_error(ctx_); undo(); return false; }
        fs.device_ms += ms;
        if (!kept) {   // no surviving posting: no copy, no refs
            (void)ns_segment_release(ctx_, fl.segs[sid]);
            fl.segs[sid] = nullptr;
            continue;
        }
        fs.postings_kept += kept;
        fs.segments_on_device++;
        fs.hbm_bytes += (kept + 256) * 12 + (uint64_t)std::max<uint32_t>(sd.N, 1) * 4;
        const uint32_t min_count = std::max<uint32_t>(64u, sd.N / 512u);   // reload()'s rule for skip tables
        std::vector<uint64_t> soff;
        std::vector<uint32_t> scnt;
        for (size_t i = 0; i < off.size(); i++) {
            if (!ncnt[i]) continue;
            fl.rows[(size_t)gid[i] * S + sid] = nsx::TermSeg{noff[i], ncnt[i], dict.row(gid[i])[sid].idf};
            if (ncnt[i] >= min_count) { soff.push_back(noff[i]); scnt.push_back(ncnt[i]); }
        }
        if (!soff.empty()) (void)ns_segment_build_skips(ctx_, fl.segs[sid], soff.data(), scnt.data(), (uint32_t)soff.size());
    }
    fl.open = true;
    fl.docs_kept = fs.docs_kept;
    filter_gen_++;
    fl.handle = (uint32_t)(filter_gen_ * kMaxFilters + slot);
    handle = fl.handle;
    filters_[slot] = std::move(fl);
    fs.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = fs;
    return true;
}

bool Engine::search_filtered_batch_flat(uint32_t handle, const QueryView* queries, size_t Q, int k, uint32_t flags, ns_hit* hits,
                                        uint32_t* nhits, uint64_t* found, uint8_t* usable) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { err_ = "no device context: this engine has no CPU scoring path"; return false; }
    OpenFilter* f = filter_of(handle);
    if (!f) { err_ = "search_filtered: handle " + std::to_string(handle) + " is stale (the filter was closed, or the index was reloaded after it was opened)"; return false; }
    if (Q && (!queries || !hits || !nhits || !found || !usable)) { err_ = "search_filtered_batch_flat: null argument"; return false; }
    const int K = std::max(1, std::min(k, 100));
    if (Q == 0) return true;
    nsx::RowSource rs;
    rs.rows = f->rows.data();
    rs.id_base = (uint32_t)(handle % kMaxFilters + 1) * (uint32_t)segments.size();
    static const nsx::TermSeg no_rows{nsx::kAbsent, 0u, 0.0f};
    if (!rs.rows) rs.rows = &no_rows;   // an index without terms: never read, but "filtered" all the same
    if (sem.enabled) {   // the expansion of search_batch_flat, then the expanded terms over the filter's rows
        std::vector<std::string> qs(Q);
        for (size_t q = 0; q < Q; q++) qs[q].assign(queries[q].p, queries[q].n);
        std::vector<nsx::WeightedTerms> expanded;
        if (!expand_queries(qs, expanded)) return false;
        std::vector<ns_query_desc> qd(Q, ns_query_desc{0, 0});
        std::vector<ns_term_ref> refs;
        std::vector<uint8_t> us(Q, 0);
        build_refs_range(qs, 0, Q, qd, refs, us, &expanded, rs, (flags & NS_FLAG_AND) != 0);
        std::memcpy(usable, us.data(), Q);
        const int rc = ns_search_batch(ctx_, qd.data(), refs.data(), (uint32_t)Q, (uint32_t)K, hits, nhits, found, flags);
        if (rc != NS_OK) { err_ = std::string("ns_search_batch: ") + ns_last_error(ctx_); return false; }
        for (size_t q = 0; q < Q; q++)
            for (uint32_t i = 0; i < nhits[q]; i++) hits[q * (size_t)K + i].seg_id -= rs.id_base;
        return true;
    }
    return run_range(ctx_, queries, 0, Q, K, flags, hits, nhits, found, usable, /*pooled_prep*/ true, err_, rs);
}

// search_filtered's and related_terms' cache of open filters: the last kFilterLru distinct filters stay open
Engine::OpenFilter* Engine::lru_filter(const nsx::DocFilter& f, nsx::DateRange& r) {
    if (!nsx::parse_filter(f, r, err_)) return nullptr;
    const std::string key = r.cache_key();
    OpenFilter* of = nullptr;
    for (auto it = filter_lru_.begin(); it != filter_lru_.end(); ++it)
        if (it->key == key) {
            of = filter_of(it->handle);
            if (of) filter_lru_.splice(filter_lru_.begin(), filter_lru_, it);
            else filter_lru_.erase(it);   // closed behind the cache's back
            break;
        }
    if (!of) {
        while (filter_lru_.size() >= kFilterLru) {   // the least recently used goes
            if (OpenFilter* old = filter_of(filter_lru_.back().handle)) close_filter_slot(*old);
            filter_lru_.pop_back();
        }
        nsx::DocFilter norm{r.from_text, r.to_text, r.keep_undated};
        uint32_t h = 0;
        if (!open_filter(norm, h, nullptr)) return nullptr;
        filter_lru_.push_front(FilterLruEnt{key, h});
        of = filter_of(h);
    }
    return of;
}

bool Engine::search_filtered_text(const std::string& query, int k, const nsx::DocFilter& f, std::string& body) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { body = err_ = "search_filtered: no device context: this engine has no CPU scoring path"; return false; }
    nsx::DateRange r;
    OpenFilter* of = lru_filter(f, r);
    if (!of) { body = err_; return false; }
    const int K = std::max(1, std::min(k, 100));
    const QueryView qv{query.data(), query.size()};
    std::vector<ns_hit> hits((size_t)K);
    uint32_t nh = 0;
    uint64_t fd = 0;
    uint8_t us = 0;
    if (!search_filtered_batch_flat(of->handle, &qv, 1, K, NS_FLAG_OR, hits.data(), &nh, &fd, &us)) { body = err_; return false; }
    SearchResult res;
    res.query = query;
    res.k = K;
    res.segments = (int)segments.size();
    res.has_found = us != 0;
    res.found = fd;
    if (res.has_found)
        for (uint32_t i = 0; i < nh; i++) res.hits.push_back(SearchHit{hits[i].score, hits[i].seg_id, hits[i].doc_id});
    // search's body with the "filter" member in front ("filter" < "found" < "k": nlohmann keeps keys sorted)
    std::string o = "{\n  \"filter\": {\n    \"date_from\": ";
    json_escape(o, r.from_text);
    o += ",\n    \"date_to\": ";
    json_escape(o, r.to_text);
    o += ",\n    \"documents\": " + std::to_string(of->docs_kept);
    o += std::string(",\n    \"keep_undated\": ") + (r.keep_undated ? "true" : "false") + "\n  },\n";
    body = o + to_json_impl(res).substr(2);
    return true;
}

std::string Engine::search_filtered(const std::string& query, int k, const nsx::DocFilter& f) {
    std::string body;
    return search_filtered_text(query, k, f, body) ? body : error_body(body);
}

// ---- facet counts (host/facet.hpp, csrc/ns_facet.hip) -------------------------------------------------------
void Engine::release_facets() {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    for (FacetSet& fs : facets_) {
        if (ctx_)
            for (ns_facet* t : fs.dev)
                if (t) (void)ns_facet_release(ctx_, t);
        fs = FacetSet{};
    }
}

size_t Engine::facet_tables_on_device() const {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    size_t n = 0;
    for (const FacetSet& fs : facets_)
        for (const ns_facet* t : fs.dev) n += t != nullptr;
    return n;
}

bool Engine::facet_buckets(const nsx::FacetSpec& spec, std::vector<std::vector<uint16_t>>& tables, std::vector<std::string>& labels) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    tables.clear();
    labels.clear();
    const size_t S = segments.size();
    if (spec.kind == nsx::FacetSpec::Custom) {
        const size_t B = spec.custom_labels.size();
        if (B < 1 || B > nsx::kMaxFacetBuckets) { err_ = "facet custom: " + std::to_string(B) + " labels; a facet has 1 to " + std::to_string(nsx::kMaxFacetBuckets) + " buckets"; return false; }
        if (spec.custom_buckets.size() != S) { err_ = "facet custom: " + std::to_string(spec.custom_buckets.size()) + " bucket arrays for " + std::to_string(S) + " segments"; return false; }
        for (size_t s = 0; s < S; s++) {
            if (spec.custom_buckets[s].size() != segments[s].N) {
                err_ = "facet custom: the bucket array of segment " + std::to_string(s) + " has " + std::to_string(spec.custom_buckets[s].size()) + " entries, the segment " + std::to_string(segments[s].N) + " documents";
                return false;
            }
            for (const uint16_t b : spec.custom_buckets[s])
                if (b >= B) { err_ = "facet custom: segment " + std::to_string(s) + " names bucket " + std::to_string(b) + " of " + std::to_string(B); return false; }
        }
        tables = spec.custom_buckets;
        labels = spec.custom_labels;
        return true;
    }
    if (spec.kind != nsx::FacetSpec::Year && spec.kind != nsx::FacetSpec::Month) { err_ = "facet: unknown kind"; return false; }
    std::vector<std::vector<uint32_t>> keys(S);
    for (uint32_t s = 0; s < S; s++) {
        keys[s].resize(segments[s].N);
        for (uint32_t d = 0; d < segments[s].N; d++) {
            const nsx::MetaFields* md = meta.get(s, d);   // nullptr: no metadata row = undated
            keys[s][d] = md ? nsx::date_key(md->publish_time) : 0u;
        }
    }
    return nsx::facet_from_keys(spec.kind, keys, tables, labels, err_);
}

// the kind's tables on the host and, for every segment with a device copy, on the device
bool Engine::ensure_facets(const nsx::FacetSpec& spec, FacetSet*& out) {
    if ((unsigned)spec.kind > 2u) { err_ = "facet: unknown kind"; return false; }
    FacetSet& fs = facets_[spec.kind];
    if (fs.built && spec.kind == nsx::FacetSpec::Custom && (fs.tables != spec.custom_buckets || fs.labels != spec.custom_labels)) {
        for (ns_facet* t : fs.dev) if (t) (void)ns_facet_release(ctx_, t);   // another custom facet takes the kind's place
        fs = FacetSet{};
    }
    if (!fs.built) {
        FacetSet fresh;
        if (!facet_buckets(spec, fresh.tables, fresh.labels)) return false;
        fresh.dev.assign(segments.size(), nullptr);
        for (uint32_t s = 0; s < segments.size(); s++) {
            if (!dev_segs_[s]) continue;
            const int rc = ns_facet_upload(ctx_, segments[s].N, fresh.tables[s].data(), (uint32_t)fresh.labels.size(), &fresh.dev[s]);
            if (rc != NS_OK) {
                err_ = std::string("ns_facet_upload: ") + ns_last_error(ctx_);
                for (ns_facet* t : fresh.dev) if (t) (void)ns_facet_release(ctx_, t);
                return false;
            }
        }
        fresh.built = true;
        fs = std::move(fresh);
    }
    out = &fs;
    return true;
}

// ---- what the facet, date-order, boolean and paged calls share ---------------------------------------------------------
// The filter under a handle (0: none) and its row source; false, with a message, for a stale handle.
bool Engine::filter_rows(const char* fn, uint32_t filter_handle, CallPrep& bp) {
    if (!filter_handle) return true;
    bp.f = filter_of(filter_handle);
    if (!bp.f) { err_ = std::string(fn) + ": handle " + std::to_string(filter_handle) + " is stale (the filter was closed, or the index was reloaded after it was opened)"; return false; }
    bp.rs.rows = bp.f->rows.data();   // search_filtered_batch_flat's row source
    bp.rs.id_base = (uint32_t)(filter_handle % kMaxFilters + 1) * (uint32_t)segments.size();
    static const nsx::TermSeg no_rows{nsx::kAbsent, 0u, 0.0f};
    if (!bp.rs.rows) bp.rs.rows = &no_rows;
    return true;
}

// The segments the refs can name, in manifest order: the index's own, or the filter's copies, without those `keep` refuses.
template <class Keep>
void Engine::list_segments(CallPrep& bp, Keep keep) {
    const uint32_t S = (uint32_t)segments.size();
    bp.is_listed.assign(S, 0);
    for (uint32_t s = 0; s < S; s++) {
        ns_seg* h = bp.f ? bp.f->segs[s] : dev_segs_[s];
        if (!h || !keep(s)) continue;
        bp.is_listed[s] = 1;
        bp.listed.push_back(s);
        bp.ids.push_back(bp.rs.id_base + s);
        bp.segs.push_back(h);
    }
}

bool Engine::boolean_prepare(const char* fn, uint32_t filter_handle, CallPrep& bp) {
    if (!filter_rows(fn, filter_handle, bp)) return false;
    list_segments(bp, [](uint32_t) { return true; });
    return true;
}

// The plain search's query preparation.  With embeddings loaded: the expansion of search_batch_flat for the whole batch up
// front, the expanded terms then go sub-batch by sub-batch (term_begin stays an index into the one refs array).  Without: one
// sub-batch at a time into the engine's kept buffers.
bool Engine::plain_prepare(const QueryView* queries, size_t Q, uint8_t* usable, const nsx::RowSource& rs, bool and_mode, PlainPrep& pp) {
    pp.whole = sem.enabled;
    if (!pp.whole) return true;
    std::vector<std::string> qs(Q);
    for (size_t q = 0; q < Q; q++) qs[q].assign(queries[q].p, queries[q].n);
    std::vector<nsx::WeightedTerms> expanded;
    if (!expand_queries(qs, expanded)) return false;
    pp.qd.assign(Q, ns_query_desc{0, 0});
    std::vector<uint8_t> us(Q, 0);
    build_refs_range(qs, 0, Q, pp.qd, pp.refs, us, &expanded, rs, and_mode);
    std::memcpy(usable, us.data(), Q);
    return true;
}

void Engine::plain_range(const QueryView* queries, size_t a, size_t b, uint8_t* usable, const nsx::RowSource& rs, bool and_mode, PlainPrep& pp) {
    if (!pp.whole) build_refs_parallel(queries, a, b, flat_qd_, flat_refs_, usable + a, rs, and_mode);
    pp.qd_at = pp.whole ? pp.qd.data() + a : flat_qd_.data();
    pp.refs_at = pp.whole ? pp.refs.data() : flat_refs_.data();
    pp.n_refs = pp.whole ? pp.refs.size() : flat_refs_.size();
}

// The sub-batch loop of every ranked call (score or date order, plain or boolean).  Per sub-batch [a, b): prep(a, b) prepares
// its queries; its cursors are translated; with nothing on the device, where no ref can exist, the outputs are filled; else
// call(a, b, cursors or nullptr, &ms) runs the device part, its time is added to the call's and the hits' segment ids become
// manifest positions again.  prep and call say false with err_ set.
template <class Prep, class Call>
bool Engine::ranked_batch(const char* fn, CallPrep& bp, const nsx::PageCursor* after, size_t Q, const RankedOut& out, Prep prep, Call call) {
    const size_t K = out.K;
    const ns_hit pad{-std::numeric_limits<float>::infinity(), 0xFFFFFFFFu, 0xFFFFFFFFu};
    return for_each_sub_batch(Q, [&](size_t a, size_t b) {
        if (!prep(a, b)) return false;
        if (!translate_cursors(fn, after, a, b, bp.rs.id_base, bp.is_listed, bp.f != nullptr, bp.cur)) return false;
        if (bp.ids.empty()) {
            std::fill(out.found + a, out.found + b, (uint64_t)0);
            if (out.rest) std::fill(out.rest + a, out.rest + b, (uint64_t)0);
            std::fill(out.nhits + a, out.nhits + b, 0u);
            std::fill(out.hits + a * K, out.hits + b * K, pad);
            if (out.keys) std::fill(out.keys + a * K, out.keys + b * K, 0u);
            return true;
        }
        float ms = 0.0f;
        if (!call(a, b, bp.cur.empty() ? nullptr : bp.cur.data(), &ms)) return false;
        if (out.device_ms) *out.device_ms += ms;
        for (size_t q = a; q < b; q++)
            for (uint32_t i = 0; i < out.nhits[q]; i++) out.hits[q * K + i].seg_id -= bp.rs.id_base;
        return true;
    });
}

bool Engine::facet_batch_flat(const nsx::FacetSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, uint32_t flags,
                              std::vector<uint32_t>& counts, uint64_t* found, uint8_t* usable, std::vector<std::string>& labels,
                              float* device_ms, double* count_ms) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    counts.clear();
    labels.clear();
    if (device_ms) *device_ms = 0.0f;
    if (count_ms) *count_ms = 0.0;
    if (!ctx_) { err_ = "facet_batch_flat: no device context: facets are counted on the device, there is no CPU path"; return false; }
    if (Q && (!queries || !found || !usable)) { err_ = "facet_batch_flat: null argument"; return false; }
    CallPrep bp;
    if (!filter_rows("facet_batch_flat", filter_handle, bp)) return false;
    FacetSet* fs = nullptr;
    if (!ensure_facets(spec, fs)) return false;
    labels = fs->labels;
    const size_t B = labels.size();
    counts.assign(Q * B, 0u);
    if (Q == 0) return true;
    const bool and_mode = (flags & NS_FLAG_AND) != 0;
    // the segments the refs can name: the index's own, or the filter's copies, each with its position's table
    list_segments(bp, [&](uint32_t s) { return fs->dev[s] != nullptr; });
    std::vector<ns_facet*> tabs;
    for (const uint32_t s : bp.listed) tabs.push_back(fs->dev[s]);
    PlainPrep pp;
    if (!plain_prepare(queries, Q, usable, bp.rs, and_mode, pp)) return false;
    return for_each_sub_batch(Q, [&](size_t a, size_t b) {
        plain_range(queries, a, b, usable, bp.rs, and_mode, pp);
        if (bp.ids.empty()) {   // nothing on the device: no ref can exist
            std::fill(found + a, found + b, (uint64_t)0);
            return true;
        }
        float ms = 0.0f;
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = ns_facet_count(ctx_, pp.qd_at, (uint32_t)(b - a), pp.refs_at, (uint32_t)pp.n_refs, flags, bp.ids.data(), bp.segs.data(), tabs.data(),
                                      (uint32_t)bp.ids.size(), counts.data() + a * B, found + a, &ms);
        if (rc != NS_OK) { err_ = std::string("ns_facet_count: ") + ns_last_error(ctx_); return false; }
        if (device_ms) *device_ms += ms;
        if (count_ms) *count_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return true;
    });
}

// the "facets" member of search_faceted's body, with the comma and newline behind it
static std::string facets_member(const nsx::FacetSpec& spec, const std::vector<std::string>& labels, const std::vector<uint32_t>& counts) {
    std::string o = "  \"facets\": {\n    ";
    json_escape(o, nsx::facet_kind_name(spec.kind));
    o += ": [";
    bool first = true;
    for (size_t b = 0; b < labels.size(); b++) {
        if (!counts[b]) continue;
        o += first ? "\n" : ",\n";
        first = false;
        o += "      {\n        \"count\": " + std::to_string(counts[b]) + ",\n        \"value\": ";
        json_escape(o, labels[b]);
        o += "\n      }";
    }
    o += first ? "]\n  },\n" : "\n    ]\n  },\n";
    return o;
}

bool Engine::search_faceted_text(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f, std::string& body) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { body = err_ = "search_faceted: no device context: this engine has no CPU scoring path"; return false; }
    uint32_t handle = 0;
    if (f) {   // search_filtered's body; its filter is then the most recently used of the cache
        if (!search_filtered_text(query, k, *f, body)) return false;
        handle = filter_lru_.front().handle;
    } else {
        SearchResult r;
        if (!search_hits_locked(query, k, NS_FLAG_OR, r)) { body = err_; return false; }
        body = to_json_impl(r);
    }
    const QueryView qv{query.data(), query.size()};
    std::vector<uint32_t> counts;
    std::vector<std::string> labels;
    uint64_t fd = 0;
    uint8_t us = 0;
    if (!facet_batch_flat(spec, handle, &qv, 1, NS_FLAG_OR, counts, &fd, &us, labels)) { body = err_; return false; }
    // the "facets" member in front ("facets" < "filter" < "found" < "k": nlohmann keeps keys sorted)
    body = "{\n" + facets_member(spec, labels, counts) + body.substr(2);
    return true;
}

std::string Engine::search_faceted(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f) {
    std::string body;
    return search_faceted_text(query, k, spec, f, body) ? body : error_body(body);
}

// ---- search sorted by date (host/sorted.hpp, csrc/ns_sorted.hip) --------------------------------------------
void Engine::release_sorted() {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    for (SortSet& ss : sorts_) {
        if (ctx_)
            for (ns_dockeys* t : ss.dev)
                if (t) (void)ns_dockeys_release(ctx_, t);
        ss = SortSet{};
    }
}

size_t Engine::sort_tables_on_device() const {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    size_t n = 0;
    for (const SortSet& ss : sorts_)
        for (const ns_dockeys* t : ss.dev) n += t != nullptr;
    return n;
}

bool Engine::sort_keys(const nsx::SortSpec& spec, std::vector<std::vector<uint32_t>>& keys) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    keys.clear();
    const size_t S = segments.size();
    if (spec.kind == nsx::SortSpec::Custom) {
        if (spec.custom_keys.size() != S) { err_ = "sort custom: " + std::to_string(spec.custom_keys.size()) + " key arrays for " + std::to_string(S) + " segments"; return false; }
        for (size_t s = 0; s < S; s++) {
            if (spec.custom_keys[s].size() != segments[s].N) {
                err_ = "sort custom: the key array of segment " + std::to_string(s) + " has " + std::to_string(spec.custom_keys[s].size()) + " entries, the segment " + std::to_string(segments[s].N) + " documents";
                return false;
            }
            for (const uint32_t k : spec.custom_keys[s])
                if (k == nsx::kSortReservedKey) { err_ = "sort custom: segment " + std::to_string(s) + " holds the reserved key 0xFFFFFFFF"; return false; }
        }
        keys = spec.custom_keys;
        return true;
    }
    if (spec.kind != nsx::SortSpec::Date) { err_ = "sort: unknown kind"; return false; }
    keys.resize(S);
    for (uint32_t s = 0; s < S; s++) {
        keys[s].resize(segments[s].N);
        for (uint32_t d = 0; d < segments[s].N; d++) {
            const nsx::MetaFields* md = meta.get(s, d);   // nullptr: no metadata row = undated
            keys[s][d] = md ? nsx::date_key(md->publish_time) : 0u;
        }
    }
    return true;
}

// the kind's keys on the host and, for every segment with a device copy, on the device
bool Engine::ensure_sorted(const nsx::SortSpec& spec, SortSet*& out) {
    if ((unsigned)spec.kind > 1u) { err_ = "sort: unknown kind"; return false; }
    SortSet& ss = sorts_[spec.kind];
    if (ss.built && spec.kind == nsx::SortSpec::Custom && ss.keys != spec.custom_keys) {
        for (ns_dockeys* t : ss.dev) if (t) (void)ns_dockeys_release(ctx_, t);   // another custom order takes the kind's place
        ss = SortSet{};
    }
    if (!ss.built) {
        SortSet fresh;
        if (!sort_keys(spec, fresh.keys)) return false;
        fresh.dev.assign(segments.size(), nullptr);
        for (uint32_t s = 0; s < segments.size(); s++) {
            if (!dev_segs_[s]) continue;
            const int rc = ns_dockeys_upload(ctx_, segments[s].N, fresh.keys[s].data(), &fresh.dev[s]);
            if (rc != NS_OK) {
                err_ = std::string("ns_dockeys_upload: ") + ns_last_error(ctx_);
                for (ns_dockeys* t : fresh.dev) if (t) (void)ns_dockeys_release(ctx_, t);
                return false;
            }
        }
        fresh.built = true;
        ss = std::move(fresh);
    }
    out = &ss;
    return true;
}

bool Engine::search_sorted_batch_flat(const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k, uint32_t flags,
                                      ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint8_t* usable, float* device_ms) {
    return sorted_batch_impl("search_sorted_batch_flat", spec, filter_handle, queries, Q, k, flags, nullptr, hits, keys, nhits, found, nullptr, usable, device_ms);
}

bool Engine::search_sorted_after_batch_flat(const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k, uint32_t flags,
                                            const nsx::PageCursor* after, ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                            uint8_t* usable, float* device_ms) {
    return sorted_batch_impl("search_sorted_after_batch_flat", spec, filter_handle, queries, Q, k, flags, after, hits, keys, nhits, found, rest, usable, device_ms);
}

// Pages past the first K (host/page.hpp): the cursors of queries [a, b), which name manifest positions, as the
// call's ns_cursors, which name the ids the refs use (under a filter: the filter copies').  listed[s]: position s is in the
// call's segment list.
bool Engine::translate_cursors(const char* fn, const nsx::PageCursor* after, size_t a, size_t b, uint32_t id_base, const std::vector<uint8_t>& listed,
                               bool filtered, std::vector<ns_cursor>& out) {
    out.clear();
    if (!after) return true;
    bool any = false;
    for (size_t q = a; q < b; q++) any = any || after[q].set;
    if (!any) return true;
    out.assign(b - a, ns_cursor{0u, 0u, 0u, 0u});
    for (size_t q = a; q < b; q++) {
        const nsx::PageCursor& c = after[q];
        if (!c.set) continue;
        if (c.seg >= listed.size()) {
            err_ = std::string(fn) + ": the cursor of query " + std::to_string(q) + " names position " + std::to_string(c.seg) + ", the index has " + std::to_string(listed.size()) + " segments";
            return false;
        }
        if (!listed[c.seg]) {
            err_ = std::string(fn) + ": the cursor of query " + std::to_string(q) + " names position " + std::to_string(c.seg) +
                   (filtered ? ", of which the filter keeps nothing" : ", which has no copy on the device");
            return false;
        }
        out[q - a] = ns_cursor{c.rank, id_base + c.seg, c.doc, 1u};
    }
    return true;
}

bool Engine::sorted_batch_impl(const char* fn, const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k, uint32_t flags,
                               const nsx::PageCursor* after, ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable,
                               float* device_ms) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (device_ms) *device_ms = 0.0f;
    if (!ctx_) { err_ = std::string(fn) + ": no device context: the sorted search runs on the device, there is no CPU path"; return false; }
    if (Q && (!queries || !hits || !keys || !nhits || !found || !usable)) { err_ = std::string(fn) + ": null argument"; return false; }
    if (flags & ~(uint32_t)NS_FLAG_AND) { err_ = std::string(fn) + ": flags are NS_FLAG_OR or NS_FLAG_AND; the direction is the spec's"; return false; }
    CallPrep bp;
    if (!filter_rows(fn, filter_handle, bp)) return false;
    SortSet* ss = nullptr;
    if (!ensure_sorted(spec, ss)) return false;
    if (Q == 0) return true;
    const bool and_mode = (flags & NS_FLAG_AND) != 0;
    const uint32_t call_flags = flags | (spec.ascending ? NS_SORT_ASC : NS_SORT_DESC);
    // each listed position with its keys; one without a key table is skipped (search_dialect_sorted_batch_flat refuses it)
    list_segments(bp, [&](uint32_t s) { return ss->dev[s] != nullptr; });
    std::vector<ns_dockeys*> tabs;
    for (const uint32_t s : bp.listed) tabs.push_back(ss->dev[s]);
    const RankedOut out{(size_t)std::max(1, std::min(k, 100)), hits, keys, nhits, found, rest, device_ms};
    PlainPrep pp;
    if (!plain_prepare(queries, Q, usable, bp.rs, and_mode, pp)) return false;
    return ranked_batch(fn, bp, after, Q, out,
        [&](size_t a, size_t b) { plain_range(queries, a, b, usable, bp.rs, and_mode, pp); return true; },
        [&](size_t a, size_t b, const ns_cursor* cur, float* ms) {
            const int rc = ns_search_sorted_after(ctx_, pp.qd_at, (uint32_t)(b - a), pp.refs_at, (uint32_t)pp.n_refs, (uint32_t)out.K, call_flags, cur, bp.ids.data(),
                                                  bp.segs.data(), tabs.data(), (uint32_t)bp.ids.size(), hits + a * out.K, keys + a * out.K, nhits + a, found + a,
                                                  rest ? rest + a : nullptr, ms);
            if (rc != NS_OK) { err_ = std::string(after ? "ns_search_sorted_after: " : "ns_search_sorted: ") + ns_last_error(ctx_); return false; }
            return true;
        });
}

bool Engine::search_sorted_text(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f, std::string& body) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { body = err_ = "search_sorted: no device context: this engine has no CPU scoring path"; return false; }
    uint32_t handle = 0;
    if (f) {   // search_filtered's body; its filter is then the most recently used of the cache
        if (!search_filtered_text(query, k, *f, body)) return false;
        handle = filter_lru_.front().handle;
    } else {
        SearchResult r;
        if (!search_hits_locked(query, k, NS_FLAG_OR, r)) { body = err_; return false; }
        body = to_json_impl(r);
    }
    const size_t K = (size_t)std::max(1, std::min(k, 100));
    const QueryView qv{query.data(), query.size()};
    std::vector<ns_hit> hits(K);
    std::vector<uint32_t> keys(K);
    uint32_t nh = 0;
    uint64_t fd = 0;
    uint8_t us = 0;
    if (!search_sorted_batch_flat(spec, handle, &qv, 1, (int)K, NS_FLAG_OR, hits.data(), keys.data(), &nh, &fd, &us)) { body = err_; return false; }
    std::vector<SearchHit> sorted;
    if (us)
        for (uint32_t i = 0; i < nh; i++) sorted.push_back(SearchHit{hits[i].score, hits[i].seg_id, hits[i].doc_id});
    // the body's "results" member replaced ("query" is escaped: no line of it starts like a member), "sort" behind "segments"
    const size_t a = body.find("\n  \"results\": "), b = body.rfind("\n  \"segments\": ");
    if (a == std::string::npos || b == std::string::npos || b < a || body.size() < 2) { body = err_ = "search_sorted: the search body has no results member"; return false; }
    std::string o = body.substr(0, a + 1);
    append_results_json(o, sorted);
    o += body.substr(b + 1, body.size() - (b + 1) - 2);   // "  \"segments\": N", without the closing "\n}"
    o += ",\n  \"sort\": ";
    json_escape(o, nsx::sort_name(spec));
    o += "\n}";
    body = std::move(o);
    return true;
}

std::string Engine::search_sorted(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f) {
    std::string body;
    return search_sorted_text(query, k, spec, f, body) ? body : error_body(body);
}

// ---- boolean queries and their dialects (host/boolean.hpp, grouped.hpp, quorum.hpp) --
// what the dialect forms call themselves in messages: the named methods of engine.hpp
struct DialectNames { const char *first_page, *after_batch, *facet_batch, *sorted_batch, *text, *faceted_text, *sorted_text; };
static const DialectNames& names_of(nsx::Dialect d) {
    static const DialectNames kNames[5] = {
        {"search_boolean_batch_flat", "search_boolean_after_batch_flat", "facet_boolean_batch_flat", "search_boolean_sorted_batch_flat", "search_boolean",
         "search_boolean_faceted", "search_boolean_sorted"},
        {"search_grouped_after_batch_flat", "search_grouped_after_batch_flat", "facet_grouped_batch_flat", "search_grouped_sorted_batch_flat", "search_grouped",
         "search_grouped_faceted", "search_grouped_sorted"},
        {"search_quorum_after_batch_flat", "search_quorum_after_batch_flat", "facet_quorum_batch_flat", "search_quorum_sorted_batch_flat", "search_quorum",
         "search_quorum_faceted", "search_quorum_sorted"},
        {"search_boosted_after_batch_flat", "search_boosted_after_batch_flat", "facet_boosted_batch_flat", "search_boosted_sorted_batch_flat", "search_boosted",
         "search_boosted_faceted", "search_boosted_sorted"},   // (Boosted has the ranked call alone: DESIGN.md §5z, left out)
        {"search_prefixed_after_batch_flat", "search_prefixed_after_batch_flat", "facet_prefixed_batch_flat", "search_prefixed_sorted_batch_flat", "search_prefixed",
         "search_prefixed_faceted", "search_prefixed_sorted"}};   // (Prefixed too: §5ab, left out)
    return kNames[(int)d];
}

// Descriptors, refs and roles of the queries [a, b) in the dialect's grammar.  A MUST term gets a ref in every listed segment,
// with count == 0 where the segment has no list of it: nothing of the segment matches a lone term, and a clause loses a
// member.  Grouped adds the clause id of every ref, Quorum its need too: an unknown member is dropped and the need stays.
// False, with a message, when a Grouped or Quorum query has more clauses than a clause value can name, or a Quorum query asks
// for more than kQuorumMaxNeed of a clause's terms.  Boolean never fails.
bool Engine::refs_range(const char* fn, nsx::Dialect dialect, const QueryView* queries, size_t a, size_t b, uint8_t* usable, CallPrep& bp) {
    const bool with_clauses = dialect != nsx::Dialect::Boolean,
               with_needs = dialect == nsx::Dialect::Quorum || dialect == nsx::Dialect::Boosted || dialect == nsx::Dialect::Prefixed;
    const uint32_t S = (uint32_t)segments.size();
    float weight = 1.0f;   // Boosted: the `^w` of the piece the scanner is in; else 1.0f
    bool star = false;     // Prefixed: the term the scanner hands over is a prefix
    // Prefixed: a term's row is one of the call's own (bp.px), which bp.rs.rows holds: a prefix's, or the dictionary term's there
    auto local_row = [&](const char* p, size_t n) -> int64_t {
        if (star) { const auto it = bp.px->of_prefix.find(std::string(p, n)); return it == bp.px->of_prefix.end() ? -1 : (int64_t)it->second; }
        const int64_t gid = dict.find(p, n);
        if (gid < 0) return -1;
        const auto it = bp.px->of_term.find((uint32_t)gid);
        return it == bp.px->of_term.end() ? -1 : (int64_t)it->second;
    };
    const nsx::RowSource& rs = bp.rs;
    bp.qd.assign(b - a, ns_query_desc{0, 0});
    bp.refs.clear();
    bp.roles.clear();
    bp.clauses.clear();
    bp.needs.clear();
    for (size_t q = a; q < b; q++) {
        bp.terms.clear();
        size_t positive = 0;
        uint32_t largest = 0;
        const nsx::QuorumShape shape = nsx::for_each_term(dialect, queries[q].p, queries[q].n, bp.scratch, [&](const char* p, size_t n, uint8_t role, uint32_t clause, uint32_t need) {
            bp.terms.push_back(CallPrep::Term{bp.px ? local_row(p, n) : dict.find(p, n), role, clause, need, weight});
            positive += role != nsx::kRoleNot;
            largest = std::max(largest, need);
        }, &weight, &star);
        uint32_t n_clauses = shape.n_clauses;
        if (shape.min_should) {   // `~m`: every optional term joins one more required clause of need m
            bool any = false;
            for (CallPrep::Term& t : bp.terms)
                if (t.role == nsx::kRoleShould) {
                    t = CallPrep::Term{t.row, nsx::kRoleMust, shape.n_clauses, shape.min_should, t.weight};
                    any = true;
                }
            if (any) n_clauses++;
            largest = std::max(largest, shape.min_should);   // refused above the limit whether or not a term is there to promote
        }
        if (with_clauses && n_clauses > 65535u) { err_ = std::string(fn) + ": query " + std::to_string(q) + " has " + std::to_string(n_clauses) + " required clauses (at most 65535)"; return false; }
        if (with_needs && largest > nsx::kQuorumMaxNeed) {
            err_ = std::string(fn) + ": query " + std::to_string(q) + " asks for " + std::to_string(largest) + " of a clause's terms (at most " + std::to_string(nsx::kQuorumMaxNeed) + ")";
            return false;
        }
        bp.qd[q - a].term_begin = (uint32_t)bp.refs.size();
        usable[q] = (positive != 0 && S != 0) ? 1 : 0;
        if (!usable[q]) continue;
        for (const uint32_t sid : bp.listed)
            for (const CallPrep::Term& t : bp.terms) {
                const nsx::TermSeg* e = t.row < 0 ? nullptr : rs.rows ? &rs.rows[(size_t)t.row * S + sid] : &dict.row((uint32_t)t.row)[sid];
                if (e && e->byte_off != nsx::kAbsent) bp.refs.push_back(ns_term_ref{rs.id_base + sid, e->count, e->byte_off, e->idf, t.weight});
                else if (t.role == nsx::kRoleMust) bp.refs.push_back(ns_term_ref{rs.id_base + sid, 0u, 0u, 0.0f, 1.0f});   // an absent member of its clause
                else continue;
                bp.roles.push_back(t.role);
                if (with_clauses) bp.clauses.push_back((uint16_t)t.clause);
                if (with_needs) bp.needs.push_back((uint8_t)t.need);
            }
        bp.qd[q - a].term_count = (uint32_t)bp.refs.size() - bp.qd[q - a].term_begin;
    }
    return true;
}

// The device calls by dialect.  The boolean call receives no clauses and the grouped call no needs: those NULLs select the
// kernels (§5w: the QUORUM instantiations are 5-7 % slower), and each dialect keeps its C entry point and so its messages.
bool Engine::ranked_call(nsx::Dialect dialect, bool paged, const CallPrep& bp, size_t a, size_t b, const RankedOut& out, const ns_cursor* cur, float* ms) {
    const uint32_t nq = (uint32_t)(b - a), n_refs = (uint32_t)bp.refs.size(), n_segs = (uint32_t)bp.ids.size(), K = (uint32_t)out.K;
    ns_hit* hits = out.hits + a * out.K;
    uint64_t* rest = out.rest ? out.rest + a : nullptr;
    const char* name = nullptr;
    int rc = NS_OK;
    switch (dialect) {
        case nsx::Dialect::Boolean:
            name = paged ? "ns_search_boolean_after: " : "ns_search_boolean: ";
            rc = ns_search_boolean_after(ctx_, bp.qd.data(), nq, bp.refs.data(), bp.roles.data(), n_refs, K, cur, bp.ids.data(), bp.segs.data(), n_segs, hits, out.nhits + a,
                                         out.found + a, rest, ms);
            break;
        case nsx::Dialect::Grouped:
            name = "ns_search_grouped_after: ";
            rc = ns_search_grouped_after(ctx_, bp.qd.data(), nq, bp.refs.data(), bp.roles.data(), bp.clauses.data(), n_refs, K, cur, bp.ids.data(), bp.segs.data(), n_segs,
                                         hits, out.nhits + a, out.found + a, rest, ms);
            break;
        case nsx::Dialect::Quorum:
            name = "ns_search_quorum_after: ";
            rc = ns_search_quorum_after(ctx_, bp.qd.data(), nq, bp.refs.data(), bp.roles.data(), bp.clauses.data(), bp.needs.data(), n_refs, K, cur, bp.ids.data(),
                                        bp.segs.data(), n_segs, hits, out.nhits + a, out.found + a, rest, ms);
            break;
        case nsx::Dialect::Boosted:   // without tables (term weights only) the call is the quorum call, kernels and all
        case nsx::Dialect::Prefixed:  // the Boosted call over the derived segments
            name = "ns_search_boosted_after: ";
            rc = ns_search_boosted_after(ctx_, bp.qd.data(), nq, bp.refs.data(), bp.roles.data(), bp.clauses.data(), bp.needs.data(), n_refs, K, cur, bp.ids.data(),
                                         bp.segs.data(), bp.boosts.empty() ? nullptr : bp.boosts.data(), n_segs, hits, out.nhits + a, out.found + a, rest, ms);
            break;
    }
    if (rc != NS_OK) { err_ = std::string(name) + ns_last_error(ctx_); return false; }
    return true;
}

bool Engine::facet_call(nsx::Dialect dialect, const CallPrep& bp, size_t a, size_t b, ns_facet* const* tabs, uint32_t* counts, uint64_t* found, float* ms) {
    const uint32_t nq = (uint32_t)(b - a), n_refs = (uint32_t)bp.refs.size(), n_segs = (uint32_t)bp.ids.size();
    const char* name = nullptr;
    int rc = NS_OK;
    switch (dialect) {
        case nsx::Dialect::Boolean:
            name = "ns_facet_count_boolean: ";
            rc = ns_facet_count_boolean(ctx_, bp.qd.data(), nq, bp.refs.data(), bp.roles.data(), n_refs, bp.ids.data(), bp.segs.data(), tabs, n_segs, counts, found, ms);
            break;
        case nsx::Dialect::Grouped:
            name = "ns_facet_count_grouped: ";
            rc = ns_facet_count_grouped(ctx_, bp.qd.data(), nq, bp.refs.data(), bp.roles.data(), bp.clauses.data(), n_refs, bp.ids.data(), bp.segs.data(), tabs, n_segs, counts,
                                        found, ms);
            break;
        case nsx::Dialect::Quorum:
            name = "ns_facet_count_quorum: ";
            rc = ns_facet_count_quorum(ctx_, bp.qd.data(), nq, bp.refs.data(), bp.roles.data(), bp.clauses.data(), bp.needs.data(), n_refs, bp.ids.data(), bp.segs.data(), tabs,
                                       n_segs, counts, found, ms);
            break;
        case nsx::Dialect::Boosted: err_ = "facet counts do not depend on a score: use the quorum call"; return false;
        case nsx::Dialect::Prefixed: err_ = "facet counts for prefixed queries are not built (DESIGN.md §5ab, left out)"; return false;
    }
    if (rc != NS_OK) { err_ = std::string(name) + ns_last_error(ctx_); return false; }
    return true;
}

bool Engine::sorted_call(nsx::Dialect dialect, const CallPrep& bp, size_t a, size_t b, uint32_t direction, ns_dockeys* const* tabs, const RankedOut& out,
                         const ns_cursor* cur, float* ms) {
    const uint32_t nq = (uint32_t)(b - a), n_refs = (uint32_t)bp.refs.size(), n_segs = (uint32_t)bp.ids.size(), K = (uint32_t)out.K;
    ns_hit* hits = out.hits + a * out.K;
    uint32_t* keys = out.keys + a * out.K;
    uint64_t* rest = out.rest ? out.rest + a : nullptr;
    const char* name = nullptr;
    int rc = NS_OK;
    switch (dialect) {
        case nsx::Dialect::Boolean:
            name = "ns_search_sorted_boolean: ";
            rc = ns_search_sorted_boolean(ctx_, bp.qd.data(), nq, bp.refs.data(), bp.roles.data(), n_refs, K, direction, cur, bp.ids.data(), bp.segs.data(), tabs, n_segs, hits,
                                          keys, out.nhits + a, out.found + a, rest, ms);
            break;
        case nsx::Dialect::Grouped:
            name = "ns_search_sorted_grouped: ";
            rc = ns_search_sorted_grouped(ctx_, bp.qd.data(), nq, bp.refs.data(), bp.roles.data(), bp.clauses.data(), n_refs, K, direction, cur, bp.ids.data(), bp.segs.data(),
                                          tabs, n_segs, hits, keys, out.nhits + a, out.found + a, rest, ms);
            break;
        case nsx::Dialect::Quorum:
            name = "ns_search_sorted_quorum: ";
            rc = ns_search_sorted_quorum(ctx_, bp.qd.data(), nq, bp.refs.data(), bp.roles.data(), bp.clauses.data(), bp.needs.data(), n_refs, K, direction, cur, bp.ids.data(),
                                         bp.segs.data(), tabs, n_segs, hits, keys, out.nhits + a, out.found + a, rest, ms);
            break;
        case nsx::Dialect::Boosted: err_ = "date order does not depend on a score: use the quorum call"; return false;
        case nsx::Dialect::Prefixed: err_ = "date order for prefixed queries is not built (DESIGN.md §5ab, left out)"; return false;
    }
    if (rc != NS_OK) { err_ = std::string(name) + ns_last_error(ctx_); return false; }
    return true;
}

bool Engine::boolean_batch_impl(const char* fn, nsx::Dialect dialect, uint32_t filter_handle, const QueryView* queries, size_t Q, int k, const nsx::PageCursor* after,
                                ns_hit* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms, const nsx::BoostSpec* boost) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (device_ms) *device_ms = 0.0f;
    if (!ctx_) { err_ = std::string(fn) + ": no device context: boolean queries run on the device, there is no CPU path"; return false; }
    if (Q && (!queries || !hits || !nhits || !found || !usable)) { err_ = std::string(fn) + ": null argument"; return false; }
    CallPrep bp;
    if (!boolean_prepare(fn, filter_handle, bp)) return false;
    if (boost && dialect == nsx::Dialect::Boosted) {   // the factor tables of the listed segments (a filter's copies keep the docIds)
        BoostSet* bs = nullptr;
        if (!ensure_boosts(*boost, bs)) { err_ = std::string(fn) + ": " + err_; return false; }
        for (const uint32_t s : bp.listed) bp.boosts.push_back(bs->dev[s]);
    }
    if (Q == 0) return true;
    const RankedOut out{(size_t)std::max(1, std::min(k, 100)), hits, nullptr, nhits, found, rest, device_ms};
    return ranked_batch(fn, bp, after, Q, out,
        [&](size_t a, size_t b) { return refs_range(fn, dialect, queries, a, b, usable, bp); },
        [&](size_t a, size_t b, const ns_cursor* cur, float* ms) { return ranked_call(dialect, after != nullptr, bp, a, b, out, cur, ms); });
}

bool Engine::search_dialect_after_batch_flat(nsx::Dialect dialect, uint32_t filter_handle, const QueryView* queries, size_t Q, int k, const nsx::PageCursor* after,
                                             ns_hit* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms, const nsx::BoostSpec* boost) {
    if (dialect == nsx::Dialect::Prefixed)   // its own call: the derived segments (the default PrefixSpec)
        return search_prefixed_after_batch_flat(boost, nsx::PrefixSpec{}, filter_handle, queries, Q, k, after, hits, nhits, found, rest, usable, device_ms);
    return boolean_batch_impl(names_of(dialect).after_batch, dialect, filter_handle, queries, Q, k, after, hits, nhits, found, rest, usable, device_ms, boost);
}

bool Engine::facet_dialect_batch_flat(nsx::Dialect dialect, const nsx::FacetSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q,
                                      std::vector<uint32_t>& counts, uint64_t* found, uint8_t* usable, std::vector<std::string>& labels, float* device_ms) {
    const char* fn = names_of(dialect).facet_batch;
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    counts.clear();
    labels.clear();
    if (device_ms) *device_ms = 0.0f;
    if (!ctx_) { err_ = std::string(fn) + ": no device context: facets are counted on the device, there is no CPU path"; return false; }
    if (Q && (!queries || !found || !usable)) { err_ = std::string(fn) + ": null argument"; return false; }
    CallPrep bp;
    if (!boolean_prepare(fn, filter_handle, bp)) return false;
    FacetSet* fs = nullptr;
    if (!ensure_facets(spec, fs)) return false;
    labels = fs->labels;
    const size_t B = labels.size();
    counts.assign(Q * B, 0u);
    if (Q == 0) return true;
    std::vector<ns_facet*> tabs;
    for (const uint32_t s : bp.listed) {
        if (!fs->dev[s]) { err_ = std::string(fn) + ": segment " + std::to_string(s) + " has no bucket table on the device"; return false; }
        tabs.push_back(fs->dev[s]);
    }
    return for_each_sub_batch(Q, [&](size_t a, size_t b) {
        if (!refs_range(fn, dialect, queries, a, b, usable, bp)) return false;
        if (bp.ids.empty()) {   // nothing on the device: no ref can exist
            std::fill(found + a, found + b, (uint64_t)0);
            return true;
        }
        float ms = 0.0f;
        if (!facet_call(dialect, bp, a, b, tabs.data(), counts.data() + a * B, found + a, &ms)) return false;
        if (device_ms) *device_ms += ms;
        return true;
    });
}

bool Engine::search_dialect_sorted_batch_flat(nsx::Dialect dialect, const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k,
                                              const nsx::PageCursor* after, ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                              uint8_t* usable, float* device_ms) {
    const char* fn = names_of(dialect).sorted_batch;
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (device_ms) *device_ms = 0.0f;
    if (!ctx_) { err_ = std::string(fn) + ": no device context: the sorted search runs on the device, there is no CPU path"; return false; }
    if (Q && (!queries || !hits || !keys || !nhits || !found || !usable)) { err_ = std::string(fn) + ": null argument"; return false; }
    CallPrep bp;
    if (!boolean_prepare(fn, filter_handle, bp)) return false;
    SortSet* ss = nullptr;
    if (!ensure_sorted(spec, ss)) return false;
    if (Q == 0) return true;
    std::vector<ns_dockeys*> tabs;
    for (const uint32_t s : bp.listed) {
        if (!ss->dev[s]) { err_ = std::string(fn) + ": segment " + std::to_string(s) + " has no key table on the device"; return false; }
        tabs.push_back(ss->dev[s]);
    }
    const RankedOut out{(size_t)std::max(1, std::min(k, 100)), hits, keys, nhits, found, rest, device_ms};
    const uint32_t direction = spec.ascending ? NS_SORT_ASC : NS_SORT_DESC;
    return ranked_batch(fn, bp, after, Q, out,
        [&](size_t a, size_t b) { return refs_range(fn, dialect, queries, a, b, usable, bp); },
        [&](size_t a, size_t b, const ns_cursor* cur, float* ms) { return sorted_call(dialect, bp, a, b, direction, tabs.data(), out, cur, ms); });
}

// one `"name": [strings]` member of a dialect's member, four spaces in: the texts of the terms that `in` keeps, in query order
template <class T, class In>
static void append_term_list(std::string& o, const char* name, const std::vector<T>& terms, In in, bool last) {
    o += std::string("    \"") + name + "\": [";
    bool any = false;
    for (const T& t : terms)
        if (in(t)) {
            o += any ? ",\n      " : "\n      ";
            json_escape(o, t.text);
            any = true;
        }
    o += any ? "\n    ]" : "]";
    o += last ? "\n" : ",\n";
}

// the "boolean" member of search_boolean's body (the parsed terms by role, in query order), with the comma and newline behind it
static std::string boolean_member(const std::string& query) {
    const std::vector<nsx::BoolTerm> terms = nsx::parse_boolean(query);
    std::string o = "  \"boolean\": {\n";
    append_term_list(o, "must", terms, [](const nsx::BoolTerm& t) { return t.role == nsx::kRoleMust; }, false);
    append_term_list(o, "must_not", terms, [](const nsx::BoolTerm& t) { return t.role == nsx::kRoleNot; }, false);
    append_term_list(o, "should", terms, [](const nsx::BoolTerm& t) { return t.role == nsx::kRoleShould; }, true);
    o += "  },\n";
    return o;
}

// the "grouped" member of search_grouped's body (§5u), which search_boolean's "boolean" member becomes: "must" is a list of clauses,
// each the list of its terms, in query order; "must_not" and "should" as in boolean_member.  nlohmann keeps keys sorted, so the
// member stands between "found" and "k" (grouped_insert), where "boolean" is the body's first.
static std::string grouped_member(const std::string& query) {
    const std::vector<nsx::GroupedTerm> terms = nsx::parse_grouped(query);
    std::string o = "  \"grouped\": {\n    \"must\": [";
    bool any_clause = false;
    for (size_t i = 0; i < terms.size(); i++) {
        if (terms[i].role != nsx::kRoleMust) continue;
        bool first_of_clause = true;
        for (size_t j = 0; j < i; j++) first_of_clause = first_of_clause && !(terms[j].role == nsx::kRoleMust && terms[j].clause == terms[i].clause);
        if (!first_of_clause) continue;
        o += any_clause ? ",\n      [" : "\n      [";
        bool any = false;
        for (size_t j = i; j < terms.size(); j++)
            if (terms[j].role == nsx::kRoleMust && terms[j].clause == terms[i].clause) {
                o += any ? ",\n        " : "\n        ";
                json_escape(o, terms[j].text);
                any = true;
            }
        o += "\n      ]";
        any_clause = true;
    }
    o += any_clause ? "\n    ],\n" : "],\n";
    append_term_list(o, "must_not", terms, [](const nsx::GroupedTerm& t) { return t.role == nsx::kRoleNot; }, false);
    append_term_list(o, "should", terms, [](const nsx::GroupedTerm& t) { return t.role == nsx::kRoleShould; }, true);
    o += "  },\n";
    return o;
}

// tail: to_json_impl's members from "found" (when usable) or "k" on; "found" is a number and "query" comes behind "k", so the first
// line that starts like the "k" member is it
static bool grouped_insert(std::string& tail, const std::string& query) {
    size_t at = tail.compare(0, 7, "  \"k\": ") == 0 ? 0 : tail.find("\n  \"k\": ");
    if (at == std::string::npos) return false;
    if (at) at++;
    tail.insert(at, grouped_member(query));
    return true;
}

// the "quorum" member of search_quorum's body (§5w): "min_should" is the `~m` piece's m (0: none); "must" lists the clauses, each
// {"need": n, "terms": [...]}, in query order, WITHOUT the clause the `~m` piece made: its terms stay under "should", where
// "min_should" says how many of them a document must hold.  "query" < "quorum" < "results": the member stands behind "query".
static std::string quorum_member(const std::string& query) {
    uint32_t min_should = 0;
    const std::vector<nsx::QuorumTerm> terms = nsx::parse_quorum(query, &min_should);
    std::string o = "  \"quorum\": {\n    \"min_should\": " + std::to_string(min_should) + ",\n    \"must\": [";
    bool any_clause = false;
    for (size_t i = 0; i < terms.size(); i++) {
        if (terms[i].role != nsx::kRoleMust || terms[i].promoted) continue;
        bool first_of_clause = true;
        for (size_t j = 0; j < i; j++) first_of_clause = first_of_clause && !(terms[j].role == nsx::kRoleMust && !terms[j].promoted && terms[j].clause == terms[i].clause);
        if (!first_of_clause) continue;
        o += any_clause ? ",\n      {" : "\n      {";
        o += "\n        \"need\": " + std::to_string(terms[i].need) + ",\n        \"terms\": [";
        bool any = false;
        for (size_t j = i; j < terms.size(); j++)
            if (terms[j].role == nsx::kRoleMust && !terms[j].promoted && terms[j].clause == terms[i].clause) {
                o += any ? ",\n          " : "\n          ";
                json_escape(o, terms[j].text);
                any = true;
            }
        o += "\n        ]\n      }";
        any_clause = true;
    }
    o += any_clause ? "\n    ],\n" : "],\n";
    append_term_list(o, "must_not", terms, [](const nsx::QuorumTerm& t) { return t.role == nsx::kRoleNot; }, false);
    append_term_list(o, "should", terms, [](const nsx::QuorumTerm& t) { return t.role == nsx::kRoleShould || t.promoted; }, true);
    o += "  },\n";
    return o;
}

// tail: to_json_impl's members; "query" is escaped, so the first line that starts like the "results" member is it
static bool quorum_insert(std::string& tail, const std::string& query) {
    const size_t at = tail.find("\n  \"results\": ");
    if (at == std::string::npos) return false;
    tail.insert(at + 1, quorum_member(query));
    return true;
}

// a double as json_number_from_float prints the widened float
static void json_number_from_double(std::string& out, double d) {
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof(buf), d);
    std::string s(buf, r.ptr);
    if (s.find_first_of(".eEn") == std::string::npos) s += ".0";
    out += s;
}

// the "boost" member of search_boosted's body (§5z): the spec as given, the origin without its blanks ("" = the newest dated document)
static std::string boost_member(const nsx::BoostSpec& b) {
    std::string o = "  \"boost\": {\n    \"kind\": ";
    json_escape(o, nsx::boost_name(b));
    o += ",\n    \"offset_days\": ";
    json_number_from_double(o, b.offset_days);
    o += ",\n    \"origin\": ";
    json_escape(o, std::string(nsx::detail::strip_blanks(b.origin)));
    o += ",\n    \"scale_days\": ";
    json_number_from_double(o, b.scale_days);
    o += ",\n    \"undated\": ";
    json_number_from_double(o, b.undated);
    o += ",\n    \"weight\": ";
    json_number_from_double(o, b.weight);
    o += "\n  },\n";
    return o;
}

// the "boosted" member of search_boosted's body (§5z): quorum_member's, where a "must" clause also carries the "weight" of its
// piece and a "should" entry is {"term", "weight"}; "must_not" stays a list of strings (a weight there says nothing)
static std::string boosted_member_of(const char* name, const std::vector<nsx::BoostedTerm>& terms, uint32_t min_should) {
    std::string o = std::string("  \"") + name + "\": {\n    \"min_should\": " + std::to_string(min_should) + ",\n    \"must\": [";
    bool any_clause = false;
    for (size_t i = 0; i < terms.size(); i++) {
        if (terms[i].role != nsx::kRoleMust || terms[i].promoted) continue;
        bool first_of_clause = true;
        for (size_t j = 0; j < i; j++) first_of_clause = first_of_clause && !(terms[j].role == nsx::kRoleMust && !terms[j].promoted && terms[j].clause == terms[i].clause);
        if (!first_of_clause) continue;
        o += any_clause ? ",\n      {" : "\n      {";
        o += "\n        \"need\": " + std::to_string(terms[i].need) + ",\n        \"terms\": [";
        bool any = false;
        for (size_t j = i; j < terms.size(); j++)
            if (terms[j].role == nsx::kRoleMust && !terms[j].promoted && terms[j].clause == terms[i].clause) {
                o += any ? ",\n          " : "\n          ";
                json_escape(o, terms[j].text);
                any = true;
            }
        o += "\n        ],\n        \"weight\": ";
        json_number_from_float(o, terms[i].weight);
        o += "\n      }";
        any_clause = true;
    }
    o += any_clause ? "\n    ],\n" : "],\n";
    append_term_list(o, "must_not", terms, [](const nsx::BoostedTerm& t) { return t.role == nsx::kRoleNot; }, false);
    o += "    \"should\": [";
    bool any = false;
    for (const nsx::BoostedTerm& t : terms)
        if (t.role == nsx::kRoleShould || t.promoted) {
            o += any ? ",\n      {\n        \"term\": " : "\n      {\n        \"term\": ";
            json_escape(o, t.text);
            o += ",\n        \"weight\": ";
            json_number_from_float(o, t.weight);
            o += "\n      }";
            any = true;
        }
    o += any ? "\n    ]\n" : "]\n";
    o += "  },\n";
    return o;
}

static std::string boosted_member(const std::string& query) {
    uint32_t min_should = 0;
    const std::vector<nsx::BoostedTerm> terms = nsx::parse_boosted(query, &min_should);
    return boosted_member_of("boosted", terms, min_should);
}

// the "prefixed" member of search_prefixed's body (§5ab): boosted_member's, where a prefix term prints with its '*'
static std::string prefixed_member(const std::string& query) {
    uint32_t min_should = 0;
    std::vector<nsx::BoostedTerm> terms;
    for (const nsx::PrefixedTerm& t : nsx::parse_prefixed(query, &min_should))
        terms.push_back(nsx::BoostedTerm{t.prefix ? t.text + "*" : t.text, t.role, t.clause, t.need, t.promoted, t.weight});
    return boosted_member_of("prefixed", terms, min_should);
}

// the "prefixes" member behind it: what the call did with the query's distinct prefixes, in query order
static std::string prefixes_member(const std::vector<nsx::PrefixInfo>& info) {
    std::string o = "  \"prefixes\": [";
    for (size_t i = 0; i < info.size(); i++) {
        o += i ? ",\n    {\n      \"expansions\": " : "\n    {\n      \"expansions\": ";
        o += std::to_string(info[i].expansions) + ",\n      \"prefix\": ";
        json_escape(o, info[i].prefix);
        o += std::string(",\n      \"truncated\": ") + (info[i].truncated ? "true" : "false") + "\n    }";
    }
    o += info.empty() ? "],\n" : "\n  ],\n";
    return o;
}

// The dialect's member (the parsed query) put into a body in its sorted place (nlohmann keeps keys sorted).  front: "{\n" and
// the "filter" member if there is one; tail: to_json_impl's members.  "boolean" is the body's first member; "grouped" stands in
// front of tail's "k", "quorum" in front of tail's "results".  -> nullptr, or the name of the member that tail lacks
// "boost" and "boosted" are the body's first two.
static const char* insert_dialect_member(nsx::Dialect dialect, const std::string& query, std::string& front, std::string& tail, const nsx::BoostSpec* boost = nullptr) {
    switch (dialect) {
        case nsx::Dialect::Boolean: front.insert(2, boolean_member(query)); return nullptr;
        case nsx::Dialect::Grouped: return grouped_insert(tail, query) ? nullptr : "k";
        case nsx::Dialect::Quorum: return quorum_insert(tail, query) ? nullptr : "results";
        default: front.insert(2, (boost ? boost_member(*boost) : std::string()) + boosted_member(query)); return nullptr;
    }
}

// search_boolean's body, or the same body over another dialect with its member in place of "boolean"
bool Engine::search_dialect_text(nsx::Dialect dialect, const std::string& query, int k, const nsx::DocFilter* f, std::string& body, const nsx::BoostSpec* boost) {
    if (dialect == nsx::Dialect::Prefixed) return search_prefixed_text(query, k, boost, nsx::PrefixSpec{}, f, body);
    const char* name = names_of(dialect).text;
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { body = err_ = std::string(name) + ": no device context: this engine has no CPU scoring path"; return false; }
    const int K = std::max(1, std::min(k, 100));
    uint32_t handle = 0;
    std::string head = "{\n";
    if (f) {   // search_filtered's filter (cached, most recently used in front) and its "filter" member
        std::string ignored;
        if (!search_filtered_text(std::string(), K, *f, ignored)) { body = err_; return false; }
        handle = filter_lru_.front().handle;
        const size_t at = ignored.find("\n  },\n");
        if (ignored.compare(0, 14, "{\n  \"filter\": ") != 0 || at == std::string::npos) { body = err_ = std::string(name) + ": the filtered body has no filter member"; return false; }
        head = ignored.substr(0, at + 6);
    }
    const QueryView qv{query.data(), query.size()};
    std::vector<ns_hit> hits((size_t)K);
    uint32_t nh = 0;
    uint64_t fd = 0;
    uint8_t us = 0;
    if (!boolean_batch_impl(names_of(dialect).first_page, dialect, handle, &qv, 1, K, nullptr, hits.data(), &nh, &fd, nullptr, &us, nullptr, boost)) { body = err_; return false; }
    SearchResult res;
    res.query = query;
    res.k = K;
    res.segments = (int)segments.size();
    res.has_found = us != 0;
    res.found = fd;
    if (res.has_found)
        for (uint32_t i = 0; i < nh; i++) res.hits.push_back(SearchHit{hits[i].score, hits[i].seg_id, hits[i].doc_id});
    std::string tail = to_json_impl(res).substr(2);
    if (const char* missing = insert_dialect_member(dialect, query, head, tail, boost)) { body = err_ = std::string(name) + ": the search body has no " + missing + " member"; return false; }
    body = head + tail;
    return true;
}

bool Engine::search_dialect_faceted_text(nsx::Dialect dialect, const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f, std::string& body) {
    const char* name = names_of(dialect).faceted_text;
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { body = err_ = std::string(name) + ": no device context: this engine has no CPU scoring path"; return false; }
    if (!search_dialect_text(dialect, query, k, f, body)) return false;
    const uint32_t handle = f ? filter_lru_.front().handle : 0u;   // search_boolean's filter is the most recently used of the cache
    const QueryView qv{query.data(), query.size()};
    std::vector<uint32_t> counts;
    std::vector<std::string> labels;
    uint64_t fd = 0;
    uint8_t us = 0;
    if (!facet_dialect_batch_flat(dialect, spec, handle, &qv, 1, counts, &fd, &us, labels)) { body = err_; return false; }
    if (dialect != nsx::Dialect::Boolean) {   // "facets" < "filter" < "found" < "grouped" < "quorum": the member is the body's first
        body.insert(2, facets_member(spec, labels, counts));
        return true;
    }
    // "boolean" < "facets" < "filter" < "found": the member goes behind the "boolean" member, which is the body's first and whose
    // strings are escaped, so that its closing line is the first of that form
    const size_t at = body.find("\n  },\n");
    if (body.compare(0, 15, "{\n  \"boolean\": ") != 0 || at == std::string::npos) { body = err_ = std::string(name) + ": the boolean body has no boolean member"; return false; }
    body.insert(at + 6, facets_member(spec, labels, counts));
    return true;
}

bool Engine::search_dialect_sorted_text(nsx::Dialect dialect, const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f, std::string& body) {
    const char* name = names_of(dialect).sorted_text;
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { body = err_ = std::string(name) + ": no device context: this engine has no CPU scoring path"; return false; }
    if (!search_dialect_text(dialect, query, k, f, body)) return false;
    const uint32_t handle = f ? filter_lru_.front().handle : 0u;   // search_boolean's filter is the most recently used of the cache
    const size_t K = (size_t)std::max(1, std::min(k, 100));
    const QueryView qv{query.data(), query.size()};
    std::vector<ns_hit> hits(K);
    std::vector<uint32_t> keys(K);
    uint32_t nh = 0;
    uint64_t fd = 0;
    uint8_t us = 0;
    if (!search_dialect_sorted_batch_flat(dialect, spec, handle, &qv, 1, (int)K, nullptr, hits.data(), keys.data(), &nh, &fd, nullptr, &us)) { body = err_; return false; }
    std::vector<SearchHit> sorted;
    if (us)
        for (uint32_t i = 0; i < nh; i++) sorted.push_back(SearchHit{hits[i].score, hits[i].seg_id, hits[i].doc_id});
    // the body's "results" member replaced ("query" is escaped: no line of it starts like a member), "sort" behind "segments"
    const size_t a = body.find("\n  \"results\": "), b = body.rfind("\n  \"segments\": ");
    if (a == std::string::npos || b == std::string::npos || b < a || body.size() < 2) { body = err_ = std::string(name) + ": the boolean body has no results member"; return false; }
    std::string o = body.substr(0, a + 1);
    append_results_json(o, sorted);
    o += body.substr(b + 1, body.size() - (b + 1) - 2);   // "  \"segments\": N", without the closing "\n}"
    o += ",\n  \"sort\": ";
    json_escape(o, nsx::sort_name(spec));
    o += "\n}";
    body = std::move(o);
    return true;
}

// ---- boosts (host/boost.hpp) --------------------------------------------------------------------------------
void Engine::release_boosts() {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (ctx_)
        for (ns_docboost* t : boosts_.dev)
            if (t) (void)ns_docboost_release(ctx_, t);
    boosts_ = BoostSet{};
}

size_t Engine::boost_tables_on_device() const {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    size_t n = 0;
    for (const ns_docboost* t : boosts_.dev) n += t != nullptr;
    return n;
}

bool Engine::boost_table(const nsx::BoostSpec& spec, std::vector<std::vector<float>>& tables) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    tables.clear();
    const size_t S = segments.size();
    uint32_t origin_key = 0;
    if (!nsx::boost_check(spec, origin_key, err_)) return false;
    if (spec.kind == nsx::BoostSpec::Custom) {
        if (spec.custom.size() != S) { err_ = "boost custom: " + std::to_string(spec.custom.size()) + " factor arrays for " + std::to_string(S) + " segments"; return false; }
        for (size_t s = 0; s < S; s++) {
            if (spec.custom[s].size() != segments[s].N) {
                err_ = "boost custom: the factor array of segment " + std::to_string(s) + " has " + std::to_string(spec.custom[s].size()) + " entries, the segment " + std::to_string(segments[s].N) + " documents";
                return false;
            }
            for (const float f : spec.custom[s])
                if (!nsx::boost_factor_ok(f)) { err_ = "boost custom: segment " + std::to_string(s) + " holds a factor that is negative or not finite"; return false; }
        }
        tables = spec.custom;
        return true;
    }
    std::vector<std::vector<uint32_t>> keys;
    if (!sort_keys(nsx::SortSpec{}, keys)) return false;   // date_key() of publish_time per document, 0 = undated
    int64_t origin_days = 0;
    if (origin_key) origin_days = nsx::days_of_key(origin_key);
    else {
        bool any = false;
        for (const auto& ks : keys)
            for (const uint32_t k : ks)
                if (k) { const int64_t d = nsx::days_of_key(k); origin_days = any ? std::max(origin_days, d) : d; any = true; }
    }
    tables.resize(S);
    for (size_t s = 0; s < S; s++) {
        tables[s].resize(keys[s].size());
        for (size_t d = 0; d < keys[s].size(); d++) tables[s][d] = nsx::boost_decay(spec, origin_days, keys[s][d]);
    }
    return true;
}

// the spec's factors on the host and, for every segment with a device copy, on the device; another spec takes the set's place
bool Engine::ensure_boosts(const nsx::BoostSpec& spec, BoostSet*& out) {
    std::string key = "custom";
    if (spec.kind != nsx::BoostSpec::Custom) {
        char buf[160];
        std::snprintf(buf, sizeof(buf), "%d|%a|%a|%a|%a|", (int)spec.kind, spec.weight, spec.scale_days, spec.offset_days, spec.undated);
        key = buf + std::string(nsx::detail::strip_blanks(spec.origin));
    }
    if (boosts_.built && (boosts_.key != key || (spec.kind == nsx::BoostSpec::Custom && boosts_.tables != spec.custom))) release_boosts();
    if (!boosts_.built) {
        BoostSet fresh;
        fresh.key = key;
        if (!boost_table(spec, fresh.tables)) return false;
        fresh.dev.assign(segments.size(), nullptr);
        for (uint32_t s = 0; s < segments.size(); s++) {
            if (!dev_segs_[s]) continue;
            const int rc = ns_docboost_upload(ctx_, segments[s].N, fresh.tables[s].data(), &fresh.dev[s]);
            if (rc != NS_OK) {
                err_ = std::string("ns_docboost_upload: ") + ns_last_error(ctx_);
                for (ns_docboost* t : fresh.dev) if (t) (void)ns_docboost_release(ctx_, t);
                return false;
            }
        }
        fresh.built = true;
        boosts_ = std::move(fresh);
    }
    out = &boosts_;
    return true;
}

// ---- collapsed hits (host/collapse.hpp) -------------------------------------------------------------------
void Engine::release_collapse() {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (ctx_)
        for (ns_dockeys* t : collapse_.dev)
            if (t) (void)ns_dockeys_release(ctx_, t);
    collapse_ = CollapseSet{};
}

size_t Engine::collapse_tables_on_device() const {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    size_t n = 0;
    for (const ns_dockeys* t : collapse_.dev) n += t != nullptr;
    return n;
}

bool Engine::collapse_table(const nsx::CollapseSpec& spec, std::vector<std::vector<uint32_t>>& tables) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    tables.clear();
    if (!nsx::collapse_check(spec, err_)) return false;
    const size_t S = segments.size();
    if (spec.kind == nsx::CollapseSpec::Custom) {
        std::vector<uint32_t> n_docs(S);
        for (size_t s = 0; s < S; s++) n_docs[s] = segments[s].N;
        if (!nsx::collapse_custom_check(spec, n_docs, err_)) return false;
        tables = spec.custom;
        return true;
    }
    nsx::CollapseIds ids;
    tables.resize(S);
    for (uint32_t s = 0; s < S; s++) {
        tables[s].resize(segments[s].N);
        for (uint32_t d = 0; d < segments[s].N; d++) {
            const nsx::MetaFields* md = meta.get(s, d);   // nullptr: no metadata row = no key
            tables[s][d] = md ? ids.key_of(spec.kind == nsx::CollapseSpec::Title ? md->title : md->author) : 0u;
        }
    }
    return true;
}

// the spec's keys on the host and, for every segment with a device copy, on the device; another spec takes the set's place
bool Engine::ensure_collapse(const nsx::CollapseSpec& spec, CollapseSet*& out) {
    if (collapse_.built && (collapse_.kind != (int)spec.kind || (spec.kind == nsx::CollapseSpec::Custom && collapse_.keys != spec.custom))) release_collapse();
    if (!collapse_.built) {
        CollapseSet fresh;
        fresh.kind = (int)spec.kind;
        if (!collapse_table(spec, fresh.keys)) return false;
        fresh.dev.assign(segments.size(), nullptr);
        for (uint32_t s = 0; s < segments.size(); s++) {
            if (!dev_segs_[s]) continue;
            const int rc = ns_dockeys_upload(ctx_, segments[s].N, fresh.keys[s].data(), &fresh.dev[s]);
            if (rc != NS_OK) {
                err_ = std::string("ns_dockeys_upload: ") + ns_last_error(ctx_);
                for (ns_dockeys* t : fresh.dev) if (t) (void)ns_dockeys_release(ctx_, t);
                return false;
            }
        }
        fresh.built = true;
        collapse_ = std::move(fresh);
    }
    out = &collapse_;
    return true;
}

bool Engine::search_collapsed_batch_flat(const nsx::CollapseSpec& collapse_spec, const nsx::BoostSpec* boost_spec, uint32_t filter_handle, const QueryView* queries,
                                         size_t Q, int k, ns_hit* hits, uint32_t* groups, uint32_t* others, uint32_t* nhits, uint64_t* found, uint8_t* usable,
                                         float* device_ms) {
    const char* fn = "search_collapsed_batch_flat";
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (device_ms) *device_ms = 0.0f;
    if (Q && (!queries || !hits || !groups || !nhits || !found || !usable)) { err_ = std::string(fn) + ": null argument"; return false; }
    CallPrep bp;
    for (size_t q = 0; q < Q; q++) {   // (before the device is asked for: the text alone decides)
        const std::string prefix = nsx::collapse_first_prefix(queries[q].p, queries[q].n, bp.scratch);
        if (!prefix.empty()) { err_ = std::string(fn) + ": query " + std::to_string(q) + " holds the prefix term " + prefix + "*: prefix terms are not collapsed (DESIGN.md 5ac, left out)"; return false; }
    }
    if (!ctx_) { err_ = std::string(fn) + ": no device context: collapsed queries run on the device, there is no CPU path"; return false; }
    if (!boolean_prepare(fn, filter_handle, bp)) return false;
    CollapseSet* cs = nullptr;
    if (!ensure_collapse(collapse_spec, cs)) { err_ = std::string(fn) + ": " + err_; return false; }
    std::vector<ns_dockeys*> tabs;
    for (const uint32_t s : bp.listed) tabs.push_back(cs->dev[s]);   // (a filter's copies keep the docIds)
    if (boost_spec) {
        BoostSet* bs = nullptr;
        if (!ensure_boosts(*boost_spec, bs)) { err_ = std::string(fn) + ": " + err_; return false; }
        for (const uint32_t s : bp.listed) bp.boosts.push_back(bs->dev[s]);
    }
    if (Q == 0) return true;
    const size_t K = (size_t)std::max(1, std::min(k, 100));
    const RankedOut out{K, hits, groups, nhits, found, nullptr, device_ms};   // (keys = groups: an empty index fills them with 0)
    if (!ranked_batch(fn, bp, nullptr, Q, out,
        [&](size_t a, size_t b) { return refs_range(fn, nsx::Dialect::Boosted, queries, a, b, usable, bp); },
        [&](size_t a, size_t b, const ns_cursor*, float* ms) {
            const int rc = ns_search_collapsed(ctx_, bp.qd.data(), (uint32_t)(b - a), bp.refs.data(), bp.roles.data(), bp.clauses.data(), bp.needs.data(),
                                               (uint32_t)bp.refs.size(), (uint32_t)K, bp.ids.data(), bp.segs.data(), bp.boosts.empty() ? nullptr : bp.boosts.data(),
                                               tabs.data(), (uint32_t)bp.ids.size(), hits + a * K, groups + a * K, others ? others + a * K : nullptr, nhits + a,
                                               found + a, ms);
            if (rc != NS_OK) { err_ = std::string("ns_search_collapsed: ") + ns_last_error(ctx_); return false; }
            return true;
        })) return false;
    if (bp.ids.empty() && others) std::fill(others, others + Q * K, 0u);   // nothing on the device: ranked_batch filled the rest
    return true;
}

bool Engine::search_collapsed_text(const std::string& query, int k, const nsx::CollapseSpec& collapse_spec, const nsx::BoostSpec* boost_spec, const nsx::DocFilter* f,
                                   std::string& body) {
    const char* name = "search_collapsed";
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    {
        std::vector<char> scratch;
        const std::string prefix = nsx::collapse_first_prefix(query.data(), query.size(), scratch);
        if (!prefix.empty()) { body = err_ = std::string(name) + ": the query holds the prefix term " + prefix + "*: prefix terms are not collapsed (DESIGN.md 5ac, left out)"; return false; }
    }
    if (!ctx_) { body = err_ = std::string(name) + ": no device context: this engine has no CPU scoring path"; return false; }
    const int K = std::max(1, std::min(k, 100));
    uint32_t handle = 0;
    std::string head = "{\n";
    if (f) {   // search_filtered's filter (cached, most recently used in front) and its "filter" member
        std::string ignored;
        if (!search_filtered_text(std::string(), K, *f, ignored)) { body = err_; return false; }
        handle = filter_lru_.front().handle;
        const size_t at = ignored.find("\n  },\n");
        if (ignored.compare(0, 14, "{\n  \"filter\": ") != 0 || at == std::string::npos) { body = err_ = std::string(name) + ": the filtered body has no filter member"; return false; }
        head = ignored.substr(0, at + 6);
    }
    const QueryView qv{query.data(), query.size()};
    std::vector<ns_hit> hits((size_t)K);
    std::vector<uint32_t> groups((size_t)K), others((size_t)K);
    uint32_t nh = 0;
    uint64_t fd = 0;
    uint8_t us = 0;
    if (!search_collapsed_batch_flat(collapse_spec, boost_spec, handle, &qv, 1, K, hits.data(), groups.data(), others.data(), &nh, &fd, &us, nullptr)) { body = err_; return false; }
    SearchResult res;
    res.query = query;
    res.k = K;
    res.segments = (int)segments.size();
    res.has_found = us != 0;
    res.found = fd;
    if (res.has_found)
        for (uint32_t i = 0; i < nh; i++) res.hits.push_back(SearchHit{hits[i].score, hits[i].seg_id, hits[i].doc_id});
    std::string tail = to_json_impl(res).substr(2);
    // "others" behind every result's "docId" line ("cord_uid" < "docId" < "others" < "publish_time"; strings are escaped, so no
    // other line of the body starts like that one)
    size_t at = 0;
    for (size_t i = 0; i < res.hits.size(); i++) {
        const std::string line = "      \"docId\": " + std::to_string(res.hits[i].doc) + ",\n";
        at = tail.find(line, at);
        if (at == std::string::npos) { body = err_ = std::string(name) + ": the search body has no docId member"; return false; }
        at += line.size();
        const std::string more = "      \"others\": " + std::to_string(others[i]) + ",\n";
        tail.insert(at, more);
        at += more.size();
    }
    uint32_t min_should = 0;
    const std::vector<nsx::BoostedTerm> terms = nsx::parse_boosted(query, &min_should);
    std::string members = boost_spec ? boost_member(*boost_spec) : std::string();
    members += std::string("  \"collapse\": {\n    \"field\": \"") + nsx::collapse_name(collapse_spec) + "\"\n  },\n";
    members += boosted_member_of("collapsed", terms, min_should);
    head.insert(2, members);   // "boost" < "collapse" < "collapsed" < "filter"
    body = head + tail;
    return true;
}

std::string Engine::search_collapsed(const std::string& query, int k, const nsx::CollapseSpec& collapse_spec, const nsx::BoostSpec* boost_spec, const nsx::DocFilter* f) {
    std::string body;
    return search_collapsed_text(query, k, collapse_spec, boost_spec, f, body) ? body : error_body(body);
}

bool Engine::search_boosted_after_batch_flat(const nsx::BoostSpec* spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k, const nsx::PageCursor* after,
                                             ns_hit* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms) {
    return search_dialect_after_batch_flat(nsx::Dialect::Boosted, filter_handle, queries, Q, k, after, hits, nhits, found, rest, usable, device_ms, spec);
}

bool Engine::search_boosted_text(const std::string& query, int k, const nsx::BoostSpec* spec, const nsx::DocFilter* f, std::string& body) {
    return search_dialect_text(nsx::Dialect::Boosted, query, k, f, body, spec);
}

std::string Engine::search_boosted(const std::string& query, int k, const nsx::BoostSpec* spec, const nsx::DocFilter* f) {
    std::string body;
    return search_boosted_text(query, k, spec, f, body) ? body : error_body(body);
}

// ---- prefix terms (host/prefix.hpp, csrc/ns_union.hip) ----------------------------------------------------
// The dictionary rows of the terms of suggest_table that begin with the prefix [p, p + n), in byte order; table_idx (may be
// nullptr): their rows in the table.  The table is sorted by bytes, so they are ONE range; more than max_expansions of them:
// the best by (score descending, table row ascending) stay.
bool Engine::expand_prefix_rows(const char* p, size_t n, uint32_t max_expansions, std::vector<uint32_t>& rows, std::vector<uint32_t>* table_idx, bool& truncated) const {
    rows.clear();
    if (table_idx) table_idx->clear();
    truncated = false;
    const nsx::SuggestTable& t = suggest_table;
    // -1, 0, +1: term i against the prefix as a byte string; begins: the term has the prefix in front
    auto begins = [&](size_t i) { return t.term_len(i) >= n && std::memcmp(t.term(i), p, n) == 0; };
    auto below = [&](size_t i) {
        const size_t m = std::min(t.term_len(i), n);
        const int c = std::memcmp(t.term(i), p, m);
        return c != 0 ? c < 0 : t.term_len(i) < n;
    };
    size_t lo = 0, hi = t.size();
    while (lo < hi) { const size_t mid = (lo + hi) / 2; if (below(mid)) lo = mid + 1; else hi = mid; }
    size_t end = lo, top = t.size();
    while (end < top) { const size_t mid = (end + top) / 2; if (begins(mid)) end = mid + 1; else top = mid; }
    std::vector<uint32_t> kept(end - lo);
    for (size_t i = lo; i < end; i++) kept[i - lo] = (uint32_t)i;
    if (kept.size() > max_expansions) {
        truncated = true;
        std::partial_sort(kept.begin(), kept.begin() + max_expansions, kept.end(),
                          [&](uint32_t a, uint32_t b) { return t.score[a] != t.score[b] ? t.score[a] > t.score[b] : a < b; });
        kept.resize(max_expansions);
        std::sort(kept.begin(), kept.end());
    }
    for (const uint32_t i : kept) {
        const int64_t gid = dict.find(t.term(i), t.term_len(i));
        if (gid < 0 || (!rows.empty() && rows.back() == (uint32_t)gid)) continue;   // not a term of the lexicons as it stands; the table's second row of a term
        rows.push_back((uint32_t)gid);
        if (table_idx) table_idx->push_back(i);
    }
    return true;
}

bool Engine::expand_prefix(const std::string& prefix, uint32_t max_expansions, std::vector<std::string>& terms, bool& truncated) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    terms.clear();
    truncated = false;
    nsx::PrefixSpec ps;
    ps.max_expansions = max_expansions;
    if (!nsx::prefix_check(ps, err_)) { err_ = "expand_prefix: " + err_; return false; }
    std::string norm;
    nsx::normalize_token(prefix.data(), prefix.size(), norm);
    std::vector<uint32_t> rows, idx;
    expand_prefix_rows(norm.data(), norm.size(), max_expansions, rows, &idx, truncated);
    for (const uint32_t i : idx) terms.emplace_back(suggest_table.term(i), suggest_table.term_len(i));
    return true;
}

void Engine::release_prefix_segments(PrefixRows& px) {
    for (ns_seg*& s : px.segs)
        if (s) { (void)ns_segment_release(ctx_, s); s = nullptr; }
}

bool Engine::search_prefixed_after_batch_flat(const nsx::BoostSpec* spec, const nsx::PrefixSpec& prefix_spec, uint32_t filter_handle, const QueryView* queries, size_t Q,
                                              int k, const nsx::PageCursor* after, ns_hit* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable,
                                              float* device_ms, std::vector<std::vector<nsx::PrefixInfo>>* prefixes) {
    const char* fn = names_of(nsx::Dialect::Prefixed).after_batch;
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (device_ms) *device_ms = 0.0f;
    if (prefixes) prefixes->assign(Q, std::vector<nsx::PrefixInfo>());
    if (!ctx_) { err_ = std::string(fn) + ": no device context: boolean queries run on the device, there is no CPU path"; return false; }
    if (Q && (!queries || !hits || !nhits || !found || !usable)) { err_ = std::string(fn) + ": null argument"; return false; }
    if (filter_handle) { err_ = std::string(fn) + ": a filter is refused: prefix terms do not run under a filter (a filtered union needs the unfiltered union's df for its idf)"; return false; }
    if (!nsx::prefix_check(prefix_spec, err_)) { err_ = std::string(fn) + ": " + err_; return false; }
    // the batch's distinct ordinary terms and distinct prefixes, in order of first appearance
    PrefixRows px;
    std::vector<std::vector<uint32_t>> per_query(prefixes ? Q : 0);
    {
        std::vector<char> scratch;
        for (size_t q = 0; q < Q; q++)
            nsx::for_each_prefixed_term(queries[q].p, queries[q].n, scratch, [&](const char* p, size_t n, uint8_t, uint32_t, uint32_t, float, bool star) {
                if (!star) {
                    const int64_t gid = dict.find(p, n);
                    if (gid >= 0 && px.of_term.emplace((uint32_t)gid, (uint32_t)px.terms.size()).second) px.terms.push_back((uint32_t)gid);
                    return;
                }
                const auto at = px.of_prefix.emplace(std::string(p, n), (uint32_t)px.info.size());
                if (at.second) px.info.push_back(nsx::PrefixInfo{std::string(p, n), 0u, false});
                if (prefixes && std::find(per_query[q].begin(), per_query[q].end(), at.first->second) == per_query[q].end()) per_query[q].push_back(at.first->second);
            });
    }
    if (px.info.empty())   // no prefix anywhere: the Boosted call, untouched
        return search_boosted_after_batch_flat(spec, 0, queries, Q, k, after, hits, nhits, found, rest, usable, device_ms);
    const uint32_t n_ord = (uint32_t)px.terms.size(), P = (uint32_t)px.info.size(), S = (uint32_t)segments.size();
    for (auto& kv : px.of_prefix) kv.second += n_ord;
    px.expansions.resize(P);
    for (uint32_t i = 0; i < P; i++) {
        expand_prefix_rows(px.info[i].prefix.data(), px.info[i].prefix.size(), prefix_spec.max_expansions, px.expansions[i], nullptr, px.info[i].truncated);
        px.info[i].expansions = (uint32_t)px.expansions[i].size();
    }
    if (prefixes)
        for (size_t q = 0; q < Q; q++)
            for (const uint32_t i : per_query[q]) (*prefixes)[q].push_back(px.info[i]);

    CallPrep bp;
    if (!boolean_prepare(fn, 0, bp)) return false;
    if (spec) {
        BoostSet* bs = nullptr;
        if (!ensure_boosts(*spec, bs)) { err_ = std::string(fn) + ": " + err_; return false; }
        for (const uint32_t s : bp.listed) bp.boosts.push_back(bs->dev[s]);
    }
    // one derived segment per listed position, under ids above the filters' range
    if (((uint64_t)kMaxFilters + 2) * S > (1u << 20)) { err_ = std::string(fn) + ": the derived segments' ids would reach 2^20"; return false; }
    const uint32_t id_base = (uint32_t)(kMaxFilters + 1) * S;
    const nsx::TermSeg absent{nsx::kAbsent, 0u, 0.0f};
    px.rows.assign((size_t)(n_ord + P) * S, absent);
    px.segs.assign(S, nullptr);
    struct Release { Engine* e; PrefixRows* px; ~Release() { e->release_prefix_segments(*px); } } release{this, &px};
    float union_ms = 0.0f;
    std::vector<uint64_t> off, noff, soff;
    std::vector<uint32_t> cnt, gb, ncnt, scnt, row_of;
    std::vector<float> idf_of;   // of a copied list: its dictionary row's; of a union: computed from its count
    std::vector<uint8_t> is_union;
    for (size_t li = 0; li < bp.listed.size(); li++) {
        const uint32_t sid = bp.listed[li];
        const nsx::SegmentData& sd = segments[sid];
        // a list that lies inside the payload (a damaged record stays absent, as under a filter)
        auto inside = [&](const nsx::TermSeg& e) { return e.byte_off != nsx::kAbsent && e.byte_off % 8 == 0 && e.byte_off / 8 + e.count <= sd.postings_bytes / 8; };
        off.clear(); cnt.clear(); row_of.clear(); idf_of.clear(); is_union.clear();
        gb.assign(1, 0u);
        for (uint32_t r = 0; r < n_ord; r++) {
            const nsx::TermSeg& e = dict.row(px.terms[r])[sid];
            if (!inside(e)) continue;
            off.push_back(e.byte_off); cnt.push_back(e.count);
            gb.push_back((uint32_t)off.size()); row_of.push_back(r); idf_of.push_back(e.idf); is_union.push_back(0);
        }
        for (uint32_t i = 0; i < P; i++) {
            const size_t first = off.size();
            float own = 0.0f;
            for (const uint32_t gid : px.expansions[i]) {
                const nsx::TermSeg& e = dict.row(gid)[sid];
                if (!inside(e)) continue;
                off.push_back(e.byte_off); cnt.push_back(e.count);
                own = e.idf;
            }
            if (off.size() == first) continue;   // an absent term of this segment
            gb.push_back((uint32_t)off.size()); row_of.push_back(n_ord + i); idf_of.push_back(own); is_union.push_back(off.size() - first >= 2);
        }
        const uint32_t G = (uint32_t)row_of.size();
        noff.assign(std::max<uint32_t>(G, 1), 0); ncnt.assign(std::max<uint32_t>(G, 1), 0);
        float ms = 0.0f;
        const int rc = ns_segment_union(ctx_, dev_segs_[sid], id_base + sid, off.data(), cnt.data(), gb.data(), G, noff.data(), ncnt.data(), nullptr, nullptr, nullptr, &ms,
                                        &px.segs[sid]);
        if (rc != NS_OK) { err_ = std::string("ns_segment_union: ") + ns_last_error(ctx_); return false; }
        union_ms += ms;
        const uint32_t min_count = std::max<uint32_t>(64u, sd.N / 512u);   // reload()'s rule for skip tables
        soff.clear(); scnt.clear();
        for (uint32_t g = 0; g < G; g++) {
            if (is_union[g] && !ncnt[g]) continue;
            px.rows[(size_t)row_of[g] * S + sid] = nsx::TermSeg{noff[g], ncnt[g], is_union[g] ? bm25_idf(sd.N, ncnt[g]) : idf_of[g]};
            if (ncnt[g] >= min_count) { soff.push_back(noff[g]); scnt.push_back(ncnt[g]); }
        }
        if (!soff.empty()) (void)ns_segment_build_skips(ctx_, px.segs[sid], soff.data(), scnt.data(), (uint32_t)soff.size());
        bp.ids[li] = id_base + sid;
        bp.segs[li] = px.segs[sid];
    }
    bp.rs.rows = px.rows.data();
    bp.rs.id_base = id_base;
    bp.px = &px;
    if (device_ms) *device_ms += union_ms;
    if (Q == 0) return true;
    const RankedOut out{(size_t)std::max(1, std::min(k, 100)), hits, nullptr, nhits, found, rest, device_ms};
    return ranked_batch(fn, bp, after, Q, out,
        [&](size_t a, size_t b) { return refs_range(fn, nsx::Dialect::Prefixed, queries, a, b, usable, bp); },
        [&](size_t a, size_t b, const ns_cursor* cur, float* ms) { return ranked_call(nsx::Dialect::Prefixed, after != nullptr, bp, a, b, out, cur, ms); });
}

// one query's page of the prefixed call and the two members of its bodies, "prefixed" and "prefixes"
bool Engine::prefix_page(const std::string& query, int k, const nsx::PageCursor* cur, const nsx::BoostSpec* boost, const nsx::PrefixSpec& ps, ns_hit* hits, uint32_t* nh,
                         uint64_t* fd, uint64_t* rs, uint8_t* us, std::string& member) {
    const QueryView qv{query.data(), query.size()};
    std::vector<std::vector<nsx::PrefixInfo>> info;
    if (!search_prefixed_after_batch_flat(boost, ps, 0, &qv, 1, k, cur, hits, nh, fd, rs, us, nullptr, &info)) return false;
    member = prefixed_member(query) + prefixes_member(info[0]);
    return true;
}

bool Engine::search_prefixed_text(const std::string& query, int k, const nsx::BoostSpec* spec, const nsx::PrefixSpec& prefix_spec, const nsx::DocFilter* f, std::string& body) {
    const char* name = names_of(nsx::Dialect::Prefixed).text;
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { body = err_ = std::string(name) + ": no device context: this engine has no CPU scoring path"; return false; }
    if (f) { body = err_ = std::string(name) + ": a filter is refused: prefix terms do not run under a filter (a filtered union needs the unfiltered union's df for its idf)"; return false; }
    const int K = std::max(1, std::min(k, 100));
    std::vector<ns_hit> hits((size_t)K);
    uint32_t nh = 0;
    uint64_t fd = 0;
    uint8_t us = 0;
    std::string member;
    if (!prefix_page(query, K, nullptr, spec, prefix_spec, hits.data(), &nh, &fd, nullptr, &us, member)) { body = err_; return false; }
    SearchResult res;
    res.query = query;
    res.k = K;
    res.segments = (int)segments.size();
    res.has_found = us != 0;
    res.found = fd;
    if (res.has_found)
        for (uint32_t i = 0; i < nh; i++) res.hits.push_back(SearchHit{hits[i].score, hits[i].seg_id, hits[i].doc_id});
    std::string tail = to_json_impl(res).substr(2);
    // "k" < "prefixed" < "prefixes" < "query": nlohmann keeps keys sorted ("query" is escaped: no line of it starts like a member)
    const size_t at = tail.find("  \"query\": ");
    if (at == std::string::npos || (at != 0 && tail[at - 1] != '\n')) { body = err_ = std::string(name) + ": the search body has no query member"; return false; }
    tail.insert(at, member);
    body = "{\n" + (spec ? boost_member(*spec) : std::string()) + tail;
    return true;
}

std::string Engine::search_prefixed(const std::string& query, int k, const nsx::BoostSpec* spec, const nsx::PrefixSpec& prefix_spec, const nsx::DocFilter* f) {
    std::string body;
    return search_prefixed_text(query, k, spec, prefix_spec, f, body) ? body : error_body(body);
}

// ---- the named methods: forwards to the dialect forms --------------------------------------------------------------------
bool Engine::search_boolean_batch_flat(uint32_t filter_handle, const QueryView* queries, size_t Q, int k, ns_hit* hits, uint32_t* nhits,
                                       uint64_t* found, uint8_t* usable, float* device_ms) {
    return boolean_batch_impl(names_of(nsx::Dialect::Boolean).first_page, nsx::Dialect::Boolean, filter_handle, queries, Q, k, nullptr, hits, nhits, found, nullptr, usable, device_ms);
}

bool Engine::search_boolean_after_batch_flat(uint32_t filter_handle, const QueryView* queries, size_t Q, int k, const nsx::PageCursor* after, ns_hit* hits,
                                            uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms) {
    return search_dialect_after_batch_flat(nsx::Dialect::Boolean, filter_handle, queries, Q, k, after, hits, nhits, found, rest, usable, device_ms);
}

bool Engine::facet_boolean_batch_flat(const nsx::FacetSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, std::vector<uint32_t>& counts,
                                     uint64_t* found, uint8_t* usable, std::vector<std::string>& labels, float* device_ms) {
    return facet_dialect_batch_flat(nsx::Dialect::Boolean, spec, filter_handle, queries, Q, counts, found, usable, labels, device_ms);
}

bool Engine::search_boolean_sorted_batch_flat(const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k,
                                             const nsx::PageCursor* after, ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                             uint8_t* usable, float* device_ms) {
    return search_dialect_sorted_batch_flat(nsx::Dialect::Boolean, spec, filter_handle, queries, Q, k, after, hits, keys, nhits, found, rest, usable, device_ms);
}

bool Engine::search_boolean_text(const std::string& query, int k, const nsx::DocFilter* f, std::string& body) {
    return search_dialect_text(nsx::Dialect::Boolean, query, k, f, body);
}

bool Engine::search_boolean_faceted_text(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f, std::string& body) {
    return search_dialect_faceted_text(nsx::Dialect::Boolean, query, k, spec, f, body);
}

bool Engine::search_boolean_sorted_text(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f, std::string& body) {
    return search_dialect_sorted_text(nsx::Dialect::Boolean, query, k, spec, f, body);
}

std::string Engine::search_boolean(const std::string& query, int k, const nsx::DocFilter* f) {
    std::string body;
    return search_dialect_text(nsx::Dialect::Boolean, query, k, f, body) ? body : error_body(body);
}

std::string Engine::search_boolean_faceted(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f) {
    std::string body;
    return search_dialect_faceted_text(nsx::Dialect::Boolean, query, k, spec, f, body) ? body : error_body(body);
}

std::string Engine::search_boolean_sorted(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f) {
    std::string body;
    return search_dialect_sorted_text(nsx::Dialect::Boolean, query, k, spec, f, body) ? body : error_body(body);
}

bool Engine::search_grouped_after_batch_flat(uint32_t filter_handle, const QueryView* queries, size_t Q, int k, const nsx::PageCursor* after, ns_hit* hits,
                                            uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms) {
    return search_dialect_after_batch_flat(nsx::Dialect::Grouped, filter_handle, queries, Q, k, after, hits, nhits, found, rest, usable, device_ms);
}

bool Engine::facet_grouped_batch_flat(const nsx::FacetSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, std::vector<uint32_t>& counts,
                                     uint64_t* found, uint8_t* usable, std::vector<std::string>& labels, float* device_ms) {
    return facet_dialect_batch_flat(nsx::Dialect::Grouped, spec, filter_handle, queries, Q, counts, found, usable, labels, device_ms);
}

bool Engine::search_grouped_sorted_batch_flat(const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k,
                                             const nsx::PageCursor* after, ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                             uint8_t* usable, float* device_ms) {
    return search_dialect_sorted_batch_flat(nsx::Dialect::Grouped, spec, filter_handle, queries, Q, k, after, hits, keys, nhits, found, rest, usable, device_ms);
}

bool Engine::search_grouped_text(const std::string& query, int k, const nsx::DocFilter* f, std::string& body) {
    return search_dialect_text(nsx::Dialect::Grouped, query, k, f, body);
}

bool Engine::search_grouped_faceted_text(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f, std::string& body) {
    return search_dialect_faceted_text(nsx::Dialect::Grouped, query, k, spec, f, body);
}

bool Engine::search_grouped_sorted_text(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f, std::string& body) {
    return search_dialect_sorted_text(nsx::Dialect::Grouped, query, k, spec, f, body);
}

std::string Engine::search_grouped(const std::string& query, int k, const nsx::DocFilter* f) {
    std::string body;
    return search_dialect_text(nsx::Dialect::Grouped, query, k, f, body) ? body : error_body(body);
}

std::string Engine::search_grouped_faceted(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f) {
    std::string body;
    return search_dialect_faceted_text(nsx::Dialect::Grouped, query, k, spec, f, body) ? body : error_body(body);
}

std::string Engine::search_grouped_sorted(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f) {
    std::string body;
    return search_dialect_sorted_text(nsx::Dialect::Grouped, query, k, spec, f, body) ? body : error_body(body);
}

bool Engine::search_quorum_after_batch_flat(uint32_t filter_handle, const QueryView* queries, size_t Q, int k, const nsx::PageCursor* after, ns_hit* hits,
                                           uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms) {
    return search_dialect_after_batch_flat(nsx::Dialect::Quorum, filter_handle, queries, Q, k, after, hits, nhits, found, rest, usable, device_ms);
}

bool Engine::facet_quorum_batch_flat(const nsx::FacetSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, std::vector<uint32_t>& counts,
                                    uint64_t* found, uint8_t* usable, std::vector<std::string>& labels, float* device_ms) {
    return facet_dialect_batch_flat(nsx::Dialect::Quorum, spec, filter_handle, queries, Q, counts, found, usable, labels, device_ms);
}

bool Engine::search_quorum_sorted_batch_flat(const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k,
                                            const nsx::PageCursor* after, ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                            uint8_t* usable, float* device_ms) {
    return search_dialect_sorted_batch_flat(nsx::Dialect::Quorum, spec, filter_handle, queries, Q, k, after, hits, keys, nhits, found, rest, usable, device_ms);
}

bool Engine::search_quorum_text(const std::string& query, int k, const nsx::DocFilter* f, std::string& body) {
    return search_dialect_text(nsx::Dialect::Quorum, query, k, f, body);
}

bool Engine::search_quorum_faceted_text(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f, std::string& body) {
    return search_dialect_faceted_text(nsx::Dialect::Quorum, query, k, spec, f, body);
}

bool Engine::search_quorum_sorted_text(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f, std::string& body) {
    return search_dialect_sorted_text(nsx::Dialect::Quorum, query, k, spec, f, body);
}

std::string Engine::search_quorum(const std::string& query, int k, const nsx::DocFilter* f) {
    std::string body;
    return search_dialect_text(nsx::Dialect::Quorum, query, k, f, body) ? body : error_body(body);
}

std::string Engine::search_quorum_faceted(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f) {
    std::string body;
    return search_dialect_faceted_text(nsx::Dialect::Quorum, query, k, spec, f, body) ? body : error_body(body);
}

std::string Engine::search_quorum_sorted(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f) {
    std::string body;
    return search_dialect_sorted_text(nsx::Dialect::Quorum, query, k, spec, f, body) ? body : error_body(body);
}

// ---- pages past the first K (host/page.hpp, csrc/ns_after_plan.hpp) -------------------------------------
// The search's own query preparation, then ns_search_boolean_after: roles == NULL is the OR search bit for bit, every role
// MUST the AND search, so page 1 is search_batch_flat's answer and page n continues it.
bool Engine::search_after_batch_flat(uint32_t filter_handle, const QueryView* queries, size_t Q, int k, uint32_t flags, const nsx::PageCursor* after,
                                     ns_hit* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms) {
    const char* fn = "search_after_batch_flat";
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (device_ms) *device_ms = 0.0f;
    if (!ctx_) { err_ = std::string(fn) + ": no device context: pages are cut on the device, there is no CPU path"; return false; }
    if (Q && (!queries || !hits || !nhits || !found || !usable)) { err_ = std::string(fn) + ": null argument"; return false; }
    if (flags & ~(uint32_t)NS_FLAG_AND) { err_ = std::string(fn) + ": flags are NS_FLAG_OR or NS_FLAG_AND"; return false; }
    CallPrep bp;
    if (!boolean_prepare(fn, filter_handle, bp)) return false;
    if (Q == 0) return true;
    const bool and_mode = (flags & NS_FLAG_AND) != 0;
    const RankedOut out{(size_t)std::max(1, std::min(k, 100)), hits, nullptr, nhits, found, rest, device_ms};
    std::vector<uint8_t> roles;
    PlainPrep pp;
    if (!plain_prepare(queries, Q, usable, bp.rs, and_mode, pp)) return false;
    return ranked_batch(fn, bp, after, Q, out,
        [&](size_t a, size_t b) { plain_range(queries, a, b, usable, bp.rs, and_mode, pp); return true; },
        [&](size_t a, size_t b, const ns_cursor* cur, float* ms) {
            if (and_mode) roles.assign(pp.n_refs, nsx::kRoleMust);
            const int rc = ns_search_boolean_after(ctx_, pp.qd_at, (uint32_t)(b - a), pp.refs_at, and_mode ? roles.data() : nullptr, (uint32_t)pp.n_refs, (uint32_t)out.K, cur,
                                                   bp.ids.data(), bp.segs.data(), (uint32_t)bp.ids.size(), hits + a * out.K, nhits + a, found + a, rest ? rest + a : nullptr, ms);
            if (rc != NS_OK) { err_ = std::string("ns_search_boolean_after: ") + ns_last_error(ctx_); return false; }
            return true;
        });
}

bool Engine::search_page_text(const std::string& query, int k, const std::string& cursor_text, const nsx::PageSpec& spec, std::string& body) {
    std::lock_guard<std::recursive_mutex> lock(mtx_);
    if (!ctx_) { body = err_ = "search_page: no device context: this engine has no CPU scoring path"; return false; }
    if ((unsigned)spec.mode > (unsigned)nsx::PageSpec::Prefixed) { body = err_ = "search_page: unknown mode"; return false; }
    const bool prefixed = spec.mode == nsx::PageSpec::Prefixed;
    if (prefixed && spec.use_filter) { body = err_ = "search_page: a filter is refused: prefix terms do not run under a filter (a filtered union needs the unfiltered union's df for its idf)"; return false; }
    const nsx::BoostSpec* boost = ((spec.mode == nsx::PageSpec::Boosted || prefixed) && spec.use_boost) ? &spec.boost : nullptr;
    std::string prefix_members;   // Prefixed: "prefixed" and "prefixes"
    const char kind = nsx::page_kind(spec.mode);
    nsx::PageCursor cur;
    if (!nsx::parse_cursor(cursor_text, kind, cur, err_)) { body = err_ = "search_page: " + err_; return false; }
    const int K = std::max(1, std::min(k, 100));
    uint32_t handle = 0;
    std::string head = "{\n";
    if (spec.use_filter) {   // search_filtered's filter (cached, most recently used in front) and its "filter" member
        std::string ignored;
        if (!search_filtered_text(std::string(), K, spec.filter, ignored)) { body = err_; return false; }
        handle = filter_lru_.front().handle;
        const size_t at = ignored.find("\n  },\n");
        if (ignored.compare(0, 14, "{\n  \"filter\": ") != 0 || at == std::string::npos) { body = err_ = "search_page: the filtered body has no filter member"; return false; }
        head = ignored.substr(0, at + 6);
    }
    const QueryView qv{query.data(), query.size()};
    std::vector<ns_hit> hits((size_t)K);
    std::vector<uint32_t> keys((size_t)K, 0u);
    uint32_t nh = 0;
    uint64_t fd = 0, rs = 0;
    uint8_t us = 0;
    const nsx::PageCall call = nsx::page_call(spec.mode);
    bool ok = false;
    if (prefixed) ok = prefix_page(query, K, &cur, boost, spec.prefix, hits.data(), &nh, &fd, &rs, &us, prefix_members);
    else if (!call.plain)
        ok = call.dated ? search_dialect_sorted_batch_flat(call.dialect, spec.sort, handle, &qv, 1, K, &cur, hits.data(), keys.data(), &nh, &fd, &rs, &us)
                        : search_dialect_after_batch_flat(call.dialect, handle, &qv, 1, K, &cur, hits.data(), &nh, &fd, &rs, &us, nullptr, boost);
    else if (call.dated) ok = search_sorted_after_batch_flat(spec.sort, handle, &qv, 1, K, NS_FLAG_OR, &cur, hits.data(), keys.data(), &nh, &fd, &rs, &us);
    else ok = search_after_batch_flat(handle, &qv, 1, K, spec.mode == nsx::PageSpec::SearchAnd ? NS_FLAG_AND : NS_FLAG_OR, &cur, hits.data(), &nh, &fd, &rs, &us);
    if (!ok) { body = err_; return false; }
    SearchResult res;
    res.query = query;
    res.k = K;
    res.segments = (int)segments.size();
    res.has_found = us != 0;
    res.found = fd;
    if (!res.has_found) { nh = 0; rs = 0; fd = 0; }
    for (uint32_t i = 0; i < nh; i++) res.hits.push_back(SearchHit{hits[i].score, hits[i].seg_id, hits[i].doc_id});
    std::string o = head;
    std::string rest_of = to_json_impl(res).substr(2);   // "found" (when usable), "k", "query", "results", "segments"
    if (prefixed) o += boost ? boost_member(*boost) : std::string();   // its own members stand behind "page"
    else if (!call.plain)   // the dialect's member, as in its search_* body
        if (const char* missing = insert_dialect_member(call.dialect, query, o, rest_of, boost)) { body = err_ = std::string("search_page: the search body has no ") + missing + " member"; return false; }
    // "k" < "page" < "query": nlohmann keeps keys sorted ("query" is escaped: no line of it starts like a member)
    const size_t at = rest_of.find("  \"query\": ");
    if (at == std::string::npos || (at != 0 && rest_of[at - 1] != '\n')) { body = err_ = "search_page: the search body has no query member"; return false; }
    std::string page = "  \"page\": {\n    \"cursor\": ";
    json_escape(page, cursor_text);
    if (rs > nh && nh > 0) {
        nsx::PageCursor next;
        next.set = true;
        uint32_t score_bits = 0;
        std::memcpy(&score_bits, &hits[nh - 1].score, 4);
        next.rank = kind == 'd' ? keys[nh - 1] : score_bits;
        next.seg = hits[nh - 1].seg_id;
        next.doc = hits[nh - 1].doc_id;
        page += ",\n    \"next\": ";
        json_escape(page, nsx::cursor_text(kind, next));
    }
    page += ",\n    \"offset\": " + std::to_string(fd - rs);
    page += ",\n    \"remaining\": " + std::to_string(rs - nh) + "\n  },\n";
    rest_of.insert(at, page + prefix_members);   // "page" < "prefixed" < "prefixes" < "query"
    o += rest_of;
    if (kind == 'd') {   // search_sorted's "sort" member behind "segments"
        o.resize(o.size() - 2);                 // the closing "\n}"
        o += ",\n  \"sort\": ";
        json_escape(o, nsx::sort_name(spec.sort));
        o += "\n}";
    }
    body = std::move(o);
    return true;
}

std::string Engine::search_page(const std::string& query, int k, const std::string& cursor_text, const nsx::PageSpec& spec) {
    std::string body;
    return search_page_text(query, k, cursor_text, spec, body) ? body : error_body(body);
}

}  // namespace nextsearch
