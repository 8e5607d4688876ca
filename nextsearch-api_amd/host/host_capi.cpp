// C wrappers of include/nextsearch_host.h over nextsearch::Engine.
// No C++ exception crosses the boundary: every entry runs inside try/catch (std::filesystem errors, bad_alloc on a
// corrupt count, ...) and reports failure through its return value and nsh_engine_error().
#include "invert.hpp"
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/nextsearch_host.h"
#include "engine.hpp"
#include "gen_index.hpp"
#include "textutil.hpp"
#include "json_writer.hpp"

struct nsh_engine {
    nextsearch::Engine eng;
    std::string err;      // the wrapper's last message; written and read under err_mtx (callers may share an engine between threads)
    std::mutex err_mtx;
    explicit nsh_engine(int device) : eng(device) {}
    explicit nsh_engine(const std::vector<int>& devices) : eng(devices) {}
};

static void nsh_set_err(nsh_engine* e, const std::string& msg) {
    if (!e) return;
    std::lock_guard<std::mutex> l(e->err_mtx);
    e->err = msg;
}
static void nsh_note(nsh_engine* e, const char* where, const char* what) {
    nsh_set_err(e, std::string(where) + ": " + what);
}
#define NSH_CATCH(e, where, failval)                                                        \
    catch (const std::exception& ex_) { nsh_note((e), (where), ex_.what()); return failval; } \
    catch (...) { nsh_note((e), (where), "unknown exception"); return failval; }
#define NSH_CATCH_VOID(e, where)                                          \
    catch (const std::exception& ex_) { nsh_note((e), (where), ex_.what()); } \
    catch (...) { nsh_note((e), (where), "unknown exception"); }

static std::vector<std::string> to_vec(const char* const* qs, uint32_t n) {
    std::vector<std::string> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = qs[i] ? qs[i] : "";
    return v;
}

extern "C" int nsh_gen_index(const char* index_dir, uint32_t n_segments, uint32_t docs_per_segment, uint32_t vocab,
                             uint64_t seed, int legacy_layout, uint64_t* total_postings_out) {
    try {
        nsx::GenParams p;
        p.index_dir = index_dir;
        p.n_segments = n_segments;
        p.docs_per_segment = docs_per_segment;
        p.vocab = vocab;
        p.seed = seed;
        p.legacy_layout = legacy_layout != 0;
        nsx::GenStats st = nsx::generate_index(p);
        if (total_postings_out) *total_postings_out = st.total_postings;
        return 0;
    } catch (const std::exception&) {
        return -1;
    }
}

extern "C" int nsh_engine_open(const char* index_dir, int device, nsh_engine** out) { try {
    if (!out) return -1;
    nsh_engine* e = new nsh_engine(device);
    e->eng.index_dir = index_dir ? index_dir : "";
    *out = e;
    if (!e->eng.reload()) { nsh_set_err(e, e->eng.last_error()); return -1; }
    return 0;
} NSH_CATCH(out ? *out : nullptr, "nsh_engine_open", -1)
}

extern "C" int nsh_engine_open_multi(const char* index_dir, const int* devices, uint32_t n_devices, nsh_engine** out) { try {
    if (!out || !devices || n_devices == 0) return -1;
    nsh_engine* e = new nsh_engine(std::vector<int>(devices, devices + n_devices));
    e->eng.index_dir = index_dir ? index_dir : "";
    *out = e;
    if (!e->eng.reload()) { nsh_set_err(e, e->eng.last_error()); return -1; }
    return 0;
} NSH_CATCH(out ? *out : nullptr, "nsh_engine_open_multi", -1)
}
extern "C" uint32_t nsh_engine_num_devices(nsh_engine* e) { try { return e ? (uint32_t)e->eng.num_devices() : 0; } NSH_CATCH(e, "nsh_engine_num_devices", 0)
}
extern "C" void nsh_shard_bounds(uint64_t n_queries, uint32_t r, uint32_t n, uint64_t* begin, uint64_t* end) {
    const auto b = nextsearch::Engine::shard_bounds((size_t)n_queries, r, n);
    if (begin) *begin = b.first;
    if (end) *end = b.second;
}

extern "C" void nsh_engine_close(nsh_engine* e) { delete e; }
// Engine::reload() (include/api_engine.hpp:65) on the directory given at open: 0 on success; on failure the engine
// keeps serving what it served before and nsh_engine_error() says why.
extern "C" int nsh_engine_reload(nsh_engine* e) { try {
    if (!e) return -1;
    if (!e->eng.reload()) { nsh_set_err(e, e->eng.last_error()); return -1; }
    return 0;
} NSH_CATCH(e, "nsh_engine_reload", -1)
}
extern "C" const char* nsh_engine_error(nsh_engine* e) { try {
    if (!e) return "null engine";
    // a copy per calling thread: the pointer stays valid until this thread asks again, whatever other threads do
    thread_local std::string mine;
    const std::string eng_err = e->eng.last_error();
    {
        std::lock_guard<std::mutex> l(e->err_mtx);
        if (!eng_err.empty()) e->err = eng_err;
        mine = e->err;
    }
    return mine.c_str();
} NSH_CATCH(e, "nsh_engine_error", "")
}
extern "C" ns_ctx* nsh_engine_ctx(nsh_engine* e) { try { return e ? e->eng.ctx() : nullptr;  } NSH_CATCH(e, "nsh_engine_ctx", nullptr)
}
extern "C" uint32_t nsh_engine_num_segments(nsh_engine* e) { try { return e ? (uint32_t)e->eng.segments.size() : 0;  } NSH_CATCH(e, "nsh_engine_num_segments", 0)
}
extern "C" const char* nsh_engine_segment_name(nsh_engine* e, uint32_t seg) { try {
    return (e && seg < e->eng.seg_names.size()) ? e->eng.seg_names[seg].c_str() : "";
} NSH_CATCH(e, "nsh_engine_segment_name", "")
}

// Result decoration (src/api_engine.cpp:516-531): the four fields of a document, valid until close/reload.
// Returns 1 if the document has a metadata row, else 0 (all four then point to "").
extern "C" int nsh_engine_doc_metadata(nsh_engine* e, uint32_t seg, uint32_t doc, const char** title, const char** url,
                                       const char** publish_time, const char** author) { try {
    static const char* kEmpty = "";
    const nsx::MetaFields* m = e ? e->eng.meta.get(seg, doc) : nullptr;
    if (title) *title = m ? m->title.c_str() : kEmpty;
    if (url) *url = m ? m->url.c_str() : kEmpty;
    if (publish_time) *publish_time = m ? m->publish_time.c_str() : kEmpty;
    if (author) *author = m ? m->author.c_str() : kEmpty;
    return m ? 1 : 0;
} NSH_CATCH(e, "nsh_engine_doc_metadata", -1)
}
// JSON text of one result assembled from given hits (the decoration + serialisation step alone; no device needed).
extern "C" int nsh_engine_hits_to_json(nsh_engine* e, const char* query, int k, int has_found, uint64_t found,
                                       const ns_hit* hits, uint32_t nhits, char** json_out) { try {
    if (!e || !json_out) return -1;
    nextsearch::SearchResult r;
    r.query = query ? query : "";
    r.k = std::max(1, std::min(k, 100));
    r.segments = (int)e->eng.segments.size();
    r.has_found = has_found != 0;
    r.found = found;
    if (nhits && !hits) return -1;
    for (uint32_t i = 0; i < nhits; i++) {
        if (hits[i].seg_id >= e->eng.segments.size()) { nsh_set_err(e, "nsh_engine_hits_to_json: hit names a segment that is not loaded"); return -1; }
        r.hits.push_back(nextsearch::SearchHit{hits[i].score, hits[i].seg_id, hits[i].doc_id});
    }
    const std::string js = e->eng.to_json(r);
    char* out = (char*)std::malloc(js.size() + 1);
    if (!out) return -1;
    std::memcpy(out, js.c_str(), js.size() + 1);
    *json_out = out;
    return 0;
} NSH_CATCH(e, "nsh_engine_hits_to_json", -1)
}

extern "C" int nsh_engine_segment_info(nsh_engine* e, uint32_t seg, uint32_t* n_docs, float* avgdl, uint64_t* n_postings,
                                       uint32_t* n_terms, int* use_barrels) { try {
    if (!e || seg >= e->eng.segments.size()) return -1;
    const auto& s = e->eng.segments[seg];
    if (n_docs) *n_docs = s.N;
    if (avgdl) *avgdl = s.avgdl;
    if (n_postings) *n_postings = s.postings_bytes / 8;
    if (n_terms) *n_terms = (uint32_t)s.lex.size();
    if (use_barrels) *use_barrels = s.use_barrels ? 1 : 0;
    return 0;
} NSH_CATCH(e, "nsh_engine_segment_info", -1)
}

extern "C" const uint32_t* nsh_engine_segment_doc_len(nsh_engine* e, uint32_t seg) { try {
    return (e && seg < e->eng.segments.size()) ? e->eng.segments[seg].doc_len.data() : nullptr;
} NSH_CATCH(e, "nsh_engine_segment_doc_len", nullptr)
}
extern "C" const void* nsh_engine_segment_postings(nsh_engine* e, uint32_t seg, uint64_t* nbytes) { try {
    if (!e || seg >= e->eng.segments.size()) return nullptr;
    const std::vector<uint8_t>* raw = e->eng.raw_postings(seg);   // read from the inverted files on first request
    if (!raw) return nullptr;
    if (nbytes) *nbytes = raw->size();
    return raw->data();
} NSH_CATCH(e, "nsh_engine_segment_postings", nullptr)
}

extern "C" int nsh_engine_lookup(nsh_engine* e, uint32_t seg, const char* term, uint32_t* term_id, uint32_t* df,
                                 uint32_t* count, uint64_t* byte_off, float* idf) { try {
    if (!e || seg >= e->eng.segments.size() || !term) return 0;
    const auto& s = e->eng.segments[seg];
    auto it = s.lex.find(term);
    if (it == s.lex.end()) return 0;
    const nsx::LexEntry& le = it->second;
    if (term_id) *term_id = le.termId;
    if (df) *df = le.df;
    if (count) *count = le.count;
    if (byte_off) *byte_off = s.list_byte_offset(le);
    if (idf) *idf = nextsearch::bm25_idf(s.N, le.df);
    return 1;
} NSH_CATCH(e, "nsh_engine_lookup", -1)
}

extern "C" float nsh_bm25_idf(uint32_t n_docs, uint32_t df) { return nextsearch::bm25_idf(n_docs, df); }   // arithmetic only

extern "C" uint32_t nsh_base_terms(const char* query, char* buf, uint32_t cap) { try {
    auto terms = nextsearch::base_terms(query ? query : "");
    std::string joined;
    for (size_t i = 0; i < terms.size(); i++) {
        if (i) joined.push_back(' ');
        joined += terms[i];
    }
    if (buf && cap) {
        size_t n = std::min<size_t>(joined.size(), cap - 1);
        std::memcpy(buf, joined.data(), n);
        buf[n] = 0;
    }
    return (uint32_t)terms.size();
} NSH_CATCH(nullptr, "nsh_base_terms", 0)
}

extern "C" int nsh_engine_build_refs(nsh_engine* e, const char* const* queries, uint32_t n_queries, ns_query_desc* qd,
                                     ns_term_ref* refs, uint32_t refs_cap, uint32_t* n_refs, uint8_t* usable) { try {
    if (!e) return -1;
    std::vector<ns_query_desc> q;
    std::vector<ns_term_ref> r;
    std::vector<uint8_t> u;
    e->eng.build_refs(to_vec(queries, n_queries), q, r, u);
    if (n_refs) *n_refs = (uint32_t)r.size();
    if (qd) std::memcpy(qd, q.data(), q.size() * sizeof(ns_query_desc));
    if (usable) std::memcpy(usable, u.data(), u.size());
    if (r.size() > refs_cap) return 1;
    if (refs && !r.empty()) std::memcpy(refs, r.data(), r.size() * sizeof(ns_term_ref));
    return 0;
} NSH_CATCH(e, "nsh_engine_build_refs", -1)
}

extern "C" int nsh_engine_search_json(nsh_engine* e, const char* query, int k, char** json_out) { try {
    if (!e || !json_out) return -1;
    std::string s;
    const bool ok = e->eng.search_text(query ? query : "", k, s);   // Engine::search: the result cache included
    if (!ok) { nsh_set_err(e, e->eng.last_error()); *json_out = nullptr; return -1; }
    *json_out = (char*)std::malloc(s.size() + 1);
    std::memcpy(*json_out, s.c_str(), s.size() + 1);
    return 0;
} NSH_CATCH(e, "nsh_engine_search_json", -1)
}

// Batch of searches to JSON bodies: *text_out receives all bodies back to back (free with nsh_free),
// offsets[q] .. offsets[q+1] delimit body q (offsets has n_queries + 1 entries).
extern "C" int nsh_engine_search_batch_json(nsh_engine* e, const char* const* queries, uint32_t n_queries, int k,
                                            char** text_out, uint64_t* offsets) { try {
    if (!e || !text_out || !offsets) return -1;
    std::vector<std::string> qs = to_vec(queries, n_queries), bodies;
    if (!e->eng.search_batch_json(qs, k, bodies)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    size_t total = 0;
    for (auto& b : bodies) total += b.size();
    char* buf = (char*)std::malloc(total + 1);
    if (!buf) return -1;
    size_t pos = 0;
    for (uint32_t q = 0; q < n_queries; q++) {
        offsets[q] = pos;
        std::memcpy(buf + pos, bodies[q].data(), bodies[q].size());
        pos += bodies[q].size();
    }
    offsets[n_queries] = pos;
    buf[pos] = 0;
    *text_out = buf;
    return 0;
} NSH_CATCH(e, "nsh_engine_search_batch_json", -1)
}
extern "C" void nsh_free(void* p) { std::free(p); }

extern "C" int nsh_engine_search_batch(nsh_engine* e, const char* const* queries, uint32_t n_queries, int k, uint32_t flags,
                                       ns_hit* hits, uint32_t* nhits, uint64_t* found, uint8_t* has_found) { try {
    if (!e) return -1;
    // Engine::search_batch_flat: the caller's arrays are the outputs; whichever the caller left out is kept in scratch
    const uint32_t K = (uint32_t)std::max(1, std::min(k, 100));
    std::vector<nextsearch::Engine::QueryView> views(n_queries);
    for (uint32_t q = 0; q < n_queries; q++) views[q] = {queries[q] ? queries[q] : "", queries[q] ? std::strlen(queries[q]) : 0};
    std::vector<ns_hit> h_;
    std::vector<uint32_t> n_;
    std::vector<uint64_t> f_;
    std::vector<uint8_t> u_;
    if (!hits) { h_.resize((size_t)n_queries * K); hits = h_.data(); }
    if (!nhits) { n_.resize(n_queries); nhits = n_.data(); }
    if (!found) { f_.resize(n_queries); found = f_.data(); }
    if (!has_found) { u_.resize(n_queries); has_found = u_.data(); }
    if (!e->eng.search_batch_flat(views.data(), n_queries, k, flags, hits, nhits, found, has_found)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    for (uint32_t q = 0; q < n_queries; q++) {
        if (has_found[q]) continue;   // the early return (src/api_engine.cpp:407): no hits, no found
        nhits[q] = 0; found[q] = 0;
        for (uint32_t i = 0; i < K; i++) hits[(size_t)q * K + i] = ns_hit{-__builtin_inff(), 0xFFFFFFFFu, 0xFFFFFFFFu};
    }
    return 0;
} NSH_CATCH(e, "nsh_engine_search_batch", -1)
}

// The reference's `lexicon <SEGMENT_DIR>` tool with the inversion on the device (host/invert.hpp).
static thread_local std::string g_invert_err;
extern "C" const char* nsh_invert_error() { return g_invert_err.c_str(); }
extern "C" int nsh_invert_segment(const char* seg_dir, int device, uint64_t* pairs, uint64_t* kept, float* device_ms,
                                  double* call_s, double* total_s) { try {
    if (!seg_dir) return -1;
    ns_ctx* ctx = nullptr;
    if (ns_ctx_create(device, &ctx) != NS_OK) { g_invert_err = std::string("ns_ctx_create: ") + ns_last_error(nullptr); return -1; }
    nsx::InvertStats st;
    const bool ok = nsx::invert_segment(ctx, seg_dir, st, g_invert_err);
    ns_ctx_destroy(ctx);
    if (pairs) *pairs = st.pairs;
    if (kept) *kept = st.kept;
    if (device_ms) *device_ms = st.device_ms;
    if (call_s) *call_s = st.call_s;
    if (total_s) *total_s = st.total_s;
    return ok ? 0 : -1;
} NSH_CATCH(nullptr, "nsh_invert_segment", -1)
}

// Indexing: documents as four length-delimited fields each (include/nextsearch_host.h)
static std::vector<nsx::DocInput> to_docs(const char* bytes, const uint64_t* fo, uint32_t n_docs) {
    std::vector<nsx::DocInput> docs(n_docs);
    for (uint32_t d = 0; d < n_docs; d++) {
        const uint64_t* o = fo + 4 * (size_t)d;
        std::string* f[4] = {&docs[d].cord_uid, &docs[d].title, &docs[d].json_relpath, &docs[d].text};
        for (int k = 0; k < 4; k++) {
            if (o[k + 1] < o[k]) throw std::runtime_error("field offsets decrease at document " + std::to_string(d));
            f[k]->assign(bytes + o[k], (size_t)(o[k + 1] - o[k]));
        }
    }
    return docs;
}
static void put_stats(nsh_index_stats* out, const nsx::IndexStats& st) {
    if (!out || out->struct_size < 4) return;
    nsh_index_stats t{};
    t.struct_size = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof(t));
    t.n_docs_in = st.n_docs_in; t.n_docs = st.n_docs; t.n_terms = st.n_terms;
    t.text_bytes = st.text_bytes; t.tokens = st.tokens; t.kept_tokens = st.kept_tokens; t.pairs = st.pairs; t.device_bytes = st.device_bytes;
    t.avgdl = st.avgdl; t.device_ms = st.device_ms; t.call_s = st.call_s; t.total_s = st.total_s;
    std::memcpy(out, &t, t.struct_size);
}
static thread_local std::string g_index_err;
extern "C" const char* nsh_index_error(void) { return g_index_err.c_str(); }
extern "C" int nsh_index_documents(const char* seg_dir, int device, const char* bytes, const uint64_t* field_offsets, uint32_t n_docs,
                                   nsh_index_stats* stats) { try {
    if (!seg_dir || (n_docs && (!field_offsets || !bytes))) { g_index_err = "nsh_index_documents: null argument"; return -1; }
    const std::vector<nsx::DocInput> docs = to_docs(bytes, field_offsets, n_docs);
    ns_ctx* ctx = nullptr;
    if (ns_ctx_create(device, &ctx) != NS_OK) { g_index_err = std::string("ns_ctx_create: ") + ns_last_error(nullptr); return -1; }
    nsx::IndexStats st;
    const bool ok = nsx::index_documents(ctx, docs, seg_dir, st, g_index_err);
    ns_ctx_destroy(ctx);
    put_stats(stats, st);
    return ok ? 0 : -1;
} catch (const std::exception& ex) { g_index_err = std::string("nsh_index_documents: ") + ex.what(); return -1; }
  catch (...) { g_index_err = "nsh_index_documents: unknown exception"; return -1; }
}
extern "C" int nsh_engine_open_noload(const char* index_dir, int device, nsh_engine** out) { try {
    if (!out) return -1;
    nsh_engine* e = new nsh_engine(device);
    e->eng.index_dir = index_dir ? index_dir : "";
    *out = e;
    return 0;
} NSH_CATCH(nullptr, "nsh_engine_open_noload", -1)
}
extern "C" int nsh_engine_add_documents(nsh_engine* e, const char* bytes, const uint64_t* field_offsets, uint32_t n_docs,
                                        nsh_index_stats* stats) { try {
    if (!e) return -1;
    if (n_docs && (!field_offsets || !bytes)) { nsh_set_err(e, "nsh_engine_add_documents: null argument"); return -1; }
    nsx::IndexStats st;
    const bool ok = e->eng.add_documents(to_docs(bytes, field_offsets, n_docs), &st);
    put_stats(stats, st);
    if (!ok) { nsh_set_err(e, e->eng.last_error()); return -1; }
    return 0;
} NSH_CATCH(e, "nsh_engine_add_documents", -1)
}

// Compaction (host/compact.hpp)
static void put_cstats(nsh_compact_stats* out, const nsx::CompactStats& st) {
    if (!out || out->struct_size < 4) return;
    nsh_compact_stats t{};
    t.struct_size = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof(t));
    t.sources = st.sources; t.n_docs = st.n_docs; t.n_terms = st.n_terms;
    t.terms_in = st.terms_in; t.pairs = st.pairs; t.device_bytes = st.device_bytes;
    t.merge_ms = st.merge_ms; t.invert_ms = st.invert_ms; t.call_s = st.call_s; t.total_s = st.total_s;
    std::memcpy(out, &t, t.struct_size);
}
static thread_local std::string g_compact_err;
extern "C" const char* nsh_compact_error(void) { return g_compact_err.c_str(); }
extern "C" int nsh_merge_segments(const char* const* source_dirs, uint32_t n_sources, const char* out_dir, int device, nsh_compact_stats* stats) { try {
    if (!out_dir || (n_sources && !source_dirs)) { g_compact_err = "nsh_merge_segments: null argument"; return -1; }
    std::vector<nsx::fs::path> dirs;
    for (uint32_t i = 0; i < n_sources; i++) {
        if (!source_dirs[i]) { g_compact_err = "nsh_merge_segments: null argument"; return -1; }
        dirs.emplace_back(source_dirs[i]);
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<nsx::SourceSegment> loaded;
    if (!nsx::load_sources(dirs, loaded, g_compact_err)) return -1;            // before the device is touched
    ns_ctx* ctx = nullptr;
    if (ns_ctx_create(device, &ctx) != NS_OK) { g_compact_err = std::string("ns_ctx_create: ") + ns_last_error(nullptr); return -1; }
    nsx::CompactStats st;
    const bool ok = nsx::merge_loaded(ctx, loaded, out_dir, st, g_compact_err);
    ns_ctx_destroy(ctx);
    st.total_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    put_cstats(stats, st);
    return ok ? 0 : -1;
} catch (const std::exception& ex) { g_compact_err = std::string("nsh_merge_segments: ") + ex.what(); return -1; }
  catch (...) { g_compact_err = "nsh_merge_segments: unknown exception"; return -1; }
}
extern "C" int nsh_engine_compact(nsh_engine* e, uint64_t first, uint64_t count, int remove_sources, nsh_compact_stats* stats) { try {
    if (!e) return -1;
    nsx::CompactStats st;
    const bool ok = e->eng.compact((size_t)first, (size_t)count, remove_sources != 0, &st);
    put_cstats(stats, st);
    nsh_set_err(e, e->eng.last_error());                                       // (success: empty, or the sources that could not be removed)
    return ok ? 0 : -1;
} NSH_CATCH(e, "nsh_engine_compact", -1)
}

// Deleting (host/purge.hpp)
static void put_dstats(nsh_delete_stats* out, const nsx::DeleteStats& st) {
    if (!out || out->struct_size < 4) return;
    nsh_delete_stats t{};
    t.struct_size = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof(t));
    t.segments_rewritten = st.segments_rewritten; t.segments_dropped = st.segments_dropped; t.docs_deleted = st.docs_deleted;
    t.uids_not_found = st.uids_not_found; t.terms_dropped = st.terms_dropped;
    t.pairs_in = st.pairs_in; t.pairs_out = st.pairs_out; t.device_bytes = st.device_bytes;
    t.merge_ms = st.merge_ms; t.invert_ms = st.invert_ms; t.call_s = st.call_s; t.total_s = st.total_s;
    std::memcpy(out, &t, t.struct_size);
}
static std::vector<std::string> to_uids(const char* bytes, const uint64_t* offsets, uint32_t n) {
    std::vector<std::string> out(n);
    for (uint32_t i = 0; i < n; i++) out[i].assign(bytes + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
    return out;
}
extern "C" int64_t nsh_engine_find_documents(nsh_engine* e, const char* bytes, const uint64_t* offsets, uint32_t n_uids,
                                             uint32_t* seg_doc_out, uint64_t capacity) { try {
    if (!e) return -1;
    if (n_uids && (!bytes || !offsets)) { nsh_set_err(e, "nsh_engine_find_documents: null argument"); return -1; }
    std::vector<std::pair<uint32_t, uint32_t>> hits;
    e->eng.find_documents(to_uids(bytes, offsets, n_uids), hits);
    for (size_t i = 0; seg_doc_out && i < hits.size() && i < capacity; i++) { seg_doc_out[2 * i] = hits[i].first; seg_doc_out[2 * i + 1] = hits[i].second; }
    return (int64_t)hits.size();
} NSH_CATCH(e, "nsh_engine_find_documents", -1)
}
extern "C" int nsh_engine_delete_documents(nsh_engine* e, const char* bytes, const uint64_t* offsets, uint32_t n_uids, nsh_delete_stats* stats) { try {
    if (!e) return -1;
    if (n_uids && (!bytes || !offsets)) { nsh_set_err(e, "nsh_engine_delete_documents: null argument"); return -1; }
    nsx::DeleteStats st;
    const bool ok = e->eng.delete_documents(to_uids(bytes, offsets, n_uids), &st);
    put_dstats(stats, st);
    nsh_set_err(e, e->eng.last_error());                                       // (success: empty, or the directories that could not be removed)
    return ok ? 0 : -1;
} NSH_CATCH(e, "nsh_engine_delete_documents", -1)
}
extern "C" int nsh_engine_delete_by_id(nsh_engine* e, const uint32_t* seg_doc, uint64_t n_pairs, nsh_delete_stats* stats) { try {
    if (!e) return -1;
    if (n_pairs && !seg_doc) { nsh_set_err(e, "nsh_engine_delete_by_id: null argument"); return -1; }
    std::vector<std::pair<uint32_t, uint32_t>> ids((size_t)n_pairs);
    for (size_t i = 0; i < ids.size(); i++) ids[i] = {seg_doc[2 * i], seg_doc[2 * i + 1]};
    nsx::DeleteStats st;
    const bool ok = e->eng.delete_by_id(ids, &st);
    put_dstats(stats, st);
    nsh_set_err(e, e->eng.last_error());
    return ok ? 0 : -1;
} NSH_CATCH(e, "nsh_engine_delete_by_id", -1)
}

// Semantic expansion (src/api_engine.cpp:409-417): rows/dim of the loaded embedding table (0/0: none), and the
// weighted terms a query is scored with, one "term<TAB>fp32 weight bits in hex" line each, in scoring order.
extern "C" int nsh_engine_semantic_info(nsh_engine* e, uint32_t* rows, uint32_t* dim) { try {
    if (!e) return -1;
    if (rows) *rows = e->eng.sem.enabled ? (uint32_t)e->eng.sem.terms.size() : 0;
    if (dim) *dim = e->eng.sem.enabled ? (uint32_t)e->eng.sem.dim : 0;
    return e->eng.sem.enabled ? 1 : 0;
} NSH_CATCH(e, "nsh_engine_semantic_info", -1)
}
extern "C" int nsh_engine_semantic_row(nsh_engine* e, uint32_t row, const char** term, const float** vec) { try {
    if (!e || !e->eng.sem.enabled || row >= e->eng.sem.terms.size()) return -1;
    if (term) *term = e->eng.sem.terms[row].c_str();
    if (vec) *vec = e->eng.sem.vecs.data() + (size_t)row * (size_t)e->eng.sem.dim;
    return 0;
} NSH_CATCH(e, "nsh_engine_semantic_row", -1)
}
extern "C" int nsh_engine_expand(nsh_engine* e, const char* query, char** text_out) { try {
    if (!e || !query || !text_out) return -1;
    std::vector<nsx::WeightedTerms> w;
    if (!e->eng.expand_queries({std::string(query)}, w)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    std::string o;
    char buf[16];
    for (const auto& tw : w[0]) {
        uint32_t bits;
        std::memcpy(&bits, &tw.second, 4);
        std::snprintf(buf, sizeof(buf), "%08x", bits);
        o += tw.first; o += '\t'; o += buf; o += '\n';
    }
    *text_out = (char*)std::malloc(o.size() + 1);
    if (!*text_out) return -1;
    std::memcpy(*text_out, o.c_str(), o.size() + 1);
    return 0;
} NSH_CATCH(e, "nsh_engine_expand", -1)
}

// Search-result cache of Engine::search (src/api_engine.cpp:190-250): on by default as in the reference.
extern "C" void nsh_engine_set_cache(nsh_engine* e, int on) { try { if (e) e->eng.set_cache(on != 0);  } NSH_CATCH_VOID(e, "nsh_engine_set_cache")
}
extern "C" uint32_t nsh_engine_cache_size(nsh_engine* e) { try { return e ? (uint32_t)e->eng.cache_size() : 0;  } NSH_CATCH(e, "nsh_engine_cache_size", 0)
}

extern "C" int nsh_engine_build_impacts(nsh_engine* e) { try {
    if (!e) return -1;
    if (!e->eng.build_impacts()) { nsh_set_err(e, e->eng.last_error()); return -1; }
    return 0;
} NSH_CATCH(e, "nsh_engine_build_impacts", -1)
}
extern "C" int nsh_engine_build_packed(nsh_engine* e) { try {
    if (!e) return -1;
    if (!e->eng.build_packed()) { nsh_set_err(e, e->eng.last_error()); return -1; }
    return 0;
} NSH_CATCH(e, "nsh_engine_build_packed", -1)
}
extern "C" void nsh_engine_use_packed(nsh_engine* e, int on) { try { if (e) e->eng.use_packed(on); } NSH_CATCH_VOID(e, "nsh_engine_use_packed")
}
extern "C" int nsh_engine_build_blockmax(nsh_engine* e) { try {
    if (!e) return -1;
    if (!e->eng.build_blockmax()) { nsh_set_err(e, e->eng.last_error()); return -1; }
    return 0;
} NSH_CATCH(e, "nsh_engine_build_blockmax", -1)
}
extern "C" void nsh_engine_use_pruning(nsh_engine* e, int on) { try { if (e) e->eng.use_pruning(on != 0); } NSH_CATCH_VOID(e, "nsh_engine_use_pruning")
}
extern "C" void nsh_engine_use_merge(nsh_engine* e, int on) { try { if (e) e->eng.use_merge(on != 0); } NSH_CATCH_VOID(e, "nsh_engine_use_merge")
}
extern "C" void nsh_engine_share_scores(nsh_engine* e, int mode) { try { if (e) e->eng.share_scores(mode); } NSH_CATCH_VOID(e, "nsh_engine_share_scores")
}
extern "C" void nsh_engine_use_skips(nsh_engine* e, int on) { try { if (e) e->eng.use_skips(on != 0);  } NSH_CATCH_VOID(e, "nsh_engine_use_skips")
}
extern "C" void nsh_engine_use_impacts(nsh_engine* e, int on) { try { if (e) e->eng.use_impacts(on != 0);  } NSH_CATCH_VOID(e, "nsh_engine_use_impacts")
}

extern "C" int nsh_engine_prepare(nsh_engine* e, const char* const* queries, uint32_t n_queries, int k, uint32_t flags,
                                  ns_batch** out) { try {
    if (!e || !out) return -1;
    if (!e->eng.prepare(to_vec(queries, n_queries), k, flags, out)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    return 0;
} NSH_CATCH(e, "nsh_engine_prepare", -1)
}

// ---- autocomplete ----------------------------------------------------------------------------
extern "C" int nsh_engine_suggest_json(nsh_engine* e, const char* input, uint64_t input_len, int limit, char** json_out) { try {
    if (!e || !json_out || (input_len && !input)) return -1;
    std::string s;
    const bool ok = e->eng.suggest_text(std::string(input ? input : "", (size_t)input_len), limit, s);
    if (!ok) { nsh_set_err(e, e->eng.last_error()); *json_out = nullptr; return -1; }
    *json_out = (char*)std::malloc(s.size() + 1);
    if (!*json_out) return -1;
    std::memcpy(*json_out, s.c_str(), s.size() + 1);
    return 0;
} NSH_CATCH(e, "nsh_engine_suggest_json", -1)
}

extern "C" int nsh_engine_suggest_batch(nsh_engine* e, const char* bytes, const uint64_t* offsets, uint32_t n_inputs, int limit,
                                        uint32_t* term_idx, uint32_t* count, uint32_t* base_len, float* device_ms) { try {
    if (!e || (n_inputs && (!offsets || !term_idx || !count || !base_len))) return -1;
    std::vector<nextsearch::Engine::QueryView> views(n_inputs);
    for (uint32_t q = 0; q < n_inputs; q++) {
        if (offsets[q + 1] < offsets[q] || (offsets[q + 1] > offsets[q] && !bytes)) { nsh_set_err(e, "nsh_engine_suggest_batch: bad offsets"); return -1; }
        views[q] = {bytes ? bytes + offsets[q] : "", (size_t)(offsets[q + 1] - offsets[q])};
    }
    if (!e->eng.suggest_batch(views.data(), n_inputs, limit, term_idx, count, base_len, device_ms)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    return 0;
} NSH_CATCH(e, "nsh_engine_suggest_batch", -1)
}

extern "C" int nsh_engine_suggest_table(nsh_engine* e, const char** pool, const uint64_t** offsets, const uint32_t** scores,
                                        uint64_t* n_terms, double* build_ms, double* upload_ms) { try {
    if (!e) return -1;
    const auto& t = e->eng.suggest_table;
    if (pool) *pool = t.pool.data();
    if (offsets) *offsets = t.off.data();
    if (scores) *scores = t.score.data();
    if (n_terms) *n_terms = t.size();
    if (build_ms) *build_ms = e->eng.suggest_build_ms;
    if (upload_ms) *upload_ms = e->eng.suggest_upload_ms;
    return 0;
} NSH_CATCH(e, "nsh_engine_suggest_table", -1)
}

extern "C" int nsh_engine_correct_batch(nsh_engine* e, const char* bytes, const uint64_t* offsets, uint32_t n_terms, int limit,
                                        int max_edits, int prefix_len, uint32_t* term_idx, uint8_t* dist, uint32_t* count,
                                        float* device_ms) { try {
    if (!e || (n_terms && (!offsets || !term_idx || !dist || !count))) return -1;
    std::vector<nextsearch::Engine::QueryView> views(n_terms);
    for (uint32_t q = 0; q < n_terms; q++) {
        if (offsets[q + 1] < offsets[q] || (offsets[q + 1] > offsets[q] && !bytes)) { nsh_set_err(e, "nsh_engine_correct_batch: bad offsets"); return -1; }
        views[q] = {bytes ? bytes + offsets[q] : "", (size_t)(offsets[q + 1] - offsets[q])};
    }
    if (!e->eng.correct_batch(views.data(), n_terms, limit, max_edits, prefix_len, term_idx, dist, count, device_ms)) {
        nsh_set_err(e, e->eng.last_error());
        return -1;
    }
    return 0;
} NSH_CATCH(e, "nsh_engine_correct_batch", -1)
}

extern "C" int nsh_engine_did_you_mean_json(nsh_engine* e, const char* query, uint64_t query_len, int limit, char** json_out) { try {
    if (!e || !json_out || (query_len && !query)) return -1;
    std::string s;
    const bool ok = e->eng.did_you_mean_text(std::string(query ? query : "", (size_t)query_len), limit, s);
    if (!ok) { nsh_set_err(e, e->eng.last_error()); *json_out = nullptr; return -1; }
    *json_out = (char*)std::malloc(s.size() + 1);
    if (!*json_out) return -1;
    std::memcpy(*json_out, s.c_str(), s.size() + 1);
    return 0;
} NSH_CATCH(e, "nsh_engine_did_you_mean_json", -1)
}

extern "C" int nsh_engine_complete_batch(nsh_engine* e, const char* bytes, const uint64_t* offsets, uint32_t n_inputs, int limit,
                                         int max_edits, int prefix_len, uint32_t* term_idx, uint8_t* dist, uint32_t* count,
                                         uint32_t* base_len, float* device_ms) { try {
    if (!e || (n_inputs && (!offsets || !term_idx || !dist || !count || !base_len))) return -1;
    std::vector<nextsearch::Engine::QueryView> views(n_inputs);
    for (uint32_t q = 0; q < n_inputs; q++) {
        if (offsets[q + 1] < offsets[q] || (offsets[q + 1] > offsets[q] && !bytes)) { nsh_set_err(e, "nsh_engine_complete_batch: bad offsets"); return -1; }
        views[q] = {bytes ? bytes + offsets[q] : "", (size_t)(offsets[q + 1] - offsets[q])};
    }
    if (!e->eng.complete_batch(views.data(), n_inputs, limit, max_edits, prefix_len, term_idx, dist, count, base_len, device_ms)) {
        nsh_set_err(e, e->eng.last_error());
        return -1;
    }
    return 0;
} NSH_CATCH(e, "nsh_engine_complete_batch", -1)
}

extern "C" int nsh_engine_complete_json(nsh_engine* e, const char* input, uint64_t input_len, int limit, char** json_out) { try {
    if (!e || !json_out || (input_len && !input)) return -1;
    std::string s;
    const bool ok = e->eng.complete_text(std::string(input ? input : "", (size_t)input_len), limit, s);
    if (!ok) { nsh_set_err(e, e->eng.last_error()); *json_out = nullptr; return -1; }
    *json_out = (char*)std::malloc(s.size() + 1);
    if (!*json_out) return -1;
    std::memcpy(*json_out, s.c_str(), s.size() + 1);
    return 0;
} NSH_CATCH(e, "nsh_engine_complete_json", -1)
}

extern "C" int nsh_correct_auto_edits(uint64_t normalized_len) { return nsx::correct_auto_edits((size_t)normalized_len); }

extern "C" double nsh_engine_correct_build_ms(nsh_engine* e) { return e ? e->eng.correct_build_ms : 0.0; }

extern "C" uint64_t nsh_suggest_split(const char* input, uint64_t input_len, uint64_t* base_len, char* prefix, uint64_t cap) {
    size_t b = 0;
    std::string p;
    nsx::split_suggest_input(input ? input : "", input ? (size_t)input_len : 0, b, p);
    if (base_len) *base_len = b;
    if (prefix && cap) std::memcpy(prefix, p.data(), std::min<size_t>(p.size(), (size_t)cap));
    return p.size();
}

extern "C" int nsh_suggest_clamp_limit(int limit) { return nsx::clamp_suggest_limit(limit); }

// ---- more like this ----
extern "C" int nsh_similar_select_host(const uint32_t* counts, uint32_t n_docs, const uint32_t* pairs, uint64_t n_pairs, const uint32_t* df,
                                       const float* idf, uint32_t n_terms, const uint32_t* doc_ids, uint32_t n, uint32_t max_terms,
                                       uint32_t min_tf, uint32_t min_df, uint32_t max_df, uint32_t* term_out, float* w_out, uint32_t* count_out) { try {
    if ((n_docs && !counts) || (n_pairs && !pairs) || (n_terms && (!df || !idf)) || (n && (!doc_ids || !term_out || !w_out || !count_out))) return -1;
    std::vector<uint64_t> off((size_t)n_docs + 1, 0);
    for (uint32_t d = 0; d < n_docs; d++) off[d + 1] = off[d] + counts[d];
    if (off[n_docs] != n_pairs) return -1;
    return nsx::similar_select_host(off.data(), n_docs, pairs, df, idf, n_terms, doc_ids, n, max_terms, min_tf, min_df, max_df, term_out, w_out, count_out) ? 0 : -1;
} catch (...) { return -1; }
}
extern "C" uint32_t nsh_similar_clamp_terms(uint32_t max_terms) { return nsx::similar_clamp_terms(max_terms); }
extern "C" int nsh_similar_clamp_k(int k) { return std::max(1, std::min(k, 99)); }
extern "C" float nsh_similar_qweight(float w, float w_first, int boost) { return nsx::similar_qweight(w, w_first, boost != 0); }
extern "C" void nsh_similar_defaults(uint32_t* max_terms, uint32_t* min_tf, uint32_t* min_df, uint32_t* max_df, int* boost) {
    const nsx::SimilarOptions o;
    if (max_terms) *max_terms = o.max_terms;
    if (min_tf) *min_tf = o.min_tf;
    if (min_df) *min_df = o.min_df;
    if (max_df) *max_df = o.max_df;
    if (boost) *boost = o.boost ? 1 : 0;
}

extern "C" int64_t nsh_engine_similar_term_stats(nsh_engine* e, uint32_t seg, uint32_t* df_out, float* idf_out, uint64_t cap) { try {
    if (!e) return -1;
    std::vector<uint32_t> df;
    std::vector<float> idf;
    if (!e->eng.similar_term_stats(seg, df, idf)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    const size_t m = (size_t)std::min<uint64_t>(cap, df.size());
    if (df_out && m) std::memcpy(df_out, df.data(), m * 4);
    if (idf_out && m) std::memcpy(idf_out, idf.data(), m * 4);
    return (int64_t)df.size();
} NSH_CATCH(e, "nsh_engine_similar_term_stats", -1)
}

extern "C" int nsh_engine_similar_batch(nsh_engine* e, const uint32_t* seg_doc, uint64_t n, int k, uint32_t max_terms, uint32_t min_tf,
                                        uint32_t min_df, uint32_t max_df, int boost, ns_hit* hits, uint32_t* nhits, uint64_t* found,
                                        uint8_t* usable, uint32_t* term_count, float* term_w, char** term_bytes_out, uint64_t** term_offsets_out) { try {
    if (!e) return -1;
    if (term_bytes_out) *term_bytes_out = nullptr;
    if (term_offsets_out) *term_offsets_out = nullptr;
    if (n && (!seg_doc || !hits || !nhits || !found || !usable)) { nsh_set_err(e, "nsh_engine_similar_batch: null argument"); return -1; }
    std::vector<std::pair<uint32_t, uint32_t>> ids((size_t)n);
    for (size_t i = 0; i < ids.size(); i++) ids[i] = {seg_doc[2 * i], seg_doc[2 * i + 1]};
    nsx::SimilarOptions opt;
    opt.max_terms = max_terms; opt.min_tf = min_tf; opt.min_df = min_df; opt.max_df = max_df; opt.boost = boost != 0;
    const bool want_terms = term_count || term_w || term_bytes_out || term_offsets_out;
    std::vector<nsx::WeightedTerms> terms;
    if (!e->eng.similar_batch(ids.data(), ids.size(), k, opt, hits, nhits, found, usable, want_terms ? &terms : nullptr)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    if (!want_terms) return 0;
    const uint32_t T = nsx::similar_clamp_terms(max_terms);
    size_t total = 0, bytes = 0;
    for (size_t q = 0; q < terms.size(); q++) {
        if (term_count) term_count[q] = (uint32_t)terms[q].size();
        for (uint32_t r = 0; r < T && term_w; r++) term_w[q * (size_t)T + r] = r < terms[q].size() ? terms[q][r].second : 0.0f;
        total += terms[q].size();
        for (const auto& t : terms[q]) bytes += t.first.size();
    }
    if (term_bytes_out && term_offsets_out) {
        char* tb = (char*)std::malloc(bytes + 1);
        uint64_t* to = (uint64_t*)std::malloc((total + 1) * sizeof(uint64_t));
        if (!tb || !to) { std::free(tb); std::free(to); nsh_set_err(e, "nsh_engine_similar_batch: out of memory"); return -1; }
        size_t j = 0, at = 0;
        for (const auto& row : terms)
            for (const auto& t : row) { to[j++] = at; std::memcpy(tb + at, t.first.data(), t.first.size()); at += t.first.size(); }
        to[j] = at;
        tb[at] = 0;
        *term_bytes_out = tb;
        *term_offsets_out = to;
    }
    return 0;
} NSH_CATCH(e, "nsh_engine_similar_batch", -1)
}

extern "C" int nsh_engine_more_like_this_json(nsh_engine* e, const char* uid, uint64_t uid_len, int k, char** json_out) { try {
    if (!e || !json_out || (uid_len && !uid)) return -1;
    std::string s;
    const bool ok = e->eng.more_like_this_text(std::string(uid ? uid : "", (size_t)uid_len), k, s);
    if (!ok) { nsh_set_err(e, e->eng.last_error()); *json_out = nullptr; return -1; }
    *json_out = (char*)std::malloc(s.size() + 1);
    if (!*json_out) return -1;
    std::memcpy(*json_out, s.c_str(), s.size() + 1);
    return 0;
} NSH_CATCH(e, "nsh_engine_more_like_this_json", -1)
}

extern "C" void nsh_engine_release_similar(nsh_engine* e) { try { if (e) e->eng.release_similar(); } NSH_CATCH_VOID(e, "nsh_engine_release_similar") }
extern "C" uint64_t nsh_engine_similar_segments_on_device(nsh_engine* e) { return e ? (uint64_t)e->eng.similar_segments_on_device() : 0; }

// ---- filtered search (host/filter.hpp) ----
extern "C" uint32_t nsh_date_key(const char* s, uint64_t len) { return nsx::date_key(std::string_view(s ? s : "", s ? (size_t)len : 0)); }

static nsx::DocFilter nsh_doc_filter(const char* from, const char* to, int keep_undated) {
    nsx::DocFilter f;
    f.date_from = from ? from : "";
    f.date_to = to ? to : "";
    f.keep_undated = keep_undated != 0;
    return f;
}

// ---- related terms ----
extern "C" int nsh_related_aggregate_host(const uint32_t* counts, uint32_t n_docs, const uint32_t* pairs, uint64_t n_pairs, const uint32_t* df,
                                          const float* idf, uint32_t n_terms, const uint32_t* doc_ids, const uint64_t* row_off, uint32_t n_rows,
                                          uint32_t max_terms, uint32_t min_tf, uint32_t min_docs, uint32_t min_df, uint32_t max_df,
                                          uint32_t* term_out, uint32_t* docs_out, float* w_out, uint32_t* count_out, uint32_t* ndocs_out) { try {
    if ((n_docs && !counts) || (n_pairs && !pairs) || (n_terms && (!df || !idf))) return -1;
    if (n_rows && (!row_off || !term_out || !docs_out || !w_out || !count_out || !ndocs_out || (row_off[n_rows] && !doc_ids))) return -1;
    std::vector<uint64_t> off((size_t)n_docs + 1, 0);
    for (uint32_t d = 0; d < n_docs; d++) off[d + 1] = off[d] + counts[d];
    if (off[n_docs] != n_pairs) return -1;
    return nsx::related_aggregate_host(off.data(), n_docs, pairs, df, idf, n_terms, doc_ids, row_off, n_rows, max_terms, min_tf, min_docs, min_df, max_df,
                                       term_out, docs_out, w_out, count_out, ndocs_out);
} catch (...) { return -1; }
}

static nsx::RelatedOptions nsh_related_options(uint32_t max_terms, uint32_t min_tf, uint32_t min_docs, uint32_t min_df, uint32_t max_df, uint32_t sample) {
    nsx::RelatedOptions o;
    o.max_terms = max_terms; o.min_tf = min_tf; o.min_docs = min_docs; o.min_df = min_df; o.max_df = max_df; o.sample = sample;
    return o;
}

extern "C" int nsh_engine_terms_batch(nsh_engine* e, const uint32_t* seg_doc, const uint64_t* row_off, uint64_t n_rows, uint32_t max_terms,
                                      uint32_t min_tf, uint32_t min_docs, uint32_t min_df, uint32_t max_df, uint32_t* docs_out, uint64_t* df_out,
                                      float* w_out, uint32_t* count_out, uint32_t* ndocs_out, char** term_bytes_out, uint64_t** term_offsets_out,
                                      float* device_ms_out) { try {
    if (!e) return -1;
    if (term_bytes_out) *term_bytes_out = nullptr;
    if (term_offsets_out) *term_offsets_out = nullptr;
    if (n_rows && (!row_off || (row_off[n_rows] && !seg_doc))) { nsh_set_err(e, "nsh_engine_terms_batch: null argument"); return -1; }
    for (uint64_t q = 0; q < n_rows; q++)
        if (row_off[q + 1] < row_off[q]) { nsh_set_err(e, "nsh_engine_terms_batch: row_off descends"); return -1; }
    std::vector<std::pair<uint32_t, uint32_t>> ids(n_rows ? (size_t)row_off[n_rows] : 0);
    for (size_t i = 0; i < ids.size(); i++) ids[i] = {seg_doc[2 * i], seg_doc[2 * i + 1]};
    const bool want_terms = term_bytes_out && term_offsets_out;
    std::vector<std::vector<std::string>> terms;
    if (!e->eng.terms_batch(ids.data(), row_off, (size_t)n_rows, nsh_related_options(max_terms, min_tf, min_docs, min_df, max_df, 100), docs_out, df_out,
                            w_out, count_out, ndocs_out, want_terms ? &terms : nullptr, device_ms_out)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    if (!want_terms) return 0;
    size_t total = 0, bytes = 0;
    for (const auto& row : terms) { total += row.size(); for (const auto& t : row) bytes += t.size(); }
    char* tb = (char*)std::malloc(bytes + 1);
    uint64_t* to = (uint64_t*)std::malloc((total + 1) * sizeof(uint64_t));
    if (!tb || !to) { std::free(tb); std::free(to); nsh_set_err(e, "nsh_engine_terms_batch: out of memory"); return -1; }
    size_t j = 0, at = 0;
    for (const auto& row : terms)
        for (const auto& t : row) { to[j++] = at; std::memcpy(tb + at, t.data(), t.size()); at += t.size(); }
    to[j] = at;
    tb[at] = 0;
    *term_bytes_out = tb;
    *term_offsets_out = to;
    return 0;
} NSH_CATCH(e, "nsh_engine_terms_batch", -1)
}

extern "C" int nsh_engine_related_terms_json(nsh_engine* e, const char* query, uint32_t max_terms, uint32_t min_tf, uint32_t min_docs, uint32_t min_df,
                                             uint32_t max_df, uint32_t sample, int filtered, const char* date_from, const char* date_to,
                                             int keep_undated, char** json_out) { try {
    if (!e || !json_out) return -1;
    std::string s;
    const nsx::DocFilter f = filtered ? nsh_doc_filter(date_from, date_to, keep_undated) : nsx::DocFilter{};
    const bool ok = e->eng.related_terms_text(query ? query : "", nsh_related_options(max_terms, min_tf, min_docs, min_df, max_df, sample), filtered ? &f : nullptr, s);
    if (!ok) { nsh_set_err(e, e->eng.last_error()); *json_out = nullptr; return -1; }
    *json_out = (char*)std::malloc(s.size() + 1);
    if (!*json_out) return -1;
    std::memcpy(*json_out, s.c_str(), s.size() + 1);
    return 0;
} NSH_CATCH(e, "nsh_engine_related_terms_json", -1)
}

static void nsh_filter_stats_out(const nsx::FilterStats& st, uint64_t* stats_u64, double* stats_ms) {
    if (stats_u64) {
        stats_u64[0] = st.docs_kept; stats_u64[1] = st.docs_total; stats_u64[2] = st.postings_kept; stats_u64[3] = st.postings_total;
        stats_u64[4] = st.segments_on_device; stats_u64[5] = st.hbm_bytes;
    }
    if (stats_ms) { stats_ms[0] = st.device_ms; stats_ms[1] = st.total_ms; }
}

// words_out (capacity cap words, may be NULL): the segments' bitmaps back to back, ceil(N / 32) words each.  Returns the
// number of words in all, or -1 (a malformed bound).
extern "C" int64_t nsh_engine_filter_bits(nsh_engine* e, const char* date_from, const char* date_to, int keep_undated, uint32_t* words_out,
                                          uint64_t cap) { try {
    if (!e) return -1;
    std::vector<std::vector<uint32_t>> bits;
    if (!e->eng.filter_bits(nsh_doc_filter(date_from, date_to, keep_undated), bits)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    uint64_t at = 0;
    for (const auto& b : bits) {
        for (size_t i = 0; i < b.size(); i++)
            if (words_out && at + i < cap) words_out[at + i] = b[i];
        at += b.size();
    }
    return (int64_t)at;
} NSH_CATCH(e, "nsh_engine_filter_bits", -1)
}

// stats_u64 (6, may be NULL): documents kept / total, postings kept / total, segments with a device copy, bytes of HBM;
// stats_ms (2, may be NULL): device passes, whole call
extern "C" int nsh_engine_open_filter(nsh_engine* e, const char* date_from, const char* date_to, int keep_undated, uint32_t* handle_out,
                                      uint64_t* stats_u64, double* stats_ms) { try {
    if (!e || !handle_out) return -1;
    nsx::FilterStats st;
    if (!e->eng.open_filter(nsh_doc_filter(date_from, date_to, keep_undated), *handle_out, &st)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    nsh_filter_stats_out(st, stats_u64, stats_ms);
    return 0;
} NSH_CATCH(e, "nsh_engine_open_filter", -1)
}

// words: the segments' bitmaps back to back (n_words in all; the engine checks them against its segments)
extern "C" int nsh_engine_open_filter_bits(nsh_engine* e, const uint32_t* words, uint64_t n_words, uint32_t* handle_out, uint64_t* stats_u64,
                                           double* stats_ms) { try {
    if (!e || !handle_out || (n_words && !words)) return -1;
    // whole bitmaps as far as the words reach; words left over become one more: the engine refuses either with a message
    std::vector<std::vector<uint32_t>> bits;
    uint64_t at = 0;
    for (size_t s = 0; s < e->eng.segments.size(); s++) {
        const uint64_t w = ((uint64_t)e->eng.segments[s].N + 31) / 32;
        if (at + w > n_words) break;
        bits.emplace_back(words + at, words + at + w);
        at += w;
    }
    if (bits.size() == e->eng.segments.size() && at != n_words) bits.emplace_back(words + at, words + n_words);
    nsx::FilterStats st;
    if (!e->eng.open_filter(bits, *handle_out, &st)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    nsh_filter_stats_out(st, stats_u64, stats_ms);
    return 0;
} NSH_CATCH(e, "nsh_engine_open_filter_bits", -1)
}

extern "C" int nsh_engine_close_filter(nsh_engine* e, uint32_t handle) { try {
    if (!e) return -1;
    if (!e->eng.close_filter(handle)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    return 0;
} NSH_CATCH(e, "nsh_engine_close_filter", -1)
}
extern "C" uint32_t nsh_engine_open_filters(nsh_engine* e) { try { return e ? (uint32_t)e->eng.open_filters() : 0; } NSH_CATCH(e, "nsh_engine_open_filters", 0)
}

// nsh_engine_search_batch under an open filter: the same arrays, hits in manifest positions
extern "C" int nsh_engine_search_filtered_batch(nsh_engine* e, uint32_t handle, const char* const* queries, uint32_t n_queries, int k,
                                                uint32_t flags, ns_hit* hits, uint32_t* nhits, uint64_t* found, uint8_t* has_found) { try {
    if (!e) return -1;
    const uint32_t K = (uint32_t)std::max(1, std::min(k, 100));
    std::vector<nextsearch::Engine::QueryView> views(n_queries);
    for (uint32_t q = 0; q < n_queries; q++) views[q] = {queries[q] ? queries[q] : "", queries[q] ? std::strlen(queries[q]) : 0};
    std::vector<ns_hit> h_;
    std::vector<uint32_t> n_;
    std::vector<uint64_t> f_;
    std::vector<uint8_t> u_;
    if (!hits) { h_.resize((size_t)n_queries * K); hits = h_.data(); }
    if (!nhits) { n_.resize(n_queries); nhits = n_.data(); }
    if (!found) { f_.resize(n_queries); found = f_.data(); }
    if (!has_found) { u_.resize(n_queries); has_found = u_.data(); }
    if (!e->eng.search_filtered_batch_flat(handle, views.data(), n_queries, k, flags, hits, nhits, found, has_found)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    for (uint32_t q = 0; q < n_queries; q++) {
        if (has_found[q]) continue;
        nhits[q] = 0; found[q] = 0;
        for (uint32_t i = 0; i < K; i++) hits[(size_t)q * K + i] = ns_hit{-__builtin_inff(), 0xFFFFFFFFu, 0xFFFFFFFFu};
    }
    return 0;
} NSH_CATCH(e, "nsh_engine_search_filtered_batch", -1)
}

// a JSON body, or on failure the engine's message as {"error": ...}, as a malloc'ed string
static int nsh_json_out(nsh_engine* e, bool ok, std::string& s, char** json_out) {
    if (!ok) {
        nsh_set_err(e, s);
        std::string o = "{\n  \"error\": ";
        nextsearch::json_escape(o, s);
        s = o + "\n}";
    }
    *json_out = (char*)std::malloc(s.size() + 1);
    if (!*json_out) return -1;
    std::memcpy(*json_out, s.c_str(), s.size() + 1);
    return ok ? 0 : -1;
}

// A JSON entry point over a filter that may be absent: call(filter or nullptr, body) is the Engine's _text call, with whatever
// else the entry point has to check in front of it (false: body = the message).
template <class Call>
static int nsh_text_json(nsh_engine* e, int use_filter, const char* date_from, const char* date_to, int keep_undated, char** json_out, Call call) {
    if (!e || !json_out) return -1;
    *json_out = nullptr;
    std::string s;
    const nsx::DocFilter f = nsh_doc_filter(date_from, date_to, keep_undated);
    const bool ok = call(use_filter ? &f : nullptr, s);
    return nsh_json_out(e, ok, s, json_out);
}

// the terms' texts joined with spaces into buf (cut at cap - 1 bytes): what the nsh_parse_* calls hand back
template <class T>
static void nsh_join_terms(const std::vector<T>& terms, char* buf, uint32_t cap) {
    if (!buf || !cap) return;
    std::string joined;
    for (size_t i = 0; i < terms.size(); i++) {
        if (i) joined.push_back(' ');
        joined += terms[i].text;
    }
    const size_t n = std::min<size_t>(joined.size(), cap - 1);
    std::memcpy(buf, joined.data(), n);
    buf[n] = 0;
}

// Engine::search_filtered: *json_out (free with nsh_free) is the body, or {"error": ...} with -1 returned
extern "C" int nsh_engine_search_filtered_json(nsh_engine* e, const char* query, int k, const char* date_from, const char* date_to,
                                               int keep_undated, char** json_out) { try {
    if (!e || !json_out) return -1;
    *json_out = nullptr;
    std::string s;
    const bool ok = e->eng.search_filtered_text(query ? query : "", k, nsh_doc_filter(date_from, date_to, keep_undated), s);
    return nsh_json_out(e, ok, s, json_out);
} NSH_CATCH(e, "nsh_engine_search_filtered_json", -1)
}

// ---- facet counts (host/facet.hpp) ----
// the C spec as the engine's; false (message in `why`): no spec, an unknown kind or a null array
static bool nsh_facet_spec_of(nsh_engine* e, const nsh_facet_spec* in, nsx::FacetSpec& out, std::string& why) {
    if (!in) { why = "facet: spec is NULL"; return false; }
    if (in->kind > 2u) { why = "facet: unknown kind " + std::to_string(in->kind); return false; }
    out.kind = (nsx::FacetSpec::Kind)in->kind;
    if (out.kind != nsx::FacetSpec::Custom) return true;
    if ((in->n_custom && !in->custom_buckets) || (in->n_custom_labels && !in->custom_labels)) { why = "facet custom: null array"; return false; }
    // whole arrays as far as the ids reach; ids left over become one more: the engine refuses either with a message
    uint64_t at = 0;
    for (const auto& sd : e->eng.segments) {
        if (at + sd.N > in->n_custom) break;
        out.custom_buckets.emplace_back(in->custom_buckets + at, in->custom_buckets + at + sd.N);
        at += sd.N;
    }
    if (out.custom_buckets.size() == e->eng.segments.size() && at != in->n_custom) out.custom_buckets.emplace_back(in->custom_buckets + at, in->custom_buckets + in->n_custom);
    for (uint32_t i = 0; i < in->n_custom_labels; i++) out.custom_labels.emplace_back(in->custom_labels[i] ? in->custom_labels[i] : "");
    return true;
}

extern "C" int64_t nsh_engine_facet_buckets(nsh_engine* e, const nsh_facet_spec* spec, uint16_t* buckets_out, uint64_t cap, uint32_t* n_buckets_out,
                                            char** labels_out, uint64_t* labels_bytes_out) { try {
    if (!e) return -1;
    if (labels_out) *labels_out = nullptr;
    nsx::FacetSpec sp;
    std::string why;
    if (!nsh_facet_spec_of(e, spec, sp, why)) { nsh_set_err(e, why); return -1; }
    std::vector<std::vector<uint16_t>> tables;
    std::vector<std::string> labels;
    if (!e->eng.facet_buckets(sp, tables, labels)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    uint64_t at = 0;
    for (const auto& t : tables) {
        for (size_t i = 0; i < t.size(); i++)
            if (buckets_out && at + i < cap) buckets_out[at + i] = t[i];
        at += t.size();
    }
    if (n_buckets_out) *n_buckets_out = (uint32_t)labels.size();
    std::string flat;
    for (const auto& l : labels) { flat += l; flat.push_back('\0'); }
    if (labels_bytes_out) *labels_bytes_out = flat.size();
    if (labels_out) {
        *labels_out = (char*)std::malloc(flat.size() + 1);
        if (!*labels_out) return -1;
        std::memcpy(*labels_out, flat.data(), flat.size());
        (*labels_out)[flat.size()] = '\0';
    }
    return (int64_t)at;
} NSH_CATCH(e, "nsh_engine_facet_buckets", -1)
}

extern "C" int nsh_engine_facet_batch(nsh_engine* e, const nsh_facet_spec* spec, uint32_t filter_handle, const char* const* queries, uint32_t n_queries,
                                      uint32_t flags, uint32_t* counts_out, uint64_t counts_cap, uint64_t* found, uint8_t* has_found,
                                      float* device_ms_out, double* count_ms_out) { try {
    if (!e) return -1;
    nsx::FacetSpec sp;
    std::string why;
    if (!nsh_facet_spec_of(e, spec, sp, why)) { nsh_set_err(e, why); return -1; }
    if (n_queries && !queries) { nsh_set_err(e, "nsh_engine_facet_batch: queries is NULL"); return -1; }
    std::vector<nextsearch::Engine::QueryView> views(n_queries);
    for (uint32_t q = 0; q < n_queries; q++) views[q] = {queries[q] ? queries[q] : "", queries[q] ? std::strlen(queries[q]) : 0};
    std::vector<uint64_t> f_;
    std::vector<uint8_t> u_;
    if (!found) { f_.resize(n_queries); found = f_.data(); }
    if (!has_found) { u_.resize(n_queries); has_found = u_.data(); }
    std::vector<uint32_t> counts;
    std::vector<std::string> labels;
    if (!e->eng.facet_batch_flat(sp, filter_handle, views.data(), n_queries, flags, counts, found, has_found, labels, device_ms_out, count_ms_out)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    if (counts.size() > counts_cap || (!counts.empty() && !counts_out)) {
        nsh_set_err(e, "nsh_engine_facet_batch: counts_out holds " + std::to_string(counts_cap) + " entries, " + std::to_string(n_queries) + " queries x " +
                           std::to_string(labels.size()) + " buckets need " + std::to_string(counts.size()));
        return -1;
    }
    if (!counts.empty()) std::memcpy(counts_out, counts.data(), counts.size() * 4);
    for (uint32_t q = 0; q < n_queries; q++)
        if (!has_found[q]) found[q] = 0;
    return 0;
} NSH_CATCH(e, "nsh_engine_facet_batch", -1)
}

extern "C" int nsh_engine_search_faceted_json(nsh_engine* e, const char* query, int k, const nsh_facet_spec* spec, int use_filter, const char* date_from,
                                              const char* date_to, int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        nsx::FacetSpec sp;
        return nsh_facet_spec_of(e, spec, sp, s) && e->eng.search_faceted_text(query ? query : "", k, sp, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_faceted_json", -1)
}

extern "C" void nsh_engine_release_facets(nsh_engine* e) { try { if (e) e->eng.release_facets(); } NSH_CATCH_VOID(e, "nsh_engine_release_facets") }
extern "C" uint64_t nsh_engine_facet_tables_on_device(nsh_engine* e) { return e ? (uint64_t)e->eng.facet_tables_on_device() : 0; }

// ---- search sorted by date (host/sorted.hpp) ----
static bool nsh_sort_spec_of(nsh_engine* e, const nsh_sort_spec* in, nsx::SortSpec& out, std::string& why) {
    if (!in) { why = "sort: spec is NULL"; return false; }
    if (in->kind > 1u) { why = "sort: unknown kind " + std::to_string(in->kind); return false; }
    out.kind = (nsx::SortSpec::Kind)in->kind;
    out.ascending = in->ascending != 0;
    if (out.kind != nsx::SortSpec::Custom) return true;
    if (in->n_custom && !in->custom_keys) { why = "sort custom: null array"; return false; }
    // whole arrays as far as the keys reach; keys left over become one more: the engine refuses either with a message
    uint64_t at = 0;
    for (const auto& sd : e->eng.segments) {
        if (at + sd.N > in->n_custom) break;
        out.custom_keys.emplace_back(in->custom_keys + at, in->custom_keys + at + sd.N);
        at += sd.N;
    }
    if (out.custom_keys.size() == e->eng.segments.size() && at != in->n_custom) out.custom_keys.emplace_back(in->custom_keys + at, in->custom_keys + in->n_custom);
    return true;
}

extern "C" int64_t nsh_engine_sort_keys(nsh_engine* e, const nsh_sort_spec* spec, uint32_t* keys_out, uint64_t cap) { try {
    if (!e) return -1;
    nsx::SortSpec sp;
    std::string why;
    if (!nsh_sort_spec_of(e, spec, sp, why)) { nsh_set_err(e, why); return -1; }
    std::vector<std::vector<uint32_t>> keys;
    if (!e->eng.sort_keys(sp, keys)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    uint64_t at = 0;
    for (const auto& t : keys) {
        for (size_t i = 0; i < t.size(); i++)
            if (keys_out && at + i < cap) keys_out[at + i] = t[i];
        at += t.size();
    }
    return (int64_t)at;
} NSH_CATCH(e, "nsh_engine_sort_keys", -1)
}

extern "C" int nsh_engine_search_sorted_batch(nsh_engine* e, const nsh_sort_spec* spec, uint32_t filter_handle, const char* const* queries, uint32_t n_queries,
                                              int k, uint32_t flags, void* hits, uint32_t* keys_out, uint32_t* nhits, uint64_t* found, uint8_t* has_found,
                                              float* device_ms_out) { try {
    if (!e) return -1;
    nsx::SortSpec sp;
    std::string why;
    if (!nsh_sort_spec_of(e, spec, sp, why)) { nsh_set_err(e, why); return -1; }
    if (n_queries && (!queries || !hits || !keys_out || !nhits)) { nsh_set_err(e, "nsh_engine_search_sorted_batch: null argument"); return -1; }
    std::vector<nextsearch::Engine::QueryView> views(n_queries);
    for (uint32_t q = 0; q < n_queries; q++) views[q] = {queries[q] ? queries[q] : "", queries[q] ? std::strlen(queries[q]) : 0};
    std::vector<uint64_t> f_;
    std::vector<uint8_t> u_;
    if (!found) { f_.resize(n_queries); found = f_.data(); }
    if (!has_found) { u_.resize(n_queries); has_found = u_.data(); }
    if (!e->eng.search_sorted_batch_flat(sp, filter_handle, views.data(), n_queries, k, flags, (ns_hit*)hits, keys_out, nhits, found, has_found, device_ms_out)) {
        nsh_set_err(e, e->eng.last_error());
        return -1;
    }
    for (uint32_t q = 0; q < n_queries; q++)
        if (!has_found[q]) found[q] = 0;
    return 0;
} NSH_CATCH(e, "nsh_engine_search_sorted_batch", -1)
}

extern "C" int nsh_engine_search_sorted_json(nsh_engine* e, const char* query, int k, const nsh_sort_spec* spec, int use_filter, const char* date_from,
                                             const char* date_to, int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        nsx::SortSpec sp;
        return nsh_sort_spec_of(e, spec, sp, s) && e->eng.search_sorted_text(query ? query : "", k, sp, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_sorted_json", -1)
}

extern "C" void nsh_engine_release_sorted(nsh_engine* e) { try { if (e) e->eng.release_sorted(); } NSH_CATCH_VOID(e, "nsh_engine_release_sorted") }
extern "C" uint64_t nsh_engine_sort_tables_on_device(nsh_engine* e) { return e ? (uint64_t)e->eng.sort_tables_on_device() : 0; }

// ---- boolean queries (host/boolean.hpp) ----
extern "C" uint32_t nsh_parse_boolean(const char* query, char* buf, uint32_t cap, uint8_t* roles, uint32_t roles_cap) { try {
    const auto terms = nsx::parse_boolean(query ? query : "");
    for (size_t i = 0; i < terms.size() && i < roles_cap; i++)
        if (roles) roles[i] = terms[i].role;
    nsh_join_terms(terms, buf, cap);
    return (uint32_t)terms.size();
} NSH_CATCH(nullptr, "nsh_parse_boolean", 0)
}

extern "C" int nsh_engine_search_boolean_batch(nsh_engine* e, uint32_t filter_handle, const char* const* queries, uint32_t n_queries, int k, void* hits,
                                               uint32_t* nhits, uint64_t* found, uint8_t* has_found, float* device_ms_out) { try {
    if (!e) return -1;
    if (n_queries && (!queries || !hits || !nhits)) { nsh_set_err(e, "nsh_engine_search_boolean_batch: null argument"); return -1; }
    std::vector<nextsearch::Engine::QueryView> views(n_queries);
    for (uint32_t q = 0; q < n_queries; q++) views[q] = {queries[q] ? queries[q] : "", queries[q] ? std::strlen(queries[q]) : 0};
    std::vector<uint64_t> f_;
    std::vector<uint8_t> u_;
    if (!found) { f_.resize(n_queries); found = f_.data(); }
    if (!has_found) { u_.resize(n_queries); has_found = u_.data(); }
    if (!e->eng.search_boolean_batch_flat(filter_handle, views.data(), n_queries, k, (ns_hit*)hits, nhits, found, has_found, device_ms_out)) {
        nsh_set_err(e, e->eng.last_error());
        return -1;
    }
    for (uint32_t q = 0; q < n_queries; q++)
        if (!has_found[q]) found[q] = 0;
    return 0;
} NSH_CATCH(e, "nsh_engine_search_boolean_batch", -1)
}

extern "C" int nsh_engine_search_boolean_json(nsh_engine* e, const char* query, int k, int use_filter, const char* date_from, const char* date_to,
                                              int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        return e->eng.search_dialect_text(nsx::Dialect::Boolean, query ? query : "", k, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_boolean_json", -1)
}

// ---- pages past the first K (host/page.hpp) ----
extern "C" int nsh_parse_cursor(const char* text, int kind, nsh_page_cursor* out, char* err, uint32_t err_cap) { try {
    if (err && err_cap) err[0] = 0;
    if (!out) return -1;
    nsx::PageCursor c;
    std::string why;
    const bool ok = nsx::parse_cursor(text ? text : "", (char)kind, c, why);
    *out = nsh_page_cursor{c.set ? 1u : 0u, c.rank, c.seg, c.doc};
    if (!ok && err && err_cap) {
        const size_t n = std::min<size_t>(why.size(), err_cap - 1);
        std::memcpy(err, why.data(), n);
        err[n] = 0;
    }
    return ok ? 0 : -1;
} NSH_CATCH(nullptr, "nsh_parse_cursor", -1)
}

extern "C" uint32_t nsh_cursor_text(int kind, const nsh_page_cursor* c, char* buf, uint32_t cap) { try {
    if (buf && cap) buf[0] = 0;
    if (!c) return 0;
    nsx::PageCursor pc;
    pc.set = c->set != 0; pc.rank = c->rank; pc.seg = c->seg; pc.doc = c->doc;
    const std::string t = nsx::cursor_text((char)kind, pc);
    if (buf && cap) {
        const size_t n = std::min<size_t>(t.size(), cap - 1);
        std::memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return (uint32_t)t.size();
} NSH_CATCH(nullptr, "nsh_cursor_text", 0)
}

static void nsh_cursors_of(const nsh_page_cursor* in, uint32_t n, std::vector<nsx::PageCursor>& out) {
    out.clear();
    if (!in) return;
    out.resize(n);
    for (uint32_t q = 0; q < n; q++) { out[q].set = in[q].set != 0; out[q].rank = in[q].rank; out[q].seg = in[q].seg; out[q].doc = in[q].doc; }
}

// mode: the nsx::PageSpec mode whose batch call this is (page_call: which call, and whether it is in date order)
static int nsh_after_batch(nsh_engine* e, const char* fn, nsx::PageSpec::Mode mode, const nsh_sort_spec* spec, uint32_t filter_handle, const char* const* queries,
                           uint32_t n_queries, int k, uint32_t flags, const nsh_page_cursor* after, void* hits, uint32_t* keys_out, uint32_t* nhits,
                           uint64_t* found, uint64_t* rest, uint8_t* has_found, float* device_ms_out, const nsx::BoostSpec* boost = nullptr) {
    if (!e) return -1;
    nsx::SortSpec sp;
    std::string why;
    const nsx::PageCall call = nsx::page_call(mode);
    const bool dated = call.dated;
    if (dated && !nsh_sort_spec_of(e, spec, sp, why)) { nsh_set_err(e, why); return -1; }
    if (n_queries && (!queries || !hits || !nhits || (dated && !keys_out))) { nsh_set_err(e, std::string(fn) + ": null argument"); return -1; }
    std::vector<nextsearch::Engine::QueryView> views(n_queries);
    for (uint32_t q = 0; q < n_queries; q++) views[q] = {queries[q] ? queries[q] : "", queries[q] ? std::strlen(queries[q]) : 0};
    std::vector<nsx::PageCursor> cur;
    nsh_cursors_of(after, n_queries, cur);
    const nsx::PageCursor* cp = after ? cur.data() : nullptr;
    std::vector<uint64_t> f_, r_;
    std::vector<uint8_t> u_;
    if (!found) { f_.resize(n_queries); found = f_.data(); }
    if (!rest) { r_.resize(n_queries); rest = r_.data(); }
    if (!has_found) { u_.resize(n_queries); has_found = u_.data(); }
    bool ok;
    if (!call.plain)
        ok = dated ? e->eng.search_dialect_sorted_batch_flat(call.dialect, sp, filter_handle, views.data(), n_queries, k, cp, (ns_hit*)hits, keys_out, nhits, found, rest, has_found, device_ms_out)
                   : e->eng.search_dialect_after_batch_flat(call.dialect, filter_handle, views.data(), n_queries, k, cp, (ns_hit*)hits, nhits, found, rest, has_found, device_ms_out, boost);
    else if (dated) ok = e->eng.search_sorted_after_batch_flat(sp, filter_handle, views.data(), n_queries, k, flags, cp, (ns_hit*)hits, keys_out, nhits, found, rest, has_found, device_ms_out);
    else ok = e->eng.search_after_batch_flat(filter_handle, views.data(), n_queries, k, flags, cp, (ns_hit*)hits, nhits, found, rest, has_found, device_ms_out);
    if (!ok) { nsh_set_err(e, e->eng.last_error()); return -1; }
    for (uint32_t q = 0; q < n_queries; q++)
        if (!has_found[q]) found[q] = rest[q] = 0;
    return 0;
}

extern "C" int nsh_engine_search_after_batch(nsh_engine* e, uint32_t filter_handle, const char* const* queries, uint32_t n_queries, int k, uint32_t flags,
                                             const nsh_page_cursor* after, void* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* has_found,
                                             float* device_ms_out) { try {
    return nsh_after_batch(e, "nsh_engine_search_after_batch", (flags & NS_FLAG_AND) ? nsx::PageSpec::SearchAnd : nsx::PageSpec::SearchOr, nullptr, filter_handle, queries, n_queries, k, flags, after, hits, nullptr,
                           nhits, found, rest, has_found, device_ms_out);
} NSH_CATCH(e, "nsh_engine_search_after_batch", -1)
}

extern "C" int nsh_engine_search_boolean_after_batch(nsh_engine* e, uint32_t filter_handle, const char* const* queries, uint32_t n_queries, int k,
                                                     const nsh_page_cursor* after, void* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                                     uint8_t* has_found, float* device_ms_out) { try {
    return nsh_after_batch(e, "nsh_engine_search_boolean_after_batch", nsx::PageSpec::Boolean, nullptr, filter_handle, queries, n_queries, k, 0u, after, hits, nullptr, nhits, found, rest,
                           has_found, device_ms_out);
} NSH_CATCH(e, "nsh_engine_search_boolean_after_batch", -1)
}

extern "C" int nsh_engine_search_sorted_after_batch(nsh_engine* e, const nsh_sort_spec* spec, uint32_t filter_handle, const char* const* queries,
                                                    uint32_t n_queries, int k, uint32_t flags, const nsh_page_cursor* after, void* hits, uint32_t* keys_out,
                                                    uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* has_found, float* device_ms_out) { try {
    return nsh_after_batch(e, "nsh_engine_search_sorted_after_batch", nsx::PageSpec::Sorted, spec, filter_handle, queries, n_queries, k, flags, after, hits, keys_out, nhits, found, rest,
                           has_found, device_ms_out);
} NSH_CATCH(e, "nsh_engine_search_sorted_after_batch", -1)
}

// ---- facet counts and date order for boolean queries ----
static int nsh_facet_boolean(nsh_engine* e, const std::string& fn, nsx::Dialect dialect, const nsh_facet_spec* spec, uint32_t filter_handle, const char* const* queries,
                             uint32_t n_queries, uint32_t* counts_out, uint64_t counts_cap, uint64_t* found, uint8_t* has_found, float* device_ms_out);

extern "C" int nsh_engine_facet_boolean_batch(nsh_engine* e, const nsh_facet_spec* spec, uint32_t filter_handle, const char* const* queries, uint32_t n_queries,
                                              uint32_t* counts_out, uint64_t counts_cap, uint64_t* found, uint8_t* has_found, float* device_ms_out) { try {
    return nsh_facet_boolean(e, "nsh_engine_facet_boolean_batch", nsx::Dialect::Boolean, spec, filter_handle, queries, n_queries, counts_out, counts_cap, found, has_found, device_ms_out);
} NSH_CATCH(e, "nsh_engine_facet_boolean_batch", -1)
}

// ---- any-of groups in boolean queries (host/grouped.hpp) ----
extern "C" uint32_t nsh_parse_grouped(const char* query, char* buf, uint32_t cap, uint8_t* roles, uint32_t* clauses, uint32_t terms_cap) { try {
    const auto terms = nsx::parse_grouped(query ? query : "");
    for (size_t i = 0; i < terms.size() && i < terms_cap; i++) {
        if (roles) roles[i] = terms[i].role;
        if (clauses) clauses[i] = terms[i].clause;
    }
    nsh_join_terms(terms, buf, cap);
    return (uint32_t)terms.size();
} NSH_CATCH(nullptr, "nsh_parse_grouped", 0)
}

extern "C" int nsh_engine_search_grouped_after_batch(nsh_engine* e, uint32_t filter_handle, const char* const* queries, uint32_t n_queries, int k,
                                                     const nsh_page_cursor* after, void* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                                     uint8_t* has_found, float* device_ms_out) { try {
    return nsh_after_batch(e, "nsh_engine_search_grouped_after_batch", nsx::PageSpec::Grouped, nullptr, filter_handle, queries, n_queries, k, 0u, after, hits, nullptr, nhits, found, rest,
                           has_found, device_ms_out);
} NSH_CATCH(e, "nsh_engine_search_grouped_after_batch", -1)
}

extern "C" int nsh_engine_facet_grouped_batch(nsh_engine* e, const nsh_facet_spec* spec, uint32_t filter_handle, const char* const* queries, uint32_t n_queries,
                                              uint32_t* counts_out, uint64_t counts_cap, uint64_t* found, uint8_t* has_found, float* device_ms_out) { try {
    return nsh_facet_boolean(e, "nsh_engine_facet_grouped_batch", nsx::Dialect::Grouped, spec, filter_handle, queries, n_queries, counts_out, counts_cap, found, has_found, device_ms_out);
} NSH_CATCH(e, "nsh_engine_facet_grouped_batch", -1)
}

extern "C" int nsh_engine_search_grouped_sorted_batch(nsh_engine* e, const nsh_sort_spec* spec, uint32_t filter_handle, const char* const* queries,
                                                      uint32_t n_queries, int k, const nsh_page_cursor* after, void* hits, uint32_t* keys_out, uint32_t* nhits,
                                                      uint64_t* found, uint64_t* rest, uint8_t* has_found, float* device_ms_out) { try {
    return nsh_after_batch(e, "nsh_engine_search_grouped_sorted_batch", nsx::PageSpec::GroupedSorted, spec, filter_handle, queries, n_queries, k, 0u, after, hits, keys_out, nhits, found, rest,
                           has_found, device_ms_out);
} NSH_CATCH(e, "nsh_engine_search_grouped_sorted_batch", -1)
}

extern "C" int nsh_engine_search_grouped_json(nsh_engine* e, const char* query, int k, int use_filter, const char* date_from, const char* date_to,
                                              int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        return e->eng.search_dialect_text(nsx::Dialect::Grouped, query ? query : "", k, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_grouped_json", -1)
}

extern "C" int nsh_engine_search_grouped_faceted_json(nsh_engine* e, const char* query, int k, const nsh_facet_spec* spec, int use_filter, const char* date_from,
                                                      const char* date_to, int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        nsx::FacetSpec sp;
        return nsh_facet_spec_of(e, spec, sp, s) && e->eng.search_dialect_faceted_text(nsx::Dialect::Grouped, query ? query : "", k, sp, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_grouped_faceted_json", -1)
}

extern "C" int nsh_engine_search_grouped_sorted_json(nsh_engine* e, const char* query, int k, const nsh_sort_spec* spec, int use_filter, const char* date_from,
                                                     const char* date_to, int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        nsx::SortSpec sp;
        return nsh_sort_spec_of(e, spec, sp, s) && e->eng.search_dialect_sorted_text(nsx::Dialect::Grouped, query ? query : "", k, sp, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_grouped_sorted_json", -1)
}

// ---- at-least-m-of-n clauses (host/quorum.hpp) ----
extern "C" uint32_t nsh_parse_quorum(const char* query, char* buf, uint32_t cap, uint8_t* roles, uint32_t* clauses, uint32_t* needs, uint8_t* promoted,
                                     uint32_t terms_cap, uint32_t* min_should_out) { try {
    uint32_t min_should = 0;
    const auto terms = nsx::parse_quorum(query ? query : "", &min_should);
    for (size_t i = 0; i < terms.size() && i < terms_cap; i++) {
        if (roles) roles[i] = terms[i].role;
        if (clauses) clauses[i] = terms[i].clause;
        if (needs) needs[i] = terms[i].need;
        if (promoted) promoted[i] = terms[i].promoted ? 1 : 0;
    }
    nsh_join_terms(terms, buf, cap);
    if (min_should_out) *min_should_out = min_should;
    return (uint32_t)terms.size();
} NSH_CATCH(nullptr, "nsh_parse_quorum", 0)
}

extern "C" int nsh_engine_search_quorum_after_batch(nsh_engine* e, uint32_t filter_handle, const char* const* queries, uint32_t n_queries, int k,
                                                    const nsh_page_cursor* after, void* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                                    uint8_t* has_found, float* device_ms_out) { try {
    return nsh_after_batch(e, "nsh_engine_search_quorum_after_batch", nsx::PageSpec::Quorum, nullptr, filter_handle, queries, n_queries, k, 0u, after, hits, nullptr, nhits, found, rest,
                           has_found, device_ms_out);
} NSH_CATCH(e, "nsh_engine_search_quorum_after_batch", -1)
}

extern "C" int nsh_engine_facet_quorum_batch(nsh_engine* e, const nsh_facet_spec* spec, uint32_t filter_handle, const char* const* queries, uint32_t n_queries,
                                             uint32_t* counts_out, uint64_t counts_cap, uint64_t* found, uint8_t* has_found, float* device_ms_out) { try {
    return nsh_facet_boolean(e, "nsh_engine_facet_quorum_batch", nsx::Dialect::Quorum, spec, filter_handle, queries, n_queries, counts_out, counts_cap, found, has_found, device_ms_out);
} NSH_CATCH(e, "nsh_engine_facet_quorum_batch", -1)
}

extern "C" int nsh_engine_search_quorum_sorted_batch(nsh_engine* e, const nsh_sort_spec* spec, uint32_t filter_handle, const char* const* queries,
                                                     uint32_t n_queries, int k, const nsh_page_cursor* after, void* hits, uint32_t* keys_out, uint32_t* nhits,
                                                     uint64_t* found, uint64_t* rest, uint8_t* has_found, float* device_ms_out) { try {
    return nsh_after_batch(e, "nsh_engine_search_quorum_sorted_batch", nsx::PageSpec::QuorumSorted, spec, filter_handle, queries, n_queries, k, 0u, after, hits, keys_out, nhits, found, rest,
                           has_found, device_ms_out);
} NSH_CATCH(e, "nsh_engine_search_quorum_sorted_batch", -1)
}

extern "C" int nsh_engine_search_quorum_json(nsh_engine* e, const char* query, int k, int use_filter, const char* date_from, const char* date_to,
                                             int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        return e->eng.search_dialect_text(nsx::Dialect::Quorum, query ? query : "", k, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_quorum_json", -1)
}

extern "C" int nsh_engine_search_quorum_faceted_json(nsh_engine* e, const char* query, int k, const nsh_facet_spec* spec, int use_filter, const char* date_from,
                                                     const char* date_to, int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        nsx::FacetSpec sp;
        return nsh_facet_spec_of(e, spec, sp, s) && e->eng.search_dialect_faceted_text(nsx::Dialect::Quorum, query ? query : "", k, sp, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_quorum_faceted_json", -1)
}

extern "C" int nsh_engine_search_quorum_sorted_json(nsh_engine* e, const char* query, int k, const nsh_sort_spec* spec, int use_filter, const char* date_from,
                                                    const char* date_to, int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        nsx::SortSpec sp;
        return nsh_sort_spec_of(e, spec, sp, s) && e->eng.search_dialect_sorted_text(nsx::Dialect::Quorum, query ? query : "", k, sp, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_quorum_sorted_json", -1)
}

// ---- boosts (host/boost.hpp) ----
// in == NULL: no spec (`have` false)
static bool nsh_boost_spec_of(nsh_engine* e, const nsh_boost_spec* in, nsx::BoostSpec& out, bool& have, std::string& why) {
    have = in != nullptr;
    if (!in) return true;
    if (in->kind > 2u) { why = "boost: unknown kind " + std::to_string(in->kind); return false; }
    out.kind = (nsx::BoostSpec::Kind)in->kind;
    out.weight = in->weight;
    out.origin = in->origin ? in->origin : "";
    out.scale_days = in->scale_days;
    out.offset_days = in->offset_days;
    out.undated = in->undated;
    if (out.kind != nsx::BoostSpec::Custom) return true;
    if (in->n_custom && !in->custom) { why = "boost custom: null array"; return false; }
    // whole arrays as far as the factors reach; factors left over become one more: the engine refuses either with a message
    uint64_t at = 0;
    for (const auto& sd : e->eng.segments) {
        if (at + sd.N > in->n_custom) break;
        out.custom.emplace_back(in->custom + at, in->custom + at + sd.N);
        at += sd.N;
    }
    if (out.custom.size() == e->eng.segments.size() && at != in->n_custom) out.custom.emplace_back(in->custom + at, in->custom + in->n_custom);
    return true;
}

extern "C" int64_t nsh_engine_boost_table(nsh_engine* e, const nsh_boost_spec* spec, float* out, uint64_t cap) { try {
    if (!e) return -1;
    nsx::BoostSpec sp;
    std::string why;
    bool have = false;
    if (!nsh_boost_spec_of(e, spec, sp, have, why)) { nsh_set_err(e, why); return -1; }
    if (!have) { nsh_set_err(e, "boost: spec is NULL"); return -1; }
    std::vector<std::vector<float>> tables;
    if (!e->eng.boost_table(sp, tables)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    uint64_t at = 0;
    for (const auto& t : tables) {
        for (size_t i = 0; i < t.size(); i++)
            if (out && at + i < cap) out[at + i] = t[i];
        at += t.size();
    }
    return (int64_t)at;
} NSH_CATCH(e, "nsh_engine_boost_table", -1)
}

extern "C" void nsh_engine_release_boosts(nsh_engine* e) { try { if (e) e->eng.release_boosts(); } NSH_CATCH_VOID(e, "nsh_engine_release_boosts") }
extern "C" uint64_t nsh_engine_boost_tables_on_device(nsh_engine* e) { return e ? (uint64_t)e->eng.boost_tables_on_device() : 0; }

extern "C" uint32_t nsh_parse_boosted(const char* query, char* buf, uint32_t cap, uint8_t* roles, uint32_t* clauses, uint32_t* needs, uint8_t* promoted,
                                      float* weights, uint32_t terms_cap, uint32_t* min_should_out) { try {
    uint32_t min_should = 0;
    const auto terms = nsx::parse_boosted(query ? query : "", &min_should);
    for (size_t i = 0; i < terms.size() && i < terms_cap; i++) {
        if (roles) roles[i] = terms[i].role;
        if (clauses) clauses[i] = terms[i].clause;
        if (needs) needs[i] = terms[i].need;
        if (promoted) promoted[i] = terms[i].promoted ? 1 : 0;
        if (weights) weights[i] = terms[i].weight;
    }
    nsh_join_terms(terms, buf, cap);
    if (min_should_out) *min_should_out = min_should;
    return (uint32_t)terms.size();
} NSH_CATCH(nullptr, "nsh_parse_boosted", 0)
}

extern "C" int nsh_engine_search_boosted_after_batch(nsh_engine* e, const nsh_boost_spec* spec, uint32_t filter_handle, const char* const* queries, uint32_t n_queries,
                                                     int k, const nsh_page_cursor* after, void* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                                     uint8_t* has_found, float* device_ms_out) { try {
    if (!e) return -1;
    nsx::BoostSpec sp;
    std::string why;
    bool have = false;
    if (!nsh_boost_spec_of(e, spec, sp, have, why)) { nsh_set_err(e, why); return -1; }
    return nsh_after_batch(e, "nsh_engine_search_boosted_after_batch", nsx::PageSpec::Boosted, nullptr, filter_handle, queries, n_queries, k, 0u, after, hits, nullptr, nhits, found, rest,
                           has_found, device_ms_out, have ? &sp : nullptr);
} NSH_CATCH(e, "nsh_engine_search_boosted_after_batch", -1)
}

extern "C" int nsh_engine_search_boosted_json(nsh_engine* e, const char* query, int k, const nsh_boost_spec* spec, int use_filter, const char* date_from,
                                              const char* date_to, int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        nsx::BoostSpec sp;
        bool have = false;
        return nsh_boost_spec_of(e, spec, sp, have, s) && e->eng.search_boosted_text(query ? query : "", k, have ? &sp : nullptr, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_boosted_json", -1)
}

// ---- collapsed hits (host/collapse.hpp) ----
static bool nsh_collapse_spec_of(nsh_engine* e, const nsh_collapse_spec* in, nsx::CollapseSpec& out, std::string& why) {
    if (!in) { why = "collapse: spec is NULL"; return false; }
    if (in->kind > 2u) { why = "collapse: unknown kind " + std::to_string(in->kind); return false; }
    out.kind = (nsx::CollapseSpec::Kind)in->kind;
    if (out.kind != nsx::CollapseSpec::Custom) return true;
    if (in->n_custom && !in->custom) { why = "collapse custom: null array"; return false; }
    // whole arrays as far as the keys reach; keys left over become one more: the engine refuses either with a message
    uint64_t at = 0;
    for (const auto& sd : e->eng.segments) {
        if (at + sd.N > in->n_custom) break;
        out.custom.emplace_back(in->custom + at, in->custom + at + sd.N);
        at += sd.N;
    }
    if (out.custom.size() == e->eng.segments.size() && at != in->n_custom) out.custom.emplace_back(in->custom + at, in->custom + in->n_custom);
    return true;
}

extern "C" int64_t nsh_engine_collapse_table(nsh_engine* e, const nsh_collapse_spec* spec, uint32_t* out, uint64_t cap) { try {
    if (!e) return -1;
    nsx::CollapseSpec sp;
    std::string why;
    if (!nsh_collapse_spec_of(e, spec, sp, why)) { nsh_set_err(e, why); return -1; }
    std::vector<std::vector<uint32_t>> tables;
    if (!e->eng.collapse_table(sp, tables)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    uint64_t at = 0;
    for (const auto& t : tables) {
        for (size_t i = 0; i < t.size(); i++)
            if (out && at + i < cap) out[at + i] = t[i];
        at += t.size();
    }
    return (int64_t)at;
} NSH_CATCH(e, "nsh_engine_collapse_table", -1)
}

extern "C" void nsh_engine_release_collapse(nsh_engine* e) { try { if (e) e->eng.release_collapse(); } NSH_CATCH_VOID(e, "nsh_engine_release_collapse") }
extern "C" uint64_t nsh_engine_collapse_tables_on_device(nsh_engine* e) { return e ? (uint64_t)e->eng.collapse_tables_on_device() : 0; }

extern "C" int nsh_engine_search_collapsed_batch(nsh_engine* e, const nsh_collapse_spec* collapse, const nsh_boost_spec* boost, uint32_t filter_handle,
                                                 const char* const* queries, uint32_t n_queries, int k, void* hits, uint32_t* groups, uint32_t* others,
                                                 uint32_t* nhits, uint64_t* found, uint8_t* has_found, float* device_ms_out) { try {
    if (!e) return -1;
    nsx::CollapseSpec cs;
    nsx::BoostSpec bs;
    std::string why;
    bool have = false;
    if (!nsh_collapse_spec_of(e, collapse, cs, why) || !nsh_boost_spec_of(e, boost, bs, have, why)) { nsh_set_err(e, why); return -1; }
    if (n_queries && (!queries || !hits || !groups || !nhits)) { nsh_set_err(e, "nsh_engine_search_collapsed_batch: null argument"); return -1; }
    std::vector<nextsearch::Engine::QueryView> views(n_queries);
    for (uint32_t q = 0; q < n_queries; q++) views[q] = {queries[q] ? queries[q] : "", queries[q] ? std::strlen(queries[q]) : 0};
    std::vector<uint64_t> f_;
    std::vector<uint8_t> u_;
    if (!found) { f_.resize(n_queries); found = f_.data(); }
    if (!has_found) { u_.resize(n_queries); has_found = u_.data(); }
    if (!e->eng.search_collapsed_batch_flat(cs, have ? &bs : nullptr, filter_handle, views.data(), n_queries, k, (ns_hit*)hits, groups, others, nhits, found, has_found,
                                            device_ms_out)) {
        nsh_set_err(e, e->eng.last_error());
        return -1;
    }
    for (uint32_t q = 0; q < n_queries; q++)
        if (!has_found[q]) found[q] = 0;
    return 0;
} NSH_CATCH(e, "nsh_engine_search_collapsed_batch", -1)
}

extern "C" int nsh_engine_search_collapsed_json(nsh_engine* e, const char* query, int k, const nsh_collapse_spec* collapse, const nsh_boost_spec* boost,
                                                int use_filter, const char* date_from, const char* date_to, int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        nsx::CollapseSpec cs;
        nsx::BoostSpec bs;
        bool have = false;
        return nsh_collapse_spec_of(e, collapse, cs, s) && nsh_boost_spec_of(e, boost, bs, have, s) &&
               e->eng.search_collapsed_text(query ? query : "", k, cs, have ? &bs : nullptr, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_collapsed_json", -1)
}

extern "C" int nsh_engine_search_boosted_page_json(nsh_engine* e, const char* query, int k, const char* cursor, const nsh_boost_spec* spec, int use_filter,
                                                   const char* date_from, const char* date_to, int keep_undated, char** json_out) { try {
    if (!e || !json_out) return -1;
    *json_out = nullptr;
    std::string s;
    nsx::PageSpec ps;
    ps.mode = nsx::PageSpec::Boosted;
    bool ok = nsh_boost_spec_of(e, spec, ps.boost, ps.use_boost, s);
    if (ok) {
        ps.use_filter = use_filter != 0;
        if (ps.use_filter) ps.filter = nsh_doc_filter(date_from, date_to, keep_undated);
        ok = e->eng.search_page_text(query ? query : "", k, cursor ? cursor : "", ps, s);
    }
    return nsh_json_out(e, ok, s, json_out);
} NSH_CATCH(e, "nsh_engine_search_boosted_page_json", -1)
}

// ---- prefix terms (host/prefix.hpp) ----
static nsx::PrefixSpec nsh_prefix_spec_of(uint32_t max_expansions) {
    nsx::PrefixSpec ps;
    if (max_expansions) ps.max_expansions = max_expansions;
    return ps;
}

extern "C" uint32_t nsh_parse_prefixed(const char* query, char* buf, uint32_t cap, uint8_t* roles, uint32_t* clauses, uint32_t* needs, uint8_t* promoted,
                                       float* weights, uint8_t* prefix, uint32_t terms_cap, uint32_t* min_should_out) { try {
    uint32_t min_should = 0;
    const auto terms = nsx::parse_prefixed(query ? query : "", &min_should);
    for (size_t i = 0; i < terms.size() && i < terms_cap; i++) {
        if (roles) roles[i] = terms[i].role;
        if (clauses) clauses[i] = terms[i].clause;
        if (needs) needs[i] = terms[i].need;
        if (promoted) promoted[i] = terms[i].promoted ? 1 : 0;
        if (weights) weights[i] = terms[i].weight;
        if (prefix) prefix[i] = terms[i].prefix ? 1 : 0;
    }
    nsh_join_terms(terms, buf, cap);
    if (min_should_out) *min_should_out = min_should;
    return (uint32_t)terms.size();
} NSH_CATCH(nullptr, "nsh_parse_prefixed", 0)
}

extern "C" int64_t nsh_engine_expand_prefix(nsh_engine* e, const char* prefix, uint32_t max_expansions, char* buf, uint64_t cap, uint64_t* bytes_out, int* truncated_out) { try {
    if (!e) return -1;
    std::vector<std::string> terms;
    bool truncated = false;
    if (!e->eng.expand_prefix(prefix ? prefix : "", nsh_prefix_spec_of(max_expansions).max_expansions, terms, truncated)) { nsh_set_err(e, e->eng.last_error()); return -1; }
    std::string joined;
    for (size_t i = 0; i < terms.size(); i++) {
        if (i) joined.push_back(' ');
        joined += terms[i];
    }
    if (bytes_out) *bytes_out = joined.size() + 1;
    if (buf && cap) {
        const size_t n = std::min<size_t>(joined.size(), cap - 1);
        std::memcpy(buf, joined.data(), n);
        buf[n] = 0;
    }
    if (truncated_out) *truncated_out = truncated ? 1 : 0;
    return (int64_t)terms.size();
} NSH_CATCH(e, "nsh_engine_expand_prefix", -1)
}

extern "C" int nsh_engine_search_prefixed_after_batch(nsh_engine* e, const nsh_boost_spec* spec, uint32_t max_expansions, uint32_t filter_handle, const char* const* queries,
                                                      uint32_t n_queries, int k, const nsh_page_cursor* after, void* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                                      uint8_t* has_found, float* device_ms_out) { try {
    const char* fn = "nsh_engine_search_prefixed_after_batch";
    if (!e) return -1;
    nsx::BoostSpec sp;
    std::string why;
    bool have = false;
    if (!nsh_boost_spec_of(e, spec, sp, have, why)) { nsh_set_err(e, why); return -1; }
    if (n_queries && (!queries || !hits || !nhits)) { nsh_set_err(e, std::string(fn) + ": null argument"); return -1; }
    std::vector<nextsearch::Engine::QueryView> views(n_queries);
    for (uint32_t q = 0; q < n_queries; q++) views[q] = {queries[q] ? queries[q] : "", queries[q] ? std::strlen(queries[q]) : 0};
    std::vector<nsx::PageCursor> cur;
    nsh_cursors_of(after, n_queries, cur);
    std::vector<uint64_t> f_, r_;
    std::vector<uint8_t> u_;
    if (!found) { f_.resize(n_queries); found = f_.data(); }
    if (!rest) { r_.resize(n_queries); rest = r_.data(); }
    if (!has_found) { u_.resize(n_queries); has_found = u_.data(); }
    if (!e->eng.search_prefixed_after_batch_flat(have ? &sp : nullptr, nsh_prefix_spec_of(max_expansions), filter_handle, views.data(), n_queries, k, after ? cur.data() : nullptr,
                                                 (ns_hit*)hits, nhits, found, rest, has_found, device_ms_out)) {
        nsh_set_err(e, e->eng.last_error());
        return -1;
    }
    for (uint32_t q = 0; q < n_queries; q++)
        if (!has_found[q]) found[q] = rest[q] = 0;
    return 0;
} NSH_CATCH(e, "nsh_engine_search_prefixed_after_batch", -1)
}

extern "C" int nsh_engine_search_prefixed_json(nsh_engine* e, const char* query, int k, const nsh_boost_spec* spec, uint32_t max_expansions, int use_filter,
                                               const char* date_from, const char* date_to, int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        nsx::BoostSpec sp;
        bool have = false;
        return nsh_boost_spec_of(e, spec, sp, have, s) && e->eng.search_prefixed_text(query ? query : "", k, have ? &sp : nullptr, nsh_prefix_spec_of(max_expansions), f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_prefixed_json", -1)
}

extern "C" int nsh_engine_search_prefixed_page_json(nsh_engine* e, const char* query, int k, const char* cursor, const nsh_boost_spec* spec, uint32_t max_expansions,
                                                    int use_filter, const char* date_from, const char* date_to, int keep_undated, char** json_out) { try {
    if (!e || !json_out) return -1;
    *json_out = nullptr;
    std::string s;
    nsx::PageSpec ps;
    ps.mode = nsx::PageSpec::Prefixed;
    ps.prefix = nsh_prefix_spec_of(max_expansions);
    bool ok = nsh_boost_spec_of(e, spec, ps.boost, ps.use_boost, s);
    if (ok) {
        ps.use_filter = use_filter != 0;
        if (ps.use_filter) ps.filter = nsh_doc_filter(date_from, date_to, keep_undated);
        ok = e->eng.search_page_text(query ? query : "", k, cursor ? cursor : "", ps, s);
    }
    return nsh_json_out(e, ok, s, json_out);
} NSH_CATCH(e, "nsh_engine_search_prefixed_page_json", -1)
}

static int nsh_facet_boolean(nsh_engine* e, const std::string& fn, nsx::Dialect dialect, const nsh_facet_spec* spec, uint32_t filter_handle, const char* const* queries,
                             uint32_t n_queries, uint32_t* counts_out, uint64_t counts_cap, uint64_t* found, uint8_t* has_found, float* device_ms_out) {
    if (!e) return -1;
    nsx::FacetSpec sp;
    std::string why;
    if (!nsh_facet_spec_of(e, spec, sp, why)) { nsh_set_err(e, why); return -1; }
    if (n_queries && !queries) { nsh_set_err(e, fn + ": queries is NULL"); return -1; }
    std::vector<nextsearch::Engine::QueryView> views(n_queries);
    for (uint32_t q = 0; q < n_queries; q++) views[q] = {queries[q] ? queries[q] : "", queries[q] ? std::strlen(queries[q]) : 0};
    std::vector<uint64_t> f_;
    std::vector<uint8_t> u_;
    if (!found) { f_.resize(n_queries); found = f_.data(); }
    if (!has_found) { u_.resize(n_queries); has_found = u_.data(); }
    std::vector<uint32_t> counts;
    std::vector<std::string> labels;
    const bool ok = e->eng.facet_dialect_batch_flat(dialect, sp, filter_handle, views.data(), n_queries, counts, found, has_found, labels, device_ms_out);
    if (!ok) { nsh_set_err(e, e->eng.last_error()); return -1; }
    if (counts.size() > counts_cap || (!counts.empty() && !counts_out)) {
        nsh_set_err(e, fn + ": counts_out holds " + std::to_string(counts_cap) + " entries, " + std::to_string(n_queries) + " queries x " +
                           std::to_string(labels.size()) + " buckets need " + std::to_string(counts.size()));
        return -1;
    }
    if (!counts.empty()) std::memcpy(counts_out, counts.data(), counts.size() * 4);
    for (uint32_t q = 0; q < n_queries; q++)
        if (!has_found[q]) found[q] = 0;
    return 0;
}

extern "C" int nsh_engine_search_boolean_sorted_batch(nsh_engine* e, const nsh_sort_spec* spec, uint32_t filter_handle, const char* const* queries,
                                                      uint32_t n_queries, int k, const nsh_page_cursor* after, void* hits, uint32_t* keys_out, uint32_t* nhits,
                                                      uint64_t* found, uint64_t* rest, uint8_t* has_found, float* device_ms_out) { try {
    return nsh_after_batch(e, "nsh_engine_search_boolean_sorted_batch", nsx::PageSpec::BooleanSorted, spec, filter_handle, queries, n_queries, k, 0u, after, hits, keys_out, nhits, found, rest,
                           has_found, device_ms_out);
} NSH_CATCH(e, "nsh_engine_search_boolean_sorted_batch", -1)
}

extern "C" int nsh_engine_search_boolean_faceted_json(nsh_engine* e, const char* query, int k, const nsh_facet_spec* spec, int use_filter, const char* date_from,
                                                      const char* date_to, int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        nsx::FacetSpec sp;
        return nsh_facet_spec_of(e, spec, sp, s) && e->eng.search_dialect_faceted_text(nsx::Dialect::Boolean, query ? query : "", k, sp, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_boolean_faceted_json", -1)
}

extern "C" int nsh_engine_search_boolean_sorted_json(nsh_engine* e, const char* query, int k, const nsh_sort_spec* spec, int use_filter, const char* date_from,
                                                     const char* date_to, int keep_undated, char** json_out) { try {
    return nsh_text_json(e, use_filter, date_from, date_to, keep_undated, json_out, [&](const nsx::DocFilter* f, std::string& s) {
        nsx::SortSpec sp;
        return nsh_sort_spec_of(e, spec, sp, s) && e->eng.search_dialect_sorted_text(nsx::Dialect::Boolean, query ? query : "", k, sp, f, s);
    });
} NSH_CATCH(e, "nsh_engine_search_boolean_sorted_json", -1)
}

extern "C" int nsh_engine_search_page_json(nsh_engine* e, const char* query, int k, const char* cursor, uint32_t mode, const nsh_sort_spec* spec, int use_filter,
                                           const char* date_from, const char* date_to, int keep_undated, char** json_out) { try {
    if (!e || !json_out) return -1;
    *json_out = nullptr;
    std::string s;
    nsx::PageSpec ps;
    bool ok = mode <= 9u;   // (9: boosted without a spec; nsh_engine_search_boosted_page_json takes one)
    if (!ok) s = "search_page: unknown mode " + std::to_string(mode);
    if (ok) {
        ps.mode = (nsx::PageSpec::Mode)mode;
        if (nsx::page_kind(ps.mode) == 'd') ok = nsh_sort_spec_of(e, spec, ps.sort, s);
    }
    if (ok) {
        ps.use_filter = use_filter != 0;
        if (ps.use_filter) ps.filter = nsh_doc_filter(date_from, date_to, keep_undated);
        ok = e->eng.search_page_text(query ? query : "", k, cursor ? cursor : "", ps, s);
    }
    return nsh_json_out(e, ok, s, json_out);
} NSH_CATCH(e, "nsh_engine_search_page_json", -1)
}
