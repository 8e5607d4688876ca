// Host facade mirroring the reference's cord19::Engine query interface
// (include/api_engine.hpp:23-91): reload() and search(query, k) -> JSON keep their names, argument
// meaning and error behaviour; search_batch() is additive (a batch == Q independent searches).
//
// What stays on the host (reference file:line):
//   tokenise / stop-word filter      include/textutil.hpp:13-37, src/api_engine.cpp:388-397
//   lexicon probe per segment        src/api_engine.cpp:454-458
//   bm25_idf via glibc logf          src/api_engine.cpp:45-47,461
//   JSON assembly                    src/api_engine.cpp:400-404,505-536
// What crosses the C-ABI (include/nextsearch_hip.h) to the MI355X kernels:
//   posting traversal, BM25 term scores, accumulation, top-k, found   src/api_engine.cpp:441-504
//
//   result decoration from metadata.csv (title, url, publish_time, author): src/api_engine.cpp:516-531
// Autocomplete (include/api_engine.hpp:67, src/api_engine.cpp:91-107,:164-187): suggest() / suggest_batch() answer from
// a sorted table built at reload() (suggest.hpp) and uploaded to the primary device (csrc/ns_suggest.hip).
// Out of scope here: the AI overview and AI summary caches.  There is no CPU scoring or autocomplete
// path: without a device search*() and suggest*() fail.
#pragma once

#include <cstdint>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/nextsearch_hip.h"
#include "forward_index.hpp"
#include "compact.hpp"
#include "purge.hpp"
#include "index_format.hpp"
#include "metadata.hpp"
#include "semantic.hpp"
#include "related.hpp"
#include "similar.hpp"
#include "correct.hpp"
#include "filter.hpp"
#include "facet.hpp"
#include "sorted.hpp"
#include "boolean.hpp"
#include "grouped.hpp"
#include "quorum.hpp"
#include "boost.hpp"
#include "collapse.hpp"
#include "prefix.hpp"
#include "page.hpp"
#include "suggest.hpp"
#include "term_dict.hpp"
#include "../csrc/ns_forkjoin.hpp"

namespace nextsearch {

struct SearchHit {
    float score;
    uint32_t seg;
    uint32_t doc;
};

struct SearchResult {
    std::string query;
    int k = 0;               // clamped K
    int segments = 0;
    bool has_found = false;  // false on the early-return path (src/api_engine.cpp:407): no "found" key
    uint64_t found = 0;
    std::vector<SearchHit> hits;
};

// bm25_idf (src/api_engine.cpp:45-47): u32 subtraction first, then int->float, fp32 throughout.
float bm25_idf(uint32_t N, uint32_t df);

class Engine {
public:
    nsx::fs::path index_dir;
    std::vector<std::string> seg_names;
    std::vector<nsx::SegmentData> segments;
    nsx::MetadataTable meta;   // <index>/metadata.csv, parsed once at reload() (src/api_engine.cpp:110-113,:516-531)
    nsx::SemanticTable sem;    // optional embeddings (src/api_engine.cpp:115-153): when loaded, every search expands its terms (:409-417)
    // term -> per-segment {byte_off, count, idf}, built at reload() next to the lexicons (term_dict.hpp):
    // the one probe per query term that replaces the reference's per-(term, segment) seg.lex.find + bm25_idf (:454-461)
    nsx::TermDict dict;
    // autocomplete's sorted (term, score) table (suggest.hpp), rebuilt by every reload(); its device copy lives on the
    // primary context.  suggest_build_ms: the table's host build (sums, normalising, sort); suggest_upload_ms: its upload
    // and the device tree build (ns_ac_upload), both of the last reload().
    nsx::SuggestTable suggest_table;
    double suggest_build_ms = 0.0, suggest_upload_ms = 0.0;
    // the spelling corrector's side structures on that device copy (ns_ac_build_fuzzy): built by the first correct_batch /
    // did_you_mean after a reload(), never by reload() itself; the time of that build (0 until it happened)
    double correct_build_ms = 0.0;

    // device < 0: host-only (index + query preparation; every search call fails loudly)
    explicit Engine(int device = 0);
    // SURVEY.md 8(e), "one host thread + ns_ctx per GPU": the index is REPLICATED on every listed device (reload() uploads
    // it to each), and search_batch_flat / search_batch cut a batch into contiguous shards of ceil(Q / N) queries, one per
    // device, each driven by its own host thread through its own context; the shards' results land in the caller's one
    // set of host arrays (plain D2H per device: in one process no collective is needed — bench.py's multi-PROCESS form
    // keeps the RCCL all-gather).  Queries are independent (the reference serialises them behind one mutex,
    // src/api_engine.cpp:372), so the cut changes no result.  The same device may be listed twice (two contexts on one
    // GPU: what the one-GPU test box exercises).  devices[0] is the primary context: single searches, semantic
    // expansion's similarity search and ctx() use it.
    explicit Engine(const std::vector<int>& devices);
    size_t num_devices() const { return 1 + replicas_.size(); }
    // [begin, end) of shard r of n over Q queries: contiguous, ceil(Q / n) each, the last ones short or empty
    static std::pair<size_t, size_t> shard_bounds(size_t Q, size_t r, size_t n) {
        const size_t per = n ? (Q + n - 1) / n : Q;
        return {std::min(Q, r * per), std::min(Q, (r + 1) * per)};
    }
    ~Engine();
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;

    bool reload();                                              // include/api_engine.hpp:65
    // What the reference's `adddocument` tool (src/AddDocument.cpp:20-60,:160-170) and its disabled /api/add_document
    // (src/api_add_document.cpp:252-421) do, for a batch: the documents become ONE new segment, the next free seg_%06u
    // under <index>/segments — forward index on the device (forward_index.hpp), inverted on the device (invert.hpp) —
    // which is appended to manifest.bin (a missing manifest is an empty list, src/AddDocument.cpp:23), then reload().
    // Works on a fresh index directory and on an engine whose reload() has not succeeded yet.  On any failure the
    // manifest keeps its bytes and the new segment directory is removed; if no document has a token left after the
    // length and stop-word rules that is a failure and nothing is written.  stats (may be null): the indexing step's.
    bool add_documents(const std::vector<nsx::DocInput>& docs, nsx::IndexStats* stats = nullptr);
    // Compaction (host/compact.hpp): the segments at manifest positions [first, first + count) (clamped)
    // become ONE new segment, the next free seg_%06u, which takes the range's place in the manifest; the engine reloads.
    // Fewer than two segments in the range: success, nothing touched.  All or nothing like add_documents: on any failure the
    // manifest keeps its bytes, the new directory is removed, no source is touched and the engine keeps answering from the
    // index it had.  The source directories are removed only after the reload succeeded and only with remove_sources; a
    // failure to remove one is reported in last_error() while the call returns true.  Needs a device (device < 0: fails).
    bool compact(size_t first = 0, size_t count = SIZE_MAX, bool remove_sources = true, nsx::CompactStats* stats = nullptr);
    // Deleting (host/purge.hpp).  find_documents: every (manifest position, docId) of the index this engine
    // serves whose docs.bin uid equals one of uids, ascending; host only (it reads what reload() loaded from docs.bin),
    // so it works on a host-only engine too.  Always true; uids that match nothing simply add no pair.
    bool find_documents(const std::vector<std::string>& uids, std::vector<std::pair<uint32_t, uint32_t>>& out);
    // delete_documents: every document that carries a listed uid is deleted, in every segment; duplicates of a uid in the
    // index all go.  A listed uid that matches nothing is counted in uids_not_found (once, however often it is listed) and
    // is not an error; if nothing matches, the call succeeds and nothing is touched.
    // delete_by_id: the same for (manifest position, docId) pairs.  A pair out of range is refused and nothing is touched;
    // a pair listed twice counts once.
    // Each affected segment is rewritten on its own into the next free seg_%06u — one ns_forward_merge_keep over the one
    // source and one ns_forward_invert; docs.bin = the surviving records copied raw, stats.bin's avgdl as compaction
    // computes it, the files written by compaction's writer — and the new segment takes the old one's place in the
    // manifest.  Untouched segments are neither read nor rewritten.  A segment with no survivor is dropped from the manifest
    // and the later positions move up.  THE SURVIVORS OF A REWRITTEN SEGMENT GET NEW docIds, their positions among the
    // survivors: the uid is the stable handle of a document, a (position, docId) pair is good until the next delete or
    // compaction.  Term ids are renumbered too; no search result depends on them.
    // All or nothing like compact: the manifest is written once, after every new segment is complete, then reload() runs
    // (which rebuilds autocomplete's table and empties the search cache); on any failure the manifest keeps its bytes, every
    // new directory is removed and the engine keeps answering from the index it had.  The old directories are removed only
    // after the reload succeeded; a failure to remove one is reported in last_error() while the call returns true.
    // A call that would delete every document of the index fails and touches nothing (an index without a segment cannot be
    // loaded).  Needs a device (device < 0: fails, and says so).  stats may be null.
    bool delete_documents(const std::vector<std::string>& uids, nsx::DeleteStats* stats = nullptr);
    bool delete_by_id(const std::vector<std::pair<uint32_t, uint32_t>>& seg_doc, nsx::DeleteStats* stats = nullptr);
    // Optional: per-posting term scores for every list of every lexicon, built on the device
    // (ns_segment_build_impacts); searches then read {docId, score} instead of {docId, tf} + norm.  Same results.
    bool build_impacts();
    void use_impacts(bool on);
    // reload() builds skip tables for every segment's frequent lists (ns_segment_build_skips); off = searches ignore them
    void use_skips(bool on);
    // Optional: blocks of 256 postings with 8/16/32-bit docId offsets, 8-bit tf and a 16-bit norm index,
    // built on the device next to the raw stream (ns_segment_build_packed); the driver streams then read 4-7 B per posting
    // instead of 12.  Same results.
    bool build_packed();
    // Optional (block-max scores): per 256 postings of every list of >= 512 postings the largest term score,
    // built on the device (ns_segment_build_blockmax).  use_pruning(true): single-term queries then skip, unread, the blocks
    // that cannot enter their top-K; `found` stays exact (it is the list's posting count).  Same results; off by default.
    bool build_blockmax();
    void use_pruning(bool on);
    // groups of exactly two lists: the two-list merge body (default) or the driver-stream body like every other group
    void use_merge(bool on);
    // ns_ctx_share_scores on every device context: 0 never, 1 (default) batches that name their lists often enough, 2 always
    void share_scores(int mode);
    void use_packed(int mode);   // 0 off, 1 packed docIds + tf with the fp32 norm stream (default), 2 norms through the 16-bit index
    std::string search(const std::string& query, int k);        // include/api_engine.hpp:66 (JSON text, dump(2) layout)
    // Search-result cache around search() (src/api_engine.cpp:190-250,:380-385,:539): key "query|K", at most 2600
    // entries, least recently used evicted, a hit returns the stored body plus "from_cache": true.  In memory only:
    // the reference also rewrites search_cache.json in the CWD on every insert (:245-249), which is not reproduced.
    bool search_text(const std::string& query, int k, std::string& body);   // search() with the failure visible to the caller (body = the message then)
    static constexpr size_t kMaxCacheSize = 2600;               // include/api_engine.hpp:42
    bool search_hits(const std::string& query, int k, uint32_t flags, SearchResult& out);
    bool search_batch(const std::vector<std::string>& queries, int k, uint32_t flags, std::vector<SearchResult>& out);
    // The same batch with flat, caller-owned outputs in the C-ABI's layout — hits Q x K (unused tail entries {-inf, ~0, ~0}),
    // nhits[Q], found[Q], usable[Q] (0 = the early return of src/api_engine.cpp:407: no "found") — and no per-query
    // allocation.  A large batch is cut into sub-batches that are pipelined on the one device context: the host prepares
    // sub-batch i+1 (tokenise, dictionary probes) while the device scores sub-batch i (include/nextsearch_hip.h:
    // NS_RUN_FETCH).  A batch == Q independent searches, so the cut changes no result.
    struct QueryView { const char* p; size_t n; };
    bool search_batch_flat(const QueryView* queries, size_t Q, int k, uint32_t flags, ns_hit* hits, uint32_t* nhits,
                           uint64_t* found, uint8_t* usable);

    // Query preparation only: flattened term refs in the C-ABI's layout.
    // usable[q] == 0 marks the early-return case (no base terms, or no segments).
    // `expanded`: the queries' weighted terms from semantic expansion (nullptr: base terms, weight 1.0)
    void build_refs_range(const std::vector<std::string>& queries, size_t q0, size_t q1, std::vector<ns_query_desc>& qd,
                          std::vector<ns_term_ref>& refs, std::vector<uint8_t>& usable,
                          const std::vector<nsx::WeightedTerms>* expanded = nullptr, const nsx::RowSource& rs = nsx::RowSource{},
                          bool and_mode = false) const;
    // The weighted query terms a search scores (base terms, or their semantic expansion when embeddings are loaded)
    bool expand_queries(const std::vector<std::string>& queries, std::vector<nsx::WeightedTerms>& out) const;
    void build_refs(const std::vector<std::string>& queries, std::vector<ns_query_desc>& qd,
                    std::vector<ns_term_ref>& refs, std::vector<uint8_t>& usable) const;
    // Staged form used by bench.py: descriptors resident on the device, caller drives ns_batch_*.
    bool prepare(const std::vector<std::string>& queries, int k, uint32_t flags, ns_batch** out);

    // Engine::suggest (include/api_engine.hpp:67, src/api_engine.cpp:164-187): JSON text {"limit", "query",
    // "suggestions"} in dump(2) layout.  Without a device context it returns {"error": ...} (suggest_text: the failure
    // visible to the caller, body = the message).
    std::string suggest(const std::string& input, int limit);
    bool suggest_text(const std::string& input, int limit, std::string& body);
    // A batch of suggest requests with flat, caller-owned outputs: for input q, L = clamp(limit, 1, 10) entries
    // term_idx[q * L + r] (rows of suggest_table, best first, ~0u past count[q]) and base_len[q]: suggestion r is
    // input[0, base_len[q]) + suggest_table term term_idx[q * L + r].  A large batch is cut into sub-batches whose host
    // preparation overlaps the device's work on the previous one.  device_ms (may be null): summed kernel time.
    bool suggest_batch(const QueryView* inputs, size_t Q, int limit, uint32_t* term_idx, uint32_t* count, uint32_t* base_len,
                       float* device_ms = nullptr);

    // Spelling correction (correct.hpp, csrc/ns_fuzzy.hip).  For term q (normalised like the table's terms)
    // the L = clamp(limit, 1, 10) best candidates of suggest_table within max_edits (0..2; -1 = auto by normalised
    // length: < 3 bytes 0, 3..5 one, above two) that share the term's first min(prefix_len, length) bytes: rows
    // term_idx[q * L + r] (best first, ~0u past count[q]) with their distances dist[q * L + r] (0xff past the end).
    // Ranked by (distance, score desc, index asc).  Large batches are cut and pipelined like suggest_batch's.
    bool correct_batch(const QueryView* terms, size_t Q, int limit, int max_edits, int prefix_len, uint32_t* term_idx, uint8_t* dist,
                       uint32_t* count, float* device_ms = nullptr);
    // "Did you mean": JSON text {"changed", "corrected", "query", "terms": [{"known", "suggestions": [{"distance",
    // "score", "term"}], "token"}]} in dump(2) layout.  Tokens are the query's alnum runs without stop words and
    // one-byte tokens; a token the term dictionary holds is known and keeps its place; an unknown one gets its best L
    // (auto edits, no prefix) and, in "corrected", is replaced by the best of them.  Without a device context:
    // {"error": ...} (did_you_mean_text: false, body = the message).
    std::string did_you_mean(const std::string& query, int limit);
    bool did_you_mean_text(const std::string& query, int limit, std::string& body);

    // Typo-tolerant completion (csrc/ns_fuzzy.hip k_fp_*): suggest for a prefix that is still being typed and
    // already has a typo in it.  An input is split like suggest_batch's (last alnum run, normalised = the prefix; the bytes
    // before it = the base, base_len[q]); the answer is the L = clamp(limit, 1, 10) best candidates of suggest_table some
    // prefix of which is within max_edits (0..2; -1 = auto by the normalised prefix length, as correct_batch) of the
    // prefix, and which share its first min(prefix_len, length) bytes exactly.  Rows and ranking as correct_batch's.
    bool complete_batch(const QueryView* inputs, size_t Q, int limit, int max_edits, int prefix_len, uint32_t* term_idx, uint8_t* dist,
                        uint32_t* count, uint32_t* base_len, float* device_ms = nullptr);
    // JSON text {"limit", "query", "suggestions": [{"distance", "score", "suggestion", "term"}]} in dump(2) layout;
    // suggestion = base + term.  Auto edits, prefix_len 1 (the first typed byte is trusted).  Without a device context:
    // {"error": ...} (complete_text: false, body = the message).  suggest() itself is unchanged.
    std::string complete(const std::string& input, int limit);
    bool complete_text(const std::string& input, int limit, std::string& body);

    // "More like this" (host/similar.hpp, csrc/ns_similar.hip).  Source q is the document seg_doc[q] =
    // (manifest position, docId), as delete_by_id names documents; a pair out of range is refused and nothing runs.  Its
    // most telling terms are selected on the device from its forward pairs (ns_docterms_select; the segment's OWN df / idf),
    // turned into byte strings through the segment's terms.bin and scored over EVERY segment as one weighted OR query, in
    // selection order (the fp32 accumulation order), qweight 1.0f or, with opt.boost, w / w_first.  The search runs with
    // K + 1, K = clamp(k, 1, 99); the source's own hit is removed if it is among the K + 1, otherwise the last hit is dropped.
    // hits Q x K (unused tail entries {-inf, ~0, ~0}), nhits[Q], found[Q] = the search's found - 1 (the source always matches
    // its own terms), usable[Q] (0 = nothing selected: no hits, no found).  terms_out (may be null): per source the selected
    // (term, w) in selection order, w = (float)tf * idf.  No semantic expansion, no search cache.  The device copy of a
    // segment's forward index is built by the first call that names the segment (never by reload()) on the primary context,
    // and freed by reload(), release_similar() and the destructor.  A segment without forward.bin / terms.bin (legacy
    // segments, gen_index output) fails the call with a message that names it; so does an engine without a device.
    bool similar_batch(const std::pair<uint32_t, uint32_t>* seg_doc, size_t Q, int k, const nsx::SimilarOptions& opt, ns_hit* hits,
                       uint32_t* nhits, uint64_t* found, uint8_t* usable, std::vector<nsx::WeightedTerms>* terms_out = nullptr);
    // JSON text {"found", "k", "query_terms": [{"term", "weight"}], "results": [search's entries], "segments", "source":
    // {"cord_uid", "docId", "segment"}} in dump(2) layout, default options.  The uid is resolved with find_documents; the
    // first match is the source.  An unknown uid, or any failure: {"error": ...} (more_like_this_text: false, body = the message).
    std::string more_like_this(const std::string& uid, int k);
    bool more_like_this_text(const std::string& uid, int k, std::string& body);
    void release_similar();
    size_t similar_segments_on_device() const;   // segments whose forward index has a device copy right now
    // df / idf by term id of segment seg as similar_batch uploads them (host only: works without a device)
    bool similar_term_stats(uint32_t seg, std::vector<uint32_t>& df, std::vector<float>& idf);

    // Related terms (host/related.hpp, csrc/ns_terms.hip): what a set of documents is about.  Row q is the
    // documents seg_doc[row_off[q] .. row_off[q + 1]) = (manifest position, docId), of any segments; a pair out of range or a
    // row_off that does not start at 0 or descends is refused and nothing runs.  The rows are split by segment; every touched
    // segment answers its parts with ONE ns_docterms_aggregate (max_terms = 64) over ensure_similar's handle, and the lists
    // meet on the host by related.hpp's merge rule: docs summed, df summed over all loaded segments, idf = bm25_idf(N, df),
    // w = (float)docs * idf.  With one loaded segment the options reach the device as they are and the answer is the device
    // row; with several the device counts with min_docs 1 and no df bounds, and min_docs / min_df / max_df judge the summed
    // numbers — a term that misses one segment's 64 is undercounted there (compact() makes it exact).  At most
    // kRelatedMaxDocs distinct documents of a row per segment.  Outputs Q x To, To = clamp(opt.max_terms, 1, 32):
    // docs_out / df_out / w_out [q * To + r] for r < count_out[q] (0 past it), ndocs_out[q] = the row's distinct documents,
    // terms_out (may be null) the byte strings.  device_ms (may be null): the aggregate calls' kernel time summed.
    bool terms_batch(const std::pair<uint32_t, uint32_t>* seg_doc, const uint64_t* row_off, size_t Q, const nsx::RelatedOptions& opt,
                     uint32_t* docs_out, uint64_t* df_out, float* w_out, uint32_t* count_out, uint32_t* ndocs_out,
                     std::vector<std::vector<std::string>>* terms_out = nullptr, float* device_ms = nullptr);
    // JSON text {"found", "query", "sample", "segments", "terms": [{"df", "docs", "term", "weight"}]} in dump(2) layout: the
    // plain search (under the filter when one is given) with K = clamp(opt.sample, 1, 100); its hits are one row ("sample" =
    // how many); the terms the query's own tokens name are dropped before the cut, which keeps the answer exact for queries of
    // at most 32 distinct terms (a segment's list holds 64).  No hits: "terms": [].  Any failure: {"error": ...}
    // (related_terms_text: false, body = the message).
    std::string related_terms(const std::string& query, const nsx::RelatedOptions& opt = {}, const nsx::DocFilter* f = nullptr);
    bool related_terms_text(const std::string& query, const nsx::RelatedOptions& opt, const nsx::DocFilter* f, std::string& body);

    // Filtered search (host/filter.hpp, csrc/ns_filter.hip).  A filter is one keep-bitmap per segment, in
    // manifest order, ceil(N / 32) words each.  filter_bits: the bitmaps of a date filter from metadata.csv's publish_time
    // (host only: works on a host-only engine); false for a malformed bound.  The unused bits of a last word are 0.
    bool filter_bits(const nsx::DocFilter& f, std::vector<std::vector<uint32_t>>& bits);
    // open_filter: per segment with a kept document ONE ns_segment_filter over every list of the dictionary, on the primary
    // context; the copies get the device ids (slot + 1) * S + position (S = segments of the index), so the order inside a
    // filter is manifest order.  A segment without a kept document or without a surviving posting gets no copy.  Lists of
    // reload()'s size get skip tables.  At most kMaxFilters are open; all or nothing.  The handle is good until
    // close_filter, the next reload() (add_documents, compact and delete_* reload) or the destructor.
    static constexpr size_t kMaxFilters = 8;
    static constexpr size_t kFilterLru = 4;     // search_filtered's own filters, which count towards kMaxFilters
    bool open_filter(const std::vector<std::vector<uint32_t>>& bits, uint32_t& handle, nsx::FilterStats* stats = nullptr);
    bool open_filter(const nsx::DocFilter& f, uint32_t& handle, nsx::FilterStats* stats = nullptr);
    bool close_filter(uint32_t handle);
    size_t open_filters() const;
    // search_batch_flat under a filter: the same query preparation, sub-batch pipeline and outputs, with the filter's rows.
    // Hits are the unfiltered ranking restricted to kept documents (score bits included), found counts kept documents only,
    // hits carry manifest positions.  Under NS_FLAG_AND a (query, segment) group one of whose lists lost all its postings
    // emits no refs.  A multi-device engine scores filtered batches on devices[0].  The search cache is not used.
    bool search_filtered_batch_flat(uint32_t handle, const QueryView* queries, size_t Q, int k, uint32_t flags, ns_hit* hits,
                                    uint32_t* nhits, uint64_t* found, uint8_t* usable);
    // JSON text: search's body plus "filter": {"date_from", "date_to", "documents", "keep_undated"} (the bounds without
    // their blanks; documents = how many are kept), dump(2) layout.  The last kFilterLru distinct filters stay open.
    // Any failure: {"error": ...} (search_filtered_text: false, body = the message).
    std::string search_filtered(const std::string& query, int k, const nsx::DocFilter& f);
    bool search_filtered_text(const std::string& query, int k, const nsx::DocFilter& f, std::string& body);

    // Facet counts (host/facet.hpp, csrc/ns_facet.hip).  facet_buckets: the spec's bucket table per segment
    // (manifest order, one uint16 per document) and the labels, bucket 0 = undated = ""; host only (works on a host-only
    // engine).  false: more than 1023 distinct values, or a Custom spec that does not fit the index.
    bool facet_buckets(const nsx::FacetSpec& spec, std::vector<std::vector<uint16_t>>& tables, std::vector<std::string>& labels);
    // facet_batch_flat: counts (resized to Q x B, B = labels.size()) [q * B + b] = the distinct documents of bucket b that
    // query q matches; found[q] = their sum.  The query preparation is search_batch_flat's (search_filtered_batch_flat's under
    // a filter handle; 0 = no filter): build_refs_parallel, semantic expansion when embeddings are loaded, the filter's rows.
    // So found[q] equals the search's found, query for query, and usable[q] its usable.  No score is computed.  Large
    // batches are cut like run_range's sub-batches.  Runs on the primary context.  The device copies of the bucket tables
    // are built by the first call that needs them (never by reload()), at most one per (kind, segment), serve the filtered
    // copies under a filter unchanged, and are freed by reload(), release_facets() and the destructor.  device_ms / count_ms
    // (may be null): the kernels' HIP-event time and the wall time inside ns_facet_count, summed over the sub-batches.
    bool facet_batch_flat(const nsx::FacetSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, uint32_t flags,
                          std::vector<uint32_t>& counts, uint64_t* found, uint8_t* usable, std::vector<std::string>& labels,
                          float* device_ms = nullptr, double* count_ms = nullptr);
    // JSON text: search's body (search_filtered's when a filter is given) plus "facets": {"<year|month|custom>": [{"count",
    // "value"}, ...]}: the nonzero buckets in bucket order (values ascending, undated first with ""), dump(2) layout.  The
    // counts are those of the query under the filter.  The search cache is not used.  Any failure: {"error": ...}
    // (search_faceted_text: false, body = the message).
    std::string search_faceted(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f = nullptr);
    bool search_faceted_text(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f, std::string& body);
    void release_facets();
    size_t facet_tables_on_device() const;   // bucket tables with a device copy right now

    // Search sorted by date (host/sorted.hpp, csrc/ns_sorted.hip).  sort_keys: the spec's key per document,
    // per segment in manifest order: date_key() of publish_time (YYYYMMDD, missing parts 0, undated 0), or the caller's
    // arrays; host only (works on a host-only engine).  false: a Custom spec that does not fit the index or holds the
    // reserved value 0xFFFFFFFF.
    bool sort_keys(const nsx::SortSpec& spec, std::vector<std::vector<uint32_t>>& keys);
    // search_sorted_batch_flat: per query the first K = clamp(k, 1, 100) matched documents in the order (key, manifest
    // position ascending, docId ascending) — newest first, or oldest first with spec.ascending; undated documents last in both
    // directions — with the BM25 score the search gives them.  hits / keys: Q x K (pad: {-inf, ~0, ~0}, key 0), nhits[q] =
    // min(K, found[q]).  flags: NS_FLAG_OR or NS_FLAG_AND.  The query preparation is facet_batch_flat's (the dictionary's
    // rows, or an open filter's under a handle, 0 = none; semantic expansion when embeddings are loaded), so found and usable
    // equal the search's, query for query; a query that is not usable has nhits = 0.  Hits carry manifest positions.  Runs on
    // the primary context.  The device key tables are built by the first call that needs them (never by reload()), one per
    // (kind, segment), serve the filtered copies unchanged, and are freed by reload(), release_sorted() and the destructor.
    bool search_sorted_batch_flat(const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k, uint32_t flags,
                                  ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint8_t* usable, float* device_ms = nullptr);
    // JSON text: search's body (search_filtered's when a filter is given) with "results" in date order, every entry decorated
    // as search's are, plus "sort": "newest" | "oldest" | "custom"; dump(2) layout.  The search cache is not used.  Any
    // failure: {"error": ...} (search_sorted_text: false, body = the message).
    std::string search_sorted(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f = nullptr);
    bool search_sorted_text(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f, std::string& body);
    void release_sorted();
    size_t sort_tables_on_device() const;   // key tables with a device copy right now

    // Boolean queries (host/boolean.hpp, csrc/ns_boolean.hip): `+word` must be held, `-word` must not, every
    // other word is optional and adds to the score (nsx::parse_boolean).  search_boolean_batch_flat: per query the K =
    // clamp(k, 1, 100) best matched documents in the search's order with the search's score bits.  hits: Q x K (pad:
    // {-inf, ~0, ~0}), nhits[q] = min(K, found[q]).  The query preparation goes through the term dictionary like the
    // search's (the dictionary's rows, or an open filter's under a handle, 0 = none) with one difference: a MUST term gets a
    // ref in EVERY segment on the device, with count == 0 where the segment (or the filter's copy) has no list of it or the
    // dictionary does not hold the term at all, so that no document of that segment matches.  usable[q] == 0 (and nhits = 0,
    // found = 0) when no MUST or SHOULD term is left or the index has no segment: exclusions alone select nothing.  No
    // semantic expansion, no search cache.  Hits carry manifest positions.  Runs on the primary context.
    bool search_boolean_batch_flat(uint32_t filter_handle, const QueryView* queries, size_t Q, int k, ns_hit* hits, uint32_t* nhits,
                                   uint64_t* found, uint8_t* usable, float* device_ms = nullptr);
    // JSON text: search's body (search_filtered's when a filter is given) over the boolean result, plus "boolean": {"must":
    // [...], "must_not": [...], "should": [...]} (the parsed terms, in query order); dump(2) layout.  Any failure:
    // {"error": ...} (search_boolean_text: false, body = the message).
    std::string search_boolean(const std::string& query, int k, const nsx::DocFilter* f = nullptr);
    bool search_boolean_text(const std::string& query, int k, const nsx::DocFilter* f, std::string& body);

    // Facet counts and date order for boolean queries (csrc/ns_boolean_sets.hip): facet_batch_flat and
    // search_sorted_after_batch_flat over search_boolean_batch_flat's matched set.  The query preparation is
    // search_boolean_batch_flat's, so found and usable equal its, query for query.
    // facet_boolean_batch_flat: counts (resized to Q x B, B = labels.size()) over ensure_facets' bucket tables.
    // search_boolean_sorted_batch_flat: the first K = clamp(k, 1, 100) matched documents in the order of spec (ensure_sorted's
    // key tables) strictly after each query's cursor (after == nullptr: page 1), with the boolean score bits; keys: Q x K;
    // rest may be nullptr.  Hits carry manifest positions.  Both need a device, run on the primary context, and use neither
    // semantic expansion nor the search cache.
    bool facet_boolean_batch_flat(const nsx::FacetSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, std::vector<uint32_t>& counts,
                                  uint64_t* found, uint8_t* usable, std::vector<std::string>& labels, float* device_ms = nullptr);
    bool search_boolean_sorted_batch_flat(const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k,
                                          const nsx::PageCursor* after, ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                          uint8_t* usable, float* device_ms = nullptr);
    // JSON text: search_boolean's body plus "facets" (search_faceted's member), and search_boolean's body with "results" in date
    // order plus "sort" (search_sorted's); dump(2) layout.  Any failure: {"error": ...} (the _text forms: false, body = the
    // message).
    std::string search_boolean_faceted(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f = nullptr);
    bool search_boolean_faceted_text(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f, std::string& body);
    std::string search_boolean_sorted(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f = nullptr);
    bool search_boolean_sorted_text(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f, std::string& body);

    // Any-of groups in boolean queries (host/grouped.hpp): the three boolean batch calls over nsx::parse_grouped's
    // dialect, `+(covid coronavirus sars) +vaccine -mouse`.  Each has its sibling's parameters and its sibling's answers for a
    // text without '('.  The query preparation is the boolean calls' (refs_range) with a clause id per MUST ref: every MUST token
    // gets a ref in every listed segment, with count == 0 where the token is absent or unknown, so an unknown synonym is dropped
    // and a clause of only unknown words kills the query.  A query with more than 65 535 clauses is refused with a message.
    bool search_grouped_after_batch_flat(uint32_t filter_handle, const QueryView* queries, size_t Q, int k, const nsx::PageCursor* after, ns_hit* hits,
                                         uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms = nullptr);
    bool facet_grouped_batch_flat(const nsx::FacetSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, std::vector<uint32_t>& counts,
                                  uint64_t* found, uint8_t* usable, std::vector<std::string>& labels, float* device_ms = nullptr);
    bool search_grouped_sorted_batch_flat(const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k,
                                          const nsx::PageCursor* after, ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                          uint8_t* usable, float* device_ms = nullptr);

    // JSON text: the boolean siblings' bodies (search_boolean, search_boolean_faceted, search_boolean_sorted) over this dialect,
    // with "grouped": {"must": [[...], ...], "must_not": [...], "should": [...]} in place of "boolean" (in its sorted place, behind
    // "found"): "must" lists the clauses, each the list of its terms.  search_page's modes Grouped and GroupedSorted page them with the cursor kinds of
    // Boolean and BooleanSorted.  Any failure: {"error": ...} (the _text forms: false, body = the message).
    std::string search_grouped(const std::string& query, int k, const nsx::DocFilter* f = nullptr);
    bool search_grouped_text(const std::string& query, int k, const nsx::DocFilter* f, std::string& body);
    std::string search_grouped_faceted(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f = nullptr);
    bool search_grouped_faceted_text(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f, std::string& body);
    std::string search_grouped_sorted(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f = nullptr);
    bool search_grouped_sorted_text(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f, std::string& body);

    // At-least-m-of-n clauses (host/quorum.hpp): the three grouped batch calls over nsx::parse_quorum's dialect,
    // `+(fever cough dyspnea fatigue)~2 -mouse` and `fever cough dyspnea ~2`, with a need per ref.  Each has its sibling's
    // parameters (filters and cursors included) and its sibling's answers for a text with neither form.  An unknown member is
    // dropped and the need stays, so a need above the known members matches nothing.  A need above nsx::kQuorumMaxNeed is refused
    // with a message, like the clause limit.
    bool search_quorum_after_batch_flat(uint32_t filter_handle, const QueryView* queries, size_t Q, int k, const nsx::PageCursor* after, ns_hit* hits,
                                        uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms = nullptr);
    bool facet_quorum_batch_flat(const nsx::FacetSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, std::vector<uint32_t>& counts,
                                 uint64_t* found, uint8_t* usable, std::vector<std::string>& labels, float* device_ms = nullptr);
    bool search_quorum_sorted_batch_flat(const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k,
                                         const nsx::PageCursor* after, ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                         uint8_t* usable, float* device_ms = nullptr);

    // JSON text: the grouped siblings' bodies over this dialect, with "quorum": {"min_should": m, "must": [{"need": n, "terms":
    // [...]}, ...], "must_not": [...], "should": [...]} in place of "grouped" (in its sorted place, behind "query").  The terms a `~m`
    // piece promoted are reported under "should".  search_page's modes Quorum and QuorumSorted page them with the cursor kinds of
    // Grouped and GroupedSorted.  Any failure: {"error": ...} (the _text forms: false, body = the message).
    std::string search_quorum(const std::string& query, int k, const nsx::DocFilter* f = nullptr);
    bool search_quorum_text(const std::string& query, int k, const nsx::DocFilter* f, std::string& body);
    std::string search_quorum_faceted(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f = nullptr);
    bool search_quorum_faceted_text(const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f, std::string& body);
    std::string search_quorum_sorted(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f = nullptr);
    bool search_quorum_sorted_text(const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f, std::string& body);

    // Boosts (host/boost.hpp, csrc/ns_boolean.hip k_bq_select<true, ., ., true>): the quorum ranked call over
    // nsx::parse_boosted's dialect, `+(covid sars)^0.5 vaccine^2.5`, whose `^w` becomes the qweight of the piece's terms, with one
    // fp32 factor per document multiplied into the finished score: relevance that prefers recent documents, or documents of a
    // high static rank.  boost_table: the spec's factors per segment in manifest order; host only (works on a host-only engine);
    // false, with a message, for a spec boost_check refuses or custom factors that do not fit the index, are negative (-0.0f
    // included) or not finite.  search_boosted_after_batch_flat is search_quorum_after_batch_flat parameter for parameter
    // (filter handle and cursors included; a cursor's rank is the product's bits) behind `spec`; spec == nullptr: term weights
    // only, through the sibling's kernels.  A weight of 0 gives the quorum call's answers bit for bit for a text without `^w`.
    // The device copies of the tables are built by the first call that needs them (never by reload()), one set at a time (another
    // spec takes its place), serve the filtered copies unchanged, and are freed by reload(), release_boosts() and the destructor.
    bool boost_table(const nsx::BoostSpec& spec, std::vector<std::vector<float>>& tables);
    bool search_boosted_after_batch_flat(const nsx::BoostSpec* spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k,
                                         const nsx::PageCursor* after, ns_hit* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable,
                                         float* device_ms = nullptr);
    // JSON text: search_quorum's body with "boosted" in place of "quorum" (the same members; a "must" clause carries "weight", a
    // "should" entry is {"term", "weight"}) and, with a spec, "boost": {"kind", "offset_days", "origin", "scale_days", "undated",
    // "weight"}; both stand in front of "filter".  search_page's mode Boosted pages it with cursors of kind 's'.  Any failure:
    // {"error": ...} (search_boosted_text: false, body = the message).
    std::string search_boosted(const std::string& query, int k, const nsx::BoostSpec* spec, const nsx::DocFilter* f = nullptr);
    bool search_boosted_text(const std::string& query, int k, const nsx::BoostSpec* spec, const nsx::DocFilter* f, std::string& body);
    void release_boosts();
    size_t boost_tables_on_device() const;   // factor tables with a device copy right now

    // Collapsed hits (host/collapse.hpp, csrc/ns_boolean.hip k_bq_select<false, ., ., ., true>, csrc/ns_collapse.hip):
    // the boosted ranked call with one hit per group of documents.  A group is the documents that share a collapse key: the
    // normalised title, the author field, or the caller's keys; a document without one stands alone.  Groups rank by their best
    // member, the hit IS that member (score, segment, docId as search_boosted reports it), and others[] says how many more
    // matched documents carry its key.  collapse_table: the spec's keys per segment in manifest order; host only (works on a
    // host-only engine); false, with a message, for custom keys that do not fit the index or hold 0xFFFFFFFF.
    // search_collapsed_batch_flat reads nsx::parse_boosted's dialect; boost_spec may be nullptr; hits name manifest positions;
    // groups and others are Q x K like hits (others may be nullptr: the count pass is skipped).  There is no cursor and no page
    // mode (§5ac, left out), and a `*` prefix term is refused with a message.  The device copies of the keys are built by the
    // first call that needs them (never by reload()), one set at a time (another spec takes its place), serve the filtered copies
    // unchanged, and are freed by reload(), release_collapse() and the destructor.
    bool collapse_table(const nsx::CollapseSpec& spec, std::vector<std::vector<uint32_t>>& tables);
    bool search_collapsed_batch_flat(const nsx::CollapseSpec& collapse_spec, const nsx::BoostSpec* boost_spec, uint32_t filter_handle, const QueryView* queries,
                                     size_t Q, int k, ns_hit* hits, uint32_t* groups, uint32_t* others, uint32_t* nhits, uint64_t* found, uint8_t* usable,
                                     float* device_ms = nullptr);
    // JSON text: search_boosted's body with "collapsed" in place of "boosted", "collapse": {"field": "title" | "author" | "custom"}
    // in front of it, and "others": n in every result.  Any failure: {"error": ...} (search_collapsed_text: false, body = the message).
    std::string search_collapsed(const std::string& query, int k, const nsx::CollapseSpec& collapse_spec, const nsx::BoostSpec* boost_spec = nullptr,
                                 const nsx::DocFilter* f = nullptr);
    bool search_collapsed_text(const std::string& query, int k, const nsx::CollapseSpec& collapse_spec, const nsx::BoostSpec* boost_spec, const nsx::DocFilter* f,
                               std::string& body);
    void release_collapse();
    size_t collapse_tables_on_device() const;   // key tables with a device copy right now

    // Prefix terms (host/prefix.hpp, csrc/ns_union.hip behind ns_segment_union): `vaccin*` in the Boosted dialect.
    // expand_prefix: the terms of suggest_table that begin with `prefix` (lower-case alnum bytes; a term equal to it included),
    // in byte order; more than max_expansions (1 .. 65535): those with the largest score, then the smallest bytes, are kept
    // (suggest's order) and `truncated` is set; a kept term the dictionary does not hold is skipped, and a term the table holds
    // twice comes once.  Host only: works on a host-only engine.  False, with a message, for a max_expansions out of range.
    bool expand_prefix(const std::string& prefix, uint32_t max_expansions, std::vector<std::string>& terms, bool& truncated);
    // search_boosted_after_batch_flat over nsx::parse_prefixed's dialect.  Per listed segment ONE ns_segment_union for the whole
    // batch on the primary context: each distinct ordinary list the batch names is a single group, each distinct prefix one group
    // of its expansions' lists there (none: an absent term; one: that term's own row, idf included; more: the union, its idf
    // bm25_idf(N, its count)).  The derived segments take ids above the filters' range, serve the call through a call-local row
    // table and are released before the call returns, on failure too; hits and cursors name manifest positions as everywhere.
    // A batch without any prefix is forwarded to search_boosted_after_batch_flat untouched.  A non-zero filter handle is refused:
    // a filtered union needs the unfiltered union's df for its idf.  prefixes (may be nullptr): per query its distinct prefixes
    // in query order.  The search cache is not used.
    bool search_prefixed_after_batch_flat(const nsx::BoostSpec* spec, const nsx::PrefixSpec& prefix_spec, uint32_t filter_handle, const QueryView* queries, size_t Q,
                                          int k, const nsx::PageCursor* after, ns_hit* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable,
                                          float* device_ms = nullptr, std::vector<std::vector<nsx::PrefixInfo>>* prefixes = nullptr);
    // JSON text: search_boosted's body with "prefixed" in place of "boosted" (a prefix term prints with its '*'), and
    // "prefixes": [{"expansions", "prefix", "truncated"}], the query's distinct prefixes in query order; keys stay sorted: both
    // stand in front of "query".  A DocFilter is refused with a message.  search_page's mode Prefixed pages it with cursors of
    // kind 's'.  Any failure: {"error": ...} (search_prefixed_text: false, body = the message).
    std::string search_prefixed(const std::string& query, int k, const nsx::BoostSpec* spec, const nsx::PrefixSpec& prefix_spec = nsx::PrefixSpec{},
                                const nsx::DocFilter* f = nullptr);
    bool search_prefixed_text(const std::string& query, int k, const nsx::BoostSpec* spec, const nsx::PrefixSpec& prefix_spec, const nsx::DocFilter* f, std::string& body);

    // The calls above by dialect (nsx::Dialect, host/boolean.hpp): each named method forwards to one of these, which name
    // themselves in messages as the dialect's named method does.  DESIGN.md §5x lists what a fourth dialect adds.
    // boost (Dialect::Boosted only; may be nullptr): the factors of search_boosted_after_batch_flat and search_boosted_text.
    bool search_dialect_after_batch_flat(nsx::Dialect dialect, uint32_t filter_handle, const QueryView* queries, size_t Q, int k, const nsx::PageCursor* after,
                                         ns_hit* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms = nullptr,
                                         const nsx::BoostSpec* boost = nullptr);
    bool facet_dialect_batch_flat(nsx::Dialect dialect, const nsx::FacetSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q,
                                  std::vector<uint32_t>& counts, uint64_t* found, uint8_t* usable, std::vector<std::string>& labels, float* device_ms = nullptr);
    bool search_dialect_sorted_batch_flat(nsx::Dialect dialect, const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k,
                                          const nsx::PageCursor* after, ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                          uint8_t* usable, float* device_ms = nullptr);
    bool search_dialect_text(nsx::Dialect dialect, const std::string& query, int k, const nsx::DocFilter* f, std::string& body, const nsx::BoostSpec* boost = nullptr);
    bool search_dialect_faceted_text(nsx::Dialect dialect, const std::string& query, int k, const nsx::FacetSpec& spec, const nsx::DocFilter* f, std::string& body);
    bool search_dialect_sorted_text(nsx::Dialect dialect, const std::string& query, int k, const nsx::SortSpec& spec, const nsx::DocFilter* f, std::string& body);

    // Pages past the first K (host/page.hpp).  A cursor is a position (rank, manifest position, docId) in a call's
    // total order; with one, a call answers with the first K matched documents STRICTLY AFTER it: found[q] stays the size of
    // the matched set, rest[q] (may be nullptr) is the number of matched documents after the cursor, nhits[q] = min(K, rest[q]).
    // after: one cursor per query, or nullptr (then, and with every cursor unset, the calls are their siblings without one).
    // The engine translates the position to the call's segment id (the filter copy's under a filter handle); a position
    // outside the index, or one the call lists no segment for, is refused with a message.  A cursor is good until a reload()
    // changes the index.
    // search_after_batch_flat is search_batch_flat's query preparation (search_filtered_batch_flat's under a handle) over the
    // boolean kernels: page 1 equals search_batch_flat bit for bit, page n continues it.
    bool search_after_batch_flat(uint32_t filter_handle, const QueryView* queries, size_t Q, int k, uint32_t flags, const nsx::PageCursor* after,
                                 ns_hit* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms = nullptr);
    bool search_boolean_after_batch_flat(uint32_t filter_handle, const QueryView* queries, size_t Q, int k, const nsx::PageCursor* after, ns_hit* hits,
                                         uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms = nullptr);
    bool search_sorted_after_batch_flat(const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k, uint32_t flags,
                                        const nsx::PageCursor* after, ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                        uint8_t* usable, float* device_ms = nullptr);
    // JSON text: the mode's body (search's, search_filtered's with spec.use_filter, search_boolean's, search_sorted's,
    // search_boolean_sorted's) over one
    // page, plus "page": {"cursor", "next", "offset", "remaining"}; "next" only when documents remain after this page; offset
    // = found - rest, remaining = rest - nhits; dump(2) layout.  cursor_text: "" for the first page, else a page's "next"; its
    // kind letter must fit the mode.  The search cache is not used.  Any failure: {"error": ...} (search_page_text: false,
    // body = the message).
    std::string search_page(const std::string& query, int k, const std::string& cursor_text, const nsx::PageSpec& spec);
    bool search_page_text(const std::string& query, int k, const std::string& cursor_text, const nsx::PageSpec& spec, std::string& body);

    std::string to_json(const SearchResult& r) const;
    std::string to_json_impl(const SearchResult& r) const;
    // A batch of searches straight to the /api/search JSON bodies (result assembly on several host threads).
    bool search_batch_json(const std::vector<std::string>& queries, int k, std::vector<std::string>& out);
    ns_ctx* ctx() const { return ctx_; }
    std::string last_error() const { std::lock_guard<std::recursive_mutex> lock(mtx_); return err_; }
    void set_cache(bool on) { std::lock_guard<std::recursive_mutex> lock(mtx_); cache_on_ = on; if (!on) { cache_.clear(); lru_.clear(); } }
    size_t cache_size() const { std::lock_guard<std::recursive_mutex> lock(mtx_); return cache_.size(); }
    // The raw posting payload of a segment in host memory, read from the inverted files on first request (tests and
    // tools; the engine itself never holds it: reload() streams the files to the device from their mappings).
    const std::vector<uint8_t>* raw_postings(uint32_t seg);

private:
    // The reference's Engine::mtx (include/api_engine.hpp:33, taken at src/api_engine.cpp:54,:168,:372): one lock around
    // every entry that touches the cache, the error string, the device context or the loaded index.
    mutable std::recursive_mutex mtx_;   // recursive: public entries call each other (search -> build_refs -> expand_queries)
    bool search_batch_locked(const std::vector<std::string>& queries, int k, uint32_t flags, std::vector<SearchResult>& out);
    bool search_hits_locked(const std::string& query, int k, uint32_t flags, SearchResult& out);
    std::vector<std::unique_ptr<std::vector<uint8_t>>> raw_postings_;
    void release_device_segments();
    struct CacheEntry { std::string body; std::list<std::string>::iterator lru; };
    std::unordered_map<std::string, CacheEntry> cache_;
    std::list<std::string> lru_;   // most recently used at the front
    bool cache_on_ = true;
    // query preparation of queries [q0, q1) through the term dictionary: refs appended to `refs`, qd[q - q0] filled with
    // term_begin relative to `refs`' start, usable[q - q0] set
    // rs: the rows the refs come from (the dictionary's own, or an open filter's); and_mode matters under a filter only
    void build_refs_views(const QueryView* queries, size_t q0, size_t q1, ns_query_desc* qd, std::vector<ns_term_ref>& refs,
                          uint8_t* usable, std::vector<char>& scratch, std::vector<uint32_t>& gids, const nsx::RowSource& rs = nsx::RowSource{},
                          bool and_mode = false) const;
    // host threads of query preparation (kept from batch to batch) and their scratch
    struct PrepScratch { std::vector<ns_term_ref> refs; std::vector<char> text; std::vector<uint32_t> gids; };
    mutable std::unique_ptr<ForkJoin> pool_;
    mutable std::vector<PrepScratch> scratch_;
    std::vector<ns_query_desc> flat_qd_;     // search_batch_flat's descriptor buffers, kept from call to call
    std::vector<ns_term_ref> flat_refs_;
    unsigned prep_width(size_t Q) const;
    void build_refs_parallel(const QueryView* queries, size_t q0, size_t q1, std::vector<ns_query_desc>& qd,
                             std::vector<ns_term_ref>& refs, uint8_t* usable, const nsx::RowSource& rs = nsx::RowSource{},
                             bool and_mode = false) const;
    mutable bool refs_failed_ = false;   // build_refs could not run the device part of the expansion (err_ says why)
    int device_;
    ns_ctx* ctx_ = nullptr;
    ns_ac* ac_ = nullptr;    // suggest_table on ctx_ (ns_ac_upload)
    bool ac_fuzzy_ = false;  // ns_ac_build_fuzzy has run on ac_
    bool ensure_fuzzy();
    bool fuzzy_batch(const char* fn, const QueryView* terms, size_t Q, int limit, int max_edits, int prefix_len, uint32_t* term_idx, uint8_t* dist,
                     uint32_t* count, uint32_t* base_len, float* device_ms);
    // more-like-this: per segment the device copy of its forward index and, on the host, the term bytes of terms.bin
    struct SimilarSeg { ns_docterms* dev = nullptr; std::vector<uint8_t> term_bytes; std::vector<uint64_t> term_offsets; };
    std::vector<SimilarSeg> similar_;
    bool ensure_similar(uint32_t seg);
    // terms_batch's rows before the cut: per row every merged candidate, in the merge rule's order
    bool related_rows(const std::pair<uint32_t, uint32_t>* seg_doc, const uint64_t* row_off, size_t Q, const nsx::RelatedOptions& opt,
                      std::vector<std::vector<nsx::RelatedCand>>& rows, std::vector<uint32_t>& ndocs, float* device_ms);
    struct OpenFilter;
    OpenFilter* lru_filter(const nsx::DocFilter& f, nsx::DateRange& r);   // search_filtered's cache of open filters; nullptr: err_ is set
    void append_results_json(std::string& o, const std::vector<SearchHit>& hits) const;
    std::vector<ns_seg*> dev_segs_;
    // further devices holding a replica of the index (multi-device engine): context + segments each
    struct Replica { int device = 0; ns_ctx* ctx = nullptr; std::vector<ns_seg*> segs; };
    std::vector<Replica> replicas_;
    // one contiguous range of a batch on one context: sub-batches pipelined (prepare(i+1) || kernels(i) || results(i-1))
    bool run_range(ns_ctx* ctx, const QueryView* queries, size_t q0, size_t q1, int K, uint32_t flags, ns_hit* hits, uint32_t* nhits,
                   uint64_t* found, uint8_t* usable, bool pooled_prep, std::string& err, const nsx::RowSource& rs = nsx::RowSource{});
    // open filters: the device copies per manifest position (nullptr: none) and the rows parallel to dict's
    struct OpenFilter {
        bool open = false;
        uint32_t handle = 0;
        std::vector<ns_seg*> segs;
        std::vector<nsx::TermSeg> rows;
        uint64_t docs_kept = 0;
    };
    OpenFilter filters_[kMaxFilters];
    uint32_t filter_gen_ = 0;
    OpenFilter* filter_of(uint32_t handle);
    bool translate_cursors(const char* fn, const nsx::PageCursor* after, size_t a, size_t b, uint32_t id_base, const std::vector<uint8_t>& listed,
                           bool filtered, std::vector<ns_cursor>& out);
    // the rows of one search_prefixed_after_batch_flat call: the batch's distinct ordinary terms first, then its distinct prefixes
    struct PrefixRows {
        std::unordered_map<uint32_t, uint32_t> of_term;       // dictionary row -> call-local row
        std::unordered_map<std::string, uint32_t> of_prefix;  // prefix -> call-local row
        std::vector<uint32_t> terms;                          // call-local row -> dictionary row, the ordinary terms
        std::vector<std::vector<uint32_t>> expansions;        // per prefix: the dictionary rows of its expansions, distinct
        std::vector<nsx::PrefixInfo> info;                    // per prefix
        std::vector<nsx::TermSeg> rows;                       // [call-local row][manifest position]
        std::vector<ns_seg*> segs;                            // the derived segments per manifest position
    };
    // What the ranked, facet and date-order calls share, plain and boolean alike: the filter's row source under a handle, the
    // segments the refs can name and the call's cursors.  The boolean dialects also keep the refs of one query range here (from
    // qd on); the plain calls keep theirs in PlainPrep.
    struct CallPrep {
        OpenFilter* f = nullptr;
        nsx::RowSource rs;
        std::vector<uint32_t> ids, listed;      // the ids the refs use; the manifest positions behind them
        std::vector<ns_seg*> segs;
        std::vector<uint8_t> is_listed;         // per manifest position
        std::vector<ns_cursor> cur;             // of the current sub-batch; empty: none is set
        std::vector<ns_query_desc> qd;
        std::vector<ns_term_ref> refs;
        std::vector<uint8_t> roles;
        std::vector<uint16_t> clauses;          // Grouped, Quorum: parallel to refs
        std::vector<uint8_t> needs;             // Quorum, Boosted: parallel to refs
        std::vector<ns_docboost*> boosts;       // Boosted under a spec: parallel to segs; empty: none
        std::vector<char> scratch;
        struct Term { int64_t row; uint8_t role; uint32_t clause, need; float weight; };   // row: the dictionary's, or -1
        std::vector<Term> terms;                // of one query
        const PrefixRows* px = nullptr;          // Prefixed: the call-local rows that rs.rows holds (a term's row is one of THEM)
    };
    bool expand_prefix_rows(const char* p, size_t n, uint32_t max_expansions, std::vector<uint32_t>& rows, std::vector<uint32_t>* table_idx, bool& truncated) const;
    void release_prefix_segments(PrefixRows& px);
    bool prefix_page(const std::string& query, int k, const nsx::PageCursor* cur, const nsx::BoostSpec* boost, const nsx::PrefixSpec& ps, ns_hit* hits, uint32_t* nh,
                     uint64_t* fd, uint64_t* rs, uint8_t* us, std::string& member);
    // boolean_prepare's two halves.  filter_rows: the stale-handle check and the filter's row source.  list_segments: the
    // positions with a device copy (the index's own, or the filter's) that `keep` does not skip, in manifest order.
    bool filter_rows(const char* fn, uint32_t filter_handle, CallPrep& bp);
    template <class Keep> void list_segments(CallPrep& bp, Keep keep);
    bool boolean_prepare(const char* fn, uint32_t filter_handle, CallPrep& bp);
    // descriptors, refs, roles (and the dialect's clauses and needs) of the queries [a, b) (qd indexed from a) and usable[a .. b)
    bool refs_range(const char* fn, nsx::Dialect dialect, const QueryView* queries, size_t a, size_t b, uint8_t* usable, CallPrep& bp);
    // the plain search's query preparation for the sub-batches of one call
    struct PlainPrep {
        bool whole = false;   // semantic expansion: prepared for the whole batch up front, term_begin indexes the one refs array
        std::vector<ns_query_desc> qd;
        std::vector<ns_term_ref> refs;
        const ns_query_desc* qd_at = nullptr;   // the current sub-batch's
        const ns_term_ref* refs_at = nullptr;
        size_t n_refs = 0;
    };
    bool plain_prepare(const QueryView* queries, size_t Q, uint8_t* usable, const nsx::RowSource& rs, bool and_mode, PlainPrep& pp);
    void plain_range(const QueryView* queries, size_t a, size_t b, uint8_t* usable, const nsx::RowSource& rs, bool and_mode, PlainPrep& pp);
    // the outputs of a ranked call: hits (and keys, or nullptr) are Q x K
    struct RankedOut { size_t K; ns_hit* hits; uint32_t* keys; uint32_t* nhits; uint64_t* found; uint64_t* rest; float* device_ms; };
    template <class Prep, class Call>
    bool ranked_batch(const char* fn, CallPrep& bp, const nsx::PageCursor* after, size_t Q, const RankedOut& out, Prep prep, Call call);
    bool sorted_batch_impl(const char* fn, const nsx::SortSpec& spec, uint32_t filter_handle, const QueryView* queries, size_t Q, int k, uint32_t flags,
                           const nsx::PageCursor* after, ns_hit* hits, uint32_t* keys, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable,
                           float* device_ms);
    // the device call of a dialect, one per shape: the only places that pick among the per-dialect C entry points
    bool ranked_call(nsx::Dialect dialect, bool paged, const CallPrep& bp, size_t a, size_t b, const RankedOut& out, const ns_cursor* cur, float* ms);
    bool facet_call(nsx::Dialect dialect, const CallPrep& bp, size_t a, size_t b, ns_facet* const* tabs, uint32_t* counts, uint64_t* found, float* ms);
    bool sorted_call(nsx::Dialect dialect, const CallPrep& bp, size_t a, size_t b, uint32_t direction, ns_dockeys* const* tabs, const RankedOut& out,
                     const ns_cursor* cur, float* ms);
    bool boolean_batch_impl(const char* fn, nsx::Dialect dialect, uint32_t filter_handle, const QueryView* queries, size_t Q, int k,
                            const nsx::PageCursor* after, ns_hit* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* usable, float* device_ms,
                            const nsx::BoostSpec* boost = nullptr);
    void close_filter_slot(OpenFilter& f);
    void close_all_filters();
    struct FilterLruEnt { std::string key; uint32_t handle; };
    std::list<FilterLruEnt> filter_lru_;   // most recently used at the front
    // facets: per kind the host tables and labels and their device copies (nullptr: the segment has none)
    struct FacetSet {
        bool built = false;
        std::vector<std::vector<uint16_t>> tables;
        std::vector<std::string> labels;
        std::vector<ns_facet*> dev;
    };
    FacetSet facets_[3];
    bool ensure_facets(const nsx::FacetSpec& spec, FacetSet*& out);
    // sort keys: per kind the host keys and their device copies (nullptr: the segment has none)
    struct SortSet {
        bool built = false;
        std::vector<std::vector<uint32_t>> keys;
        std::vector<ns_dockeys*> dev;
    };
    SortSet sorts_[2];
    bool ensure_sorted(const nsx::SortSpec& spec, SortSet*& out);
    // boost factors: the last spec's host tables and their device copies (nullptr: the segment has none); key: the decay's parameters
    struct BoostSet {
        bool built = false;
        std::string key;
        std::vector<std::vector<float>> tables;
        std::vector<ns_docboost*> dev;
    };
    BoostSet boosts_;
    bool ensure_boosts(const nsx::BoostSpec& spec, BoostSet*& out);
    // collapse keys: the last spec's host keys and their device copies (nullptr: the segment has none)
    struct CollapseSet {
        bool built = false;
        int kind = 0;
        std::vector<std::vector<uint32_t>> keys;
        std::vector<ns_dockeys*> dev;
    };
    CollapseSet collapse_;
    bool ensure_collapse(const nsx::CollapseSpec& spec, CollapseSet*& out);
    mutable std::string err_;
};

}  // namespace nextsearch
