/*
 * nextsearch_host.h — C wrappers over the C++ host facade (nextsearch::Engine, the mirror of the
 * reference's cord19::Engine, include/api_engine.hpp:23-91) so that Python tests and bench.py can
 * drive it through ctypes.  The compute entry points all go through include/nextsearch_hip.h; this
 * header adds no scoring code and no CPU fallback.
 */
#ifndef NEXTSEARCH_HOST_H
#define NEXTSEARCH_HOST_H

#include <stdint.h>

#include "nextsearch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nsh_engine nsh_engine;

/* Deterministic synthetic index in the reference's on-disk format. */
int nsh_gen_index(const char* index_dir, uint32_t n_segments, uint32_t docs_per_segment, uint32_t vocab,
                  uint64_t seed, int legacy_layout, uint64_t* total_postings_out);

/* Engine::reload() on index_dir.  device >= 0: create an ns_ctx on that GPU and upload every
 * segment; device < 0: host-only (index + query preparation; search calls fail).  On failure
 * returns non-zero and *out still receives an engine whose nsh_engine_error() explains why
 * (free it with nsh_engine_close). */
int  nsh_engine_open(const char* index_dir, int device, nsh_engine** out);
/* The multi-device engine ("one host thread + ns_ctx per GPU"): the index is replicated on every device
 * of devices[0 .. n_devices) (the same device may be listed twice: two contexts on one GPU), and nsh_engine_search_batch
 * cuts a batch into contiguous shards of ceil(Q / n_devices) queries, one per device, each driven by its own host thread;
 * the results land in the caller's one set of arrays.  devices[0] is the primary context (nsh_engine_ctx, single searches).
 * Same failure convention as nsh_engine_open. */
int  nsh_engine_open_multi(const char* index_dir, const int* devices, uint32_t n_devices, nsh_engine** out);
uint32_t nsh_engine_num_devices(nsh_engine* e);
/* [begin, end) of shard r of n over n_queries queries, as nsh_engine_search_batch cuts them (arithmetic only) */
void nsh_shard_bounds(uint64_t n_queries, uint32_t r, uint32_t n, uint64_t* begin, uint64_t* end);
void nsh_engine_close(nsh_engine* e);
/* Engine::reload() again on the same directory.  0 on success.  On failure (non-zero) the engine keeps the index,
 * the device copy and the caches it had (the reference swaps its segments in only after every one loaded,
 * src/api_engine.cpp:76-90).  On success the device context is a NEW one: re-read nsh_engine_ctx(). */
int  nsh_engine_reload(nsh_engine* e);
/* The engine's last failure message.  The pointer stays valid for the CALLING thread until it asks again (a copy per thread). */
const char* nsh_engine_error(nsh_engine* e);
ns_ctx* nsh_engine_ctx(nsh_engine* e);

/* The reference's `lexicon <SEGMENT_DIR>` tool (src/lexicon.cpp) with the inversion on the device
 * (ns_invert_forward): reads <seg>/terms.bin + forward.bin, writes barrels.bin, lexicon_bNNN.bin and
 * inverted_bNNN.bin byte for byte as the reference does.  0 on success; nsh_invert_error() otherwise. */
int nsh_invert_segment(const char* seg_dir, int device, uint64_t* pairs, uint64_t* kept, float* device_ms,
                       double* call_s, double* total_s);
const char* nsh_invert_error(void);

/* Search-result cache around nsh_engine_search_json (src/api_engine.cpp:190-250,:380-385,:539): "query|K" keys,
 * 2600 entries, LRU eviction, hits carry "from_cache": true.  On by default, in memory only; the batch entry
 * points never use it. */
void nsh_engine_set_cache(nsh_engine* e, int on);
uint32_t nsh_engine_cache_size(nsh_engine* e);

/* Semantic query expansion (src/api_engine.cpp:115-153,:409-417; src/semantic_embedding.cpp): reload() loads
 * <index>/embeddings.vec|embeddings.txt|glove.txt|vectors.txt (or $EMBEDDINGS_PATH) for the lexicons' terms and
 * uploads the table; every search then scores the expanded, weighted terms (similarity search on the device,
 * ns_sem_topk).  nsh_engine_semantic_info: 1 if a table is loaded (+ rows, dim).  nsh_engine_expand: the weighted
 * terms of one query, "term<TAB>%08x weight bits" per line in scoring order; free with nsh_free. */
int nsh_engine_semantic_info(nsh_engine* e, uint32_t* rows, uint32_t* dim);
int nsh_engine_expand(nsh_engine* e, const char* query, char** text_out);
/* Row `row` of the loaded table: its term and its `dim` L2-normalised values (valid until close/reload); -1 if absent. */
int nsh_engine_semantic_row(nsh_engine* e, uint32_t row, const char** term, const float** vec);

/* Optional impact streams for every list of every loaded lexicon (include/nextsearch_hip.h:
 * ns_segment_build_impacts / ns_ctx_use_impacts).  Not part of reload(): 8 B of HBM per posting. */
int  nsh_engine_build_impacts(nsh_engine* e);
void nsh_engine_use_impacts(nsh_engine* e, int on);
/* reload() builds skip tables for the frequent lists of every segment (ns_segment_build_skips); on = 0: searches ignore them. */
void nsh_engine_use_skips(nsh_engine* e, int on);
/* Optional packed posting streams for every loaded segment (include/nextsearch_hip.h: ns_segment_build_packed /
 * ns_ctx_use_packed): 4-7 B read per posting instead of 12, same results.  Not part of reload(): 8 B of HBM per posting. */
int  nsh_engine_build_packed(nsh_engine* e);
void nsh_engine_use_packed(nsh_engine* e, int on);
/* Optional block maxima for every list of >= 512 postings of every loaded segment (include/nextsearch_hip.h:
 * ns_segment_build_blockmax) and the switch for `found`-exact pruning of single-term queries (ns_ctx_use_pruning; off by
 * default).  Same results either way. */
int  nsh_engine_build_blockmax(nsh_engine* e);
void nsh_engine_use_pruning(nsh_engine* e, int on);
/* on = 0: two-list groups take the driver-stream body instead of the merge body (ns_ctx_use_merge; default 1).  Same results. */
void nsh_engine_use_merge(nsh_engine* e, int on);
/* Shared term scores (include/nextsearch_hip.h: ns_ctx_share_scores) on every device context of the engine: 0 never, 1 (default)
 * batches that name each distinct list often enough compute its BM25 term scores once per run, 2 every batch that can.  Same results. */
void nsh_engine_share_scores(nsh_engine* e, int mode);

/* ---- inspection (tests and tools).  NOT reload-safe: these accessors read the loaded index without taking the engine
 * lock and hand out pointers into it, and nsh_engine_reload() replaces that index — do not call them, or use what they
 * returned, while another thread reloads.  (The search and query-preparation entries above do take the lock, as every
 * entry of the reference's engine takes Engine::mtx.)  Likewise an ns_batch obtained through nsh_engine_prepare belongs
 * to the device context it was prepared on: fetch and destroy it before reloading. */
uint32_t nsh_engine_num_segments(nsh_engine* e);
const char* nsh_engine_segment_name(nsh_engine* e, uint32_t seg);
int nsh_engine_segment_info(nsh_engine* e, uint32_t seg, uint32_t* n_docs, float* avgdl, uint64_t* n_postings,
                            uint32_t* n_terms, int* use_barrels);
/* Result decoration from <index>/metadata.csv (src/api_engine.cpp:516-531, src/api_metadata.cpp): the
 * decorated fields of one document, valid until close/reload; 1 if the document has a metadata row. */
int nsh_engine_doc_metadata(nsh_engine* e, uint32_t seg, uint32_t doc, const char** title, const char** url,
                            const char** publish_time, const char** author);
/* Result assembly alone (src/api_engine.cpp:400-404,:505-536): JSON text for given hits; free with nsh_free. */
int nsh_engine_hits_to_json(nsh_engine* e, const char* query, int k, int has_found, uint64_t found,
                            const ns_hit* hits, uint32_t nhits, char** json_out);
/* Host copies of what gets uploaded (valid until close/reload). */
const uint32_t* nsh_engine_segment_doc_len(nsh_engine* e, uint32_t seg);
const void* nsh_engine_segment_postings(nsh_engine* e, uint32_t seg, uint64_t* nbytes);
/* Lexicon probe (src/api_engine.cpp:454-461).  Returns 1 if found, 0 if absent. */
int nsh_engine_lookup(nsh_engine* e, uint32_t seg, const char* term, uint32_t* term_id, uint32_t* df, uint32_t* count,
                      uint64_t* byte_off, float* idf);

float nsh_bm25_idf(uint32_t n_docs, uint32_t df);
/* Tokenise + filter (include/textutil.hpp:13-37, src/api_engine.cpp:391-397): writes the kept terms
 * separated by single spaces into buf (NUL-terminated, truncated to cap); returns the term count. */
uint32_t nsh_base_terms(const char* query, char* buf, uint32_t cap);

/* Query preparation only: fills qd[n_queries], usable[n_queries] and up to refs_cap refs;
 * *n_refs receives the number needed.  Returns 0, or 1 if refs_cap was too small. */
int nsh_engine_build_refs(nsh_engine* e, const char* const* queries, uint32_t n_queries, ns_query_desc* qd,
                          ns_term_ref* refs, uint32_t refs_cap, uint32_t* n_refs, uint8_t* usable);

/* Engine::search(query, k) -> JSON text with the reference's keys; caller frees with nsh_free. */
int  nsh_engine_search_json(nsh_engine* e, const char* query, int k, char** json_out);
void nsh_free(void* p);
/* A batch of searches straight to the /api/search JSON bodies (result assembly on several host threads):
 * *text_out receives all bodies back to back (free with nsh_free); offsets[q] .. offsets[q+1] delimit body q
 * (offsets has n_queries + 1 entries). */
int  nsh_engine_search_batch_json(nsh_engine* e, const char* const* queries, uint32_t n_queries, int k,
                                  char** text_out, uint64_t* offsets);
/* Batch search through ns_search_batch.  hits: n_queries*K (K = clamp(k,1,100)). */
int nsh_engine_search_batch(nsh_engine* e, const char* const* queries, uint32_t n_queries, int k, uint32_t flags,
                            ns_hit* hits, uint32_t* nhits, uint64_t* found, uint8_t* has_found);
/* Staged: query prep on the host, descriptors to the device; drive the result with ns_batch_*. */
int nsh_engine_prepare(nsh_engine* e, const char* const* queries, uint32_t n_queries, int k, uint32_t flags,
                       ns_batch** out);

/* Indexing (host/forward_index.hpp; the reference's `forwardindex` tool from the text handed to tokenize onwards,
 * src/ForwardIndex.cpp:139-230): n_docs documents of four fields each — cord_uid, title, json_relpath, text, in this
 * order — as raw bytes with explicit lengths: field f of document d = bytes[field_offsets[4 d + f] .. field_offsets[4 d + f + 1])
 * (4 * n_docs + 1 offsets).  Tokenising, tf counting and the term dictionary run on the device (ns_forward_build). */
typedef struct nsh_index_stats {
    uint32_t struct_size;   /* IN: sizeof(nsh_index_stats) as the caller was compiled; no more than that is written */
    uint32_t n_docs_in, n_docs, n_terms;
    uint64_t text_bytes, tokens, kept_tokens, pairs, device_bytes;
    float    avgdl, device_ms;
    double   call_s, total_s;
} nsh_index_stats;
/* Writes docs.bin, stats.bin, forward.bin, terms.bin into seg_dir (created) on a context of its own on `device`.
 * -1 on failure, also when no document survives the length and stop-word rules (nothing is written then);
 * nsh_index_error() says why.  stats may be NULL. */
int nsh_index_documents(const char* seg_dir, int device, const char* bytes, const uint64_t* field_offsets, uint32_t n_docs,
                        nsh_index_stats* stats);
const char* nsh_index_error(void);
/* An engine on index_dir WITHOUT the initial reload (nsh_engine_open fails on a directory that holds no segment yet):
 * what nsh_engine_add_documents needs on a fresh index directory.  Searches fail until a reload succeeded. */
int nsh_engine_open_noload(const char* index_dir, int device, nsh_engine** out);
/* Engine::add_documents: the batch becomes the next free segments/seg_%06u (forward index and inversion on the device),
 * manifest.bin gains its name (src/AddDocument.cpp:20-60,:160-170) and the engine reloads.  -1 on failure: the manifest
 * keeps its bytes, the new segment directory is gone, nsh_engine_error() says why. */
int nsh_engine_add_documents(nsh_engine* e, const char* bytes, const uint64_t* field_offsets, uint32_t n_docs,
                             nsh_index_stats* stats);

/* Compaction (host/compact.hpp): several segments become one.  The sources' docs.bin, stats.bin,
 * forward.bin and terms.bin are read and cross-checked on the host; the term lists are merged, the pairs remapped and
 * re-sorted (ns_forward_merge) and inverted (ns_forward_invert) on the device; the result is a complete segment: the four
 * forward files, barrels.bin and the 64 + 64 barrel files.  For sources whose term ids follow ns_forward_build's rule it is
 * byte for byte the segment ONE nsh_index_documents + nsh_invert_segment over all their documents writes. */
typedef struct nsh_compact_stats {
    uint32_t struct_size;   /* IN: sizeof(nsh_compact_stats) as the caller was compiled; no more than that is written */
    uint32_t sources, n_docs, n_terms;
    uint64_t terms_in, pairs, device_bytes;
    float    merge_ms, invert_ms;   /* HIP events around the device parts */
    double   call_s, total_s;
} nsh_compact_stats;
/* Merges the segment directories source_dirs[0 .. n_sources) into out_dir (created) on a context of its own on `device`.
 * The sources are read and checked before the device is touched.  -1 on failure: nothing is written,
 * nsh_compact_error() says why and names the file or the source.  stats may be NULL. */
int nsh_merge_segments(const char* const* source_dirs, uint32_t n_sources, const char* out_dir, int device, nsh_compact_stats* stats);
const char* nsh_compact_error(void);
/* Engine::compact: the segments at manifest positions [first, first + count) (clamped to the manifest) become the next
 * free segments/seg_%06u, whose name takes the range's place in manifest.bin; the engine reloads; with remove_sources the
 * source directories are removed afterwards.  Fewer than two segments in the range: 0, nothing touched.  -1 on failure
 * (also on a host-only engine): the manifest keeps its bytes, the new directory is gone, no source is touched, the engine
 * answers as before, nsh_engine_error() says why.  0 with a non-empty nsh_engine_error(): a source could not be removed. */
int nsh_engine_compact(nsh_engine* e, uint64_t first, uint64_t count, int remove_sources, nsh_compact_stats* stats);

/* Deleting documents (host/purge.hpp).  A uid list travels as uid i = bytes[offsets[i] .. offsets[i + 1])
 * (offsets: n_uids + 1 entries). */
typedef struct nsh_delete_stats {
    uint32_t struct_size;   /* IN: sizeof(nsh_delete_stats) as the caller was compiled; no more than that is written */
    uint32_t segments_rewritten, segments_dropped, docs_deleted, uids_not_found, terms_dropped;
    uint64_t pairs_in, pairs_out, device_bytes;   /* pairs of the rewritten segments before / after */
    float    merge_ms, invert_ms;                 /* HIP events around the device parts, summed over the rewritten segments */
    double   call_s, total_s;
} nsh_delete_stats;
/* Engine::find_documents: every (manifest position, docId) whose docs.bin uid is listed, ascending, as u32 pairs into
 * seg_doc_out (capacity pairs; may be NULL).  Returns the number of matches (which may exceed capacity: call again), -1
 * on failure.  Host only: works on a host-only engine. */
int64_t nsh_engine_find_documents(nsh_engine* e, const char* bytes, const uint64_t* offsets, uint32_t n_uids,
                                  uint32_t* seg_doc_out, uint64_t capacity);
/* Engine::delete_documents: every document that carries a listed uid goes, in every segment.  Each affected segment is
 * rewritten on the device into the next free segments/seg_%06u, which takes its place in manifest.bin; a segment with no
 * survivor leaves the manifest; untouched segments are not rewritten; the engine reloads; the old directories are removed
 * afterwards.  Uids that match nothing are counted in stats->uids_not_found; nothing matching at all: 0, nothing touched.
 * Surviving documents of a rewritten segment get new docIds (their positions): the uid is the stable handle.
 * -1 on failure (also on a host-only engine, and when every document of the index would go): the manifest keeps its bytes,
 * the new directories are gone, the engine answers as before, nsh_engine_error() says why.  0 with a non-empty
 * nsh_engine_error(): an old directory could not be removed. */
int nsh_engine_delete_documents(nsh_engine* e, const char* bytes, const uint64_t* offsets, uint32_t n_uids, nsh_delete_stats* stats);
/* Engine::delete_by_id: the same for n_pairs u32 pairs (manifest position, docId).  A pair out of range: -1, nothing
 * touched; a pair listed twice counts once. */
int nsh_engine_delete_by_id(nsh_engine* e, const uint32_t* seg_doc, uint64_t n_pairs, nsh_delete_stats* stats);

/* Autocomplete: Engine::suggest(input, limit) (include/api_engine.hpp:67, src/api_engine.cpp:164-187).  The input is
 * input_len raw bytes (NUL and other control bytes included); *json_out receives {"limit", "query", "suggestions"} in
 * dump(2) layout (free with nsh_free).  -1 without a device context (there is no CPU path) or on failure. */
int nsh_engine_suggest_json(nsh_engine* e, const char* input, uint64_t input_len, int limit, char** json_out);
/* A batch of suggest requests: input q = bytes[offsets[q] .. offsets[q + 1]) (offsets: n_inputs + 1 entries).  With
 * L = clamp(limit, 1, 10): term_idx[q * L + r] = row of the suggest table (nsh_engine_suggest_table) of suggestion r,
 * best first, ~0u past count[q]; suggestion r = input[0 .. base_len[q]) + that row's term.  device_ms (may be NULL):
 * kernel time summed over the batch's device calls. */
int nsh_engine_suggest_batch(nsh_engine* e, const char* bytes, const uint64_t* offsets, uint32_t n_inputs, int limit,
                             uint32_t* term_idx, uint32_t* count, uint32_t* base_len, float* device_ms);
/* The sorted suggest table the last reload built (valid until close/reload): term i = pool[offsets[i] .. offsets[i + 1]),
 * scores[i] = its df summed over the segments.  build_ms: the table's host build time in that reload; upload_ms: its
 * upload and device tree build (0 on a host-only engine, which has the table too).  Any output may be NULL. */
int nsh_engine_suggest_table(nsh_engine* e, const char** pool, const uint64_t** offsets, const uint32_t** scores,
                             uint64_t* n_terms, double* build_ms, double* upload_ms);
/* The request split alone (src/api_autocomplete.cpp:176-187): *base_len = bytes of the input before its last alnum run;
 * the run lower-cased (the prefix) is written to prefix (up to cap bytes, not NUL-terminated); returns its length. */
uint64_t nsh_suggest_split(const char* input, uint64_t input_len, uint64_t* base_len, char* prefix, uint64_t cap);
/* The limit clamp of Engine::suggest (src/api_engine.cpp:171): 1..10. */
int nsh_suggest_clamp_limit(int limit);

/* Spelling correction ("did you mean") over the suggest table, on the primary device.  The first call after
 * a reload builds the corrector's side structures (nsh_engine_correct_build_ms: that build's time, 0 before it).
 * nsh_engine_correct_batch: term q = bytes[offsets[q] .. offsets[q + 1]), normalised like the table's terms (ASCII alnum
 * bytes, lower-cased).  With L = clamp(limit, 1, 10): term_idx[q * L + r] = suggest-table row of the r-th best candidate
 * (~0u past count[q]), dist[q * L + r] = its distance (0xff past the end).  Candidates: rows with a score above 0, of equal
 * strings the first; distance: optimal string alignment over bytes, at most max_edits (0..2, or -1 = auto:
 * nsh_correct_auto_edits of the normalised length); with p = min(prefix_len, length) a candidate shares the term's first p
 * bytes; order: distance, score descending, row ascending.  A term that normalises to nothing or to more than 64 bytes
 * gets count 0.  -1 without a device context, for max_edits above 2, or on failure. */
int nsh_engine_correct_batch(nsh_engine* e, const char* bytes, const uint64_t* offsets, uint32_t n_terms, int limit,
                             int max_edits, int prefix_len, uint32_t* term_idx, uint8_t* dist, uint32_t* count, float* device_ms);
/* Engine::did_you_mean(query, limit): *json_out receives {"changed", "corrected", "query", "terms"} in dump(2) layout
 * (free with nsh_free).  "terms" lists the query's alnum runs without stop words and one-byte tokens: "known" = the term
 * dictionary holds it (no suggestions), else its best L with auto edits and no prefix; "corrected" = the query with each
 * unknown token that has a suggestion replaced by the best one, every other byte kept. */
int nsh_engine_did_you_mean_json(nsh_engine* e, const char* query, uint64_t query_len, int limit, char** json_out);
/* The auto rule: under 3 bytes 0 edits, 3..5 one, above 5 two. */
int nsh_correct_auto_edits(uint64_t normalized_len);
double nsh_engine_correct_build_ms(nsh_engine* e);

/* Typo-tolerant completion over the suggest table, on the primary device: suggest for a prefix that is still
 * being typed and already has a typo in it.  Shares the corrector's side structures (built by the first call after a reload).
 * nsh_engine_complete_batch: input q = bytes[offsets[q] .. offsets[q + 1]) is split like a suggest request: its last alnum
 * run, lower-cased, is the prefix and base_len[q] counts the bytes before it.  Rows as nsh_engine_correct_batch's, for the
 * candidates SOME PREFIX OF WHICH is within max_edits (0..2, or -1 = auto: nsh_correct_auto_edits of the prefix length) of the
 * prefix, of any length, that share its first min(prefix_len, length) bytes exactly; order: distance, score descending, row
 * ascending; completion r of input q = input[0, base_len[q]) + term term_idx[q * L + r].  A prefix of 0 or more than 64
 * bytes gets count 0.  -1 without a device context, for max_edits above 2, or on failure. */
int nsh_engine_complete_batch(nsh_engine* e, const char* bytes, const uint64_t* offsets, uint32_t n_inputs, int limit,
                              int max_edits, int prefix_len, uint32_t* term_idx, uint8_t* dist, uint32_t* count,
                              uint32_t* base_len, float* device_ms);
/* Engine::complete(input, limit): *json_out receives {"limit", "query", "suggestions": [{"distance", "score", "suggestion",
 * "term"}]} in dump(2) layout (free with nsh_free): auto edits, prefix_len 1; suggestion = base + term. */
int nsh_engine_complete_json(nsh_engine* e, const char* input, uint64_t input_len, int limit, char** json_out);

/* "More like this" (host/similar.hpp is the rule, csrc/ns_similar.hip runs it on the device).
 * nsh_similar_select_host: the selection rule on one host thread, over the arrays ns_docterms_upload / ns_docterms_select
 * take: counts[n_docs] and pairs (u32 {termId, tf} x n_pairs) of a segment's forward index, df[n_terms] / idf[n_terms] by
 * term id, doc_ids[n]; term_out / w_out n x T with T = nsh_similar_clamp_terms(max_terms), count_out[n]; rows padded
 * with ~0u / 0.0f.  -1 for counts that do not sum to n_pairs, a doc id >= n_docs or a termId >= n_terms. */
int nsh_similar_select_host(const uint32_t* counts, uint32_t n_docs, const uint32_t* pairs, uint64_t n_pairs, const uint32_t* df,
                            const float* idf, uint32_t n_terms, const uint32_t* doc_ids, uint32_t n, uint32_t max_terms,
                            uint32_t min_tf, uint32_t min_df, uint32_t max_df, uint32_t* term_out, float* w_out, uint32_t* count_out);
uint32_t nsh_similar_clamp_terms(uint32_t max_terms);   /* 1..32 */
int nsh_similar_clamp_k(int k);                          /* 1..99: the search behind it runs with k + 1 */
/* the query weight of a selected term: 1.0f, or with boost w / w_first (one fp32 division) */
float nsh_similar_qweight(float w, float w_first, int boost);
/* The defaults of Engine::more_like_this (any output may be NULL). */
void nsh_similar_defaults(uint32_t* max_terms, uint32_t* min_tf, uint32_t* min_df, uint32_t* max_df, int* boost);
/* df / idf by term id of segment seg (manifest position), as similar_batch uploads them: the segment's own lexicon entry of
 * terms.bin[t], idf = bm25_idf(N, df); a term without an entry has df 0 and idf 0.  Returns the segment's number of terms
 * and fills up to cap entries of each array (either may be NULL); -1 when the segment has no forward.bin / terms.bin (the
 * message names it).  Host only. */
int64_t nsh_engine_similar_term_stats(nsh_engine* e, uint32_t seg, uint32_t* df_out, float* idf_out, uint64_t cap);
/* Engine::similar_batch: source q = (manifest position, docId) = (seg_doc[2q], seg_doc[2q + 1]).  With K = nsh_similar_clamp_k(k):
 * hits n x K (unused tail entries {-inf, ~0, ~0}), nhits[n], found[n], usable[n] (0: nothing selected).  Optional (each may be
 * NULL): term_count[n] and term_w[n x T] (the selected terms' weights w = tf * idf, 0.0f past the count) and, malloc'ed
 * (nsh_free), *term_bytes_out / *term_offsets_out: the selected terms of all sources back to back, source-major in selection
 * order, term j = bytes[offsets[j] .. offsets[j + 1]), sum(term_count) + 1 offsets.  -1 for a pair out of range (nothing runs),
 * a segment without forward files, no device, or on failure. */
int nsh_engine_similar_batch(nsh_engine* e, const uint32_t* seg_doc, uint64_t n, int k, uint32_t max_terms, uint32_t min_tf,
                             uint32_t min_df, uint32_t max_df, int boost, ns_hit* hits, uint32_t* nhits, uint64_t* found,
                             uint8_t* usable, uint32_t* term_count, float* term_w, char** term_bytes_out, uint64_t** term_offsets_out);
/* Engine::more_like_this(uid, k): *json_out receives {"found", "k", "query_terms": [{"term", "weight"}], "results", "segments",
 * "source": {"cord_uid", "docId", "segment"}} in dump(2) layout (free with nsh_free); default options; the first document that
 * carries the uid is the source.  -1 for an unknown uid and on failure (nsh_engine_error has the message). */
int nsh_engine_more_like_this_json(nsh_engine* e, const char* uid, uint64_t uid_len, int k, char** json_out);
/* Frees the device copies similar_batch built (reload does too); the count of segments that have one right now. */
void nsh_engine_release_similar(nsh_engine* e);
uint64_t nsh_engine_similar_segments_on_device(nsh_engine* e);

/* Related terms (host/related.hpp is the rule, csrc/ns_terms.hip runs it on the device).
 * nsh_related_aggregate_host: the rule on one host thread, over the arrays ns_docterms_upload / ns_docterms_aggregate take:
 * counts[n_docs] and pairs (u32 {termId, tf} x n_pairs), df[n_terms] / idf[n_terms] by term id, row i = doc_ids[row_off[i] ..
 * row_off[i + 1]); term_out / docs_out / w_out n_rows x T with T = clamp(max_terms, 1, 64), count_out / ndocs_out[n_rows];
 * rows padded with ~0u / 0 / 0.0f.  -1 for counts that do not sum to n_pairs, a bad row_off, a doc id >= n_docs, a termId
 * >= n_terms, a row of more than 255 distinct documents and a visited document whose term ids do not ascend. */
int nsh_related_aggregate_host(const uint32_t* counts, uint32_t n_docs, const uint32_t* pairs, uint64_t n_pairs, const uint32_t* df,
                               const float* idf, uint32_t n_terms, const uint32_t* doc_ids, const uint64_t* row_off, uint32_t n_rows,
                               uint32_t max_terms, uint32_t min_tf, uint32_t min_docs, uint32_t min_df, uint32_t max_df,
                               uint32_t* term_out, uint32_t* docs_out, float* w_out, uint32_t* count_out, uint32_t* ndocs_out);
/* Engine::terms_batch: row q = the (manifest position, docId) pairs seg_doc[2j], seg_doc[2j + 1] for j in row_off[q] ..
 * row_off[q + 1].  With To = clamp(max_terms, 1, 32): docs_out / df_out / w_out n_rows x To (0 past count_out[q]),
 * ndocs_out[n_rows]; optional, malloc'ed (nsh_free): *term_bytes_out / *term_offsets_out, the terms of all rows back to back,
 * row-major in rank order, sum(count_out) + 1 offsets.  device_ms_out may be NULL.  -1 for a pair out of range or a bad
 * row_off (nothing runs), a row over the cap, a segment without forward files, no device, or on failure. */
int nsh_engine_terms_batch(nsh_engine* e, const uint32_t* seg_doc, const uint64_t* row_off, uint64_t n_rows, uint32_t max_terms,
                           uint32_t min_tf, uint32_t min_docs, uint32_t min_df, uint32_t max_df, uint32_t* docs_out, uint64_t* df_out,
                           float* w_out, uint32_t* count_out, uint32_t* ndocs_out, char** term_bytes_out, uint64_t** term_offsets_out,
                           float* device_ms_out);
/* Engine::related_terms: *json_out receives {"found", "query", "sample", "segments", "terms": [{"df", "docs", "term",
 * "weight"}]} in dump(2) layout (free with nsh_free).  filtered != 0: the search runs under the date filter (date_from,
 * date_to, keep_undated) as nsh_engine_search_filtered_json's.  -1 on failure (nsh_engine_error has the message). */
int nsh_engine_related_terms_json(nsh_engine* e, const char* query, uint32_t max_terms, uint32_t min_tf, uint32_t min_docs, uint32_t min_df,
                                  uint32_t max_df, uint32_t sample, int filtered, const char* date_from, const char* date_to,
                                  int keep_undated, char** json_out);

/* ---- filtered search (host/filter.hpp) ----
 * nsh_date_key: "YYYY", "YYYY-MM" (01..12) or "YYYY-MM-DD" (01..31), blanks stripped -> Y * 10000 + M * 100 + D with the
 * missing parts 0; anything else 0 = undated.
 * A date filter keeps the documents with date_from <= key <= date_to; a missing part of date_to counts as 99, an empty or NULL
 * bound is open, undated documents (no metadata row included) are kept only with keep_undated; a bound that is neither empty
 * nor a date fails the call.  With date_from = "2020-03" a document dated just "2020" is NOT kept. */
uint32_t nsh_date_key(const char* s, uint64_t len);
/* Engine::filter_bits (host only): words_out (capacity cap words, may be NULL) receives the segments' keep-bitmaps back to
 * back in manifest order, ceil(N / 32) words each, unused bits 0.  Returns the number of words in all, or -1. */
int64_t nsh_engine_filter_bits(nsh_engine* e, const char* date_from, const char* date_to, int keep_undated, uint32_t* words_out, uint64_t cap);
/* Engine::open_filter: filtered copies of the segments' posting streams on the primary device (ns_segment_filter).  At most 8
 * filters are open; all or nothing.  stats_u64 (6 values, may be NULL): documents kept / total, postings kept / total,
 * segments that got a device copy, bytes of HBM; stats_ms (2, may be NULL): the device passes, the whole call.  The handle is
 * good until nsh_engine_close_filter or the next reload (add_documents, compact and delete reload).  -1 without a device. */
int nsh_engine_open_filter(nsh_engine* e, const char* date_from, const char* date_to, int keep_undated, uint32_t* handle_out,
                           uint64_t* stats_u64, double* stats_ms);
/* The same for a caller's bitmaps (laid out as nsh_engine_filter_bits writes them; n_words must match exactly). */
int nsh_engine_open_filter_bits(nsh_engine* e, const uint32_t* words, uint64_t n_words, uint32_t* handle_out, uint64_t* stats_u64,
                                double* stats_ms);
/* -1 for a stale handle (the message says so). */
int nsh_engine_close_filter(nsh_engine* e, uint32_t handle);
uint32_t nsh_engine_open_filters(nsh_engine* e);
/* nsh_engine_search_batch under an open filter: the unfiltered ranking restricted to kept documents (same score bits), found =
 * kept documents that match, hits in manifest positions.  A query with base terms stays usable with found = 0 when nothing
 * kept matches.  NS_FLAG_AND: a document must hold every term the unfiltered query has in its segment. */
int nsh_engine_search_filtered_batch(nsh_engine* e, uint32_t handle, const char* const* queries, uint32_t n_queries, int k, uint32_t flags,
                                     ns_hit* hits, uint32_t* nhits, uint64_t* found, uint8_t* has_found);
/* Engine::search_filtered: *json_out (free with nsh_free) = search's body plus "filter": {"date_from", "date_to", "documents",
 * "keep_undated"}; the last 4 distinct filters stay open (they count towards the 8).  On failure -1 and *json_out =
 * {"error": ...}. */
int nsh_engine_search_filtered_json(nsh_engine* e, const char* query, int k, const char* date_from, const char* date_to, int keep_undated,
                                    char** json_out);

/* ---- facet counts (host/facet.hpp) ----
 * kind: 0 year, 1 month (metadata.csv's publish_time through nsh_date_key: key / 10000, key / 100), 2 custom.  Bucket 0 is
 * "undated" with the label ""; the other buckets are the distinct values present in the index, ascending ("2020", "2020-03";
 * under month a document dated only "2020" lands in a bucket labelled "2020" in front of 2020's months).  More than 1023
 * distinct values fail the call.  The documents of year bucket "Y" are exactly what the date filter Y..Y keeps.
 * custom: custom_buckets = the segments' bucket arrays back to back in manifest order (n_custom ids in all, one per document,
 * each < n_custom_labels <= 1024); labels as given. */
typedef struct nsh_facet_spec {
    uint32_t kind;
    uint32_t n_custom_labels;
    const uint16_t* custom_buckets;
    uint64_t n_custom;
    const char* const* custom_labels;
} nsh_facet_spec;
/* Engine::facet_buckets (host only): buckets_out (capacity cap ids, may be NULL) receives the segments' tables back to back in
 * manifest order; *n_buckets_out the number of buckets; *labels_out (free with nsh_free; may be NULL) the labels, each
 * followed by a 0 byte, *labels_bytes_out bytes in all.  Returns the number of ids in all (= documents), or -1. */
int64_t nsh_engine_facet_buckets(nsh_engine* e, const nsh_facet_spec* spec, uint16_t* buckets_out, uint64_t cap, uint32_t* n_buckets_out,
                                 char** labels_out, uint64_t* labels_bytes_out);
/* Engine::facet_batch_flat: counts_out[q * B + b] = the distinct documents of bucket b that query q matches (B as
 * nsh_engine_facet_buckets reports it; counts_cap entries of capacity, fewer than n_queries * B fail the call), found[q] their
 * sum = the found of nsh_engine_search_batch (nsh_engine_search_filtered_batch under filter_handle; 0 = no filter) for the
 * same query and flags, has_found[q] as there.  The device copies of the tables are built by the first call that needs them.
 * device_ms_out, count_ms_out (may be NULL): the kernels' HIP-event time and the wall time inside ns_facet_count, summed over
 * the sub-batches.  -1 without a device, for a stale handle, or on failure. */
int nsh_engine_facet_batch(nsh_engine* e, const nsh_facet_spec* spec, uint32_t filter_handle, const char* const* queries, uint32_t n_queries,
                           uint32_t flags, uint32_t* counts_out, uint64_t counts_cap, uint64_t* found, uint8_t* has_found, float* device_ms_out,
                           double* count_ms_out);
/* Engine::search_faceted: *json_out (free with nsh_free) = search's body (search_filtered's with use_filter != 0) plus
 * "facets": {"<year|month|custom>": [{"count", "value"}, ...]}, nonzero buckets only, in bucket order.  On failure -1 and
 * *json_out = {"error": ...}. */
int nsh_engine_search_faceted_json(nsh_engine* e, const char* query, int k, const nsh_facet_spec* spec, int use_filter, const char* date_from,
                                   const char* date_to, int keep_undated, char** json_out);
/* Frees the device copies of the bucket tables (reload does too); how many tables have one right now. */
void nsh_engine_release_facets(nsh_engine* e);
uint64_t nsh_engine_facet_tables_on_device(nsh_engine* e);

/* ---- search sorted by date (host/sorted.hpp) ----
 * A sort order is one uint32 key per document and a direction: kind 0 = date_key() of metadata.csv's publish_time (YYYYMMDD,
 * missing parts 0, undated 0), kind 1 = the caller's keys (the segments' arrays back to back in manifest order; n_custom =
 * their total).  Key 0 is last in both directions; 0xFFFFFFFF is reserved and refused. */
typedef struct nsh_sort_spec {
    uint32_t kind;         /* 0 date, 1 custom */
    uint32_t ascending;    /* 0: newest (largest key) first; else oldest (smallest non-zero key) first */
    const uint32_t* custom_keys;
    uint64_t n_custom;
} nsh_sort_spec;
/* Engine::sort_keys (host only): keys_out (capacity cap keys, may be NULL) receives the segments' keys back to back in
 * manifest order.  Returns their total number, or -1 (nsh_engine_error). */
int64_t nsh_engine_sort_keys(nsh_engine* e, const nsh_sort_spec* spec, uint32_t* keys_out, uint64_t cap);
/* Engine::search_sorted_batch_flat: per query the first K = clamp(k, 1, 100) matched documents in the order (key, manifest
 * position ascending, docId ascending) with their BM25 scores; hits (n_queries x K nsh/ns_hit {score, segment position,
 * docId}), keys_out (n_queries x K), nhits, found, has_found as nsh_engine_search_batch's (found 0 where has_found is 0).
 * flags: NS_FLAG_OR or NS_FLAG_AND.  filter_handle: an open filter's, or 0.  device_ms_out (may be NULL): the kernels' time. */
int nsh_engine_search_sorted_batch(nsh_engine* e, const nsh_sort_spec* spec, uint32_t filter_handle, const char* const* queries, uint32_t n_queries,
                                   int k, uint32_t flags, void* hits, uint32_t* keys_out, uint32_t* nhits, uint64_t* found, uint8_t* has_found,
                                   float* device_ms_out);
/* Engine::search_sorted: *json_out (free with nsh_free) = search's body (search_filtered's with use_filter != 0) with "results"
 * in date order plus "sort": "newest" | "oldest" | "custom".  On failure -1 and {"error": ...}. */
int nsh_engine_search_sorted_json(nsh_engine* e, const char* query, int k, const nsh_sort_spec* spec, int use_filter, const char* date_from,
                                  const char* date_to, int keep_undated, char** json_out);
void nsh_engine_release_sorted(nsh_engine* e);
uint64_t nsh_engine_sort_tables_on_device(nsh_engine* e);

/* ---- boolean queries (host/boolean.hpp) ----
 * nsx::parse_boolean (host only, no engine): the query is split on whitespace; a piece that begins with '+' (MUST) or '-' (NOT)
 * gives that role to every token the search's tokenizer takes from the rest of the piece, all other pieces are SHOULD; stop
 * words and one-byte tokens are dropped, duplicates stay.  buf receives the terms joined by single spaces (NUL-terminated,
 * truncated to cap), roles (capacity roles_cap, may be NULL) one NS_ROLE_* byte per term.  Returns the number of terms. */
uint32_t nsh_parse_boolean(const char* query, char* buf, uint32_t cap, uint8_t* roles, uint32_t roles_cap);
/* Engine::search_boolean_batch_flat: per query the K = clamp(k, 1, 100) best documents that hold every `+word`, no `-word` and,
 * without a `+word`, at least one other word, in the search's order with the search's scores; hits (n_queries x K nsh/ns_hit
 * {score, segment position, docId}), nhits, found, has_found as nsh_engine_search_batch's (found 0 where has_found is 0).
 * filter_handle: an open filter's, or 0.  device_ms_out (may be NULL): the kernels' time. */
int nsh_engine_search_boolean_batch(nsh_engine* e, uint32_t filter_handle, const char* const* queries, uint32_t n_queries, int k, void* hits,
                                    uint32_t* nhits, uint64_t* found, uint8_t* has_found, float* device_ms_out);
/* Engine::search_boolean: *json_out (free with nsh_free) = search's body (search_filtered's with use_filter != 0) over the
 * boolean result plus "boolean": {"must", "must_not", "should"}.  On failure -1 and {"error": ...}. */
int nsh_engine_search_boolean_json(nsh_engine* e, const char* query, int k, int use_filter, const char* date_from, const char* date_to,
                                   int keep_undated, char** json_out);

/* ---- pages past the first K (host/page.hpp) ----
 * A cursor is a position (rank, manifest position of the segment, docId) in the total order of a ranked call: rank = the fp32
 * score bits in score order (kind 's'), the sort key as uploaded in date order (kind 'd').  A call with a cursor answers with
 * the first K matched documents strictly after it.  set == 0: no cursor.  A cursor is good until a reload changes the index. */
typedef struct nsh_page_cursor {
    uint32_t set, rank, seg, doc;
} nsh_page_cursor;
/* nsx::parse_cursor (host only, no engine): the text form is the kind letter, 8 lowercase hex digits of rank, '.', the position
 * in decimal, '.', the docId in decimal, e.g. s41a3c28f.0.5121; the empty string is the unset cursor; anything else, or a
 * cursor of another kind than `kind` ('s' or 'd'), fails with -1 and a message in err (NUL-terminated, truncated to err_cap). */
int nsh_parse_cursor(const char* text, int kind, nsh_page_cursor* out, char* err, uint32_t err_cap);
/* nsx::cursor_text: the text form into buf (NUL-terminated, truncated to cap); returns its length, 0 for an unset cursor. */
uint32_t nsh_cursor_text(int kind, const nsh_page_cursor* c, char* buf, uint32_t cap);
/* Engine::search_after_batch_flat / search_boolean_after_batch_flat / search_sorted_after_batch_flat: nsh_engine_search_batch
 * (nsh_engine_search_filtered_batch under a handle), nsh_engine_search_boolean_batch and nsh_engine_search_sorted_batch with one
 * cursor per query (after: n_queries, or NULL for none).  found is unchanged by a cursor; rest[q] (may be NULL) = the matched
 * documents strictly after the cursor, nhits[q] = min(K, rest[q]); without a cursor rest = found.  A cursor whose position is
 * outside the index, or of which the filter keeps nothing, is refused: -1 and nsh_engine_error. */
int nsh_engine_search_after_batch(nsh_engine* e, uint32_t filter_handle, const char* const* queries, uint32_t n_queries, int k, uint32_t flags,
                                  const nsh_page_cursor* after, void* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* has_found,
                                  float* device_ms_out);
int nsh_engine_search_boolean_after_batch(nsh_engine* e, uint32_t filter_handle, const char* const* queries, uint32_t n_queries, int k,
                                          const nsh_page_cursor* after, void* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                          uint8_t* has_found, float* device_ms_out);
int nsh_engine_search_sorted_after_batch(nsh_engine* e, const nsh_sort_spec* spec, uint32_t filter_handle, const char* const* queries,
                                         uint32_t n_queries, int k, uint32_t flags, const nsh_page_cursor* after, void* hits, uint32_t* keys_out,
                                         uint32_t* nhits, uint64_t* found, uint64_t* rest, uint8_t* has_found, float* device_ms_out);
/* ---- facet counts and date order for boolean queries ----
 * Engine::facet_boolean_batch_flat: nsh_engine_facet_batch over nsh_engine_search_boolean_batch's matched set (`+word`, `-word`);
 * found and has_found equal nsh_engine_search_boolean_batch's.
 * Engine::search_boolean_sorted_batch_flat: nsh_engine_search_sorted_after_batch over that set, hits with the boolean score bits;
 * after: n_queries cursors of kind 'd', or NULL for page 1; rest may be NULL. */
int nsh_engine_facet_boolean_batch(nsh_engine* e, const nsh_facet_spec* spec, uint32_t filter_handle, const char* const* queries, uint32_t n_queries,
                                   uint32_t* counts_out, uint64_t counts_cap, uint64_t* found, uint8_t* has_found, float* device_ms_out);
int nsh_engine_search_boolean_sorted_batch(nsh_engine* e, const nsh_sort_spec* spec, uint32_t filter_handle, const char* const* queries,
                                           uint32_t n_queries, int k, const nsh_page_cursor* after, void* hits, uint32_t* keys_out, uint32_t* nhits,
                                           uint64_t* found, uint64_t* rest, uint8_t* has_found, float* device_ms_out);
/* Engine::search_boolean_faceted / search_boolean_sorted: *json_out (free with nsh_free) = nsh_engine_search_boolean_json's body
 * plus "facets" (as nsh_engine_search_faceted_json's), or with "results" in date order plus "sort" (as
 * nsh_engine_search_sorted_json's).  On failure -1 and {"error": ...}. */
int nsh_engine_search_boolean_faceted_json(nsh_engine* e, const char* query, int k, const nsh_facet_spec* spec, int use_filter, const char* date_from,
                                           const char* date_to, int keep_undated, char** json_out);
int nsh_engine_search_boolean_sorted_json(nsh_engine* e, const char* query, int k, const nsh_sort_spec* spec, int use_filter, const char* date_from,
                                          const char* date_to, int keep_undated, char** json_out);

/* Engine::search_page: *json_out (free with nsh_free) = the mode's body (0 search OR, 1 search AND, 2 boolean, 3 sorted by spec,
 * 4 boolean sorted by spec: nsh_engine_search_boolean_sorted_json's body, cursors of kind 'd';
 * search_filtered's with use_filter != 0) over one page, plus "page": {"cursor", "next", "offset", "remaining"}; "next" is
 * present only when documents remain.  cursor: "" or NULL for the first page, else a page's "next".  On failure -1 and
 * {"error": ...}. */
int nsh_engine_search_page_json(nsh_engine* e, const char* query, int k, const char* cursor, uint32_t mode, const nsh_sort_spec* spec, int use_filter,
                                const char* date_from, const char* date_to, int keep_undated, char** json_out);

/* ---- any-of groups in boolean queries (host/grouped.hpp) ----
 * nsx::parse_grouped: parse_boolean's dialect with one level of parentheses.  A piece that begins, after an optional '+' or '-',
 * with '(' opens a group that runs to the first ')' (or to the end of the query); every token of its body gets the group's role,
 * and the tokens of a MUST group share one clause id: `+(covid coronavirus sars) +vaccine -mouse`.  Every other MUST token is a
 * clause of its own; a text without '(' parses as nsh_parse_boolean parses it.  The terms go to buf joined by single spaces
 * (truncated to cap - 1 bytes), roles[i] and clauses[i] (i < terms_cap; clause ids count up from 0 in query order, 0 on SHOULD
 * and NOT terms) next to them; returns the number of terms. */
uint32_t nsh_parse_grouped(const char* query, char* buf, uint32_t cap, uint8_t* roles, uint32_t* clauses, uint32_t terms_cap);
/* Engine::search_grouped_after_batch_flat, facet_grouped_batch_flat, search_grouped_sorted_batch_flat: the boolean batch calls
 * (nsh_engine_search_boolean_after_batch, nsh_engine_facet_boolean_batch, nsh_engine_search_boolean_sorted_batch) over that
 * dialect, parameter for parameter: a document must hold at least one term of every required group.  A term of a group that the
 * index does not know is dropped; a group of only unknown terms matches nothing.  More than 65 535 required clauses in one query:
 * -1 with a message. */
int nsh_engine_search_grouped_after_batch(nsh_engine* e, uint32_t filter_handle, const char* const* queries, uint32_t n_queries, int k,
                                          const nsh_page_cursor* after, void* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                          uint8_t* has_found, float* device_ms_out);
int nsh_engine_facet_grouped_batch(nsh_engine* e, const nsh_facet_spec* spec, uint32_t filter_handle, const char* const* queries, uint32_t n_queries,
                                   uint32_t* counts_out, uint64_t counts_cap, uint64_t* found, uint8_t* has_found, float* device_ms_out);
int nsh_engine_search_grouped_sorted_batch(nsh_engine* e, const nsh_sort_spec* spec, uint32_t filter_handle, const char* const* queries,
                                           uint32_t n_queries, int k, const nsh_page_cursor* after, void* hits, uint32_t* keys_out, uint32_t* nhits,
                                           uint64_t* found, uint64_t* rest, uint8_t* has_found, float* device_ms_out);
/* Engine::search_grouped, search_grouped_faceted, search_grouped_sorted: *json_out (free with nsh_free) = the body of
 * nsh_engine_search_boolean_json / _faceted_json / _sorted_json over this dialect, with "grouped": {"must": [[...], ...], "must_not":
 * [...], "should": [...]} in place of "boolean" (keys stay sorted): "must" lists the clauses, each the list of its terms.  On failure -1 and
 * {"error": ...}.  nsh_engine_search_page_json pages them with mode 5 (grouped, cursors of kind 's') and mode 6 (grouped, sorted by
 * spec, cursors of kind 'd'). */
int nsh_engine_search_grouped_json(nsh_engine* e, const char* query, int k, int use_filter, const char* date_from, const char* date_to,
                                   int keep_undated, char** json_out);
int nsh_engine_search_grouped_faceted_json(nsh_engine* e, const char* query, int k, const nsh_facet_spec* spec, int use_filter, const char* date_from,
                                           const char* date_to, int keep_undated, char** json_out);
int nsh_engine_search_grouped_sorted_json(nsh_engine* e, const char* query, int k, const nsh_sort_spec* spec, int use_filter, const char* date_from,
                                          const char* date_to, int keep_undated, char** json_out);

/* ---- at-least-m-of-n clauses in boolean queries (host/quorum.hpp) ----
 * nsx::parse_quorum: nsh_parse_grouped's dialect plus two forms.  A group's ')' directly followed by '~' and decimal digits sets
 * the group's need m: `+(fever cough dyspnea fatigue)~2` is a required clause of which a document must hold at least two terms, and
 * so is the bare `(...)~2`; on a `-( )` group the suffix is consumed and ignored.  A whole piece `~m` makes ALL optional terms of
 * the query one required clause of need m (the last such piece wins, `~0` is none).  A text with neither form parses as
 * nsh_parse_grouped parses it.  The terms go to buf joined by single spaces (truncated to cap - 1 bytes); roles[i], clauses[i],
 * needs[i] (the need of a MUST term's clause, 0 on SHOULD and NOT terms) and promoted[i] (1: an optional term that `~m` made a
 * member of the last clause) next to them (i < terms_cap; each may be NULL); *min_should_out (may be NULL) = the `~m` piece's m,
 * 0 for none; returns the number of terms.  The parser is total; the engine refuses a need above 7. */
uint32_t nsh_parse_quorum(const char* query, char* buf, uint32_t cap, uint8_t* roles, uint32_t* clauses, uint32_t* needs, uint8_t* promoted,
                          uint32_t terms_cap, uint32_t* min_should_out);
/* Engine::search_quorum_after_batch_flat, facet_quorum_batch_flat, search_quorum_sorted_batch_flat: the grouped batch calls over
 * that dialect, parameter for parameter, filters and cursors included.  A term of a clause that the index does not know is dropped
 * and the need stays: a need above the known terms matches nothing.  A need above 7, or more than 65 535 required clauses in one
 * query: -1 with a message. */
int nsh_engine_search_quorum_after_batch(nsh_engine* e, uint32_t filter_handle, const char* const* queries, uint32_t n_queries, int k,
                                         const nsh_page_cursor* after, void* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                         uint8_t* has_found, float* device_ms_out);
int nsh_engine_facet_quorum_batch(nsh_engine* e, const nsh_facet_spec* spec, uint32_t filter_handle, const char* const* queries, uint32_t n_queries,
                                  uint32_t* counts_out, uint64_t counts_cap, uint64_t* found, uint8_t* has_found, float* device_ms_out);
int nsh_engine_search_quorum_sorted_batch(nsh_engine* e, const nsh_sort_spec* spec, uint32_t filter_handle, const char* const* queries,
                                          uint32_t n_queries, int k, const nsh_page_cursor* after, void* hits, uint32_t* keys_out, uint32_t* nhits,
                                          uint64_t* found, uint64_t* rest, uint8_t* has_found, float* device_ms_out);
/* Engine::search_quorum, search_quorum_faceted, search_quorum_sorted: *json_out (free with nsh_free) = the body of
 * nsh_engine_search_grouped_json / _faceted_json / _sorted_json over this dialect, with "quorum": {"min_should": m, "must": [{"need":
 * n, "terms": [...]}, ...], "must_not": [...], "should": [...]} in place of "grouped" (keys stay sorted: behind "query"); the terms a
 * `~m` piece promoted are listed under "should".  On failure -1 and {"error": ...}.  nsh_engine_search_page_json pages them with
 * mode 7 (quorum, cursors of kind 's') and mode 8 (quorum, sorted by spec, cursors of kind 'd'). */
int nsh_engine_search_quorum_json(nsh_engine* e, const char* query, int k, int use_filter, const char* date_from, const char* date_to,
                                  int keep_undated, char** json_out);
int nsh_engine_search_quorum_faceted_json(nsh_engine* e, const char* query, int k, const nsh_facet_spec* spec, int use_filter, const char* date_from,
                                          const char* date_to, int keep_undated, char** json_out);
int nsh_engine_search_quorum_sorted_json(nsh_engine* e, const char* query, int k, const nsh_sort_spec* spec, int use_filter, const char* date_from,
                                         const char* date_to, int keep_undated, char** json_out);

/* ---- boosts: per-document factors, recency decay and term^w (host/boost.hpp) ----
 * A boost is one fp32 factor per document; the device multiplies a matched document's finished score by it, once, and ranks by
 * the product.  kind 0 custom: `custom` holds the segments' factor arrays back to back in manifest order, n_custom = the documents
 * of the index; a factor that is negative (-0.0f included) or not finite is refused.  kind 1 exponential: f = 2^(-age /
 * scale_days); kind 2 linear: f = max(0, 1 - age / scale_days); age = max(0, |days(origin) - days(date)| - offset_days) in civil
 * days of the document's publish_time (a missing month or day reads as 1); origin: a date as the filter bounds are, NULL or "" =
 * the newest dated document; an undated document takes f = undated.  The factor of kinds 1 and 2 is (1 - weight) + weight * f,
 * computed in double and rounded once to fp32; weight = 0 gives 1.0f everywhere and so the unboosted answers, bit for bit.
 * Refused with a message: weight outside [0, 1], scale_days <= 0, offset_days or undated below 0, an origin that is not a date. */
typedef struct nsh_boost_spec {
    uint32_t kind;
    double weight;
    const char* origin;
    double scale_days, offset_days, undated;
    const float* custom;
    uint64_t n_custom;
} nsh_boost_spec;
/* Engine::boost_table (host only: works with device < 0): the factors of every document, the segments back to back in manifest
 * order, into out[0 .. cap); returns their number (call with cap = 0 to size the array), or -1 with a message. */
int64_t nsh_engine_boost_table(nsh_engine* e, const nsh_boost_spec* spec, float* out, uint64_t cap);
/* The device copies of a spec's tables are built by the first call that needs them and kept until another spec, a reload() or
 * this call drops them. */
void nsh_engine_release_boosts(nsh_engine* e);
uint64_t nsh_engine_boost_tables_on_device(nsh_engine* e);
/* nsx::parse_boosted: nsh_parse_quorum's dialect plus the suffix `^w` on a word or `+word` (`vaccine^2.5`) and on a group behind
 * its ')' and optional `~m` (`+(covid sars)^0.5`, `(a b c)~2^3`).  w is digits with at most one '.', in (0, 1e6]; anything else
 * leaves the '^' to the tokenizer; on a `-` piece the suffix is consumed and ignored.  weights[i] (may be NULL) = the weight of
 * term i, 1.0f without a suffix; everything else as nsh_parse_quorum, whose answer this is for a text without a valid `^w`. */
uint32_t nsh_parse_boosted(const char* query, char* buf, uint32_t cap, uint8_t* roles, uint32_t* clauses, uint32_t* needs, uint8_t* promoted,
                           float* weights, uint32_t terms_cap, uint32_t* min_should_out);
/* Engine::search_boosted_after_batch_flat: nsh_engine_search_quorum_after_batch over that dialect, parameter for parameter, behind
 * spec (NULL: term weights only).  A hit's score, and so a cursor's rank, is the bits of fp32(score * factor). */
int nsh_engine_search_boosted_after_batch(nsh_engine* e, const nsh_boost_spec* spec, uint32_t filter_handle, const char* const* queries, uint32_t n_queries,
                                          int k, const nsh_page_cursor* after, void* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                          uint8_t* has_found, float* device_ms_out);
/* Engine::search_boosted: *json_out (free with nsh_free) = the body of nsh_engine_search_quorum_json over this dialect with
 * "boosted" in place of "quorum" (the same members; a "must" clause also carries "weight", a "should" entry is {"term", "weight"})
 * and, with a spec, "boost": {"kind", "offset_days", "origin", "scale_days", "undated", "weight"}; keys stay sorted: both stand in
 * front of "filter".  On failure -1 and {"error": ...}.  nsh_engine_search_boosted_page_json pages it (cursors of kind 's');
 * nsh_engine_search_page_json's mode 9 is that call without a spec. */
int nsh_engine_search_boosted_json(nsh_engine* e, const char* query, int k, const nsh_boost_spec* spec, int use_filter, const char* date_from,
                                   const char* date_to, int keep_undated, char** json_out);
int nsh_engine_search_boosted_page_json(nsh_engine* e, const char* query, int k, const char* cursor, const nsh_boost_spec* spec, int use_filter,
                                        const char* date_from, const char* date_to, int keep_undated, char** json_out);

/* ---- prefix terms: `vaccin*` (host/prefix.hpp) ----
 * nsx::parse_prefixed: nsh_parse_boosted's dialect plus the prefix term.  A '*' directly behind a token's last byte marks the token
 * as a prefix, provided the next byte is not alphanumeric or the text ends there, inside or outside a group and before a `^w`;
 * every other '*' stays a separator.  A prefix is lower-cased, dropped below 2 bytes and NOT tested against the stop-word list.
 * prefix[i] (may be NULL) = 1 where term i is a prefix (its text comes without the '*'); everything else as nsh_parse_boosted,
 * whose answer this is for a text without such a '*'. */
uint32_t nsh_parse_prefixed(const char* query, char* buf, uint32_t cap, uint8_t* roles, uint32_t* clauses, uint32_t* needs, uint8_t* promoted,
                            float* weights, uint8_t* prefix, uint32_t terms_cap, uint32_t* min_should_out);
/* Engine::expand_prefix (host only: works with device < 0): the terms of the autocomplete table that begin with `prefix` (a term
 * equal to it included), in byte order, joined with blanks into buf (cut at cap - 1 bytes; *bytes_out, may be NULL: the bytes the
 * whole answer needs); returns their number, or -1 with a message.  max_expansions: 1 .. 65535, 0 = the default, 1024; with more
 * matches those of the largest summed df, then the smallest bytes, stay (nsh_engine_suggest_json's order) and *truncated_out (may
 * be NULL) is 1.  A term the dictionary does not hold is skipped. */
int64_t nsh_engine_expand_prefix(nsh_engine* e, const char* prefix, uint32_t max_expansions, char* buf, uint64_t cap, uint64_t* bytes_out, int* truncated_out);
/* Engine::search_prefixed_after_batch_flat: nsh_engine_search_boosted_after_batch over that dialect, parameter for parameter, with
 * max_expansions behind spec.  In a segment a prefix is ONE blended term: the union of its expansions' lists there with the tf
 * summed per document, the df the size of the union and the idf computed from that df (ns_segment_union builds the lists on the
 * device, once per call and segment); with one expansion there it is that term's own list and idf.  A non-zero filter_handle is
 * refused with a message.  A batch without a prefix is nsh_engine_search_boosted_after_batch's call. */
int nsh_engine_search_prefixed_after_batch(nsh_engine* e, const nsh_boost_spec* spec, uint32_t max_expansions, uint32_t filter_handle, const char* const* queries,
                                           uint32_t n_queries, int k, const nsh_page_cursor* after, void* hits, uint32_t* nhits, uint64_t* found, uint64_t* rest,
                                           uint8_t* has_found, float* device_ms_out);
/* Engine::search_prefixed: *json_out (free with nsh_free) = nsh_engine_search_boosted_json's body with "prefixed" in place of
 * "boosted" (a prefix term prints with its '*') and "prefixes": [{"expansions", "prefix", "truncated"}], the query's distinct
 * prefixes in query order; keys stay sorted: both stand in front of "query".  use_filter != 0 is refused.  On failure -1 and
 * {"error": ...}.  nsh_engine_search_prefixed_page_json pages it (cursors of kind 's'). */
int nsh_engine_search_prefixed_json(nsh_engine* e, const char* query, int k, const nsh_boost_spec* spec, uint32_t max_expansions, int use_filter,
                                    const char* date_from, const char* date_to, int keep_undated, char** json_out);
int nsh_engine_search_prefixed_page_json(nsh_engine* e, const char* query, int k, const char* cursor, const nsh_boost_spec* spec, uint32_t max_expansions,
                                         int use_filter, const char* date_from, const char* date_to, int keep_undated, char** json_out);

/* ---- collapsed hits: one hit per title, author or custom key (host/collapse.hpp) ----
 * kind: 0 title (a dense id per normalised title, by first appearance in manifest order; an empty title is key 0 = stands alone),
 * 1 author (the same over the author field), 2 custom: `custom` holds one uint32 per document, the segments back to back in
 * manifest order (n_custom of them; 0 = no key, 0xFFFFFFFF refused). */
typedef struct nsh_collapse_spec {
    uint32_t kind;
    const uint32_t* custom;
    uint64_t n_custom;
} nsh_collapse_spec;
/* Engine::collapse_table (host only: works with device < 0): the keys of every document, the segments back to back in manifest
 * order, into out[0 .. cap); returns their number (call with cap = 0 to size the array), or -1 with a message. */
int64_t nsh_engine_collapse_table(nsh_engine* e, const nsh_collapse_spec* spec, uint32_t* out, uint64_t cap);
/* The device copies of a spec's keys are built by the first call that needs them and kept until another spec, a reload() or this
 * call drops them. */
void nsh_engine_release_collapse(nsh_engine* e);
uint64_t nsh_engine_collapse_tables_on_device(nsh_engine* e);
/* Engine::search_collapsed_batch_flat: nsh_engine_search_boosted_after_batch without cursors, one hit per group.  hits, groups and
 * others are n_queries x clamp(k, 1, 100); groups[q * K + r] = the hit's key, others[q * K + r] = the other matched documents
 * with that key (others may be NULL: not counted).  boost may be NULL.  A `*` prefix term is refused.  -1 with a message on
 * failure. */
int nsh_engine_search_collapsed_batch(nsh_engine* e, const nsh_collapse_spec* collapse, const nsh_boost_spec* boost, uint32_t filter_handle,
                                      const char* const* queries, uint32_t n_queries, int k, void* hits, uint32_t* groups, uint32_t* others, uint32_t* nhits,
                                      uint64_t* found, uint8_t* has_found, float* device_ms_out);
/* Engine::search_collapsed: *json_out (free with nsh_free) = nsh_engine_search_boosted_json's body with "collapsed" in place of
 * "boosted", "collapse": {"field": "title" | "author" | "custom"} in front of it and "others": n in every result.  On failure -1
 * and {"error": ...}. */
int nsh_engine_search_collapsed_json(nsh_engine* e, const char* query, int k, const nsh_collapse_spec* collapse, const nsh_boost_spec* boost, int use_filter,
                                     const char* date_from, const char* date_to, int keep_undated, char** json_out);

#ifdef __cplusplus
}
#endif
#endif /* NEXTSEARCH_HOST_H */
