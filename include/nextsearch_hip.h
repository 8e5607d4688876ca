/*
 * nextsearch_hip.h — C-ABI of libnextsearch_hip.so: the MI355X (gfx950) posting-traversal /
 * BM25-scoring / top-k hot path of NextSearch's cord19::Engine::search.
 *
 * The reference has no FFI seam: the path is an inline loop inside Engine::search.  The boundary is
 * therefore cut where that loop begins and ends (reference file:line, /root/reference/...):
 *
 *   enter : src/api_engine.cpp:441   (qterms_w final; per segment: lexicon probe :454-458 and
 *                                     bm25_idf :45-47,:461 stay on the HOST and arrive here as
 *                                     ns_term_ref{byte_off,count,idf,qweight})
 *   leave : src/api_engine.cpp:504-505 (hits sorted by score + total_found)
 *
 * Everything is plain-old-data; no exceptions cross the boundary; every entry point returns
 * NS_OK (0) or a negative NS_E* code and leaves a message retrievable with ns_last_error().
 * There is NO CPU fallback: without a usable HIP device ns_ctx_create fails with NS_E_NODEVICE.
 *
 * Threading: an ns_ctx is bound to one device and one stream and is not re-entrant (the reference
 * serialises every engine entry behind Engine::mtx, src/api_engine.cpp:372).  Segments are
 * immutable after upload.  Use one ctx per host thread / per GPU.
 */
#ifndef NEXTSEARCH_HIP_H
#define NEXTSEARCH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NS_OK            0
#define NS_E_INVAL      -1   /* bad argument (null pointer, K out of range, offset outside segment ...) */
#define NS_E_NODEVICE   -2   /* no HIP device / HIP runtime failure at init */
#define NS_E_HIP        -3   /* a HIP call failed; see ns_last_error */
#define NS_E_NOMEM      -4
#define NS_E_STATE      -5   /* call sequence error (e.g. fetch before run) */

#define NS_MAX_K        100u /* src/api_engine.cpp:377: K = clamp(k,1,100) */

/* flags for ns_search_batch / ns_batch_prepare */
#define NS_FLAG_OR      0u   /* reference semantics: every touched doc is a candidate (src/api_engine.cpp:449-492) */
#define NS_FLAG_AND     1u   /* extension (BASELINE config 2): keep docs matched by every term ref of their segment */
#define NS_INFO_IMPACTS 0x100u /* ns_batch_info.flags only (output): the batch reads impact streams (ns_segment_build_impacts) */
#define NS_INFO_PACKED  0x200u /* ns_batch_info.flags only (output): the batch's driver streams read the packed posting blocks (ns_segment_build_packed) */
#define NS_INFO_SHARED  0x800u /* ns_batch_info.flags only (output): the batch computes the BM25 term scores of its distinct lists once per run (ns_ctx_share_scores) */
#define NS_INFO_PRUNED  0x400u /* ns_batch_info.flags only (output): some single-term queries of the batch skip posting blocks by their block maxima (ns_ctx_use_pruning) */

typedef struct ns_ctx   ns_ctx;
typedef struct ns_seg   ns_seg;
typedef struct ns_batch ns_batch;

/* One scored (query term, segment) pair — replaces the reference's
 * {seg.lex.find(term) -> LexEntry; bm25_idf(seg.N,e.df); seekg(e.offset)} triple
 * (src/api_engine.cpp:454-470).  Refs of one query are contiguous and in QUERY-TERM ORDER; refs of
 * different segments may interleave (their relative order per segment is what matters: it is the
 * fp32 accumulation order of src/api_engine.cpp:480). */
typedef struct ns_term_ref {
    uint32_t seg_id;     /* id given to ns_segment_upload */
    uint32_t count;      /* LexEntry.count: postings in the list (include/api_types.hpp:27) */
    uint64_t byte_off;   /* byte offset of the list inside the uploaded posting buffer (multiple of 8) */
    float    idf;        /* host-computed bm25_idf(N, df) (src/api_engine.cpp:45-47) */
    float    qweight;    /* 1.0f, or the semantic-expansion weight (src/api_engine.cpp:410-421) */
} ns_term_ref;

typedef struct ns_query_desc {
    uint32_t term_begin; /* first ns_term_ref of this query */
    uint32_t term_count; /* may be 0: such a query returns nhits = 0, found = 0 */
} ns_query_desc;

/* struct Hit {float s; uint32_t segId; uint32_t docId;} (src/api_engine.cpp:427-431) */
typedef struct ns_hit {
    float    score;
    uint32_t seg_id;
    uint32_t doc_id;
} ns_hit;

typedef struct ns_batch_info {
    uint64_t postings;        /* P = sum over term refs of count */
    uint64_t algo_bytes;      /* 8 * P: algorithmic bytes of one run */
    uint32_t n_queries;
    uint32_t n_items;         /* (query, segment, doc-range) work items == workgroups of the scoring kernel */
    uint32_t n_term_refs;
    uint32_t tile_docs;       /* docs per LDS accumulator tile */
    uint32_t k;
    uint32_t flags;
    float    last_score_kernel_ms; /* HIP-event time of the scoring kernel in the last timed run, <0 if none */
    float    last_total_ms;        /* HIP-event time of all kernels of the last timed run, <0 if none */
    uint32_t timed_runs;           /* timed runs accumulated since prepare (read back at every sync) */
    uint32_t shared_lists;         /* distinct posting lists whose term scores the batch computes once per run (0: it does not share) */
    double   sum_score_kernel_ms;  /* sum over timed runs of the scoring kernel's HIP-event time (with the shared-score kernel in front of it, if any) */
    double   sum_total_ms;         /* sum over timed runs of first-kernel-start .. last-kernel-end */
    uint64_t shared_postings;      /* postings of those lists */
} ns_batch_info;

/* ---- context ------------------------------------------------------------------------------ */
int  ns_ctx_create(int device, ns_ctx** out);
void ns_ctx_destroy(ns_ctx* ctx);
/* Use an externally owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) for all work
 * of this ctx; NULL restores the ctx's own stream. */
int  ns_ctx_set_stream(ns_ctx* ctx, void* hip_stream);
/* Message of the last failing call on this ctx (ctx == NULL: last failing ns_ctx_create of the
 * calling thread).  Never NULL. */
const char* ns_last_error(ns_ctx* ctx);
/* "gfx950 ..." device string of the ctx's device */
const char* ns_device_name(ns_ctx* ctx);

/* ---- segments (replaces the reference's open ifstreams: include/api_types.hpp:54-59) ------- */
/* Copies doc_len[N] and the flattened posting payload (all inverted_bNNN.bin back to back, or
 * inverted.bin) to HBM through a pinned staging buffer, once; precomputes the per-doc BM25 norm
 * k1*((1-b) + b*(dl/avgdl)) in fp32 with the reference's operation order (src/api_engine.cpp:478).
 * Host buffers stay owned by the caller and may be freed on return. */
int ns_segment_upload(ns_ctx* ctx, uint32_t seg_id, uint32_t n_docs, float avgdl,
                      const uint32_t* doc_len, const void* postings, uint64_t nbytes, ns_seg** out);
int ns_segment_release(ns_ctx* ctx, ns_seg* seg);
/* The same upload for a posting payload that is NOT one host buffer.  The reference keeps a segment's postings in
 * up to 64 inverted_bNNN.bin files and reads them through open streams (include/api_types.hpp:54-59,
 * src/api_segment.cpp:70-102); the host maps those files one after the other and appends each mapping, so the
 * payload never exists in host memory as a whole.  begin: reserves HBM for total_nbytes of postings and takes doc_len;
 * append: the next nbytes of the payload, in payload order (any multiple of 8; copied through the pinned staging
 * buffers before the call returns); end: all bytes must have arrived; publishes the segment under seg_id.
 * ns_segment_release abandons an upload that was begun but not ended. */
int ns_segment_upload_begin(ns_ctx* ctx, uint32_t seg_id, uint32_t n_docs, float avgdl, const uint32_t* doc_len,
                            uint64_t total_nbytes, ns_seg** out);
int ns_segment_upload_append(ns_ctx* ctx, ns_seg* seg, const void* bytes, uint64_t nbytes);
int ns_segment_upload_end(ns_ctx* ctx, ns_seg* seg);

/* Optional second posting stream of a segment (a format loaded NEXT TO the reference's).
 * For every list given here the device stores {u32 docId, f32 term score} per posting, index-aligned with the
 * uploaded {docId, tf} stream, where term score = (idf * (tf * (k1 + 1))) / (tf + k1*((1-b) + b*dl/avgdl)) —
 * src/api_engine.cpp:477-479 evaluated ONCE per posting with the same fp32 operations, instead of once per
 * posting per query.  A batch reads the impact stream when EVERY term ref in it names a registered list with
 * the bit-identical idf (otherwise the whole batch takes the {docId, tf} path); results are bit-identical
 * either way.  Costs 8 B of HBM per posting of the segment.  byte_off/counts as in ns_term_ref; lists must
 * not overlap.  May be called again to add lists or to replace a list's idf. */
int ns_segment_build_impacts(ns_ctx* ctx, ns_seg* seg, const uint64_t* byte_off, const uint32_t* counts,
                             const float* idfs, uint32_t n_lists);
/* on != 0: batches prepared from now on alternate between the ctx's stream and a second one, so that the first work
 * items of batch i+1 fill the wave slots the draining tail of batch i leaves idle (matters most for small batches:
 * a 2048-query shard of a strong-scaled batch).  The alternation applies to the ctx's own stream (a caller who passes
 * streams with ns_ctx_set_stream alternates them itself).  A batch's upload, kernels and result copy all stay on the one
 * stream it was prepared on; with overlap on, the descriptor upload is pulled by a kernel instead of the DMA engine (copies
 * of all streams share one in-order DMA queue, which would chain batch i+1's upload to batch i's result copy). */
int ns_ctx_set_overlap(ns_ctx* ctx, int on);
/* Host threads ns_batch_prepare may use for a large batch (regrouping the term refs, cutting work items, writing the
 * descriptors): 0 = automatic (up to 8, one per ~1500 queries), 1 = the calling thread only.  The prepared batch — every
 * descriptor byte and the launch order — does not depend on this number. */
int ns_ctx_set_host_threads(ns_ctx* ctx, uint32_t n);
/* Compressed, blocked posting stream of a segment, loaded NEXT TO the reference's raw format
 * (src/lexicon.cpp:104-128: {u32 docId, u32 tf} per posting) and built from it on the device, once:
 *   blocks of 256 postings; per block a base docId and a width code; per posting a docId offset of 8, 16 or 32 bits
 *   (frame of reference: whatever the block's doc span needs), tf in 8 bits (255 = escape to the raw stream) and a
 *   16-bit index into the segment's table of DISTINCT BM25 norms — the norm is a function of doc_len alone, so the
 *   index loses nothing; the per-posting fp32 norm stream (4 B) is not read at all.
 * 4 B (dense lists), 5 B or 7 B per posting are read instead of 12; results are bit-identical (same operations on the
 * same values; every test runs both ways).  `found` (src/api_engine.cpp:495) needs every posting visited, so this is
 * compression, not skipping.  The scoring kernel's DRIVER streams read the packed blocks (the bulk of the bytes);
 * foreign windows and doc tiles keep reading the raw stream.  Fails with NS_E_INVAL for a segment with more than
 * 65536 distinct document lengths.  Costs 8 B of HBM per posting (fixed 2 KB stride per block). */
int ns_segment_build_packed(ns_ctx* ctx, ns_seg* seg);
/* mode 0: batches prepared from now on ignore packed streams.  mode 1 (default): a batch whose segments all have one
 * reads docIds and tf from the packed blocks and the norms from the per-posting fp32 norm stream (6-7 B per posting, one
 * memory latency per round).  mode 2: the norms come through the blocks' 16-bit norm index instead (4-5 B per posting, but
 * the table look-up is a second, dependent access per round). */
int ns_ctx_use_packed(ns_ctx* ctx, int mode);
/* on = 0: batches prepared from now on ignore impact streams, and do not share term scores either (ns_ctx_share_scores builds
 * into the same per-segment buffer) (default: on = 1). */
int ns_ctx_use_impacts(ns_ctx* ctx, int on);
/* Skip tables (block metadata next to the reference's raw posting format, src/lexicon.cpp:104-128,
 * which has none: the reference walks every list from its first posting, src/api_engine.cpp:470-481).  For every list
 * given here the device stores, per 1024-doc cell of the segment's doc space, the index of the list's first posting in
 * that cell (4 B per cell and list, built from the uploaded postings on the device).  Term groups that are scored in
 * doc tiles (several frequent lists) then walk those cells and take exactly a list's postings of the cell instead of
 * estimating how many to load and searching the cell's end by docId; every posting is still visited (`found`,
 * src/api_engine.cpp:495) and results are bit-identical either way.  byte_off/counts as in ns_term_ref; a list that
 * is not docId-ascending keeps no table (its groups take the cursor path); lists given again are left as they are.
 * Meant for the frequent lists of a segment (the facade registers lists of >= n_docs / 512 postings at reload). */
int ns_segment_build_skips(ns_ctx* ctx, ns_seg* seg, const uint64_t* byte_off, const uint32_t* counts, uint32_t n_lists);
/* A filtered copy of a segment (csrc/ns_filter.hip).  keep_bits (host, ceil(n_docs / 32) words): bit d % 32 of
 * word d / 32 says whether document d of `src` is kept; bits past n_docs are ignored.  The postings of kept documents, in
 * stream order, become the payload of a NEW segment published under new_seg_id: same n_docs, avgdl and norms as the source,
 * padded like an uploaded one, without packed / impact streams, skip tables or block maxima (ns_segment_build_skips works on
 * it as on any segment), and without any pointer into `src`: the two are released in either order with ns_segment_release.
 * A posting whose docId is >= n_docs is dropped.  The lists [byte_off[i] / 8, + counts[i]) of the source (as in ns_term_ref;
 * they may overlap, leave gaps and come in any order) are answered with their place in the copy: new_byte_off_out[i],
 * new_counts_out[i]; compaction keeps the order, so a docId-ascending list stays one.  A list with no kept posting has
 * count 0.  postings_out (host, may be NULL; capacity: the source's payload bytes): the filtered payload, for tests and
 * tools; the postings do not visit the host otherwise.  kept_postings_out, device_ms_out (may be NULL): postings kept; time
 * of the four passes.  Synchronous.  NS_E_INVAL: a null argument, new_seg_id in use or >= 2^20, a source that is not a
 * published segment of this ctx (an upload that has not ended included), a list outside the source's payload. */
int ns_segment_filter(ns_ctx* ctx, ns_seg* src, uint32_t new_seg_id, const uint32_t* keep_bits, const uint64_t* byte_off,
                      const uint32_t* counts, uint32_t n_lists, uint64_t* new_byte_off_out, uint32_t* new_counts_out,
                      void* postings_out, uint64_t* kept_postings_out, float* device_ms_out, ns_seg** out);
/* A derived segment of copied lists and union lists (csrc/ns_union.hip).  Group g, g < n_groups, names the
 * member lists [group_begin[g], group_begin[g + 1]) of `src`; member i is [member_off[i] / 8, + member_cnt[i]) as in
 * ns_term_ref (members may overlap, repeat and come in any order); n_members = group_begin[n_groups].  The NEW segment,
 * published under new_seg_id, holds one list per group:
 *   one member         the list copied verbatim, a docId >= n_docs included
 *   two or more        the docId-ascending list {d, sum of tf over the member postings that name d} for every d < n_docs that a
 *                      member names with a non-zero sum.  Members are summed as given (a list named twice counts twice), a
 *                      member posting with docId >= n_docs is dropped, the sum is a uint32_t and wraps.
 *   none, or all empty count 0
 * new_byte_off_out[g], new_counts_out[g]: the group's place in the new payload; lists do not overlap and start at multiples
 * of 8.  The segment has the source's n_docs, avgdl and norms, is padded like an uploaded one, has no packed / impact streams,
 * skip tables or block maxima (ns_segment_build_skips works on it as on any segment) and keeps no pointer into `src`: the two
 * are released in either order with ns_segment_release.  postings_out (host, may be NULL; needs n_postings_out): the new
 * payload, for tests and tools; its capacity is the caller's: the single groups' counts plus, per group of two or more,
 * min(sum of member counts, n_docs) postings.  n_postings_out, rounds_out, device_ms_out (may be NULL): postings written;
 * rounds of table scratch the multi groups took (ns_ctx_union_scratch); device time of the call.  Synchronous.  NS_E_INVAL:
 * what ns_segment_filter refuses, a group_begin that is not non-decreasing from 0, postings_out without n_postings_out. */
int ns_segment_union(ns_ctx* ctx, ns_seg* src, uint32_t new_seg_id, const uint64_t* member_off, const uint32_t* member_cnt,
                     const uint32_t* group_begin, uint32_t n_groups, uint64_t* new_byte_off_out, uint32_t* new_counts_out,
                     void* postings_out, uint64_t* n_postings_out, uint32_t* rounds_out, float* device_ms_out, ns_seg** out);
/* Table scratch of ns_segment_union per round, in bytes: one uint32_t[n_docs] table per group of two or more members, as many
 * groups a round as fit, and always at least one.  0: the default, 64 MiB.  NS_E_INVAL above 16 GiB. */
int ns_ctx_union_scratch(ns_ctx* ctx, uint64_t bytes);
/* on = 0: batches prepared from now on ignore skip tables (default: on = 1). */
int ns_ctx_use_skips(ns_ctx* ctx, int on);
/* Block-max scores with `found`-exact pruning.  The reference reads every posting of every scored list
 * (src/api_engine.cpp:470-481) because `found` (:495) is the size of the union of the lists' docs.  For a query whose term
 * group in a segment is ONE list that size needs no reading: it is the number of the list's postings (every posting is a
 * doc of its own), and the group's top-K (:485-492) only needs the blocks whose best score can still enter it.
 * ns_segment_build_blockmax stores, for every list given, per 256 postings of the LIST the largest term score
 * (idf * (tf * (k1 + 1))) / (tf + k1*((1-b) + b*dl/avgdl)) — src/api_engine.cpp:477-479 with the given idf, the same fp32
 * operations as the scoring kernels (4 B per 256 postings, built on the device from the uploaded postings).  With
 * ns_ctx_use_pruning(ctx, 1) (default 0: every posting is read, as the reference does, and that is what bench.py's `value`
 * and `roofline` measure) a single-term group whose list is registered with the bit-identical idf and whose weight is
 * positive visits its blocks in docId order and skips, unread, every block whose maximum times the weight is <= the score
 * of its current K-th best (ties go to the smaller docId, which is already in).  hits, their order, nhits and found are
 * bit-identical to the exhaustive path (tests run both ways).  Multi-term groups are not pruned: their `found` needs the
 * lists merged.  byte_off/counts/idfs as in ns_term_ref; a list given again with another idf is rebuilt. */
int ns_segment_build_blockmax(ns_ctx* ctx, ns_seg* seg, const uint64_t* byte_off, const uint32_t* counts,
                              const float* idfs, uint32_t n_lists);
int ns_ctx_use_pruning(ns_ctx* ctx, int on);
/* on = 0: term groups of exactly two lists take the driver-stream body (table + probes) like every other group instead of
 * the two-list merge body (default: on = 1; both sorted lists advance in lockstep, B's postings find their docs among A's
 * round by a lower bound in LDS: src/api_engine.cpp:449-481 for two lists without a hash table).  Same results. */
int ns_ctx_use_merge(ns_ctx* ctx, int on);
/* Shared term scores.  The reference evaluates the BM25 term score of a posting, src/api_engine.cpp:477-479, once per query
 * that names the posting's list (src/api_engine.cpp:449,464-481: every request walks its lists alone).  The score depends on
 * the list and on the list's idf, not on the query, and a BATCH names the same lists again and again (16384 queries of
 * BASELINE's cfg5 law: ~50 000 term refs, ~40 000 distinct lists, the 32 most frequent ~460 times each).  A sharing batch
 * computes the scores of each DISTINCT list it names once per run — a kernel in front of its scoring kernel, inside
 * ns_batch_run, reading the uploaded {docId, tf} postings and norms and writing {docId, score} (8 B of HBM per posting of
 * the segment, allocated by the first sharing batch) — and its scoring bodies read those.  Nothing is carried from one
 * batch to the next and nothing outlives the run: this is common-subexpression elimination inside one batch, with the
 * reference's operations in the reference's order, and hits, order, nhits, found and score bits are identical (tests run
 * both ways).  mode 1 (default): a batch shares when it scans >= 4 Mi postings and names each distinct posting >= 48 times on
 * average (measured break-even on MI355X: the extra kernel costs ~6 ps per distinct posting, sharing saves ~0.12 ps per use); mode 2: every batch that can (tests); mode 0: never.  A batch never shares when all its segments carry packed
 * streams that it reads (ns_ctx_use_packed 1 or 2), when every list of it has a registered impact stream (it reads those), when a list of it overlaps another
 * list ever shared in the segment, when a segment of it carries an optional impact stream that lacks one of its lists, or
 * when a list's idf differs from the one a live sharing batch uses; it then scores every posting in place, as with mode 0.
 * ns_batch_info reports NS_INFO_SHARED, shared_lists and shared_postings; sum_score_kernel_ms covers both kernels. */
int ns_ctx_share_scores(ns_ctx* ctx, int mode);

/* Shared top rows.  A "thin" (query, segment) group is one hot list H plus tail lists that hold at most 1/32 of its postings.
 * Every doc that no tail holds scores 0.0f + w * s_H(d), whichever query asks, so a sharing batch (ns_ctx_share_scores) ranks
 * H ONCE per cell of its doc space (a power-of-two cut that leaves at most 64 Ki of H's postings per cell): the best 64
 * postings of the cell, one row of a per-batch buffer (64 hits per row; allocated with the batch, nothing is kept between
 * batches or runs).  The thin groups of the batch that name H with the same idf and weight are cut into exactly those cells
 * and scored by a kernel of their own that does not stream H: the tails' docs look H up by docId through its skip table
 * (ns_segment_build_skips), every other candidate comes from the row.  An item whose row cannot prove its top-K (more than
 * 64 - K of the row's docs are docs of the tails, and the row does not hold the whole cell) is scored once more by the
 * streaming body, inside the same launch.  Hits, order, nhits, found and score bits are identical either way.
 * Eligible: OR mode, K <= 32, at most 16 term refs, no negative idf or weight, H has a skip table.  mode 1 (default): H gets
 * rows when at least 4 eligible groups of the batch name it; mode 2: always (tests); mode 0: never.
 * Only a batch that shares its term scores takes rows: one that reads packed blocks (ns_ctx_use_packed) or registered impact
 * streams (ns_segment_build_impacts, complete or not) does not share and takes none.  Under ns_ctx_use_pruning(1) a group of
 * one list is no user of H and takes no row (where H has block maxima the block-max body scores it).  H with one idf under two weights is two
 * keys, each with users and rows of its own; the same list offsets in two segments are two keys as well. */
int ns_ctx_share_rows(ns_ctx* ctx, int mode);
/* out: producer items (rows) and consumer items of the batch as prepared, then, summed over the batch's runs so far (waits
 * for them): consumer items that fell back to the streaming body, row entries that were docs of a tail. */
int ns_batch_row_stats(ns_batch* b, uint32_t out[4]);

/* Class model: which scoring body a (query, segment) group takes.  The density rule sends a group of two or more lists with at
 * least 0.25 postings per doc to the doc-tile body and every other group that no single list dominates to the driver-stream
 * body (or, with two lists, the merge).  mode 1 (the default of a ctx): in a batch large enough to fill the chip, such a group
 * also takes doc tiles when their modelled cost (per 1024-doc tile, per (list, tile) visit, per posting) undercuts the modelled
 * cost of the body it would have, and tile groups are cut and ordered by that model.  mode 0: the density rule alone.  mode 2:
 * the model in every batch, however small (tests, sweeps).  Results are byte-identical in every mode.  NS_CLASS_MODEL in the
 * environment of ns_ctx_create overrides the default. */
int ns_ctx_class_model(ns_ctx* ctx, int mode);
/* out: groups of the batch as prepared that take the driver-stream or merge body, the thin driver-stream body (row consumers
 * included) and the doc-tile body; then how many of the last the class model promoted. */
int ns_batch_class_stats(ns_batch* b, uint32_t out[4]);
/* Sweeps only (tools/class_fit.py): groups of three or more lists that the density rule leaves to the driver-stream body, whose
 * share of postings outside the largest list lies in [share10 / 10, (share10 + 1) / 10) and whose postings per 64 docs lie in
 * [dens64_lo, dens64_hi), take the doc-tile body (body 1) or keep the driver-stream body (body 2), whatever the mode and the
 * size of the batch; body 0 ends the forcing. */
int ns_ctx_class_force(ns_ctx* ctx, uint32_t body, uint32_t share10, uint32_t dens64_lo, uint32_t dens64_hi);

/* ---- one-shot search (host buffers in, host buffers out) ------------------------------------ */
/* hits_out: Q*K entries, query-major, best first: score desc, then seg_id asc, then doc_id asc
 * (the reference leaves ties unspecified: src/api_engine.cpp:485-492); unused tail entries are
 * {-inf, 0xFFFFFFFF, 0xFFFFFFFF}.  nhits_out[Q], found_out[Q] (src/api_engine.cpp:495,505). */
int ns_search_batch(ns_ctx* ctx, const ns_query_desc* queries, const ns_term_ref* terms,
                    uint32_t n_queries, uint32_t k, ns_hit* hits_out, uint32_t* nhits_out,
                    uint64_t* found_out, uint32_t flags);

/* ---- staged search (descriptors resident in HBM; what bench.py times) ----------------------- */
int  ns_batch_prepare(ns_ctx* ctx, const ns_query_desc* queries, const ns_term_ref* terms,
                      uint32_t n_queries, uint32_t k, uint32_t flags, ns_batch** out);
/* Optional: write results into caller-owned DEVICE buffers (e.g. torch tensors that are then
 * all-gathered by RCCL): d_hits Q*K ns_hit, d_nhits Q u32, d_found Q u64.  NULLs restore the
 * batch's own buffers. */
int  ns_batch_bind_outputs(ns_batch* b, void* d_hits, void* d_nhits, void* d_found);
/* Enqueue one pass of the hot path on the ctx stream (asynchronous).  run_flags:
 *   NS_RUN_TIMED  brackets the kernels with HIP events on that stream (read back through ns_batch_get_info after a
 *                 sync or fetch);
 *   NS_RUN_FETCH  also enqueues, right behind the kernels, the copy of the results into pinned host memory and
 *                 records a completion event, so that a later ns_batch_fetch / ns_batch_destroy waits for THIS batch
 *                 only.  That is what lets batches overlap on one ctx:
 *                     prepare(i+1)   host threads regroup and upload while the device scores batch i
 *                     run(i+1, NS_RUN_FETCH)
 *                     fetch(i)       returns as soon as batch i's results have landed
 *                 At most 8 batches may sit between their run and their fetch.  Not for batches with bound outputs. */
#define NS_RUN_TIMED 1
#define NS_RUN_FETCH 2
int  ns_batch_run(ns_batch* b, int run_flags);
/* The hipStream_t this batch's work is enqueued on (the ctx's stream, or its second one under ns_ctx_set_overlap) —
 * for callers that order their own device work behind the batch (bench.py: the RCCL all-gather of a rank's results). */
void* ns_batch_stream(ns_batch* b);
/* Diagnostic for pipelined loops: device time from the end of `prev`'s last kernel to the start of `next`'s first one (both
 * run with NS_RUN_TIMED, both still alive); negative when they overlapped.  NS_E_STATE while `next` has not started. */
int  ns_batch_gap_ms(ns_batch* prev, ns_batch* next, float* ms);
int  ns_batch_sync(ns_batch* b);
int  ns_batch_fetch(ns_batch* b, ns_hit* hits_out, uint32_t* nhits_out, uint64_t* found_out);
int  ns_batch_get_info(ns_batch* b, ns_batch_info* info);
void ns_batch_destroy(ns_batch* b);

/* Semantic query expansion's similarity search: SemanticIndex::most_similar_to_vec,
 * src/semantic_embedding.cpp:104-145.  ns_sem_upload takes the row-major table of L2-normalised fp32 vectors
 * (SemanticIndex::vecs, include/semantic_embedding.hpp:24).  ns_sem_topk: for each of n_q query vectors (host,
 * n_q x dim) the up-to-topk rows with the largest dot product among rows that are not banned for that query
 * (ban_off[n_q + 1] / ban_rows, may be NULL) and have sim >= min_sim — best first, ties to the smaller row;
 * dot products are accumulated in index order in fp32 (the reference's bits).  rows_out / sims_out:
 * n_q x topk (host), counts_out[q] = entries valid for query q.  topk <= 64. */
typedef struct ns_sem ns_sem;
int ns_sem_upload(ns_ctx* ctx, const float* vecs, uint32_t n_rows, uint32_t dim, ns_sem** out);
int ns_sem_release(ns_ctx* ctx, ns_sem* sem);
int ns_sem_topk(ns_ctx* ctx, ns_sem* sem, const float* qvecs, uint32_t n_q, uint32_t topk, float min_sim,
                const uint32_t* ban_off, const uint32_t* ban_rows, uint32_t* rows_out, float* sims_out,
                uint32_t* counts_out, float* device_ms_out);

/* Autocomplete (the reference's AutocompleteIndex, src/api_autocomplete.cpp, behind Engine::suggest): a dictionary of
 * n_terms terms SORTED BY THEIR BYTES (memcmp order; equal terms may repeat), term i = pool[offsets[i] .. offsets[i + 1]),
 * with a u32 score each.  ns_ac_upload copies it to the device and builds the range top-10 tree there; it fails with
 * NS_E_INVAL for unsorted terms, offsets[0] != 0, decreasing offsets, or a pool of 4 GiB or more (offsets[n_terms]).
 * n_terms == 0 is a valid, empty table.
 * ns_ac_suggest: for each of n_q prefixes (host: prefix q = prefix_bytes[prefix_offsets[q] .. prefix_offsets[q + 1]))
 * the L (1..10) best terms that start with it, best first — score descending, then term ascending (== index ascending) —
 * as dictionary indices in idx_out[q * L + r] (host, n_q x L; ~0u past the end) and their number in count_out[q].  The
 * prefix is compared as raw bytes (the caller normalises it); an empty prefix matches every term.  Synchronous; staged
 * through the ctx's pinned buffers.  device_ms_out (may be NULL): the kernel's time.
 * Lifetime: a table belongs to its ctx, like a segment.  Release it with ns_ac_release(ctx, table) before the ctx; a
 * ctx destroyed first frees the tables it still holds, after which their handles are dangling and must not be passed
 * to any call. */
typedef struct ns_ac ns_ac;
int ns_ac_upload(ns_ctx* ctx, const uint8_t* pool, const uint64_t* offsets, const uint32_t* scores, uint32_t n_terms, ns_ac** out);
int ns_ac_suggest(ns_ctx* ctx, ns_ac* ac, const uint8_t* prefix_bytes, const uint32_t* prefix_offsets, uint32_t n_q, uint32_t L,
                  uint32_t* idx_out, uint32_t* count_out, float* device_ms_out);
int ns_ac_release(ns_ctx* ctx, ns_ac* ac);

/* Spelling correction over the same table (csrc/ns_fuzzy.hip): for each query term the L best CANDIDATES
 * within a bounded edit distance.
 *   candidates  the table's entries whose score is not 0 and whose bytes differ from their predecessor's (of a run of equal
 *               strings only the first)
 *   distance    optimal string alignment over bytes (Levenshtein + transposition of two adjacent bytes, no substring
 *               edited twice: d("ab","ba") = 1, d("ca","abc") = 3), at most max_edits[q] (0, 1 or 2; more: NS_E_INVAL)
 *   prefix      with p = min(prefix_len, length of the query term) a candidate shares its first p bytes with the term
 *   order       distance ascending, then score descending, then index ascending: a strict total order, so two calls return
 *               equal bytes
 * ns_ac_build_fuzzy builds the side structures once per table (the candidates ordered by length with a byte-set
 * signature each: 12 B per candidate); it is idempotent, fails with NS_E_INVAL for a table of 2^30 terms or more, and
 * leaves ns_ac_suggest's answers as they were.  *device_ms_out (may be NULL): the kernels' time, 0 when already built.
 * ns_ac_fuzzy: term q = term_bytes[term_offsets[q] .. term_offsets[q + 1]) (host, raw bytes: the caller normalises).  L is
 * clamped to 1..10 and the rows have the clamped width: idx_out[q * L + r] = table index of the r-th answer (~0u past
 * count_out[q]), dist_out[q * L + r] = its distance (0xff past the end).  An empty term or one longer than
 * NS_FUZZY_MAX_LEN bytes gets count 0 and is not sent to the device.  Synchronous; staged through the ctx's pinned
 * buffers.  NS_E_STATE before ns_ac_build_fuzzy.  ns_ac_release frees the side structures with the table. */
#define NS_FUZZY_MAX_LEN   64u
#define NS_FUZZY_MAX_EDITS 2u
int ns_ac_build_fuzzy(ns_ctx* ctx, ns_ac* ac, float* device_ms_out);
int ns_ac_fuzzy(ns_ctx* ctx, ns_ac* ac, const uint8_t* term_bytes, const uint32_t* term_offsets, uint32_t n_q,
                const uint8_t* max_edits, uint32_t prefix_len, uint32_t L, uint32_t* idx_out, uint8_t* dist_out,
                uint32_t* count_out, float* device_ms_out);

/* Typo-tolerant completion over the same table and side structures (csrc/ns_fuzzy.hip): for each prefix that is
 * still being typed the L best candidates that some prefix of which is within a bounded edit distance of it.
 *   distance    the PREFIX distance pd(q, c) = min over 0 <= j <= |c| of osa(q, c[0, j)), osa = ns_ac_fuzzy's optimal string
 *               alignment: pd("cornoa", "coronavirus") = 1, pd("ca", "abc") = 1, pd("abcd", "ab") = 2, pd("abcde", "cdxxx") = 3;
 *               at most max_edits[q] (0, 1 or 2; more: NS_E_INVAL)
 *   candidates  ns_ac_fuzzy's (score not 0; of a run of equal strings only the first), of ANY length from
 *               |q| - max_edits[q] upwards: terms longer than 66 bytes are found as well
 *   prefix      with p = min(prefix_len, |q|) a candidate shares its first p bytes with q exactly; the distance is still taken
 *               over the whole strings
 *   order       distance ascending, then score descending, then index ascending (strict and total: two calls return equal
 *               bytes)
 * With max_edits 0 the answer is the candidates that start with q, best score first; a query of at most max_edits bytes matches
 * every candidate (all of it can be deleted) and gets the table's best L by score.  Arguments, clamping of L, row layout
 * (~0u / 0xff tails), the limits on a query's length (0 or more than NS_FUZZY_MAX_LEN bytes: count 0, never sent), staging and
 * refusals are ns_ac_fuzzy's; NS_E_STATE before ns_ac_build_fuzzy.  ns_ac_suggest's and ns_ac_fuzzy's answers stay as they are. */
int ns_ac_fuzzy_prefix(ns_ctx* ctx, ns_ac* ac, const uint8_t* prefix_bytes, const uint32_t* prefix_offsets, uint32_t n_q,
                       const uint8_t* max_edits, uint32_t prefix_len, uint32_t L, uint32_t* idx_out, uint8_t* dist_out,
                       uint32_t* count_out, float* device_ms_out);

/* Segment-sharded multi-GPU (the alternative to query sharding for an index that outgrows one
 * GPU's HBM): rank r holds a subset of the segments and scores ALL queries over it; the fixed-size per-rank rows
 * are all-gathered rank-major (hits [n_ranks][n_queries][k], nhits and found [n_ranks][n_queries]) and joined here
 * into the one global heap of src/api_engine.cpp:434-435,485-492 (score desc, global seg asc, doc asc; found =
 * sum, :495).  d_seg_map[r * seg_map_stride + local seg id] = the segment's position in the full manifest
 * (NULL: ids are already global).  All pointers are device pointers; asynchronous on the ctx stream. */
int ns_merge_rank_rows(ns_ctx* ctx, const void* d_hits, const void* d_nhits, const void* d_found, uint32_t n_ranks,
                       uint32_t n_queries, uint32_t k, const uint32_t* d_seg_map, uint32_t seg_map_stride,
                       void* d_out_hits, void* d_out_nhits, void* d_out_found);

/* Index inversion (the step before the path): replaces the per-term std::vector<Posting> +
 * std::sort of the reference's `lexicon` tool (src/lexicon.cpp:52-128).
 *   doc_term_counts[d]  number of (termId, tf) pairs of document d (forward.bin's per-document `cnt`, :63)
 *   pairs               the u32 {termId, tf} pairs of all documents back to back, in file order (:66-67)
 *   n_terms             size of the term dictionary; pairs with termId >= n_terms are dropped (:69)
 * Outputs (host memory): df_out[n_terms] = postings per term; postings_out (capacity n_pairs * 8 bytes) receives
 * the {docId, tf} lists in termId order, each sorted by docId (equal docIds keep file order) — i.e. the
 * reference's inverted_bNNN.bin files concatenated in barrel order; *kept_out = number of postings written;
 * device_ms_out (optional) = HIP-event time of the device part, copies excluded. */
int ns_invert_forward(ns_ctx* ctx, const uint32_t* doc_term_counts, uint32_t n_docs, const uint32_t* pairs,
                      uint64_t n_pairs, uint32_t n_terms, uint32_t* df_out, void* postings_out, uint64_t* kept_out,
                      float* device_ms_out);
/* The same inversion, with the result KEPT on the device as a segment's posting stream (build -> serve without the
 * postings crossing PCIe twice): `seg` is an upload in progress — ns_segment_upload_begin(ctx, id, n_docs, avgdl, doc_len,
 * n_pairs * 8, &seg) with nothing appended yet; the call inverts the forward pairs (doc_term_counts has the segment's
 * n_docs entries), leaves the {docId, tf} lists in termId order in the segment (shorter than announced by the dropped
 * pairs: *kept_out postings), and ns_segment_upload_end(ctx, seg) then publishes it.  df_out[n_terms] gives the
 * caller the lexicon: list t starts at byte 8 * sum(df_out[0..t)) and holds df_out[t] postings.  postings_out (may be
 * NULL) additionally receives the lists in host memory, e.g. to write the inverted files. */
int ns_segment_upload_inverted(ns_ctx* ctx, ns_seg* seg, const uint32_t* doc_term_counts, const uint32_t* pairs,
                               uint64_t n_pairs, uint32_t n_terms, uint32_t* df_out, void* postings_out,
                               uint64_t* kept_out, float* device_ms_out);

/* Indexing (csrc/ns_ingest.hip): document texts -> forward index, the step in front of ns_invert_forward.
 * Replaces tokenize + the per-document tf map + the term dictionary of the reference's `forwardindex` tool
 * (include/textutil.hpp:13-37, src/ForwardIndex.cpp:139-179; the same loop in src/AddDocument.cpp:80-130 and
 * src/api_add_document.cpp:252-421).
 *   text, text_bytes   the texts of all documents back to back; any byte may occur, NUL included
 *   offsets[n_docs+1]  document d = text[offsets[d] .. offsets[d + 1]); offsets[0] == 0, non-decreasing,
 *                      offsets[n_docs] <= text_bytes (bytes past it are ignored)
 * Semantics (byte for byte the reference's): a token is a maximal run of [0-9A-Za-z] bytes inside one document,
 * lower-cased; every other byte and every document boundary separates; tokens shorter than 2 bytes and the 24 stop
 * words are dropped (:146-147); doc_len = kept tokens of the document, tf = occurrences of a term in it (:148-149); a
 * document with doc_len == 0 is dropped and the later ones move up (:152-155).  No cap on a token's length.
 * TERM IDS: the reference numbers terms in std::unordered_map iteration order (:159-173), an accident nothing downstream
 * reads.  Here term id = rank of the term's first kept occurrence in the input (document order, then byte position):
 * deterministic and independent of GPU scheduling.  Two different byte strings never share an id (the hash only routes;
 * the bytes are compared).
 * Limits: offsets[n_docs] < 4 GiB - 64 KiB (positions are 32 bits wide); n_docs < 2^32 - 1.  Beyond: NS_E_INVAL (NS_E_ARG).
 * n_docs == 0, or no surviving document, is NS_OK with an empty result (kept_docs == 0).
 * The result stays on the device behind the handle until ns_forward_destroy; sizes come from ns_forward_get_info. */
#define NS_E_ARG NS_E_INVAL
typedef struct ns_forward ns_forward;
typedef struct ns_forward_info {
    uint32_t struct_size;   /* IN: sizeof(ns_forward_info) as the caller was compiled; no more than that many bytes are written */
    uint32_t kept_docs;     /* documents with doc_len > 0 */
    uint32_t n_terms;
    uint32_t n_docs;        /* documents handed in */
    uint64_t n_pairs;       /* (termId, tf) pairs of all kept documents */
    uint64_t term_bytes;    /* bytes of all terms back to back */
    uint64_t n_tokens;      /* tokens before the length and stop-word rules */
    uint64_t kept_tokens;   /* sum of doc_len */
    uint64_t device_bytes;  /* device memory the build used at its peak (scratch + result) */
    float    device_ms;     /* HIP events around the device part (upload excluded) */
    uint32_t pad;
} ns_forward_info;
int ns_forward_build(ns_ctx* ctx, const uint8_t* text, uint64_t text_bytes, const uint64_t* offsets, uint32_t n_docs,
                     ns_forward** out);
/* NS_E_INVAL for a NULL argument or struct_size < 4. */
int ns_forward_get_info(const ns_forward* fwd, ns_forward_info* info);
/* Copies the result to host memory; every pointer may be NULL (that array is skipped); may be called any number of times.
 *   kept_docs_out[kept_docs]   input index of each surviving document, ascending (docId j = kept_docs_out[j])
 *   doc_len_out[kept_docs]     (src/ForwardIndex.cpp:149), counts_out[kept_docs]: pairs of the document (forward.bin's cnt, :218)
 *   pairs_out[2 * n_pairs]     u32 {termId, tf}, documents back to back, termId ascending inside a document (:176, :219-222):
 *                              with counts_out exactly ns_invert_forward's `pairs` and `doc_term_counts`
 *   term_bytes_out[term_bytes], term_offsets_out[n_terms + 1]   term t = bytes [term_offsets_out[t], term_offsets_out[t + 1]) (terms.bin, :225-230)
 * NS_E_STATE if the handle's ctx has been destroyed (the result went with it). */
int ns_forward_fetch(ns_forward* fwd, uint32_t* kept_docs_out, uint32_t* doc_len_out, uint32_t* counts_out,
                     uint32_t* pairs_out, uint8_t* term_bytes_out, uint64_t* term_offsets_out);
/* Lifetime: the ctx keeps a list of its live handles.  ns_ctx_destroy frees their device memory and orphans them; an
 * orphaned handle still answers ns_forward_get_info, fails ns_forward_fetch with NS_E_STATE and is freed by
 * ns_forward_destroy without touching the ctx.  Errors of these three calls are read with ns_last_error(NULL) when the
 * handle has no ctx any more. */
void ns_forward_destroy(ns_forward* fwd);

/* Compaction (csrc/ns_compact.hip): the forward indexes of several segments -> the forward index of ONE
 * segment.  A source is what a segment's docs.bin / forward.bin / terms.bin hold, in host memory: */
typedef struct ns_forward_src {
    uint32_t n_docs;  const uint32_t* doc_len;  const uint32_t* counts;   /* [n_docs]: kept tokens, pairs of each document */
    uint64_t n_pairs; const uint32_t* pairs;                              /* u32 {termId, tf} x n_pairs, file order */
    uint32_t n_terms; const uint8_t* term_bytes; const uint64_t* term_offsets;   /* [n_terms + 1]: term t = term_bytes[term_offsets[t] .. term_offsets[t + 1]) */
} ns_forward_src;
/* The result is an ordinary ns_forward handle: ns_forward_get_info, ns_forward_fetch, ns_forward_destroy and the lifetime
 * rules above apply; kept_docs_out is the identity, n_docs == kept_docs, n_tokens == kept_tokens == the sum of doc_len.
 *   DOCUMENTS  the sources' documents back to back in source order; docId = position.
 *   TERM IDS   walk the sources' term lists in source order, each in its own id order: a byte string gets the next free id
 *              the first time it is seen.  For sources numbered by ns_forward_build's rule this IS "rank of the first kept
 *              occurrence in the concatenated input": merging the segments of batches D1 .. Dn gives the arrays that one
 *              ns_forward_build of D1 + .. + Dn gives.  For sources numbered otherwise (the reference's unordered_map
 *              order) it is still deterministic and independent of GPU scheduling.
 *   PAIRS      termId replaced through that map, then ascending termId inside each document (src/ForwardIndex.cpp:176).
 * Refused with NS_E_INVAL and a message that names the source, nothing left allocated: a termId >= the source's n_terms;
 * the same byte string twice in ONE source's term list (two pairs of a document could collide); counts that do not sum to
 * n_pairs; term offsets that decrease; totals beyond the widths the kernels use — term bytes of all sources below
 * 4 GiB - 64 KiB, pairs below 2^32 - 4096, documents below 2^32 - 1, source terms below 2^31; the totals are checked from
 * the counts and offsets before a byte of payload is read.  n_src == 0, or no document at all: NS_OK, empty result. */
int ns_forward_merge(ns_ctx* ctx, const ns_forward_src* src, uint32_t n_src, ns_forward** out);
/* ns_invert_forward over a handle's pairs and counts where they are, on the device: nothing is uploaded.  df_out[n_terms],
 * postings_out (capacity n_pairs * 8 bytes), kept_out and device_ms_out as there.  NS_E_STATE on an orphaned handle. */
int ns_forward_invert(ns_forward* fwd, uint32_t* df_out, void* postings_out, uint64_t* kept_out, float* device_ms_out);
/* ns_forward_merge sorts the pairs of a document where they lie: up to 64 pairs in one wave's registers, up to
 * ns_compact_doc_cut() pairs in LDS by one workgroup; longer documents go through the global radix sort.  on == 0 sends
 * every document through the radix sort (the A/B baseline; same bytes).  Default: on. */
uint32_t ns_compact_doc_cut(void);
/* The radix sort under ns_invert_forward, ns_forward_build and ns_forward_merge (csrc/ns_invert.hip) sorts keys below
 * key_range in 1 .. 3 passes of 8 .. 11 bits, a function of key_range alone (csrc/ns_radix_plan.hpp).  ns_radix_plan writes
 * the digit of each pass, lowest first, to pbits_out (8 for the passes not used) and returns the number of passes;
 * ns_radix_tile() is the number of items one workgroup of a pass sorts.  Both are for the tests, which build their shapes
 * from them. */
uint32_t ns_radix_plan(uint32_t key_range, uint32_t pbits_out[3]);
uint32_t ns_radix_tile(void);
int ns_ctx_use_docsort(ns_ctx* ctx, int on);

/* Deleting documents (csrc/ns_delete.hip): ns_forward_merge over FILTERED sources.  keep[s] is a bitmap
 * over source s's documents: document d stays iff bit (d & 31) of word (d >> 5) is set; (n_docs + 31) / 32 words are read
 * and the bits at and past n_docs in the last word are ignored.  keep == NULL or keep[s] == NULL: the source passes
 * through unchanged; with every entry NULL the call IS ns_forward_merge, byte for byte and launch for launch.
 * DEFINITION  the result is what ns_forward_merge returns over the filtered sources, and the refusals are the ones it makes
 * over them.  A source with a bitmap is filtered like this: it loses its dropped documents and their pairs; it loses every
 * term that no surviving pair names; the surviving terms keep their relative id order (new id = number of surviving terms
 * with a smaller old id); the surviving pairs are renumbered through that map.  The merge's own rules stay: sources in
 * order, a byte string gets the next free id the first time the walk meets it.  It follows that
 *   - the pairs of dropped documents are not read: an out-of-range termId inside a dropped document is not reported (one
 *     in a surviving pair is, with the smallest such source named, as ns_forward_merge does);
 *   - "the same byte string twice in one source" is refused among the SURVIVING terms only;
 *   - a source whose documents are all dropped contributes nothing, neither documents nor terms;
 *   - when nothing survives anywhere the call returns NS_OK with an empty handle (kept_docs == 0);
 *   - the result is an ordinary ns_forward handle: ns_forward_get_info, ns_forward_fetch, ns_forward_invert,
 *     ns_forward_destroy and the lifetime rules apply unchanged; n_docs == kept_docs == the surviving documents, docId =
 *     position among them;
 *   - the limits and the message style are ns_forward_merge's (messages start with "ns_forward_merge_keep:").  The limits
 *     and the structural checks (counts that sum to n_pairs, term offsets that do not decrease) are applied to the sources
 *     as handed in, before the filter: the counts of dropped documents are needed to find the surviving pairs. */
int ns_forward_merge_keep(ns_ctx* ctx, const ns_forward_src* src, const uint32_t* const* keep, uint32_t n_src, ns_forward** out);

/* "More like this" (csrc/ns_similar.hip): for a batch of documents of ONE segment the most telling terms
 * of each, picked from the document's forward pairs — the step in front of a weighted OR search over those terms.
 * ns_docterms_upload makes a device copy of the segment: the pairs, a document offset array built from src->counts, and
 * df[n_terms] / idf[n_terms] by term id (the caller computes idf on the host: bm25_idf(N, df) with glibc logf, the value
 * search uses; no logf runs on the device).  src->doc_len, term_bytes and term_offsets are not read.  Structural checks
 * and limits are ns_forward_merge's (counts that sum to n_pairs; pairs below 2^32 - 4096, documents below 2^32 - 1, terms
 * below 2^31); a termId >= n_terms is found by a kernel at upload time and refused with NS_E_INVAL, so that selection never
 * indexes df / idf out of range.  An empty source (no document, or documents without pairs) is valid.
 * RULE (host/similar.hpp is the authority): a pair (t, tf) qualifies when tf >= max(min_tf, 1), min_df <= df[t] <= max_df,
 * df[t] >= 1 and 0 < idf[t] < inf.  Its weight is w = (float)tf * idf[t], one fp32 multiply.  The selection is the first
 * T = clamp(max_terms, 1, 32) qualifying pairs by (bit pattern of w descending, termId ascending).
 * ns_docterms_select: host arrays in and out; row i answers doc_ids[i] (the same document may be listed any number of
 * times): term_out[i * T + r], w_out[i * T + r] for r < count_out[i], ~0u and 0.0f past the count.  A doc id >= n_docs
 * returns NS_E_INVAL before anything is launched; n == 0 returns NS_OK.  Synchronous.  device_ms_out (may be NULL): the
 * kernels' time.
 * Lifetime: as ns_forward handles — the ctx keeps a list of its live handles, ns_ctx_destroy frees their device memory and
 * orphans them; an orphaned handle fails ns_docterms_select with NS_E_STATE (message: ns_last_error(NULL)) and is freed by
 * ns_docterms_destroy without touching the ctx. */
typedef struct ns_docterms ns_docterms;
int ns_docterms_upload(ns_ctx* ctx, const ns_forward_src* src, const uint32_t* df, const float* idf, ns_docterms** out);
int ns_docterms_select(ns_docterms* h, const uint32_t* doc_ids, uint32_t n, uint32_t max_terms, uint32_t min_tf, uint32_t min_df,
                       uint32_t max_df, uint32_t* term_out /* n * T */, float* w_out /* n * T */, uint32_t* count_out /* n */,
                       float* device_ms_out);
void ns_docterms_destroy(ns_docterms* h);
/* Documents of at most this many pairs are streamed by one wave, longer ones by a workgroup (the tests' size classes; a
 * document of at most 64 pairs is one chunk of the wave's stream). */
uint32_t ns_docterms_doc_cut(void);
/* Related terms (csrc/ns_terms.hip, csrc/ns_terms_plan.hpp): what a SET of documents is about.  Row i is
 * the documents doc_ids[row_off[i] .. row_off[i + 1]) of the handle's segment; the call sorts them and drops repeats, so a
 * document named twice counts once.  RULE (host/related.hpp is the authority): fg[t] = the row's documents that hold a
 * pair (t, tf) with tf >= max(min_tf, 1); t qualifies when fg[t] >= max(min_docs, 1), min_df <= df[t] <= max_df,
 * df[t] >= 1 and 0 < idf[t] < inf; w = (float)fg[t] * idf[t], one fp32 multiply; the selection is the first
 * T = clamp(max_terms, 1, 64) qualifying terms by (bit pattern of w descending, termId ascending).
 * Outputs: term_out / docs_out (= fg) / w_out [i * T + r] for r < count_out[i], ~0u, 0 and 0.0f past the count;
 * ndocs_out[i] = the distinct documents of row i.  An empty row is valid (count 0).  Synchronous; device_ms_out (may be
 * NULL): the counting kernel's time.  n_rows == 0 returns NS_OK.  NS_E_INVAL with a message, and nothing launched, for a
 * NULL argument, a row_off that does not start at 0 or descends, a doc id >= n_docs and a row of more than
 * ns_docterms_max_row_docs() distinct documents (the device counts in bytes).  The counting needs every document's term
 * ids strictly ascending, the order ns_forward_fetch gives: the first call checks the handle once with a kernel and
 * remembers the answer; a handle that fails is refused here with NS_E_INVAL (ns_docterms_select still answers it).  An
 * orphaned handle returns NS_E_STATE. */
int ns_docterms_aggregate(ns_docterms* h, const uint32_t* doc_ids, const uint64_t* row_off /* n_rows + 1 */, uint32_t n_rows,
                          uint32_t max_terms, uint32_t min_tf, uint32_t min_docs, uint32_t min_df, uint32_t max_df,
                          uint32_t* term_out, uint32_t* docs_out, float* w_out /* n_rows * T each */,
                          uint32_t* count_out, uint32_t* ndocs_out /* n_rows each */, float* device_ms_out);
uint32_t ns_docterms_window(void);          /* term ids per window of the counting kernel's LDS table */
uint32_t ns_docterms_max_row_docs(void);    /* 255 */

/* ---- facet counts (csrc/ns_facet.hip, csrc/ns_facet_plan.hpp) ------------------ */
/* A per-document bucket table on the device, independent of any ns_seg: bucket_of_doc[n_docs], each < n_buckets,
 * 1 <= n_buckets <= 1024.  A bucket id >= n_buckets is found by a kernel at upload and refused with NS_E_INVAL (as
 * ns_docterms_upload does for termIds), nothing left allocated.  Release every table before ns_ctx_destroy. */
typedef struct ns_facet ns_facet;
int ns_facet_upload(ns_ctx* ctx, uint32_t n_docs, const uint16_t* bucket_of_doc, uint32_t n_buckets, ns_facet** out);
int ns_facet_release(ns_ctx* ctx, ns_facet* table);
/* counts_out[q * n_buckets + b] = the number of DISTINCT documents d, summed over the segments, with bucket_of_doc[d] == b,
 * that query q matches.  NS_FLAG_OR: d is in at least one list that the query's refs name in d's segment.  NS_FLAG_AND: d is
 * in every one of them (NS_FLAG_AND's rule for scoring: per segment, over the refs of that segment).  found_out[q] (may be
 * NULL) = the sum over b.  queries / terms are what ns_batch_prepare takes; idf and qweight are ignored: no score is
 * computed and no norm is read.  seg_ids[i] is the id the refs use for segs[i], whose documents tables[i] buckets, i < n_segs;
 * a filtered copy (ns_segment_filter) is an ordinary segment here and takes its source's table.
 * Lists must be docId-ascending (what the index writers produce and ns_segment_filter preserves); a posting whose docId is
 * >= n_docs is not counted.  A ref listed twice in a query counts its documents once.  term_count == 0: a row of zeros.
 * Any term_count works.  Synchronous; device_ms_out (may be NULL) = HIP-event time of the kernels.
 * NS_E_INVAL, with a message and nothing launched: a null argument, a seg_id listed twice, a ref that names a seg_id not
 * listed, a list outside its segment's payload, a table whose n_docs differs from its segment's, tables of different
 * n_buckets, a segment or table of another ctx.  n_queries == 0 is NS_OK. */
int ns_facet_count(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, uint32_t n_terms,
                   uint32_t flags, const uint32_t* seg_ids, ns_seg* const* segs, ns_facet* const* tables, uint32_t n_segs,
                   uint32_t* counts_out /* n_queries * n_buckets */, uint64_t* found_out /* n_queries */, float* device_ms_out);
/* Documents per work item's tile: 131072 in the product library.  The variants and counting builds read the test knob
 * NS_FACET_TILE_DOCS (a power of two, 32 .. 131072) from the environment at every call, so that tile edges can be hit with a
 * few hundred documents; the product library ignores it. */
uint32_t ns_facet_tile_docs(void);

/* ---- search sorted by a per-document key (csrc/ns_sorted.hip, csrc/ns_sorted_plan.hpp) ---- */
/* A per-document uint32 sort key on the device, independent of any ns_seg, like ns_facet: keys[n_docs].  Key 0 means "no key"
 * (an undated article).  The value 0xFFFFFFFF is reserved: a kernel finds it at upload and the call refuses it with
 * NS_E_INVAL, nothing left allocated.  Release every table before ns_ctx_destroy. */
typedef struct ns_dockeys ns_dockeys;
int ns_dockeys_upload(ns_ctx* ctx, uint32_t n_docs, const uint32_t* keys, ns_dockeys** out);
int ns_dockeys_release(ns_ctx* ctx, ns_dockeys* table);
/* direction of ns_search_sorted, or-ed into its flags next to NS_FLAG_OR / NS_FLAG_AND */
#define NS_SORT_DESC    0u       /* larger key first ("newest first") */
#define NS_SORT_ASC     0x1000u  /* smaller non-zero key first ("oldest first") */
/* The first K = clamp(k, 1, NS_MAX_K) documents of each query's matched set in key order, with their BM25 scores.
 *   MATCHED SET  exactly ns_facet_count's.  NS_FLAG_OR: per segment, a document in at least one list the query's refs name
 *                there; NS_FLAG_AND: in every one of them.  Postings with docId >= n_docs are ignored; a list named twice
 *                matches once; term_count == 0 gives nhits = 0, found = 0; any term_count works.  found_out[q] (may be NULL)
 *                is the size of the set summed over the segments: ns_facet_count's found and the scoring path's.
 *   ORDER        one total order, so the answer is unique: (rank key, position of the segment in the call's list ascending,
 *                docId ascending).  NS_SORT_DESC: a larger key first; NS_SORT_ASC: a smaller non-zero key first.  KEY 0 IS
 *                LAST IN BOTH DIRECTIONS.  (One transform gives both: t = key, or t = key ? ~key : 0 under NS_SORT_ASC, larger t
 *                first; that is why 0xFFFFFFFF is reserved.)  The position in seg_ids orders, not the id's value.
 *   HITS         hits_out[q * K + r] = {score, seg_ids[i] of the segment, docId}, keys_out[q * K + r] = the document's key as
 *                uploaded.  nhits_out[q] = min(K, found); the tail past it is {-inf, 0xFFFFFFFF, 0xFFFFFFFF} with key 0.
 *   SCORE        the BM25 score the scoring path gives that document for that query, bit for bit: the accumulator starts at
 *                +0.0f; over the query's refs of the hit's segment IN QUERY ORDER, duplicates included, it adds
 *                qweight * ((idf * (tf * 2.2f)) / (tf + norm[doc])), every operation rounded to fp32, with the segment's
 *                per-document norm and the correctly rounded division.  A ref whose list does not hold the document adds
 *                nothing.  NS_FLAG_AND scores over the same refs.
 * seg_ids[i] is the id the refs use for segs[i], whose documents keys[i] keys, i < n_segs; a filtered copy (ns_segment_filter)
 * is an ordinary segment here: it takes its source's key table and its own norms.  Lists must be docId-ascending; one that is
 * not may lose hits but nothing is read or written out of bounds.  Synchronous; device_ms_out (may be NULL) = HIP-event time
 * of the kernels.  A large batch is cut into sub-batches so that the candidate rows (work items x K x 8 B) never exceed
 * 64 MiB of device memory.
 * NS_E_INVAL, with a message and nothing launched: a null argument, no segment listed, a seg_id listed twice, a ref that names
 * a seg_id not listed, a list outside its segment's payload, a key table whose n_docs differs from its segment's, a segment
 * or table of another ctx, a flag bit other than NS_FLAG_AND and NS_SORT_ASC, a single query whose work items alone exceed
 * the candidate buffer.  n_queries == 0 is NS_OK. */
int ns_search_sorted(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, uint32_t n_terms,
                     uint32_t k, uint32_t flags, const uint32_t* seg_ids, ns_seg* const* segs, ns_dockeys* const* keys, uint32_t n_segs,
                     ns_hit* hits_out /* Q x K */, uint32_t* keys_out /* Q x K */, uint32_t* nhits_out, uint64_t* found_out,
                     float* device_ms_out);
/* HIP-event time of k_sd_select, k_sd_join and k_sd_score, summed over the calling thread's ns_search_sorted calls (and their
 * sub-batches) since the last reset: out3[0..2], milliseconds; reset != 0 zeroes the sums after the read.  For
 * tools/sorted_bench.py. */
int ns_sorted_kernel_ms(float* out3, int reset);

/* ---- boolean queries ----------------------------------------------------------- */
/* role of a term ref in ns_search_boolean: one byte per ref, parallel to the ref array */
#define NS_ROLE_SHOULD 0u   /* optional: adds to the score; matches when the group has no MUST ref */
#define NS_ROLE_MUST   1u   /* required */
#define NS_ROLE_NOT    2u   /* excluded: never scored */
/* The K = clamp(k, 1, NS_MAX_K) best documents of each query's matched set by BM25 score.  roles[r] is the role of terms[r]
 * (roles == NULL: every ref is NS_ROLE_SHOULD, which is the NS_FLAG_OR search).
 *   MATCHED SET  defined per (query, segment) group, over the refs the query has in that segment: M = its MUST refs, S = its
 *                SHOULD refs with count > 0, X = its NOT refs with count > 0.  A MUST ref with count == 0 kills the group (no
 *                document of that segment holds the term).  M not empty: the documents in every list of M and in no list of
 *                X.  M empty, S not: the documents in at least one list of S and in no list of X.  Otherwise nothing: a group
 *                of NOT refs alone matches nothing.  Postings with docId >= n_docs are ignored; a list named twice matches
 *                once; term_count == 0 gives nhits = 0, found = 0; any term_count works.  found_out[q] (may be NULL) is the
 *                size of the set summed over the segments.
 *   SCORE        the scoring path's, bit for bit: the accumulator starts at +0.0f; over the group's refs whose role is not
 *                NS_ROLE_NOT, IN QUERY ORDER, duplicates included, SHOULD refs next to MUST refs, it adds
 *                qweight * ((idf * (tf * 2.2f)) / (tf + norm[doc])), every operation rounded to fp32, with the segment's
 *                per-document norm and the correctly rounded division.  A ref whose list does not hold the document adds
 *                nothing.
 *   ORDER        the search's canonical one: score descending as floats compare, then position of the segment in the call's
 *                list ascending (the position in seg_ids orders, not the id's value), then docId ascending.
 *   HITS         hits_out[q * K + r] = {score, seg_ids[i] of the segment, docId}; nhits_out[q] = min(K, found); the tail past
 *                it is {-inf, 0xFFFFFFFF, 0xFFFFFFFF}.
 *   ODD NUMBERS  a MUST or SHOULD ref whose idf or qweight is NaN or infinite is REFUSED (ns_batch_prepare takes such refs and
 *                leaves the order to the kernels; here the order is a promise).  Negative values and -0.0f are taken: the
 *                accumulator starts at +0.0f and x + y is -0.0f only for x = y = -0.0f, so no score is a negative zero.  The
 *                kernels order by the fp32 bits mapped monotonically (negative: ~bits, else bits | 0x80000000), which is the
 *                order of the floats for every score that is not a NaN; a NaN that finite refs still produce (an overflow to
 *                +inf and one to -inf in one sum, a norm of -tf) sorts by that map: above +inf with its sign bit clear,
 *                below -inf with it set.
 * seg_ids[i] is the id the refs use for segs[i], i < n_segs; a filtered copy (ns_segment_filter) is an ordinary segment here.
 * Lists must be docId-ascending; one that is not may lose hits but nothing is read or written out of bounds.  Synchronous;
 * device_ms_out (may be NULL) = HIP-event time of the kernels.  A large batch is cut into sub-batches so that the candidate
 * rows (work items x K x 8 B) never exceed 64 MiB of device memory, as ns_search_sorted's.
 * NS_E_INVAL, with a message, nothing launched and the output arrays untouched: a null argument, no segment listed, a seg_id
 * listed twice, a ref that names a seg_id not listed, a list outside its segment's payload or at a byte offset that is not a
 * multiple of 8, refs running past n_terms, a role above 2, a non-finite idf or qweight as above, a segment of another ctx,
 * a single query whose work items alone exceed the candidate buffer.  n_queries == 0 is NS_OK. */
int ns_search_boolean(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms,
                      const uint8_t* roles /* n_terms; NULL = all SHOULD */, uint32_t n_terms, uint32_t k, const uint32_t* seg_ids,
                      ns_seg* const* segs, uint32_t n_segs, ns_hit* hits_out /* Q x K */, uint32_t* nhits_out,
                      uint64_t* found_out /* may be NULL */, float* device_ms_out /* may be NULL */);
/* HIP-event time of k_bq_select and k_bq_join, summed over the calling thread's ns_search_boolean calls (and their sub-batches)
 * since the last reset: out2[0..1], milliseconds; reset != 0 zeroes the sums after the read.  For tools/boolean_bench.py. */
int ns_boolean_kernel_ms(float* out2, int reset);

/* ---- pages past the first K (csrc/ns_after_plan.hpp, csrc/ns_after.hip) -------- */
/* A cursor is a position in the total order of a ranked call, not an offset:
 *   ns_search_boolean_after   (ord(score bits) descending, position of the segment in the call's list ascending, docId
 *                             ascending); rank = the fp32 score bits, compared through the kernels' monotone map (negative:
 *                             ~bits, else bits | 0x80000000), so -0.0f is legal, equals no score and sorts just below +0.0f,
 *                             and NaN bits sort as ns_search_boolean says
 *   ns_search_sorted_after    (t descending, position ascending, docId ascending), t = key, or key ? ~key : 0 under
 *                             NS_SORT_ASC; rank = the key as uploaded, the direction is the call's flags
 * seg_id is an id the call lists (its position orders), doc_id any value.  The cursor need not be a matched document, or a
 * document at all.  set == 0: no cursor, the other fields are ignored. */
typedef struct ns_cursor {
    uint32_t rank, seg_id, doc_id, set;
} ns_cursor;
/* ns_search_boolean / ns_search_sorted with one cursor per query (after[n_queries]; NULL = none): the first K documents of the
 * matched set that come STRICTLY AFTER the cursor, scores bit for bit those of the call without one.
 *   found_out[q]  unchanged by a cursor: the size of the matched set.
 *   rest_out[q]   (may be NULL) the number of matched documents strictly after the cursor; nhits_out[q] = min(K, rest); without
 *                 a cursor rest = found.  found - rest is the offset of the page; rest > nhits means there is a next page.
 * Handing the last hit of a page back as the cursor walks the matched set once: nothing repeats, nothing is skipped.  With
 * after == NULL, or every cursor unset, the call is the one without cursors: the same kernels, the same outputs.
 * NS_E_INVAL as the calls without cursors, and, with a message, nothing launched and the output arrays untouched: set > 1, a
 * set cursor whose seg_id the call does not list, for ns_search_sorted_after a set cursor with rank 0xFFFFFFFF.
 * ns_boolean_kernel_ms / ns_sorted_kernel_ms sum these calls' launches too. */
int ns_search_boolean_after(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms,
                            const uint8_t* roles /* n_terms; NULL = all SHOULD */, uint32_t n_terms, uint32_t k,
                            const ns_cursor* after /* n_queries; NULL = none */, const uint32_t* seg_ids, ns_seg* const* segs,
                            uint32_t n_segs, ns_hit* hits_out /* Q x K */, uint32_t* nhits_out, uint64_t* found_out /* may be NULL */,
                            uint64_t* rest_out /* may be NULL */, float* device_ms_out /* may be NULL */);
int ns_search_sorted_after(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms, uint32_t n_terms,
                           uint32_t k, uint32_t flags, const ns_cursor* after /* n_queries; NULL = none */, const uint32_t* seg_ids,
                           ns_seg* const* segs, ns_dockeys* const* keys, uint32_t n_segs, ns_hit* hits_out /* Q x K */,
                           uint32_t* keys_out /* Q x K */, uint32_t* nhits_out, uint64_t* found_out /* may be NULL */,
                           uint64_t* rest_out /* may be NULL */, float* device_ms_out /* may be NULL */);

/* ---- facet counts and date order for boolean queries (csrc/ns_boolean_sets.hip) - */
/* ns_facet_count and ns_search_sorted(_after) over ns_search_boolean's MATCHED SET: roles[r] is the role of terms[r]
 * (roles == NULL: every ref is NS_ROLE_SHOULD, and the answers are those of the calls under NS_FLAG_OR; every ref
 * NS_ROLE_MUST gives those under NS_FLAG_AND).  Nothing else changes:
 *   ns_facet_count_boolean    counts_out[q * n_buckets + b] = distinct matched documents of query q in bucket b, summed over
 *                             the segments; found_out[q] (may be NULL) = the row sum = ns_search_boolean's found.
 *   ns_search_sorted_boolean  the first K = clamp(k, 1, NS_MAX_K) documents of the matched set in ns_search_sorted's total order
 *                             (rank key, position of the segment in the call's list, docId; key 0 last in both directions),
 *                             STRICTLY AFTER the query's cursor where after[q].set == 1 (after == NULL: none), with
 *                             ns_search_sorted_after's found / rest / nhits.  hits_out[..].score is ns_search_boolean's SCORE
 *                             of that document, bit for bit: NOT refs add nothing.  flags: NS_SORT_ASC or 0.
 * Synchronous; device_ms_out (may be NULL) = HIP-event time of the kernels.  NS_E_INVAL, with a message, nothing launched and
 * the output arrays untouched: what ns_facet_count / ns_search_sorted_after refuse (a segment or table of another ctx, a cursor
 * that names a segment the call does not list, a single query whose work items alone exceed the candidate buffer, ...), what
 * ns_search_boolean refuses (a role above NS_ROLE_NOT, a ref past its segment's postings, a non-finite idf or qweight on a MUST
 * or SHOULD ref, ...), and for ns_search_sorted_boolean a flag bit other than NS_SORT_ASC.  n_queries == 0 is NS_OK. */
int ns_facet_count_boolean(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms,
                           const uint8_t* roles /* n_terms; NULL = all SHOULD */, uint32_t n_terms, const uint32_t* seg_ids,
                           ns_seg* const* segs, ns_facet* const* tables, uint32_t n_segs, uint32_t* counts_out /* Q x n_buckets */,
                           uint64_t* found_out /* may be NULL */, float* device_ms_out /* may be NULL */);
int ns_search_sorted_boolean(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms,
                             const uint8_t* roles /* n_terms; NULL = all SHOULD */, uint32_t n_terms, uint32_t k, uint32_t flags,
                             const ns_cursor* after /* n_queries; NULL = none */, const uint32_t* seg_ids, ns_seg* const* segs,
                             ns_dockeys* const* keys, uint32_t n_segs, ns_hit* hits_out /* Q x K */, uint32_t* keys_out /* Q x K */,
                             uint32_t* nhits_out, uint64_t* found_out /* may be NULL */, uint64_t* rest_out /* may be NULL */,
                             float* device_ms_out /* may be NULL */);
/* HIP-event time of k_bs_count, k_bs_select, k_sd_join and k_bs_score, summed over the calling thread's two calls above (and
 * their sub-batches) since the last reset: out4[0..3], milliseconds; reset != 0 zeroes the sums after the read.  For
 * tools/boolean_sets_bench.py. */
int ns_boolean_sets_kernel_ms(float* out4, int reset);

/* ---- any-of groups in boolean queries ------------------------------------------ */
/* One level of grouping, conjunctive normal form: a required clause may be a SET of terms, of which a document must hold at
 * least one:  +(coronavirus covid sars) +(vaccine vaccination) -mouse safety.  Each call is its boolean sibling (ns_search_boolean_after,
 * ns_facet_count_boolean, ns_search_sorted_boolean) with clauses[r] next to roles[r]: the clause of terms[r].
 *   clauses[r]   is read for NS_ROLE_MUST refs only; the values on SHOULD and NOT refs are ignored.  Values need not be dense
 *                or ordered.  Per (query, segment) group the MUST refs with equal value form one clause.
 *   MATCHED SET  refs of a clause with count == 0 are dropped; a clause whose refs ALL have count == 0 kills the group (one-ref
 *                clauses: "a MUST ref with count == 0 kills the group").  S and X as in ns_search_boolean.  At least one
 *                clause: the documents that lie in at least one list of EVERY clause and in no list of X.  No clause, S not
 *                empty: the documents in at least one list of S and in no list of X.  Otherwise nothing.  Postings with
 *                docId >= n_docs are ignored; a list named twice in a clause matches once.
 *   SCORE, ORDER, HITS, cursors, found, rest, ODD NUMBERS: exactly the sibling's.  The score runs over all MUST and SHOULD
 *                refs in query order, duplicates included; a clause member that does not hold the document adds nothing.
 *   clauses == NULL: the call IS its sibling (the same plan, the same kernels, the same bytes out).  Clause values that are all
 *                distinct give the sibling's answers byte for byte, through the grouped kernels.  One clause holding every ref
 *                gives the answers of roles == NULL.
 * Refusals are the siblings'. */
int ns_search_grouped_after(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms,
                            const uint8_t* roles /* n_terms; NULL = all SHOULD */, const uint16_t* clauses /* n_terms; NULL = the sibling */,
                            uint32_t n_terms, uint32_t k, const ns_cursor* after /* n_queries; NULL = none (page 1) */,
                            const uint32_t* seg_ids, ns_seg* const* segs, uint32_t n_segs, ns_hit* hits_out /* Q x K */,
                            uint32_t* nhits_out, uint64_t* found_out /* may be NULL */, uint64_t* rest_out /* may be NULL */,
                            float* device_ms_out /* may be NULL */);
int ns_facet_count_grouped(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms,
                           const uint8_t* roles /* n_terms; NULL = all SHOULD */, const uint16_t* clauses /* n_terms; NULL = the sibling */,
                           uint32_t n_terms, const uint32_t* seg_ids, ns_seg* const* segs, ns_facet* const* tables, uint32_t n_segs,
                           uint32_t* counts_out /* Q x n_buckets */, uint64_t* found_out /* may be NULL */,
                           float* device_ms_out /* may be NULL */);
int ns_search_sorted_grouped(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms,
                             const uint8_t* roles /* n_terms; NULL = all SHOULD */, const uint16_t* clauses /* n_terms; NULL = the sibling */,
                             uint32_t n_terms, uint32_t k, uint32_t flags, const ns_cursor* after /* n_queries; NULL = none */,
                             const uint32_t* seg_ids, ns_seg* const* segs, ns_dockeys* const* keys, uint32_t n_segs,
                             ns_hit* hits_out /* Q x K */, uint32_t* keys_out /* Q x K */, uint32_t* nhits_out,
                             uint64_t* found_out /* may be NULL */, uint64_t* rest_out /* may be NULL */,
                             float* device_ms_out /* may be NULL */);
/* HIP-event time of the launches of the three calls above that were given clauses (with clauses == NULL the siblings' sums
 * count them), summed over the calling thread's calls since the last reset: out6[0..5] = k_bq_select, k_bq_join, k_bs_count,
 * k_bs_select, k_sd_join, k_bs_score, milliseconds; reset != 0 zeroes the sums after the read.  For tools/grouped_bench.py. */
int ns_grouped_kernel_ms(float* out6, int reset);

/* ---- at-least-m-of-n clauses in boolean queries -------------------------------- */
/* "At least two of these four":  +(fever cough dyspnea fatigue)~2.  Each call is its grouped sibling with needs[r] behind
 * clauses[r]: how many DISTINCT lists of the clause of terms[r] a document must lie in.
 *   needs[r]     is read for NS_ROLE_MUST refs only.  0 reads as 1.  A value above 7 is refused.  The refs of one clause in one
 *                (query, segment) group must carry the same need; needs with clauses == NULL are refused.
 *   MATCHED SET  a clause with need m holds for a document that lies in at least m distinct lists of the clause.  Refs with
 *                count == 0 are dropped.  A list named twice in a clause (the same byte_off and count) counts once.  A clause
 *                with fewer than m distinct lists left kills the group (m = 1: the sibling's rule).  Everything else is the
 *                sibling's: every clause must hold, no NOT list may, postings with docId >= n_docs are ignored.
 *   SCORE, ORDER, HITS, cursors, found, rest, ODD NUMBERS: exactly the sibling's.
 *   needs == NULL: the call IS its grouped sibling (the same plan, the same kernels, the same bytes out).  Needs that are all 1
 *                give the sibling's answers byte for byte, through the quorum kernels.  A clause of n distinct lists with
 *                postings and need n gives the answers of n one-term clauses.
 * "At least m of the optional terms" is one required clause holding those terms: MUST and SHOULD refs score alike.
 * Refusals are the siblings', and the three above. */
int ns_search_quorum_after(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms,
                           const uint8_t* roles /* n_terms; NULL = all SHOULD */, const uint16_t* clauses /* n_terms; NULL = the boolean call */,
                           const uint8_t* needs /* n_terms; NULL = the sibling */, uint32_t n_terms, uint32_t k,
                           const ns_cursor* after /* n_queries; NULL = none (page 1) */, const uint32_t* seg_ids, ns_seg* const* segs,
                           uint32_t n_segs, ns_hit* hits_out /* Q x K */, uint32_t* nhits_out, uint64_t* found_out /* may be NULL */,
                           uint64_t* rest_out /* may be NULL */, float* device_ms_out /* may be NULL */);
int ns_facet_count_quorum(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms,
                          const uint8_t* roles /* n_terms; NULL = all SHOULD */, const uint16_t* clauses /* n_terms; NULL = the boolean call */,
                          const uint8_t* needs /* n_terms; NULL = the sibling */, uint32_t n_terms, const uint32_t* seg_ids,
                          ns_seg* const* segs, ns_facet* const* tables, uint32_t n_segs, uint32_t* counts_out /* Q x n_buckets */,
                          uint64_t* found_out /* may be NULL */, float* device_ms_out /* may be NULL */);
int ns_search_sorted_quorum(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms,
                            const uint8_t* roles /* n_terms; NULL = all SHOULD */, const uint16_t* clauses /* n_terms; NULL = the boolean call */,
                            const uint8_t* needs /* n_terms; NULL = the sibling */, uint32_t n_terms, uint32_t k, uint32_t flags,
                            const ns_cursor* after /* n_queries; NULL = none */, const uint32_t* seg_ids, ns_seg* const* segs,
                            ns_dockeys* const* keys, uint32_t n_segs, ns_hit* hits_out /* Q x K */, uint32_t* keys_out /* Q x K */,
                            uint32_t* nhits_out, uint64_t* found_out /* may be NULL */, uint64_t* rest_out /* may be NULL */,
                            float* device_ms_out /* may be NULL */);
/* HIP-event time of the launches of the three calls above that were given needs (with needs == NULL the siblings' sums count
 * them), summed over the calling thread's calls since the last reset: out6[0..5] as ns_grouped_kernel_ms. */
int ns_quorum_kernel_ms(float* out6, int reset);

/* ---- per-document boost factors in ranked boolean search ------------------------ */
/* A table of one fp32 factor per document, on the device, independent of any ns_seg and indexed by docId (so it serves a filter's
 * copy of the segment unchanged), as ns_dockeys is.  A factor that is not finite or has its sign bit set (-0.0f included) is
 * refused with NS_E_INVAL by a check on the device, and nothing stays allocated; 0.0f is legal. */
typedef struct ns_docboost ns_docboost;
int ns_docboost_upload(ns_ctx* ctx, uint32_t n_docs, const float* boost, ns_docboost** out);
int ns_docboost_release(ns_ctx* ctx, ns_docboost* table);
/* ns_search_quorum_after, parameter for parameter, with one table per listed segment behind `segs`.
 *   MATCHED SET, found, rest, ORDER, HITS, cursors, refusals: the sibling's.
 *   SCORE        fp32(score * boosts[i][docId]): ONE rounded multiply of the sibling's finished sum.  The product's bits are the
 *                rank (a negative score times 0.0f is -0.0f, which ranks just below +0.0f); a hit's score and a cursor's rank
 *                are those bits.
 *   boosts == NULL: the call IS the sibling (the same plan, the same kernels, the same bytes out).  Tables that are all 1.0f give
 *                the sibling's answers byte for byte, through the boosted kernels.
 *   A NULL entry, a table of another ctx or a table shorter than its segment's n_docs: NS_E_INVAL.
 * roles / clauses / needs == NULL mean what they mean in the sibling, so plain OR and AND search (every ref SHOULD, every ref
 * MUST) get factors through this call too. */
int ns_search_boosted_after(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms,
                            const uint8_t* roles /* n_terms; NULL = all SHOULD */, const uint16_t* clauses /* n_terms; NULL = the boolean call */,
                            const uint8_t* needs /* n_terms; NULL = the grouped call */, uint32_t n_terms, uint32_t k,
                            const ns_cursor* after /* n_queries; NULL = none (page 1) */, const uint32_t* seg_ids, ns_seg* const* segs,
                            ns_docboost* const* boosts /* n_segs; NULL = the sibling */, uint32_t n_segs, ns_hit* hits_out /* Q x K */,
                            uint32_t* nhits_out, uint64_t* found_out /* may be NULL */, uint64_t* rest_out /* may be NULL */,
                            float* device_ms_out /* may be NULL */);
/* HIP-event time of the launches of ns_search_boosted_after calls that were given tables (with boosts == NULL the sibling's sums
 * count them), summed over the calling thread's calls since the last reset: out2[0..1] = k_bq_select, k_bq_join, milliseconds. */
int ns_boosted_kernel_ms(float* out2, int reset);

/* ---- one hit per group: ranked hits collapsed by a per-document key ------------ */
/* ns_search_boosted_after without a cursor, plus one group table per listed segment: an ns_dockeys table as ns_dockeys_upload
 * makes it, indexed by docId (so it serves a filter's copy of the segment unchanged).
 *   KEYS         0 keeps its meaning, "no key": the document stands alone and is never collapsed with anything, not even with
 *                other key-0 documents.  Any other key names a group; the keys of one call are ONE key space, so equal keys in
 *                different segments are the same group.  0xFFFFFFFF stays refused by the upload.
 *   HITS         Take the sibling's matched set in its one total order: ord(bits of fp32(score * factor)) descending, then the
 *                position of the segment in the call's list, then docId.  Delete every document that has an earlier document of
 *                the same non-zero key.  The first K = clamp(k, 1, NS_MAX_K) of what remains are the hits: each is its group's
 *                first member in the uncollapsed order and carries that document's score bits, segment and docId exactly as the
 *                sibling reports them.
 *   nhits[q]     min(K, distinct non-zero keys in the matched set + matched key-0 documents); the tail is padded as the sibling's.
 *   found[q]     the size of the matched set in documents: the sibling's value.
 *   groups_out   [q * K + r] the hit's key as uploaded (0 for a stand-alone hit, 0 in the padded tail).
 *   others_out   [q * K + r] the matched documents of the whole call that carry the hit's key, minus one; 0 for key 0 and in the
 *                tail.  Documents a NOT ref or a filter removed are not matched and not counted.  NULL skips that pass entirely.
 *   Tables that are all 0, and tables in which every document has a key of its own, give ns_search_boosted_after(after = NULL)'s
 *   hits, nhits and found byte for byte, through the collapsing kernels.  One key on every document gives one hit per query, the
 *   sibling's first, with others = found - 1.
 *   boosts / roles / clauses / needs == NULL mean what they mean in the sibling.
 *   Refusals (NS_E_INVAL, nothing launched): the sibling's, and a NULL group table, a table of another ctx, a table whose n_docs
 *   differs from its segment's.
 * There is no cursor: a document behind a cursor represents its group only if no member lies in front of the cursor, which a
 * cursor over tile-local rows cannot know.  The first K <= NS_MAX_K groups are what the call answers. */
int ns_search_collapsed(ns_ctx* ctx, const ns_query_desc* queries, uint32_t n_queries, const ns_term_ref* terms,
                        const uint8_t* roles /* n_terms; NULL = all SHOULD */, const uint16_t* clauses /* n_terms; NULL = the boolean call */,
                        const uint8_t* needs /* n_terms; NULL = the grouped call */, uint32_t n_terms, uint32_t k,
                        const uint32_t* seg_ids, ns_seg* const* segs, ns_docboost* const* boosts /* n_segs; NULL = none */,
                        ns_dockeys* const* groups /* n_segs */, uint32_t n_segs, ns_hit* hits_out /* Q x K */,
                        uint32_t* groups_out /* Q x K */, uint32_t* others_out /* Q x K; may be NULL */, uint32_t* nhits_out,
                        uint64_t* found_out /* may be NULL */, float* device_ms_out /* may be NULL */);
/* HIP-event time of the launches of ns_search_collapsed, summed over the calling thread's calls since the last reset:
 * out3[0..2] = k_bq_select, k_bq_join_collapsed, k_cl_count (0 while no call asked for others), milliseconds. */
int ns_collapsed_kernel_ms(float* out3, int reset);

/* ---- tuning knobs (per ctx; 0 = library default) --------------------------------------------- */
/* variant: 0 = the product's one scoring launch, k_uscore — every work item picks the driver-stream body, the doc-tile body
 * or (ns_ctx_use_pruning) the block-max body; term groups of more than 64 terms fall back to the workgroup-tile kernel
 * k_score.  libnextsearch_hip.so accepts variant 0 only.  The forced variants — 12..17 = the driver-stream body as a kernel
 * of its own for every group (other table / foreign-budget sizes), 18..20 = the doc-tile body for every group (512 / 1024 /
 * 2048-doc tiles), 1..4 = k_score for every group (four tile sizes) — are test and sweep infrastructure and exist in
 * libnextsearch_hip_variants.so (`make -C nextsearch-api_amd variants`); 5..11 were retired in round 2 and are rejected by
 * both builds.  min_items: number of work items below which groups are additionally split across doc ranges.
 * split_postings: a (query, segment) group is split into doc ranges of about this much estimated work (variant 0: units of
 * one streamed posting, default 98304 for K <= 32 and 131072 above; forced variants: postings). */
int  ns_set_tuning(ns_ctx* ctx, uint32_t variant, uint32_t min_items, uint32_t split_postings);

#ifdef __cplusplus
}
#endif
#endif /* NEXTSEARCH_HIP_H */
