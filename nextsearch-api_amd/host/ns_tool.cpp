// ns_tool — small CLI over the host facade.
//   ns_tool gen-index <index_dir> <n_segments> <docs_per_segment> [vocab=65536] [seed=1337] [--legacy]
//   ns_tool search <index_dir> <k> <query text ...>        (needs an MI355X; prints the /api/search JSON body)
//   ns_tool index <segment_dir> <documents_file> [device=0]  (needs an MI355X)
//        documents_file: u32 n, then n x {string cord_uid, string title, string json_relpath, string text} with
//        string = u32 length + bytes (include/indexio.hpp:18-29).  Runs the reference's two offline steps on the device:
//        `forwardindex` from the extracted text onwards (forward_index.hpp) and `lexicon` (invert.hpp).  One JSON line.
//   ns_tool compact <index_dir> [first count]             (needs an MI355X)
//        Engine::compact: the manifest's segments [first, first + count) (default: all) become one (compact.hpp).  One JSON line.
//   ns_tool delete <index_dir> <uid>...                   (needs an MI355X)
//        Engine::delete_documents: every document that carries one of the uids goes; the segments that lose documents are
//        rewritten on the device (purge.hpp).  One JSON line.
//   ns_tool similar <index_dir> <uid> [k=10]               (needs an MI355X)
//        Engine::more_like_this: the documents most like the one that carries the uid (similar.hpp); prints the JSON body.
//   ns_tool search-filtered <index_dir> <from> <to> <k> <query text ...>   (needs an MI355X)
//        Engine::search_filtered: the search restricted to the documents dated from..to (YYYY, YYYY-MM or YYYY-MM-DD; "" or
//        "-" leaves a bound open); prints search's JSON body plus the "filter" member (filter.hpp).
//   ns_tool search-faceted <index_dir> <year|month> <from> <to> <k> <query text ...>   (needs an MI355X)
//        Engine::search_faceted: search's JSON body plus "facets": the matched documents per year (month) of publish_time
//        (facet.hpp).  from / to as search-filtered's; "-" "-" searches the whole index, without a "filter" member.
//   ns_tool search-sorted <index_dir> <newest|oldest> <from> <to> <k> <query text ...>   (needs an MI355X)
//        Engine::search_sorted: search's JSON body with "results" in date order (publish_time; undated documents last in both
//        directions) plus "sort" (sorted.hpp).  from / to as search-filtered's; "-" "-" searches the whole index.
//   ns_tool search-boolean <index_dir> <from> <to> <k> <query words ...>   (needs an MI355X)
//        Engine::search_boolean: `+word` must be held, `-word` must not, other words are optional (boolean.hpp); search's JSON
//        body plus "boolean".  from / to as search-filtered's; "-" "-" searches the whole index.
//   ns_tool search-boolean-faceted <index_dir> <year|month> <from> <to> <k> <query words ...>   (needs an MI355X)
//        Engine::search_boolean_faceted: search-boolean's JSON body plus "facets", as search-faceted's.
//   ns_tool search-boolean-sorted <index_dir> <newest|oldest> <from> <to> <k> <query words ...>   (needs an MI355X)
//        Engine::search_boolean_sorted: search-boolean's JSON body with "results" in date order plus "sort", as search-sorted's.
//   ns_tool search-grouped <index_dir> <from> <to> <k> <query words ...>                          (needs an MI355X; `+(a b) +c -d`)
//   ns_tool search-grouped-faceted <index_dir> <year|month> <from> <to> <k> <query words ...>     (needs an MI355X)
//   ns_tool search-grouped-sorted <index_dir> <newest|oldest> <from> <to> <k> <query words ...>   (needs an MI355X)
//   ns_tool search-quorum <index_dir> <from> <to> <k> <query words ...>                           (needs an MI355X; `+(a b c)~2 -d`, `a b c ~2`)
//   ns_tool search-quorum-faceted <index_dir> <year|month> <from> <to> <k> <query words ...>      (needs an MI355X)
//   ns_tool search-quorum-sorted <index_dir> <newest|oldest> <from> <to> <k> <query words ...>    (needs an MI355X)
//        Engine::search_quorum, search_quorum_faceted, search_quorum_sorted: the grouped bodies with "quorum" in place of "grouped".
//        The page modes quorum, quorum-newest and quorum-oldest page them.
//   ns_tool search-boosted <index_dir> <none|exponential|linear> <weight> <scale_days> <offset_days> <origin|-> <from> <to> <k> <query words ...>   (needs an MI355X; `+(a b)^0.5 c^2.5`)
//        Engine::search_boosted: search-quorum's body with "boosted" in place of "quorum" and, unless the decay is none, "boost";
//        relevance times a recency factor per document (host/boost.hpp); undated documents keep their score.
//   ns_tool search-collapsed <index_dir> <title|author> <from> <to> <k> <query words ...>   (needs an MI355X)
//        Engine::search_collapsed: search-boosted's body (decay none) with one hit per title or author, "collapsed" in place of
//        "boosted", "collapse": {"field"} and "others": n in every result.  from / to as search-filtered's.
//   ns_tool page <index_dir> <or|and|boolean|newest|oldest|boolean-newest|boolean-oldest|grouped|grouped-newest|grouped-oldest|quorum|quorum-newest|quorum-oldest> <from> <to> <k> <cursor|-> <query words ...>   (needs an MI355X)
//        Engine::search_page: one page of that mode's result, its JSON body plus "page": {"cursor", "next", "offset",
//        "remaining"} (page.hpp).  cursor: "-" for the first page, else a page's "next".  from / to as search-filtered's.
//   ns_tool facade-bench <index_dir> <queries.txt> <k> [reps=5] [device=0]
//        times the C++ facade from INSIDE the process (no ctypes, no Python): query preparation alone (tokenise,
//        dictionary probes, idf: src/api_engine.cpp:388-397,:454-461) and Engine::search_batch_flat, query TEXT in ->
//        hits in host memory out.  device < 0: query preparation only (runs without a GPU).  One JSON line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <chrono>
#include <fstream>
#include <vector>
#include <algorithm>

#include "engine.hpp"
#include "gen_index.hpp"
#include "invert.hpp"

// search-boolean*, search-grouped*, search-quorum*: the dialect the subcommand names
static nsx::Dialect tool_dialect(const char* subcommand) {
    return subcommand[7] == 'q' ? nsx::Dialect::Quorum : subcommand[7] == 'g' ? nsx::Dialect::Grouped : nsx::Dialect::Boolean;
}

int main(int argc, char** argv) {
    if (argc >= 5 && std::strcmp(argv[1], "gen-index") == 0) {
        nsx::GenParams p;
        p.index_dir = argv[2];
        p.n_segments = (uint32_t)std::strtoul(argv[3], nullptr, 10);
        p.docs_per_segment = (uint32_t)std::strtoul(argv[4], nullptr, 10);
        int pos = 0;
        for (int i = 5; i < argc; i++) {
            if (std::strcmp(argv[i], "--legacy") == 0) { p.legacy_layout = true; continue; }
            if (pos == 0) p.vocab = (uint32_t)std::strtoul(argv[i], nullptr, 10);
            if (pos == 1) p.seed = std::strtoull(argv[i], nullptr, 10);
            pos++;
        }
        nsx::GenStats st = nsx::generate_index(p);
        std::printf("{\"postings\": %llu, \"bytes\": %llu}\n", (unsigned long long)st.total_postings, (unsigned long long)st.total_bytes);
        return 0;
    }
    if (argc >= 5 && std::strcmp(argv[1], "search") == 0) {
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        int k = std::atoi(argv[3]);
        std::string q;
        for (int i = 4; i < argc; i++) { if (i > 4) q.push_back(' '); q += argv[i]; }
        std::printf("%s\n", eng.search(q, k).c_str());
        return 0;
    }
    if (argc >= 7 && std::strcmp(argv[1], "search-filtered") == 0) {
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        nsx::DocFilter f;
        if (std::strcmp(argv[3], "-") != 0) f.date_from = argv[3];
        if (std::strcmp(argv[4], "-") != 0) f.date_to = argv[4];
        const int k = std::atoi(argv[5]);
        std::string q, body;
        for (int i = 6; i < argc; i++) { if (i > 6) q.push_back(' '); q += argv[i]; }
        if (!eng.search_filtered_text(q, k, f, body)) { std::fprintf(stderr, "search-filtered failed: %s\n", body.c_str()); return 1; }
        std::printf("%s\n", body.c_str());
        return 0;
    }
    if (argc >= 8 && std::strcmp(argv[1], "search-faceted") == 0) {
        nsx::FacetSpec spec;
        if (std::strcmp(argv[3], "year") == 0) spec.kind = nsx::FacetSpec::Year;
        else if (std::strcmp(argv[3], "month") == 0) spec.kind = nsx::FacetSpec::Month;
        else { std::fprintf(stderr, "search-faceted: the facet is year or month, not %s\n", argv[3]); return 2; }
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        nsx::DocFilter f;
        const bool filtered = std::strcmp(argv[4], "-") != 0 || std::strcmp(argv[5], "-") != 0;
        if (std::strcmp(argv[4], "-") != 0) f.date_from = argv[4];
        if (std::strcmp(argv[5], "-") != 0) f.date_to = argv[5];
        const int k = std::atoi(argv[6]);
        std::string q, body;
        for (int i = 7; i < argc; i++) { if (i > 7) q.push_back(' '); q += argv[i]; }
        if (!eng.search_faceted_text(q, k, spec, filtered ? &f : nullptr, body)) { std::fprintf(stderr, "search-faceted failed: %s\n", body.c_str()); return 1; }
        std::printf("%s\n", body.c_str());
        return 0;
    }
    if (argc >= 8 && std::strcmp(argv[1], "search-sorted") == 0) {
        nsx::SortSpec spec;
        if (std::strcmp(argv[3], "newest") == 0) spec.ascending = false;
        else if (std::strcmp(argv[3], "oldest") == 0) spec.ascending = true;
        else { std::fprintf(stderr, "search-sorted: the order is newest or oldest, not %s\n", argv[3]); return 2; }
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        nsx::DocFilter f;
        const bool filtered = std::strcmp(argv[4], "-") != 0 || std::strcmp(argv[5], "-") != 0;
        if (std::strcmp(argv[4], "-") != 0) f.date_from = argv[4];
        if (std::strcmp(argv[5], "-") != 0) f.date_to = argv[5];
        const int k = std::atoi(argv[6]);
        std::string q, body;
        for (int i = 7; i < argc; i++) { if (i > 7) q.push_back(' '); q += argv[i]; }
        if (!eng.search_sorted_text(q, k, spec, filtered ? &f : nullptr, body)) { std::fprintf(stderr, "search-sorted failed: %s\n", body.c_str()); return 1; }
        std::printf("%s\n", body.c_str());
        return 0;
    }
    if (argc >= 7 && (std::strcmp(argv[1], "search-boolean") == 0 || std::strcmp(argv[1], "search-grouped") == 0 || std::strcmp(argv[1], "search-quorum") == 0)) {
        const nsx::Dialect dialect = tool_dialect(argv[1]);
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        nsx::DocFilter f;
        const bool filtered = std::strcmp(argv[3], "-") != 0 || std::strcmp(argv[4], "-") != 0;
        if (std::strcmp(argv[3], "-") != 0) f.date_from = argv[3];
        if (std::strcmp(argv[4], "-") != 0) f.date_to = argv[4];
        const int k = std::atoi(argv[5]);
        std::string q, body;
        for (int i = 6; i < argc; i++) { if (i > 6) q.push_back(' '); q += argv[i]; }
        if (!eng.search_dialect_text(dialect, q, k, filtered ? &f : nullptr, body)) { std::fprintf(stderr, "%s failed: %s\n", argv[1], body.c_str()); return 1; }
        std::printf("%s\n", body.c_str());
        return 0;
    }
    if (argc >= 12 && std::strcmp(argv[1], "search-boosted") == 0) {
        nsx::BoostSpec spec;
        const bool boosted = std::strcmp(argv[3], "none") != 0;
        if (std::strcmp(argv[3], "exponential") == 0) spec.kind = nsx::BoostSpec::Exponential;
        else if (std::strcmp(argv[3], "linear") == 0) spec.kind = nsx::BoostSpec::Linear;
        else if (boosted) { std::fprintf(stderr, "search-boosted: the decay is none, exponential or linear, not %s\n", argv[3]); return 2; }
        spec.weight = std::atof(argv[4]);
        spec.scale_days = std::atof(argv[5]);
        spec.offset_days = std::atof(argv[6]);
        if (std::strcmp(argv[7], "-") != 0) spec.origin = argv[7];
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        nsx::DocFilter f;
        const bool filtered = std::strcmp(argv[8], "-") != 0 || std::strcmp(argv[9], "-") != 0;
        if (std::strcmp(argv[8], "-") != 0) f.date_from = argv[8];
        if (std::strcmp(argv[9], "-") != 0) f.date_to = argv[9];
        const int k = std::atoi(argv[10]);
        std::string q, body;
        for (int i = 11; i < argc; i++) { if (i > 11) q.push_back(' '); q += argv[i]; }
        if (!eng.search_boosted_text(q, k, boosted ? &spec : nullptr, filtered ? &f : nullptr, body)) { std::fprintf(stderr, "search-boosted failed: %s\n", body.c_str()); return 1; }
        std::printf("%s\n", body.c_str());
        return 0;
    }
    if (argc >= 8 && std::strcmp(argv[1], "search-collapsed") == 0) {
        nsx::CollapseSpec spec;
        if (std::strcmp(argv[3], "title") == 0) spec.kind = nsx::CollapseSpec::Title;
        else if (std::strcmp(argv[3], "author") == 0) spec.kind = nsx::CollapseSpec::Author;
        else { std::fprintf(stderr, "search-collapsed: the field is title or author, not %s\n", argv[3]); return 2; }
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        nsx::DocFilter f;
        const bool filtered = std::strcmp(argv[4], "-") != 0 || std::strcmp(argv[5], "-") != 0;
        if (std::strcmp(argv[4], "-") != 0) f.date_from = argv[4];
        if (std::strcmp(argv[5], "-") != 0) f.date_to = argv[5];
        const int k = std::atoi(argv[6]);
        std::string q, body;
        for (int i = 7; i < argc; i++) { if (i > 7) q.push_back(' '); q += argv[i]; }
        if (!eng.search_collapsed_text(q, k, spec, nullptr, filtered ? &f : nullptr, body)) { std::fprintf(stderr, "search-collapsed failed: %s\n", body.c_str()); return 1; }
        std::printf("%s\n", body.c_str());
        return 0;
    }
    if (argc >= 8 && (std::strcmp(argv[1], "search-boolean-faceted") == 0 || std::strcmp(argv[1], "search-grouped-faceted") == 0 || std::strcmp(argv[1], "search-quorum-faceted") == 0)) {
        const nsx::Dialect dialect = tool_dialect(argv[1]);
        nsx::FacetSpec spec;
        if (std::strcmp(argv[3], "year") == 0) spec.kind = nsx::FacetSpec::Year;
        else if (std::strcmp(argv[3], "month") == 0) spec.kind = nsx::FacetSpec::Month;
        else { std::fprintf(stderr, "%s: the facet is year or month, not %s\n", argv[1], argv[3]); return 2; }
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        nsx::DocFilter f;
        const bool filtered = std::strcmp(argv[4], "-") != 0 || std::strcmp(argv[5], "-") != 0;
        if (std::strcmp(argv[4], "-") != 0) f.date_from = argv[4];
        if (std::strcmp(argv[5], "-") != 0) f.date_to = argv[5];
        const int k = std::atoi(argv[6]);
        std::string q, body;
        for (int i = 7; i < argc; i++) { if (i > 7) q.push_back(' '); q += argv[i]; }
        if (!eng.search_dialect_faceted_text(dialect, q, k, spec, filtered ? &f : nullptr, body)) { std::fprintf(stderr, "%s failed: %s\n", argv[1], body.c_str()); return 1; }
        std::printf("%s\n", body.c_str());
        return 0;
    }
    if (argc >= 8 && (std::strcmp(argv[1], "search-boolean-sorted") == 0 || std::strcmp(argv[1], "search-grouped-sorted") == 0 || std::strcmp(argv[1], "search-quorum-sorted") == 0)) {
        const nsx::Dialect dialect = tool_dialect(argv[1]);
        nsx::SortSpec spec;
        if (std::strcmp(argv[3], "newest") == 0) spec.ascending = false;
        else if (std::strcmp(argv[3], "oldest") == 0) spec.ascending = true;
        else { std::fprintf(stderr, "%s: the order is newest or oldest, not %s\n", argv[1], argv[3]); return 2; }
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        nsx::DocFilter f;
        const bool filtered = std::strcmp(argv[4], "-") != 0 || std::strcmp(argv[5], "-") != 0;
        if (std::strcmp(argv[4], "-") != 0) f.date_from = argv[4];
        if (std::strcmp(argv[5], "-") != 0) f.date_to = argv[5];
        const int k = std::atoi(argv[6]);
        std::string q, body;
        for (int i = 7; i < argc; i++) { if (i > 7) q.push_back(' '); q += argv[i]; }
        if (!eng.search_dialect_sorted_text(dialect, q, k, spec, filtered ? &f : nullptr, body)) { std::fprintf(stderr, "%s failed: %s\n", argv[1], body.c_str()); return 1; }
        std::printf("%s\n", body.c_str());
        return 0;
    }
    if (argc >= 9 && std::strcmp(argv[1], "page") == 0) {
        nsx::PageSpec spec;
        if (std::strcmp(argv[3], "or") == 0) spec.mode = nsx::PageSpec::SearchOr;
        else if (std::strcmp(argv[3], "and") == 0) spec.mode = nsx::PageSpec::SearchAnd;
        else if (std::strcmp(argv[3], "boolean") == 0) spec.mode = nsx::PageSpec::Boolean;
        else if (std::strcmp(argv[3], "newest") == 0) { spec.mode = nsx::PageSpec::Sorted; spec.sort.ascending = false; }
        else if (std::strcmp(argv[3], "oldest") == 0) { spec.mode = nsx::PageSpec::Sorted; spec.sort.ascending = true; }
        else if (std::strcmp(argv[3], "boolean-newest") == 0) { spec.mode = nsx::PageSpec::BooleanSorted; spec.sort.ascending = false; }
        else if (std::strcmp(argv[3], "boolean-oldest") == 0) { spec.mode = nsx::PageSpec::BooleanSorted; spec.sort.ascending = true; }
        else if (std::strcmp(argv[3], "grouped") == 0) spec.mode = nsx::PageSpec::Grouped;
        else if (std::strcmp(argv[3], "grouped-newest") == 0) { spec.mode = nsx::PageSpec::GroupedSorted; spec.sort.ascending = false; }
        else if (std::strcmp(argv[3], "grouped-oldest") == 0) { spec.mode = nsx::PageSpec::GroupedSorted; spec.sort.ascending = true; }
        else if (std::strcmp(argv[3], "quorum") == 0) spec.mode = nsx::PageSpec::Quorum;
        else if (std::strcmp(argv[3], "quorum-newest") == 0) { spec.mode = nsx::PageSpec::QuorumSorted; spec.sort.ascending = false; }
        else if (std::strcmp(argv[3], "quorum-oldest") == 0) { spec.mode = nsx::PageSpec::QuorumSorted; spec.sort.ascending = true; }
        else { std::fprintf(stderr, "page: the mode is or, and, boolean, newest, oldest, boolean-newest, boolean-oldest, grouped, grouped-newest, grouped-oldest, quorum, quorum-newest or quorum-oldest, not %s\n", argv[3]); return 2; }
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        spec.use_filter = std::strcmp(argv[4], "-") != 0 || std::strcmp(argv[5], "-") != 0;
        if (std::strcmp(argv[4], "-") != 0) spec.filter.date_from = argv[4];
        if (std::strcmp(argv[5], "-") != 0) spec.filter.date_to = argv[5];
        const int k = std::atoi(argv[6]);
        const std::string cursor = std::strcmp(argv[7], "-") != 0 ? argv[7] : "";
        std::string q, body;
        for (int i = 8; i < argc; i++) { if (i > 8) q.push_back(' '); q += argv[i]; }
        if (!eng.search_page_text(q, k, cursor, spec, body)) { std::fprintf(stderr, "page failed: %s\n", body.c_str()); return 1; }
        std::printf("%s\n", body.c_str());
        return 0;
    }
    if (argc >= 4 && std::strcmp(argv[1], "correct") == 0) {
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        std::string body;
        if (!eng.did_you_mean_text(argv[3], argc > 4 ? std::atoi(argv[4]) : 5, body)) { std::fprintf(stderr, "correct failed: %s\n", body.c_str()); return 1; }
        std::printf("%s\n", body.c_str());
        return 0;
    }
    if (argc >= 4 && std::strcmp(argv[1], "complete") == 0) {
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        std::string body;
        if (!eng.complete_text(argv[3], argc > 4 ? std::atoi(argv[4]) : 5, body)) { std::fprintf(stderr, "complete failed: %s\n", body.c_str()); return 1; }
        std::printf("%s\n", body.c_str());
        return 0;
    }
    if (argc >= 4 && std::strcmp(argv[1], "similar") == 0) {
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        std::string body;
        if (!eng.more_like_this_text(argv[3], argc > 4 ? std::atoi(argv[4]) : 10, body)) { std::fprintf(stderr, "similar failed: %s\n", body.c_str()); return 1; }
        std::printf("%s\n", body.c_str());
        return 0;
    }
    if (argc >= 3 && std::strcmp(argv[1], "compact") == 0) {
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        const size_t first = argc > 3 ? (size_t)std::strtoull(argv[3], nullptr, 10) : 0;
        const size_t count = argc > 4 ? (size_t)std::strtoull(argv[4], nullptr, 10) : SIZE_MAX;
        nsx::CompactStats st;
        if (!eng.compact(first, count, true, &st)) { std::fprintf(stderr, "compact failed: %s\n", eng.last_error().c_str()); return 1; }
        if (!eng.last_error().empty()) std::fprintf(stderr, "%s\n", eng.last_error().c_str());
        std::printf("{\"sources\": %u, \"docs\": %u, \"terms_in\": %llu, \"terms\": %u, \"pairs\": %llu, \"merge_ms\": %.3f, \"invert_ms\": %.3f, \"call_s\": %.4f, \"total_s\": %.4f, \"segments\": %zu}\n",
                    st.sources, st.n_docs, (unsigned long long)st.terms_in, st.n_terms, (unsigned long long)st.pairs, st.merge_ms, st.invert_ms, st.call_s, st.total_s, eng.segments.size());
        return 0;
    }
    if (argc >= 4 && std::strcmp(argv[1], "delete") == 0) {
        nextsearch::Engine eng(0);
        eng.index_dir = argv[2];
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        std::vector<std::string> uids(argv + 3, argv + argc);
        nsx::DeleteStats st;
        if (!eng.delete_documents(uids, &st)) { std::fprintf(stderr, "delete failed: %s\n", eng.last_error().c_str()); return 1; }
        if (!eng.last_error().empty()) std::fprintf(stderr, "%s\n", eng.last_error().c_str());
        std::printf("{\"docs_deleted\": %u, \"uids_not_found\": %u, \"segments_rewritten\": %u, \"segments_dropped\": %u, \"terms_dropped\": %u, \"pairs_in\": %llu, \"pairs_out\": %llu, \"merge_ms\": %.3f, \"invert_ms\": %.3f, \"call_s\": %.4f, \"total_s\": %.4f, \"segments\": %zu}\n",
                    st.docs_deleted, st.uids_not_found, st.segments_rewritten, st.segments_dropped, st.terms_dropped, (unsigned long long)st.pairs_in, (unsigned long long)st.pairs_out,
                    st.merge_ms, st.invert_ms, st.call_s, st.total_s, eng.segments.size());
        return 0;
    }
    if (argc >= 4 && std::strcmp(argv[1], "index") == 0) {
        nsx::FileBytes in;
        if (!in.load(argv[3])) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 1; }
        const uint32_t n = in.u32();
        if ((uint64_t)n * 16 > in.size()) { std::fprintf(stderr, "%s: document count %u does not fit the file\n", argv[3], n); return 1; }
        std::vector<nsx::DocInput> docs(n);
        for (auto& d : docs) { d.cord_uid = in.str(); d.title = in.str(); d.json_relpath = in.str(); d.text = in.str(); }
        ns_ctx* ctx = nullptr;
        if (ns_ctx_create(argc > 4 ? std::atoi(argv[4]) : 0, &ctx) != NS_OK) { std::fprintf(stderr, "ns_ctx_create: %s\n", ns_last_error(nullptr)); return 1; }
        nsx::IndexStats st;
        nsx::InvertStats ist;
        std::string err;
        const bool ok = nsx::index_documents(ctx, docs, argv[2], st, err) && nsx::invert_segment(ctx, argv[2], ist, err);
        ns_ctx_destroy(ctx);
        if (!ok) { std::fprintf(stderr, "index failed: %s\n", err.c_str()); return 1; }
        std::printf("{\"docs_in\": %u, \"docs\": %u, \"terms\": %u, \"text_bytes\": %llu, \"tokens\": %llu, \"kept_tokens\": %llu, \"pairs\": %llu, "
                    "\"forward_device_ms\": %.3f, \"forward_total_s\": %.4f, \"invert_device_ms\": %.3f, \"invert_total_s\": %.4f}\n",
                    st.n_docs_in, st.n_docs, st.n_terms, (unsigned long long)st.text_bytes, (unsigned long long)st.tokens,
                    (unsigned long long)st.kept_tokens, (unsigned long long)st.pairs, st.device_ms, st.total_s, ist.device_ms, ist.total_s);
        return 0;
    }
    if (argc >= 5 && std::strcmp(argv[1], "facade-bench") == 0) {
        const int k = std::atoi(argv[4]);
        const int reps = argc > 5 ? std::max(1, std::atoi(argv[5])) : 5;
        const int device = argc > 6 ? std::atoi(argv[6]) : 0;
        std::vector<std::string> qs;
        {
            std::ifstream in(argv[3]);
            std::string ln;
            while (std::getline(in, ln)) qs.push_back(ln);
        }
        if (qs.empty()) { std::fprintf(stderr, "no queries in %s\n", argv[3]); return 1; }
        nextsearch::Engine eng(device);
        eng.index_dir = argv[2];
        auto now = []() { return std::chrono::steady_clock::now(); };
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        const auto r0 = now();
        if (!eng.reload()) { std::fprintf(stderr, "reload failed: %s\n", eng.last_error().c_str()); return 1; }
        const double reload_ms = ms(r0, now());
        const size_t Q = qs.size();
        const int K = std::max(1, std::min(k, 100));
        std::vector<nextsearch::Engine::QueryView> views(Q);
        for (size_t q = 0; q < Q; q++) views[q] = {qs[q].data(), qs[q].size()};
        std::vector<ns_query_desc> qd;
        std::vector<ns_term_ref> refs;
        std::vector<uint8_t> usable;
        std::vector<double> t_prep, t_flat;
        for (int r = 0; r < reps + 1; r++) {
            const auto a = now();
            eng.build_refs(qs, qd, refs, usable);
            if (r) t_prep.push_back(ms(a, now()));
        }
        std::vector<ns_hit> hits(Q * (size_t)K);
        std::vector<uint32_t> nhits(Q);
        std::vector<uint64_t> found(Q);
        uint64_t check = 0;
        if (device >= 0) {
            for (int r = 0; r < reps + 2; r++) {
                const auto a = now();
                if (!eng.search_batch_flat(views.data(), Q, k, NS_FLAG_OR, hits.data(), nhits.data(), found.data(), usable.data())) {
                    std::fprintf(stderr, "search_batch_flat failed: %s\n", eng.last_error().c_str());
                    return 1;
                }
                if (r >= 2) t_flat.push_back(ms(a, now()));
            }
            for (size_t q = 0; q < Q; q++) check += found[q] + nhits[q];
        }
        auto med = [](std::vector<double> v) { if (v.empty()) return 0.0; std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
        const double p = med(t_prep), f = med(t_flat);
        std::printf("{\"queries\": %zu, \"k\": %d, \"term_refs\": %zu, \"reload_ms\": %.1f, \"query_prep_ms\": %.3f, \"query_prep_qps\": %.0f, "
                    "\"search_batch_flat_ms\": %.3f, \"search_batch_flat_qps\": %.0f, \"reps\": %d, \"checksum\": %llu}\n",
                    Q, K, refs.size(), reload_ms, p, p > 0 ? Q / (p * 1e-3) : 0.0, f, f > 0 ? Q / (f * 1e-3) : 0.0, reps, (unsigned long long)check);
        return 0;
    }
    std::fprintf(stderr, "usage: %s gen-index <dir> <n_segments> <docs_per_segment> [vocab] [seed] [--legacy]\n       %s search <dir> <k> <query...>\n       %s index <segment_dir> <documents_file> [device]\n       %s compact <index_dir> [first count]\n       %s delete <index_dir> <uid>...\n       %s correct <index_dir> <query> [limit]\n       %s complete <index_dir> <input> [limit]\n       %s similar <index_dir> <uid> [k]\n       %s search-filtered <index_dir> <from> <to> <k> <query...>\n       %s search-faceted <index_dir> <year|month> <from> <to> <k> <query...>\n", argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0]);
    return 2;
}
