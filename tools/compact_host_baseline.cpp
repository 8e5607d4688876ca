// One-thread host restatement of ns_forward_merge for tools/compact_bench.py: the term walk with a
// std::unordered_map, the remap of the pairs, a std::sort inside each document.  Input file: u32 n_src, then per source
// u32 n_docs, u32 n_terms, u64 n_pairs, counts[n_docs], pairs[2 * n_pairs], then per term u32 length + bytes.
// Prints one JSON line: seconds (arrays in memory -> merged arrays in memory), terms, pairs and a checksum of the merged pairs.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>

struct Source {
    std::vector<uint32_t> counts, pairs;
    std::vector<std::string> terms;
};

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: compact_host_baseline <parts file>\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    auto rd = [&](void* p, size_t n) { if (n && std::fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(1); } };
    uint32_t n_src = 0;
    rd(&n_src, 4);
    std::vector<Source> src(n_src);
    for (auto& s : src) {
        uint32_t n_docs = 0, n_terms = 0;
        uint64_t n_pairs = 0;
        rd(&n_docs, 4); rd(&n_terms, 4); rd(&n_pairs, 8);
        s.counts.resize(n_docs); s.pairs.resize(n_pairs * 2); s.terms.resize(n_terms);
        rd(s.counts.data(), (size_t)n_docs * 4);
        rd(s.pairs.data(), (size_t)n_pairs * 8);
        for (auto& t : s.terms) { uint32_t len = 0; rd(&len, 4); t.resize(len); rd(&t[0], len); }
    }
    std::fclose(f);
    const auto t0 = std::chrono::steady_clock::now();
    std::unordered_map<std::string, uint32_t> ids;
    std::vector<const std::string*> terms;
    std::vector<uint64_t> merged;                       // termId << 32 | tf, documents back to back
    std::vector<uint32_t> counts;
    for (const auto& s : src) {
        std::vector<uint32_t> map(s.terms.size());
        for (size_t t = 0; t < s.terms.size(); t++) {
            auto it = ids.emplace(s.terms[t], (uint32_t)terms.size());
            if (it.second) terms.push_back(&it.first->first);
            map[t] = it.first->second;
        }
        size_t at = 0;
        for (uint32_t c : s.counts) {
            const size_t begin = merged.size();
            for (uint32_t j = 0; j < c; j++, at++) merged.push_back(((uint64_t)map[s.pairs[2 * at]] << 32) | s.pairs[2 * at + 1]);
            std::sort(merged.begin() + begin, merged.end());
            counts.push_back(c);
        }
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    uint64_t check = 0, doc = 1, at = 0;
    for (uint32_t c : counts) {
        for (uint32_t j = 0; j < c; j++, at++) check += doc * 1000003ull + (merged[at] >> 32) * 7919ull + (merged[at] & 0xFFFFFFFFull);
        doc++;
    }
    std::printf("{\"seconds\": %.4f, \"terms\": %zu, \"pairs\": %zu, \"check\": %llu}\n", seconds, terms.size(), merged.size(), (unsigned long long)check);
    return 0;
}
