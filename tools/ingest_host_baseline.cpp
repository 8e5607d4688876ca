// The single-thread host comparator of tools/ingest_bench.py: the project's own tokeniser (host/textutil.hpp, the
// restatement of the reference's include/textutil.hpp:13-37) + std::unordered_map, doing what src/ForwardIndex.cpp:139-179
// does per document — tf map, term ids (first-seen, this project's rule), pairs sorted by term id.
//   ingest_host_baseline <texts_file>     texts_file: u32 n, then n x (u32 length + bytes)
// Prints one JSON line; `check` = a sum over (docId, termId, tf) that tools/ingest_bench.py compares with the device's.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "textutil.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    uint32_t n = 0;
    if (std::fread(&n, 4, 1, f) != 1) return 1;
    std::vector<std::string> texts(n);
    for (auto& t : texts) {
        uint32_t len = 0;
        if (std::fread(&len, 4, 1, f) != 1) return 1;
        t.resize(len);
        if (len && std::fread(&t[0], 1, len, f) != len) return 1;
    }
    std::fclose(f);
    const auto t0 = std::chrono::steady_clock::now();
    std::unordered_map<std::string, uint32_t> term_to_id;
    term_to_id.reserve(400000);
    uint64_t tokens = 0, kept = 0, pairs = 0, check = 0, bytes = 0;
    uint32_t docs = 0;
    std::vector<std::pair<uint32_t, uint32_t>> post;
    for (const auto& text : texts) {
        bytes += text.size();
        std::unordered_map<uint32_t, uint32_t> tf;
        uint32_t doc_len = 0;
        for (auto& t : nextsearch::tokenize(text)) {
            tokens++;
            if (t.size() < 2 || nextsearch::is_stopword(t)) continue;
            auto it = term_to_id.find(t);
            if (it == term_to_id.end()) it = term_to_id.emplace(t, (uint32_t)term_to_id.size()).first;
            tf[it->second] += 1;
            doc_len++;
        }
        if (!doc_len) continue;
        post.assign(tf.begin(), tf.end());
        std::sort(post.begin(), post.end());
        for (auto& p : post) check += (uint64_t)(docs + 1) * 1000003ull + (uint64_t)p.first * 7919ull + p.second;
        pairs += post.size();
        kept += doc_len;
        docs++;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("{\"seconds\": %.4f, \"text_bytes\": %llu, \"tokens\": %llu, \"kept_tokens\": %llu, \"docs\": %u, \"terms\": %zu, \"pairs\": %llu, \"check\": %llu}\n",
                s, (unsigned long long)bytes, (unsigned long long)tokens, (unsigned long long)kept, docs, term_to_id.size(),
                (unsigned long long)pairs, (unsigned long long)check);
    return 0;
}
