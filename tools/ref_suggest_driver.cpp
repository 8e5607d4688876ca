// TEST INFRASTRUCTURE ONLY — driver around the REAL reference engine's autocomplete (cord19::Engine::suggest,
// src/api_engine.cpp:164-187, over the AutocompleteIndex that Engine::reload builds, :91-107).
//
// This file is ours; it #includes the reference's own headers the way oracle/ref_driver.cpp does and is linked against
// the reference's translation units that `make -C oracle ref` compiled under oracle/_ref/.  tools/gen_golden_suggest.py
// compiles it into a temporary directory; the binary is never committed and never needed on a GPU machine.
//
//   ref_suggest_driver json <index_dir> <requests.bin> <out.bin>
//       requests.bin: records {i32 limit, u32 n, n bytes of input} (length-prefixed: NUL and control bytes survive).
//       out.bin, per request: u8 dumped (0: dump(2) threw, e.g. on invalid UTF-8), u32 n + n bytes of
//       Engine::suggest(input, limit).dump(2), u32 count, count x (u32 n + n bytes) of the suggestions.
//   ref_suggest_driver time <index_dir> <requests.bin> <repeats>
//       one JSON line: the trie's build time (AutocompleteIndex::build over the df sums, as reload() runs it) and the
//       mean time of Engine::suggest over the requests, on this CPU.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <unistd.h>
#include <unordered_map>
#include <vector>

#include "api_engine.hpp"

struct Request {
    int limit;
    std::string input;
};

static std::vector<Request> read_requests(const std::string& path) {
    std::ifstream in(path, std::ios::binary);
    std::vector<Request> out;
    for (;;) {
        int32_t limit = 0;
        uint32_t n = 0;
        if (!in.read((char*)&limit, 4) || !in.read((char*)&n, 4)) break;
        std::string s(n, '\0');
        if (n && !in.read(&s[0], n)) break;
        out.push_back({limit, std::move(s)});
    }
    return out;
}

static void put_u32(std::string& o, uint32_t v) { o.append((const char*)&v, 4); }

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s json|time <index_dir> <requests.bin> <out.bin|repeats>\n", argv[0]);
        return 2;
    }
    const std::string mode = argv[1];
    const std::string index_dir = fs::absolute(argv[2]).string();
    const auto reqs = read_requests(fs::absolute(argv[3]).string());
    const std::string last = argv[4];
    const std::string outpath = mode == "json" ? fs::absolute(last).string() : std::string();

    // the engine persists its caches into the CWD: run from a private scratch directory
    char tmpl[] = "/tmp/ns_ref_suggest_XXXXXX";
    char* scratch = mkdtemp(tmpl);
    if (!scratch || chdir(scratch) != 0) { std::perror("scratch"); return 1; }

    cord19::Engine engine;
    engine.index_dir = index_dir;
    if (!engine.reload()) { std::fprintf(stderr, "reload failed for %s\n", index_dir.c_str()); return 1; }

    if (mode == "json") {
        std::string o;
        for (const auto& r : reqs) {
            cord19::json j = engine.suggest(r.input, r.limit);
            std::string text;
            uint8_t dumped = 1;
            try { text = j.dump(2); } catch (const std::exception&) { dumped = 0; text.clear(); }
            o.push_back((char)dumped);
            put_u32(o, (uint32_t)text.size());
            o += text;
            const auto& sug = j["suggestions"];
            put_u32(o, (uint32_t)sug.size());
            for (const auto& s : sug) {
                const std::string t = s.get<std::string>();
                put_u32(o, (uint32_t)t.size());
                o += t;
            }
        }
        std::ofstream out(outpath, std::ios::binary);
        out.write(o.data(), (std::streamsize)o.size());
        return out ? 0 : 1;
    }
    if (mode == "time") {
        const int repeats = std::max(1, std::atoi(last.c_str()));
        // the build as reload() runs it (:94-106), timed alone
        double build_s = 1e30;
        for (int rep = 0; rep < 3; rep++) {
            const auto t0 = std::chrono::steady_clock::now();
            std::unordered_map<std::string, uint32_t> term_to_score;
            term_to_score.reserve(200000);
            for (const auto& seg : engine.segments)
                for (const auto& kv : seg.lex) term_to_score[kv.first] += kv.second.df;
            cord19::AutocompleteIndex ac;
            ac.build(term_to_score, 10);
            build_s = std::min(build_s, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
        size_t n_sugg = 0;
        for (const auto& r : reqs) n_sugg += engine.suggest(r.input, r.limit)["suggestions"].size();   // warm-up
        const auto t0 = std::chrono::steady_clock::now();
        for (int rep = 0; rep < repeats; rep++)
            for (const auto& r : reqs) n_sugg += engine.suggest(r.input, r.limit)["suggestions"].size();
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const double n = (double)reqs.size() * repeats;
        std::printf("{\"build_s\": %.6f, \"requests\": %.0f, \"seconds\": %.6f, \"us_per_request\": %.4f, \"requests_per_s\": %.1f, \"suggestions\": %zu}\n",
                    build_s, n, s, 1e6 * s / n, n / s, n_sugg);
        return 0;
    }
    std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
    return 2;
}
