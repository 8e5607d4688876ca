// merge_plan (csrc/ns_merge_plan.hpp) and invert_plan (csrc/ns_radix_plan.hpp) for tests/test_merge_plan_cpu.py (built by g++
// inside the test; no HIP, no device).  A case and its answer are arrays of 64-bit words, so that the shared library that the
// test loads and, with -DMERGE_PLAN_MAIN, the program of its own that runs the same cases under the host sanitizers go through
// ONE decoder:
//   merge case   0, n_src, cp_inplace, keep given; per source n_docs, n_pairs, n_terms, then the arrays doc_len, counts, pairs
//                (two words a pair), term_bytes, term_offsets and the bitmap, each as {given, length, the elements}
//   invert case  1, n_docs, n_pairs, n_terms, the counts as {given, length, the elements}
//   answer       0, the length of the refusal, its characters   |   1, the scalars, then every array as {length, the elements}
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "ns_merge_plan.hpp"
#include "ns_radix_plan.hpp"

namespace {

struct Reader {
    const uint64_t* w;
    size_t n, at = 0;
    bool bad = false;
    uint64_t next() { if (at >= n) { bad = true; return 0; } return w[at++]; }
    // -> whether the array is given; elements narrowed to T
    template <class T> bool array(std::vector<T>& out) {
        const bool given = next() != 0;
        const uint64_t len = next();
        if (len > n - at) { bad = true; return given; }
        out.reserve((size_t)len + 1);   // (an array given with no element is still not NULL)
        out.resize((size_t)len);
        for (size_t i = 0; i < (size_t)len; i++) out[i] = (T)next();
        return given;
    }
};

template <class T> void put(std::vector<uint64_t>& out, const std::vector<T>& a) {
    out.push_back(a.size());
    for (const T& v : a) out.push_back((uint64_t)v);
}

void refuse(std::vector<uint64_t>& out, const std::string& err) {
    out.assign({0, err.size()});
    for (unsigned char c : err) out.push_back(c);
}

struct Source {
    std::vector<uint32_t> doc_len, counts, pairs, bits;
    std::vector<uint8_t> term_bytes;
    std::vector<uint64_t> term_offsets;
};

bool run_case(const uint64_t* words, size_t n_words, std::vector<uint64_t>& out) {
    Reader r{words, n_words};
    std::string err;
    const uint64_t kind = r.next();
    if (kind == 0) {
        const uint32_t n_src = (uint32_t)r.next();
        const bool cp_inplace = r.next() != 0, keep_given = r.next() != 0;
        if (n_src > n_words) return false;
        std::vector<Source> store(n_src);
        std::vector<ns_forward_src> src(n_src);
        std::vector<const uint32_t*> keep(n_src, nullptr);
        for (uint32_t s = 0; s < n_src; s++) {
            Source& S = store[s];
            src[s].n_docs = (uint32_t)r.next(); src[s].n_pairs = r.next(); src[s].n_terms = (uint32_t)r.next();
            src[s].doc_len = r.array(S.doc_len) ? S.doc_len.data() : nullptr;
            src[s].counts = r.array(S.counts) ? S.counts.data() : nullptr;
            src[s].pairs = r.array(S.pairs) ? S.pairs.data() : nullptr;
            src[s].term_bytes = r.array(S.term_bytes) ? S.term_bytes.data() : nullptr;
            src[s].term_offsets = r.array(S.term_offsets) ? S.term_offsets.data() : nullptr;
            keep[s] = r.array(S.bits) ? S.bits.data() : nullptr;
        }
        if (r.bad || r.at != n_words) return false;
        ns::MergePlan p;
        if (!ns::merge_plan(n_src ? src.data() : nullptr, keep_given ? keep.data() : nullptr, n_src, cp_inplace, p, err)) { refuse(out, err); return true; }
        out.assign({1, p.filtered, p.raw_pairs, p.T, p.text_bytes, p.n_docs, p.n_pairs, p.total_len, p.n_wave, p.n_lds, p.n_bigdocs, p.n_big});
        put(out, p.term_base); put(out, p.pair_base); put(out, p.raw_base); put(out, p.prefix); put(out, p.srcpos); put(out, p.kept_len);
        put(out, p.kept_cnt); put(out, p.live0); put(out, p.kstart); put(out, p.klen); put(out, p.lists);
        return true;
    }
    if (kind == 1) {
        const uint32_t n_docs = (uint32_t)r.next();
        const uint64_t n_pairs = r.next();
        const uint32_t n_terms = (uint32_t)r.next();
        std::vector<uint32_t> counts;
        r.array(counts);
        if (r.bad || r.at != n_words || counts.size() != n_docs) return false;
        ns::InvertPlan p;
        if (!ns::invert_plan(counts.data(), n_docs, n_pairs, n_terms, p, err)) { refuse(out, err); return true; }
        out.assign({1, p.n_tiles, p.m_max, p.scan_blocks_max, (uint64_t)p.rp.passes});
        put(out, p.prefix); put(out, p.tile_docs);
        return true;
    }
    return false;
}

}  // namespace

extern "C" {

// -> the answer's length in words (copied to `out` where cap holds it), or -1 for a case that does not decode
int64_t plan_case(const uint64_t* words, uint64_t n_words, uint64_t* out, uint64_t cap) {
    std::vector<uint64_t> a;
    if (!run_case(words, (size_t)n_words, a)) return -1;
    if (a.size() <= cap) for (size_t i = 0; i < a.size(); i++) out[i] = a[i];
    return (int64_t)a.size();
}

void plan_consts(uint32_t out[3]) { out[0] = (uint32_t)ns::kIvTile; out[1] = ns::kCpWaveMax; out[2] = ns::kCpDocCut; }

}  // extern "C"

#ifdef MERGE_PLAN_MAIN
// merge_plan_main CASES ANSWERS: both files are 64-bit words; CASES holds {length, the case} back to back, ANSWERS gets
// {length, the answer} in the same order.
int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s CASES ANSWERS\n", argv[0]); return 2; }
    std::vector<uint64_t> in;
    if (FILE* f = std::fopen(argv[1], "rb")) {
        uint64_t w;
        while (std::fread(&w, 8, 1, f) == 1) in.push_back(w);
        std::fclose(f);
    } else { std::perror(argv[1]); return 2; }
    FILE* g = std::fopen(argv[2], "wb");
    if (!g) { std::perror(argv[2]); return 2; }
    size_t at = 0, n_cases = 0;
    while (at < in.size()) {
        const uint64_t len = in[at++];
        std::vector<uint64_t> a;
        if (len > in.size() - at || !run_case(in.data() + at, (size_t)len, a)) { std::fprintf(stderr, "merge_plan_harness: case %zu does not decode\n", n_cases); return 1; }
        at += (size_t)len;
        const uint64_t alen = a.size();
        std::fwrite(&alen, 8, 1, g);
        if (alen) std::fwrite(a.data(), 8, a.size(), g);
        n_cases++;
    }
    std::fclose(g);
    std::printf("merge_plan_harness: %zu cases\n", n_cases);
    return 0;
}
#endif
