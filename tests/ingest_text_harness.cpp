// C entry points over csrc/ns_ingest_text.hpp and host/textutil.hpp for tests/test_ingest_shapes_cpu.py (built by g++ inside the
// test; no HIP, no device).  With -DINGEST_TEXT_MAIN it is a program of its own that checks the join of chunk hashes against the
// sequential hash, for a run under the host sanitizers.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "ns_ingest_text.hpp"
#include "textutil.hpp"

// the hash of a token as k_ig_hash_long computes it: thread t's polynomial over its chunk, then thread 0's join
static uint64_t chunked_hash(const uint8_t* p, uint32_t len) {
    uint64_t part[256];
    const uint32_t chunk = (len + 255u) / 256u;
    for (uint32_t t = 0; t < 256; t++) {
        const uint32_t b = len < t * chunk ? len : t * chunk, e = len < b + chunk ? len : b + chunk;
        uint64_t h = 0;
        for (uint32_t j = b; j < e; j++) h = h * ns::kIgP + (uint64_t)(p[j] + 1u);
        part[t] = h;
    }
    return ns::ig_hash_join(part, len);
}

extern "C" {

int ig_alnum_c(uint32_t c) { return ns::ig_alnum(c) ? 1 : 0; }
int host_alnum_c(uint32_t c) { return nextsearch::is_alnum_ascii((unsigned char)c) ? 1 : 0; }

// Every word of `len` bytes (2 .. 4) over `alphabet` (n_alpha bytes): word i has alphabet[(i / n_alpha^j) % n_alpha] as its byte j.
// ig_out[i]: ig_stop of the word packed as k_ig_keep packs it (byte j at bits 8 j); host_out[i]: host/textutil.hpp's is_stopword.
void stop_words_c(const uint8_t* alphabet, uint32_t n_alpha, uint32_t len, uint8_t* ig_out, uint8_t* host_out) {
    uint64_t total = 1;
    for (uint32_t j = 0; j < len; j++) total *= n_alpha;
    std::string s(len, ' ');
    for (uint64_t i = 0; i < total; i++) {
        uint32_t w = 0;
        uint64_t r = i;
        for (uint32_t j = 0; j < len; j++, r /= n_alpha) {
            const uint8_t c = alphabet[r % n_alpha];
            w |= (uint32_t)c << (8 * j);
            s[j] = (char)c;
        }
        ig_out[i] = ns::ig_stop(w) ? 1 : 0;
        host_out[i] = nextsearch::is_stopword(s) ? 1 : 0;
    }
}

uint64_t ig_hash_bytes_c(const uint8_t* p, uint32_t len) { return ns::ig_hash_bytes(p, len); }
uint64_t ig_hash_chunked_c(const uint8_t* p, uint32_t len) { return chunked_hash(p, len); }

uint64_t ig_table_slots_c(uint64_t k) { return ns::ig_table_slots(k); }

// 0: kIgTile, 1: kIgLong, 2: kIgEmpty, 3: kIgP, 4: kIgMinTable
uint64_t ig_const_c(int which) {
    switch (which) {
        case 0: return (uint64_t)ns::kIgTile;
        case 1: return ns::kIgLong;
        case 2: return ns::kIgEmpty;
        case 3: return ns::kIgP;
        case 4: return ns::kIgMinTable;
    }
    return 0;
}

}  // extern "C"

#ifdef INGEST_TEXT_MAIN
int main() {
    unsigned long long bad = 0, seen = 0;
    const uint32_t lens[] = {1, 2, 255, 256, 257, 1023, 1024, 1025, 1279, 1280, 1281, 4096, 65535, 65536, 65537, 70001};
    for (uint32_t len : lens) {
        std::vector<uint8_t> v(len);
        uint32_t x = len * 2654435761u + 1u;
        for (uint32_t i = 0; i < len; i++) { x = x * 1664525u + 1013904223u; v[i] = (uint8_t)(x >> 24); }
        seen++;
        if (chunked_hash(v.data(), len) != ns::ig_hash_bytes(v.data(), len)) { std::printf("ingest_text_harness: WRONG: length %u\n", len); bad++; }
    }
    int alnum = 0;
    for (uint32_t c = 0; c < 256; c++) alnum += ns::ig_alnum(c) ? 1 : 0;
    if (alnum != 62) { std::printf("ingest_text_harness: WRONG: %d alnum bytes\n", alnum); bad++; }
    std::printf("ingest_text_harness: %llu lengths, %llu wrong\n", seen, bad);
    return bad ? 1 : 0;
}
#endif
