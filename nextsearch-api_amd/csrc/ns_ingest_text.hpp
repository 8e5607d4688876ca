// SPDX-License-Identifier: MIT
// The text rules of indexing on the device (csrc/ns_ingest.hip) and of compaction's dictionary stage
// (csrc/ns_compact.hip, §5j): which bytes make a token, which words are dropped, the 64-bit polynomial hash of a byte range
// and how a workgroup's chunk hashes join into it, and the size of the dictionary table.  Host and device code, no HIP type and no runtime call, like
// ns_after_plan.hpp; tests/ingest_text_harness.cpp compiles it with g++ for the CPU suite.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NS_IG_HD __host__ __device__ __forceinline__
#else
#define NS_IG_HD inline
#endif

namespace ns {

constexpr int kIgTile = 256 * 16;            // text bytes per workgroup
constexpr uint32_t kIgLong = 1024;           // tokens longer than this are hashed by a workgroup, not by a thread
constexpr uint32_t kIgEmpty = 0xFFFFFFFFu;
constexpr uint64_t kIgP = 0x9E3779B97F4A7C15ull;   // odd: the polynomial's base modulo 2^64
constexpr uint64_t kIgMinTable = 1024;       // the dictionary table's smallest size, in slots

NS_IG_HD bool ig_alnum(uint32_t c) { return (c - '0' < 10u) || ((c | 0x20u) - 'a' < 26u); }
NS_IG_HD uint64_t ig_mix(uint64_t h) {   // the low bits of a polynomial modulo 2^64 only see the bytes' low bits
    h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;
    return h;
}
NS_IG_HD uint64_t ig_pow(uint64_t b, uint32_t e) {
    uint64_t r = 1;
    for (; e; e >>= 1, b *= b) if (e & 1u) r *= b;
    return r;
}

// include/textutil.hpp:31-37, the words of 2 .. 4 bytes packed little-endian ("a" falls to the length rule)
constexpr uint32_t ig_w(const char* s) {
    uint32_t w = 0;
    for (int i = 0; s[i]; i++) w |= (uint32_t)(unsigned char)s[i] << (8 * i);
    return w;
}
NS_IG_HD bool ig_stop(uint32_t w) {
    constexpr uint32_t sw[] = {ig_w("the"), ig_w("an"), ig_w("and"), ig_w("or"), ig_w("of"), ig_w("to"), ig_w("in"), ig_w("for"),
                               ig_w("on"), ig_w("with"), ig_w("by"), ig_w("as"), ig_w("is"), ig_w("are"), ig_w("was"), ig_w("were"),
                               ig_w("be"), ig_w("been"), ig_w("it"), ig_w("this"), ig_w("that"), ig_w("from"), ig_w("at")};
    bool hit = false;
#ifdef __clang__
#pragma unroll
#endif
    for (uint32_t s : sw) hit |= (w == s);
    return hit;
}

// The slots of the dictionary table for k entries (kept tokens in ns_forward_build, source terms in the merge): a power of two,
// at least twice k, so that an empty slot always ends a probe.  k < 2^31: at most 2^32 slots, the mask fits 32 bits.
NS_IG_HD uint64_t ig_table_slots(uint64_t k) {
    uint64_t cap = kIgMinTable;
    while (cap < 2ull * k) cap <<= 1;
    return cap;
}

// the hash of the `len` bytes at p, by one thread: the polynomial in kIgP over byte + 1, mixed with the length
NS_IG_HD uint64_t ig_hash_bytes(const uint8_t* p, uint32_t len) {
    uint64_t h = 0;
    for (uint32_t j = 0; j < len; j++) h = h * kIgP + (uint64_t)(p[j] + 1u);
    return ig_mix(h ^ len);
}

// The same hash from a workgroup's 256 chunk polynomials: part[t] is the polynomial (not mixed) over the bytes
// [min(len, t * chunk), min(len, (t + 1) * chunk)) with chunk = ceil(len / 256); h(AB) = h(A) * P^|B| + h(B).  The last
// chunk with bytes may be short, the threads behind it have none.
NS_IG_HD uint64_t ig_hash_join(const uint64_t* part, uint32_t len) {
    const uint32_t chunk = (len + 255u) / 256u;
    uint64_t H = 0;
    const uint64_t pc = ig_pow(kIgP, chunk);
    for (uint32_t t = 0; t < 256; t++) {
        const uint32_t tb = len < t * chunk ? len : t * chunk, te = len < tb + chunk ? len : tb + chunk;
        if (te == tb) break;
        H = H * (te - tb == chunk ? pc : ig_pow(kIgP, te - tb)) + part[t];
    }
    return ig_mix(H ^ len);
}

}  // namespace ns
