// One host thread doing what ns_ac_fuzzy does (csrc/ns_fuzzy.hip), with the same definition and the same filters: the
// candidates in a length-ordered permutation with a byte-set signature each, the prefix's index range per length, the
// signature test, then the banded optimal-string-alignment DP (rows over the query's bytes), and the best L by the key
// (distance, ~score, index).  The yardstick of tools/correct_bench.py, which also checks its answers equal to the device's.
//
//   g++ -O2 -std=c++17 -o correct_host_baseline tools/correct_host_baseline.cpp
//   correct_host_baseline <workload file> <answers file>        prints one JSON line: build and scan seconds, pairs, DP share
//
// workload file (little-endian): u32 n, n_q, L, prefix_len | u64 offsets[n + 1] | pool | u32 scores[n] |
//                                u32 q_offsets[n_q + 1] | query bytes | u8 max_edits[n_q]
// answers file:                  u32 idx[n_q * L] | u8 dist[n_q * L] | u32 count[n_q]
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static constexpr int kMaxLen = 64, kBuckets = kMaxLen + 4;
static constexpr uint64_t kSigBits = (1ull << 37) - 1, kEmpty = ~0ull;

static uint64_t sig_bit(uint8_t c) {
    if (c >= '0' && c <= '9') return 1ull << (c - '0');
    if (c >= 'a' && c <= 'z') return 1ull << (10 + c - 'a');
    return 1ull << 36;
}

// D[n][m] of the query q[0, n) against c[0, m), |m - n| <= E, cells j = i - E .. i + E per row; above E: some value above E
template <int E>
static uint32_t osa_band(const uint8_t* q, int n, const uint8_t* c, int m) {
    constexpr int B = 2 * E + 1;
    constexpr uint32_t kInf = 255;
    uint32_t p1[B], p2[B], cur[B];
    for (int t = 0; t < B; t++) { p1[t] = t >= E ? (uint32_t)(t - E) : kInf; p2[t] = kInf; cur[t] = kInf; }
    for (int i = 1; i <= n; i++) {
        uint32_t before = kInf, now = kInf;
        for (int t = 0; t < B; t++) {
            const int j = i + t - E;
            uint32_t v = kInf;
            if (j == 0) v = (uint32_t)i;
            else if (j > 0) {
                const uint8_t c1 = j - 1 < m ? c[j - 1] : 0;
                v = p1[t] + (q[i - 1] != c1 ? 1u : 0u);
                if (t + 1 < B) v = std::min(v, p1[t + 1] + 1);
                if (t >= 1) v = std::min(v, cur[t - 1] + 1);
                if (i >= 2 && j >= 2 && j - 1 < m && q[i - 1] == c[j - 2] && q[i - 2] == c1) v = std::min(v, p2[t] + 1);
            }
            cur[t] = v;
            before = std::min(before, p1[t]);
            now = std::min(now, v);
        }
        for (int t = 0; t < B; t++) { p2[t] = p1[t]; p1[t] = cur[t]; }
        if (std::min(before, now) > (uint32_t)E && i < n) return kInf;
    }
    const int dd = m - n + E;
    return dd >= 0 && dd < B ? p1[dd] : kInf;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <workload file> <answers file>\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    uint32_t hdr[4];
    bool ok = std::fread(hdr, 4, 4, f) == 4;
    const uint32_t n = hdr[0], n_q = hdr[1], L = hdr[2], prefix_len = hdr[3];
    std::vector<uint64_t> off(n + 1);
    ok = ok && std::fread(off.data(), 8, n + 1, f) == n + 1;
    std::vector<uint8_t> pool(ok ? off[n] : 0);
    ok = ok && std::fread(pool.data(), 1, pool.size(), f) == pool.size();
    std::vector<uint32_t> score(n), qoff(n_q + 1);
    ok = ok && std::fread(score.data(), 4, n, f) == n && std::fread(qoff.data(), 4, n_q + 1, f) == n_q + 1;
    std::vector<uint8_t> qb(ok ? qoff[n_q] : 0), edits(n_q);
    ok = ok && std::fread(qb.data(), 1, qb.size(), f) == qb.size() && std::fread(edits.data(), 1, n_q, f) == n_q;
    std::fclose(f);
    if (!ok || L < 1 || L > 10) { std::fprintf(stderr, "%s: short or malformed\n", argv[1]); return 1; }

    // ---- the side structures ----
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> len_start(kBuckets + 1, 0), bucket(n);
    std::vector<uint8_t> cand(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t len = off[i + 1] - off[i];
        bucket[i] = (uint32_t)std::min<uint64_t>(len, kBuckets - 1);
        const bool dup = i > 0 && off[i] - off[i - 1] == len && std::memcmp(&pool[off[i - 1]], &pool[off[i]], len) == 0;
        cand[i] = score[i] != 0 && !dup;
        if (cand[i]) len_start[bucket[i] + 1]++;
    }
    for (int b = 0; b < kBuckets; b++) len_start[b + 1] += len_start[b];
    std::vector<uint32_t> perm(len_start[kBuckets]), next(len_start.begin(), len_start.end() - 1);
    std::vector<uint64_t> psig(perm.size());
    for (uint32_t i = 0; i < n; i++) {
        if (!cand[i]) continue;
        uint64_t s = 0;
        for (uint64_t j = off[i]; j < off[i + 1]; j++) s |= sig_bit(pool[j]);
        perm[next[bucket[i]]] = i;
        psig[next[bucket[i]]++] = s;
    }
    const double build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    // ---- the scan ----
    std::vector<uint32_t> idx((size_t)n_q * L, ~0u), count(n_q, 0);
    std::vector<uint8_t> dist((size_t)n_q * L, 0xff);
    uint64_t pairs = 0, reached_dp = 0;
    const auto t1 = std::chrono::steady_clock::now();
    for (uint32_t q = 0; q < n_q; q++) {
        const uint8_t* t = &qb[qoff[q]];
        const int len = (int)(qoff[q + 1] - qoff[q]), e = edits[q];
        if (len == 0 || len > kMaxLen) continue;
        const size_t plen = std::min<size_t>(prefix_len, (size_t)len);
        // [lo, hi): the terms that start with the query's first plen bytes
        auto cmp = [&](uint32_t i) {   // sign of compare(term i truncated to plen bytes, prefix)
            const size_t tl = off[i + 1] - off[i], m = std::min(tl, plen);
            const int c = std::memcmp(&pool[off[i]], t, m);
            return c != 0 ? c : (tl >= plen ? 0 : -1);
        };
        uint32_t lo = 0, hi = n;
        if (plen) {
            uint32_t a = 0, b = n;
            while (a < b) { const uint32_t m = a + (b - a) / 2; if (cmp(m) < 0) a = m + 1; else b = m; }
            lo = a; b = n;
            while (a < b) { const uint32_t m = a + (b - a) / 2; if (cmp(m) <= 0) a = m + 1; else b = m; }
            hi = a;
        }
        uint64_t qsig = 0;
        for (int j = 0; j < len; j++) qsig |= sig_bit(t[j]);
        uint64_t best[10];
        std::fill(best, best + 10, kEmpty);
        for (int l = std::max(0, len - e); l <= len + e; l++) {
            const uint32_t* a = std::lower_bound(&perm[0] + len_start[l], &perm[0] + len_start[l + 1], lo);
            const uint32_t* b = std::lower_bound(a, (const uint32_t*)&perm[0] + len_start[l + 1], hi);
            pairs += (uint64_t)(b - a);
            for (const uint32_t* p = a; p < b; p++) {
                if (__builtin_popcountll((psig[p - &perm[0]] ^ qsig) & kSigBits) > 2 * e) continue;
                reached_dp++;
                const uint8_t* c = &pool[off[*p]];
                const uint32_t d = e == 0 ? osa_band<0>(t, len, c, l) : e == 1 ? osa_band<1>(t, len, c, l) : osa_band<2>(t, len, c, l);
                if (d > (uint32_t)e) continue;
                const uint64_t key = ((uint64_t)d << 62) | ((uint64_t)(~score[*p]) << 30) | *p;
                if (key >= best[L - 1]) continue;
                uint32_t r = L - 1;
                for (; r > 0 && best[r - 1] > key; r--) best[r] = best[r - 1];
                best[r] = key;
            }
        }
        for (uint32_t r = 0; r < L && best[r] != kEmpty; r++) {
            idx[(size_t)q * L + r] = (uint32_t)best[r] & ((1u << 30) - 1);
            dist[(size_t)q * L + r] = (uint8_t)(best[r] >> 62);
            count[q] = r + 1;
        }
    }
    const double scan_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    f = std::fopen(argv[2], "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    std::fwrite(idx.data(), 4, idx.size(), f);
    std::fwrite(dist.data(), 1, dist.size(), f);
    std::fwrite(count.data(), 4, count.size(), f);
    std::fclose(f);
    std::printf("{\"n\": %u, \"n_q\": %u, \"candidates\": %u, \"build_s\": %.6f, \"scan_s\": %.6f, \"pairs\": %llu, \"reached_dp\": %llu, \"pairs_per_s\": %.4g}\n",
                n, n_q, (uint32_t)perm.size(), build_s, scan_s, (unsigned long long)pairs, (unsigned long long)reached_dp,
                scan_s > 0 ? (double)((uint64_t)n_q * n) / scan_s : 0.0);
    return 0;
}
