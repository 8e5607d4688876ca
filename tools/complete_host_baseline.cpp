// One host thread doing what ns_ac_fuzzy_prefix does (csrc/ns_fuzzy.hip), with the same definition and the
// same filters: the candidates in a length-ordered permutation with a byte-set signature each (none for the bucket of
// terms past 66 bytes), the fixed prefix's index range per length bucket from n - e upwards, the one-sided signature test,
// then the banded DP of the PREFIX distance (rows over the query's bytes; the minimum over the last row's cells inside
// the candidate), and the best L by the key (distance, ~score, index).  The yardstick of tools/complete_bench.py, which
// also checks its answers equal to the device's.
//
//   make -C nextsearch-api_amd complete_host_baseline
//   complete_host_baseline <workload file> <answers file>       prints one JSON line: build and scan seconds, pairs, DP share
//   complete_host_baseline --self-test                          hand-made tables against the unbanded definition; prints "self-test OK"
//
// workload file (little-endian): u32 n, n_q, L, prefix_len | u64 offsets[n + 1] | pool | u32 scores[n] |
//                                u32 q_offsets[n_q + 1] | query bytes | u8 max_edits[n_q]
// answers file:                  u32 idx[n_q * L] | u8 dist[n_q * L] | u32 count[n_q]
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static constexpr int kMaxLen = 64, kBuckets = kMaxLen + 4;
static constexpr uint64_t kSigBits = (1ull << 37) - 1, kEmpty = ~0ull;

static uint64_t sig_bit(uint8_t c) {
    if (c >= '0' && c <= '9') return 1ull << (c - '0');
    if (c >= 'a' && c <= 'z') return 1ull << (10 + c - 'a');
    return 1ull << 36;
}

// min over j of D[n][j] of the query q[0, n) against c[0, m), m >= n - E, cells j = i - E .. i + E per row (only the cells
// with j <= m count, and no byte at or past c[m] is read); above E: some value above E
template <int E>
static uint32_t pd_band(const uint8_t* q, int n, const uint8_t* c, int m) {
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
    uint32_t d = kInf;
    for (int t = 0; t < B; t++) {
        const int j = n - E + t;
        if (j >= 0 && j <= m) d = std::min(d, p1[t]);
    }
    return d;
}

struct Workload {
    uint32_t n = 0, n_q = 0, L = 0, prefix_len = 0;
    std::vector<uint64_t> off;
    std::vector<uint8_t> pool;
    std::vector<uint32_t> score, qoff;
    std::vector<uint8_t> qb, edits;
};

struct Answers {
    std::vector<uint32_t> idx, count;
    std::vector<uint8_t> dist;
    uint64_t pairs = 0, reached_dp = 0;
    uint32_t candidates = 0;
    double build_s = 0, scan_s = 0;
};

static void run(const Workload& w, Answers& out);

// ---- the self test: hand-made tables against the definition, min over j of the full-table osa(q, c[0, j)) ----
static int osa_full(const std::string& a, const std::string& b) {
    const size_t n = a.size(), m = b.size();
    std::vector<std::vector<int>> d(n + 1, std::vector<int>(m + 1, 0));
    for (size_t i = 0; i <= n; i++) d[i][0] = (int)i;
    for (size_t j = 0; j <= m; j++) d[0][j] = (int)j;
    for (size_t i = 1; i <= n; i++)
        for (size_t j = 1; j <= m; j++) {
            int v = std::min({d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1])});
            if (i > 1 && j > 1 && a[i - 1] == b[j - 2] && a[i - 2] == b[j - 1]) v = std::min(v, d[i - 2][j - 2] + 1);
            d[i][j] = v;
        }
    return d[n][m];
}

static int pd_full(const std::string& q, const std::string& c) {
    int best = 1 << 20;
    for (size_t j = 0; j <= c.size(); j++) best = std::min(best, osa_full(q, c.substr(0, j)));
    return best;
}

static int self_test() {
    struct Pair { const char* q; std::string c; int pd; };
    const std::vector<Pair> pairs = {
        {"ca", "abc", 1}, {"abcd", "axxbcdzz", 2}, {"abxxcd", "abcd", 2}, {"abdc", "abcdef", 1}, {"ab", "bazz", 1}, {"abcd", "ab", 2},
        {"abcd", "abc", 1}, {"a", "zzzz", 1}, {"virsu", "viruses", 1}, {"cornoa", "coronavirus", 1}, {"abcd", "abcd" + std::string(300, 'x'), 0},
        {"abcde", "cdxxx", 3}};
    for (const Pair& p : pairs)
        if (pd_full(p.q, p.c) != p.pd) { std::fprintf(stderr, "self-test: pd(%s, %.20s) = %d, not %d\n", p.q, p.c.c_str(), pd_full(p.q, p.c), p.pd); return 1; }
    // tables: the pairs' terms, repeated strings, score 0, bytes outside [0-9a-z], lengths around 64 and far past it
    std::vector<std::string> terms = {"", "a", "ab", "ab", "abc", "abcd", "abcdef", "axxbcdzz", "bazz", "cd", "cdxxx", "coronavirus", "viruses", "zzzz",
                                      "A-b_9", "a0\xc3\xa9t", std::string(63, 'q'), std::string(64, 'q'), std::string(65, 'q'), std::string(66, 'q'),
                                      std::string(67, 'q'), std::string(80, 'q'), "abcd" + std::string(300, 'x'), std::string(70, 'q') + "r"};
    std::sort(terms.begin(), terms.end());
    const std::vector<std::string> queries = {"", "a", "ab", "ca", "abcd", "abxxcd", "abdc", "virsu", "cornoa", "abcde", "zz", "A-b9", "a0\xc3t",
                                              std::string(64, 'q'), std::string(65, 'q'), std::string(62, 'q') + "rq", std::string(40, 'q') + "x", "qqqr"};
    uint64_t checked = 0;
    for (int variant = 0; variant < 2; variant++) {
        for (uint32_t prefix_len : {0u, 1u, 3u, 100u}) {
            for (uint32_t L : {1u, 5u, 10u}) {
                Workload w;
                w.n = (uint32_t)terms.size(); w.L = L; w.prefix_len = prefix_len;
                w.off.push_back(0);
                for (size_t i = 0; i < terms.size(); i++) {
                    w.pool.insert(w.pool.end(), terms[i].begin(), terms[i].end());
                    w.off.push_back(w.pool.size());
                    w.score.push_back(variant == 0 ? 7u : (uint32_t)((i * 2654435761u) >> 29));   // 0..7: some score 0, many ties
                }
                w.qoff.push_back(0);
                for (const std::string& q : queries)
                    for (uint8_t e = 0; e <= 2; e++) {
                        w.qb.insert(w.qb.end(), q.begin(), q.end());
                        w.qoff.push_back((uint32_t)w.qb.size());
                        w.edits.push_back(e);
                    }
                w.n_q = (uint32_t)w.edits.size();
                Answers a;
                run(w, a);
                for (uint32_t qi = 0; qi < w.n_q; qi++) {
                    const std::string& q = queries[qi / 3];
                    const int e = w.edits[qi];
                    std::vector<uint64_t> want;
                    if (!q.empty() && q.size() <= (size_t)kMaxLen)
                        for (size_t i = 0; i < terms.size(); i++) {
                            if (w.score[i] == 0 || (i > 0 && terms[i] == terms[i - 1])) continue;
                            const size_t p = std::min<size_t>(prefix_len, q.size());
                            if (terms[i].compare(0, p, q, 0, p) != 0 || terms[i].size() < p) continue;
                            const int d = pd_full(q, terms[i]);
                            if (d <= e) want.push_back(((uint64_t)d << 62) | ((uint64_t)(~w.score[i]) << 30) | i);
                        }
                    std::sort(want.begin(), want.end());
                    if (want.size() > L) want.resize(L);
                    bool ok = a.count[qi] == want.size();
                    for (size_t r = 0; r < want.size() && ok; r++)
                        ok = a.idx[(size_t)qi * L + r] == (uint32_t)(want[r] & ((1u << 30) - 1)) && a.dist[(size_t)qi * L + r] == (uint8_t)(want[r] >> 62);
                    for (size_t r = want.size(); r < L && ok; r++) ok = a.idx[(size_t)qi * L + r] == ~0u && a.dist[(size_t)qi * L + r] == 0xff;
                    if (!ok) { std::fprintf(stderr, "self-test: query %u (edits %d, prefix_len %u, L %u, scores %d) differs\n", qi / 3, e, prefix_len, L, variant); return 1; }
                    checked++;
                }
            }
        }
    }
    std::printf("self-test OK: %zu hand-computed prefix distances, %llu answers on hand-made tables equal to the unbanded definition\n", pairs.size(),
                (unsigned long long)checked);
    return 0;
}

static void run(const Workload& w, Answers& out) {
    const uint32_t n = w.n, n_q = w.n_q, L = w.L, prefix_len = w.prefix_len;
    const std::vector<uint64_t>& off = w.off;
    const std::vector<uint8_t>&pool = w.pool, &qb = w.qb, &edits = w.edits;
    const std::vector<uint32_t>&score = w.score, &qoff = w.qoff;
    // ---- the side structures (ns_ac_build_fuzzy's: the bucket past 66 bytes keeps signature 0) ----
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> len_start(kBuckets + 1, 0), bucket(n);
    std::vector<uint8_t> cand(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t len = off[i + 1] - off[i];
        bucket[i] = (uint32_t)std::min<uint64_t>(len, kBuckets - 1);
        const bool dup = i > 0 && off[i] - off[i - 1] == len && std::memcmp(pool.data() + off[i - 1], pool.data() + off[i], len) == 0;
        cand[i] = score[i] != 0 && !dup;
        if (cand[i]) len_start[bucket[i] + 1]++;
    }
    for (int b = 0; b < kBuckets; b++) len_start[b + 1] += len_start[b];
    std::vector<uint32_t> perm(len_start[kBuckets]), next(len_start.begin(), len_start.end() - 1);
    std::vector<uint64_t> psig(perm.size());
    for (uint32_t i = 0; i < n; i++) {
        if (!cand[i]) continue;
        uint64_t s = 0;
        if (bucket[i] < (uint32_t)kBuckets - 1)
            for (uint64_t j = off[i]; j < off[i + 1]; j++) s |= sig_bit(pool[j]);
        perm[next[bucket[i]]] = i;
        psig[next[bucket[i]]++] = s;
    }
    out.candidates = (uint32_t)perm.size();
    out.build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    // ---- the scan ----
    out.idx.assign((size_t)n_q * L, ~0u);
    out.count.assign(n_q, 0);
    out.dist.assign((size_t)n_q * L, 0xff);
    const bool use_sig = !(std::getenv("NS_FUZZY_NO_SIG") && std::getenv("NS_FUZZY_NO_SIG")[0] == '1');
    const auto t1 = std::chrono::steady_clock::now();
    for (uint32_t q = 0; q < n_q; q++) {
        const uint8_t* t = qb.data() + qoff[q];
        const int len = (int)(qoff[q + 1] - qoff[q]), e = edits[q];
        if (len == 0 || len > kMaxLen) continue;
        const size_t plen = std::min<size_t>(prefix_len, (size_t)len);
        // [lo, hi): the terms that start with the query's first plen bytes
        auto cmp = [&](uint32_t i) {   // sign of compare(term i truncated to plen bytes, prefix)
            const size_t tl = off[i + 1] - off[i], m = std::min(tl, plen);
            const int c = m ? std::memcmp(pool.data() + off[i], t, m) : 0;
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
        for (int l = std::max(0, len - e); l < kBuckets; l++) {
            const uint32_t* base = perm.data();
            const uint32_t* a = std::lower_bound(base + len_start[l], base + len_start[l + 1], lo);
            const uint32_t* b = std::lower_bound(a, base + len_start[l + 1], hi);
            out.pairs += (uint64_t)(b - a);
            for (const uint32_t* p = a; p < b; p++) {
                const uint64_t cs = psig[p - base];
                // a byte class of the query that the candidate lacks costs an edit of its own; no signature: no test
                if (use_sig && cs != 0 && __builtin_popcountll(qsig & ~cs & kSigBits) > e) continue;
                out.reached_dp++;
                const uint8_t* c = pool.data() + off[*p];
                const int m = (int)std::min<uint64_t>(off[*p + 1] - off[*p], (uint64_t)len + 2);   // no cell past column n + e is read
                const uint32_t d = e == 0 ? pd_band<0>(t, len, c, m) : e == 1 ? pd_band<1>(t, len, c, m) : pd_band<2>(t, len, c, m);
                if (d > (uint32_t)e) continue;
                const uint64_t key = ((uint64_t)d << 62) | ((uint64_t)(~score[*p]) << 30) | *p;
                if (key >= best[L - 1]) continue;
                uint32_t r = L - 1;
                for (; r > 0 && best[r - 1] > key; r--) best[r] = best[r - 1];
                best[r] = key;
            }
        }
        for (uint32_t r = 0; r < L && best[r] != kEmpty; r++) {
            out.idx[(size_t)q * L + r] = (uint32_t)best[r] & ((1u << 30) - 1);
            out.dist[(size_t)q * L + r] = (uint8_t)(best[r] >> 62);
            out.count[q] = r + 1;
        }
    }
    out.scan_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "--self-test") == 0) return self_test();
    if (argc < 3) { std::fprintf(stderr, "usage: %s <workload file> <answers file> | --self-test\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    Workload w;
    uint32_t hdr[4];
    bool ok = std::fread(hdr, 4, 4, f) == 4;
    w.n = hdr[0]; w.n_q = hdr[1]; w.L = hdr[2]; w.prefix_len = hdr[3];
    const uint32_t n = ok ? w.n : 0, n_q = ok ? w.n_q : 0;
    w.off.resize((size_t)n + 1);
    ok = ok && std::fread(w.off.data(), 8, (size_t)n + 1, f) == (size_t)n + 1;
    w.pool.resize(ok ? w.off[n] : 0);
    ok = ok && std::fread(w.pool.data(), 1, w.pool.size(), f) == w.pool.size();
    w.score.resize(n);
    w.qoff.resize((size_t)n_q + 1);
    ok = ok && std::fread(w.score.data(), 4, n, f) == n && std::fread(w.qoff.data(), 4, (size_t)n_q + 1, f) == (size_t)n_q + 1;
    w.qb.resize(ok ? w.qoff[n_q] : 0);
    w.edits.resize(n_q);
    ok = ok && std::fread(w.qb.data(), 1, w.qb.size(), f) == w.qb.size() && std::fread(w.edits.data(), 1, n_q, f) == n_q;
    std::fclose(f);
    if (!ok || w.L < 1 || w.L > 10) { std::fprintf(stderr, "%s: short or malformed\n", argv[1]); return 1; }
    for (uint32_t q = 0; q < n_q; q++)
        if (w.edits[q] > 2) { std::fprintf(stderr, "%s: max_edits above 2\n", argv[1]); return 1; }
    Answers a;
    run(w, a);
    f = std::fopen(argv[2], "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    std::fwrite(a.idx.data(), 4, a.idx.size(), f);
    std::fwrite(a.dist.data(), 1, a.dist.size(), f);
    std::fwrite(a.count.data(), 4, a.count.size(), f);
    std::fclose(f);
    std::printf("{\"n\": %u, \"n_q\": %u, \"candidates\": %u, \"build_s\": %.6f, \"scan_s\": %.6f, \"pairs\": %llu, \"reached_dp\": %llu, \"pairs_per_s\": %.4g}\n",
                n, n_q, a.candidates, a.build_s, a.scan_s, (unsigned long long)a.pairs, (unsigned long long)a.reached_dp,
                a.scan_s > 0 ? (double)a.pairs / a.scan_s : 0.0);
    return 0;
}
