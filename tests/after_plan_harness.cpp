// C entry points over csrc/ns_after_plan.hpp for tests/test_after_cpu.py (built by g++ inside the test; no HIP, no device).
// With -DAFTER_PLAN_MAIN it is a program of its own that walks the same grid of inputs against a comparison written out
// in full, for a run under the host sanitizers.
#include <cstdint>
#include <cstdio>

#include "ns_after_plan.hpp"

extern "C" {

uint64_t after_last_c(uint32_t rank_mapped, uint32_t cursor_pos, uint32_t cursor_doc, uint32_t item_pos, uint32_t doc_lo, uint32_t doc_hi) {
    return ns::after_last(rank_mapped, cursor_pos, cursor_doc, item_pos, doc_lo, doc_hi);
}

// n cases at once: in[i * 6 ..] = the six arguments
void after_last_many(const uint32_t* in, uint64_t n, uint64_t* out) {
    for (uint64_t i = 0; i < n; i++) out[i] = ns::after_last(in[i * 6], in[i * 6 + 1], in[i * 6 + 2], in[i * 6 + 3], in[i * 6 + 4], in[i * 6 + 5]);
}

uint64_t after_all(void) { return ns::kAfterAll; }
uint32_t after_ord_c(uint32_t bits) { return ns::after_ord(bits); }
uint32_t after_sort_rank_c(uint32_t key, int asc) { return ns::after_sort_rank(key, asc != 0); }
int after_in_tile_c(uint64_t last) { return ns::after_in_tile(last) ? 1 : 0; }

}  // extern "C"

#ifdef AFTER_PLAN_MAIN
// strictly after the cursor, on (rank descending, position ascending, docId ascending)
static bool strictly_after(uint32_t r, uint32_t pos, uint32_t doc, uint32_t cr, uint32_t cpos, uint32_t cdoc) {
    if (r != cr) return r < cr;
    if (pos != cpos) return pos > cpos;
    return doc > cdoc;
}

int main() {
    const uint32_t ranks[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    const uint32_t tiles[][2] = {{0u, 32u}, {128u, 256u}, {1u << 17, 1u << 18}};
    unsigned long long cases = 0, bad = 0;
    for (uint32_t cr : ranks)
        for (uint32_t cpos = 4; cpos <= 6; cpos++)                      // the item sits at position 5
            for (const auto& t : tiles) {
                const uint32_t lo = t[0], hi = t[1];
                const uint32_t docs[] = {0u, lo - 1u, lo, lo + 1u, hi - 2u, hi - 1u, hi, 0xFFFFFFFFu};
                for (uint32_t cdoc : docs) {
                    const uint64_t last = ns::after_last(cr, cpos, cdoc, 5u, lo, hi);
                    for (uint32_t d = lo; d < hi; d++)
                        for (int dr = -1; dr <= 1; dr++) {
                            if ((dr < 0 && cr == 0u) || (dr > 0 && cr == 0xFFFFFFFFu)) continue;
                            const uint32_t r = cr + (uint32_t)dr;
                            const uint64_t key = ((uint64_t)r << 32) | (uint32_t)~(d - lo);
                            cases++;
                            if ((key <= last) != strictly_after(r, 5u, d, cr, cpos, cdoc)) bad++;
                        }
                }
            }
    std::printf("after_plan_harness: %llu cases, %llu wrong\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
