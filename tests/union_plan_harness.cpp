// Stand-alone host program (its own main; no HIP, no device): what ns_segment_union plans before it touches the device
// (csrc/ns_union_plan.hpp), built by tests/test_prefix_cpu.py with -fsanitize=address,undefined and run on the CPU.  Exit status 0
// and "union plan check OK" when every expectation holds.
#include <cstdio>
#include <numeric>
#include <set>
#include <vector>

#include "ns_union_plan.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

struct Input {
    std::vector<uint32_t> first, cnt, gb{0};
    void group(std::initializer_list<std::pair<uint32_t, uint32_t>> members) {
        for (const auto& m : members) { first.push_back(m.first); cnt.push_back(m.second); }
        gb.push_back((uint32_t)first.size());
    }
    uint32_t n_groups() const { return (uint32_t)gb.size() - 1; }
    ns::UnionPlan plan(uint32_t n_docs, uint64_t scratch) const { return ns::union_plan(first.data(), cnt.data(), gb.data(), n_groups(), n_docs, scratch); }
};

// the items of one member cover [first, first + count) once, in order, 64 at a time, the last one partial
template <class Item>
static void covers(const std::vector<Item>& items, size_t from, size_t to, uint32_t first, uint32_t count) {
    EXPECT(to - from == (count + 63) / 64);
    uint32_t at = first;
    for (size_t i = from; i < to && i < items.size(); i++) {
        EXPECT(items[i].src == at && items[i].n >= 1 && items[i].n <= 64);
        EXPECT(i + 1 == to ? items[i].n == first + count - at : items[i].n == 64);
        at += items[i].n;
    }
    EXPECT(at == first + count);
}

static void wave_items() {
    // members of 0, 1, 63, 64, 65 and 129 postings: as the members of one multi group, and each as a single group
    const uint32_t sizes[6] = {0, 1, 63, 64, 65, 129};
    Input in;
    in.group({{1000, 0}, {2000, 1}, {3000, 63}, {4000, 64}, {5000, 65}, {6000, 129}});
    for (uint32_t i = 0; i < 6; i++) in.group({{100 * i, sizes[i]}});
    const ns::UnionPlan p = in.plan(500, ns::kUnDefaultScratch);
    EXPECT(p.tabled.size() == 1 && p.tabled[0] == 0 && p.rounds.size() == 1);
    EXPECT(p.rounds[0].first_table == 0 && p.rounds[0].n_tables == 1 && p.rounds[0].first_item == 0 && p.rounds[0].n_items == p.add_items.size());
    EXPECT(p.add_items.size() == 0 + 1 + 1 + 1 + 2 + 3);
    size_t at = 0;
    for (uint32_t i = 0; i < 6; i++) {
        const size_t n = (sizes[i] + 63) / 64;
        covers(p.add_items, at, at + n, 1000 * (i + 1), sizes[i]);
        at += n;
    }
    for (const ns::UnAddItem& it : p.add_items) EXPECT(it.table == 0);
    // the singles: packed back to back in group order from 0; their copy items mirror the add items
    EXPECT(p.copy_items.size() == 8 && p.single_postings == 322);
    uint32_t off = 0;
    at = 0;
    for (uint32_t i = 0; i < 6; i++) {
        EXPECT(p.single_off[1 + i] == off);
        const size_t n = (sizes[i] + 63) / 64;
        covers(p.copy_items, at, at + n, 100 * i, sizes[i]);
        for (size_t j = at; j < at + n; j++) EXPECT(p.copy_items[j].dst == off + (p.copy_items[j].src - 100 * i));
        at += n;
        off += sizes[i];
    }
    EXPECT(p.single_off[0] == 0);
    // the bound: the singles whole, the multi group min(sum, n_docs)
    EXPECT(p.bound == 322 + 322);
    EXPECT(in.plan(300, ns::kUnDefaultScratch).bound == 322 + 300);
    EXPECT(in.plan(1, ns::kUnDefaultScratch).bound == 322 + 1);
}

static void rounds() {
    for (const uint32_t n_docs : {1u, 64u, 4099u}) {
        const uint64_t one = (uint64_t)n_docs * 4;
        for (const uint32_t multi : {1u, 2u, 5u}) {
            Input in;
            in.group({});                                          // empty
            for (uint32_t g = 0; g < multi; g++) {
                in.group({{10 * g, 3}, {10 * g + 5, 70}});
                in.group({{7, 9}});                                // a single between them
                in.group({{0, 0}, {50, 0}});                       // a multi group without a posting: no table, no round
            }
            struct Case { uint64_t scratch; uint32_t per_round; } cases[] = {{one, 1}, {2 * one, 2}, {one - 1, 1}, {0, 1}, {2 * one + one - 1, 2}, {100 * one, 100}};
            for (const Case& c : cases) {
                const ns::UnionPlan p = in.plan(n_docs, c.scratch);
                EXPECT(p.tables_per_round == c.per_round);
                EXPECT(p.tabled.size() == multi);
                EXPECT(p.rounds.size() == (multi + c.per_round - 1) / c.per_round);
                uint32_t tables = 0, items = 0;
                for (size_t r = 0; r < p.rounds.size(); r++) {
                    const ns::UnRound& rd = p.rounds[r];
                    EXPECT(rd.first_table == tables && rd.first_item == items);
                    EXPECT(rd.n_tables >= 1 && rd.n_tables <= c.per_round && (r + 1 == p.rounds.size() || rd.n_tables == c.per_round));
                    EXPECT(rd.n_items == rd.n_tables * 3);       // 3 postings: one item; 70: two
                    for (uint32_t i = 0; i < rd.n_items; i++) {
                        const ns::UnAddItem& it = p.add_items[rd.first_item + i];
                        EXPECT(it.table == i / 3);                 // tables count from 0 in every round, in group order
                        const uint32_t g = (rd.first_table + it.table);
                        EXPECT(it.src >= 10 * g && it.src < 10 * g + 75);
                    }
                    tables += rd.n_tables;
                    items += rd.n_items;
                }
                EXPECT(tables == multi && items == p.add_items.size());
                for (uint32_t t = 0; t < multi; t++) EXPECT(p.tabled[t] == 1 + 3 * t);
                EXPECT(p.single_postings == 9ull * multi && p.copy_items.size() == multi);
                EXPECT(p.bound == 9ull * multi + (uint64_t)multi * std::min<uint64_t>(73, n_docs));
            }
        }
    }
    EXPECT(ns::union_tables_per_round(ns::kUnDefaultScratch, 1u << 20) == 16);
    EXPECT(ns::union_tables_per_round(ns::kUnDefaultScratch, 0) == (64u << 20) / 4);
    EXPECT(ns::union_tables_per_round(1, 0xFFFFFFFFu) == 1);
    // nothing at all, and a segment without documents: no table, no round
    Input none;
    const ns::UnionPlan p0 = none.plan(10, ns::kUnDefaultScratch);
    EXPECT(p0.rounds.empty() && p0.copy_items.empty() && p0.add_items.empty() && p0.bound == 0 && p0.single_off.empty());
    Input nodocs;
    nodocs.group({{0, 5}, {5, 5}});
    nodocs.group({{0, 5}});
    const ns::UnionPlan p1 = nodocs.plan(0, ns::kUnDefaultScratch);
    EXPECT(p1.rounds.empty() && p1.tabled.empty() && p1.bound == 5 && p1.copy_items.size() == 1);
}

int main() {
    wave_items();
    rounds();
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("union plan check OK");
    return 0;
}
