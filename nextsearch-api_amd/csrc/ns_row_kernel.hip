// k_rscore — the consumer of "shared top rows" (ns_ctx_share_rows).
//
// A thin group is one hot list H plus tail lists.  The batch ranks H once per cell of its doc space — producer items, plain
// single-term items of the scoring launch's own instantiation with K' = kRowLen, one result row each in the batch's row
// buffer — and every thin group that names H with the same idf and weight is cut into those cells.  One WAVE scores one
// such item with the driver-stream body in its ROW form (ns_driver_kernel.hip): windows, table, accumulation passes,
// read-back and top-K as ever; H itself is looked up by docId for the tails' docs and otherwise read from the row.
// An item whose row cannot prove the result (too many of its entries are docs of the tails) runs the streaming body over
// the same item, once, in the same wave; stats[0] counts those, stats[1] the row entries that hit the table.
// Ordering against the producers is by stream and event only (ns_batch_run); no flag is read or written here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ns_driver_kernel.hip"

namespace ns {

template <int HK, int CB, int TMAX>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 8))) k_rscore(const DevRItem* __restrict__ items, uint32_t n_items,
                                                const DevTerm* __restrict__ terms, const DevSeg* __restrict__ segs,
                                                const Hit* __restrict__ row_hits, const uint32_t* __restrict__ row_nhits,
                                                Hit* __restrict__ out_hits, uint32_t* __restrict__ out_nhits,
                                                uint64_t* __restrict__ out_found, uint32_t K, uint32_t* __restrict__ stats) {
    __shared__ __attribute__((aligned(16))) uint32_t s_tbl[2 * HK];   // HK / 2 buckets of 4 entries
    __shared__ __attribute__((aligned(16))) float s_vals[64];
    __shared__ __attribute__((aligned(16))) uint8_t s_mcnt[16];
    __shared__ uint64_t s_cand[CB];
    __shared__ __attribute__((aligned(16))) uint4 s_tab[TMAX];
    __shared__ uint32_t s_aux[TMAX];
    const int lane = threadIdx.x & 63;
    const uint32_t item_idx = blockIdx.x;
    if (item_idx >= n_items) return;
    const DevRItem ri = items[item_idx];
    DevWItem it = ri.it;
    it.whole &= 121u;   // as k_uscore: whole segment, short division, signed inputs, skip grid
    RowArgs ra;
    ra.hits = row_hits + (size_t)ri.row * kRowLen;
    ra.nhits = row_nhits[ri.row];
    ra.dterm = ri.dterm;
    ra.stats = stats;
    if (dscore_body<HK / 2, 64, false, CB, true, 0, true>(it, terms, segs, s_tbl, s_vals, s_mcnt, s_cand, s_tab, s_aux, out_hits, out_nhits,
                                                          out_found, K, lane, ra))
        return;
    if (lane == 0) atomicAdd(stats, 1u);
    wave_sync();
    dscore_body<HK / 2, 64, false, CB, true, 0, false>(it, terms, segs, s_tbl, s_vals, s_mcnt, s_cand, s_tab, s_aux, out_hits, out_nhits,
                                                       out_found, K, lane);
}

}  // namespace ns
