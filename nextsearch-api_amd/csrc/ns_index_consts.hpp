// The sizes that the index-building kernels (ns_invert.hip, ns_compact.hip) share with the host-only plans of their calls
// (ns_radix_plan.hpp, ns_merge_plan.hpp).  Host and device: plain constants, no HIP type.
#pragma once
#include <cstdint>

namespace ns {

constexpr int kIvItems = 16;                 // pairs per thread per tile
constexpr int kIvTile = 256 * kIvItems;      // pairs per workgroup of the radix sort (ns_radix_tile() hands it to the tests)

constexpr uint32_t kCpWaveMax = 64;       // pairs of a document sorted by one wave
// pairs of a document sorted in LDS by one workgroup: 32 KiB of 64-bit keys, so that four workgroups stay resident on a
// CU's 160 KiB (ns_compact_doc_cut() hands it to the tests)
constexpr uint32_t kCpDocCut = 4096;

}  // namespace ns
