// The tile of the three-kernel exclusive scan and the scan of one 256-thread block.
// Included by scan_sort.hip (exclusiveSumU32) and build_chain.hip (K2 / K3: the chain's one scan over [cells | beam keys]).
#pragma once
#include <hip/hip_runtime.h>

#include "vec.h"

namespace gvpm {

constexpr uint32_t SCAN_BLOCK = 256, SCAN_PER_THREAD = 8, SCAN_TILE = SCAN_BLOCK * SCAN_PER_THREAD;
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t *lds, uint32_t &total) {
  // 256 threads = 4 waves: wave scan, then the 4 wave totals
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t incl = wave_scan_incl(v, lane);
  if (lane == 63) lds[wv] = incl;
  __syncthreads();
  uint32_t base = 0;
  for (int k = 0; k < wv; ++k) base += lds[k];
  total = lds[0] + lds[1] + lds[2] + lds[3];
  __syncthreads();
  return base + incl - v;
}

}  // namespace gvpm
