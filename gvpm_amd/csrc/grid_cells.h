// What the two builds of the photon grid share: the stripes of a bundle cell's counter and pass Y of the summed-volume table.
// Included by grid_build.hip (cell_count_kernel, sat_y_kernel) and build_chain.hip (chain_count_kernel, chain_mid_kernel).
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"

namespace gvpm {

// Counters a bundle cell's count is split into (cell_count_kernel, grid_build.hip, says why).  One value for every unit: the
// counting kernels, the scatter and the host's buffer size (cell_stripes()) must agree.
// (C4, a rank of 8: 4 / 8 / 16 / 32 stripes: 2.57 / 2.58 / 2.48 / 2.55 ms per step; one counter: 2.75)
constexpr uint32_t CELL_STRIPES = 16;

// pass Z of the summed-volume table (sat_z_kernel, grid_build.hip): launch_sat's second launch and the chain's fifth
void launch_sat_z(const Grid &g, uint32_t *sat, hipStream_t s);

// pass Y of the summed-volume table for thread t (sat_y_kernel, grid_build.hip, has the table's layout)
__device__ __forceinline__ void satYBody(const uint32_t *__restrict__ cellStart, const Grid &g, uint32_t *__restrict__ sat, uint32_t t) {
  const uint32_t nx1 = g.dim[0] + 1, ny1 = g.dim[1] + 1;
  if (t >= nx1 * (uint32_t)g.dim[2]) return;
  const uint32_t x = t % nx1, z = t / nx1;
  uint32_t run = 0;
  sat[((size_t)z * ny1 + 0) * nx1 + x] = 0u;
#pragma unroll 8
  for (int y = 0; y < g.dim[1]; ++y) {
    const size_t row = ((size_t)z * g.dim[1] + y) * g.dim[0];
    run += cellStart[row + x] - cellStart[row];
    sat[((size_t)z * ny1 + (y + 1)) * nx1 + x] = run;
  }
}

}  // namespace gvpm
