// The host-side radix sort and exclusive scan of scan_sort.hip, the only unit that includes hipCUB.
// Included by context.h (the gather drivers) and by synth_device.hip (the device generator's compactions).
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"

namespace gvpm {
hipError_t sortPairsU32(SortTemp &tmp, const uint32_t *kIn, uint32_t *kOut, const uint32_t *vIn, uint32_t *vOut,
                        uint32_t n, int endBit, hipStream_t s);
hipError_t reserveScanTemp(SortTemp &tmp, uint32_t n);
hipError_t exclusiveSumU32(SortTemp &tmp, const uint32_t *in, uint32_t *out, uint32_t n, hipStream_t s);
}  // namespace gvpm
