// The two host-driven primitives every build is made with: a radix sort of (key, value) pairs (hipCUB) and an exclusive
// prefix sum in three plain kernels.  Both work in the caller's SortTemp, which grows to a high-water mark and is then
// reused; this is the only unit that includes hipCUB.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "device_types.h"
#include "scan_block.h"
#include "scan_sort.h"
#include "vec.h"

namespace gvpm {

static hipError_t ensureTemp(SortTemp &t, size_t need) {
  if (need <= t.bytes) return hipSuccess;
  if (t.d) (void)hipFree(t.d);
  t.d = nullptr;
  t.bytes = 0;
  hipError_t e = hipMalloc(&t.d, need);
  if (e == hipSuccess) t.bytes = need;
  return e;
}

// (The size query is a full host-side pass of the library's dispatch -- ~240 us, device properties included -- and the G-Beams
// step paid it twice per sort with the GPU idle behind it: asked once per high-water mark, for 1.25 x the count.)
hipError_t sortPairsU32(SortTemp &tmp, const uint32_t *kIn, uint32_t *kOut, const uint32_t *vIn, uint32_t *vOut,
                        uint32_t n, int endBit, hipStream_t s) {
  if (n > tmp.sortN || tmp.sortNeed == 0) {
    const uint32_t nq = (uint32_t)std::min<uint64_t>((uint64_t)n + n / 4u + 1024u, 0x7FFFFFF0u);
    size_t need = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, need, kIn, kOut, vIn, vOut, (int)nq, 0, 32, s);
    if (e != hipSuccess) return e;
    tmp.sortN = nq;
    tmp.sortNeed = std::max(need, tmp.sortNeed);
  }
  hipError_t e = ensureTemp(tmp, tmp.sortNeed);
  if (e != hipSuccess) return e;
  size_t have = tmp.bytes;
  return hipcub::DeviceRadixSort::SortPairs(tmp.d, have, kIn, kOut, vIn, vOut, (int)n, 0, endBit, s);
}

// make the temporary large enough for scans of up to n elements (so that no scan of a step allocates)
hipError_t reserveScanTemp(SortTemp &tmp, uint32_t n) {
  return ensureTemp(tmp, ((size_t)n / 2048 + 2) * sizeof(uint32_t) + 256);
}

// Exclusive prefix sum in three plain kernels: block sums, their scan by one block, down-sweep.  (hipCUB's single-pass
// scan makes every block look back at its predecessors' flags: beside the persistent evaluation waves of the previous
// step, which hold most of the chip until they finish, those predecessors are often not resident yet -- the two scans of
// a G-BRE build, 50 us each alone, took 260 us each in the pipelined run.  Nothing here waits for another block.)
__global__ __launch_bounds__(256) void scan_reduce_kernel(const uint32_t *__restrict__ in, uint32_t n, uint32_t *blockSum) {
  __shared__ uint32_t lds[4];
  const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_PER_THREAD;
  uint32_t v = 0;
#pragma unroll
  for (uint32_t k = 0; k < SCAN_PER_THREAD; ++k)
    if (base + k < n) v += in[base + k];
  uint32_t total;
  (void)block_scan_excl(v, lds, total);
  if (threadIdx.x == 0) blockSum[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void scan_spine_kernel(uint32_t *blockSum, uint32_t nblocks) {
  __shared__ uint32_t lds[4];
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < nblocks; b0 += SCAN_BLOCK) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t v = i < nblocks ? blockSum[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_scan_excl(v, lds, total);
    if (i < nblocks) blockSum[i] = carry + ex;
    carry += total;
  }
}
__global__ __launch_bounds__(256) void scan_down_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t n,
                                                        const uint32_t *__restrict__ blockSum) {
  __shared__ uint32_t lds[4];
  const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_PER_THREAD;
  uint32_t x[SCAN_PER_THREAD], v = 0;
#pragma unroll
  for (uint32_t k = 0; k < SCAN_PER_THREAD; ++k) {
    x[k] = base + k < n ? in[base + k] : 0u;
    v += x[k];
  }
  uint32_t total;
  uint32_t run = blockSum[blockIdx.x] + block_scan_excl(v, lds, total);
#pragma unroll
  for (uint32_t k = 0; k < SCAN_PER_THREAD; ++k) {
    if (base + k < n) out[base + k] = run;  // (in == out is fine: every thread has read its own eight before it writes)
    run += x[k];
  }
}
hipError_t exclusiveSumU32(SortTemp &tmp, const uint32_t *in, uint32_t *out, uint32_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint32_t nblocks = (n + SCAN_TILE - 1) / SCAN_TILE;
  hipError_t e = ensureTemp(tmp, (size_t)nblocks * sizeof(uint32_t) + 256);
  if (e != hipSuccess) return e;
  uint32_t *blockSum = reinterpret_cast<uint32_t *>(tmp.d);
  hipLaunchKernelGGL(scan_reduce_kernel, dim3(nblocks), dim3(SCAN_BLOCK), 0, s, in, n, blockSum);
  hipLaunchKernelGGL(scan_spine_kernel, dim3(1), dim3(SCAN_BLOCK), 0, s, blockSum, nblocks);
  hipLaunchKernelGGL(scan_down_kernel, dim3(nblocks), dim3(SCAN_BLOCK), 0, s, in, out, n, blockSum);
  return hipGetLastError();
}

}  // namespace gvpm
