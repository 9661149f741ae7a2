// Device-side acceleration-structure build for gfx950.
//
// Replaces GPhotonMap::build() (PointKDTree sliding midpoint, serial on the CPU;
// gvpm/gvpm_accel.h:201-203, include/mitsuba/core/kdtree.h:326-395) and the
// GradientBeamRadianceEstimator constructor (gvpm/gvpm_accel.cpp:10-54).  Every
// photon of a BRE pass has the same radius (gvpm.cpp:989,  gvpm_accel.cpp:27), so a
// uniform grid sorted by cell index (x fastest) gives x-contiguous photon ranges
// for any axis-aligned cell box -- the access pattern the gather kernel streams.
//
// Also orders the camera beam sets by image tile so that one wave works on a
// coherent bundle of beams (the role of BlockScheduler's image blocks,
// photonmapper/utilities/block_sched.h:19-136): segment_start_kernel here, the tile keys and the counting sort in
// beams_build.hip.
//
// This unit holds the step-by-step build.  The scans and the radix sort it is driven with are scan_sort.hip's, G-Beams'
// photon-beam records beams_build.hip's, and G-BRE's six-launch chain, which reuses reorderBody and satYBody, build_chain.hip's.
#include <hip/hip_runtime.h>

#include "bundle_grid.h"
#include "device_types.h"
#include "shift_device.h"
#include "tile_walk.h"
#include "vec.h"
#include "grid_cells.h"
#include "photon_scatter.h"

namespace gvpm {

// ---- bounds: per-block min/max of the photon positions -----------------------------------
__global__ __launch_bounds__(256) void bounds_kernel(const float *__restrict__ pos, uint32_t n, float *partial) {
  __shared__ float red[6][4];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = pos[3 * (size_t)i + c];
      mn[c] = fminf(mn[c], v);
      mx[c] = fmaxf(mx[c], v);
    }
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = wave_min(mn[c]), b = wave_max(mx[c]);
    if (lane == 0) {
      red[c][wave] = a;
      red[3 + c][wave] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int c = threadIdx.x;
    float v = red[c][0];
    for (int w = 1; w < (int)(blockDim.x / 64u); ++w) v = c < 3 ? fminf(v, red[c][w]) : fmaxf(v, red[c][w]);
    partial[blockIdx.x * 6 + c] = v;
  }
}

// hostOut (optional): device-visible pinned host memory -- the result lands there without a copy
// operation in the stream (copy engines and the streams' kernels do not overlap reliably)
// (word / wordOut, optional: one more 32-bit value for the host -- G-VPM's largest scale rides along instead of a launch of its own)
__global__ void bounds_final_kernel(const float *partial, int nblocks, float *out6, float *hostOut, const uint32_t *word,
                                    uint32_t *wordOut) {
  const int lane = threadIdx.x;  // one wave
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = lane; b < nblocks; b += 64)
    for (int c = 0; c < 3; ++c) {
      lo[c] = fminf(lo[c], partial[b * 6 + c]);
      hi[c] = fmaxf(hi[c], partial[b * 6 + 3 + c]);
    }
  for (int c = 0; c < 3; ++c) {
    lo[c] = wave_min(lo[c]);
    hi[c] = wave_max(hi[c]);
  }
  if (lane == 0)
    for (int c = 0; c < 3; ++c) {
      out6[c] = lo[c];
      out6[3 + c] = hi[c];
      if (hostOut) {
        hostOut[c] = lo[c];
        hostOut[3 + c] = hi[c];
      }
    }
  if (lane == 0 && word && wordOut) wordOut[0] = word[0];
}

// counters -> pinned host memory (same reason)
__global__ void export_u32_kernel(const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d,
                                  const uint32_t *e, uint32_t *hostOut) {
  if (threadIdx.x == 0) {
    hostOut[0] = a ? *a : 0u;
    hostOut[1] = b ? *b : 0u;
    hostOut[2] = c ? *c : 0u;
    hostOut[3] = d ? *d : 0u;
    hostOut[4] = e ? *e : 0u;
    __threadfence_system();
  }
}

// ---- cell keys ---------------------------------------------------------------------------

// counting sort, pass 1: key of every photon, its arrival rank within the cell, photons per cell
// `stripes` (bundle cells): the counter of cell k is split into CELL_STRIPES counters, stripe s at sub[s * ncells + k], and
// photon i counts in stripe i % CELL_STRIPES.  Image-space cells are far from equally filled (every photon around a light
// seen by the camera shares a handful of them) and atomics on one address retire ~11 ns apart: 4 M photons took 0.53 ms
// through one counter per cell (0.21 ms through the 3D grid's, < 0.03 ms with the atomic compiled out).
// cell_stripes_kernel then turns the stripes into exclusive prefixes within the cell and writes the cell's total to count[].
// (zeroWord / oneWord, optional: the near lists' overflow counter and the cursor of their extension lists, which the scatter
// behind this kernel starts from 0 and 1 -- two memsets less in the build chain)
__global__ __launch_bounds__(256) void cell_count_kernel(const float *__restrict__ pos, uint32_t n, Grid g,
                                                         uint32_t *keys, uint32_t *rank, uint32_t *count, uint32_t *sub,
                                                         uint32_t *zeroWord, uint32_t *oneWord) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    if (zeroWord) *zeroWord = 0u;
    if (oneWord) *oneWord = 1u;
  }
  if (i >= n) return;
  uint32_t k;
  if (g.mode == 1) {
    k = bundlePhotonKey(g, pos[3 * (size_t)i + 0], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]);
    keys[i] = k;
    // a photon no ray of the bundle can meet is not sorted at all (no box reaches the dump cell; reorder_kernel skips it)
    if (k == GVPM_BUNDLE_DUMP_CELL(g.dim[0])) rank[i] = 0xFFFFFFFFu;
    else if (sub) rank[i] = atomicAdd(&sub[(size_t)(i % CELL_STRIPES) * g.ncells + k], 1u);
    else rank[i] = atomicAdd(&count[k], 1u);
    return;
  }
  const int cx = cellCoord(pos[3 * (size_t)i + 0], g.org[0], g.invCell, g.dim[0]);
  const int cy = cellCoord(pos[3 * (size_t)i + 1], g.org[1], g.invCell, g.dim[1]);
  const int cz = cellCoord(pos[3 * (size_t)i + 2], g.org[2], g.invCell, g.dim[2]);
  k = ((uint32_t)cz * g.dim[1] + cy) * g.dim[0] + cx;
  keys[i] = k;
  rank[i] = atomicAdd(&count[k], 1u);
}
__global__ __launch_bounds__(256) void cell_stripes_kernel(uint32_t *sub, uint32_t ncells, uint32_t *count) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ncells) return;
  uint32_t run = 0;
#pragma unroll
  for (uint32_t st = 0; st < CELL_STRIPES; ++st) {
    const uint32_t c = sub[(size_t)st * ncells + k];
    sub[(size_t)st * ncells + k] = run;
    run += c;
  }
  count[k] = run;
}

// ---- summed-volume table over the cell counts: T(x,y,z) = photons in cells {x' < x, y' < y, z' < z},
// (dimx+1)(dimy+1)(dimz+1) entries, x fastest.  The planner counts the photons of a cell box with 8
// reads instead of two per cell row.
// pass Y: S1(x,y,z) = sum_{y' < y} rowPrefix(x,y',z), one thread per (x,z); the row prefixes come
// straight from cellStart (an exclusive prefix in x-fastest order)
__global__ __launch_bounds__(256) void sat_y_kernel(const uint32_t *__restrict__ cellStart, Grid g, uint32_t *sat) {
  satYBody(cellStart, g, sat, blockIdx.x * blockDim.x + threadIdx.x);
}
// pass Z (in place): T(x,y,z) = sum_{z' < z} S1(x,y,z'), one thread per (x,y)
__global__ __launch_bounds__(256) void sat_z_kernel(Grid g, uint32_t *sat) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nx1 = g.dim[0] + 1, ny1 = g.dim[1] + 1;
  if (t >= nx1 * ny1) return;
  const size_t layer = (size_t)nx1 * ny1;
  uint32_t run = 0;
#pragma unroll 8
  for (int z = 0; z < g.dim[2]; ++z) {
    const uint32_t v = sat[(size_t)z * layer + t];
    sat[(size_t)z * layer + t] = run;
    run += v;
  }
  sat[(size_t)g.dim[2] * layer + t] = run;
}

// ---- reorder: SoA upload layout -> sorted hot/cold planes (reorderBody, photon_scatter.h) ----
template <int MODE>
__global__ __launch_bounds__(64) void reorder_kernel(RawPhotons r, const uint32_t *__restrict__ keys,
                                                      const uint32_t *__restrict__ rank,
                                                      const uint32_t *__restrict__ cellStart, uint32_t n,
                                                      gvpm_params cfg, const float4 *bvh, const float4 *tri4,
                                                      uint32_t ntri, float dmax, NearGrid ng, uint32_t *nearExt,
                                                      uint32_t extCap, float4 *hot, float4 *cold, uint32_t *overflow,
                                                      uint32_t *origIdx, const uint32_t *__restrict__ sub, uint32_t ncells) {
  __shared__ ReorderLds L;
  reorderBody<MODE>(r, keys, rank, cellStart, n, cfg, bvh, tri4, ntri, dmax, ng, nearExt, extCap, hot, cold, overflow, origIdx, sub,
                    ncells, blockIdx.x, nullptr, nullptr, L);
}

// ---- the occluder grid of nearVisit: triangle i is listed in every cell its bounding box, grown by `reach`, overlaps and
// whose centre is within reach + the cell's half extent (projected on the normal) of its plane.  One wave per triangle,
// the lanes striding over the cells of its box (built once per scene).  mode 0 counts, mode 1 fills.
__global__ __launch_bounds__(64) void near_grid_kernel(const float4 *__restrict__ tri4, uint32_t ntri, NearGrid g, float reach,
                                                       uint32_t *counts, uint32_t *tris, int mode) {
  const uint32_t i = blockIdx.x;
  if (i >= ntri) return;
  const float4 t0 = tri4[3 * (size_t)i], t1 = tri4[3 * (size_t)i + 1], t2 = tri4[3 * (size_t)i + 2];
  const f3 a = mk3(t0.x, t0.y, t0.z), e1 = mk3(t1.x, t1.y, t1.z), e2 = mk3(t2.x, t2.y, t2.z), n = mk3(t0.w, t1.w, t2.w);
  int lo[3], hi[3];
  float cs[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float ak = comp(a, k), bk = comp(e1, k), ck = comp(e2, k);
    const float l = ak + fminf(0.f, fminf(bk, ck)) - reach * 1.001f, h = ak + fmaxf(0.f, fmaxf(bk, ck)) + reach * 1.001f;
    cs[k] = 1.f / g.inv[k];
    lo[k] = max(0, (int)floorf((l - g.org[k]) * g.inv[k]) - 1);           // (one cell of slack either side: the
    hi[k] = min(g.dim[k] - 1, (int)floorf((h - g.org[k]) * g.inv[k]) + 1);  //  float cell index of a query may round)
  }
  const float slab = reach * 1.001f + 0.5f * 1.001f * (fabsf(n.x) * cs[0] + fabsf(n.y) * cs[1] + fabsf(n.z) * cs[2]) + 1e-6f * (cs[0] + cs[1] + cs[2]);
  const bool flat = n.x == 0.f && n.y == 0.f && n.z == 0.f;  // degenerate: no plane to cull with
  const int nx = hi[0] - lo[0] + 1, ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
  if (nx <= 0 || ny <= 0 || nz <= 0) return;
  const long long ncell = (long long)nx * ny * nz;
  for (long long q = threadIdx.x; q < ncell; q += blockDim.x) {
        const int x = lo[0] + (int)(q % nx), y = lo[1] + (int)((q / nx) % ny), z = lo[2] + (int)(q / ((long long)nx * ny));
        const f3 c = mk3(g.org[0] + ((float)x + 0.5f) * cs[0], g.org[1] + ((float)y + 0.5f) * cs[1], g.org[2] + ((float)z + 0.5f) * cs[2]);
        if (!flat && fabsf(dot(n, c - a)) > slab + cs[0] + cs[1] + cs[2]) continue;  // (a whole cell of slack again)
        const uint32_t cell = ((uint32_t)z * (uint32_t)g.dim[1] + (uint32_t)y) * (uint32_t)g.dim[0] + (uint32_t)x;
        if (mode == 0) atomicAdd(&counts[cell], 1u);
        else tris[g.start[cell] + atomicAdd(&counts[cell], 1u)] = i;
  }
}
void launch_near_grid(const float4 *tri4, uint32_t ntri, const NearGrid &g, float reach, uint32_t *counts, uint32_t *tris, int mode,
                      hipStream_t s) {
  if (ntri) hipLaunchKernelGGL(near_grid_kernel, dim3(ntri), dim3(64), 0, s, tri4, ntri, g, reach, counts, tris, mode);
}

// ---- segment starts of a sorted key array: start[c] = first i with (key[i] >> shift) >= c ----
// one thread per segment, binary search (segments far outnumber the long empty runs a
// per-element scatter would serialise on)
__global__ __launch_bounds__(256) void segment_start_kernel(const uint32_t *__restrict__ keys, uint32_t n,
                                                            uint32_t nseg, uint32_t shift, uint32_t *start) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > nseg) return;
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((keys[mid] >> shift) < c) lo = mid + 1;
    else hi = mid;
  }
  start[c] = lo;
}

// ---- host-side launchers -----------------------------------------------------------------------
void launch_bounds(const float *pos, uint32_t n, float *partial, int nblocks, float *out6, float *hostOut,
                   hipStream_t s, const uint32_t *word, uint32_t *wordOut) {
  // single-wave workgroups: beside the traversal's 22 000 one-wave workgroups a 4-wave workgroup waits for four slots
  // to fall free on ONE CU at the same moment -- this 10 us reduction sat 450 us in front of the next build
  hipLaunchKernelGGL(bounds_kernel, dim3(nblocks), dim3(64), 0, s, pos, n, partial);
  hipLaunchKernelGGL(bounds_final_kernel, dim3(1), dim3(64), 0, s, partial, nblocks, out6, hostOut, word, wordOut);
}

void launch_export_u32(const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, const uint32_t *e,
                       uint32_t *hostOut, hipStream_t s) {
  hipLaunchKernelGGL(export_u32_kernel, dim3(1), dim3(64), 0, s, a, b, c, d, e, hostOut);
}

// ---- the ray bundle of an upload of camera beams (Grid::mode 1, bundle_grid.h) ------------
// One workgroup, run once per fit (the host keeps the frame until a planner reports a ray outside it).  The base rays
// start where their camera path enters the medium, so what they share is a point C on their LINES, the sensor's
// pinhole: the least-squares point of sum |(I - d d^T)(C - o)|^2.
// pass 0 (sums, fp64): out = {M = sum (I - d d^T): xx xy xz yy yz zz; b = sum (I - d d^T) o (3); sum d (3); valid base rays}
// pass 1 (frame in g): out = {uMin, uMax, vMin, vMax, min d.A, max |(I - d d^T)(o - C)|^2, min (o - C).d, max (o - C).d}
__global__ __launch_bounds__(1024) void bundle_fit_kernel(const gvpm_camera_ray *__restrict__ rays, uint32_t nsets, int pass, Grid g,
                                                          double *out) {
  constexpr int NV = 13;
  __shared__ double red[NV][16];
  double v[NV];
  // kind of reduction per slot: 0 sum, 1 min, 2 max
  auto kind = [&](int k) { return pass == 0 ? 0 : ((k == 0 || k == 2 || k == 4 || k == 6) ? 1 : (k < 8 ? 2 : 0)); };
  for (int k = 0; k < NV; ++k) v[k] = kind(k) == 0 ? 0.0 : (kind(k) == 1 ? (double)INFINITY : -(double)INFINITY);
  for (uint32_t i = threadIdx.x; i < nsets; i += blockDim.x) {
    const gvpm_camera_ray &r = rays[(size_t)i * 5];
    if (!GVPM_RAY_VALID(r.info)) continue;
    const double dx = r.d[0], dy = r.d[1], dz = r.d[2];
    if (pass == 0) {
      const double ox = r.o[0], oy = r.o[1], oz = r.o[2];
      const double od = ox * dx + oy * dy + oz * dz;
      v[0] += 1.0 - dx * dx; v[1] -= dx * dy; v[2] -= dx * dz;
      v[3] += 1.0 - dy * dy; v[4] -= dy * dz; v[5] += 1.0 - dz * dz;
      v[6] += ox - dx * od; v[7] += oy - dy * od; v[8] += oz - dz * od;
      v[9] += dx; v[10] += dy; v[11] += dz;
      v[12] += 1.0;
    } else {
      const double dA = dx * g.ba[0] + dy * g.ba[1] + dz * g.ba[2];
      const double inv = 1.0 / fmax(dA, 1e-30);
      const double u = (dx * g.bu[0] + dy * g.bu[1] + dz * g.bu[2]) * inv;
      const double w = (dx * g.bv[0] + dy * g.bv[1] + dz * g.bv[2]) * inv;
      const double wx = (double)r.o[0] - g.bo[0], wy = (double)r.o[1] - g.bo[1], wz = (double)r.o[2] - g.bo[2];
      const double sd = wx * dx + wy * dy + wz * dz;
      const double px = wx - sd * dx, py = wy - sd * dy, pz = wz - sd * dz;
      v[0] = fmin(v[0], u); v[1] = fmax(v[1], u);
      v[2] = fmin(v[2], w); v[3] = fmax(v[3], w);
      v[4] = fmin(v[4], dA);
      v[5] = fmax(v[5], px * px + py * py + pz * pz);
      v[6] = fmin(v[6], sd);
      v[7] = fmax(v[7], sd);
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = 0; k < NV; ++k) {
    double x = v[k];
    for (int o = 32; o > 0; o >>= 1) {
      const double y = __shfl_xor(x, o, 64);
      x = kind(k) == 0 ? x + y : (kind(k) == 1 ? fmin(x, y) : fmax(x, y));
    }
    if (lane == 0) red[k][wave] = x;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int k = threadIdx.x;
    double x = red[k][0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) x = kind(k) == 0 ? x + red[k][w] : (kind(k) == 1 ? fmin(x, red[k][w]) : fmax(x, red[k][w]));
    out[k] = x;
  }
}
void launch_bundle_fit(const gvpm_camera_ray *rays, uint32_t nsets, int pass, const Grid &g, double *out, hipStream_t s) {
  hipLaunchKernelGGL(bundle_fit_kernel, dim3(1), dim3(1024), 0, s, rays, nsets, pass, g, out);
}

// (pass Z alone: the build chain's fifth launch, behind its own pass Y in chain_mid_kernel)
void launch_sat_z(const Grid &g, uint32_t *sat, hipStream_t s) {
  const uint32_t nx1 = g.dim[0] + 1, ny1 = g.dim[1] + 1;
  hipLaunchKernelGGL(sat_z_kernel, dim3((nx1 * ny1 + 255) / 256), dim3(256), 0, s, g, sat);
}
void launch_sat(const uint32_t *cellStart, const Grid &g, uint32_t *sat, hipStream_t s) {
  const uint32_t nx1 = g.dim[0] + 1;
  hipLaunchKernelGGL(sat_y_kernel, dim3((nx1 * g.dim[2] + 255) / 256), dim3(256), 0, s, cellStart, g, sat);
  launch_sat_z(g, sat, s);
}

// sub (optional, bundle cells only): CELL_STRIPES x ncells counters, zeroed by the caller like count[]
uint32_t cell_stripes() { return CELL_STRIPES; }
void launch_cell_count(const float *pos, uint32_t n, const Grid &g, uint32_t *keys, uint32_t *rank, uint32_t *count, uint32_t *sub,
                       hipStream_t s, uint32_t *zeroWord, uint32_t *oneWord) {
  if (g.mode != 1) sub = nullptr;
  hipLaunchKernelGGL(cell_count_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pos, n, g, keys, rank, count, sub, zeroWord, oneWord);
  if (sub) hipLaunchKernelGGL(cell_stripes_kernel, dim3((g.ncells + 255) / 256), dim3(256), 0, s, sub, g.ncells, count);
}

void launch_reorder(const gvpm_photon_soa &raw, const uint32_t *keys, const uint32_t *rank, const uint32_t *cellStart,
                    uint32_t n, const gvpm_params &cfg, const float4 *bvh, const float4 *tri4, uint32_t ntri, float dmax,
                    const NearGrid &ng, uint32_t *nearExt, uint32_t extCap, float4 *hot, float4 *cold, uint32_t *overflow,
                    uint32_t *origIdx, const uint32_t *sub, uint32_t ncells, hipStream_t s, bool nearScalar) {
  const RawPhotons r = rawOf(raw);
#define GVPM_REORDER(M) \
  hipLaunchKernelGGL(reorder_kernel<M>, dim3((n + 63) / 64), dim3(64), 0, s, r, keys, rank, cellStart, n, cfg, bvh, tri4, ntri, \
                     dmax, ng, nearExt, extCap, hot, cold, overflow, origIdx, sub, ncells)
  switch (nearMode(ntri, ng, nearScalar)) {
    case NEAR_SCAN_SCALAR: GVPM_REORDER(NEAR_SCAN_SCALAR); break;
    case NEAR_SCAN_VECTOR: GVPM_REORDER(NEAR_SCAN_VECTOR); break;
    case NEAR_GRID: GVPM_REORDER(NEAR_GRID); break;
    default: GVPM_REORDER(NEAR_BVH); break;
  }
#undef GVPM_REORDER
}

void launch_segment_start(const uint32_t *keys, uint32_t n, uint32_t nseg, uint32_t shift, uint32_t *start,
                          hipStream_t s) {
  hipLaunchKernelGGL(segment_start_kernel, dim3((nseg + 1 + 255) / 256), dim3(256), 0, s, keys, n, nseg, shift, start);
}

}  // namespace gvpm
