// The beam builds.  Camera beams (every technique that walks image tiles): the tile keys of the beam sets and their counting
// sort, so that one wave works on the sets of one tile (grid_build.hip's head names the reference's counterpart).  Photon
// beams (G-Beams): one 128-byte record per beam, the reach of the uploaded shifts, and each beam's near-occluder list with
// the free cone of its reconnections.  The scans and the radix sort between these kernels are scan_sort.hip's.
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "shift_device.h"
#include "vec.h"
#include "photon_scatter.h"

namespace gvpm {

// ---- camera beam sets: tile keys -------------------------------------------------------------
// key =((tileIndex * tilePixels + pixelInTile) << 3 | (edge & 7)); tile index = key >> tileShift
__global__ __launch_bounds__(256) void beam_key_kernel(const gvpm_camera_ray *__restrict__ rays, uint32_t nsets,
                                                       int width, int tw, int th, uint32_t *keys, uint32_t *vals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nsets) return;
  const gvpm_camera_ray &b = rays[(size_t)i * 5];
  const uint32_t px = b.pixel & 0xFFFFu, py = b.pixel >> 16;
  const uint32_t tilesX = (width + tw - 1) / tw;
  const uint32_t tile = (py / th) * tilesX + px / tw;
  const uint32_t inTile = (py % th) * tw + px % tw;
  keys[i] = ((tile * (uint32_t)(tw * th) + inTile) << 3) | (GVPM_RAY_EDGE(b.info) & 7u);
  vals[i] = i;
}

// counting sort of the beam sets by the same key
__global__ __launch_bounds__(256) void beam_count_kernel(const gvpm_camera_ray *__restrict__ rays, uint32_t nsets,
                                                         int width, int tw, int th, uint32_t *keys, uint32_t *rank,
                                                         uint32_t *count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nsets) return;
  const gvpm_camera_ray &b = rays[(size_t)i * 5];
  const uint32_t px = b.pixel & 0xFFFFu, py = b.pixel >> 16;
  const uint32_t tilesX = (width + tw - 1) / tw;
  const uint32_t tile = (py / th) * tilesX + px / tw;
  const uint32_t inTile = (py % th) * tw + px % tw;
  const uint32_t k = ((tile * (uint32_t)(tw * th) + inTile) << 3) | (GVPM_RAY_EDGE(b.info) & 7u);
  keys[i] = k;
  rank[i] = atomicAdd(&count[k], 1u);
}

__global__ __launch_bounds__(256) void beam_scatter_kernel(const uint32_t *__restrict__ keys,
                                                           const uint32_t *__restrict__ rank,
                                                           const uint32_t *__restrict__ start, uint32_t n,
                                                           uint32_t *setPerm) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  setPerm[start[keys[i]] + rank[i]] = i;
}

// tileStart[t] = first slot of tile t = start[t << shift]; start has (ntiles << shift) + 1 entries
__global__ __launch_bounds__(256) void tile_start_kernel(const uint32_t *__restrict__ start, uint32_t ntiles,
                                                         uint32_t shift, uint32_t *tileStart) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > ntiles) return;
  tileStart[t] = start[(size_t)t << shift];
}

void launch_beam_count(const gvpm_camera_ray *rays, uint32_t nsets, int width, int tw, int th, uint32_t *keys,
                       uint32_t *rank, uint32_t *count, hipStream_t s) {
  hipLaunchKernelGGL(beam_count_kernel, dim3((nsets + 255) / 256), dim3(256), 0, s, rays, nsets, width, tw, th, keys,
                     rank, count);
}
void launch_beam_scatter(const uint32_t *keys, const uint32_t *rank, const uint32_t *start, uint32_t n,
                         uint32_t *setPerm, hipStream_t s) {
  hipLaunchKernelGGL(beam_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, s, keys, rank, start, n, setPerm);
}
void launch_tile_start(const uint32_t *start, uint32_t ntiles, uint32_t shift, uint32_t *tileStart, hipStream_t s) {
  hipLaunchKernelGGL(tile_start_kernel, dim3((ntiles + 1 + 255) / 256), dim3(256), 0, s, start, ntiles, shift, tileStart);
}

void launch_beam_keys(const gvpm_camera_ray *rays, uint32_t nsets, int width, int tw, int th, uint32_t *keys,
                      uint32_t *vals, hipStream_t s) {
  hipLaunchKernelGGL(beam_key_kernel, dim3((nsets + 255) / 256), dim3(256), 0, s, rays, nsets, width, tw, th, keys,
                     vals);
}

// ---- photon beams (G-Beams) ----------------------------------------------------------------------
// records of photon beams (indexed by beam, not sorted), 128 bytes = one cache line per evaluation (the nine
// plane-major float4 arrays of round 1 cost nine):
//   0 {flux, parentPdf} 1 {p1, parentRR} 2 {parentN, parentG} 3 {prefixW, near0} 4 {parentScat, near1}
//   5 {parentWi, near2} 6 {p2, bits} 7 {endN, length}   (near0..2: beam_near_kernel)
__global__ __launch_bounds__(64) void beam_cold_kernel(RawPhotons r, const float *__restrict__ endN, uint32_t n,
                                                       gvpm_params cfg, const uint32_t *__restrict__ subCounts, float4 *cold,
                                                       float4 *aux) {
  // The record is assembled in LDS and written by EIGHT lanes (one 16-byte quad each), as reorder_kernel does: a store
  // instruction then covers eight whole 128-byte lines instead of sixty-four 16-byte pieces of sixty-four lines.
  __shared__ float4 stg[64][GVPM_REC_QUADS + 1];  // +1: odd stride against bank conflicts
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = threadIdx.x;
  if (i < n) {
    uint32_t bits = r.flags[i] & ~((1u << 6) | (1u << GVPM_HOT_PARITY_BIT));
    // for beams the debugShift filter only suppresses the shifts (shift_volume_beams.cpp:210-216),
    // so only computeVolumeContribution is folded into bit 6
    gvpm_params c2 = cfg;
    c2.debug_shift = GVPM_SHIFT_ALL;
    if (photonContributes(bits, c2)) bits |= 1u << 6;
    bits |= (r.path_id[i] & 1u) << GVPM_HOT_PARITY_BIT;
    stg[t][0] = ld3(r.flux, i, r.parent_pdf[i]);
    stg[t][1] = ld3(r.parent_pos, i, r.parent_rr[i]);
    stg[t][2] = ld3(r.parent_n, i, r.parent_g[i]);
    stg[t][3] = ld3(r.prefix_w, i, 0.f);
    stg[t][4] = ld3(r.parent_scat, i, 0.f);
    stg[t][5] = ld3(r.parent_wi, i, 0.f);
    stg[t][6] = ld3(r.pos, i, __uint_as_float(bits));
    // PhotonBeam::setEndPoint, pm/beams_struct.h:73-81: the length, once, in fp64 (an fp64 square root and division
    // per evaluation otherwise)
    const double dx = (double)r.pos[3 * (size_t)i] - (double)r.parent_pos[3 * (size_t)i];
    const double dy = (double)r.pos[3 * (size_t)i + 1] - (double)r.parent_pos[3 * (size_t)i + 1];
    const double dz = (double)r.pos[3 * (size_t)i + 2] - (double)r.parent_pos[3 * (size_t)i + 2];
    const double lenD = sqrt(dx * dx + dy * dy + dz * dz);
    stg[t][7] = ld3(endN, i, (float)lenD);
    // what the sorted sub-beam records are made of (sub_hot_kernel), 32 bytes per beam: {p1, bits} {direction, sub-beam
    // length} -- the fp64 norm and division once per beam instead of once per sub-beam (47 M of them at C3)
    if (aux) {
      const double inv = 1.0 / lenD;
      aux[2 * (size_t)i] = ld3(r.parent_pos, i, __uint_as_float(bits));
      aux[2 * (size_t)i + 1] = make_float4((float)(dx * inv), (float)(dy * inv), (float)(dz * inv), (float)lenD / (float)subCounts[i]);
    }
  }
  __syncthreads();
  const uint32_t base = blockIdx.x * blockDim.x;
  for (int e = t; e < 64 * GVPM_REC_QUADS; e += 64) {
    const int rec = e / GVPM_REC_QUADS, part = e % GVPM_REC_QUADS;
    if (base + (uint32_t)rec < n) cold[(size_t)(base + rec) * GVPM_REC_QUADS + part] = stg[rec][part];
  }
}

// ---- occluders near a photon beam -----------------------------------------------------------------------------
// The reconnection of a beam shift tests the whole NEW beam parent -> offset position for occluders
// (shift_volume_beams.cpp:420-426).  The offset position lies within `delta` of the point X of the original beam the
// kernel sits at, so every point of the new segment lies within delta of the original segment [p1, p2] (the two
// segments share p1 and end delta apart): only triangles whose box, inflated by delta, the original segment crosses
// can be hit.  delta = 4 r + S: |offsetPos - X| <= |shiftRay(w) - baseRay(w)| + (kernel offset, replayed in the
// shifted frame: 2 r) + (mirror adjustment of getShiftPos, shift_volume_beams.cpp:120-135: 2 r), and S bounds the
// first term over every uploaded beam set (shift_extent_kernel).  Up to 12 byte indices per beam go into the spare
// words of quads 3-5 of its record; a beam with more (or a scene of more than 253 occluders) is marked 0xFE in the
// top byte of word 0 and takes the full test.
__global__ __launch_bounds__(256) void shift_extent_kernel(const gvpm_camera_ray *__restrict__ rays, uint32_t nsets,
                                                           uint32_t *extentBits) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  float S = 0.f;
  if (i < nsets) {
    const gvpm_camera_ray b = rays[(size_t)i * 5];
    for (int k = 1; k < 5; ++k) {
      const gvpm_camera_ray s = rays[(size_t)i * 5 + k];
      if (!GVPM_RAY_VALID(s.info)) continue;
      const float ox = s.o[0] - b.o[0], oy = s.o[1] - b.o[1], oz = s.o[2] - b.o[2];
      const float dx = s.d[0] - b.d[0], dy = s.d[1] - b.d[1], dz = s.d[2] - b.d[2];
      // w <= min(len_b, len_s) (shift_volume_beams.cpp: the shift is dropped when w exceeds the shifted edge)
      const float e = sqrtf(ox * ox + oy * oy + oz * oz) + fminf(b.len, s.len) * sqrtf(dx * dx + dy * dy + dz * dz);
      S = fmaxf(S, e);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) S = fmaxf(S, __shfl_xor(S, o, 64));
  // S >= 0: bit order = value order; a wave first looks whether it would raise the maximum (same-address atomics retire ~11 ns apart)
  if ((threadIdx.x & 63) == 0 && S > 0.f &&
      __float_as_uint(S * 1.0001f) > __hip_atomic_load(extentBits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(extentBits, __float_as_uint(S * 1.0001f));
}

// The FREE CONE of a beam (round 3).  A new beam of a reconnection is a straight segment from the beam's origin p1: every
// point of it is seen from p1 under ONE angle to the beam's direction, alpha = angle(nd, bd), and lies no farther than
// its length.  For a listed triangle T let cosT = the largest cosine of that angle over the points of T (0 angle: the
// beam's line pierces it) and, when the line pierces T's PLANE at t_p > 0, alongMin = t_p - delta tan(incidence): every
// point of the plane within delta of the line -- all a new beam can reach, it stays within delta of the beam -- lies at
// least that far along the beam.  With M1 = the smallest alongMin of the triangles the beam points at (cosT ~ 1: the
// surface it ends on) and cosA0 = the largest cosT of the others,
//     dot(nd, bd) > cosA0  and  |new beam| < M1   =>   the new beam meets no occluder,
// because it is inside the cone no other triangle enters and too short for the ones in front.  The evaluation skips the
// any-hit loop for such reconnections (85-95 % of them at C3: a beam through the aperture is certified unless the new
// beam grazes the aperture's edge or reaches the floor), and takes the others through it as before.
// Returned in clear[i] = {cosA0 + margin, M1 - margin}; {2, 0} = never certified (list overflowed, degenerate).
struct BeamClearTri {
  float cosT, alongMin;
};
__device__ __forceinline__ BeamClearTri beamClearTri(const float p1[3], const float bd[3], float delta, float eps, const float4 t0, const float4 t1,
                                                     const float4 t2) {
  const float a[3] = {t0.x - p1[0], t0.y - p1[1], t0.z - p1[2]};
  const float e1[3] = {t1.x, t1.y, t1.z}, e2[3] = {t2.x, t2.y, t2.z};
  const float b[3] = {a[0] + e1[0], a[1] + e1[1], a[2] + e1[2]}, c[3] = {a[0] + e2[0], a[1] + e2[1], a[2] + e2[2]};
  auto dot3 = [](const float *x, const float *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
  // the largest cosine over an edge P + s E, s in [0, 1]: g(s) = (al + be s) / |P + s E|, stationary at
  // s* = (al d - be c0) / (be d - al e)
  auto edgeMax = [&](const float *P, const float *Q) {
    const float E[3] = {Q[0] - P[0], Q[1] - P[1], Q[2] - P[2]};
    const float al = dot3(P, bd), be = dot3(E, bd), c0 = dot3(P, P), d = dot3(P, E), e = dot3(E, E);
    float m = -1.f;
    auto at = [&](float sp) {
      const float l2 = c0 + 2.f * d * sp + e * sp * sp;
      if (l2 > 1e-30f) m = fmaxf(m, (al + be * sp) * rsqrtf(l2));
      else m = 1.f;  // the beam's origin ON the edge: every direction of the plane is met
    };
    at(0.f);
    at(1.f);
    const float den = be * d - al * e;
    if (fabsf(den) > 1e-30f) {
      const float sp = (al * d - be * c0) / den;
      if (sp > 0.f && sp < 1.f) at(sp);
    }
    return m;
  };
  BeamClearTri o;
  o.cosT = fmaxf(edgeMax(a, b), fmaxf(edgeMax(b, c), edgeMax(c, a)));
  // the beam's line through the triangle (Moeller-Trumbore from p1 along bd, with slack: a near miss is a hit here)
  const float nrm[3] = {t0.w, t1.w, t2.w};
  const float cn = dot3(bd, nrm), dn = dot3(a, nrm);  // plane: nrm . (x - v0) = 0, a = v0 - p1
  // The wall the beam STARTS on (p1 within position rounding of the plane; round 5): p1 may lie |delta| BEHIND it, and a new beam
  // whose cosine to the normal is below |delta| / Epsilon then meets the plane at t = |delta| / cos >= Epsilon -- the reference's
  // rayIntersect reports that hit (shift_volume_beams.cpp:420-426).  The cone such a wall leaves free is drawn inside its plane
  // by that reach, taken from what is known of delta here: |dn| plus the rounding of dn (the fp32 difference a = v0 - p1 and the
  // stored unit normal: 5e-7 |a|_1), times 1.5.  In the unit room that is the 0.02 rad this sliver used to be as a constant
  // (|delta| a few 1e-7, Epsilon 1e-4); a room 256 wide 1400 from the origin has |delta| ~ Epsilon and NO direction is free of
  // its own wall -- the constant certified reconnections there that self-hit in the reference (found by the `centimetres`
  // transform, tests/test_similarity_gpu.py: 15 of 145 000 shifts).  Reconnections in the sliver take the any-hit loop, whose
  // undecided triangles go to the exact pass.
  {
    const float scale = fabsf(p1[0]) + fabsf(p1[1]) + fabsf(p1[2]) + fabsf(t0.x) + fabsf(t0.y) + fabsf(t0.z);
    if (fabsf(dn) <= 2e-6f * (1.f + scale) && o.cosT < 1.f) {
      const float a1 = fabsf(a[0]) + fabsf(a[1]) + fabsf(a[2]);
      const float sinS = 1.5f * (fabsf(dn) + 5e-7f * a1) / eps;
      const float sinT = sqrtf(fmaxf(1.f - o.cosT * o.cosT, 0.f));
      o.cosT = sinS < 1.f ? fminf(1.f, o.cosT * sqrtf(1.f - sinS * sinS) + sinT * sinS) : 1.f;  // cos(angle - asin(sinS))
    }
  }
  o.alongMin = -INFINITY;
  // The pierce test runs at ANY incidence: a line that crosses a large triangle at a grazing angle (|cn| <= 0.05) sees it
  // under angle 0 although every edge is far off axis -- filed under "others" with the edges' cosine, such a triangle let
  // reconnections inside that cone skip the any-hit test (a thin plate with medium on both sides).  alongMin is only
  // trusted away from grazing (delta tan(incidence) explodes there): a grazed triangle the beam points at leaves
  // M1 = -inf, i.e. the beam is never certified.
  if (fabsf(cn) > 1e-12f) {
    const float tp = dn / cn;  // p1 + tp bd on the plane
    if (tp > 0.f) {
      if (fabsf(cn) > 0.05f) o.alongMin = tp - delta * sqrtf(fmaxf(1.f - cn * cn, 0.f)) / fabsf(cn);
      // inside (or within slack of) the triangle?  barycentrics of the piercing point
      const float q[3] = {tp * bd[0] - a[0], tp * bd[1] - a[1], tp * bd[2] - a[2]};  // from v0
      const float d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2), q1 = dot3(q, e1), q2 = dot3(q, e2);
      const float det = d11 * d22 - d12 * d12;
      if (det > 1e-30f) {
        const float u = (q1 * d22 - q2 * d12) / det, v = (q2 * d11 - q1 * d12) / det;
        if (u > -1e-3f && v > -1e-3f && u + v < 1.001f) o.cosT = 1.f;
      }
    }
  }
  return o;
}

__global__ __launch_bounds__(128) void beam_near_kernel(float4 *cold, uint32_t n, const float4 *__restrict__ tri4, uint32_t ntri,
                                                        float r, float eps, const uint32_t *__restrict__ extentBits, float2 *clear, bool freeCone) {
  __shared__ float2 ctab[19][128];  // (19: the longest list, BeamNearFmt)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t N = GVPM_REC_QUADS;
  uint32_t w[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  const BeamNearFmt fmt = beamNearFmt(ntri);
  if (fmt.bits != 8u) w[2] &= 0x7FFFFFFFu;  // (bit 95: the narrow formats' overflow flag)
  if (ntri > GVPM_NEAR_NARROW_MAX) {
    w[0] = 0xFE000000u | 0x00FFFFFFu;
  } else {
    const float delta = 4.f * r + __uint_as_float(*extentBits);
    const float4 c2 = cold[N * i + 1], c7 = cold[N * i + 6];
    const float p1[3] = {c2.x, c2.y, c2.z}, p2[3] = {c7.x, c7.y, c7.z};
    uint32_t cnt = 0;
    for (uint32_t t = 0; t < ntri; ++t) {
      const float4 t0 = tri4[3 * t], t1 = tri4[3 * t + 1], t2 = tri4[3 * t + 2];
      const float v0[3] = {t0.x, t0.y, t0.z}, e1[3] = {t1.x, t1.y, t1.z}, e2[3] = {t2.x, t2.y, t2.z};
      // segment [p1, p2] against the triangle's box inflated by delta (slab test, conservative)
      float t0s = 0.f, t1s = 1.f;
      bool hit = true;
      for (int c = 0; c < 3; ++c) {
        const float lo = fminf(v0[c], fminf(v0[c] + e1[c], v0[c] + e2[c])) - delta;
        const float hi = fmaxf(v0[c], fmaxf(v0[c] + e1[c], v0[c] + e2[c])) + delta;
        const float d = p2[c] - p1[c];
        if (fabsf(d) < 1e-20f) {
          hit = hit && p1[c] >= lo && p1[c] <= hi;
        } else {
          const float inv = 1.f / d;
          const float a = (lo - p1[c]) * inv, b = (hi - p1[c]) * inv;
          t0s = fmaxf(t0s, fminf(a, b) - 1e-5f);
          t1s = fminf(t1s, fmaxf(a, b) + 1e-5f);
        }
      }
      hit = hit && t0s <= t1s;
      if (hit) {
        if (cnt < fmt.cap) {
          // entry cnt: fmt.bits bits at bit cnt * fmt.bits of the 96-bit string (it may straddle two words)
          const uint32_t off = cnt * fmt.bits, wi = off >> 5, sh = off & 31u;
          w[wi] = (w[wi] & ~(fmt.mask << sh)) | (t << sh);
          if (sh + fmt.bits > 32u) w[wi + 1] = (w[wi + 1] & ~(fmt.mask >> (32u - sh))) | (t >> (32u - sh));
        }
        cnt++;
      }
    }
    // (index 0xFE / 0xFF cannot occur in the top byte of word 0: ntri <= 253)
    if (cnt > fmt.cap) {
      if (fmt.bits == 8u) w[0] = 0xFE000000u | 0x00FFFFFFu;
      else w[2] |= 0x80000000u;
    }
  }
  cold[N * i + 3].w = __uint_as_float(w[0]);
  cold[N * i + 4].w = __uint_as_float(w[1]);
  cold[N * i + 5].w = __uint_as_float(w[2]);
  // the beam's free cone over its list (see above): two passes over the listed triangles
  float2 cl = make_float2(2.f, 0.f);
  if (freeCone && ntri <= GVPM_NEAR_NARROW_MAX && !beamNearOverflow(fmt, w[0], w[2])) {
    const float delta = 4.f * r + __uint_as_float(*extentBits);
    const float4 c2 = cold[N * i + 1], c7 = cold[N * i + 6];
    const float p1[3] = {c2.x, c2.y, c2.z};
    float bd[3] = {c7.x - c2.x, c7.y - c2.y, c7.z - c2.z};
    const float l2 = bd[0] * bd[0] + bd[1] * bd[1] + bd[2] * bd[2];
    if (l2 > 1e-30f) {
      const float il = rsqrtf(l2);
      bd[0] *= il; bd[1] *= il; bd[2] *= il;
      const float cosSmall = 0.99955f;  // ~0.03 rad: "the beam points at this triangle"
      // (each listed triangle's {cosT, alongMin} once: parked in this lane's LDS column between the two passes)
      float M1 = INFINITY;
      uint32_t nl = 0;
      for (uint32_t q = 0; q < fmt.cap; ++q) {
        const uint32_t t = beamNearEntry(fmt, w[0], w[1], w[2], q);
        if (t == fmt.mask) break;
        const BeamClearTri ct = beamClearTri(p1, bd, delta, eps, tri4[3 * t], tri4[3 * t + 1], tri4[3 * t + 2]);
        ctab[q][threadIdx.x] = make_float2(ct.cosT, ct.alongMin);
        nl = q + 1;
        if (ct.cosT > cosSmall) M1 = fminf(M1, ct.alongMin);
      }
      float cosA0 = -1.f;
      for (uint32_t q = 0; q < nl; ++q) {
        const float2 ct = ctab[q][threadIdx.x];
        if (!(ct.y >= M1)) cosA0 = fmaxf(cosA0, ct.x);
      }
      if (M1 > 0.f) cl = make_float2(cosA0 + 1e-5f, M1 * (1.f - 1e-5f) - 1e-6f);
    }
  }
  if (clear) clear[i] = cl;
}

void launch_shift_extent(const gvpm_camera_ray *rays, uint32_t nsets, uint32_t *extentBits, hipStream_t s) {
  (void)hipMemsetAsync(extentBits, 0, sizeof(uint32_t), s);
  if (nsets) hipLaunchKernelGGL(shift_extent_kernel, dim3((nsets + 255) / 256), dim3(256), 0, s, rays, nsets, extentBits);
}

// GVPM_BEAMS_TRACE: how long the beams' near-occluder lists are -- hist[k] = lists of k entries (k <= 19), hist[20] = overflowed
__global__ __launch_bounds__(256) void beam_near_hist_kernel(const float4 *__restrict__ cold, uint32_t n, uint32_t ntri, uint32_t *hist) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t N = GVPM_REC_QUADS;
  const uint32_t w[3] = {__float_as_uint(cold[N * i + 3].w), __float_as_uint(cold[N * i + 4].w), __float_as_uint(cold[N * i + 5].w)};
  const BeamNearFmt fmt = beamNearFmt(ntri);
  uint32_t k = 20;
  if (!beamNearOverflow(fmt, w[0], w[2])) {
    k = 0;
    for (uint32_t q = 0; q < fmt.cap; ++q)
      if (beamNearEntry(fmt, w[0], w[1], w[2], q) != fmt.mask) k++;
  }
  atomicAdd(&hist[k], 1u);
}
void launch_beam_near_hist(const float4 *cold, uint32_t n, uint32_t ntri, uint32_t *hist, hipStream_t s) {
  if (n) hipLaunchKernelGGL(beam_near_hist_kernel, dim3((n + 255) / 256), dim3(256), 0, s, cold, n, ntri, hist);
}
void launch_beam_near(float4 *cold, uint32_t n, const float4 *tri4, uint32_t ntri, float r, float eps, const uint32_t *extentBits,
                      float2 *clear, bool freeCone, hipStream_t s) {
  if (n) hipLaunchKernelGGL(beam_near_kernel, dim3((n + 127) / 128), dim3(128), 0, s, cold, n, tri4, ntri, r, eps, extentBits, clear, freeCone);
}

void launch_beam_cold(const gvpm_photon_soa &raw, const float *endN, uint32_t n, const gvpm_params &cfg,
                      const uint32_t *subCounts, float4 *cold, float4 *aux, hipStream_t s) {
  const RawPhotons r = rawOf(raw);
  hipLaunchKernelGGL(beam_cold_kernel, dim3((n + 63) / 64), dim3(64), 0, s, r, endN, n, cfg, subCounts, cold, aux);
}

}  // namespace gvpm
