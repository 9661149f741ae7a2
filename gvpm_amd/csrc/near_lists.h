// The per-photon near-occluder lists as the photon scatter writes them (occlusion.h reads them back in the evaluation).
// Included by photon_scatter.h, and through it by grid_build.hip (reorder_kernel) and build_chain.hip (chain_tail_kernel).
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "vec.h"

namespace gvpm {

// Occluders a shadow segment of length <= dmax starting at the photon's parent can reach:
// parent within dmax of the triangle's plane and of its (dmax-inflated) bounding box.
// Packs up to twelve 8-bit indices into three words (0xFF = empty slot); 0xFE in the top byte of the
// first word = overflow / too many occluders for 8-bit indices: such photons need the BVH kernels.
// Three formats, chosen by the occluder count (GVPM_NEAR_* in device_types.h):
//   narrow  (<= 253)    twelve 8-bit indices in the three words, 0xFF = empty
//   wide    (<= 64767)  six 16-bit indices, 0xFFFF = empty
//   ext                 word 0 = 0xFD << 24, word 1 = offset into the extension array {count, index...}: lists too long for
//                       the inline slots, and every non-empty list of a scene too large for 16-bit indices
// 0xFE in the top byte of word 0 = the extension array is full: such photons need the BVH kernels.
// Near = within dmax of the triangle's plane and of its (dmax-inflated) bounding box; found by a linear scan for
// small scenes, else by a point query of the occluder BVH (boxes inflated by dmax): the as-written segment is a
// thousandth of the reconnection distance, so the query touches a handful of leaves whatever the scene size.
__device__ __forceinline__ bool nearTriangle(f3 P, const float4 *tri4, uint32_t i, float dmax) {
  const float4 t0 = tri4[3 * (size_t)i], t1 = tri4[3 * (size_t)i + 1], t2 = tri4[3 * (size_t)i + 2];
  const f3 a = mk3(t0.x, t0.y, t0.z), b = mk3(t1.x, t1.y, t1.z), c = mk3(t2.x, t2.y, t2.z);
  const f3 n = mk3(t0.w, t1.w, t2.w);  // unit normal (zero for a degenerate triangle)
  if (fabsf(dot(n, P - a)) > dmax * 1.0001f) return false;
  bool out = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float ak = comp(a, k), bk = comp(b, k), ck = comp(c, k), pk = comp(P, k);
    const float lo = ak + fminf(0.f, fminf(bk, ck)), hi = ak + fmaxf(0.f, fmaxf(bk, ck));
    if (pk < lo - dmax || pk > hi + dmax) out = true;
  }
  return !out;
}
// MODE (one per instantiation of reorder_kernel, chosen at launch: the three walks inlined together cost the small
// scenes' kernel a quarter of its speed): 0 linear scan (<= 64 occluders), 1 BVH point query, 2 occluder grid
template <int MODE, class F>
__device__ __forceinline__ void nearVisit(f3 P, const float4 *bvh, const float4 *tri4, uint32_t ntri, float dmax,
                                          const NearGrid &ng, F f) {
  if (MODE == 0) {
    for (uint32_t i = 0; i < ntri; ++i)
      if (nearTriangle(P, tri4, i, dmax)) f(i);
    return;
  }
  if (MODE == 2) {
    // the cell's occluder list (built for a reach >= dmax): one dependent load instead of a stack walk of the BVH,
    // which was latency-bound per lane -- 2.1 ms of a 4.4 ms step for 4 M photons among 780 occluders (C4)
    const float cx = (P.x - ng.org[0]) * ng.inv[0], cy = (P.y - ng.org[1]) * ng.inv[1], cz = (P.z - ng.org[2]) * ng.inv[2];
    if (!(cx >= 0.f && cy >= 0.f && cz >= 0.f && cx < (float)ng.dim[0] && cy < (float)ng.dim[1] && cz < (float)ng.dim[2])) return;
    const uint32_t c = ((uint32_t)cz * (uint32_t)ng.dim[1] + (uint32_t)cy) * (uint32_t)ng.dim[0] + (uint32_t)cx;
    const uint32_t e0 = ng.start[c], e1 = ng.start[c + 1];
    for (uint32_t e = e0; e < e1; ++e) {
      const uint32_t i = ng.tris[e];
      if (nearTriangle(P, tri4, i, dmax)) f(i);
    }
    return;
  }
  uint32_t stack[32];
  int sp = 0;
  uint32_t cur = 0;
  const float pad = dmax * 1.0001f;
  for (;;) {
    const float4 lo = bvh[2 * (size_t)cur], hi = bvh[2 * (size_t)cur + 1];
    bool descend = false;
    if (P.x >= lo.x - pad && P.x <= hi.x + pad && P.y >= lo.y - pad && P.y <= hi.y + pad && P.z >= lo.z - pad &&
        P.z <= hi.z + pad) {
      const uint32_t first = __float_as_uint(lo.w), count = __float_as_uint(hi.w);
      if (count == 0u) {
        if (sp < 32) stack[sp++] = first + 1u;  // (the host builder's depth is far below 32)
        cur = first;
        descend = true;
      } else {
        for (uint32_t i = first; i < first + count; ++i)
          if (nearTriangle(P, tri4, i, dmax)) f(i);
      }
    }
    if (!descend) {
      if (sp == 0) break;
      cur = stack[--sp];
    }
  }
}
// The wall the parent SITS ON cannot block its reconnections (round 4): the segment starts Epsilon along a direction that
// leaves the wall's plane on the photon's side -- a direction into the wall fails the shift before visibility matters
// (shift_volume_photon.cpp:404-412: the sign test on dot(n_g, dProj) / dot(n_g, edge.d)) -- and moves away from it.  Such
// triangles (coplanar with the parent to position rounding, normal parallel to the parent's) were 95 % of S-cbox's list
// entries: every evaluation wave walked the any-hit loop for tests that cannot succeed.  A medium parent has no normal
// (zero): nothing is skipped for it.
// Round 5 -- the skip derived from the segment instead of a tolerance.  The parent's fp32 position lies delta = N . (P - a)
// off the triangle's plane (rounding: 0 for an axis-aligned wall, a few 1e-7 either way for a tilted one); a segment
// along an admissible direction d (n_parent . d > 0: the sign test and the cosine tests of the reconnection) meets that
// plane at t_self = -delta / (N . d).  With the parent ON the plane or on the side its normal points to, t_self <= 0 for
// every admissible d: the wall can never be hit and is left out.  With the parent BEHIND the plane, directions within
// |delta| / Epsilon of grazing meet it at t_self >= Epsilon -- the reference's rayIntersect reports that self-hit
// (shift_volume_photon.cpp:396-398) -- so the wall STAYS in the list and the evaluation decides (triHitChecked,
// occlusion.h: fp64 where fp32 cannot tell).  delta's sign is pure rounding noise of the inputs: it is taken in fp64
// from the fp32 data, as the oracle's (and a double-precision reference's) Moeller-Trumbore sees it.
// cstar (in / out): for a parent BEHIND the plane the wall is left out all the same and its reach is kept instead --
// max over the parent's own-wall triangles of |delta| / Epsilon, delta the distance to the triangle's plane (unit normal):
// the segment along d meets that plane at t_self >= Epsilon  <=>  n . d <= |delta| / Epsilon.  The evaluation compares the
// reconnection's cosine with it (shiftDiffuse): above, no self-hit is possible; at or below, the shift goes to the exact pass.
__device__ __forceinline__ bool ownWall(f3 P, f3 pn, const float4 *tri4, uint32_t i, float eps, float &cstar) {
  const float4 t0 = tri4[3 * (size_t)i], t1 = tri4[3 * (size_t)i + 1], t2 = tri4[3 * (size_t)i + 2];
  const f3 a = mk3(t0.x, t0.y, t0.z), n = mk3(t0.w, t1.w, t2.w);
  const float tol = 1e-6f * (1.f + fabsf(P.x) + fabsf(P.y) + fabsf(P.z) + fabsf(a.x) + fabsf(a.y) + fabsf(a.z));
  const float align = dot(n, pn);
  // (parallel to 1e-3 rad: the parent's normal is this triangle's to rounding -- 6e-5 rad through the packed upload's
  // octahedral code -- and the evaluation's cosine is taken against the PARENT's normal)
  if (!(fabsf(align) > 0.9999995f && fabsf(dot(n, P - a)) <= tol)) return false;
  // N = e1 x e2 and delta in fp64 (exact products of fp32 data up to the last additions: |error| ~ 1e-16 of O(1) terms)
  const double e1x = t1.x, e1y = t1.y, e1z = t1.z, e2x = t2.x, e2y = t2.y, e2z = t2.z;
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const double delta = nx * ((double)P.x - (double)a.x) + ny * ((double)P.y - (double)a.y) + nz * ((double)P.z - (double)a.z);
  const bool front = align > 0.f ? delta >= 0.0 : delta <= 0.0;
  if (!front) {
    const double nl = sqrt(nx * nx + ny * ny + nz * nz);
    if (nl > 0.0) cstar = fmaxf(cstar, (float)(fabs(delta) / (nl * (double)eps)) * 1.000001f);
  }
  return true;
}

template <int MODE>
// cstarOut > 0: the parent lies behind a wall it sits on (ownWall); word 2 then carries that reach instead of entries (the
// inline lists hold 8 / 4 of them; bit 15 of the record's flags says so)
__device__ __forceinline__ void nearOccluders(f3 P, f3 pn, const float4 *bvh, const float4 *tri4, uint32_t ntri, float dmax,
                                              const NearGrid &ng, uint32_t *ext, uint32_t extCap, float eps, uint32_t &w0, uint32_t &w1,
                                              uint32_t &w2, float &cstarOut) {
  w0 = w1 = w2 = 0xFFFFFFFFu;
  cstarOut = 0.f;
  if (ntri == 0u) return;
  const bool narrow = ntri <= GVPM_NEAR_NARROW_MAX, wide = !narrow && ntri <= GVPM_NEAR_WIDE_MAX;
  const uint32_t cap = narrow ? 12u : (wide ? 6u : 0u);
  uint32_t cnt = 0, a0 = 0xFFFFFFFFu, a1 = 0xFFFFFFFFu, a2 = 0xFFFFFFFFu;
  float cstar = 0.f;
  nearVisit<MODE>(P, bvh, tri4, ntri, dmax, ng, [&](uint32_t i) {
    if (ownWall(P, pn, tri4, i, eps, cstar)) return;
    if (cnt < cap) {
      uint32_t word, sh, m;
      if (narrow) { word = cnt >> 2; sh = 8u * (cnt & 3u); m = ~(0xFFu << sh); }
      else        { word = cnt >> 1; sh = 16u * (cnt & 1u); m = ~(0xFFFFu << sh); }
      const uint32_t v = i << sh;
      if (word == 0u) a0 = (a0 & m) | v;
      else if (word == 1u) a1 = (a1 & m) | v;
      else a2 = (a2 & m) | v;
    }
    cnt++;
  });
  cstarOut = cstar;
  const uint32_t capC = cstar > 0.f ? (cap * 2u) / 3u : cap;  // (word 2 is taken)
  if (cnt <= capC) {
    w0 = a0; w1 = a1; w2 = cstar > 0.f ? __float_as_uint(cstar) : a2;
    return;
  }
  // extension list {count, indices}
  const uint32_t off = atomicAdd(ext, cnt + 1u);  // ext[0] = the allocation cursor (starts at 1)
  if ((unsigned long long)off + cnt + 1u > extCap) {
    w0 = 0xFEFFFFFFu;
    return;
  }
  ext[off] = cnt;
  uint32_t k = 0;
  float dummy = 0.f;
  nearVisit<MODE>(P, bvh, tri4, ntri, dmax, ng, [&](uint32_t i) {
    if (!ownWall(P, pn, tri4, i, eps, dummy)) ext[off + 1u + (k++)] = i;
  });
  w0 = 0xFDFFFFFFu;
  w1 = off;
  if (cstar > 0.f) w2 = __float_as_uint(cstar);
}

}  // namespace gvpm
