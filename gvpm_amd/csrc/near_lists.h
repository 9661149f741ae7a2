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

// One occluder's three quads {a, n.x} {b - a, n.y} {c - a, n.z} as VALUES: loaded once a visit and handed to both tests below.
// loadTri reads them per lane (vector loads); loadTriUniform, for an index that is the same in every lane of the wave, reads
// them through the constant address space -- the scalar cache, into SGPRs: no lane waits for a vector-memory round trip, and
// the compiler need not prove that the kernel's own stores leave the table alone.  (The table is written by the scene
// upload only, launches before any kernel that scans it.)
struct Tri3 {
  float4 t0, t1, t2;
};
__device__ __forceinline__ Tri3 loadTri(const float4 *tri4, uint32_t i) {
  return Tri3{tri4[3 * (size_t)i], tri4[3 * (size_t)i + 1], tri4[3 * (size_t)i + 2]};
}
typedef const __attribute__((address_space(4))) float *UniformF32;
__device__ __forceinline__ UniformF32 uniformView(const float4 *tri4) {
  return (UniformF32)(reinterpret_cast<const float *>(tri4));
}
__device__ __forceinline__ Tri3 loadTriUniform(UniformF32 tab, uint32_t i) {
  const UniformF32 p = tab + 12u * (size_t)i;
  return Tri3{make_float4(p[0], p[1], p[2], p[3]), make_float4(p[4], p[5], p[6], p[7]), make_float4(p[8], p[9], p[10], p[11])};
}
__device__ __forceinline__ bool nearTriangle(f3 P, const Tri3 &t, float dmax) {
  const float4 t0 = t.t0, t1 = t.t1, t2 = t.t2;
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
__device__ __forceinline__ bool nearTriangle(f3 P, const float4 *tri4, uint32_t i, float dmax) {
  return nearTriangle(P, loadTri(tri4, i), dmax);
}
// MODE (one per instantiation of reorder_kernel, chosen at launch: the three walks inlined together cost the small
// scenes' kernel a quarter of its speed): 0 linear scan (<= 64 occluders) on scalar data -- written out in nearOccluders,
// it does not come through here --, 1 BVH point query, 2 occluder grid, 3 the linear scan with per-lane vector loads
// (GVPM_NEAR_SCALAR=0: kept as the cross-check of 0)
constexpr int NEAR_SCAN_SCALAR = 0, NEAR_BVH = 1, NEAR_GRID = 2, NEAR_SCAN_VECTOR = 3;
// the launchers' choice among them
inline int nearMode(uint32_t ntri, const NearGrid &ng, bool scalarScan) {
  return ntri <= 64u ? (scalarScan ? NEAR_SCAN_SCALAR : NEAR_SCAN_VECTOR) : (ng.start ? NEAR_GRID : NEAR_BVH);
}
template <int MODE, class F>
__device__ __forceinline__ void nearVisit(f3 P, const float4 *bvh, const float4 *tri4, uint32_t ntri, float dmax,
                                          const NearGrid &ng, F f) {
  static_assert(MODE != NEAR_SCAN_SCALAR, "the scalar scan is nearOccluders' own loop");
  if (MODE == NEAR_SCAN_VECTOR) {
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
// (values in, values out: `own`, and cstar raised where the parent lies behind the wall)
struct OwnWall {
  bool own;
  float cstar;
};
__device__ __forceinline__ OwnWall ownWall(f3 P, f3 pn, const Tri3 &t, float eps, float cstar) {
  const float4 t0 = t.t0, t1 = t.t1, t2 = t.t2;
  const f3 a = mk3(t0.x, t0.y, t0.z), n = mk3(t0.w, t1.w, t2.w);
  const float tol = 1e-6f * (1.f + fabsf(P.x) + fabsf(P.y) + fabsf(P.z) + fabsf(a.x) + fabsf(a.y) + fabsf(a.z));
  const float align = dot(n, pn);
  // (parallel to 1e-3 rad: the parent's normal is this triangle's to rounding -- 6e-5 rad through the packed upload's
  // octahedral code -- and the evaluation's cosine is taken against the PARENT's normal)
  if (!(fabsf(align) > 0.9999995f && fabsf(dot(n, P - a)) <= tol)) return OwnWall{false, cstar};
  // N = e1 x e2 and delta in fp64 (exact products of fp32 data up to the last additions: |error| ~ 1e-16 of O(1) terms)
  const double e1x = t1.x, e1y = t1.y, e1z = t1.z, e2x = t2.x, e2y = t2.y, e2z = t2.z;
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const double delta = nx * ((double)P.x - (double)a.x) + ny * ((double)P.y - (double)a.y) + nz * ((double)P.z - (double)a.z);
  const bool front = align > 0.f ? delta >= 0.0 : delta <= 0.0;
  if (!front) {
    const double nl = sqrt(nx * nx + ny * ny + nz * nz);
    if (nl > 0.0) cstar = fmaxf(cstar, (float)(fabs(delta) / (nl * (double)eps)) * 1.000001f);
  }
  return OwnWall{true, cstar};
}

// The inline list under construction, carried BY VALUE through the scan (no lambda holds a pointer to it: captured by
// reference, the four words lived in private memory in the build chain's tail kernel): the count of near occluders
// seen, the three words, and cstar.
struct NearScan {
  uint32_t cnt, a0, a1, a2;
  float cstar;
};
// occluder i, already known to be near: dropped if it is the parent's own wall, else counted and, while there is room, packed
__device__ __forceinline__ NearScan nearAppend(NearScan s, f3 P, f3 pn, const Tri3 &t, uint32_t i, float eps, bool narrow, uint32_t cap) {
  const OwnWall o = ownWall(P, pn, t, eps, s.cstar);
  s.cstar = o.cstar;
  if (o.own) return s;
  if (s.cnt < cap) {
    uint32_t word, sh, m;
    if (narrow) { word = s.cnt >> 2; sh = 8u * (s.cnt & 3u); m = ~(0xFFu << sh); }
    else        { word = s.cnt >> 1; sh = 16u * (s.cnt & 1u); m = ~(0xFFFFu << sh); }
    const uint32_t v = i << sh;
    if (word == 0u) s.a0 = (s.a0 & m) | v;
    else if (word == 1u) s.a1 = (s.a1 & m) | v;
    else s.a2 = (s.a2 & m) | v;
  }
  s.cnt++;
  return s;
}

// The list of one photon: its three words, and cstar > 0: the parent lies behind a wall it sits on (ownWall); word 2 then
// carries that reach instead of entries (the inline lists hold 8 / 4 of them; bit 15 of the record's flags says so)
struct NearList {
  uint32_t w0, w1, w2;
  float cstar;
};
template <int MODE>
__device__ __forceinline__ NearList nearOccluders(f3 P, f3 pn, const float4 *bvh, const float4 *tri4, uint32_t ntri, float dmax,
                                                  const NearGrid &ng, uint32_t *ext, uint32_t extCap, float eps) {
  NearList r{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0.f};
  if (ntri == 0u) return r;
  // (the linear scans run for <= 64 occluders only, nearMode: always the narrow format)
  constexpr bool LINEAR = MODE == NEAR_SCAN_SCALAR || MODE == NEAR_SCAN_VECTOR;
  const bool narrow = LINEAR || ntri <= GVPM_NEAR_NARROW_MAX, wide = !narrow && ntri <= GVPM_NEAR_WIDE_MAX;
  const uint32_t cap = narrow ? 12u : (wide ? 6u : 0u);
  NearScan s{0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0.f};
  if constexpr (MODE == NEAR_SCAN_SCALAR) {
    // i is the same in every lane: the occluder comes through the scalar cache, once, for both tests; ascending i and the
    // expressions of the vector scan, so the lists are the same
    const UniformF32 tab = uniformView(tri4);
    for (uint32_t i = 0; i < ntri; ++i) {
      const Tri3 t = loadTriUniform(tab, i);
      if (nearTriangle(P, t, dmax)) s = nearAppend(s, P, pn, t, i, eps, narrow, cap);
    }
  } else {
    nearVisit<MODE>(P, bvh, tri4, ntri, dmax, ng, [&](uint32_t i) { s = nearAppend(s, P, pn, loadTri(tri4, i), i, eps, narrow, cap); });
  }
  const float cstar = s.cstar;
  r.cstar = cstar;
  const uint32_t capC = cstar > 0.f ? (cap * 2u) / 3u : cap;  // (word 2 is taken)
  if (s.cnt <= capC) {
    r.w0 = s.a0; r.w1 = s.a1; r.w2 = cstar > 0.f ? __float_as_uint(cstar) : s.a2;
    return r;
  }
  // extension list {count, indices}: rare (more near occluders than the inline slots), a second visit with per-lane loads
  const uint32_t off = atomicAdd(ext, s.cnt + 1u);  // ext[0] = the allocation cursor (starts at 1)
  if ((unsigned long long)off + s.cnt + 1u > extCap) {
    r.w0 = 0xFEFFFFFFu;
    return r;
  }
  ext[off] = s.cnt;
  uint32_t k = 0;
  if constexpr (MODE == NEAR_SCAN_SCALAR) {
    for (uint32_t i = 0; i < ntri; ++i) {
      const Tri3 t = loadTri(tri4, i);
      if (nearTriangle(P, t, dmax) && !ownWall(P, pn, t, eps, 0.f).own) ext[off + 1u + (k++)] = i;
    }
  } else {
    nearVisit<MODE>(P, bvh, tri4, ntri, dmax, ng, [&](uint32_t i) {
      if (!ownWall(P, pn, loadTri(tri4, i), eps, 0.f).own) ext[off + 1u + (k++)] = i;
    });
  }
  r.w0 = 0xFDFFFFFFu;
  r.w1 = off;
  if (cstar > 0.f) r.w2 = __float_as_uint(cstar);
  return r;
}

}  // namespace gvpm
