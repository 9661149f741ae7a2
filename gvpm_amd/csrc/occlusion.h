// Occlusion for the gather kernels: the three-state triangle tests, both walks of the occluder BVH, the per-photon
// near-occluder lists and the shadow segment of a reconnection built on them.
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "vec.h"

namespace gvpm {

// Moeller-Trumbore, triangle.h:109-145 + interval test skdtree.h:318-320, in THREE states (round 5).
//
// The reference decides  det != 0, 0 <= u <= 1, v >= 0, u + v <= 1, mint <= t <= maxt  with u = A / C, v = B / C, t = T / C,
// C = e1 . (d x e2), A = tvec . (d x e2), B = d . (tvec x e1), T = e2 . (tvec x e1), tvec = o - v0.  Here the four
// barycentric comparisons are taken division-free on sg A, sg B, |C| (sg = sign C) and the interval test on the plane
// distances of the segment's ends (see triHit3), each with a RIGOROUS fp32 error margin: with eps = 2^-24,
// S = |o|_1 + |v0|_1, L1 = |e1|_1, L2 = |e2|_1 the rounding of the sums above (and the ~1e-7 the device's fp32 direction
// is off the oracle's) is bounded by  errC <= 5 eps L1 L2,  errA <= 8 eps S L2,  errB <= 18 eps S L1;
// the margins take 1e-6 ~ 17 eps.  Outside every margin the decision is the one exact arithmetic
// on the same fp32 data takes -- the fp64 oracle's, and a double-precision reference's.  Inside one:
//   TRI_AMB -- fp32 cannot tell.  The caller DEFERS the shift to the exact pass (exact_shift.hip: the reference's
//   statement in uncontracted fp64), or, where no exact pass exists, takes bit 0: the plain fp32 decision.
// The systematic case is a segment that STARTS within rounding of the triangle's plane -- a parent that fp32 left behind
// the wall it sits on (near_lists.h, ownWall) -- along a grazing direction: the plane distance of the start is pure
// rounding residue and t >= mint is decided by it.  The generic near-threshold cases (a hit within 1e-6 of an edge) go the same way.
#define GVPM_TRI_MISS 0
#define GVPM_TRI_HIT 1
#define GVPM_TRI_AMB 2
// s0 = n . (o - v0), sd = n . d with the stored unit normal (callers have them for the plane-side early-out).  The interval
// test  mint <= t <= maxt  is the statement "the segment's ends lie on different sides of the triangle's plane":
// e0 = s0 + sd mint and e1 = s0 + sd maxt, each good to mE ~ 5e-7 (|o|_1 + |v0|_1 + maxt) -- eight times tighter than the
// same decision through T = e2 . (tvec x e1), whose rounding carries the triangle's extent.
__device__ __forceinline__ int triHit3(f3 v0, f3 e1, f3 e2, f3 o, f3 d, float mint, float maxt, float oAbs1, float s0, float sd) {
  const f3 pvec = cross(d, e2);
  const float C = dot(e1, pvec);
  const f3 tvec = o - v0;
  const float A = dot(tvec, pvec);
  const f3 qvec = cross(tvec, e1);
  const float Bq = dot(d, qvec);
  const float L1 = fabsf(e1.x) + fabsf(e1.y) + fabsf(e1.z), L2 = fabsf(e2.x) + fabsf(e2.y) + fabsf(e2.z);
  const float S = oAbs1 + fabsf(v0.x) + fabsf(v0.y) + fabsf(v0.z);
  const float k = 1e-6f;
  const float mC = k * L1 * L2, mA = k * S * L2, mB = k * S * L1, mE = 5e-7f * (S + maxt);
  const float aC = fabsf(C);
  const float sA = C < 0.f ? -A : A, sB = C < 0.f ? -Bq : Bq;
  const float s2 = aC - sA, s4 = s2 - sB;
  const float m2 = mA + mC, m4 = m2 + mB;
  const float e0 = s0 + sd * mint, e1p = s0 + sd * maxt;
  const float lo = fminf(e0, e1p), hi = fmaxf(e0, e1p);
  const bool noCross = lo > mE || hi < -mE, cross = lo < -mE && hi > mE;
  // (an EMPTY interval, mint > maxt -- the as-written visibility of a reconnection shorter than Epsilon / ShadowEpsilon: the
  // reference's mint <= t <= maxt holds for no t.  The ends' sides are symmetric in the two: a plane certainly crossed between
  // them is then a certain miss -- found by tests/stress_vpm.py, a medium parent 1e-4 from a wall)
  const bool empty = mint > maxt;
  const bool fail = noCross || (cross && empty) || sA < -mA || s2 < -m2 || sB < -mB || s4 < -m4;
  const bool pass = cross && !empty && aC > mC && sA > mA && s2 > m2 && sB > mB && s4 > m4;
  return fail ? GVPM_TRI_MISS : (pass ? GVPM_TRI_HIT : GVPM_TRI_AMB);
}
__device__ __forceinline__ int triHit3(const float4 t0, const float4 t1, const float4 t2, f3 o, f3 d, float mint, float maxt, float oAbs1) {
  const f3 v0 = mk3(t0.x, t0.y, t0.z), nrm = mk3(t0.w, t1.w, t2.w);
  return triHit3(v0, mk3(t1.x, t1.y, t1.z), mk3(t2.x, t2.y, t2.z), o, d, mint, maxt, oAbs1, dot(nrm, o - v0), dot(nrm, d));
}
// A second opinion on a triangle triHit3 left undecided (the G-Beams shadow segments, beams_shift_f32.h).  The division-free
// comparisons above bound the errors of A, B and C independently -- each carries |o - v0| |e|, the distance to the triangle's
// FAR corner -- although an error of the direction moves A / C only by the lever from the origin to the crossing point.
// Here the crossing point itself is formed, P = (o - v0) + d t with t = -s0 / sd, and tested against the edges in the
// triangle's plane: its error is ~4u (|o - v0| + t) of rounding, dirErr t of the direction (the device's fp32 direction
// against the reference's: dirErr ~ 1e-6) and the plane distance's own error over |sd| -- 1e-6 of the scene where the
// margins above are 1e-5 |e| / sin(crossing angle): the plate of S-laser, whose thin triangles' edge LINES run through the
// aperture, went from 2.8 % undecided shadow segments to ~0.03 %.  The normal is recomputed (N = e1 x e2: a point exactly in
// an axis plane gets a plane distance of exactly zero error).  endErr: absolute error of the segment's end point.
__device__ __forceinline__ int triHitFine(f3 v0, f3 e1, f3 e2, f3 o, f3 d, float mint, float maxt, float dirErr, float endErr) {
  const f3 tv = o - v0;  // (one rounding per component)
  const f3 N = cross(e1, e2);
  const float n1 = fabsf(N.x) + fabsf(N.y) + fabsf(N.z);
  const float s0 = dot(N, tv), sd = dot(N, d);
  const float a0 = fabsf(N.x * tv.x) + fabsf(N.y * tv.y) + fabsf(N.z * tv.z);
  const float t1 = fabsf(tv.x) + fabsf(tv.y) + fabsf(tv.z);
  const float eS = s0 + sd * mint, eE = s0 + sd * maxt;
  const float mS = 5e-7f * (a0 + fabsf(sd) * mint) + n1 * dirErr * mint;
  const float mE = 5e-7f * (a0 + fabsf(sd) * maxt) + n1 * endErr;
  const bool sP = eS > mS, sN = eS < -mS, eP = eE > mE, eN = eE < -mE;
  if ((sP && eP) || (sN && eN)) return GVPM_TRI_MISS;
  if (!((sP && eN) || (sN && eP))) return GVPM_TRI_AMB;
  if (mint > maxt) return GVPM_TRI_MISS;  // (an empty interval whose ends certainly straddle the plane: see triHit3)
  const float isd = frcp(sd);
  const float t = -s0 * isd;
  const f3 P = tv + d * t;
  const float p1n = fabsf(P.x) + fabsf(P.y) + fabsf(P.z);
  // position error of P: rounding of tv + d t, the direction's error over t, the plane distance's error over |sd|
  const float pe = 3e-7f * (t1 + t + p1n) + dirErr * t + 5e-7f * a0 * fabsf(isd);
  const float l1 = fabsf(e1.x) + fabsf(e1.y) + fabsf(e1.z), l2 = fabsf(e2.x) + fabsf(e2.y) + fabsf(e2.z);
  const float NN = dot(N, N);
  // one edge function per edge, each with the margin of ITS edge (u + v <= 1 taken as 1 - u - v would add the margins of two
  // nearly parallel edges of a thin triangle: forty times the third edge's own)
  const f3 e3 = e2 - e1;
  const float l3 = fabsf(e3.x) + fabsf(e3.y) + fabsf(e3.z);
  const float uN = dot(cross(P, e2), N), vN = dot(cross(e1, P), N), wN = dot(cross(e3, P - e1), N);
  const float mu = pe * l2 * n1, mv = pe * l1 * n1, mw = (pe + 2e-7f * l1) * l3 * n1;
  if (!(NN > 0.f)) return GVPM_TRI_AMB;
  if (uN < -mu || vN < -mv || wN < -mw) return GVPM_TRI_MISS;
  if (uN > mu && vN > mv && wN > mw) return GVPM_TRI_HIT;
  return GVPM_TRI_AMB;
}
// any-hit over a list: a certain hit settles it; else an undecidable triangle makes the whole answer undecidable
__device__ __forceinline__ int triCombine(int acc, int t) {
  if (acc == GVPM_TRI_HIT || t == GVPM_TRI_HIT) return GVPM_TRI_HIT;
  return (acc | t) & GVPM_TRI_AMB;
}
// the plain fp32 test (branch-free: the tests of the reference are and-ed; a zero determinant gives inf / NaN, which fail
// the comparisons like the early return): probe builds' plain visibility (GVPM_PROBE_PLAINVIS); the literal fp64 cross-check of
// G-Beams (GVPM_BEAMS_FP64) walked the scene with it until its shadow segments went to anyHitExact
__device__ __forceinline__ bool triHit(f3 v0, f3 e1, f3 e2, f3 o, f3 d, float mint, float maxt) {
  const f3 pvec = cross(d, e2);
  const float det = dot(e1, pvec);
  const float inv = frcp(det);
  const f3 tvec = o - v0;
  const float u = dot(tvec, pvec) * inv;
  const f3 qvec = cross(tvec, e1);
  const float v = dot(d, qvec) * inv;
  const float t = dot(e2, qvec) * inv;
  return det != 0.f && u >= 0.f && u <= 1.f && v >= 0.f && u + v <= 1.f && t >= mint && t <= maxt;
}
// The same test in uncontracted fp64, in the operation order of the oracle's (and the reference's) statement.
__device__ __forceinline__ bool triHitExact(f3 v0f, f3 e1f, f3 e2f, f3 of, d3 dd, double mint, double maxt) {
#pragma clang fp contract(off)
  const double e1x = e1f.x, e1y = e1f.y, e1z = e1f.z, e2x = e2f.x, e2y = e2f.y, e2z = e2f.z;
  const double dx = dd.x, dy = dd.y, dz = dd.z;
  const double px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
  const double det = e1x * px + e1y * py + e1z * pz;
  if (det == 0.0) return false;
  const double inv = 1.0 / det;
  const double tx = (double)of.x - (double)v0f.x, ty = (double)of.y - (double)v0f.y, tz = (double)of.z - (double)v0f.z;
  const double u = (tx * px + ty * py + tz * pz) * inv;
  if (u < 0.0 || u > 1.0) return false;
  const double qx = ty * e1z - tz * e1y, qy = tz * e1x - tx * e1z, qz = tx * e1y - ty * e1x;
  const double v = (dx * qx + dy * qy + dz * qz) * inv;
  if (!(v >= 0.0 && u + v <= 1.0)) return false;
  const double t = (e2x * qx + e2y * qy + e2z * qz) * inv;
  return t >= mint && t <= maxt;
}

// scene->rayIntersect(ray), any-hit, exactly: the occluder BVH's boxes are padded (scene_bvh.cpp), the slab test runs in
// fp64 on them -- conservative -- and every triangle of a reached leaf takes the reference's test in fp64.
static __device__ bool anyHitExact(const GatherArgs &a, f3 o, d3 d, double mint, double maxt) {
#pragma clang fp contract(off)
  if (a.ntri == 0u) return false;
  const double ox = o.x, oy = o.y, oz = o.z;
  const double ix = 1.0 / d.x, iy = 1.0 / d.y, iz = 1.0 / d.z;
  uint32_t stack[32];
  int sp = 0;
  uint32_t cur = 0;
  for (;;) {
    const float4 lo = a.bvh[2 * (size_t)cur], hi = a.bvh[2 * (size_t)cur + 1];
    const double tx0 = ((double)lo.x - ox) * ix, tx1 = ((double)hi.x - ox) * ix;
    const double ty0 = ((double)lo.y - oy) * iy, ty1 = ((double)hi.y - oy) * iy;
    const double tz0 = ((double)lo.z - oz) * iz, tz1 = ((double)hi.z - oz) * iz;
    // (fmin / fmax drop the NaNs of 0 * inf; a box is entered when in doubt: slack of 1e-9 on the interval)
    const double tn = fmax(fmax(fmin(tx0, tx1), fmin(ty0, ty1)), fmax(fmin(tz0, tz1), mint)) - 1e-9;
    const double tf = fmin(fmin(fmax(tx0, tx1), fmax(ty0, ty1)), fmin(fmax(tz0, tz1), maxt)) + 1e-9;
    bool descend = false;
    if (tn <= tf) {
      const uint32_t first = __float_as_uint(lo.w), count = __float_as_uint(hi.w);
      if (count == 0u) {
        if (sp < 32) stack[sp++] = first + 1u;
        cur = first;
        descend = true;
      } else {
        for (uint32_t i = first; i < first + count; ++i) {
          const float4 t0 = a.tri4[3 * (size_t)i], t1 = a.tri4[3 * (size_t)i + 1], t2 = a.tri4[3 * (size_t)i + 2];
          if (triHitExact(mk3(t0.x, t0.y, t0.z), mk3(t1.x, t1.y, t1.z), mk3(t2.x, t2.y, t2.z), o, d, mint, maxt)) return true;
        }
      }
    }
    if (!descend) {
      if (sp == 0) return false;
      cur = stack[--sp];
    }
  }
}

// scene->rayIntersect(ray), any-hit: stack walk of the occluder BVH (scene_bvh.h), triangles as
// {v0,n.x} {e1,n.y} {e2,n.z} in leaf order.  Deliberately not inlined: it is the rare path (the
// as-written shadow segment is served by the per-photon near-occluder list below) and inlining
// it cost the evaluation kernels ~160 VGPRs.  Returns a GVPM_TRI_* state.
template <bool PLAIN = false>
static __device__ __noinline__ int anyHitScene(const float4 *bvh, const float4 *tri4, uint32_t ntri, f3 o, f3 d, float mint,
                                        float maxt) {
  if (ntri == 0u) return GVPM_TRI_MISS;
  const f3 inv = mk3(1.f / d.x, 1.f / d.y, 1.f / d.z);
  const float oAbs1 = fabsf(o.x) + fabsf(o.y) + fabsf(o.z);
  uint32_t stack[32];
  int sp = 0;
  uint32_t cur = 0;
  int res = GVPM_TRI_MISS;
  for (;;) {
    const float4 lo = bvh[2 * (size_t)cur], hi = bvh[2 * (size_t)cur + 1];
    // slab test; fminf/fmaxf drop the NaNs of 0 * inf
    const float tx0 = (lo.x - o.x) * inv.x, tx1 = (hi.x - o.x) * inv.x;
    const float ty0 = (lo.y - o.y) * inv.y, ty1 = (hi.y - o.y) * inv.y;
    const float tz0 = (lo.z - o.z) * inv.z, tz1 = (hi.z - o.z) * inv.z;
    const float tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), mint));
    const float tf = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fminf(fmaxf(tz0, tz1), maxt));
    bool descend = false;
    if (tn <= tf) {
      const uint32_t first = __float_as_uint(lo.w), count = __float_as_uint(hi.w);
      if (count == 0u) {
        if (sp < 32) stack[sp++] = first + 1u;
        cur = first;
        descend = true;
      } else {
        for (uint32_t i = first; i < first + count; ++i) {
          if (PLAIN) {
            // (PLAIN: the fp64 cross-check of G-Beams -- its shadow segment's direction is the double one, rounded once)
            const float4 t0 = tri4[3 * (size_t)i], t1 = tri4[3 * (size_t)i + 1], t2 = tri4[3 * (size_t)i + 2];
            if (triHit(mk3(t0.x, t0.y, t0.z), mk3(t1.x, t1.y, t1.z), mk3(t2.x, t2.y, t2.z), o, d, mint, maxt)) return GVPM_TRI_HIT;
          } else {
            res = triCombine(res, triHit3(tri4[3 * (size_t)i], tri4[3 * (size_t)i + 1], tri4[3 * (size_t)i + 2], o, d, mint, maxt, oAbs1));
            if (res == GVPM_TRI_HIT) return res;
          }
        }
      }
    }
    if (!descend) {
      if (sp == 0) return res;
      cur = stack[--sp];
    }
  }
}

// As written (shift_volume_photon.cpp:396) the shadow segment is [Epsilon, lProj*ShadowEpsilon]
// from the photon's parent: only occluders within that distance of the parent can be hit.  The
// grid build lists them per photon (reorder_kernel: up to 12 byte indices in the three spare
// words of the record), so the loop touches 0-12 triangles.  FULLVIS kernels (intended visibility,
// more than 254 occluders, or a photon whose list overflowed) walk the BVH instead; the fast
// kernels carry no call, which is worth ~30 VGPRs.
// Margin of the plane-side early-out in front of a triangle test: the signed distances s0 + sd * t of the segment's
// two ends to the triangle's plane are fp32 sums of products of O(|o|_1 + |v0|_1) and O(maxt) operands, so their
// rounding error is a few ulps of that magnitude.  A triangle is skipped only when BOTH ends lie on one side by MORE
// than this margin; anything closer goes to triHit3, which decides as the reference's rayIntersect does -- or says it cannot.
__device__ __forceinline__ float planeSideMargin(float triAbs1, f3 o, float maxt) {
  return 2e-6f * (fabsf(o.x) + fabsf(o.y) + fabsf(o.z) + triAbs1 + maxt);
}
__device__ __forceinline__ bool planeSideMiss(float s0, float sd, float mint, float maxt, float margin) {
  const float e0 = s0 + sd * mint, e1 = s0 + sd * maxt;
  return fminf(e0, e1) > margin || fmaxf(e0, e1) < -margin;
}

template <bool PLAIN = false>
__device__ __forceinline__ int nearListHit(const float4 *tri, uint32_t nl0, uint32_t nl1, uint32_t nl2, f3 o, f3 d,
                                           float mint, float maxt, float margin) {
  int res = GVPM_TRI_MISS;
  const float oAbs1 = fabsf(o.x) + fabsf(o.y) + fabsf(o.z);
  uint32_t l = nl0;
#pragma unroll 1
  for (int k = 0; k < 12; ++k) {
    const uint32_t i = l & 0xFFu;
    if (i == 0xFFu) break;
    l = k == 3 ? nl1 : (k == 7 ? nl2 : (l >> 8) | 0xFF000000u);
    const float4 t0 = tri[3 * i], t1 = tri[3 * i + 1], t2 = tri[3 * i + 2];
    // both ends of the segment strictly on one side of the triangle's plane (the stored unit normal; zero for a
    // degenerate triangle, which then goes to the full test): nothing to intersect -- a quarter of the work of the test
    // it spares, and at C3 a third of a beam's listed occluders (ceiling and floor under and above a vertical beam)
    const f3 v0 = mk3(t0.x, t0.y, t0.z), nrm = mk3(t0.w, t1.w, t2.w);
    const float s0 = dot(nrm, o - v0), sd = dot(nrm, d);
    if (planeSideMiss(s0, sd, mint, maxt, margin)) continue;
    if (PLAIN) res |= triHit(v0, mk3(t1.x, t1.y, t1.z), mk3(t2.x, t2.y, t2.z), o, d, mint, maxt) ? GVPM_TRI_HIT : GVPM_TRI_MISS;
    else res = triCombine(res, triHit3(v0, mk3(t1.x, t1.y, t1.z), mk3(t2.x, t2.y, t2.z), o, d, mint, maxt, oAbs1, s0, sd));
  }
  return res;
}
// the same for scenes of more than 254 occluders: six 16-bit indices (near_lists.h, nearOccluders)
__device__ __forceinline__ int nearListHitWide(const float4 *tri, uint32_t nl0, uint32_t nl1, uint32_t nl2, f3 o, f3 d,
                                               float mint, float maxt) {
  int res = GVPM_TRI_MISS;
  const float oAbs1 = fabsf(o.x) + fabsf(o.y) + fabsf(o.z);
  uint32_t l = nl0;
#pragma unroll 1
  for (int k = 0; k < 6; ++k) {
    const uint32_t i = l & 0xFFFFu;
    if (i == 0xFFFFu) break;
    l = k == 1 ? nl1 : (k == 3 ? nl2 : (l >> 16) | 0xFFFF0000u);
    res = triCombine(res, triHit3(tri[3 * (size_t)i], tri[3 * (size_t)i + 1], tri[3 * (size_t)i + 2], o, d, mint, maxt, oAbs1));
  }
  return res;
}
// extension list (lists longer than the inline slots; every list of a scene beyond 16-bit indices)
__device__ __forceinline__ int nearListHitExt(const float4 *tri, const uint32_t *ext, uint32_t off, f3 o, f3 d,
                                              float mint, float maxt) {
  int res = GVPM_TRI_MISS;
  const float oAbs1 = fabsf(o.x) + fabsf(o.y) + fabsf(o.z);
  const uint32_t n = ext[off];
#pragma unroll 1
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t i = ext[off + 1u + k];
    res = triCombine(res, triHit3(tri[3 * (size_t)i], tri[3 * (size_t)i + 1], tri[3 * (size_t)i + 2], o, d, mint, maxt, oAbs1));
  }
  return res;
}
// ldsTri: the occluders staged in LDS by the kernel (small scenes), or null.  Returns a GVPM_TRI_* state.
template <bool FULLVIS>
__device__ __forceinline__ int shadowBlocked(const GatherArgs &a, const float4 *ldsTri, uint32_t nl0, uint32_t nl1,
                                             uint32_t nl2, f3 o, f3 d, float mint, float maxt) {
#ifdef GVPM_PROBE_PLAINVIS
  constexpr bool PL = true;  // probe builds only: what the three-state test costs
#else
  constexpr bool PL = false;
#endif
  if (FULLVIS) return anyHitScene<PL>(a.bvh, a.tri4, a.ntri, o, d, mint, maxt);
  if (a.ntri > GVPM_NEAR_NARROW_MAX) {
    if ((nl0 >> 24) == 0xFDu) return nearListHitExt(a.tri4, a.nearExt, nl1, o, d, mint, maxt);
    return nearListHitWide(a.tri4, nl0, nl1, nl2, o, d, mint, maxt);
  }
  if ((nl0 >> 24) == 0xFDu) return nearListHitExt(a.tri4, a.nearExt, nl1, o, d, mint, maxt);
  const float margin = planeSideMargin(a.triAbs1, o, maxt);
  return ldsTri ? nearListHit<PL>(ldsTri, nl0, nl1, nl2, o, d, mint, maxt, margin)
                : nearListHit<PL>(a.tri4, nl0, nl1, nl2, o, d, mint, maxt, margin);
}

}  // namespace gvpm
