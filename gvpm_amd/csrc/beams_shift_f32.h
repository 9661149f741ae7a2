// The fp32 local-frame evaluation of G-Beams above the kernel record of beams_eval_f32.h: the exact settlement of the
// banded decisions (beamKernelExact, through the transcription of beams_eval_f64.h), the visibility of a reconnection's new
// beam over the near lists, the reconnection itself, the request a manifold-typed shift leaves for the host, and the three
// steps the evaluation kernels are built from -- beamBase (kernel record + base term), beamShift1 (null shifts, the
// reconnections queued), beamShift2 (the queued reconnections).  The fused kernel (gather_beams.hip) and the split pair
// (gather_beams_split.hip) include it; each unit gets its own copy of the static __noinline__ functions.
#pragma once
#include <hip/hip_runtime.h>

#include "beams_common.h"
#include "beams_eval_f32.h"
#include "beams_eval_f64.h"
#include "device_types.h"
#include "dmath.h"
#include "shift_device.h"
#include "tile_walk.h"
#include "vec.h"

namespace gvpm {

#ifdef GVPM_BEAMS_AUDIT
// probe builds only (bash scripts/build_variant.sh baudit gather_beams.hip -DGVPM_BEAMS_AUDIT; scripts/beams_audit.py):
// the fp32 kernel record runs the fp64 transcription for EVERY pair and logs (i) the pairs whose banded fp32 decision
// was taken as sure and differs from the transcription's, (ii) the largest observed |fp32 - fp64| / band per quantity
// over the pairs both accept: the safety factor of each band.  One copy per unit built with the macro (static); the reader,
// gvpm_debug_beams_audit, is gather_beams.hip's and reads that unit's.
static __device__ unsigned int gvpmAuditCount;
static __device__ float gvpmAuditLog[256][16];
static __device__ unsigned int gvpmAuditRatio[8];  // float bits (positive): [0] tN [1] v [2] w [3] pdfKernel (relative, no band)
#endif

// The geometric part of BeamKernelRecord::eval for sub-beam `sub` of a (camera ray, beam) pair in the fp64
// transcription -- every validity decision of the reference up to the radiometry (3D: cylinderIntersection, the
// ownership rule, v in [0, len], the kernel centre inside the ray's cylinder, w in [mint, maxt]; 1D: all of
// rayIntersectInternal1D with its float intermediates) -- and the numbers the rest of the evaluation is built on:
// v, w, pdfKernel (1D: sin theta) and u.  The fp32 evaluation calls it for the pairs one of whose decisions falls
// inside its fp32 error band (3D), and for every pair of the 1D kernel, whose reference derives v from float dot
// products of absolute positions (beams_struct.h:275-290): its result follows the reference's rounding, not the
// geometry, and only the transcription reproduces it.  The evaluated set is therefore the fp64 oracle's.
static __device__ __noinline__ bool beamKernelExact(f3 p1f, f3 p2f, f3 of, f3 df, float camLen, float eps, float radius,
                                                    uint32_t sub, float subLen, int technique, float uvf, float uwf,
                                                    double &vOut, double &wOut, double &pdfOut, double &uOut,
                                                    double *dbg = nullptr) {
  BeamD b;
  b.p1 = tod(p1f);
  b.p2 = tod(p2f);
  b.dir = b.p2 - b.p1;
  b.len = sqrt(dotU(b.dir, b.dir));  // (uncontracted: the oracle's length and direction to the bit, see rayIntersect1D)
  b.dir = b.dir / b.len;
  const uint32_t nSub = subBeamCount((float)b.len, subLen);
  const float ls = (float)b.len / (float)nSub;
  const double tmin = (double)(ls * (float)sub);
  double tmax = (sub + 1u >= nSub) ? INFINITY : (double)(ls * (float)(sub + 1u));
  if (tmax > b.len) tmax = b.len;
  const RayD cam{tod(of), tod(df), (double)eps, (double)camLen - (double)eps};
  vOut = wOut = pdfOut = uOut = 0.0;
  if (technique == GVPM_BEAM_BEAM_1D) {
    double u, v, w, st;
    if (!beamOwner1D(b, cam, sub, nSub, tmin, tmax)) return false;
    if (!rayIntersect1D(b, (double)radius, cam, 0.0, b.len, u, v, w, st)) return false;
    vOut = v; wOut = w; pdfOut = st; uOut = u;
    return true;
  }
  // BeamKernelRecord::eval (3D), shift_volume_beams.h:157-290, as krecEval above
  const RayD _cam{at(cam, cam.mint), cam.d, 0.0, cam.maxt - cam.mint};
  const RayD _beam{b.p1, b.dir, 0.0, b.len};
  double tN, tF;
  if (dbg) dbg[0] = 1.0;
  if (!cylinderIntersection(_cam, _beam, (double)radius, tN, tF)) return false;
  if (dbg) { dbg[0] = 2.0; dbg[1] = tN; dbg[2] = tF; }
  if (!((tN < 0 && tmin <= (double)eps) || (tN > tmin && tN < tmax))) return false;
  const double v = tN + (tF - tN) * (double)uvf;
  double pdfK = 1.0 / fmax(tF - tN, 0.0001);
  if (dbg) { dbg[0] = 3.0; dbg[3] = v; }
  if (v < 0 || v > b.len) return false;
  const d3 kc = b.p1 + b.dir * v;
  const double distToProj = dot(kc - cam.o, cam.d);
  const double distSqr = len2(at(cam, distToProj) - kc);
  const double radSqr = (double)radius * (double)radius;
  if (dbg) { dbg[0] = 4.0; dbg[4] = distSqr; }
  if (distSqr >= radSqr) return false;
  const double deltaT = sqrt(fmax(0.0, radSqr - distSqr));
  const double w = distToProj - deltaT + 2 * deltaT * (double)uwf;
  pdfK *= 1.0 / fmax(2.0 * deltaT, 0.0001);
  if (dbg) { dbg[0] = 5.0; dbg[5] = w; }
  if (w < cam.mint || w > cam.maxt) return false;
  vOut = v; wOut = w; pdfOut = pdfK;
  if (dbg) dbg[0] = 6.0;
  return true;
}

// Occluders of a small scene staged in LDS once per (persistent) workgroup: the visibility test of the beam
// reconnection then is a wave-uniform loop over every triangle (broadcast LDS reads, no divergence, no memory
// latency) instead of a per-lane stack walk of the BVH in global memory, which at one or two waves per SIMD was
// latency-bound and cost more than the rest of the evaluation together.
constexpr uint32_t SCENE_LDS_TRIS = 128;

// shiftBeamDiffuse + diffuseReconnectionPhotonBeam (shift_volume_beams.cpp:410-539, shift_diffuse.cpp:136-268) in
// the local frame.
//
// Visibility over the whole new beam [Epsilon, dist] (shift_volume_beams.cpp:420-426): the occluders listed near the
// beam (beam_near_kernel, beams_build.hip), or all of them when the list overflowed / the scene is large.
// One loop for the lanes that walk their beam's list and the lanes whose list overflowed (every occluder).  In a wave of 64
// unrelated segments some lane's triangle always passes the plane-side early-out, so every trip (the longest list:
// 16-19) runs the full Moeller-Trumbore test; marking the crossed planes first and testing only those in a second loop
// was measured at C3: 30.0 ms against 22.6 (two decodes and two rounds of LDS reads per entry).  What pays is not
// entering the loop: beamShift2 sends only the reconnections outside their beam's free cone through it.
// (TRI: the occluders in LDS or in global memory -- one loop for the lanes that walk their beam's list and, in LDS, the lanes
// whose list overflowed: every occluder)
// the triangles triHit3 left undecided once more, through the crossing point (occlusion.h, triHitFine).  Rare (a few
// per cent of the segments that take the loop) and not inlined: inlined, its temporaries cost the evaluation kernel 23 spilled
// registers.  The new beam's direction is good to ~1e-6 of the reference's, its end point (the offset position) to endErr.
static __device__ __noinline__ int beamNearRefine(const BeamNearFmt fmt, bool ovf, uint32_t nl0, uint32_t nl1, uint32_t nl2, const float4 *tri,
                                                  f3 o, f3 nd, float mint, float maxt, float endErr, uint32_t ambMask) {
  int res = GVPM_TRI_MISS;
  while (ambMask) {
    const uint32_t k = (uint32_t)__builtin_ctz(ambMask);
    ambMask &= ambMask - 1u;
    const uint32_t i = ovf ? k : beamNearEntry(fmt, nl0, nl1, nl2, k);
    const float4 t0 = tri[3 * i], t1 = tri[3 * i + 1], t2 = tri[3 * i + 2];
    res = triCombine(res, triHitFine(mk3(t0.x, t0.y, t0.z), mk3(t1.x, t1.y, t1.z), mk3(t2.x, t2.y, t2.z), o, nd, mint, maxt, 1e-6f, endErr));
  }
  return res;
}
// (round 5: three states, occlusion.h triHit3 -- MISS, HIT, or AMB: some listed triangle's test lies inside its fp32 margin
// and none is a certain hit; the reconnection then goes to the exact pass)
__device__ __forceinline__ int beamNearLoop(const GatherArgs &a, const BeamNearFmt fmt, bool ovf, const BeamF &b, const float4 *tri, f3 nd,
                                            float dist) {
  const f3 o = b.p1;
  const float mint = a.cfg.epsilon, maxt = dist;
  const float margin = planeSideMargin(a.triAbs1, o, maxt);
  const float oAbs1 = fabsf(o.x) + fabsf(o.y) + fabsf(o.z);
  bool hit = false;
  uint32_t ambMask = 0u;  // list positions triHit3 left undecided (a 33rd makes the segment undecidable as a whole)
  bool ambMore = false;
  bool more1 = true;
#pragma unroll 1
  for (uint32_t k = 0;; ++k) {
    uint32_t i;
    if (ovf) {
      i = k;
      more1 = k < a.ntri;
    } else {
      i = k < fmt.cap ? beamNearEntry(fmt, b.nl0, b.nl1, b.nl2, k) : fmt.mask;
      more1 = more1 && i != fmt.mask;
    }
    if (__ballot(more1) == 0ull) break;
    if (more1) {
      const float4 t0 = tri[3 * i], t1 = tri[3 * i + 1], t2 = tri[3 * i + 2];
      const f3 v0 = mk3(t0.x, t0.y, t0.z), nrm = mk3(t0.w, t1.w, t2.w);
      const float s0 = dot(nrm, o - v0), sd = dot(nrm, nd);
      if (!planeSideMiss(s0, sd, mint, maxt, margin)) {
        const int th = triHit3(v0, mk3(t1.x, t1.y, t1.z), mk3(t2.x, t2.y, t2.z), o, nd, mint, maxt, oAbs1, s0, sd);
        hit = hit || th == GVPM_TRI_HIT;
        if (th == GVPM_TRI_AMB) {
          if (k < 32u) ambMask |= 1u << k; else ambMore = true;
        }
      }
    }
  }
  if (hit) return GVPM_TRI_HIT;
  if (ambMore) return GVPM_TRI_AMB;
  if (ambMask == 0u) return GVPM_TRI_MISS;
  return beamNearRefine(fmt, ovf, b.nl0, b.nl1, b.nl2, tri, o, nd, mint, maxt, 1e-6f * (beamLocalScale(a) + dist), ambMask);
}

// a GVPM_TRI_* state
__device__ __forceinline__ int beamShadowBlocked(const GatherArgs &a, const BeamF &b, const float4 *ldsTri, f3 nd, float dist) {
  const BeamNearFmt fmt = beamNearFmt(a.ntri);  // (wave-uniform)
  const bool ovf = beamNearOverflow(fmt, b.nl0, b.nl2);
  if (!ldsTri) {
    // (more occluders than the kernel's LDS holds: the lists' triangles from global memory; a list that overflowed walks the BVH)
    if (ovf) return anyHitScene<false>(a.bvh, a.tri4, a.ntri, b.p1, nd, a.cfg.epsilon, dist);
    if (fmt.bits == 8u)
      return nearListHit<false>(a.tri4, b.nl0, b.nl1, b.nl2, b.p1, nd, a.cfg.epsilon, dist, planeSideMargin(a.triAbs1, b.p1, dist));
    return beamNearLoop(a, fmt, false, b, a.tri4, nd, dist);
  }
  return beamNearLoop(a, fmt, ovf, b, ldsTri, nd, dist);
}

__device__ __forceinline__ bool beamBorder(const GatherArgs &a, uint32_t pix, int i);

// ---- manifold shifts through the host for G-Beams (gvpm_enable_host_shifts; shiftBeamME, shift_volume_beams.cpp:601-746) ----
// A manifold-typed beam's shift needs Mitsuba's walk (generateShiftPathME + ShiftME over the functor's cached source path,
// :541-599,612-646): the request carries what the walk takes -- beam, set, shifted ray, the offset position newPos, the radius,
// baseCameraRay(w - mint) / shiftRay(w - mint) (:627-628), w, and the kernel's place v on the beam (cacheSourcePath moves
// vertex c there) -- and FIVE float4 of device context: {shifted ray o, maxt} {d, w} {base term * weights, weightKernel * rr}
// {eye, sensorMIS} {radius, pixel, shift, -}.  Rare and register hungry: not inlined.  False: the list is full.
static __device__ __noinline__ bool recordBeamShiftRequest(ReqSink a, uint32_t beamIdx, uint32_t set, int i, f3 offsetAbs,
                                                           f3 basePt, f3 shiftPt, float w, float v, float kpdfBase, float radius, f3 shO, float shMaxt,
                                                           f3 shD, f3 bcv, float wkrr, f3 eye, float sMIS, uint32_t pix) {
  const uint32_t slot = atomicAdd(a.count, 1u);
  if (slot >= a.cap) return false;
  gvpm_shift_request rq;
  rq.photon = beamIdx;
  rq.set = set;
  rq.shift = (uint32_t)i;
  rq.reserved = __float_as_uint(kpdfBase);  // kRec.pdf(): the pdf cacheSourcePath gives the re-cut last edge (:574)
  rq.offset_pos[0] = offsetAbs.x; rq.offset_pos[1] = offsetAbs.y; rq.offset_pos[2] = offsetAbs.z;
  rq.radius = radius;
  rq.base_point[0] = basePt.x; rq.base_point[1] = basePt.y; rq.base_point[2] = basePt.z;
  rq.t = w;
  rq.shift_point[0] = shiftPt.x; rq.shift_point[1] = shiftPt.y; rq.shift_point[2] = shiftPt.z;
  rq.reserved2 = v;
  a.host[slot] = rq;
  float4 *c = a.ctx + 5 * (size_t)slot;
  c[0] = make_float4(shO.x, shO.y, shO.z, shMaxt);
  c[1] = make_float4(shD.x, shD.y, shD.z, w);
  c[2] = make_float4(bcv.x, bcv.y, bcv.z, wkrr);
  c[3] = make_float4(eye.x, eye.y, eye.z, sMIS);
  c[4] = make_float4(radius, __uint_as_float(pix), __uint_as_float((uint32_t)i), 0.f);
  return true;
}

// what the reconnections of one pair share (diffuseReconnectionPhotonBeam's base side, the medium up to w)
struct BeamRecPair {
  float pdfBasePos;   // parentPdf * |p1 - p2|^2 [/ |n_end . d|] / v^2
  float trW;          // transmittance of the camera ray up to w (the shifted rays keep w)
  float pdfKernelAndDist;
  float trOverKernelAndDist;  // the new beam's transmittance over pdfKernelAndDist (beamShift2: from the lengths' difference)
};

// one reconnection once its new beam p1 -> newPos is known to be unoccluded: nd / dist its direction and length
__device__ __forceinline__ float reconnectBeamF(const GatherArgs &a, const BeamF &b, const BeamRecPair &pr, f3 shEye, float sMIS,
                                                const LocalRay &sr, f3 newPos, f3 nd, float dist, int technique,
                                                f3 &shiftedFlux, bool &ok, bool &amb) {
  ok = false;
  shiftedFlux = mk3(0.f);
  const uint32_t ptype = GVPM_PF_PARENT_TYPE(b.flags);
  f3 thr;
  float pdfValueSA;
  bool pdfTiny = false;
  if (ptype == GVPM_PARENT_SURFACE || ptype == GVPM_PARENT_SURFACE_BSDF) {
    const float cosWo = dot(b.parentN, nd), cosWi = dot(b.parentN, b.parentWi);
    // (the new beam's direction is good to ~1e-6: a cosine this close to zero is the exact pass's to sign)
    if (fabsf(cosWo) <= 1e-5f || fabsf(cosWi) <= 1e-5f) amb = true;
    if (cosWo <= 0.f || (ptype == GVPM_PARENT_SURFACE_BSDF ? cosWi == 0.f : cosWi <= 0.f)) return 1.f;
    thr = b.parentScat * (INV_PI_F * cosWo);
    pdfValueSA = INV_PI_F * cosWo;
    if (ptype == GVPM_PARENT_SURFACE_BSDF) {
      uint32_t gst = 0u;
      if (!glossyParentEval(a, b.parentG, b.parentScat, b.parentN, b.parentWi, nd, cosWi, cosWo, thr, pdfValueSA, &gst)) return 1.f;
      // (a pdf that underflowed here but not in the reference's double -- the specular component of a Phong wall alone: the
      // shift succeeds there with weight 1 and a flux that rounds to zero; inside the band of the double's own underflow the
      // exact pass decides)
      pdfTiny = (gst & 1u) != 0u;
      if (gst & 2u) amb = true;
    }
  } else if (ptype == GVPM_PARENT_MEDIUM) {
    const float ph = phaseEval(b.parentG, b.parentWi, nd);
    thr = b.parentScat * ph;
    pdfValueSA = ph;
  } else {
    const float dp = fmaxf(dot(nd, b.parentN), 0.f);
    thr = mk3(INV_PI_F * dp);
    pdfValueSA = INV_PI_F * dp;
  }
  const float GOpNew = frcp(dist * dist);
  float sPdf = pdfValueSA * GOpNew;
  thr = thr * GOpNew;
  if (pr.pdfBasePos == 0.f) return 1.f;
  thr = thr * fdiv(b.parentRR, pr.pdfBasePos);
  if (GVPM_PF_EDGE_IN_MEDIUM(b.flags)) {
    const MRecF m = mediumEvalF(a.med, dist);
    sPdf *= m.pdfFailure;
    thr = thr * (m.tr == 0.f ? 0.f : pr.trOverKernelAndDist);
  }
  if (sPdf == 0.f && !pdfTiny) return 1.f;
  // BeamKernelRecord::kernelPDF of the new beam p1 -> newPos against the shifted ray (shift_volume_beams.h:300-336)
  float shiftKernelPDF = 0.f;
  if (technique == GVPM_BEAM_BEAM_1D) {
    const f3 c = cross(sr.d, nd);
    shiftKernelPDF = fsqrt(dot(c, c));
  } else {
    const f3 q = newPos + sr.D0;  // newPos from the shifted ray's foot point
    const float zq = dot(q, sr.d);
    const f3 D0n = q - sr.d * zq;
    const float z0 = (float)(-sr.s0) - zq, z1 = (float)((double)sr.maxt - sr.s0) - zq;
    float tN, tF;
    if (cylLocal(D0n, nd, sr.d, z0, z1, a.kernelRadius, -dist, INFINITY, tN, tF, &amb)) {
      const float radSqr = a.kernelRadius * a.kernelRadius, distSqr = dot(D0n, D0n);
      if (nearSq(distSqr, radSqr, distSqr + zq * zq)) amb = true;  // (|q|^2: q = D0n + d zq, D0n perpendicular to d)
      if (distSqr < radSqr)
        shiftKernelPDF = frcp(fmaxf(tF - tN, 0.0001f)) * frcp(fmaxf(2.f * fsqrt(fmaxf(0.f, radSqr - distSqr)), 0.0001f));
    }
  }
  if (shiftKernelPDF == 0.f) return 1.f;
  const f3 sigS = mk3(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]);
  const float ph = phaseEval(a.med.g, -nd, -sr.d) * pr.trW;
  shiftedFlux = b.prefixW * thr * sigS * shEye * ph;
  ok = true;
  float w = 0.5f;
  if (a.cfg.use_mis) {
    const float basePdf = pr.pdfBasePos * pr.pdfKernelAndDist;
    const float offsetPdf = shiftKernelPDF * sPdf;
    if ((offsetPdf == 0.f && !pdfTiny) || basePdf == 0.f) {
      ok = false;
      return 1.f;
    }
    const float x = sMIS * fdiv(offsetPdf, basePdf);
    w = a.cfg.power_heuristic ? frcp(1.f + x * x) : frcp(1.f + x);
  }
  return w;
}

// The shifted ray seen from the local origin, from the base ray's local form (cam) and the relative ray:
//   s0_s = s0_b + delta, delta = D0_b . relD + s0_b (d_b . relD) - relO . d_s
//   D0_s = D0_b - relO - relD s0_b - d_s delta
// every term is a product with a small factor, so fp32 holds them to ~1e-10; deriving them from the absolute
// positions took a dozen fp64 operations per shift.
__device__ __forceinline__ LocalRay shiftedLocal(const LocalRay &cam, const ShiftRel &sh, float eps, float &delta) {
  LocalRay sr;
  delta = dot(cam.D0, sh.rd) + cam.s0f * dot(cam.d, sh.rd) - dot(sh.ro, sh.d);
  sr.D0 = cam.D0 - sh.ro - sh.rd * cam.s0f - sh.d * delta;
  sr.s0 = cam.s0 + (double)delta;
  sr.d = sh.d;
  sr.s0f = (float)sr.s0;
  sr.mint = eps;
  sr.maxt = sh.len;
  return sr;
}

// One (camera ray, sub-beam) candidate in fp32 (beams_eval_f32.h): BeamGradRadianceQuery::operator(), in two phases
// like the G-BRE evaluation.  Phase 1 (a lane per pair): filters, kernel record, base contribution, then per offset
// pixel the null shift (shiftNull3D) or -- only PREPARED here -- the reconnection: its offset position goes into a
// wave-wide queue.  Phase 2 (a lane per queued reconnection, dense): shiftBeamDiffuse with its visibility test over
// the whole new beam.  Fused, every lane of a wave walked the reconnection of every shift some lane needed: 55 % of
// the shifts at C3, ~9100 lane-instructions per evaluation.
struct BeamP1 {
  BeamF b;
  LocalRay cam;
  KRecF k;
  d3 O;             // local origin: the sub-beam's centre
  f3 p1rel, kc, camW, baseContrib;
  double wD;
  float rr, tc;
  uint32_t edge, pix, st, id;
};
// a reconnection to do (phase 2): 28 bytes -- what phase 2 cannot rebuild from the beam's record and the ray tile.
// (Round 3 tried one entry per PAIR with a mask of its shifts, the pair's record and frame rebuilt once and the new beams of
// its shifts tested together against each listed triangle: 30.5 ms against 23.0 at C3 -- a pair has 1.8 reconnections on
// average, not 0 or 4, so the per-shift work ran at 46 % of the wave's width.)
struct BeamPQ {
  uint32_t id;    // beam | sub << 24
  uint32_t meta;  // ray | shift << 8
  float4 k;       // kRec.v - tc, kRec.w - (camera foot parameter), kRec.pdfEdgeFailure * kRec.pdfKernel, rr * weightKernel * sc
  float u;        // kRec.u (the 1D kernel's distance between the lines)
};

// filters + kernel record + base contribution; false: the pair produces nothing
template <int B, typename LDS>
__device__ __forceinline__ bool beamBase(const GatherArgs &a, LDS &s, uint32_t id, uint32_t bIdx, BeamP1 &o) {
  const uint32_t beamIdx = id & 0xFFFFFFu, sub = id >> 24;
  o.id = id;
  o.b = loadBeamF(a, beamIdx);
  const BeamF &b = o.b;
  const RayReg base = loadRay(s, 0, bIdx);
  o.edge = s.edge[bIdx];
  o.pix = s.pix[bIdx];
  const int px = (int)(o.pix & 0xFFFFu), py = (int)(o.pix >> 16);
  const int technique = a.cfg.vol_technique;
  const bool is1D = technique == GVPM_BEAM_BEAM_1D;
  // filters, shift_volume_beams.cpp:142-184
  const int pathLength = (int)o.edge + (int)GVPM_PF_DEPTH(b.flags);
  if (a.cfg.max_depth > 0 && pathLength > a.cfg.max_depth) return false;
  if (!((b.flags >> 6) & 1u)) return false;
  o.rr = 1.f;
  if (a.cfg.path_set) {
    if (((b.flags >> GVPM_HOT_PARITY_BIT) & 1u) != (uint32_t)((px + py) & 1)) return false;
    o.rr = 2.f;
  }
  const float r = a.kernelRadius, eps = a.cfg.epsilon;
  const uint32_t nSub = subBeamCount(b.len, a.subLen);
  const float ls = b.len / (float)nSub;
  const float tmin = ls * (float)sub;
  const float tmax = (sub + 1u >= nSub) ? b.len : fminf(ls * (float)(sub + 1u), b.len);
  const float tc = ls * ((float)sub + 0.5f);
  o.tc = tc;
  // local origin: the sub-beam's centre, kept in fp64 so that it lies on the beam's line
  const d3 p1D = tod(b.p1);
  o.O = p1D + (tod(b.p2) - p1D) * (double)(tc * frcp(b.len));
  LocalRay &cam = o.cam;
  {
    const d3 c = o.O - tod(base.o), dd = tod(base.d);
    cam.s0 = dot(c, dd);
    cam.D0 = tof(c - dd * cam.s0);
    cam.d = base.d;
    cam.s0f = (float)cam.s0;
    cam.mint = eps;
    cam.maxt = base.len - eps;
  }
  o.p1rel = b.bd * (-tc);
  const float bdd = dot(b.bd, base.d);
  const float sin2 = fmaxf(1.f - bdd * bdd, 0.f);
  uint32_t o0, o1;
  philox4x32_10(__float_as_uint(s.rnd[bIdx]), 0x6265616du, beamIdx, o0, o1);
  const float uv = (float)(o0 >> 8) * (1.0f / 16777216.0f);
  const float uw = (float)(o1 >> 8) * (1.0f / 16777216.0f);
  const f3 sigS = mk3(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]);

  KRecF &k = o.k;
  k.u = 0.f;
  const float band0 = 2e-6f * (r + ls) * frcp(fmaxf(sin2, 1e-12f));
  if (is1D) {
    // PhotonBeam::rayIntersectInternal1D (pm/beams_struct.h:250-311): closest approach of the two lines.  The
    // reference derives v and w from FLOAT dot products of absolute positions divided by d1.d2 and d1.d2^2 - 1: what
    // it accepts follows that rounding (~1e-6 / (sin^2 |d1.d2|) on v against sub-beams of ~1e-2), so the decision and
    // the four numbers come from the transcription; the cheap fp32 line-distance test in front of it only removes
    // pairs that miss by more than its own error.
    const f3 cr = cross(base.d, b.bd);
    const float ad = dot(cam.D0, cr);
    if (ad * ad >= r * r * sin2 * 1.001f + 1e-12f) return false;
    double vD, wD, pdfD, uD;
    if (!beamKernelExact(b.p1, b.p2, base.o, base.d, base.len, eps, r, sub, a.subLen, technique, uv, uw, vD, wD, pdfD, uD))
      return false;
    const float v = (float)vD, w = (float)wD;
    const float tau0 = (float)(vD - (double)tc);
    const float sig0 = (float)(wD - cam.s0);
    const float sinT = (float)pdfD;
    k.u = (float)uD;
    k.tauV = tau0;
    k.v = v;
    k.w = w;
    k.sigmaW = sig0;
    k.pdfKernel = sinT;
    const MRecF mCam = mediumEvalF(a.med, w), mB = mediumEvalF(a.med, v);
    k.weightKernel = 0.5f * frcp(r);
    k.pdfEdgeFailure = mB.pdfFailure;
    if (mB.pdfFailure == 0.f && mB.tr != 0.f) return false;
    const float sc = fdiv(mB.tr * mCam.tr * phaseEval(a.med.g, -b.bd, -base.d), mB.pdfFailure * k.pdfKernel);
    k.sc = sc;
    k.contrib = sigS * b.flux * sc;
  } else {
    // BeamKernelRecord::eval, shift_volume_beams.h:157-290, with cylinderIntersection (beams_3d_intersections.h:77-140)
    // in the local frame.  Every comparison that decides whether the pair is evaluated carries an error band (the
    // fp32 rounding of its operands, with a margin): `rej` collects the rejections that are sure, `amb` the comparisons
    // that fell inside their band -- those pairs (~1e-4) are decided, and their v / w / pdfKernel computed, by the
    // fp64 transcription (beamKernelExact), so the evaluated set is the reference's.
    const float z0 = (float)((double)cam.mint - cam.s0), z1 = (float)((double)cam.maxt - cam.s0);
    const float radSqr = r * r;
    bool amb = !(sin2 > 1e-6f), rej = false;
    // the view line is the beam (origin O, direction bd), the cylinder the camera ray: rel = O - foot = D0
    const float rzc = dot(cam.D0, base.d);
    const float Bh = dot(cam.D0, b.bd) - rzc * bdd;
    const float rel2 = dot(cam.D0, cam.D0);
    const float Cq = rel2 - rzc * rzc - radSqr;
    const float disc = Bh * Bh - sin2 * Cq;
    // rounding of the discriminant (a bound: ~8 ulps of its largest term); a pair within 32 of them of tangency goes to
    // the transcription, and for the others the root carries errDisc / (2 sqrt(disc)): near tangency the chord ends move
    // by much more than the operands' own rounding (measured with the audit build: 100 x the band that ignored it)
    const float errDisc = 6e-7f * (Bh * Bh + sin2 * (rel2 + radSqr));
    amb |= fabsf(disc) <= 32.f * errDisc;
    rej |= !(disc > 0.f);
    const float sq = fsqrt(fmaxf(disc, 0.f));
    const float tErr = fdiv(16.f * errDisc, fmaxf(sq * sin2, 1e-30f));
    const float bandT = 6.f * band0 + 3e-6f * (tc + ls + r) + tErr;       // beam parameters (absolute: tc + tau)
    const float bandZ = bandT + 2e-6f * r + 4e-7f * (fabsf(z0) + fabsf(z1));  // camera parameters from the foot point
    const float qq = Bh < 0.f ? (sq - Bh) : -(Bh + sq);
    float tN = fdiv(qq, fmaxf(sin2, 1e-12f)), tF = fdiv(Cq, qq);
    if (tN > tF) { const float t = tN; tN = tF; tF = t; }
    // tNear > view.maxt || tFar < 0 (the beam's own extent, absolute parameters tc + t)
    {
      const float tHi = b.len - tc, tLo = -tc;
      amb |= fabsf(tN - tHi) <= bandT || fabsf(tF - tLo) <= bandT;
      rej |= tN > tHi || tF < tLo;
    }
    // the caps of the camera ray's cylinder
    float bandTc = bandT;  // the band of tNear once it has been moved to a cap
    {
      const float zN = rzc + bdd * tN, zF = rzc + bdd * tF;
      amb |= fabsf(zN - z0) <= bandZ || fabsf(zN - z1) <= bandZ;
      const bool below = zN < z0, above = zN > z1;
      const float zc = below ? z0 : z1;
      if (below || above) {
        amb |= fabsf(zF - zc) <= bandZ;
        rej |= below ? zF < z0 : zF > z1;
        // the entry point through a cap divides by the beam's slope along the ray, zN - zF = (d_beam . d_ray)(tN - tF): the
        // error of the z's (the large ray parameters behind z0 / z1) comes back multiplied by chord / |zN - zF|
        const float dz = fabsf(zN - zF);
        bandTc += (tF - tN) * fdiv(2.f * bandZ, fmaxf(dz, 1e-30f));
        tN = tN + (tF - tN) * fdiv(zN - zc, zN - zF);
      }
    }
    // ownership: tmin < tNear < tmax, or the first sub-beam when the ray's cylinder contains the beam's origin
    {
      const float tNa = tc + tN;
      amb |= fabsf(tNa - tmin) <= bandTc || fabsf(tNa - tmax) <= bandTc || (sub == 0u && fabsf(tNa) <= bandTc);
      rej |= !((tNa < 0.f && tmin <= eps) || (tNa > tmin && tNa < tmax));
    }
    k.tauV = tN + (tF - tN) * uv;
    k.v = tc + k.tauV;
    k.pdfKernel = frcp(fmaxf(tF - tN, 0.0001f));
    amb |= fabsf(k.v) <= bandTc || fabsf(k.v - b.len) <= bandTc;
    rej |= k.v < 0.f || k.v > b.len;
    f3 perp = cam.D0 + (b.bd - base.d * bdd) * k.tauV;
    perp = perp - base.d * dot(perp, base.d);
    const float distSqr = dot(perp, perp);
    // the kernel centre moves with tauV's error at the beam's slope across the ray
    const float errD2 = 4e-6f * radSqr + 2.f * r * fsqrt(sin2) * bandTc;
    amb |= fabsf(distSqr - radSqr) <= 8.f * errD2;
    rej |= distSqr >= radSqr;
    const float deltaT = fsqrt(fmaxf(0.f, radSqr - distSqr));
    // distToProj = s0 + dot(D0, d) + tauV * (b.d): the kernel centre's parameter on the camera ray
    k.sigmaW = (rzc + k.tauV * bdd) - deltaT + 2.f * deltaT * uw;
    k.w = (float)(cam.s0 + (double)k.sigmaW);
    k.pdfKernel *= frcp(fmaxf(2.f * deltaT, 0.0001f));
    const float bandW = bandTc + fdiv(errD2, fmaxf(deltaT, 1e-30f)) + 2e-6f * r + 4e-7f * base.len;
    amb |= fabsf(k.w - cam.mint) <= bandW || fabsf(k.w - cam.maxt) <= bandW;
    rej |= k.w < cam.mint || k.w > cam.maxt;
#ifdef GVPM_BEAMS_AUDIT
    {
      double vD, wD, pdfD, uD, dbg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      const bool ex = beamKernelExact(b.p1, b.p2, base.o, base.d, base.len, eps, r, sub, a.subLen, technique, uv, uw, vD, wD,
                                      pdfD, uD, dbg);
      if (!amb && ex == rej) {
        const unsigned int slot = atomicAdd(&gvpmAuditCount, 1u);
        if (slot < 256u) {
          float *L = gvpmAuditLog[slot];
          L[0] = __uint_as_float(id); L[1] = __uint_as_float(o.pix); L[2] = ex ? 1.f : 0.f; L[3] = (float)dbg[0];
          L[4] = tc + tN; L[5] = (float)dbg[1]; L[6] = tc + tF; L[7] = (float)dbg[2]; L[8] = k.v; L[9] = (float)dbg[3];
          L[10] = distSqr / radSqr; L[11] = (float)(dbg[4] / ((double)r * r)); L[12] = k.w; L[13] = (float)dbg[5];
          L[14] = sin2; L[15] = bandT;
        }
      }
      if (!amb && !rej && ex) {
        atomicMax(&gvpmAuditRatio[0], __float_as_uint(fabsf((float)((double)tc + (double)tN - dbg[1])) / bandTc));
        atomicMax(&gvpmAuditRatio[1], __float_as_uint(fabsf((float)((double)k.v - vD)) / bandTc));
        atomicMax(&gvpmAuditRatio[5], __float_as_uint(fabsf((float)((double)tc + (double)tF - dbg[2])) / bandT));
        atomicMax(&gvpmAuditRatio[2], __float_as_uint(fabsf((float)((double)k.w - wD)) / bandW));
        atomicMax(&gvpmAuditRatio[3], __float_as_uint(fabsf((float)(((double)k.pdfKernel - pdfD) / pdfD))));
        atomicMax(&gvpmAuditRatio[4], __float_as_uint(fabsf((float)(((double)distSqr - dbg[4]) / ((double)errD2 * 8.0)))));
      }
    }
#endif
#ifdef GVPM_BEAMS_NOBAND
    amb = false;
#endif
    if (amb) {
      // (Measured at C3: this call, taken by 3 % of the blocks, costs the kernel ~1 ms of 20 whether it is taken or not; a
      // late pass over the undecided pairs -- the call outside this function, the block's code run a second time for
      // them as in the G-BRE evaluation -- cost 2.8 ms more than it saved.)
      double vD, wD, pdfD, uD;
      if (!beamKernelExact(b.p1, b.p2, base.o, base.d, base.len, eps, r, sub, a.subLen, technique, uv, uw, vD, wD, pdfD, uD))
        return false;
      k.v = (float)vD;
      k.tauV = (float)(vD - (double)tc);
      k.w = (float)wD;
      k.sigmaW = (float)(wD - cam.s0);
      k.pdfKernel = (float)pdfD;
    } else if (rej) {
      return false;
    }
    const MRecF mB = mediumEvalF(a.med, k.v), mCam = mediumEvalF(a.med, k.w);
    const float kernelVol = (4.0f / 3.0f) * 3.14159265358979323846f * r * r * r;
    const float sc = fdiv(mB.tr * mCam.tr * phaseEval(a.med.g, -b.bd, -base.d), k.pdfKernel * mB.pdfFailure);
    k.sc = sc;
    k.contrib = b.flux * sigS * sc;
    k.weightKernel = frcp(kernelVol);
    k.pdfEdgeFailure = mB.pdfFailure;
  }
  if (k.contrib.x == 0.f && k.contrib.y == 0.f && k.contrib.z == 0.f) return false;
  if (!(k.contrib.x == k.contrib.x)) return false;

  o.baseContrib = base.eye * k.contrib * k.weightKernel;
  atomicAdd(&s.acc[0][bIdx], (double)(o.baseContrib.x * o.rr));
  atomicAdd(&s.acc[1][bIdx], (double)(o.baseContrib.y * o.rr));
  atomicAdd(&s.acc[2][bIdx], (double)(o.baseContrib.z * o.rr));
  o.st = GVPM_PF_SHIFT_TYPE(b.flags);
  if (a.cfg.debug_shift != GVPM_SHIFT_ALL && a.cfg.debug_shift != GVPM_SHIFT_NULL) {
    const uint32_t st = o.st;
    const int cur = st == 1u ? GVPM_SHIFT_DIFFUSE : st == 2u ? GVPM_SHIFT_MEDIUM : st == 3u ? GVPM_SHIFT_MANIFOLD : GVPM_SHIFT_INVALID;
    if (a.cfg.debug_shift != cur) o.st = 0xFFu;  // base contribution kept, no shifts (shift_volume_beams.cpp:210-216)
  }
  o.wD = cam.s0 + (double)k.sigmaW;
  o.kc = b.bd * k.tauV;                 // kernel centre on the beam, local
  o.camW = atLocal(cam, k.sigmaW);      // camera ray at w, local
  return true;
}

// the border rule: no reverse shift at the right and top borders, shift_volume_beams.cpp (as the photon functors)
__device__ __forceinline__ bool beamBorder(const GatherArgs &a, uint32_t pix, int i) {
  const int px = (int)(pix & 0xFFFFu), py = (int)(pix >> 16);
  return (i == GVPM_RIGHT && px == a.cfg.width - 1) || (i == GVPM_TOP && py == a.cfg.height - 1);
}

// shift i of a pair that passed beamBase: the null shift is evaluated here; `rec`: the shift needs the offset-path
// reconnection, which phase 2 does (beamShift2)
// shift i of a pair that passed beamBase: the null shift is evaluated here; `rec`: the shift needs the offset-path
// reconnection, which phase 2 does (beamShift2).
// Round 5: every DECISION of the shift -- the shifted edge's length against w, the null-shift test, the shifted kernel's
// validity (cylLocal), the distance of the beam's origin to the shifted ray -- is taken in fp32 only outside a generous band
// of its operands' rounding; inside one the shift adds and counts nothing here and is noted for the exact pass
// (exact_beams_kernel: the fp64 transcription decides and adds it), as G-BRE's and G-VPM's are (shift_device.h, deferNote).
template <int B, bool HS, typename LDS>
__device__ __forceinline__ void beamShift1(const GatherArgs &a, LDS &s, const BeamP1 &o, uint32_t bIdx, int i, bool &rec,
                                           uint32_t &nNull, uint32_t &nFail, uint32_t setBase) {
  rec = false;
  if (o.st == 0xFFu) return;
  const BeamF &b = o.b;
  const KRecF &k = o.k;
  const LocalRay &cam = o.cam;
  const bool is1D = a.cfg.vol_technique == GVPM_BEAM_BEAM_1D;
  const float r = a.kernelRadius, eps = a.cfg.epsilon;
  const ShiftRel sh = loadShiftRel(s, i, bIdx, cam.d);
  float w = 1.f;
  f3 sflux = mk3(0.f);
  bool amb = a.cfg.reserved[4] != 0;  // (GVPM_EXACT_ALL: every shift through the exact pass, tests/test_exact_pass_gpu.py)
  uint32_t cause = 0u;                // which decision (GVPM_TRACE_EXACT prints the counts): 0 all, 1 w against the edge, 2 null test,
                                      // 3 shifted kernel, 4 its distance, 5 origin on the ray, 6 mirror, 7 flip, 8 visibility, 9 cosine / new kernel
  if (sh.valid && !amb) {
    const float shiftDistMAX = sh.len;
    const float L = beamLocalScale(a);
    float delta;
    const LocalRay sr = shiftedLocal(cam, sh, eps, delta);
    bool alreadyShift = false;
    // w against the shifted edge [Epsilon, shiftDistMAX]: absolute parameters, w = (float)(s0 + sigma) with sigma local
    amb = fabsf(k.w - shiftDistMAX) <= 1e-6f * (k.w + shiftDistMAX) + 1e-5f * L || k.w - eps <= 1e-6f * eps + 1e-5f * L;
    if (amb) cause = 1u;
    if (a.cfg.use_shift_null && !is1D && !amb) {
      const float sigS_w = k.sigmaW - delta;  // the same distance w on the shifted ray, from its foot point
      const f3 dz = atLocal(sr, sigS_w) - o.kc;
      const float dz2 = dot(dz, dz);
      amb = nearSq(dz2, r * r, sigS_w * sigS_w + dot(sr.D0, sr.D0) + k.tauV * k.tauV);
      if (amb) cause = 2u;
      if (!amb && dz2 < r * r && k.w <= shiftDistMAX) {
        // BeamKernelRecord copy-shift constructor (shift_volume_beams.h:40-144) + shiftNull3D (.cpp:748-786)
        float tN, tF;
        const float z0 = (float)((double)eps - sr.s0), z1 = (float)((double)shiftDistMAX - sr.s0);
        const bool cylOk = cylLocal(sr.D0, b.bd, sr.d, z0, z1, r, -o.tc, b.len - o.tc, tN, tF, &amb);
        if (amb) cause = 3u;
        if (cylOk && !amb) {
          float pdfK = frcp(fmaxf(tF - tN, 0.0001f));
          const float bds = dot(b.bd, sr.d);
          f3 perp = sr.D0 + (b.bd - sr.d * bds) * k.tauV;
          perp = perp - sr.d * dot(perp, sr.d);
          const float distSqr = dot(perp, perp), radSqr = r * r;
          amb = nearSq(distSqr, radSqr, dot(sr.D0, sr.D0) + k.tauV * k.tauV);
          if (amb) cause = 4u;
          if (!amb && distSqr < radSqr && !(k.w < sr.mint || k.w > sr.maxt)) {
            pdfK *= frcp(fmaxf(2.f * fsqrt(fmaxf(0.f, radSqr - distSqr)), 0.0001f));
            nNull++;
            sflux = k.contrib * sh.eye;  // kS.contrib * kpdf(kS) / kpdf(kRec): the pdf ratios cancel
            w = 0.5f;
            if (a.cfg.use_mis) {
              const float x = sh.sMIS * fdiv(pdfK, k.pdfKernel);
              w = a.cfg.power_heuristic ? frcp(1.f + x * x) : frcp(1.f + x);
            }
            alreadyShift = true;
          }
        }
      }
    }
    if (!amb && !alreadyShift && k.w <= shiftDistMAX) {
      // shiftBeam dispatch, shift_volume_beams.cpp:355-408.  (The reference first asks whether the beam's origin lies ON
      // the shifted ray, `minDistSqr > kRec.u^2` -- no shift then, weight 1: phase 2 asks for the shifts it is given;
      // for a light path that cannot be reconnected the question is asked here)
      if (a.cfg.debug_shift == GVPM_SHIFT_NULL || k.w > sr.maxt) {
        w = 1.f;
      } else if (o.st == 1u || o.st == 2u || (HS && o.st == 3u)) {
        // shiftBeamDiffuse: phase 2, which also adds the weighted base term of this shift (HS: a manifold-typed beam goes
        // there too -- it records the host's request, gvpm_enable_host_shifts)
        rec = true;
        return;
      } else {
        bool doShift = true;
        if (!is1D) {
          f3 pv = o.p1rel + sr.D0;
          pv = pv - sr.d * dot(pv, sr.d);
          const float pv2 = dot(pv, pv), u2 = k.u * k.u, e = 3e-5f * (o.tc + L);
          amb = fabsf(pv2 - u2) <= e * (2.f * fsqrt(fmaxf(pv2, u2)) + e);
          if (amb) cause = 5u;
          doShift = pv2 > u2;
        }
        if (doShift && !amb) nFail++;
      }
    }
  }
  if (amb) {
    deferNote(a, GVPM_EX_KIND_BEAMS, a.setPerm[setBase + bIdx], o.id, (uint32_t)i, cause);
    return;
  }
  if (beamBorder(a, o.pix, i)) w = 1.f;
  const float ws = w * o.rr;
  if (sflux.x != 0.f || sflux.y != 0.f || sflux.z != 0.f) {
    const float wk = ws * k.weightKernel;
    atomicAdd(&s.acc[3 + 3 * i + 0][bIdx], (double)(sflux.x * wk));
    atomicAdd(&s.acc[3 + 3 * i + 1][bIdx], (double)(sflux.y * wk));
    atomicAdd(&s.acc[3 + 3 * i + 2][bIdx], (double)(sflux.z * wk));
  }
  atomicAdd(&s.acc[15 + 3 * i + 0][bIdx], (double)(o.baseContrib.x * ws));
  atomicAdd(&s.acc[15 + 3 * i + 1][bIdx], (double)(o.baseContrib.y * ws));
  atomicAdd(&s.acc[15 + 3 * i + 2][bIdx], (double)(o.baseContrib.z * ws));
}

// phase 2: one reconnection (shiftBeamDiffuse) -> the shifted and the weighted sums of its (ray, shift).  The offset
// position (getShiftPos / getShiftPos1D) is computed HERE, where every lane has one to compute: in phase 1 the lanes
// with a null shift waited for the lanes that prepared a reconnection.
// withVis (wave-uniform) = false: the first round -- a reconnection whose new beam is not inside its beam's free cone
// (beamClear: inside, nothing can occlude it) is DEFERRED, untouched; true: the second round over the deferred ones,
// through the any-hit loop.
// Round 5: its decisions -- the origin's distance to the shifted ray, the mirror test of getShiftPos, the flip of
// getShiftPos1D, the triangle tests of the new beam's shadow segment (three states), the cosines' signs, the new kernel's
// validity -- are banded like phase 1's; inside a band the shift is noted for the exact pass and nothing is added or counted.
template <int B, bool HS, typename LDS>
__device__ __forceinline__ void beamShift2(const GatherArgs &a, LDS &s, const BeamPQ &q, const float4 *ldsTri, bool withVis,
                                           bool &defer, uint32_t &nDiff, uint32_t &nFail, uint32_t setBase) {
  defer = false;
  const uint32_t beamIdx = q.id & 0xFFFFFFu, sub = q.id >> 24;
  const uint32_t bIdx = q.meta & 0xFFu;
  const int i = (int)((q.meta >> 8) & 3u);
  const int technique = a.cfg.vol_technique;
  const bool is1D = technique == GVPM_BEAM_BEAM_1D;
  const float r = a.kernelRadius, eps = a.cfg.epsilon;
  const BeamF b = loadBeamF(a, beamIdx);
  const RayReg base = loadRay(s, 0, bIdx);
  const uint32_t nSub = subBeamCount(b.len, a.subLen);
  const float ls = b.len / (float)nSub;
  const float tc = ls * ((float)sub + 0.5f);
  const d3 p1D = tod(b.p1);
  const d3 O = p1D + (tod(b.p2) - p1D) * (double)(tc * frcp(b.len));  // (the expression of beamBase: same origin)
  LocalRay cam;
  {
    const d3 c = O - tod(base.o), dd = tod(base.d);
    cam.s0 = dot(c, dd);
    cam.D0 = tof(c - dd * cam.s0);
    cam.d = base.d;
    cam.s0f = (float)cam.s0;
    cam.mint = eps;
    cam.maxt = base.len - eps;
  }
  const float tauV = q.k.x, sigmaW = q.k.y;
  const float kV = tc + tauV, kW = (float)(cam.s0 + (double)sigmaW);
  const f3 p1rel = b.bd * (-tc);
  const ShiftRel sh = loadShiftRel(s, i, bIdx, cam.d);
  float delta;
  const LocalRay sr = shiftedLocal(cam, sh, eps, delta);
  const float sigS_w = sigmaW - delta;  // the same distance w on the shifted ray, from its foot point
  const f3 shW = atLocal(sr, sigS_w);
  bool doShift = true;
  bool amb = false;
  uint32_t cause = 0u;
  const float L = beamLocalScale(a);
  f3 offsetPos;
  if (!is1D) {
    // distance of the beam's origin to the shifted ray against kRec.u (= 0 for the 3D kernel)
    f3 pv = p1rel + sr.D0;
    pv = pv - sr.d * dot(pv, sr.d);
    const float pv2 = dot(pv, pv), u2 = q.u * q.u, e = 3e-5f * (tc + L);
    amb = fabsf(pv2 - u2) <= e * (2.f * fsqrt(fmaxf(pv2, u2)) + e);
    if (amb) cause = 5u;
    doShift = pv2 > u2;  // else result.weight = 1
    // getShiftPos (3D), shift_volume_beams.cpp:93-137: the kernel offset in the base ray's coherent frame, replayed in
    // the shifted ray's
    const f3 kc = b.bd * tauV;             // kernel centre on the beam, local
    const f3 camW = atLocal(cam, sigmaW);  // camera ray at w, local
    const f3 u = kc - camW;
    f3 bs, bt, ns, nt;
    coordSysCoherentF(cam.d, bs, bt);
    coordSysCoherentF(sr.d, ns, nt);
    const float lx = dot(u, bs), ly = dot(u, bt), lz = dot(u, cam.d);
    offsetPos = shW + (ns * lx + nt * ly + sr.d * lz);
    if (a.cfg.use_shift_null) {
      const f3 dv = camW - offsetPos;
      if (nearSq(dot(dv, dv), r * r, dot(camW, camW) + dot(shW, shW) + dot(u, u))) { amb = true; cause = 6u; }  // (the mirror decision moves the offset position by up to 2 r)
      if (dot(dv, dv) < r * r) {
        f3 dShift = shW - camW;
        dShift = dShift * frsq(dot(dShift, dShift));
        const float cosD = dot(dShift, shW - offsetPos);
        offsetPos = offsetPos + dShift * (cosD * 2.0f);
      }
    }
  } else {
    // getShiftPos1D, shift_volume_beams.cpp:81-91
    const f3 aCam = p1rel + cam.D0;  // p1 from the base ray's foot point
    f3 back = shiftPointLocal(cam.d, aCam, q.u, sigmaW, false) - aCam;
    const float ib = frsq(dot(back, back));
    back = back * ib;
    const f3 df = back - b.bd;
    // (`back` spans the beam from p1 to the kernel: good to ~2.4e-7 (tc + L), its direction to that over its length -- and df2
    // genuinely ranges over [0, (2 r / v)^2], which straddles the reference's 0.001: a band of 1e-5 deferred 0.2 % of the 1D
    // kernel's reconnections, this one 1e-4 of them)
    // (and shift()'s sine, sqrt(1 - (u / ly)^2), loses everything where the point's distance ly to the ray comes down to u --
    // the kernel at the beam's very origin: |back| ~ 1e-4 with a direction that is noise, found by tests/stress_beams.py on
    // S-cbox rotated -- : shiftSinErr is that error, on the base side part of the band, on the shifted side a reason to defer
    // once it exceeds what the decisions behind it allow for)
    const float dly = 4e-6f * (tc + L);
    const float df2 = dot(df, df), eb = (dly + q.u * shiftSinErr(cam.d, aCam, q.u, dly)) * ib;
    if (!(fabsf(df2 - 0.001f) > eb * (2.f * fsqrt(fmaxf(df2, 0.001f)) + eb) + 1e-7f)) { amb = true; cause = 7u; }
    const bool flip = df2 > 0.001f;
    offsetPos = shiftPointLocal(sr.d, p1rel + sr.D0, q.u, sigS_w, flip) - sr.D0;
    if (!(q.u * shiftSinErr(sr.d, p1rel + sr.D0, q.u, dly) <= 4.f * dly)) { amb = true; cause = 7u; }
#ifdef GVPM_DBG_SHIFT2
    {
      const f3 aS = p1rel + sr.D0, avS = aS - sr.d * dot(aS, sr.d), avC = aCam - cam.d * dot(aCam, cam.d);
      printf("1D i %d df2 %.9g eb %g flip %d u %.9g lyCam %.9g lySh %.9g |back|^-1 %g tc %g L %g\n", i, df2, eb, (int)flip, q.u, sqrtf(dot(avC, avC)),
             sqrtf(dot(avS, avS)), ib, tc, L);
    }
#endif
  }
  float w = 1.f;
  f3 sflux = mk3(0.f);
  // (a manifold-typed beam under gvpm_enable_host_shifts keeps the plain fp32 decisions: its walk is the host's)
  const bool hostShift = HS && GVPM_PF_SHIFT_TYPE(b.flags) == 3u;
  if (amb && !hostShift) {
    deferNote(a, GVPM_EX_KIND_BEAMS, a.setPerm[setBase + bIdx], q.id, (uint32_t)i, cause);
    return;
  }
  if (HS && doShift && GVPM_PF_SHIFT_TYPE(b.flags) == 3u) {
    // EManifoldShift -> shiftBeamME (shift_volume_beams.cpp:398-404,601-746): the walk is the host's.  Absolute positions:
    // the local frame's origin O plus the local vectors; the rays at (w - mint), as generateShiftPathME is handed them.
    const f3 Of = tof(O);
    const f3 sigSv = mk3(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]);
    const f3 bcvR = base.eye * b.flux * sigSv * q.k.w;
    const float wkrrR = (a.cfg.path_set ? 2.f : 1.f) *
                        (is1D ? 0.5f * frcp(r) : frcp((4.0f / 3.0f) * 3.14159265358979323846f * r * r * r));
    const f3 shO = base.o + sh.ro;
    if (recordBeamShiftRequest(reqSink(a), beamIdx, a.setPerm[setBase + bIdx], i, Of + offsetPos, base.o + base.d * (kW - eps),
                               shO + sh.d * (kW - eps), kW, kV, q.k.z, r, shO, sh.len, sh.d, bcvR, wkrrR, sh.eye, sh.sMIS, s.pix[bIdx]))
      return;  // (nothing is added now: the answer's terms and the weighted base term come with gvpm_upload_host_shifts)
    nFail++;   // the list is full: a failed shift, weight 1
    doShift = false;
  }
  if (doShift) {
    f3 nd = offsetPos - p1rel;
    const float dist = fsqrt(dot(nd, nd));
    nd = nd * frcp(dist);
    bool ok = false;
    if (!withVis) {
      const float2 cl = a.beamClear[beamIdx];
      if (!(dot(nd, b.bd) > cl.x && dist < cl.y)) {
        defer = true;
        return;
      }
    }
    const int vis = withVis ? beamShadowBlocked(a, b, ldsTri, nd, dist) : GVPM_TRI_MISS;
    if (vis & GVPM_TRI_AMB) { amb = true; cause = 8u; }
    if (vis == GVPM_TRI_MISS) {
      BeamRecPair pr;
      pr.pdfBasePos = b.parentPdf * (b.len * b.len);
      if (b.endOnSurface) pr.pdfBasePos = fdiv(pr.pdfBasePos, fabsf(dot(b.endN, b.bd)));
      pr.pdfBasePos *= frcp(kV * kV);
      // Under a thick medium the reconnection's flux is exp(sigma_t (v - dist)) times the base term's scale -- 10^3 at
      // sigma_t (v - dist) = 7 -- and every rounding of a LENGTH costs sigma_t ulp(length) of it: 1e-6 each for dist, v and w
      // at sigma_t = 64, one such shift 1e-2 of a frame's mean luminance (tests/test_medium_space_gpu.py, `opaque`).  So
      // (a) w's optical depth is formed in double from the foot parameter and rounded once, with its remainder;
      // (b) where pdfFailure is the bare exponential (msw = 1), tr(dist) / pdfFailure(v) = exp(-sigma_t (dist - v)) with
      //     dist - v = (dist^2 - v^2) / (dist + v) and dist^2 - v^2 = 2 tc (bd.offsetPos - tauV) + |offsetPos|^2 - tauV^2 from
      //     LOCAL operands (nd = offsetPos + bd tc, v = tc + tauV: tc^2 cancels), good to ~1e-9; pdfKernel is taken back
      //     out of the queue's product with the same pdfFailure(v) phase 1 multiplied it by.  With msw < 1 pdfFailure is
      //     bounded below by 1 - msw, nothing is amplified, and the quotient stays as it was.
      const float sigT = a.med.sigmaT[0];
      {
        const double xw = -(double)sigT * (cam.s0 + (double)sigmaW);
        const float xh = (float)xw;
        const float eW = expSplit(xh, (float)(xw - (double)xh));
        pr.trW = eW < 1e-20f ? 0.f : eW;
      }
      pr.pdfKernelAndDist = q.k.z;
      if (a.med.msw == 1.f) {
        const MRecF mV = mediumEvalF(a.med, kV);
        const float d2 = 2.f * tc * (dot(b.bd, offsetPos) - tauV) + (dot(offsetPos, offsetPos) - tauV * tauV);
        pr.trOverKernelAndDist = expSplit(-sigT * fdiv(d2, dist + kV), 0.f) * fdiv(mV.pdfFailure, q.k.z);
      } else {
        pr.trOverKernelAndDist = fdiv(mediumEvalF(a.med, dist).tr, q.k.z);
      }
      w = reconnectBeamF(a, b, pr, sh.eye, sh.sMIS, sr, offsetPos, nd, dist, technique, sflux, ok, amb);
    }
#ifdef GVPM_DBG_SHIFT2  // (probe builds: scripts/probes_py/beams_bisect.py narrows a counter mismatch down to one pair first)
    printf("shift2 i %d withVis %d vis %d amb %d ok %d w %g dist %g nd %g %g %g cosWo %g cosWi %g clear %g %g flip-u %g\n", i, (int)withVis, vis,
           (int)amb, (int)ok, w, dist, nd.x, nd.y, nd.z, dot(b.parentN, nd), dot(b.parentN, b.parentWi), a.beamClear[beamIdx].x,
           a.beamClear[beamIdx].y, q.u);
#endif
    if (amb) {
      deferNote(a, GVPM_EX_KIND_BEAMS, a.setPerm[setBase + bIdx], q.id, (uint32_t)i, cause ? cause : 9u);
      return;
    }
    if (ok) nDiff++; else nFail++;
  }
  if (beamBorder(a, s.pix[bIdx], i)) w = 1.f;
  const f3 sigS = mk3(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]);
  const f3 bcv = base.eye * b.flux * sigS * q.k.w;
  // rr * weightKernel: the same for every pair of a launch (shift_volume_beams.h: 0.5 / r, or 1 / (4/3 pi r^3))
  const float wkrr = (a.cfg.path_set ? 2.f : 1.f) *
                     (is1D ? 0.5f * frcp(r) : frcp((4.0f / 3.0f) * 3.14159265358979323846f * r * r * r));
  if (sflux.x != 0.f || sflux.y != 0.f || sflux.z != 0.f) {
    atomicAdd(&s.acc[3 + 3 * i + 0][bIdx], (double)(sflux.x * (w * wkrr)));
    atomicAdd(&s.acc[3 + 3 * i + 1][bIdx], (double)(sflux.y * (w * wkrr)));
    atomicAdd(&s.acc[3 + 3 * i + 2][bIdx], (double)(sflux.z * (w * wkrr)));
  }
  atomicAdd(&s.acc[15 + 3 * i + 0][bIdx], (double)(bcv.x * w));
  atomicAdd(&s.acc[15 + 3 * i + 1][bIdx], (double)(bcv.y * w));
  atomicAdd(&s.acc[15 + 3 * i + 2][bIdx], (double)(bcv.z * w));
}

// ---- the evaluation's LDS budget (the fused kernel's tile; the split pair sizes its occluder stage by the same figure) ----
constexpr int BPOOL = 384;
// LDS is what bounds this kernel's residency (253 VGPRs allow 8 waves per CU, 20480 bytes each): the shifted rays of the tile
// are kept RELATIVE to their base ray in the ray tile's own slots (relToBase), the queue entries are 28 bytes (36 until round
// 3, when they carried the offset position phase 2 now computes itself).
template <int B> struct BeamEvalLds : RayTile<B> {
  double acc[27][B];
  uint32_t qid[BPOOL], qmeta[BPOOL];  // beam | sub << 24; ray | shift << 8
  float4 qk[BPOOL];                   // BeamPQ::k
  float qu[BPOOL];                    // BeamPQ::u
};
// occluders in LDS only while they leave the eighth wave its room: measured at C3 (22 occluders) with the two rings, 7 waves
// with the triangles in LDS 20.4 ms, 8 waves reading the near lists' triangles from global memory 18.3 ms
#ifdef GVPM_BEAM_LDS_TRIS  // (probe builds)
constexpr uint32_t BEAM_LDS_TRIS = GVPM_BEAM_LDS_TRIS;
#else
constexpr uint32_t BEAM_LDS_TRIS = (20480u - (uint32_t)sizeof(BeamEvalLds<16>)) / 48u;
#endif
static_assert(BEAM_LDS_TRIS <= SCENE_LDS_TRIS && sizeof(BeamEvalLds<16>) + 32u * 48u <= 20480u, "the beam evaluation's LDS budget");

}  // namespace gvpm
