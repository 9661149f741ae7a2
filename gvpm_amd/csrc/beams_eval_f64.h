// The literal fp64 transcription of the reference's beam x beam estimator, with its float intermediates: one
// (camera ray, sub-beam) candidate at a time (evaluateBeam).  The counterpart of beams_eval_f32.h / beams_shift_f32.h.
//
// Transcribes
//   BeamGradRadianceQuery::operator()             gvpm/shift/shift_volume_beams.cpp:139-353
//   BeamKernelRecord (1D, 3D "optimized")         gvpm/shift/shift_volume_beams.h:24-338
//   PhotonBeam::rayIntersectInternal1D/getContrib pm/beams_struct.h:250-311,136-185
//   cylinderIntersection                          pm/beams_3d_intersections.h:77-140
//   getShiftPos / getShiftPos1D / shift           shift_volume_beams.cpp:37-137
//   shiftBeam / shiftBeamDiffuse / shiftNull3D    shift_volume_beams.cpp:355-539,748-786
//   diffuseReconnectionPhotonBeam                 gvpm/shift/operation/shift_diffuse.cpp:136-268
// (pm/ = src/integrators/photonmapper/).
//
// It is kept as the on-device cross-check (GVPM_BEAMS_FP64=1, evaluate_beams_exact_kernel), settles the ownership decisions
// that fall inside the fp32 error band (beamKernelExact, beams_shift_f32.h) and -- round 5 -- is what exact_beams_kernel
// evaluates, one at a time, the shifts with whose own decisions fp32 cannot be trusted (beamShift1 / beamShift2 note them).
// Both kernels are in gather_beams.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "beams_common.h"
#include "device_types.h"
#include "dmath.h"
#include "shift_device.h"
#include "tile_walk.h"
#include "vec.h"

namespace gvpm {

struct BeamD {
  d3 p1, p2, dir;
  double len;
  d3 flux, prefixW, parentScat;
  d3 parentN, parentWi, endN;
  double parentPdf, parentRR, parentG;
  uint32_t flags;
  bool endOnSurface;
};

__device__ __forceinline__ void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t &o0, uint32_t &o1) {
  uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o0 = c0;
  o1 = c1;
}

// coordinateSystem, src/libcore/util.cpp:600-609
__device__ __forceinline__ void coordSys(d3 a, d3 &b, d3 &c) {
  if (fabs(a.x) > fabs(a.y)) {
    const double invLen = 1.0 / sqrt(a.x * a.x + a.z * a.z);
    c = mkd(a.z * invLen, 0.0, -a.x * invLen);
  } else {
    const double invLen = 1.0 / sqrt(a.y * a.y + a.z * a.z);
    c = mkd(0.0, a.z * invLen, -a.y * invLen);
  }
  b = crossd(c, a);
}
// coordinateSystemCoherent (float intermediates), util.cpp:592-599
__device__ __forceinline__ void coordSysCoherent(d3 n, d3 &b1, d3 &b2) {
  const float sign = copysignf(1.0f, (float)n.z);
  const float aa = (float)(-1.0f / ((double)sign + n.z));
  const float bb = (float)(n.x * n.y * (double)aa);
  b1 = mkd(1.0 + (double)sign * n.x * n.x * (double)aa, (double)sign * (double)bb, -(double)sign * n.x);
  b2 = mkd((double)bb, (double)sign + n.y * n.y * (double)aa, -n.y);
}

__device__ __forceinline__ bool solveQuadraticD(double a, double b, double c, double &x0, double &x1) {
  if (a == 0) {
    if (b != 0) {
      x0 = x1 = -c / b;
      return true;
    }
    return false;
  }
  const double discrim = b * b - 4.0 * a * c;
  if (discrim < 0) return false;
  const double sq = sqrt(discrim);
  const double temp = b < 0 ? -0.5 * (b - sq) : -0.5 * (b + sq);
  x0 = temp / a;
  x1 = c / temp;
  if (x0 > x1) { const double t = x0; x0 = x1; x1 = t; }
  return true;
}

// cylinderIntersection(rCylinder, view, radius), pm/beams_3d_intersections.h:77-140
__device__ __forceinline__ bool cylinderIntersection(const RayD &cyl, const RayD &view, double radius, double &tNear,
                                                     double &tFar) {
  const d3 d1d2c = crossd(view.d, cyl.d);
  const float sinThetaSqr = (float)dot(d1d2c, d1d2c);
  const float ad = (float)dot(cyl.o - view.o, d1d2c);
  if ((double)(ad * ad) >= (radius * radius) * (double)sinThetaSqr) return false;
  d3 s, t;
  coordSys(cyl.d, s, t);
  const double lMax = cyl.maxt;
  const d3 rel = view.o - cyl.o;
  const double ox = dot(s, rel), oy = dot(t, rel), oz = dot(cyl.d, rel);
  const double dx = dot(s, view.d), dy = dot(t, view.d), dz = dot(cyl.d, view.d);
  const double A = dx * dx + dy * dy;
  const double Bq = 2 * (dx * ox + dy * oy);
  const double C = ox * ox + oy * oy - radius * radius;
  if (!solveQuadraticD(A, Bq, C, tNear, tFar)) return false;
  if (tNear > view.maxt || tFar < 0) return false;
  const double zPosNear = oz + dz * tNear, zPosFar = oz + dz * tFar;
  if (zPosNear < 0) {
    if (zPosFar < 0) return false;
    tNear = (double)(float)(tNear + (tFar - tNear) * (zPosNear) / (zPosNear - zPosFar));
    return true;
  } else if (zPosNear >= 0 && zPosNear < lMax) {
    return true;
  } else if (zPosNear > lMax) {
    if (zPosFar > lMax) return false;
    tNear = (double)(float)(tNear + (tFar - tNear) * (zPosNear - lMax) / (zPosNear - zPosFar));
    return true;
  }
  return false;
}

struct KRecD {
  double radius, v, w, pdfKernel, pdfEdgeFailure, u, weightKernel, beamTrans;
  d3 contrib;
  bool valid;
};
__device__ __forceinline__ double kpdf(const KRecD &k) { return k.pdfEdgeFailure * k.pdfKernel; }

// PhotonBeam::rayIntersectInternal1D, pm/beams_struct.h:250-311 (float intermediates as written)
// UNCONTRACTED (round 5): the statement rounds its double dot products to float and divides by d1.d2 -- a last-bit difference of a
// double (an FMA where the oracle's compiler has a multiply and an add) moves a float rounding, and 1 / d1.d2 makes that a
// different v: tests/stress_beams.py found a pair accepted here at v = 2e-5 that the oracle rejects.
__device__ __forceinline__ double dotU(d3 a, d3 b) {
#pragma clang fp contract(off)
  return a.x * b.x + a.y * b.y + a.z * b.z;
}
__device__ __forceinline__ d3 crossU(d3 a, d3 b) {
#pragma clang fp contract(off)
  return d3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ bool rayIntersect1D(const BeamD &b, double radius, const RayD &ray, double tminBeam,
                                               double tmaxBeam, double &u, double &v, double &w, double &sinTheta) {
#pragma clang fp contract(off)
  const d3 d1d2c = crossU(ray.d, b.dir);
  const float sinThetaSqr = (float)dotU(d1d2c, d1d2c);
  const float ad = (float)dotU(b.p1 - ray.o, d1d2c);
  if ((double)(ad * ad) >= (radius * radius) * (double)sinThetaSqr) return false;
  const float d1d2 = (float)dotU(ray.d, b.dir);
  const float d1d2Sqr = d1d2 * d1d2;
  const float d1d2SqrMinus1 = d1d2Sqr - 1.0f;
  if (d1d2SqrMinus1 < 1e-5f && d1d2SqrMinus1 > -1e-5f) return false;
  const float d1O1 = (float)dotU(ray.d, ray.o);
  const float d1O2 = (float)dotU(ray.d, b.p1);
  w = ((double)(d1O1 - d1O2) - (double)d1d2 * (dotU(b.dir, ray.o) - dotU(b.dir, b.p1))) / (double)d1d2SqrMinus1;
  if (w <= ray.mint || w >= ray.maxt) return false;
  v = (w + (double)d1O1 - (double)d1O2) / (double)d1d2;
  if (v <= 0.0 || v >= b.len || isnan(v)) return false;
  if (tminBeam >= v || tmaxBeam < v) return false;
  // (the reference's FLOAT sqrt and division, correctly rounded -- through double, whose 53 bits make the second rounding
  // innocuous: this library is built with -fno-hip-fp32-correctly-rounded-divide-sqrt, and a u one ulp off the oracle's moved
  // sqrt(1 - (u / ly)^2) by 8 % on a pair whose kernel sits at the beam's origin: tests/stress_beams.py, STRESS_IT=5)
  const float sinThetaConst = (float)sqrt((double)sinThetaSqr);
  u = (double)(float)((double)fabsf(ad) / (double)sinThetaConst);
  sinTheta = (double)sinThetaConst;
  return true;
}

// 1D kernel: WHICH sub-beam evaluates a (camera ray, beam) pair the reference's test accepts.  The reference asks
// every sub-beam whose box the ray meets for `tmin < v <= tmax` with ITS v -- float dot products of absolute positions
// divided by d1.d2 (beams_struct.h:275-290): for near-perpendicular lines (|d1.d2| < 1e-4: 3e-4 of C3's pairs, whose
// camera rays are horizontal and beams vertical) that v is off by whole sub-beams, up to anything, and lands in a
// sub-beam far from where the lines meet -- which the reference evaluates or not depending on whether its BVH happens to
// visit that box.  The accel-independent statement (the reference's own ENoAccel loop, pm/beams.h:289-294, and the
// oracle's): the pair is evaluated iff the test over the WHOLE beam accepts it, with the reference's v and w.  Here the
// sub-beam that contains the GEOMETRIC closest approach (well conditioned, fp64, the same for every sub-beam that asks)
// speaks for the beam; it is always among the traversal's candidates when the lines pass within the radius.
__device__ __forceinline__ bool beamOwner1D(const BeamD &b, const RayD &cam, uint32_t sub, uint32_t nSub, double tmin,
                                            double tmax) {
  const d3 op = cam.o - b.p1;
  const double c12 = dot(cam.d, b.dir);
  const double vg = (dot(op, b.dir) - c12 * dot(op, cam.d)) / (1.0 - c12 * c12);
  return (sub == 0u || vg > tmin) && (sub + 1u >= nSub || vg <= tmax);
}

// BeamKernelRecord::eval, shift_volume_beams.h:157-290 (short beams)
__device__ __forceinline__ void krecEval(const GatherArgs &a, const BeamD &b, const RayD &cam, double tmin, double tmax,
                                         double uv, double uw, int technique, KRecD &k) {
  const d3 sigS = mkd(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]);
  k.valid = false;
  if (tmax > b.len) tmax = b.len;
  if (technique == GVPM_BEAM_BEAM_1D) {
    if (!rayIntersect1D(b, k.radius, cam, tmin, tmax, k.u, k.v, k.w, k.pdfKernel)) return;
    const MRecD mCam = mediumEvalD(a.med, k.w);
    k.weightKernel = 0.5 / k.radius;
    const MRecD mB = mediumEvalD(a.med, k.v);
    k.beamTrans = mB.tr;
    k.pdfEdgeFailure = mB.pdfFailure;
    if (mB.pdfFailure == 0.0 && mB.tr != 0.0) return;
    const double ph = phaseD((double)a.med.g, -b.dir, -cam.d);
    const double sc = mB.tr * mCam.tr * ph / mB.pdfFailure / k.pdfKernel;
    k.contrib = mkd(sigS.x * b.flux.x * sc, sigS.y * b.flux.y * sc, sigS.z * b.flux.z * sc);
  } else {
    const RayD _cam{at(cam, cam.mint), cam.d, 0.0, cam.maxt - cam.mint};
    const RayD _beam{b.p1, b.dir, 0.0, b.len};
    double tN, tF;
    if (!cylinderIntersection(_cam, _beam, k.radius, tN, tF)) return;
    if (tN < 0 && tmin <= (double)a.cfg.epsilon) {
    } else if (tN > tmin && tN < tmax) {
    } else {
      return;
    }
    k.v = tN + (tF - tN) * uv;
    k.pdfKernel = 1.0 / fmax(tF - tN, 0.0001);
    if (k.v < 0 || k.v > b.len) return;
    const d3 kc = b.p1 + b.dir * k.v;
    const double distToProj = dot(kc - cam.o, cam.d);
    const double distSqr = len2(at(cam, distToProj) - kc);
    const double radSqr = k.radius * k.radius;
    if (distSqr >= radSqr) return;
    const double deltaT = sqrt(fmax(0.0, radSqr - distSqr));
    k.w = distToProj - deltaT + 2 * deltaT * uw;
    k.pdfKernel *= 1.0 / fmax(2.0 * deltaT, 0.0001);
    if (k.w < cam.mint || k.w > cam.maxt) return;
    const MRecD mB = mediumEvalD(a.med, k.v);
    const MRecD mCam = mediumEvalD(a.med, k.w);
    const double ph = phaseD((double)a.med.g, -b.dir, -cam.d);
    const double kernelVol = (4.0 / 3.0) * 3.14159265358979323846 * k.radius * k.radius * k.radius;
    const double sc = mB.tr * mCam.tr * ph / k.pdfKernel / mB.pdfFailure;
    k.contrib = mkd(b.flux.x * sigS.x * sc, b.flux.y * sigS.y * sc, b.flux.z * sigS.z * sc);
    k.weightKernel = 1.0 / kernelVol;
    k.beamTrans = mB.tr;
    k.pdfEdgeFailure = mB.pdfFailure;
  }
  k.valid = !(k.contrib.x == 0 && k.contrib.y == 0 && k.contrib.z == 0);
}

// BeamKernelRecord copy-shift constructor (3D), shift_volume_beams.h:40-144
__device__ __forceinline__ void krecShifted(const KRecD &ori, const BeamD &b, const RayD &cam, KRecD &k) {
  k = ori;
  k.u = 0;
  k.contrib = mkd(0, 0, 0);
  k.valid = false;
  const RayD _cam{at(cam, cam.mint), cam.d, 0.0, cam.maxt - cam.mint};
  const RayD _beam{b.p1, b.dir, 0.0, b.len};
  double tN, tF;
  if (!cylinderIntersection(_cam, _beam, k.radius, tN, tF)) return;
  k.v = ori.v;
  k.pdfKernel = 1.0 / fmax(tF - tN, 0.0001);
  if (k.v < 0 || k.v > b.len) return;
  const d3 kc = b.p1 + b.dir * k.v;
  const double distToProj = dot(kc - cam.o, cam.d);
  const double distSqr = len2(at(cam, distToProj) - kc);
  const double radSqr = k.radius * k.radius;
  if (distSqr >= radSqr) return;
  const double deltaT = sqrt(fmax(0.0, radSqr - distSqr));
  k.w = ori.w;
  k.pdfKernel *= 1.0 / fmax(2.0 * deltaT, 0.0001);
  if (k.w < cam.mint || k.w > cam.maxt) return;
  k.contrib = ori.contrib * (ori.pdfKernel / k.pdfKernel);
  k.valid = !(k.contrib.x == 0 && k.contrib.y == 0 && k.contrib.z == 0);
}

// BeamKernelRecord::kernelPDF, shift_volume_beams.h:300-336
__device__ __forceinline__ double kernelPDF(const KRecD &k, int technique, const RayD &cam, d3 orgBeam, d3 dBeam,
                                            double newDLength) {
  if (technique == GVPM_BEAM_BEAM_1D) return sqrt(len2(crossd(cam.d, dBeam)));
  const RayD _beam{orgBeam, dBeam, 0.0, INFINITY};
  const RayD _cam{cam.o, cam.d, 0.0, cam.maxt};
  double tN, tF;
  if (cylinderIntersection(_cam, _beam, k.radius, tN, tF)) {
    double pk = 1.0 / fmax(tF - tN, 0.0001);
    const d3 kc = orgBeam + dBeam * newDLength;
    const double distToProj = dot(kc - cam.o, cam.d);
    const double distSqr = len2(at(cam, distToProj) - kc);
    const double radSqr = k.radius * k.radius;
    if (distSqr < radSqr) {
      const double deltaT = sqrt(fmax(0.0, radSqr - distSqr));
      pk *= 1.0 / fmax(2.0 * deltaT, 0.0001);
      return pk;
    }
    return 0.0;
  }
  return 0.0;
}

// shift(), shift_volume_beams.cpp:47-79 with localMatrix (:37-42)
__device__ __forceinline__ d3 shiftPoint(const RayD &r, d3 a, double u, double w, bool flip) {
  const double d = dot(a - r.o, r.d);
  d3 sv = a - at(r, d);
  sv = sv / sqrt(len2(sv));
  const d3 tv = crossd(r.d, sv);
  // Frame{s = r.d, t = sv, n = tv}
  const d3 av = a - at(r, d);
  const double ly = dot(av, sv);
  const double x = u / fabs(ly);
  double phi = 1.57079632679489661923 - asin(fmin(1.0, fmax(-1.0, x)));
  if (flip) phi = -phi;
  const double lwy = u * cos(phi), lwz = u * sin(phi);
  return at(r, w) + (sv * lwy + tv * lwz);
}

__device__ __forceinline__ d3 getShiftPos1D(const RayD &bRay, const RayD &sRay, d3 a, d3 bBeamDir, double w, double u) {
  d3 back = shiftPoint(bRay, a, u, w, false) - a;
  back = back / sqrt(len2(back));
  const bool flip = len2(back - bBeamDir) > 0.001;
  return shiftPoint(sRay, a, u, w, flip);
}

__device__ __forceinline__ d3 getShiftPos3D(const GatherArgs &a, const RayD &bRay, const RayD &sRay, double w, d3 u,
                                            double radius, double newW) {
  d3 bs, bt, ns, nt;
  coordSysCoherent(bRay.d, bs, bt);
  coordSysCoherent(sRay.d, ns, nt);
  const double lx = dot(u, bs), ly = dot(u, bt), lz = dot(u, bRay.d);
  d3 newPos = at(sRay, newW) + (ns * lx + nt * ly + sRay.d * lz);
  if (a.cfg.use_shift_null) {
    const d3 bCamW = at(bRay, w);
    if (len2(bCamW - newPos) < radius * radius) {
      d3 dShift = at(sRay, newW) - bCamW;
      dShift = dShift / sqrt(len2(dShift));
      const double cosD = dot(dShift, -(newPos - at(sRay, newW)));
      newPos = newPos + dShift * (cosD * 2.0);
    }
  }
  return newPos;
}

// shiftBeamDiffuse + diffuseReconnectionPhotonBeam.  Returns the MIS weight.
template <int B, bool EXV = false>
__device__ __forceinline__ double shiftBeamDiffuse(const GatherArgs &a, const TileLds<B> &s, const BeamD &b,
                                                   const RayReg &sh, const RayReg &base, uint32_t edge,
                                                   const RayD &shiftRay, double shiftW, const KRecD &kRec, d3 newPos,
                                                   int technique, d3 &shiftedFlux, bool &ok) {
  const double INV_PI = 0.31830988618379067154;
  ok = false;
  shiftedFlux = mkd(0, 0, 0);
  d3 newPBDir = newPos - b.p1;
  const double newPBDist = sqrt(len2(newPBDir));
  newPBDir = newPBDir / newPBDist;
  // visibility over the whole new beam [Epsilon, newPBDist], shift_volume_beams.cpp:420-426
  // (EXV: the exact pass -- every triangle test of the segment in fp64, occlusion.h anyHitExact)
  if (EXV ? anyHitExact(a, tof(b.p1), newPBDir, (double)a.cfg.epsilon, newPBDist)
          : (anyHitScene<true>(a.bvh, a.tri4, a.ntri, tof(b.p1), tof(newPBDir), a.cfg.epsilon, (float)newPBDist) & 1) != 0)
    return 1.0;
  const d3 basePos = b.p1 + b.dir * kRec.v;
  const double pdfKernelAndDist = kpdf(kRec);
  // diffuseReconnectionPhotonBeam, shift_diffuse.cpp:136-268
  const uint32_t ptype = GVPM_PF_PARENT_TYPE(b.flags);
  d3 thr;
  double pdfValueSA;
  if (ptype == GVPM_PARENT_SURFACE || ptype == GVPM_PARENT_SURFACE_BSDF) {
    const double cosWo = dot(b.parentN, newPBDir), cosWi = dot(b.parentN, b.parentWi);
    // eval = pdf = 0 (or the shading-normal reject): sRec.pdf == 0; a glossy parent met from the other side (a transmitted
    // photon of a rough dielectric) is glossyParentEval's to decide
    if (cosWo <= 0 || (ptype == GVPM_PARENT_SURFACE_BSDF ? cosWi == 0 : cosWi <= 0)) return 1.0;
    thr = b.parentScat * (INV_PI * cosWo);
    pdfValueSA = INV_PI * cosWo;
    if (ptype == GVPM_PARENT_SURFACE_BSDF) {
      // a glossy parent (gvpm_upload_bsdfs): Phong in fp64 (src/bsdfs/phong.cpp:121-186,331-342; parent_bsdf.h phongEvalD)
      if (!phongEvalD(a, (float)b.parentG, b.parentScat, b.parentN, b.parentWi, newPBDir, cosWi, cosWo, thr, pdfValueSA)) {
        // (the other table entries -- the rough conductor -- through the fp32 statement the default path uses)
        f3 ff;
        float pp;
        if (!glossyParentEval(a, (float)b.parentG, tof(b.parentScat), tof(b.parentN), tof(b.parentWi), tof(newPBDir), (float)cosWi,
                              (float)cosWo, ff, pp))
          return 1.0;
        thr = tod(ff);
        pdfValueSA = (double)pp;
      }
    }
  } else if (ptype == GVPM_PARENT_MEDIUM) {
    const double p = phaseD(b.parentG, b.parentWi, newPBDir);
    thr = b.parentScat * p;
    pdfValueSA = p;
  } else {
    double dp = dot(newPBDir, b.parentN);
    if (dp < 0) dp = 0.0;
    thr = mkd(INV_PI * dp, INV_PI * dp, INV_PI * dp);
    pdfValueSA = INV_PI * dp;
  }
  const double GOpNew = 1.0 / (newPBDist * newPBDist);
  double sPdf = pdfValueSA * GOpNew;
  thr = thr * GOpNew;
  double pdfBasePos = b.parentPdf * len2(b.p1 - b.p2);
  if (b.endOnSurface) pdfBasePos /= fabs(dot(b.endN, b.dir));
  pdfBasePos *= 1.0 / len2(b.p1 - basePos);
  if (pdfBasePos == 0.0) return 1.0;
  thr = thr * (b.parentRR / pdfBasePos);
  if (GVPM_PF_EDGE_IN_MEDIUM(b.flags)) {
    const MRecD m = mediumEvalD(a.med, newPBDist);
    sPdf *= m.pdfFailure;
    thr = thr * (m.tr / pdfKernelAndDist);
  }
  if (sPdf == 0.0) return 1.0;
  const double shiftKernelPDF = kernelPDF(kRec, technique, shiftRay, b.p1, newPBDir, newPBDist);
  if (shiftKernelPDF == 0) return 1.0;
  const d3 sigS = mkd(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]);
  const MRecD mS = mediumEvalD(a.med, shiftW);
  const double ph = phaseD((double)a.med.g, -newPBDir, -shiftRay.d) * mS.tr;
  const d3 eye = tod(sh.eye);
  shiftedFlux = mkd(b.prefixW.x * thr.x * sigS.x * ph * eye.x, b.prefixW.y * thr.y * sigS.y * ph * eye.y,
                    b.prefixW.z * thr.z * sigS.z * ph * eye.z);
  ok = true;
  double w = 0.5;
  if (a.cfg.use_mis) {
    double basePdf = b.parentPdf * len2(b.p1 - b.p2);
    if (b.endOnSurface) basePdf /= fabs(dot(b.endN, b.dir));
    basePdf /= len2(b.p1 - basePos);
    basePdf *= pdfKernelAndDist;
    const double offsetPdf = shiftKernelPDF * sPdf;
    if (offsetPdf == 0.0 || basePdf == 0.0) {
      ok = false;
      return 1.0;
    }
    // sensorMIS(currCameraEdge, base, shiftW, kRec.w): the two distances are equal
    const double x = (double)sensorMIS(sh, base, edge) * offsetPdf / basePdf;
    w = a.cfg.power_heuristic ? 1.0 / (1.0 + x * x) : 1.0 / (1.0 + x);
  }
  return w;
}

__device__ __forceinline__ BeamD loadBeam(const GatherArgs &a, uint32_t idx) {
  const float4 *rec = a.cold + (size_t)idx * GVPM_REC_QUADS;
  const float4 c1 = rec[0], c2 = rec[1], c3 = rec[2], c4 = rec[3], c5 = rec[4], c6 = rec[5], c7 = rec[6], c8 = rec[7];
  BeamD b;
  b.parentPdf = c1.w;
  b.flux = mkd(c1.x, c1.y, c1.z);
  b.p1 = mkd(c2.x, c2.y, c2.z); b.parentRR = c2.w;
  b.parentN = mkd(c3.x, c3.y, c3.z); b.parentG = c3.w;
  b.prefixW = mkd(c4.x, c4.y, c4.z);
  b.parentScat = mkd(c5.x, c5.y, c5.z);
  b.parentWi = mkd(c6.x, c6.y, c6.z);
  b.p2 = mkd(c7.x, c7.y, c7.z); b.flags = __float_as_uint(c7.w);
  b.endN = mkd(c8.x, c8.y, c8.z);
  b.endOnSurface = !(c8.x == 0.f && c8.y == 0.f && c8.z == 0.f);
  // PhotonBeam::setEndPoint, pm/beams_struct.h:73-81
  b.dir = b.p2 - b.p1;
  b.len = sqrt(len2(b.dir));
  b.dir = b.dir / b.len;
  return b;
}

// One (camera ray, sub-beam) candidate: BeamGradRadianceQuery::operator().  Returns true when it
// produced a contribution (an evaluation).
// only >= 0 (the exact pass, exact_beams_kernel): shift `only` of a pair the fp32 evaluation has already evaluated -- its
// terms and its counter, not the base contribution, not the other shifts.
template <int B, bool EXV = false>
__device__ __forceinline__ bool evaluateBeam(const GatherArgs &a, TileLds<B> &s, uint32_t id, uint32_t bIdx,
                                             uint32_t &nNull, uint32_t &nDiff, uint32_t &nFail, int only = -1) {
  const uint32_t beamIdx = id & 0xFFFFFFu, sub = id >> 24;
  const BeamD b = loadBeam(a, beamIdx);
  const RayReg base = loadRay(s, 0, bIdx);
  const uint32_t edge = s.edge[bIdx];
  const uint32_t pix = s.pix[bIdx];
  const int px = (int)(pix & 0xFFFFu), py = (int)(pix >> 16);
  const int technique = a.cfg.vol_technique;
  // filters, shift_volume_beams.cpp:142-184
  const int pathLength = (int)edge + (int)GVPM_PF_DEPTH(b.flags);
  if (a.cfg.max_depth > 0 && pathLength > a.cfg.max_depth) return false;
  if (!((b.flags >> 6) & 1u)) return false;  // computeVolumeContribution (folded at build time)
  double rr = 1.0;
  if (a.cfg.path_set) {
    if (((b.flags >> GVPM_HOT_PARITY_BIT) & 1u) != (uint32_t)((px + py) & 1)) return false;
    rr = 2.0;
  }
  // the sub-beam [tmin, tmax) of this candidate (SubBeamBVH, pm/beams_accel.h:119-131)
  const uint32_t nSub = subBeamCount((float)b.len, a.subLen);
  const float ls = (float)b.len / (float)nSub;
  const double tmin = (double)(ls * (float)sub);
  const double tmax = (sub + 1u >= nSub) ? INFINITY : (double)(ls * (float)(sub + 1u));
  const double eps = (double)a.cfg.epsilon;
  const RayD cam{tod(base.o), tod(base.d), eps, (double)base.len - eps};
  uint32_t o0, o1;
  philox4x32_10(__float_as_uint(s.rnd[bIdx]), 0x6265616du, beamIdx, o0, o1);
  const double uv = (double)((float)(o0 >> 8) * (1.0f / 16777216.0f));
  const double uw = (double)((float)(o1 >> 8) * (1.0f / 16777216.0f));
  KRecD kRec;
  kRec.radius = (double)a.kernelRadius;
  kRec.v = kRec.w = kRec.pdfKernel = kRec.pdfEdgeFailure = kRec.u = kRec.weightKernel = kRec.beamTrans = 0;
  kRec.contrib = mkd(0, 0, 0);
  if (technique == GVPM_BEAM_BEAM_1D) {
    if (!beamOwner1D(b, cam, sub, nSub, tmin, tmax)) return false;
    krecEval(a, b, cam, 0.0, INFINITY, uv, uw, technique, kRec);
  } else {
    krecEval(a, b, cam, tmin, tmax, uv, uw, technique, kRec);
  }
  if (!kRec.valid) return false;
  const d3 eyeB = tod(base.eye);
  const d3 baseContrib = mkd(eyeB.x * kRec.contrib.x, eyeB.y * kRec.contrib.y, eyeB.z * kRec.contrib.z) * kRec.weightKernel;
  if (only < 0) {
    atomicAdd(&s.acc[0][bIdx], (double)(float)(baseContrib.x * rr));
    atomicAdd(&s.acc[1][bIdx], (double)(float)(baseContrib.y * rr));
    atomicAdd(&s.acc[2][bIdx], (double)(float)(baseContrib.z * rr));
  }
  const uint32_t st = GVPM_PF_SHIFT_TYPE(b.flags);
  if (a.cfg.debug_shift != GVPM_SHIFT_ALL && a.cfg.debug_shift != GVPM_SHIFT_NULL) {
    const int cur = st == 1u ? GVPM_SHIFT_DIFFUSE : st == 2u ? GVPM_SHIFT_MEDIUM : st == 3u ? GVPM_SHIFT_MANIFOLD : GVPM_SHIFT_INVALID;
    if (a.cfg.debug_shift != cur) return false;  // base contribution kept, no shifts (shift_volume_beams.cpp:210-216)
  }
  const double radius = kRec.radius;
#pragma unroll 1
  for (int i = 0; i < 4; ++i) {
    if (only >= 0 && i != only) continue;
    const RayReg sh = loadRay(s, 1 + i, bIdx);
    double w = 1.0;
    d3 sflux = mkd(0, 0, 0);
    if (sh.valid) {
      const double shiftDistMAX = (double)sh.len;
      const RayD shiftRay{tod(sh.o), tod(sh.d), eps, shiftDistMAX};
      const double shiftW = kRec.w;
      bool alreadyShift = false;
      if (a.cfg.use_shift_null && technique != GVPM_BEAM_BEAM_1D) {
        const d3 kernelPos = b.p1 + b.dir * kRec.v;
        const double ZPtoY = len2(at(shiftRay, shiftW) - kernelPos);
        if (ZPtoY < radius * radius && kRec.w <= shiftDistMAX) {
          KRecD kS;
          krecShifted(kRec, b, shiftRay, kS);
          if (kS.valid) {
            // shiftNull3D, shift_volume_beams.cpp:748-786
            nNull++;
            const d3 eyeS = tod(sh.eye);
            const double f = kpdf(kS) / kpdf(kRec);
            sflux = mkd(kS.contrib.x * f * eyeS.x, kS.contrib.y * f * eyeS.y, kS.contrib.z * f * eyeS.z);
            w = 0.5;
            if (a.cfg.use_mis) {
              const double basePdf = kpdf(kRec), offsetPdf = kpdf(kS);
              if (offsetPdf == 0.0 || basePdf == 0.0) w = 1.0;
              else {
                const double x = (double)sensorMIS(sh, base, edge) * (offsetPdf / basePdf);
                w = a.cfg.power_heuristic ? 1.0 / (1.0 + x * x) : 1.0 / (1.0 + x);
              }
            }
            alreadyShift = true;
          }
        }
      }
      if (!alreadyShift && kRec.w <= shiftDistMAX) {
        bool doShift = true;
        d3 offsetPos;
        if (technique != GVPM_BEAM_BEAM_1D) {  // newShiftBeam == false
          const double minDistSqr = len2(b.p1 - at(shiftRay, dot(b.p1 - shiftRay.o, shiftRay.d)));
          if (minDistSqr > kRec.u * kRec.u) {
            offsetPos = getShiftPos3D(a, cam, shiftRay, kRec.w, (b.p1 + b.dir * kRec.v) - at(cam, kRec.w), radius, shiftW);
          } else {
            doShift = false;  // result.weight = 1
          }
        } else {
          offsetPos = getShiftPos1D(cam, shiftRay, b.p1, b.dir, kRec.w, kRec.u);
        }
        if (doShift) {
          // shiftBeam dispatch, shift_volume_beams.cpp:355-408
          if (a.cfg.debug_shift == GVPM_SHIFT_NULL || shiftW > shiftRay.maxt) {
            w = 1.0;
          } else {
            bool ok = false;
            if (st == 1u || st == 2u)
              w = shiftBeamDiffuse<B, EXV>(a, s, b, sh, base, edge, shiftRay, shiftW, kRec, offsetPos, technique, sflux, ok);
            if (ok) nDiff++; else nFail++;
          }
        }
      }
    }
    if ((i == GVPM_RIGHT && px == a.cfg.width - 1) || (i == GVPM_TOP && py == a.cfg.height - 1)) w = 1.0;
    const double ws = w * rr;
    if (sflux.x != 0 || sflux.y != 0 || sflux.z != 0) {
      const double wk = ws * kRec.weightKernel;
      atomicAdd(&s.acc[3 + 3 * i + 0][bIdx], (double)(float)(sflux.x * wk));
      atomicAdd(&s.acc[3 + 3 * i + 1][bIdx], (double)(float)(sflux.y * wk));
      atomicAdd(&s.acc[3 + 3 * i + 2][bIdx], (double)(float)(sflux.z * wk));
    }
    atomicAdd(&s.acc[15 + 3 * i + 0][bIdx], (double)(float)(baseContrib.x * ws));
    atomicAdd(&s.acc[15 + 3 * i + 1][bIdx], (double)(float)(baseContrib.y * ws));
    atomicAdd(&s.acc[15 + 3 * i + 2][bIdx], (double)(float)(baseContrib.z * ws));
  }
  return true;
}

}  // namespace gvpm
