// G-Beams (beam x beam) gather + gradient-domain shift for gfx950, hand-written HIP.
//
// Replaces, for one SPPM iteration, the body of
//   GPMIntegrator::computeVolumeGradientBeams     gvpm/gvpm.cpp:880-986
//   SubBeamBVH (build + query)                    pm/beams_accel.h:82-267
//   BeamGradRadianceQuery::operator()             gvpm/shift/shift_volume_beams.cpp:139-353
//   BeamKernelRecord (1D, 3D "optimized")         gvpm/shift/shift_volume_beams.h:24-338
//   PhotonBeam::rayIntersectInternal1D/getContrib pm/beams_struct.h:250-311,136-185
//   cylinderIntersection                          pm/beams_3d_intersections.h:77-140
//   getShiftPos / getShiftPos1D / shift           shift_volume_beams.cpp:37-137
//   shiftBeam / shiftBeamDiffuse / shiftNull3D    shift_volume_beams.cpp:355-539,748-786
//   diffuseReconnectionPhotonBeam                 gvpm/shift/operation/shift_diffuse.cpp:136-268
// (pm/ = src/integrators/photonmapper/).
//
// Acceleration structure: like the reference, every photon beam is cut into sub-beams (here of
// about one grid cell) and each sub-beam is binned ONCE, by its centre, into the same sorted
// uniform grid the photon kernels use; the camera tile walks the grid with the kernel radius
// inflated by half a sub-beam.  A (camera ray, beam) pair is evaluated by the one sub-beam that
// owns the intersection -- the reference's own rule (1D: v in (t1,t2], beams_struct.h:297-299;
// 3D: tNear in (t1,t2), shift_volume_beams.h:213-220) -- so the result does not depend on how
// beams are cut.  Traversal, LDS staging, ballot compaction and the work queue are those of the
// BRE kernel (tile_walk.h).  The evaluation runs in fp32 in a local frame (beams_eval_f32.h), in two
// phases (base + null shifts, then the queued reconnections); the literal fp64 transcription of the
// reference with its float intermediates is kept as the on-device cross-check (GVPM_BEAMS_FP64=1), settles the ownership
// decisions that fall inside the fp32 error band and -- round 5 -- is what exact_beams_kernel evaluates, one at a time, the shifts
// with whose own decisions fp32 cannot be trusted (beamShift1 / beamShift2 note them).
#include <hip/hip_runtime.h>

#include "beams_eval_f32.h"
#include "device_types.h"
#include "dmath.h"
#include "shift_device.h"
#include "tile_walk.h"
#include "vec.h"

#ifndef GVPM_BSTAGE
#define GVPM_BSTAGE 128
#endif

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

// number of sub-beams of a beam of length len for target length ls (shared with the grid build)
__device__ __forceinline__ uint32_t subBeamCount(float len, float ls) {
  const float n = ceilf(len / ls);
  return (uint32_t)fminf(fmaxf(n, 1.f), 255.f);
}

// fp32 necessary condition for evaluateBeam to produce anything for (camera ray, sub-beam): the two lines pass
// within the kernel radius and the parameter that decides ownership (3D: where the beam enters the camera ray's
// capped cylinder, shift_volume_beams.h:213-220; 1D: the closest approach, beams_struct.h:297-299) falls in this
// sub-beam's range, fattened by a margin that covers the fp32 error.  Everything is measured from the sub-beam's
// centre, which the sphere test already placed within radius + half a sub-beam of the ray, so the operands are small
// and well conditioned; near-parallel pairs are passed through.  The fp64 evaluation that follows repeats the
// reference's tests exactly: the prefilter only removes pairs it would reject (~7 of 8: each beam crosses the ray's
// neighbourhood with several sub-beams and exactly one owns the pair).
__device__ __forceinline__ bool beamPrefilter(const RayReg &base, f3 C, f3 bd, float ls, uint32_t sub, float r, float eps,
                                              int technique) {
  const f3 co = C - base.o;
  const float sC = dot(co, base.d);
  const f3 D0 = co - base.d * sC;  // centre relative to its projection on the camera line
  const float bdd = dot(bd, base.d);
  const float sin2 = fmaxf(1.f - bdd * bdd, 0.f);
  if (sin2 < 1e-5f) return true;
  const float inv = frcp(sin2);
  const float tau0 = -(dot(D0, bd) - dot(D0, base.d) * bdd) * inv;  // closest approach, from the centre
  const f3 cr = cross(bd, base.d);
  const float ad = dot(D0, cr);
  const float dmin2 = ad * ad * inv;
  if (dmin2 >= r * r * 1.002f) return false;
  const float delta = 0.01f * ls + 1e-5f * (r + ls) * inv;
  const float half = 0.5f * ls;
  float tau;
  if (technique == GVPM_BEAM_BEAM_1D) {
    // the sub-beam that contains the geometric closest approach speaks for the beam (beamOwner1D; the first one also
    // for an approach before the beam's origin -- one beyond either end can only be accepted through the reference's
    // rounding, and then by no candidate of this traversal: the bounded difference DESIGN.md states)
    tau = tau0;
    return tau < half + delta && (sub == 0u || tau > -half - delta);
  }
  const float hw = fsqrt(fmaxf(r * r - dmin2, 0.f) * inv);
  float tN = tau0 - hw, tF = tau0 + hw;
  // caps of the camera ray's cylinder [mint, maxt] (cylinderIntersection, beams_3d_intersections.h:118-137)
  const float lMax = base.len - 2.f * eps;
  const float zc = sC - eps;
  const float zN = zc + tN * bdd, zF = zc + tF * bdd;
  const float zmarg = 1e-4f * (fabsf(zc) + r);
  if (zN < 0.f) {
    if (zF < -zmarg) return false;
    if (zN != zF) tN = tN + (tF - tN) * fminf(fmaxf(zN / (zN - zF), 0.f), 1.f);
  } else if (zN > lMax) {
    if (zF > lMax + zmarg) return false;
    if (zN != zF) tN = tN + (tF - tN) * fminf(fmaxf((zN - lMax) / (zN - zF), 0.f), 1.f);
  }
  tau = tN;
  // owner: tmin < tN < tmax, or the first sub-beam when the ray's cylinder already contains the beam's origin
  if (tau > -half - delta && tau < half + delta) return true;
  return sub == 0u && tau < -half + delta;
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

#ifdef GVPM_BEAMS_AUDIT
// probe builds only (bash scripts/build_variant.sh baudit gather_beams.hip -DGVPM_BEAMS_AUDIT; scripts/beams_audit.py):
// the fp32 kernel record runs the fp64 transcription for EVERY pair and logs (i) the pairs whose banded fp32 decision
// was taken as sure and differs from the transcription's, (ii) the largest observed |fp32 - fp64| / band per quantity
// over the pairs both accept: the safety factor of each band.
__device__ unsigned int gvpmAuditCount;
__device__ float gvpmAuditLog[256][16];
__device__ unsigned int gvpmAuditRatio[8];  // float bits (positive): [0] tN [1] v [2] w [3] pdfKernel (relative, no band)
extern "C" int gvpm_debug_beams_audit(unsigned int *count, float *log, float *ratio) {
  if (hipMemcpyFromSymbol(count, HIP_SYMBOL(gvpmAuditCount), 4) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(log, HIP_SYMBOL(gvpmAuditLog), sizeof(float) * 256 * 16) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(ratio, HIP_SYMBOL(gvpmAuditRatio), 32) != hipSuccess) return -1;
  return 0;
}
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
// beam (beam_near_kernel, grid_build.hip), or all of them when the list overflowed / the scene is large.
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

// The rest of shiftBeamME once the host has run the walks (results == nullptr: it has not -- every request is a failed shift):
// kernelPDF of the proposal's last edge against the shifted ray (:653-663), Jacobian (:665-686), the shifted camera terms
// (:688-703), MIS (:705-733), then the accumulation of BeamGradRadianceQuery::operator() (:330-350).  For G-Beams the answer's
// `wi` is the proposal's last edge as a VECTOR from the new vertex to its predecessor (direction and length).
__global__ __launch_bounds__(256) void apply_host_shifts_beams_kernel(GatherArgs a, const gvpm_host_shift *__restrict__ results, uint32_t n) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t ok = 0, bad = 0;
  if (k < n) {
    const float4 c0 = a.reqCtx[5 * (size_t)k], c1 = a.reqCtx[5 * (size_t)k + 1], c2 = a.reqCtx[5 * (size_t)k + 2],
                 c3 = a.reqCtx[5 * (size_t)k + 3], c4 = a.reqCtx[5 * (size_t)k + 4];
    const f3 bcv = mk3(c2.x, c2.y, c2.z), eye = mk3(c3.x, c3.y, c3.z);
    const float shiftW = c1.w, wkrr = c2.w, sMIS = c3.w, radius = c4.x;
    const uint32_t pix = __float_as_uint(c4.y);
    const int i = (int)__float_as_uint(c4.z);
    float w = 1.f;
    f3 sflux = mk3(0.f);
    bool good = false;
    if (results && results[k].ok) {
      const gvpm_host_shift r = results[k];
      const gvpm_shift_request rq = a.reqHost[k];
      const d3 wiV = mkd(r.wi[0], r.wi[1], r.wi[2]);
      const double newLen = sqrt(len2(wiV));
      const double jac = (double)r.det_ratio;
      if (newLen > 0.0) {
        const d3 edgeD = wiV * (-1.0 / newLen);  // proposal.edge(c - 1)->d
        const d3 newPos = mkd(rq.offset_pos[0], rq.offset_pos[1], rq.offset_pos[2]);
        const d3 orgBeam = newPos + wiV;         // proposal.vertex(c - 1)
        KRecD kr;
        kr.radius = (double)radius;
        const RayD shRay{mkd(c0.x, c0.y, c0.z), mkd(c1.x, c1.y, c1.z), (double)a.cfg.epsilon, (double)c0.w};
        const double shiftKernelPDF = kernelPDF(kr, a.cfg.vol_technique, shRay, orgBeam, edgeD, newLen);
        if (shiftKernelPDF != 0.0 && jac > 0.0 && isfinite(jac)) {
          good = true;
          const float tr = mediumEvalF(a.med, shiftW).tr;
          const f3 sigS = mk3(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]);
          const f3 shD = mk3(c1.x, c1.y, c1.z);
          const float phaseTerm = phaseEval(a.med.g, tof(edgeD) * -1.f, -shD);
          sflux = mk3(r.throughput[0], r.throughput[1], r.throughput[2]) * sigS * (tr * phaseTerm) * eye * (float)jac;
          w = 0.5f;
          if (a.cfg.use_mis) {
            const double offsetPdf = (double)r.pdf * shiftKernelPDF, basePdf = (double)r.base_pdf;
            if (basePdf == 0.0) {
              w = 0.f;
            } else if (offsetPdf == 0.0) {
              w = 1.f;
            } else {
              const double x = (double)sMIS * jac * (offsetPdf / basePdf);
              w = (float)(a.cfg.power_heuristic ? 1.0 / (1.0 + x * x) : 1.0 / (1.0 + x));
            }
          }
        }
      }
    }
    if (beamBorder(a, pix, i)) w = 1.f;
    const size_t p = (size_t)(pix >> 16) * a.cfg.width + (pix & 0xFFFFu);
    float *dst = a.iter + p * 27;
    const float ws = w * wkrr * a.iterScale, wb = w * a.iterScale;
    if (sflux.x != 0.f || sflux.y != 0.f || sflux.z != 0.f) {
      atomicAdd(&dst[3 + 3 * i + 0], sflux.x * ws);
      atomicAdd(&dst[3 + 3 * i + 1], sflux.y * ws);
      atomicAdd(&dst[3 + 3 * i + 2], sflux.z * ws);
    }
    atomicAdd(&dst[15 + 3 * i + 0], bcv.x * wb);
    atomicAdd(&dst[15 + 3 * i + 1], bcv.y * wb);
    atomicAdd(&dst[15 + 3 * i + 2], bcv.z * wb);
    ok = good ? 1u : 0u;
    bad = good ? 0u : 1u;
  }
  const uint32_t nOk = (uint32_t)__popcll(__ballot(ok != 0u)), nBad = (uint32_t)__popcll(__ballot(bad != 0u));
  if ((threadIdx.x & 63) == 0 && (nOk | nBad)) {
    atomicAdd(&statRow(a)[3], (unsigned long long)nOk);
    atomicAdd(&statRow(a)[4], (unsigned long long)nBad);
  }
}
void launch_apply_host_shifts_beams(const GatherArgs &a, const gvpm_host_shift *results, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(apply_host_shifts_beams_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, results, n);
}

// what the reconnections of one pair share (diffuseReconnectionPhotonBeam's base side, the medium up to w)
struct BeamRecPair {
  float pdfBasePos;   // parentPdf * |p1 - p2|^2 [/ |n_end . d|] / v^2
  float trW;          // transmittance of the camera ray up to w (the shifted rays keep w)
  float pdfKernelAndDist;
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
    thr = thr * fdiv(m.tr, pr.pdfKernelAndDist);
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
      pr.trW = mediumEvalF(a.med, kW).tr;
      pr.pdfKernelAndDist = q.k.z;
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


// ---- traversal: (camera ray, sub-beam) pairs that survive the sphere test and the fp32 prefilter ---------------
// Persistent waves over the planner's items (tile_walk.h), built like the BRE traversal: the sub-beam records of a
// slab box -- {centre, beam | sub << 24} {direction, sub-beam length} + the beam's filter bits, 36 bytes -- are
// staged in LDS; every lane (ray b = lane % B, slot = lane / B) sphere-tests G staged records branch-free, then the
// wave resolves the marked ones one per lane and round: flag filters (contribution, checkerboard parity, depth) and
// the ownership prefilter, straight from LDS and the lane's own ray registers.  Survivors are compacted by ballot
// into an LDS ring and appended to the global pair list 64 at a time (one atomic per 64 pairs; the tail of an item
// is padded with empty pairs so that a block of 64 never mixes tiles).  pair = {beam | sub << 24, sorted set index}.
// (a stage of 128: the one-layer slab boxes hold ~100 sub-beams, and 6 KB of LDS per wave instead of 10 leaves room
// for more resident waves, which is what hides the per-slab latency chain)
constexpr int BSTAGE = GVPM_BSTAGE;
constexpr int BCQ = 512;  // sphere-test survivors waiting for the prefilter (a group adds at most 4 x 64, 63 wait; power of 2)
typedef float v2fb __attribute__((ext_vector_type(2)));
struct alignas(16) BeamTravLds {
  float4 st0[BSTAGE], st1[BSTAGE];
  // the centres and the filter bits once more, one array per component: the sphere test reads FOUR consecutive staged
  // sub-beams with four ds_read_b128 issued together and tests two at a time in packed fp32 (as the G-BRE traversal)
  float sx[BSTAGE], sy[BSTAGE], sz[BSTAGE];
  uint32_t stF[BSTAGE];
  uint2 outq[QCAP];
  float4 rayO[64], rayD[64];  // the tile's base rays {o, len} {d, -}: a candidate is resolved by ANY lane
  uint16_t candq[BCQ];        // staged record | ray << 8
};

#ifdef GVPM_TRAV_TIMING
// probe builds only: per wave of the last launch {start, end (wall clock, 100 MHz), items, candidates}
__device__ unsigned long long gvpmBeamTravLog[4 * 8192];
extern "C" int gvpm_debug_beamtrav_timing(unsigned long long *out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(gvpmBeamTravLog), sizeof(gvpmBeamTravLog)) == hipSuccess ? 0 : -1;
}
#endif
template <int B>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void traverse_beams_kernel(GatherArgs a, const uint32_t *__restrict__ hotFlags,
                                                            const uint4 *__restrict__ items,
                                                            const uint32_t *__restrict__ itemCount, uint32_t itemCap, uint32_t *queueHead,
                                                            uint2 *__restrict__ pairs, uint32_t *pairCount,
                                                            uint32_t pairCap, uint32_t *__restrict__ blockKey,
                                                            uint32_t *__restrict__ blockVal) {
  constexpr int LPB = 64 / B;
  __shared__ BeamTravLds s;
  const int lane = threadIdx.x;
  const int technique = a.cfg.vol_technique;
  // (the planner counts the items it had no room to write: never read past the list; the host regrows it and repeats)
  const uint32_t nItems = min(*itemCount, itemCap);
  const int b = lane % B, sub = lane / B;
  const float rT = a.radius;  // test radius = kernel radius + half a sub-beam
  const float r = a.kernelRadius;
  const float eps = a.cfg.epsilon;
  const bool pathSet = a.cfg.path_set != 0;
  const int maxDepth = a.cfg.max_depth;
  unsigned long long nCand = 0;
#ifdef GVPM_TRAV_TIMING
  const unsigned long long tw0 = wall_clock64();
  unsigned long long nIt = 0;
#endif
  // Blocks of the pair list are reserved RESERVE at a time: atomics on one address retire at ~11 ns each on this
  // part whatever the number of waves (scripts/probes/atomics_bench.hip), so one atomic per block (~260 k per pass)
  // bounded the kernel at 3 ms.  What a wave has left over at the end is written as empty blocks of its last tile.
  constexpr uint32_t RESERVE = 8u;
  uint32_t resSlot = 0, resLeft = 0, lastSet = 0;

  // the first item of every wave is its own index; the shared counter (one address: ~11 ns per atomic whatever the
  // number of waves) serves the rest
  bool firstItem = true;
  for (;;) {
    uint32_t it = blockIdx.x;
    if (!firstItem) {
      if (lane == 0) it = gridDim.x + atomicAdd(queueHead, 1u);
      it = __shfl(it, 0, 64);
    }
    firstItem = false;
    it = (uint32_t)__builtin_amdgcn_readfirstlane((int)it);  // (wave-uniform: the item's record in scalar registers)
    if (it >= nItems) break;
#ifdef GVPM_TRAV_TIMING
    nIt++;
#endif
    const uint4 item = items[it];
    // a heavy item comes as `parts` items that take its staging windows round-robin (plan_kernel)
    const uint32_t setBase = item.x, nb = item.y & 0xFFu, part = (item.y >> 8) & 0xFFFu, parts = max(item.y >> 20, 1u);
    if (nb == 0) continue;
    uint32_t winIdx = 0;  // staging windows of the item so far (wave-uniform)
    BaseInfo bi;
    const RayReg base = loadBaseDirect<B>(a, setBase, nb, lane, bi);
    TileWalk w;
    tileSetupFrom(a, base, base.valid, w);
    const bool beamValid = w.beamValid;
    const float mint = eps, maxt = base.len - eps;
    const uint32_t pixParity = ((bi.pix & 0xFFFFu) + (bi.pix >> 16)) & 1u;
    const int edge = (int)bi.edge;
    // the sphere test's thresholds (an invalid beam set passes nothing) and filter words
    // (plus the fp32 error of the test itself, bounded as in the G-BRE traversal by the beam's own length: a centre that
    // passes the exact test lies within rT of the segment)
    const float eT = 1.25e-6f * 1.7321f * (fmaxf(base.len, 0.f) + 3.f * rT);
    const float thrD2 = beamValid ? rT * rT * 1.001f + 4.f * rT * eT : -1.f, thrLo = mint - rT * 1.001f - eT,
                thrHi = maxt + rT * 1.001f + eT;
    const uint32_t fmask = 0x40u | (pathSet ? (1u << GVPM_HOT_PARITY_BIT) : 0u);
    const uint32_t fwant = 0x40u | (pathSet ? (pixParity << GVPM_HOT_PARITY_BIT) : 0u);
    const int dmaxB = maxDepth - edge;
    // the tile's bounding cylinder (tile_walk.h tileCylinder; round 3): sub-beams whose centre lies outside it are not
    // staged at all -- the box of a slab step holds about three times the centres any of the tile's rays can accept
    const bool prefilter = !(a.cfg.reserved[0] & 128);
    TileCyl cyl;
    cyl.ok = false;
    if (prefilter) cyl = tileCylinder(base, beamValid, fminf(thrLo, 0.f) - rT, thrHi + rT, rT * 1.0005f, 2.f * eT);
    const bool haveCyl = prefilter && __builtin_amdgcn_readfirstlane((int)cyl.ok);
    uint32_t qHead = 0, qCount = 0;
    auto emit = [&](uint32_t n) __attribute__((always_inline)) {  // n <= 64 pairs of the ring -> one block of 64 in the global list
      if (resLeft == 0u) {
        if (lane == 0) resSlot = atomicAdd(pairCount, 64u * RESERVE);
        resSlot = __shfl(resSlot, 0, 64);
        resLeft = RESERVE;
      }
      const uint32_t slot = resSlot;
      resSlot += 64u;
      resLeft--;
      lastSet = setBase;
      const uint2 e = (uint32_t)lane < n ? s.outq[(qHead + lane) % QCAP] : make_uint2(0xFFFFFFFFu, 0u);
      if (slot + 64u <= pairCap) {  // past the capacity: counted, not written (host regrows)
        pairs[slot + lane] = e;
        if (lane == 0) {
          // the block's tile (first sorted set of its item): the evaluation takes the blocks tile by tile
          blockKey[slot / 64u] = setBase;
          blockVal[slot / 64u] = slot / 64u;
        }
      }
      qHead = (qHead + n) % QCAP;
      qCount -= n;
    };
    __syncthreads();
    if (sub == 0) {
      s.rayO[b] = make_float4(base.o.x, base.o.y, base.o.z, base.len);
      s.rayD[b] = make_float4(base.d.x, base.d.y, base.d.z, 0.f);
    }
    __syncthreads();
    uint32_t cHead = 0, cCount = 0;  // candidate ring, wave-uniform
    auto resolve = [&](uint32_t n) __attribute__((always_inline)) {  // n <= 64 candidates: ownership prefilter, survivors -> the pair ring
      __syncthreads();
      bool keep = false;
      uint32_t id = 0, rb = 0;
      if ((uint32_t)lane < n) {
        const uint32_t c = s.candq[(cHead + (uint32_t)lane) % BCQ];
        const uint32_t j = c & 0xFFu;
        rb = c >> 8;
        const float4 h0 = s.st0[j], h1 = s.st1[j], ro = s.rayO[rb], rd = s.rayD[rb];
        id = __float_as_uint(h0.w);
        RayReg ray;
        ray.o = mk3(ro.x, ro.y, ro.z);
        ray.d = mk3(rd.x, rd.y, rd.z);
        ray.len = ro.w;
        keep = beamPrefilter(ray, mk3(h0.x, h0.y, h0.z), mk3(h1.x, h1.y, h1.z), h1.w, id >> 24, r, eps, technique);
      }
      nCand += n;
      cHead = (cHead + n) % BCQ;
      cCount -= n;
      const unsigned long long km = __ballot(keep);
      if (km) {
        if (keep)
          s.outq[(qHead + qCount + (uint32_t)__popcll(km & ((1ull << lane) - 1ull))) % QCAP] = make_uint2(id, setBase + rb);
        qCount += (uint32_t)__popcll(km);
        if (qCount >= 64u) {
          __syncthreads();
          emit(64u);
          __syncthreads();
        }
      }
    };
    const int cBeg = max((int)item.z, w.cA0), cEnd = min((int)item.w, w.cA1);
    for (int cA = cBeg; cA <= cEnd; cA += w.K) {
      const int cAe = min(cA + w.K - 1, cEnd);
      CellBox bx;
      if (!slabBox(a, w, cA, cAe, bx)) continue;
      const int nranges = (bx.by1 - bx.by0 + 1) * (bx.bz1 - bx.bz0 + 1);
      for (int rbase = 0; rbase < nranges; rbase += 64) {
        uint32_t start, count;
        boxRange(a, bx, rbase + lane, nranges, start, count);
        const uint32_t incl = wave_scan_incl(count, lane);
        const uint32_t excl = incl - count;
        const uint32_t total = __shfl(incl, 63, 64);
        for (uint32_t win = 0; win < total; win += BSTAGE) {
          if (winIdx++ % parts != part) continue;
          __syncthreads();
          const uint32_t nwin = min((uint32_t)BSTAGE, total - win);
          // staged so far (wave-uniform): the window's entries inside the tile's cylinder whose beam contributes at all,
          // compacted -- and, with the checkerboard (pathSet), PARTITIONED by the beam's parity: parity 0 from slot 0 upwards,
          // parity 1 from the last slot downwards.  A ray only meets beams of its pixel's parity (shift_volume_beams.cpp:
          // 142-184), so its lanes walk their own half: half the sphere tests (round 4; the filter bits are still tested --
          // where the halves' last groups of 16 overlap, a lane reads entries of the other parity)
          uint32_t n0 = 0, n1 = 0;
          // Staging: entry k of the window is element win + k of the concatenated ranges.  Consecutive LANES take
          // consecutive entries (the range an entry falls in is found by a 6-step search over the exclusive scan,
          // through ds_bpermute), so a load instruction reads a few contiguous runs of records instead of 64
          // separate ones -- with ~80 sub-beams per range (C3: 47 M sub-beams) the per-lane copy loops had made the
          // staging alone 58 of the traversal's 104 ms.
#pragma unroll
          for (uint32_t k = (uint32_t)lane; k < (uint32_t)BSTAGE; k += 64u) {
            const uint32_t e = win + k;
            uint32_t rr = 0;
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1) {
              const uint32_t cand = rr + step;
              const uint32_t v = (uint32_t)__shfl((int)excl, (int)(cand & 63u), 64);
              if (v <= e) rr = cand;
            }
            const uint32_t rStart = (uint32_t)__shfl((int)start, (int)rr, 64), rExcl = (uint32_t)__shfl((int)excl, (int)rr, 64);
            const uint32_t gi = rStart + (e - rExcl);
            float4 c0 = make_float4(0.f, 0.f, 0.f, 0.f);
            uint32_t fl = 0;
            bool keep = k < nwin;
            if (keep) {
              c0 = a.hot[2 * (size_t)gi];
              fl = hotFlags[gi];
              keep = (fl & 0x40u) && (!haveCyl || insideCylinder(cyl, mk3(c0.x, c0.y, c0.z)));
            }
            const bool up = keep && pathSet && ((fl >> GVPM_HOT_PARITY_BIT) & 1u);
            const unsigned long long km = __ballot(keep), um = __ballot(up), lm = km & ~um;
            if (keep) {
              const unsigned long long below = (1ull << lane) - 1ull;
              const uint32_t dst = up ? (uint32_t)BSTAGE - 1u - n1 - (uint32_t)__popcll(um & below) : n0 + (uint32_t)__popcll(lm & below);
              s.st0[dst] = c0;
              s.st1[dst] = a.hot[2 * (size_t)gi + 1];
              s.sx[dst] = c0.x;
              s.sy[dst] = c0.y;
              s.sz[dst] = c0.z;
              s.stF[dst] = fl;
            }
            n0 += (uint32_t)__popcll(lm);
            n1 += (uint32_t)__popcll(um);
          }
          // the FREE slots up to each half's next multiple of 16 hold centres no ray can meet
          {
            const uint32_t free0 = n0, free1 = (uint32_t)BSTAGE - n1;  // the free slots: [free0, free1)
            const uint32_t lo = n0 + (uint32_t)lane, hi = free1 - 1u - (uint32_t)lane;
            if (lane < 16 && lo < ((n0 + 15u) & ~15u) && lo < free1) s.sx[lo] = 3.0e38f;
            if (lane < 16 && (uint32_t)lane < (((n1 + 15u) & ~15u) - n1) && free1 >= free0 + 1u + (uint32_t)lane) s.sx[hi] = 3.0e38f;
          }
          __syncthreads();
          constexpr uint32_t G = 4;
          static_assert(BSTAGE % (G * LPB) == 0, "a lane reads four consecutive staged sub-beams with one b128 per component");
          // (wave-uniform trip count: the longer half; a lane whose own half is exhausted marks nothing -- the slots it
          // reads then hold the other half or an earlier window)
          const uint32_t nmax = max(n0, n1);
          const bool upper = pathSet && pixParity != 0u;
          const uint32_t nMine = upper ? n1 : n0;
          for (uint32_t jb = 0; jb < nmax; jb += G * LPB) {
            const uint32_t j0 = (upper ? (uint32_t)BSTAGE - (uint32_t)(G * LPB) - jb : jb) + (uint32_t)sub * G;
            uint32_t cm = 0;
            if (jb < nMine)
            {
              const float4 X = *reinterpret_cast<const float4 *>(&s.sx[j0]);
              const float4 Y = *reinterpret_cast<const float4 *>(&s.sy[j0]);
              const float4 Z = *reinterpret_cast<const float4 *>(&s.sz[j0]);
              const uint4 Ft = *reinterpret_cast<const uint4 *>(&s.stF[j0]);
              const v2fb ox = {base.o.x, base.o.x}, oy = {base.o.y, base.o.y}, oz = {base.o.z, base.o.z};
              const v2fb dx = {base.d.x, base.d.x}, dy = {base.d.y, base.d.y}, dz = {base.d.z, base.d.z};
              const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
              const uint32_t fs[4] = {Ft.x, Ft.y, Ft.z, Ft.w};
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const v2fb wx = (v2fb){xs[2 * h], xs[2 * h + 1]} - ox, wy = (v2fb){ys[2 * h], ys[2 * h + 1]} - oy,
                           wz = (v2fb){zs[2 * h], zs[2 * h + 1]} - oz;
                const v2fb disk = wx * dx + (wy * dy + wz * dz);
                const v2fb vx = wx - dx * disk, vy = wy - dy * disk, vz = wz - dz * disk;
                const v2fb d2 = vx * vx + (vy * vy + vz * vz);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                  const int u = 2 * h + e;
                  // conservative: sub-beam centre within (kernel radius + half sub-beam) of the ray segment; the
                  // beam's filter bits (contribution, checkerboard parity, depth) are tested here too: they halve
                  // the pairs that reach the ownership prefilter
                  uint32_t ok = (uint32_t)(d2[e] < thrD2) & (uint32_t)(disk[e] > thrLo) & (uint32_t)(disk[e] < thrHi);
                  ok &= (uint32_t)((fs[u] & fmask) == fwant);
                  if (maxDepth > 0) ok &= (uint32_t)((int)GVPM_PF_DEPTH(fs[u]) <= dmaxB);
                  cm |= ok << u;
                }
              }
            }
            // the survivors (a few per cent of the tests, scattered over the lanes) are compacted into a candidate
            // ring and go through the ownership prefilter 64 at a time, one per lane whatever ray they belong to:
            // resolved in place -- every lane looping over its own marks -- a round ran the ~100 instructions of
            // the prefilter for the one lane in ten that had a mark
#pragma unroll
            for (uint32_t u = 0; u < G; ++u) {
              const bool bit = (cm >> u) & 1u;
              const unsigned long long m = __ballot(bit);
              if (bit)
                s.candq[(cHead + cCount + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))) % BCQ] =
                    (uint16_t)((j0 + u) | ((uint32_t)b << 8));
              cCount += (uint32_t)__popcll(m);
            }
            while (cCount >= 64u) resolve(64u);
          }
          // the stage is about to be overwritten: the candidates that refer to it go first
          while (cCount) resolve(min(cCount, 64u));
        }
      }
    }
    __syncthreads();
    if (qCount) emit(qCount);
    __syncthreads();
  }
  for (; resLeft; --resLeft, resSlot += 64u) {
    if (resSlot + 64u <= pairCap) {
      pairs[resSlot + lane] = make_uint2(0xFFFFFFFFu, 0u);
      if (lane == 0) {
        blockKey[resSlot / 64u] = lastSet;
        blockVal[resSlot / 64u] = resSlot / 64u;
      }
    }
  }
  if (lane == 0 && nCand) atomicAdd(&statRow(a)[1], nCand);
#ifdef GVPM_TRAV_TIMING
  if (lane == 0 && blockIdx.x < 8192u) {
    gvpmBeamTravLog[4 * blockIdx.x] = tw0;
    gvpmBeamTravLog[4 * blockIdx.x + 1] = wall_clock64();
    gvpmBeamTravLog[4 * blockIdx.x + 2] = nIt;
    gvpmBeamTravLog[4 * blockIdx.x + 3] = nCand;
  }
#endif
}

// ---- evaluation, literal fp64 path (GVPM_BEAMS_FP64=1: the on-device cross-check) ------------------------------
// One pair per lane, blocks of 64 pairs of one tile.  The block's camera-beam sets (at most B consecutive sorted
// sets) are loaded into LDS, the lanes evaluate their pairs (evaluateBeam: the reference transcribed in fp64) into
// the block's LDS accumulators, and the touched accumulators go to the film with one global atomic each.
// The blocks arrive sorted by tile (radix sort of the block keys on the host side of the launch), and a wave takes
// RUN consecutive blocks at a time: the tile's rays are loaded, the accumulators zeroed and flushed once per tile
// and run instead of once per block (that bookkeeping was 3.2 of the kernel's 5.9 ms at the probe).
#ifndef GVPM_BEAMS_RUN  // (probe builds)
#define GVPM_BEAMS_RUN 256
#endif
#ifndef GVPM_BEAMS_RUN_MIN
#define GVPM_BEAMS_RUN_MIN 16
#endif
template <int B>
__global__ __launch_bounds__(64, 1) void evaluate_beams_exact_kernel(GatherArgs a, const uint2 *__restrict__ pairs,
                                                                     const uint32_t *__restrict__ sortedKey,
                                                                     const uint32_t *__restrict__ sortedBlock,
                                                                     uint32_t nBlocks, uint32_t *queueHead) {
  constexpr uint32_t RUN = GVPM_BEAMS_RUN, RUN_MIN = GVPM_BEAMS_RUN_MIN;
  __shared__ TileLds<B> s;
  const int lane = threadIdx.x;
  uint32_t nEval = 0, nNull = 0, nDiff = 0, nFail = 0;
  uint32_t curBase = 0xFFFFFFFFu, curNb = 0;
  auto flushTile = [&]() __attribute__((always_inline)) {
    __syncthreads();
    if (curBase != 0xFFFFFFFFu) {
      for (int idx = lane; idx < 27 * B; idx += 64) {
        const int k = idx / B, bb = idx % B;
        if ((uint32_t)bb < curNb) {
          const float v = (float)s.acc[k][bb];
          if (v != 0.f) {
            const uint32_t pv = s.pix[bb];
            const size_t p = (size_t)(pv >> 16) * a.cfg.width + (pv & 0xFFFFu);
            atomicAdd(&a.iter[p * 27 + k], v);
          }
        }
      }
    }
    __syncthreads();
  };
  // the first item of every wave is its own index; the shared counter (one address: ~11 ns per atomic whatever the
  // number of waves) serves the rest
  // (guided runs of blocks, as in evaluate_beams2_kernel below)
  bool firstItem = true;
  const uint32_t run0 = min(RUN, max(RUN_MIN, nBlocks / (4u * gridDim.x)));  // the first run of every wave is its own
  const uint32_t firstDyn = gridDim.x * run0;
  for (;;) {
    uint32_t b0 = blockIdx.x * run0, cnt = run0;
    if (!firstItem) {
      if (lane == 0) {
        const uint32_t seen = firstDyn + __hip_atomic_load(queueHead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t rem = seen < nBlocks ? nBlocks - seen : 0u;
        cnt = min(RUN, max(RUN_MIN, rem / (2u * gridDim.x)));
        b0 = firstDyn + atomicAdd(queueHead, cnt);
      }
      b0 = __shfl(b0, 0, 64);
      cnt = __shfl(cnt, 0, 64);
    }
    firstItem = false;
    if (b0 >= nBlocks) break;
    const uint32_t b1 = min(nBlocks, b0 + cnt);
    for (uint32_t bi = b0; bi < b1; ++bi) {
      const uint32_t setBase = sortedKey[bi];
      if (setBase != curBase) {
        flushTile();
        curBase = setBase;
        curNb = min((uint32_t)B, a.nsets - setBase);
        loadTileRays<B>(a, s, setBase, curNb, lane);
        for (int idx = lane; idx < 27 * B; idx += 64) (&s.acc[0][0])[idx] = 0.0;
        __syncthreads();
      }
      const uint2 e = pairs[(size_t)sortedBlock[bi] * 64u + lane];
      const bool live = e.x != 0xFFFFFFFFu && e.y >= setBase && e.y - setBase < curNb;
      if (live) {
        if (evaluateBeam<B>(a, s, e.x, e.y - setBase, nNull, nDiff, nFail)) nEval++;
      }
    }
    flushTile();
    curBase = 0xFFFFFFFFu;
  }
  {
    unsigned long long ev = nEval, nu = nNull, di = nDiff, fa = nFail;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ev += __shfl_xor(ev, o, 64);
      nu += __shfl_xor(nu, o, 64);
      di += __shfl_xor(di, o, 64);
      fa += __shfl_xor(fa, o, 64);
    }
    if (lane == 0 && ev) {
      atomicAdd(&statRow(a)[0], ev);
      atomicAdd(&statRow(a)[2], nu);
      atomicAdd(&statRow(a)[3], di);
      atomicAdd(&statRow(a)[4], fa);
    }
  }
}

// ---- the exact pass of G-Beams (round 5) ------------------------------------------------------------------------------------
// The shifts the fp32 evaluation could not decide (beamShift1 / beamShift2: a decision inside its band) were noted --
// {beam set, beam | sub << 24, GVPM_EX_KIND_BEAMS | shift << 8 | cause << 16} in a.exOvf -- and added nothing.  This kernel
// runs BEHIND the evaluation on the same stream, every gather (the beams' build is not pipelined: nothing the notes refer to
// has moved): a lane per note, the reference's statements in fp64 (evaluateBeam above with the triangle tests of the shadow
// segment in fp64 too), the shift's terms to the iteration's sums, its counter to the statistics.  A lane's rays and sums
// live in ITS column of a 64-wide tile.
__global__ __launch_bounds__(64) void exact_beams_kernel(GatherArgs a, unsigned long long *totals) {
  __shared__ TileLds<64> s;
  const int lane = threadIdx.x;
  const uint32_t total = *a.exOvfCount, n = min(total, a.exOvfCap);
  uint32_t nNull = 0, nDiff = 0, nFail = 0;
  for (uint32_t j0 = blockIdx.x * 64u; j0 < n; j0 += gridDim.x * 64u) {
    const uint32_t j = j0 + (uint32_t)lane;
    const bool have = j < n;
    const uint4 note = have ? a.exOvf[j] : make_uint4(0u, 0u, 0u, 0u);
    uint32_t pix = 0u;
    for (int k = 0; k < 5; ++k) {
      float4 q0 = make_float4(0.f, 0.f, 0.f, -1e-30f), q1 = make_float4(0.f, 0.f, 1.f, 0.f), q2 = make_float4(0.f, 0.f, 0.f, 0.f),
             q3 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (have) {
        const gvpm_camera_ray *ray = a.rays + (size_t)note.x * 5 + k;
        const float4 *rp = reinterpret_cast<const float4 *>(ray);
        q0 = rp[0]; q1 = rp[1]; q2 = rp[2]; q3 = rp[3];
        const float l = fabsf(q0.w);
        q0.w = GVPM_RAY_VALID(ray->info) != 0 ? l : -fmaxf(l, 1e-30f);  // (the valid bit rides on the sign of len, tile_walk.h)
      }
      s.ray4[k][0][lane] = q0;
      s.ray4[k][1][lane] = q1;
      s.ray4[k][2][lane] = q2;
      s.gop[k][lane] = q3.x;
      if (k == 0) {
        s.rnd[lane] = q3.z;
        s.pix[lane] = pix = __float_as_uint(q3.w);
        s.edge[lane] = GVPM_RAY_EDGE(__float_as_uint(q3.y));
      }
    }
    for (int k = 0; k < 27; ++k) s.acc[k][lane] = 0.0;
    __syncthreads();
    if (have) {
      if (totals) atomicAdd(&totals[4 + min((note.z >> 16) & 0xFFu, 15u)], 1ull);
      evaluateBeam<64, true>(a, s, note.y, (uint32_t)lane, nNull, nDiff, nFail, (int)((note.z >> 8) & 0xFFu));
      const size_t p = (size_t)(pix >> 16) * a.cfg.width + (pix & 0xFFFFu);
      for (int k = 3; k < 27; ++k) {
        const float v = (float)s.acc[k][lane];
        if (v != 0.f) atomicAdd(&a.iter[p * 27 + k], v);
      }
    }
    __syncthreads();
  }
  if (nNull) atomicAdd(&statRow(a)[2], (unsigned long long)nNull);
  if (nDiff) atomicAdd(&statRow(a)[3], (unsigned long long)nDiff);
  if (nFail) atomicAdd(&statRow(a)[4], (unsigned long long)nFail);
}
// the list is empty again; totals: {evaluated, lost, largest list} as exact_pass_kernel keeps them (exact_shift.hip)
__global__ void exact_beams_done_kernel(GatherArgs a, unsigned long long *totals) {
  const uint32_t total = *a.exOvfCount, n = min(total, a.exOvfCap);
  if (totals) {
    totals[0] += n;
    if (total > n) totals[1] += total - n;
    if (totals[2] < total) totals[2] = total;
  }
  if (total > n) atomicAdd(&a.stats[7], (unsigned long long)(total - n));  // dropped (gvpm_stats::dropped_pairs): gvpm_get_stats fails
  *a.exOvfCount = 0u;
}
void launch_exact_beams(const GatherArgs &a, unsigned long long *totals, hipStream_t stream) {
  // (a wave per workgroup, 37 KB of LDS each: four per CU resident; the empty ones leave at once)
  hipLaunchKernelGGL(exact_beams_kernel, dim3(2048), dim3(64), 0, stream, a, totals);
  hipLaunchKernelGGL(exact_beams_done_kernel, dim3(1), dim3(1), 0, stream, a, totals);
}

// ---- evaluation, fp32 path: two phases ----------------------------------------------------------------------------
// As above (blocks of 64 pairs sorted by tile, RUN blocks per reservation), but a block goes through phase 1 only
// (beamBase + beamShift1: kernel record, base contribution, null shifts); the reconnections it needs are appended to
// a wave-wide LDS ring (ballot + popcount; 40 bytes each) and run 64 at a time through phase 2 (beamShift2) whenever
// the ring holds a full wave of them, and completely before the tile's accumulators are flushed.
// The reconnections waiting for phase 2 and the ones the first round deferred share ONE pool of entries, as two stacks
// growing towards each other (the order of the reconnections is free: they only add to the accumulators): a block appends at
// most 4 x 64 to at most 63 that wait from the block before, and at most 63 deferred ones wait beside them -- 382; a drain moves
// entries from the lower stack to the upper one, never more.  (Until round 4 two rings of 320 + 128 entries: the 1.8 KB this
// saves are what takes the kernel from 7 to 8 resident waves per CU at B = 16.)
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

#ifdef GVPM_EVAL_TIMING
// probe builds only: per wave of the last launch, shader-clock ticks in [0] beamBase [1] beamShift1 + push [2] phase 2
// [3] tile change (flush, rays) [7] lifetime; [4] blocks [5] pairs alive after beamBase [6] reconnections
__device__ unsigned long long gvpmBeamsLog[8 * 16384];
extern "C" int gvpm_debug_beams_timing(unsigned long long *out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(gvpmBeamsLog), sizeof(gvpmBeamsLog)) == hipSuccess ? 0 : -1;
}
__device__ __forceinline__ unsigned long long beamsTick() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
  return t;
}
#define BTICK() beamsTick()
#else
#define BTICK() 0ull
#endif

template <int B, bool HS = false>
__global__ __launch_bounds__(64, B == 64 ? 1 : 2) void evaluate_beams2_kernel(GatherArgs a, const uint2 *__restrict__ pairs,
                                                                             const uint32_t *__restrict__ sortedKey,
                                                                             const uint32_t *__restrict__ sortedBlock,
                                                                             uint32_t nBlocks, uint32_t *queueHead) {
  constexpr uint32_t RUN = GVPM_BEAMS_RUN, RUN_MIN = GVPM_BEAMS_RUN_MIN;
  __shared__ BeamEvalLds<B> s;
  extern __shared__ float4 sceneTri[];  // occluders of a small scene (dynamic: 48 bytes each, none for larger scenes)
  const int lane = threadIdx.x;
  const float4 *ldsTri = nullptr;
  if (a.ntri <= BEAM_LDS_TRIS) {
    for (uint32_t i = lane; i < 3u * a.ntri; i += 64u) sceneTri[i] = a.tri4[i];
    ldsTri = sceneTri;
    __syncthreads();
  }
  uint32_t nEval = 0, nNull = 0, nDiff = 0, nFail = 0;
  uint32_t curBase = 0xFFFFFFFFu, curNb = 0;
  uint32_t qCount = 0;  // the lower stack of the pool, wave-uniform
  [[maybe_unused]] unsigned long long bt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  [[maybe_unused]] const unsigned long long btStart = BTICK();
  uint32_t vCount = 0;  // the deferred ones: the upper stack, wave-uniform
  auto drainVis = [&](uint32_t n) __attribute__((always_inline)) {  // n <= 64 deferred reconnections through the any-hit loop
    __syncthreads();
    if ((uint32_t)lane < n) {
      const uint32_t e = (uint32_t)BPOOL - vCount + (uint32_t)lane;  // the last n pushed
      BeamPQ q;
      q.id = s.qid[e];
      q.meta = s.qmeta[e];
      q.k = s.qk[e];
      q.u = s.qu[e];
      bool defer;
      beamShift2<B, HS>(a, s, q, ldsTri, true, defer, nDiff, nFail, curBase);
    }
    vCount -= n;
  };
  auto drain = [&](uint32_t n) __attribute__((always_inline)) {   // n <= 64 entries of the ring through phase 2 (first round)
    [[maybe_unused]] const unsigned long long d0 = BTICK();
    bt[6] += n;
    __syncthreads();
    bool defer = false;
    BeamPQ q = {};
    if ((uint32_t)lane < n) {
      const uint32_t e = qCount - n + (uint32_t)lane;  // the last n pushed
      q.id = s.qid[e];
      q.meta = s.qmeta[e];
      q.k = s.qk[e];
      q.u = s.qu[e];
      beamShift2<B, HS>(a, s, q, ldsTri, false, defer, nDiff, nFail, curBase);
    }
    qCount -= n;
    const unsigned long long dm = __ballot(defer);
    if (dm) {
      // (one wave per workgroup: every lane has read its entry before any lane pushes -- the upper stack may grow into the
      // slots just popped)
      if (defer) {
        const uint32_t slot = (uint32_t)BPOOL - 1u - vCount - (uint32_t)__popcll(dm & ((1ull << lane) - 1ull));
        s.qid[slot] = q.id;
        s.qmeta[slot] = q.meta;
        s.qk[slot] = q.k;
        s.qu[slot] = q.u;
      }
      vCount += (uint32_t)__popcll(dm);
      if (vCount >= 64u) drainVis(64u);
    }
    bt[2] += BTICK() - d0;
  };
  auto flushTile = [&]() __attribute__((always_inline)) {
    while (qCount) drain(min(qCount, 64u));
    while (vCount) drainVis(min(vCount, 64u));
    __syncthreads();
    if (curBase != 0xFFFFFFFFu) {
      for (int idx = lane; idx < 27 * B; idx += 64) {
        const int k = idx / B, bb = idx % B;
        if ((uint32_t)bb < curNb) {
          const float v = (float)s.acc[k][bb];
          if (v != 0.f) {
            const uint32_t pv = s.pix[bb];
            const size_t p = (size_t)(pv >> 16) * a.cfg.width + (pv & 0xFFFFu);
            atomicAdd(&a.iter[p * 27 + k], v);
          }
        }
      }
    }
    __syncthreads();
  };
  // Runs of blocks, guided: a run ends with the tile's flush (27 x B film atomics, the next tile's rays), so runs are long (at
  // C3 a tile has ~134 blocks: runs of 8 spent 11 % of the kernel in tile changes, 18.1 ms; runs of 32: 16.7; guided from 256
  // down to 16: 16.2) and shrink towards the end of the list, so that the waves still finish together.
  bool firstItem = true;
  const uint32_t run0 = min(RUN, max(RUN_MIN, nBlocks / (4u * gridDim.x)));  // the first run of every wave is its own
  const uint32_t firstDyn = gridDim.x * run0;
  for (;;) {
    uint32_t b0 = blockIdx.x * run0, cnt = run0;
    if (!firstItem) {
      if (lane == 0) {
        const uint32_t seen = firstDyn + __hip_atomic_load(queueHead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t rem = seen < nBlocks ? nBlocks - seen : 0u;
        cnt = min(RUN, max(RUN_MIN, rem / (2u * gridDim.x)));
        b0 = firstDyn + atomicAdd(queueHead, cnt);
      }
      b0 = __shfl(b0, 0, 64);
      cnt = __shfl(cnt, 0, 64);
    }
    // (wave-uniform, and said so: the run's bounds, the blocks' keys and the tile's base then live in scalar registers)
    b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
    cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt);
    firstItem = false;
    if (b0 >= nBlocks) break;
    const uint32_t b1 = min(nBlocks, b0 + cnt);
    for (uint32_t bi = b0; bi < b1; ++bi) {
      const uint32_t setBase = sortedKey[bi];
      [[maybe_unused]] const unsigned long long c0 = BTICK(), dr0 = bt[2];
      if (setBase != curBase) {
        flushTile();
        curBase = setBase;
        curNb = min((uint32_t)B, a.nsets - setBase);
        loadTileRays<B>(a, s, setBase, curNb, lane);
        for (int idx = lane; idx < 27 * B; idx += 64) (&s.acc[0][0])[idx] = 0.0;
        relToBase<B>(s, lane);
        __syncthreads();
      }
      [[maybe_unused]] const unsigned long long c1 = BTICK();
      bt[3] += (c1 - c0) - (bt[2] - dr0);
      const uint2 e = pairs[(size_t)sortedBlock[bi] * 64u + lane];
      const bool live = e.x != 0xFFFFFFFFu && e.y >= setBase && e.y - setBase < curNb;
      const uint32_t bIdx = e.y - setBase;
      BeamP1 st;
      const bool alive = live && beamBase<B>(a, s, e.x, bIdx, st);
      if (alive && st.st != 0xFFu) nEval++;  // (debugShift mismatch: base contribution kept, not an evaluation -- as the reference returns)
#ifdef GVPM_EVAL_TIMING
      asm volatile("" :: "v"((int)alive));
      const unsigned long long c2 = BTICK();
      bt[0] += c2 - c1;
      bt[4] += 1;
      bt[5] += (unsigned long long)__popcll(__ballot(alive));
#endif
      // (primal: the sppm integrator's beam pass -- BeamRadianceQuery, pm/beams.h:29-223 -- is the kernel record's base term
      // alone: no shifts.  cfg.reserved[5], set by gvpm_gather_primal's driver)
      const bool primal = a.cfg.reserved[5] != 0;
#pragma unroll 1
      for (int i = 0; i < 4; ++i) {
        bool rec = false;
        if (alive && !primal) beamShift1<B, HS>(a, s, st, bIdx, i, rec, nNull, nFail, setBase);
        const unsigned long long m = __ballot(rec);
        if (rec) {
          const uint32_t slot = qCount + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
          s.qid[slot] = st.id;
          s.qmeta[slot] = bIdx | ((uint32_t)i << 8);
          // base.eye * k.contrib * weightKernel * rr = (base.eye * flux * sigS) * (sc * weightKernel * rr): the scalar is carried
          s.qk[slot] = make_float4(st.k.tauV, st.k.sigmaW, st.k.pdfEdgeFailure * st.k.pdfKernel, st.k.sc * st.k.weightKernel * st.rr);
          s.qu[slot] = st.k.u;
        }
        qCount += (uint32_t)__popcll(m);
      }
#ifdef GVPM_EVAL_TIMING
      bt[1] += BTICK() - c2;
#endif
      while (qCount >= 64u) drain(64u);
    }
    {
      [[maybe_unused]] const unsigned long long f0 = BTICK(), dr0 = bt[2];
      flushTile();
      bt[3] += (BTICK() - f0) - (bt[2] - dr0);
    }
    curBase = 0xFFFFFFFFu;
  }
#ifdef GVPM_EVAL_TIMING
  bt[7] = BTICK() - btStart;
  if (lane == 0 && blockIdx.x < 16384u)
    for (int k = 0; k < 8; ++k) gvpmBeamsLog[8 * blockIdx.x + k] = bt[k];
#endif
  {
    unsigned long long ev = nEval, nu = nNull, di = nDiff, fa = nFail;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ev += __shfl_xor(ev, o, 64);
      nu += __shfl_xor(nu, o, 64);
      di += __shfl_xor(di, o, 64);
      fa += __shfl_xor(fa, o, 64);
    }
    if (lane == 0 && ev) {
      atomicAdd(&statRow(a)[0], ev);
      atomicAdd(&statRow(a)[2], nu);
      atomicAdd(&statRow(a)[3], di);
      atomicAdd(&statRow(a)[4], fa);
    }
  }
}

// ---- evaluation in TWO kernels (GVPM_BEAMS_SPLIT=1; experiment of round 4) ---------------------------------------------
// evaluate_beams2_kernel holds 253 VGPRs and 19.6 KB of LDS: 8 waves per CU, its vector unit ~65 % busy.  Alone, phase 1
// (kernel record, base term, null shifts) and phase 2 (reconnections) need fewer registers and far less LDS each, so each
// can run three waves per SIMD -- at the price of the reconnection entries going through HBM (28 bytes each, SoA) and of
// every tile being loaded and flushed twice.  Phase 1 works through guided runs of blocks as the fused kernel does; a run
// reserves room for its worst case (256 entries a block) with one atomic, appends densely, and leaves {first block, blocks,
// first entry} in a run table and the entries of every block in blkCnt[]; phase 2 takes the runs one at a time and walks
// their tile segments 64 entries at a time.
struct SplitQ {
  uint32_t *id, *meta;  // BeamPQ::id, ::meta
  float4 *k;
  float *u;
  uint32_t *blkCnt;     // entries of block bi (sorted block order)
  uint4 *runTab;        // {first block, blocks, first entry, -}
  uint32_t *ctl;        // [0] entry cursor [1] runs [2] phase 2's queue head
};
template <int B> struct BeamP1Lds : RayTile<B> {
  double acc[27][B];
};
template <int B> struct BeamP2Lds : RayTile<B> {
  double acc[27][B];
  uint32_t vid[128], vmeta[128];
  float4 vk[128];
  float vu[128];
};

#ifndef GVPM_SPLIT_P1_MINW
#define GVPM_SPLIT_P1_MINW 3
#endif
#ifndef GVPM_SPLIT_P2_MINW
#define GVPM_SPLIT_P2_MINW 3
#endif
template <int B>
__global__ __launch_bounds__(64, GVPM_SPLIT_P1_MINW) void evaluate_beams_p1_kernel(GatherArgs a, SplitQ sq, const uint2 *__restrict__ pairs,
                                                                  const uint32_t *__restrict__ sortedKey,
                                                                  const uint32_t *__restrict__ sortedBlock, uint32_t nBlocks,
                                                                  uint32_t *queueHead) {
  constexpr uint32_t RUN = GVPM_BEAMS_RUN, RUN_MIN = GVPM_BEAMS_RUN_MIN;
  __shared__ BeamP1Lds<B> s;
  const int lane = threadIdx.x;
  uint32_t nEval = 0, nNull = 0, nFail = 0;
  uint32_t curBase = 0xFFFFFFFFu, curNb = 0;
  auto flushTile = [&]() __attribute__((always_inline)) {
    __syncthreads();
    if (curBase != 0xFFFFFFFFu) {
      for (int idx = lane; idx < 27 * B; idx += 64) {
        const int k = idx / B, bb = idx % B;
        if ((uint32_t)bb < curNb) {
          const float v = (float)s.acc[k][bb];
          if (v != 0.f) {
            const uint32_t pv = s.pix[bb];
            const size_t p = (size_t)(pv >> 16) * a.cfg.width + (pv & 0xFFFFu);
            atomicAdd(&a.iter[p * 27 + k], v);
          }
        }
      }
    }
    __syncthreads();
  };
  bool firstItem = true;
  const uint32_t run0 = min(RUN, max(RUN_MIN, nBlocks / (4u * gridDim.x)));
  const uint32_t firstDyn = gridDim.x * run0;
  for (;;) {
    uint32_t b0 = blockIdx.x * run0, cnt = run0;
    if (!firstItem) {
      if (lane == 0) {
        const uint32_t seen = firstDyn + __hip_atomic_load(queueHead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t rem = seen < nBlocks ? nBlocks - seen : 0u;
        cnt = min(RUN, max(RUN_MIN, rem / (2u * gridDim.x)));
        b0 = firstDyn + atomicAdd(queueHead, cnt);
      }
      b0 = __shfl(b0, 0, 64);
      cnt = __shfl(cnt, 0, 64);
    }
    firstItem = false;
    if (b0 >= nBlocks) break;
    const uint32_t b1 = min(nBlocks, b0 + cnt);
    // room for the run's worst case, and its row of the run table
    uint32_t eBase = 0;
    if (lane == 0) {
      eBase = atomicAdd(&sq.ctl[0], (b1 - b0) * 256u);
      const uint32_t r = atomicAdd(&sq.ctl[1], 1u);
      sq.runTab[r] = make_uint4(b0, b1 - b0, eBase, 0u);
    }
    eBase = __shfl(eBase, 0, 64);
    uint32_t eCount = 0;  // entries of the run so far (wave-uniform)
    for (uint32_t bi = b0; bi < b1; ++bi) {
      const uint32_t setBase = sortedKey[bi];
      if (setBase != curBase) {
        flushTile();
        curBase = setBase;
        curNb = min((uint32_t)B, a.nsets - setBase);
        loadTileRays<B>(a, s, setBase, curNb, lane);
        for (int idx = lane; idx < 27 * B; idx += 64) (&s.acc[0][0])[idx] = 0.0;
        relToBase<B>(s, lane);
        __syncthreads();
      }
      const uint2 e = pairs[(size_t)sortedBlock[bi] * 64u + lane];
      const bool live = e.x != 0xFFFFFFFFu && e.y >= setBase && e.y - setBase < curNb;
      const uint32_t bIdx = e.y - setBase;
      BeamP1 st;
      const bool alive = live && beamBase<B>(a, s, e.x, bIdx, st);
      if (alive && st.st != 0xFFu) nEval++;
      const bool primal = a.cfg.reserved[5] != 0;
      const uint32_t eBlock = eCount;
#pragma unroll 1
      for (int i = 0; i < 4; ++i) {
        bool rec = false;
        if (alive && !primal) beamShift1<B, false>(a, s, st, bIdx, i, rec, nNull, nFail, setBase);
        const unsigned long long m = __ballot(rec);
        if (rec) {
          const size_t slot = (size_t)eBase + eCount + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
          sq.id[slot] = st.id;
          sq.meta[slot] = bIdx | ((uint32_t)i << 8);
          sq.k[slot] = make_float4(st.k.tauV, st.k.sigmaW, st.k.pdfEdgeFailure * st.k.pdfKernel, st.k.sc * st.k.weightKernel * st.rr);
          sq.u[slot] = st.k.u;
        }
        eCount += (uint32_t)__popcll(m);
      }
      if (lane == 0) sq.blkCnt[bi] = eCount - eBlock;
    }
    flushTile();
    curBase = 0xFFFFFFFFu;
  }
  {
    unsigned long long ev = nEval, nu = nNull, fa = nFail;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ev += __shfl_xor(ev, o, 64);
      nu += __shfl_xor(nu, o, 64);
      fa += __shfl_xor(fa, o, 64);
    }
    if (lane == 0 && ev) {
      atomicAdd(&statRow(a)[0], ev);
      atomicAdd(&statRow(a)[2], nu);
      atomicAdd(&statRow(a)[4], fa);
    }
  }
}

template <int B>
__global__ __launch_bounds__(64, GVPM_SPLIT_P2_MINW) void evaluate_beams_p2_kernel(GatherArgs a, SplitQ sq, const uint32_t *__restrict__ sortedKey) {
  __shared__ BeamP2Lds<B> s;
  extern __shared__ float4 sceneTri[];
  const int lane = threadIdx.x;
  const float4 *ldsTri = nullptr;
  if (a.ntri <= BEAM_LDS_TRIS) {
    for (uint32_t i = lane; i < 3u * a.ntri; i += 64u) sceneTri[i] = a.tri4[i];
    ldsTri = sceneTri;
    __syncthreads();
  }
  const uint32_t nRuns = sq.ctl[1];
  uint32_t nDiff = 0, nFail = 0;
  uint32_t curBase = 0xFFFFFFFFu, curNb = 0;
  uint32_t vHead = 0, vCount = 0;  // the deferred ring, wave-uniform
  auto drainVis = [&](uint32_t n) __attribute__((always_inline)) {
    __syncthreads();
    if ((uint32_t)lane < n) {
      const uint32_t e = (vHead + (uint32_t)lane) & 127u;
      BeamPQ q;
      q.id = s.vid[e];
      q.meta = s.vmeta[e];
      q.k = s.vk[e];
      q.u = s.vu[e];
      bool defer;
      beamShift2<B, false>(a, s, q, ldsTri, true, defer, nDiff, nFail, curBase);
    }
    vHead = (vHead + n) & 127u;
    vCount -= n;
  };
  auto flushTile = [&]() __attribute__((always_inline)) {
    while (vCount) drainVis(min(vCount, 64u));
    __syncthreads();
    if (curBase != 0xFFFFFFFFu) {
      for (int idx = lane; idx < 27 * B; idx += 64) {
        const int k = idx / B, bb = idx % B;
        if ((uint32_t)bb < curNb) {
          const float v = (float)s.acc[k][bb];
          if (v != 0.f) {
            const uint32_t pv = s.pix[bb];
            const size_t p = (size_t)(pv >> 16) * a.cfg.width + (pv & 0xFFFFu);
            atomicAdd(&a.iter[p * 27 + k], v);
          }
        }
      }
    }
    __syncthreads();
  };
  bool firstItem = true;
  for (;;) {
    uint32_t r = blockIdx.x;
    if (!firstItem) {
      if (lane == 0) r = gridDim.x + atomicAdd(&sq.ctl[2], 1u);
      r = __shfl(r, 0, 64);
    }
    firstItem = false;
    if (r >= nRuns) break;
    const uint4 run = sq.runTab[r];
    uint32_t ePos = run.z;  // the next block's first entry
    uint32_t bi = run.x;
    const uint32_t bEnd = run.x + run.y;
    while (bi < bEnd) {
      // the tile segment: consecutive blocks of one tile, their entries laid end to end
      const uint32_t setBase = sortedKey[bi];
      const uint32_t segBeg = ePos;
      while (bi < bEnd && sortedKey[bi] == setBase) ePos += sq.blkCnt[bi++];
      if (ePos == segBeg) continue;
      if (setBase != curBase) {
        flushTile();
        curBase = setBase;
        curNb = min((uint32_t)B, a.nsets - setBase);
        loadTileRays<B>(a, s, setBase, curNb, lane);
        for (int idx = lane; idx < 27 * B; idx += 64) (&s.acc[0][0])[idx] = 0.0;
        relToBase<B>(s, lane);
        __syncthreads();
      }
      for (uint32_t e0 = segBeg; e0 < ePos; e0 += 64u) {
        const uint32_t n = min(64u, ePos - e0);
        __syncthreads();
        bool defer = false;
        BeamPQ q = {};
        if ((uint32_t)lane < n) {
          const size_t e = (size_t)e0 + lane;
          q.id = sq.id[e];
          q.meta = sq.meta[e];
          q.k = sq.k[e];
          q.u = sq.u[e];
          beamShift2<B, false>(a, s, q, ldsTri, false, defer, nDiff, nFail, curBase);
        }
        const unsigned long long dm = __ballot(defer);
        if (dm) {
          if (defer) {
            const uint32_t slot = (vHead + vCount + (uint32_t)__popcll(dm & ((1ull << lane) - 1ull))) & 127u;
            s.vid[slot] = q.id;
            s.vmeta[slot] = q.meta;
            s.vk[slot] = q.k;
            s.vu[slot] = q.u;
          }
          vCount += (uint32_t)__popcll(dm);
          if (vCount >= 64u) drainVis(64u);
        }
      }
    }
    flushTile();
    curBase = 0xFFFFFFFFu;
  }
  {
    unsigned long long di = nDiff, fa = nFail;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      di += __shfl_xor(di, o, 64);
      fa += __shfl_xor(fa, o, 64);
    }
    if (lane == 0 && (di | fa)) {
      atomicAdd(&statRow(a)[3], di);
      atomicAdd(&statRow(a)[4], fa);
    }
  }
}

// (B = 16 only: the tile size every launch of the product uses; the fused kernel serves the others)
void launch_evaluate_beams_split(const GatherArgs &a, uint32_t *qId, uint32_t *qMeta, float4 *qK, float *qU, uint32_t *blkCnt,
                                 uint4 *runTab, uint32_t *ctl, const uint2 *pairs, const uint32_t *sortedKey,
                                 const uint32_t *sortedBlock, uint32_t nBlocks, uint32_t *queueHead, uint32_t ncu,
                                 hipStream_t stream) {
  if (a.nsets == 0 || nBlocks == 0) return;
  SplitQ sq{qId, qMeta, qK, qU, blkCnt, runTab, ctl};
  const uint32_t nw = ncu * 4u * GVPM_SPLIT_P1_MINW, nw2 = ncu * 4u * GVPM_SPLIT_P2_MINW;
  hipLaunchKernelGGL((evaluate_beams_p1_kernel<16>), dim3(nw), dim3(64), 0, stream, a, sq, pairs, sortedKey, sortedBlock, nBlocks,
                     queueHead);
  const size_t dyn = a.ntri <= BEAM_LDS_TRIS ? (size_t)a.ntri * 48u : 0u;
  hipLaunchKernelGGL((evaluate_beams_p2_kernel<16>), dim3(nw2), dim3(64), dyn, stream, a, sq, sortedKey);
}

void launch_traverse_beams(const GatherArgs &a, const uint32_t *hotFlags, int beamsPerWave, const uint4 *items,
                           const uint32_t *itemCount, uint32_t itemCap, uint32_t *queueHead, uint2 *pairs, uint32_t *pairCount,
                           uint32_t pairCap, uint32_t *blockKey, uint32_t *blockVal, uint32_t nwaves, hipStream_t stream) {
  if (a.nsets == 0) return;
  switch (beamsPerWave) {
    case 64: hipLaunchKernelGGL(traverse_beams_kernel<64>, dim3(nwaves), dim3(64), 0, stream, a, hotFlags, items, itemCount, itemCap, queueHead, pairs, pairCount, pairCap, blockKey, blockVal); break;
    case 32: hipLaunchKernelGGL(traverse_beams_kernel<32>, dim3(nwaves), dim3(64), 0, stream, a, hotFlags, items, itemCount, itemCap, queueHead, pairs, pairCount, pairCap, blockKey, blockVal); break;
    default: hipLaunchKernelGGL(traverse_beams_kernel<16>, dim3(nwaves), dim3(64), 0, stream, a, hotFlags, items, itemCount, itemCap, queueHead, pairs, pairCount, pairCap, blockKey, blockVal); break;
  }
}

void launch_evaluate_beams(const GatherArgs &a, int beamsPerWave, bool exact, const uint2 *pairs, const uint32_t *sortedKey,
                           const uint32_t *sortedBlock, uint32_t nBlocks, uint32_t *queueHead, uint32_t nwaves,
                           hipStream_t stream) {
  if (a.nsets == 0 || nBlocks == 0) return;
#define GVPM_LAUNCH_BEAMS(BB) \
  hipLaunchKernelGGL((evaluate_beams_exact_kernel<BB>), dim3(nwaves), dim3(64), 0, stream, a, pairs, sortedKey, sortedBlock, \
                     nBlocks, queueHead)
  if (exact) {
    switch (beamsPerWave) {
      case 64: GVPM_LAUNCH_BEAMS(64); break;
      case 32: GVPM_LAUNCH_BEAMS(32); break;
      default: GVPM_LAUNCH_BEAMS(16); break;
    }
  } else if (a.reqHost) {
    // manifold-typed shifts go to the host's request list (an instantiation of its own: the default keeps its registers)
    const size_t dyn = a.ntri <= BEAM_LDS_TRIS ? (size_t)a.ntri * 48u : 0u;
    switch (beamsPerWave) {
      case 64: hipLaunchKernelGGL((evaluate_beams2_kernel<64, true>), dim3(nwaves), dim3(64), dyn, stream, a, pairs, sortedKey, sortedBlock, nBlocks, queueHead); break;
      case 32: hipLaunchKernelGGL((evaluate_beams2_kernel<32, true>), dim3(nwaves), dim3(64), dyn, stream, a, pairs, sortedKey, sortedBlock, nBlocks, queueHead); break;
      default: hipLaunchKernelGGL((evaluate_beams2_kernel<16, true>), dim3(nwaves), dim3(64), dyn, stream, a, pairs, sortedKey, sortedBlock, nBlocks, queueHead); break;
    }
  } else {
    const size_t dyn = a.ntri <= BEAM_LDS_TRIS ? (size_t)a.ntri * 48u : 0u;
    switch (beamsPerWave) {
      case 64: hipLaunchKernelGGL((evaluate_beams2_kernel<64>), dim3(nwaves), dim3(64), dyn, stream, a, pairs, sortedKey, sortedBlock, nBlocks, queueHead); break;
      case 32: hipLaunchKernelGGL((evaluate_beams2_kernel<32>), dim3(nwaves), dim3(64), dyn, stream, a, pairs, sortedKey, sortedBlock, nBlocks, queueHead); break;
      default: hipLaunchKernelGGL((evaluate_beams2_kernel<16>), dim3(nwaves), dim3(64), dyn, stream, a, pairs, sortedKey, sortedBlock, nBlocks, queueHead); break;
    }
  }
#undef GVPM_LAUNCH_BEAMS
}

// ---- grid build helpers for sub-beams ------------------------------------------------------
// counts[i] = number of sub-beams of beam i; maxLs = longest sub-beam (float bits, atomicMax)
__global__ __launch_bounds__(256) void beam_subcount_kernel(const float *__restrict__ p2, const float *__restrict__ p1,
                                                            uint32_t n, float ls, uint32_t *counts, uint32_t *maxLs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  float sub = 0.f;
  if (i < n) {
    const double dx = (double)p2[3 * (size_t)i] - (double)p1[3 * (size_t)i];
    const double dy = (double)p2[3 * (size_t)i + 1] - (double)p1[3 * (size_t)i + 1];
    const double dz = (double)p2[3 * (size_t)i + 2] - (double)p1[3 * (size_t)i + 2];
    const float len = (float)sqrt(dx * dx + dy * dy + dz * dz);
    const uint32_t c = subBeamCount(len, ls);
    counts[i] = c;
    sub = len / (float)c;
  }
  sub = wave_max(sub);
  // (one address: atomics on it retire ~11 ns apart -- 31 k waves of them were 0.34 of this kernel's 0.36 ms -- so a wave
  // first looks whether it would raise the maximum at all)
  if ((threadIdx.x & 63) == 0 && __float_as_uint(sub) > __hip_atomic_load(maxLs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(maxLs, __float_as_uint(sub));
}

// for every sub-beam j = offsets[beam] + sub: keys[j] = the grid cell of its centre, vals[j] = beam | sub << 24 -- the pair
// the sort takes (until round 4: centres and ids written here, a key kernel over the centres, the sort carrying indices and
// sub_hot_kernel gathering ids[order[j]]: 16 bytes a sub-beam more traffic and one dependent gather more).
// A wave expands 64 beams TOGETHER: their sub-beams laid end to end, consecutive lanes take consecutive ones (the beam an
// element belongs to: a 6-step search over the wave's exclusive scan), so the stores are whole lines -- a lane looping over
// its own beam's ~12 sub-beams wrote 64 scattered pieces per instruction (0.25 ms at C3 for 0.2 GB).
__global__ __launch_bounds__(256) void beam_expand_kernel(const float *__restrict__ p2, const float *__restrict__ p1,
                                                          uint32_t n, const uint32_t *__restrict__ counts,
                                                          const uint32_t *__restrict__ offsets, Grid g, uint32_t *keys,
                                                          uint32_t *vals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool have = i < n;
  const uint32_t c = have ? counts[i] : 0u, o = have ? offsets[i] : 0u;
  const f3 a = have ? mk3(p1[3 * (size_t)i], p1[3 * (size_t)i + 1], p1[3 * (size_t)i + 2]) : mk3(0.f);
  const f3 b = have ? mk3(p2[3 * (size_t)i], p2[3 * (size_t)i + 1], p2[3 * (size_t)i + 2]) : mk3(0.f);
  const uint32_t incl = wave_scan_incl(c, lane), excl = incl - c;
  const uint32_t total = __shfl(incl, 63, 64);
  const uint32_t base = __shfl(o, 0, 64);  // (offsets are the exclusive scan of counts: the wave's elements are contiguous)
  for (uint32_t e0 = 0; e0 < total; e0 += 64u) {
    const uint32_t e = e0 + (uint32_t)lane;
    uint32_t r = 0;
#pragma unroll
    for (uint32_t step = 32; step; step >>= 1) {
      const uint32_t cand = r + step;
      const uint32_t v = (uint32_t)__shfl((int)excl, (int)(cand & 63u), 64);
      if (cand < 64u && v <= e) r = cand;
    }
    const uint32_t rc = (uint32_t)__shfl((int)c, (int)r, 64), rx = (uint32_t)__shfl((int)excl, (int)r, 64);
    const f3 ra = mk3(__shfl(a.x, (int)r, 64), __shfl(a.y, (int)r, 64), __shfl(a.z, (int)r, 64));
    const f3 rb = mk3(__shfl(b.x, (int)r, 64), __shfl(b.y, (int)r, 64), __shfl(b.z, (int)r, 64));
    if (e < total) {
      const uint32_t k = e - rx;
      const float t = ((float)k + 0.5f) / (float)rc;
      const f3 m = ra + (rb - ra) * t;
      const int cx = cellCoord(m.x, g.org[0], g.invCell, g.dim[0]);
      const int cy = cellCoord(m.y, g.org[1], g.invCell, g.dim[1]);
      const int cz = cellCoord(m.z, g.org[2], g.invCell, g.dim[2]);
      keys[base + e] = ((uint32_t)cz * g.dim[1] + cy) * g.dim[0] + cx;
      vals[base + e] = (blockIdx.x * blockDim.x + (threadIdx.x & ~63u) + r) | (k << 24);
    }
  }
}

// sorted sub-beam records for the traversal: {centre, beam | sub << 24} {beam direction, sub-beam length} and the
// beam's filter bits (cold word 7.w: contribution, parity, depth).  The length is the evaluation's (fp64 norm
// rounded to float), so that sub-beam ranges agree.
__global__ __launch_bounds__(256) void sub_hot_kernel(const uint32_t *__restrict__ sortedIds, uint32_t n,
                                                      const float4 *__restrict__ aux, float4 *hot, uint32_t *hotFlags) {
  // (the two quads of a record go through LDS: consecutive lanes then write consecutive quads -- whole lines -- instead
  // of every lane its two halves of a 32-byte record)
  __shared__ float4 stg[256][2];
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = threadIdx.x;
  if (j < n) {
    const uint32_t id = sortedIds[j], beam = id & 0xFFFFFFu, sub = id >> 24;
    // {p1, bits} {direction, sub-beam length} of the beam (beam_cold_kernel): one 32-byte gather; the centre is computed,
    // not gathered (to a few ulp the one beam_expand_kernel binned: every test downstream carries a margin)
    const float4 a0 = aux[2 * (size_t)beam], a1 = aux[2 * (size_t)beam + 1];
    const float tt = a1.w * ((float)sub + 0.5f);
    stg[t][0] = make_float4(a0.x + a1.x * tt, a0.y + a1.y * tt, a0.z + a1.z * tt, __uint_as_float(id));
    stg[t][1] = a1;
    hotFlags[j] = __float_as_uint(a0.w);
  }
  __syncthreads();
  const size_t base = 2 * (size_t)blockIdx.x * blockDim.x;
  const float4 *flat = &stg[0][0];
#pragma unroll
  for (int e = t; e < 512; e += 256)
    if (base + (size_t)e < 2 * (size_t)n) hot[base + e] = flat[e];
}

void launch_beam_subcount(const float *p2, const float *p1, uint32_t n, float ls, uint32_t *counts, uint32_t *maxLs,
                          hipStream_t s) {
  hipLaunchKernelGGL(beam_subcount_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p2, p1, n, ls, counts, maxLs);
}
void launch_beam_expand(const float *p2, const float *p1, uint32_t n, const uint32_t *counts, const uint32_t *offsets,
                        const Grid &g, uint32_t *keys, uint32_t *vals, hipStream_t s) {
  hipLaunchKernelGGL(beam_expand_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p2, p1, n, counts, offsets, g, keys, vals);
}
void launch_sub_hot(const uint32_t *sortedIds, uint32_t n, const float4 *aux, float4 *hot, uint32_t *hotFlags, hipStream_t s) {
  hipLaunchKernelGGL(sub_hot_kernel, dim3((n + 255) / 256), dim3(256), 0, s, sortedIds, n, aux, hot, hotFlags);
}

}  // namespace gvpm
