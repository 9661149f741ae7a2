// The evaluation of the G-BRE gather (gather_bre.hip: the execution model, the planner and the traversal that writes the pair
// lists this unit reads): evaluate_bre_kernel / evaluate_bre_mix_kernel in all their forms, their helpers and their launcher.
//
// A translation unit of its own because it is built with other flags than the rest of the library (Makefile:
// -fno-slp-vectorize).  The SLP vectoriser packs this kernel's scalar fp32 arithmetic into v_pk_* operations whose operands
// must sit in aligned register pairs: a fifth of the vector instructions were the moves that marshal them, and the pairs
// cost the spills (NOTEBOOK.md round 22).  The traversal's packed test is hand-written and keeps its flags.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "device_types.h"
#include "gather_bre_common.h"
#include "shift_device.h"
#include "tile_walk.h"
#include "vec.h"

namespace gvpm {

// coordinateSystemCoherent, src/libcore/util.cpp:592-599 (its intermediates are float)
__device__ __forceinline__ void coherentFrame(f3 n, f3 &b1, f3 &b2) {
  const float sign = copysignf(1.0f, n.z);
  const float aa = -frcp(sign + n.z);
  const float bb = n.x * n.y * aa;
  b1 = mk3(1.0f + sign * n.x * n.x * aa, sign * bb, -sign * n.x);
  b2 = mk3(bb, sign + n.y * n.y * aa, -n.y);
}

// One evaluation = VolumeGradientBREQuery::operator() after the filters, in two phases so that
// the expensive, divergent part runs on full waves:
//   phase 1 (one lane per (photon, beam) pair): base contribution, then for each of the four
//     shifted rays the null shift if it applies (cheap); a shift that needs the offset-path
//     reconnection is only QUEUED (2 bytes: step, lane, shift, beam);
//   phase 2 (one lane per queued shift): the diffuse reconnection with its shadow ray, Jacobian
//     and MIS weight, in a dense loop of its own (see the kernel).
// At C2 ~70 % of the shifts are null shifts: running both branches on every lane of a mixed
// wave cost ~1.5x the VALU work of this arrangement.
//
// Accumulation: LDS float atomics (ds_add_f32) retire about one lane per clock on CDNA4 -- 24 of
// them per evaluation were half of this kernel's time.  The traversal therefore writes one photon
// list PER BEAM, the evaluation wave cuts the concatenated lists of an item into 64 equal chunks
// (perfect balance) and every lane sums its 27 outputs in REGISTERS; a lane touches the LDS
// accumulators (double: ds_add_f64 runs ~25x the rate of ds_add_f32, scripts/probes/lds_atomics_bench.hip)
// only when its chunk crosses into the next beam and at the end of a segment.
//
// Numerics: every quantity that the reference obtains by subtracting O(1) positions to get an
// O(radius) vector (photon - ray point, shifted ray point - base ray point) is formed in fp64 and
// then carried as a small fp32 vector; everything downstream of those differences (kernel chord
// lengths sqrt(r^2 - d^2), pdfs, BSDF / phase / transmittance products, MIS weights) is fp32.

// The hit decision of one (photon, beam) candidate: gvpm_accel.h:279-301 (disk, distSqr, own box) and, for the
// 3D kernel, the validity of the resampled t' (shift_volume_photon.cpp:707-726).  Decided in fp32 when the error
// band (hitBand, ownBoxBand: gather_bre_common.h) cannot change the reference's decision.
// Returns 1 (hit), 0 (no hit) or 2: the band cannot decide -- about one candidate in 10^5 at C2, plus the photons
// that project beyond the beam's end when the own-box test cannot decide those either.
// (CFG: the compile-time configuration, shift_device.h -- where it fixes the kernel, the argument is not read)
template <typename CFG = EvalCfgGeneric>
__device__ __forceinline__ int decidePair(f3 pos, const RayReg &base, float rnd, float r, float eps, bool use3DCfg) {
  const bool use3D = cfgFlag<CFG::FIXED, CFG::USE3D>(use3DCfg);
  const float r2f = r * r, mint = eps, maxt = base.len - eps;
  const f3 wv = pos - base.o;
  const float disk = dot(wv, base.d);
  const f3 v = wv - base.d * disk;
  const float d2 = dot(v, v);
  float E, band;
  hitBand(wv, disk, r, r2f, E, band);
  bool in0 = d2 < r2f - band && disk > mint + E && disk < maxt - E;
  // surely outside: beyond the band of the disk test (the own-box test can only remove more)
  bool outside = d2 > r2f + band || disk < mint - E;
  if (!outside && disk >= maxt - E && d2 < r2f - band) {
    // at or beyond the beam's end: the own-box test decides (round 5: with bands, here, instead of in fp64 later)
    const int bx = ownBoxBand(pos, base.o, base.d, r, mint, maxt);
    in0 = bx == 1;
    outside = bx == 0;
  }
  bool in = in0;
  if (use3D) {
    // t' = (disk - deltaT) + 2 deltaT rnd must lie in [mint, len]: bracket it with deltaT in [dTlo, dTup]
    const float q = r2f - d2;
    const float dTup = fsqrt(fmaxf(q + band, 0.f)) * 1.000001f, dTlo = fsqrt(fmaxf(q - band, 0.f)) * 0.999999f;
    const float slop = 2.f * E + 4e-7f * (fabsf(disk) + dTup);
    const float tLo = (disk - dTup) + 2.f * dTlo * rnd - slop;
    const float tHi = (disk - dTlo) + 2.f * dTup * rnd + slop;
    in = in0 && tLo > mint && tHi < base.len;
    outside = outside || (in0 && (tHi < mint || tLo > base.len));
  }
  return in ? 1 : (outside ? 0 : 2);
}
// The same decision for a candidate the bands above left open -- almost all of them at the RIM of the kernel: the band of d2
// is 4 r E with E the rounding of O(1) coordinate differences, 1e-3 of r^2 -- with the difference vector and the projection
// formed in fp64, as baseTerms forms them, and the perpendicular offset as a small fp32 vector: d2 to ~4e-7 relative, disk
// and t' to ~1e-15.  What is still inside THAT band (~1e-6 of the candidates) goes to the exact pass.
template <typename CFG = EvalCfgGeneric>
__device__ __forceinline__ int decidePairFine(f3 pos, const RayReg &base, float rnd, float r, float eps, bool use3DCfg) {
  const bool use3D = cfgFlag<CFG::FIXED, CFG::USE3D>(use3DCfg);
  const d3 wD = tod(pos) - tod(base.o), bdD = tod(base.d);
  const double disk = dot(wD, bdD);
  const f3 perp = tof(wD - bdD * disk);
  const float d2 = dot(perp, perp), r2f = r * r;
  const float band = 2e-6f * r2f;
  const double mint = (double)eps, maxt = (double)base.len - (double)eps, tE = 1e-12 * (1.0 + fabs(disk));
  bool in0 = d2 < r2f - band && disk > mint + tE && disk < maxt - tE;
  bool outside = d2 > r2f + band || disk < mint - tE;
  if (!outside && disk >= maxt - tE && d2 < r2f - band) {
    const int bx = ownBoxBand(pos, base.o, base.d, r, eps, base.len - eps);
    in0 = bx == 1;
    outside = bx == 0;
  }
  bool in = in0;
  if (use3D) {
    const float q = r2f - d2;
    const double dTup = (double)(fsqrt(fmaxf(q + band, 0.f)) * 1.000001f), dTlo = (double)(fsqrt(fmaxf(q - band, 0.f)) * 0.999999f);
    const double tLo = (disk - dTup) + 2.0 * dTlo * (double)rnd - tE, tHi = (disk - dTlo) + 2.0 * dTup * (double)rnd + tE;
    in = in0 && tLo > mint && tHi < (double)base.len;
    outside = outside || (in0 && (tHi < mint || tLo > (double)base.len));
  }
  return in ? 1 : (outside ? 0 : 2);
}

// the 27 per-beam outputs of one lane, in registers
struct Acc27 {
  float v[27];
};

struct BaseTerms {
  f3 rel;  // photon - baseRay(t')
  double tPrime;
  float pdfCam, scale, tr;  // tr: transmittance over [Epsilon, t'] (equal in the three channels)
  f3 bc;                    // base contribution * scale
};

// hit geometry + base contribution of a (photon, beam) pair, shift_volume_photon.cpp:701-751
template <int B, typename CFG = EvalCfgGeneric, typename LDS>
__device__ __forceinline__ BaseTerms baseTerms(const GatherArgs &a, const LDS &s, f3 pos, f3 wi, f3 flux,
                                               const RayReg &base, uint32_t b) {
  BaseTerms t;
  const bool use3D = cfgFlag<CFG::FIXED, CFG::USE3D>(a.cfg.vol_technique == GVPM_VOL_BRE3D);
  const float r = a.radius, r2 = r * r;
  // gvpm_accel.h:296-299: disk in fp64, the perpendicular offset as a small vector
  const d3 wD = tod(pos) - tod(base.o), bdD = tod(base.d);
  const double disk = dot(wD, bdD);
  const f3 perp = tof(wD - bdD * disk);
  const float distSqr = dot(perp, perp);
  t.tPrime = disk;
  float kernelVol = 3.14159265358979323846f * r2;
  t.pdfCam = 1.f;
  if (use3D) {
    // shift_volume_photon.cpp:707-726
    const float deltaT = fsqrt(fmaxf(0.f, r2 - distSqr));
    t.tPrime = (disk - (double)deltaT) + (double)(2.f * deltaT * s.rnd[b]);
    kernelVol = (4.0f / 3.0f) * 3.14159265358979323846f * r2 * r;
    t.pdfCam = frcp(fmaxf(deltaT * 2.f, 0.0001f));
  }
  t.rel = perp + base.d * (float)(disk - t.tPrime);
  const float rr = cfgFlag<CFG::FIXED, CFG::PATH_SET>(a.cfg.path_set) ? 2.f : 1.f;
  t.scale = rr * frcp(kernelVol * t.pdfCam);
  // the base and the four shifted rays all carry mint = Epsilon and maxt = t' (:769-770): one transmittance
  f3 trT;
  float dummy;
  mediumEval(a.med, (float)t.tPrime - a.cfg.epsilon, trT, dummy);
  t.tr = trT.x;
  const f3 sigS = mk3(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]);
  t.bc = (sigS * flux) * (t.tr * phaseEval(a.med.g, wi, -base.d) * t.scale) * base.eye;
  return t;
}

// phase 1: base contribution + the four shift attempts of one pair; reconnections are returned in qMask
// (HS: manifold-typed shifts are recorded for the host, gvpm_enable_host_shifts -- its own instantiation of the kernel)
// A shift whose branch fp32 cannot decide as the reference does (round 5) -- the null-shift test |z' - y|^2 < r^2 or t'
// against the shifted edge's length within the error band of the fp32 quantities (branchAmbiguous) -- adds nothing and
// counts nothing here: it is QUEUED like a reconnection, and phase 2, which re-derives the test from the same numbers,
// hands it to the exact pass (one deferral site in the kernel: its copy loops cost registers).
template <typename CFG = EvalCfgGeneric>
__device__ __forceinline__ bool branchAmbiguous(const GatherArgs &a, float y2, float r2, float tPf, float shLen) {
  // y is good to ~2e-7 |y| (the two differences are formed in fp64 / as exact fp32 differences), t' to half an ulp
  // (cfg.reserved[4]: GVPM_EXACT_ALL -- the band widened to everything, so that the exact pass evaluates EVERY shift: a test
  // of the pass against the oracle on whole frames, tests/test_exact_pass_gpu.py)
  if (cfgFlag<CFG::FIXED, CFG::EXACT_ALL>(a.cfg.reserved[4])) return true;
  return (cfgFlag<CFG::FIXED, CFG::SHIFT_NULL>(a.cfg.use_shift_null) && fabsf(y2 - r2) <= 4e-6f * r2) || fabsf(tPf - shLen) <= 4e-7f * (tPf + shLen);
}
template <int B, bool HS, typename CFG = EvalCfgGeneric, typename LDS>
__device__ __forceinline__ void evalPhase1(const GatherArgs &a, LDS &s, const PhotonFront &ph, const RayReg &base,
                                           uint32_t b, Acc27 &acc, uint32_t &nNull, uint32_t &nFail, uint32_t &qMask) {
  const uint32_t pix = s.pix[b];
  const float r2 = a.radius * a.radius;
  const BaseTerms bt = baseTerms<B, CFG>(a, s, ph.pos, ph.wi, ph.flux, base, b);
  const f3 bc = bt.bc;
  acc.v[0] += bc.x;
  acc.v[1] += bc.y;
  acc.v[2] += bc.z;
  qMask = 0u;

  const f3 photonIn = mk3(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]) * ph.flux;
  const float tPf = (float)bt.tPrime;
  const uint32_t st = GVPM_PF_SHIFT_TYPE(ph.bits);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // branch-free: the null-shift arithmetic is cheap and some lane of the wave needs it anyway; a wave
    // spends more on exec-mask bookkeeping and taken branches than on the arithmetic they would skip
    // the shifted ray RELATIVE to the base ray (relToBase, tile_walk.h): shiftRay(t') - baseRay(t') = relO + relD t' is a
    // small fp32 vector (pixel spacing at depth t'), accurate to ~1e-10; the sensorMIS factor rides along
    const ShiftRel sh = loadShiftRel(s, i, b, base.d);
    // photon relative to shiftRay(t') = (photon - baseRay(t')) - (shiftRay(t') - baseRay(t'))
    const f3 y = bt.rel - (sh.ro + sh.rd * tPf);
    // shiftNull, shift_volume_photon.cpp:119-158 with the kernel pdfs of :782-801
    const float y2 = dot(y, y);
    const bool ambBranch = sh.valid && !(HS && st == 3u) && branchAmbiguous<CFG>(a, y2, r2, tPf, sh.len);
    const bool isNull = !ambBranch && sh.valid && cfgFlag<CFG::FIXED, CFG::SHIFT_NULL>(a.cfg.use_shift_null) && y2 < r2 && tPf < sh.len;
    const f3 yp = y - sh.d * dot(y, sh.d);
    const float deltaS = fsqrt(fmaxf(0.f, r2 - dot(yp, yp)));
    const float pdfShiftPos = frcp(fmaxf(2.f * deltaS, 0.0001f));
    float wNull = 0.5f;
    if (cfgFlag<CFG::FIXED, CFG::USE_MIS>(a.cfg.use_mis))
      wNull = (pdfShiftPos == 0.f || bt.pdfCam == 0.f)
                  ? 1.f
                  : frcp(1.f + sh.sMIS * pdfShiftPos * frcp(bt.pdfCam));
    const f3 nullFlux = photonIn * (bt.tr * phaseEval(a.med.g, ph.wi, -sh.d)) * sh.eye;
    // shiftPhoton dispatch, shift_volume_photon.cpp:49-117: reconnections go to phase 2
    const bool wantsShift = !ambBranch && sh.valid && !isNull && sh.len >= tPf &&
                            !cfgFlag<CFG::FIXED, CFG::DEBUG_SHIFT_NULL>(a.cfg.debug_shift == GVPM_SHIFT_NULL);
    // (a manifold-typed photon goes to phase 2 as well when the host answers such shifts: it records the request there)
    const bool queued = wantsShift && (st == 1u || st == 2u || (HS && st == 3u));
    nNull += isNull ? 1u : 0u;
    nFail += (wantsShift && !queued) ? 1u : 0u;
    qMask |= (queued || ambBranch) ? (1u << i) : 0u;
    float w = isNull ? wNull : 1.f;
    borderRule(a, pix, i, w);
    const float keep = (queued || ambBranch) ? 0.f : 1.f;  // a queued / deferred shift adds nothing here
    const float ws = isNull ? w * bt.scale : 0.f;  // only the null shift has a shifted flux in phase 1
    acc.v[3 + 3 * i + 0] += nullFlux.x * ws;
    acc.v[3 + 3 * i + 1] += nullFlux.y * ws;
    acc.v[3 + 3 * i + 2] += nullFlux.z * ws;
    acc.v[15 + 3 * i + 0] += bc.x * (w * keep);
    acc.v[15 + 3 * i + 1] += bc.y * (w * keep);
    acc.v[15 + 3 * i + 2] += bc.z * (w * keep);
  }
}

// phase 2: one queued reconnection shift (shiftPhotonDiffuse through getShiftPos); the result goes to
// the lane's registers when it belongs to the lane's current beam, else straight to the LDS accumulators
template <int B, bool FULLVIS, bool HS, bool MIX, typename CFG = EvalCfgGeneric, typename LDS>
__device__ __forceinline__ void evalPhase2Core(const GatherArgs &a, LDS &s, uint32_t pidx, uint32_t b, int i, f3 &sf,
                                               f3 &wb, uint32_t &nDiff, uint32_t &nFail, const float4 *ldsTri) {
  const PhotonCold ph = loadCold(a, pidx);
  const RayReg base = loadRay(s, 0, b);
  const ShiftRel sr = loadShiftRel(s, i, b, base.d);
  RayReg sh;  // what the reconnection reads of the shifted ray: direction, eye contribution
  sh.d = sr.d;
  sh.eye = sr.eye;
  sh.len = sr.len;
  sh.valid = sr.valid;
  const bool use3D = cfgFlag<CFG::FIXED, CFG::USE3D>(a.cfg.vol_technique == GVPM_VOL_BRE3D);
  const bool useShiftNull = cfgFlag<CFG::FIXED, CFG::SHIFT_NULL>(a.cfg.use_shift_null);
  const float r = a.radius, r2 = r * r;
  // t', pdfCameraPos and the photon relative to baseRay(t') exactly as phase 1 derived them (baseTerms)
  double tPrime;
  float pdfCam = 1.f;
  f3 rel;
  {
    const d3 wD = tod(ph.pos) - tod(base.o), bdD = tod(base.d);
    const double disk = dot(wD, bdD);
    const f3 perp = tof(wD - bdD * disk);
    tPrime = disk;
    if (use3D) {
      const float deltaT = fsqrt(fmaxf(0.f, r2 - dot(perp, perp)));
      tPrime = (disk - (double)deltaT) + (double)(2.f * deltaT * s.rnd[b]);
      pdfCam = frcp(fmaxf(deltaT * 2.f, 0.0001f));
    }
    rel = perp + base.d * (float)(disk - tPrime);
  }
  const float rr = cfgFlag<CFG::FIXED, CFG::PATH_SET>(a.cfg.path_set) ? 2.f : 1.f;
  const float kernelVol = use3D ? (4.0f / 3.0f) * 3.14159265358979323846f * r2 * r : 3.14159265358979323846f * r2;
  const float scale = rr * frcp(kernelVol * pdfCam);
  f3 trT;
  float dummy;
  mediumEval(a.med, (float)tPrime - a.cfg.epsilon, trT, dummy);
  const f3 sigS = mk3(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]);
  const f3 bc = (sigS * ph.flux) * (trT.x * phaseEval(a.med.g, ph.wi, -base.d) * scale) * base.eye;

  const f3 basePt = base.o + base.d * (float)tPrime;  // baseRay(t'), absolute (for the segment to the parent)
  const f3 dS = sr.ro + sr.rd * (float)tPrime;  // shiftRay(t') - baseRay(t')
  // phase 1's branch test from phase 1's numbers (evalPhase1): an undecidable branch was queued to be deferred here
  uint32_t amb = 0u;
  if (!(HS && GVPM_PF_SHIFT_TYPE(ph.bits) == 3u)) {
    const f3 y = rel - dS;
    const float y2 = dot(y, y), tPf = (float)tPrime;
    amb = branchAmbiguous<CFG>(a, y2, r2, tPf, sh.len) ? 2u : 0u;
    //  Phase 1 queues a shift for two reasons -- it IS a reconnection, or its branch is undecidable -- and
    // tells phase 2 neither: the test above is re-derived from the same numbers.  Should the two sites ever round differently,
    // an entry that is neither here -- not ambiguous, yet a null shift, a photon type without a reconnection, or a shifted edge
    // too short -- was queued as undecidable there: it goes to the exact pass, it is not evaluated as a reconnection.
    const uint32_t stq = GVPM_PF_SHIFT_TYPE(ph.bits);
    const bool nullNow = useShiftNull && y2 < r2 && tPf < sh.len;
    const bool reconnects = sh.valid && !nullNow && sh.len >= tPf &&
                            !cfgFlag<CFG::FIXED, CFG::DEBUG_SHIFT_NULL>(a.cfg.debug_shift == GVPM_SHIFT_NULL) && (stq == 1u || stq == 2u);
    if (!amb && !reconnects) amb = 2u;
  }
  // getShiftPos, shift_volume_photon.cpp:858-896: offsetPos = shiftRay(t') + offRel
  f3 offRel = rel;
  if (!use3D) {
    f3 bs, bt, ns, nt;
    coherentFrame(base.d, bs, bt);
    coherentFrame(sh.d, ns, nt);
    offRel = ns * dot(rel, bs) + nt * dot(rel, bt) + sh.d * dot(rel, base.d);
  }
  if (useShiftNull) {
    const f3 bo = dS + offRel;       // offsetPos - baseRay(t')
    const float bo2 = dot(bo, bo);
    // (the mirror decision of getShiftPos moves the offset position by up to 2 r: not a counter, but a different shift)
    amb |= fabsf(bo2 - r2) <= (use3D ? 4e-6f : 2e-5f) * r2 ? 8u : 0u;
    const float cosD2 = bo2 < r2 ? -2.f * dot(dS, offRel) * frcp(dot(dS, dS)) : 0.f;
    offRel = offRel + dS * cosD2;
  }
  float pdfShiftPos = 1.f;
  if (use3D) {
    const f3 op = offRel - sh.d * dot(offRel, sh.d);
    const float deltaO = fsqrt(fmaxf(0.f, r2 - dot(op, op)));
    pdfShiftPos = frcp(fmaxf(2.f * deltaO, 0.0001f));
  }
  if (HS && GVPM_PF_SHIFT_TYPE(ph.bits) == 3u) {
    // EManifoldShift: the walk is the host's (recordShiftRequest); nothing is added now
    const f3 shiftPt = basePt + dS;
    if (recordShiftRequest(reqSink(a), a.radius, pidx, a.setPerm[s.setBase + b], i, shiftPt + offRel, basePt, shiftPt, (float)tPrime, trT.x, pdfCam,
                           pdfShiftPos, sr.sMIS, scale, bc, sh.d, sh.eye, s.pix[b])) {
      sf = wb = mk3(0.f);
    } else {
      nFail++;
      sf = mk3(0.f);
      wb = bc;  // weight 1
    }
    return;
  }
  bool ok = false;
  f3 sflux;
  // offsetPos - parent is a difference of two ABSOLUTE positions: baseRay(t') - parent is formed from the difference of the
  // two fp32 origins (one rounding, relative to the DIFFERENCE), never through the fp32 point basePt, whose rounding is half an
  // ulp of a COORDINATE -- 1e-7 of the unit room, but 1e-4 of a reconnection 2000 units from the origin: the film's L2 at
  // 1.4e-4 and two cosine tests at a Phong wall decided differently (found by the `far` transform, tests/test_similarity_gpu.py)
  const f3 dProjU = (((base.o - ph.parentPos) + base.d * (float)tPrime) + dS) + offRel;
  uint32_t ambVis = 0u;
  float w = shiftDiffuse<FULLVIS, MIX, CFG>(a, ph, ph.bits, dProjU, sh, base, s.edge[b], trT, pdfCam, pdfShiftPos, sflux, ok, ldsTri,
                                 sr.sMIS, &ambVis);
  if (amb | ambVis) {
    // fp32 cannot decide this shift as the reference does: the exact pass evaluates it (nothing added, nothing counted)
    deferNote(a, GVPM_EX_KIND_BRE, a.setPerm[s.setBase + b], pidx, (uint32_t)i, amb | ambVis);
    sf = wb = mk3(0.f);
    return;
  }
  if (ok) nDiff++; else nFail++;
  borderRule(a, s.pix[b], i, w);
  const float ws = w * scale;
  sf = sflux * ws;
  wb = bc * w;
}

// a lane's register sums -> the LDS accumulators of `beam`
template <int B, typename LDS> __device__ __forceinline__ void flushAcc(LDS &s, Acc27 &acc, uint32_t beam) {
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    atomicAdd(&s.acc[k][beam], (double)(acc.v[k]));
    acc.v[k] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------
// evaluation: persistent waves, one item at a time, the two phases in SEPARATE loops.
//
// A wave walks a SEGMENT of its item's pairs through the decision + phase 1 only (<= SEG_STEPS steps, or until
// the queue could overflow), appending the reconnections it meets to ONE compact queue (ballot + popcount, 2 bytes
// per entry: step, lane, shift, beam), folds its register sums into the LDS accumulators, and then runs the queue
// through phase 2 in a dense loop of its own: every lane takes an equal, contiguous share of the queue, whose
// entries come in runs of one (beam, shift), so a lane keeps 6 sums in registers and touches the LDS accumulators
// once per run.  (Round 1 interleaved the reconnections with the phase-1 walk: the 27 register sums of phase 1
// stayed live across phase 2, the allocation was the union of both -- 187 VGPRs, two waves per SIMD -- and each
// wave held per-lane queues of 4 KB.)  Here the allocation is the larger of the two loops, the queue is a quarter
// of the size, and the 4 waves of a workgroup share the staged occluders: 12 KB of LDS per wave, 3 waves per SIMD.
// Measured at C2 (MI355X, isolated): 1.09 -> 0.78 ms.
// ------------------------------------------------------------------------------------------
constexpr int SEG_STEPS = 16;   // steps per segment (4 bits of a queue entry)
constexpr int SEG_QCAP = 1024;  // queue entries per wave; a step appends at most 4 * 64
template <int B> struct SegCfg {
  // waves per workgroup: they share nothing but the staged occluders
  static constexpr int WPB = B == 16 ? 4 : (B == 32 ? 2 : 1);
  using Entry = typename std::conditional<B == 16, uint16_t, uint32_t>::type;
  static constexpr int BEAM_BITS = B == 16 ? 4 : 6;
};
template <int B> struct SegLds : RayTile<B> {
  double acc[27][B];
  uint32_t boff[B + 1];
  typename SegCfg<B>::Entry q[SEG_QCAP];  // step | lane | shift | beam
  uint32_t setBase;                       // of the item (host-shift requests name the beam set)
  // (the shifted rays are kept RELATIVE to their base ray in the ray tile's own slots, with sensorMIS: relToBase)
};

#ifdef GVPM_EVAL_TIMING
// probe builds only: shader-clock ticks per part of the evaluation kernel, summed over waves
// [0] wave lifetime [1] item header + LDS setup [2] decision + phase 1 [3] phase 2 [4] late pass bookkeeping [5] write-out [6] items
__device__ unsigned long long gvpmEvalTiming[16];  // [12] longest wave [13] longest item [14] waves
// wall clock (100 MHz, the same on every XCD) at the start and the end of every wave of the LAST launch, and its units
__device__ unsigned long long gvpmEvalWaveLog[16 * 16384];
extern "C" int gvpm_debug_eval_timing(unsigned long long *out, int reset) {
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(gvpmEvalTiming), sizeof(gvpmEvalTiming)) != hipSuccess) return -1;
  if (out && hipMemcpyFromSymbol(out + 16, HIP_SYMBOL(gvpmEvalWaveLog), sizeof(gvpmEvalWaveLog)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(gvpmEvalTiming), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
__device__ __forceinline__ unsigned long long tickNow() {
  unsigned long long t;
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
  return t;
}
#define TICK() tickNow()
__device__ __forceinline__ unsigned long long tickLight() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
  return t;
}
#define LTICK() tickLight()
#else
#define TICK() 0ull
#define LTICK() 0ull
#endif

// evaluate_bre_kernel, and evaluate_bre_mix_kernel for a BSDF table that holds mixture heads: the mixture arm inlined into
// evaluate_bre_kernel cost the kernel of a plain benchmark run 8 more spilled VGPRs and 24 bytes of scratch per lane, in whatever
// form and place (NOTEBOOK.md, "Mixture parents"), so that kernel stays as it was and scenes with such walls run the other one.
#define GVPM_EVAL_KERNEL evaluate_bre_kernel
#define GVPM_EVAL_MIX false
#include "gather_bre_eval.inc"
#undef GVPM_EVAL_KERNEL
#undef GVPM_EVAL_MIX
#define GVPM_EVAL_KERNEL evaluate_bre_mix_kernel
#define GVPM_EVAL_MIX true
#include "gather_bre_eval.inc"
#undef GVPM_EVAL_KERNEL
#undef GVPM_EVAL_MIX

uint32_t eval_unit_pairs() { return EVAL_UNIT; }

// The configuration EvalCfgHeadline<!FULLVIS> fixes (shift_device.h), and nothing else: a handle whose gvpm_params differ in any
// flag the specialised kernel no longer reads runs the generic one, as does GVPM_EVAL_GENERIC=1 (gvpm_api.hip).
template <bool FULLVIS> static bool headlineConfig(const GatherArgs &a) {
  using C = EvalCfgHeadline<!FULLVIS>;
  const auto &c = a.cfg;
  return !(c.reserved[0] & GVPM_EVAL_FORCE_GENERIC) && (c.vol_technique == GVPM_VOL_BRE3D) == C::USE3D &&
         (c.use_shift_null != 0) == C::SHIFT_NULL && c.debug_shift == GVPM_SHIFT_ALL && (c.reserved[4] != 0) == C::EXACT_ALL &&
         (c.path_set != 0) == C::PATH_SET && (c.use_mis != 0) == C::USE_MIS && (c.power_heuristic != 0) == C::POWER_HEURISTIC &&
         (!C::VIS_FIXED || (c.visibility_as_written != 0) == C::VIS_AS_WRITTEN);
}

template <bool FULLVIS, bool PF, bool HS = false>
static void launchEvaluate(const GatherArgs &a, int beamsPerWave, const uint4 *items, const uint2 *itemOff,
                           const uint32_t *itemCount, uint32_t *queueHead, const uint32_t *pairs, const uint32_t *pairCnt,
                           uint32_t nwaves, bool persistent, hipStream_t stream, const uint2 *units, const uint32_t *unitCtl,
                           uint32_t unitCap) {
  const uint32_t persist = persistent ? 1u : 0u;
  const size_t dyn = (!FULLVIS && a.ntri <= EVAL_LDS_TRIS && !(a.cfg.reserved[0] & 16)) ? (size_t)a.ntri * 48u : 0u;
  // (a table with mixture heads: the kernel that evaluates them; the bit is set where the arguments are filled, gather_drivers.hip)
  const bool mix = (a.cfg.reserved[0] & GVPM_TABLE_HAS_MIXTURE) != 0;
#define GVPM_LAUNCH_EVAL_B(BB)                                                                                                             \
  do {                                                                                                                                     \
    const dim3 grid((nwaves + SegCfg<BB>::WPB - 1) / SegCfg<BB>::WPB), block(64 * SegCfg<BB>::WPB);                                        \
    if (mix)                                                                                                                               \
      hipLaunchKernelGGL((evaluate_bre_mix_kernel<BB, FULLVIS, PF, HS>), grid, block, dyn, stream, a, items, itemOff, itemCount, queueHead, \
                         pairs, pairCnt, persist, units, unitCtl, unitCap);                                                                \
    else                                                                                                                                   \
      hipLaunchKernelGGL((evaluate_bre_kernel<BB, FULLVIS, PF, HS>), grid, block, dyn, stream, a, items, itemOff, itemCount, queueHead,     \
                         pairs, pairCnt, persist, units, unitCtl, unitCap);                                                                \
  } while (0)
  switch (beamsPerWave) {
    case 64: GVPM_LAUNCH_EVAL_B(64); break;
    case 32: GVPM_LAUNCH_EVAL_B(32); break;
    default:
      if constexpr (!PF && !HS) {
        // the specialised instantiations: B = 16 without the record prefetch and without host shifts
        if (headlineConfig<FULLVIS>(a)) {
          using C = EvalCfgHeadline<!FULLVIS>;
          const dim3 grid((nwaves + SegCfg<16>::WPB - 1) / SegCfg<16>::WPB), block(64 * SegCfg<16>::WPB);
          if (mix)
            hipLaunchKernelGGL((evaluate_bre_mix_kernel<16, FULLVIS, false, false, C>), grid, block, dyn, stream, a, items, itemOff, itemCount,
                               queueHead, pairs, pairCnt, persist, units, unitCtl, unitCap);
          else
            hipLaunchKernelGGL((evaluate_bre_kernel<16, FULLVIS, false, false, C>), grid, block, dyn, stream, a, items, itemOff, itemCount,
                               queueHead, pairs, pairCnt, persist, units, unitCtl, unitCap);
          break;
        }
      }
      GVPM_LAUNCH_EVAL_B(16);
      break;
  }
#undef GVPM_LAUNCH_EVAL_B
}

// fullVis: shadow rays walk the occluder BVH (intended visibility, > 254 occluders, near-list overflow)
void launch_evaluate_bre(const GatherArgs &a, int beamsPerWave, bool fullVis, const uint4 *items, const uint2 *itemOff,
                         const uint32_t *itemCount, uint32_t *queueHead, const uint32_t *pairs, const uint32_t *pairCnt,
                         uint32_t nwaves, bool persistent, hipStream_t stream, const uint2 *units, const uint32_t *unitCtl,
                         uint32_t unitCap) {
  if (!persistent) units = nullptr;  // (one item per wave: the grid is the item count)
  if (a.nsets == 0 || nwaves == 0) return;
  // the record prefetch of phase 1 pays when the records (128 bytes each) no longer fit the 256 MB Infinity Cache: measured
  // +5 % on a rank's step at C4 (4 M photons), -1 % at C2 (1 M).  GVPM_RECORD_PREFETCH=0/1 (cfg.reserved[0] bits 5, 6) forces it.
  const bool pf = (a.cfg.reserved[0] & 32) ? false : ((a.cfg.reserved[0] & 64) ? true : (size_t)a.nph * 128u > ((size_t)256 << 20));
#define GVPM_LAUNCH_EVAL(FV, P) \
  launchEvaluate<FV, P>(a, beamsPerWave, items, itemOff, itemCount, queueHead, pairs, pairCnt, nwaves, persistent, stream, units, unitCtl, unitCap)
  if (a.reqHost) {
    // manifold-typed shifts go to the host's request list (no record prefetch variant of these)
    if (fullVis) launchEvaluate<true, false, true>(a, beamsPerWave, items, itemOff, itemCount, queueHead, pairs, pairCnt, nwaves, persistent, stream, units, unitCtl, unitCap);
    else launchEvaluate<false, false, true>(a, beamsPerWave, items, itemOff, itemCount, queueHead, pairs, pairCnt, nwaves, persistent, stream, units, unitCtl, unitCap);
  } else if (fullVis) {
    if (pf) GVPM_LAUNCH_EVAL(true, true);
    else GVPM_LAUNCH_EVAL(true, false);
  } else {
    if (pf) GVPM_LAUNCH_EVAL(false, true);
    else GVPM_LAUNCH_EVAL(false, false);
  }
#undef GVPM_LAUNCH_EVAL
}

}  // namespace gvpm
