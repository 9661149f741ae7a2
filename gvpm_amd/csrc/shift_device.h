// Device helpers shared by the gather kernels: the closed-form pieces of the shift
// (phase / medium / reconnection / MIS) -- see gather_bre.hip for the citations.  The occluder tests live in occlusion.h,
// the BSDF models of a glossy surface parent in parent_bsdf.h.
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "occlusion.h"
#include "parent_bsdf.h"
#include "vec.h"

namespace gvpm {

struct RayReg {
  f3 o, d, eye;
  float len, pdf, jac, gop;
  bool valid;
};

// g == 0: the isotropic plugin's constant (src/phase/isotropic.cpp:76-78) -- the formula returns 1/4pi exactly there too,
// but g is wave-uniform wherever it is the medium's: a scalar branch instead of a dot product, a square root and a
// reciprocal per call (six calls an evaluation; C2: -1 % on the step)
__device__ __forceinline__ float phaseEval(float g, f3 wi, f3 wo) {
  if (g == 0.f) return INV_FOURPI_F;
  const float temp = 1.0f + g * g + 2.0f * g * dot(wi, wo);
  return INV_FOURPI_F * (1.f - g * g) * frcp(temp * fsqrt(temp));
}

// HomogeneousMedium::eval over a distance (balance strategy)
// (sigma_t is equal across channels -- homogeneous.cpp:196-200, enforced by gvpm_upload_medium --
// so the three channel exponentials are one)
__device__ __forceinline__ void mediumEval(const MediumDev &m, float dist, f3 &tr, float &pdfSuccess) {
  float e = __expf(-m.sigmaT[0] * dist);
  pdfSuccess = m.sigmaT[0] * e * m.msw;
  if (e < 1e-20f) e = 0.f;
  tr = mk3(e);
}

// ---- deferral to the exact pass (device_types.h, ExEntry) ----
// the hot loops' side: one global atomic and one 16-byte store per deferred shift (rare)
__device__ __forceinline__ void deferNote(const GatherArgs &a, uint32_t kind, uint32_t set, uint32_t recIdx, uint32_t shift, uint32_t cause) {
  const uint32_t slot = atomicAdd(a.exOvfCount, 1u);
  if (slot < a.exOvfCap) a.exOvf[slot] = make_uint4(set, recIdx, kind | (shift << 8) | (cause << 16), 0u);
}
// one quad of an entry: 0 header, 1..8 the record, 9..28 the five rays, 29 per technique, 30..31 zero
__device__ __forceinline__ float4 exQuad(const GatherArgs &a, uint32_t set, uint32_t recIdx, uint32_t meta, uint32_t part) {
  float outScale = a.iterScale, radius = a.radius;
  float4 extra = make_float4(0.f, 0.f, 0.f, 0.f);
  if ((meta & 0xFFu) == GVPM_EX_KIND_VPM) {
    // G-VPM notes name the camera SAMPLE: its beam set, its random number and selection pdf, the pixel's own radius
    // (querySize = R * POURCENTAGE_BS * gp.scaleVol, gvpm.cpp:1082,1132 -- read before this iteration's update)
    const gvpm_vpm_sample sm = a.samples[set];
    set = sm.set;
    const uint32_t pix = a.rays[(size_t)set * 5].pixel;
    const float scaleVol = a.scaleVol[(size_t)(pix >> 16) * a.cfg.width + (pix & 0xFFFFu)];
    radius = (a.cfg.bsphere_radius * 0.01f) * scaleVol;
    outScale = 1.f / (float)a.cfg.nb_camera_samples;
    extra = make_float4(sm.rand, sm.pdf_sel, scaleVol, 0.f);  // (the pixel's scale itself: the pass forms the radius in double)
  }
  if (part == 0u) return make_float4(__uint_as_float(meta), 0.f, outScale, radius);
  if (part <= GVPM_REC_QUADS) return a.cold[(size_t)recIdx * GVPM_REC_QUADS + (part - 1u)];
  if (part <= GVPM_REC_QUADS + 20u) return reinterpret_cast<const float4 *>(a.rays + (size_t)set * 5)[part - 1u - GVPM_REC_QUADS];
  if (part == GVPM_REC_QUADS + 21u) return extra;
  return make_float4(0.f, 0.f, 0.f, 0.f);
}

// GatherPoint::sensorMIS, gvpm_struct.h:608-631 (sDist == bDist for BRE: same t')
__device__ __forceinline__ float sensorMIS(const RayReg &s, const RayReg &b, uint32_t edge) {
  float jacobian = s.jac;
  float ratio = fdiv(s.pdf, b.pdf);
  if (edge != 1u) {
    jacobian *= fdiv(s.gop, b.gop);
    ratio *= fdiv(b.gop, s.gop);
  }
  return ratio * jacobian;
}

struct PhotonCold {
  f3 pos, wi, flux, parentPos, parentN, prefixW, parentScat, parentWi;
  float parentPdf, edgePdf, parentRR, parentG;
  uint32_t bits;
  uint32_t nl0, nl1, nl2;  // up to 12 occluder indices near the parent (0xFF = none); top byte of nl0 0xFE: overflow
};

// the front of the record: all the base contribution and the null shifts need
struct PhotonFront {
  f3 pos, wi, flux;
  uint32_t bits;
};
__device__ __forceinline__ PhotonFront loadFront(const GatherArgs &a, uint32_t idx) {
  PhotonFront c;
  const float4 *rec = a.cold + (size_t)idx * GVPM_REC_QUADS;
  const float4 c0 = rec[0], c1 = rec[1], c2 = rec[2];
  c.pos = mk3(c0.x, c0.y, c0.z); c.bits = __float_as_uint(c0.w);
  c.wi = mk3(c1.x, c1.y, c1.z);
  c.flux = mk3(c2.x, c2.y, c2.z);
  return c;
}

// the photon's 128-byte record (one cache line)
__device__ __forceinline__ PhotonCold loadCold(const GatherArgs &a, uint32_t idx) {
  PhotonCold c;
  const float4 *rec = a.cold + (size_t)idx * GVPM_REC_QUADS;
  const float4 c0 = rec[0], c1 = rec[1], c2 = rec[2], c3 = rec[3], c4 = rec[4], c5 = rec[5], c6 = rec[6], c7 = rec[7];
  c.pos = mk3(c0.x, c0.y, c0.z); c.bits = __float_as_uint(c0.w);
  c.wi = mk3(c1.x, c1.y, c1.z); c.parentPdf = c1.w;
  c.flux = mk3(c2.x, c2.y, c2.z); c.edgePdf = c2.w;
  c.parentPos = mk3(c3.x, c3.y, c3.z); c.parentRR = c3.w;
  c.parentN = mk3(c4.x, c4.y, c4.z); c.parentG = c4.w;
  c.prefixW = mk3(c5.x, c5.y, c5.z);
  c.nl0 = __float_as_uint(c5.w);
  c.parentScat = mk3(c6.x, c6.y, c6.z);
  c.nl1 = __float_as_uint(c6.w);
  c.parentWi = mk3(c7.x, c7.y, c7.z);
  c.nl2 = __float_as_uint(c7.w);
  return c;
}

// A compile-time view of the integrator configuration (gvpm_params: fixed at gvpm_create) for the G-BRE evaluation kernel and the
// helpers it calls.  FIXED = false: every flag is read from a.cfg where it is used.  FIXED = true: the flags are the constants
// below and the other side of every test on them is not compiled -- its code counts toward a kernel's register allocation and
// its uniform compares and selects sit in the hot loops ("Specialised evaluation").
struct EvalCfgGeneric {
  static constexpr bool FIXED = false, VIS_FIXED = false;
  // (not read)
  static constexpr bool USE3D = false, SHIFT_NULL = false, USE_MIS = false, POWER_HEURISTIC = false, DEBUG_SHIFT_NULL = false,
                        PATH_SET = false, VIS_AS_WRITTEN = false, EXACT_ALL = false;
};
// The configuration of the synthetic hosts' workloads (defaultParams, host/synth.cpp): the 3D kernel with null shifts, MIS with
// the balance heuristic, the checkerboard path set, no debug filter, no GVPM_EXACT_ALL.  visibility_as_written is fixed (on)
// where the kernel reads the near lists: the driver starts that form only with it on.  The form that walks the occluder BVH
// serves both settings -- an overflowing near list sends a handle with it on there -- and keeps the test (VIS = false).
template <bool VIS> struct EvalCfgHeadline {
  static constexpr bool FIXED = true, VIS_FIXED = VIS;
  static constexpr bool USE3D = true, SHIFT_NULL = true, USE_MIS = true, POWER_HEURISTIC = false, DEBUG_SHIFT_NULL = false,
                        PATH_SET = true, VIS_AS_WRITTEN = true, EXACT_ALL = false;
};
// a flag of the configuration: the constant where it is fixed, else what a.cfg says
template <bool FIXED, bool VALUE> __device__ __forceinline__ constexpr bool cfgFlag(bool fromCfg) {
  if constexpr (FIXED) return VALUE;
  else return fromCfg;
}

// shiftPhotonDiffuse + diffuseReconnection.  Returns the MIS weight, writes the shifted flux.
// Written branch-free apart from the shadow-ray loop: every early `return false` of the reference
// (shift_volume_photon.cpp:398-412, shift_diffuse.cpp:43-47, 100-104, :463-470) clears `good`, the
// arithmetic runs for all lanes and the result is selected at the end.
template <bool FULLVIS, bool MIX = true, typename CFG = EvalCfgGeneric>
__device__ __forceinline__ float shiftDiffuse(const GatherArgs &a, const PhotonCold &ph,
                                              uint32_t bits, f3 dProjU, const RayReg &sh, const RayReg &base,
                                              uint32_t edge, f3 trShift, float pdfBaseRay, float pdfShiftRay,
                                              f3 &shiftedFlux, bool &ok, const float4 *ldsTri = nullptr,
                                              float sensorMisPre = -1.f, uint32_t *amb = nullptr) {
  const uint32_t ptype = GVPM_PF_PARENT_TYPE(bits);
  const float l2Proj = dot(dProjU, dProjU);
  const float lProj = fsqrt(l2Proj);
  const f3 dProj = dProjU * frcp(lProj);
  const float eps = a.cfg.epsilon, seps = a.cfg.shadow_epsilon;
  const float vmax = cfgFlag<CFG::VIS_FIXED, CFG::VIS_AS_WRITTEN>(a.cfg.visibility_as_written) ? lProj * seps : lProj * (1.f - seps);
  // (amb: the caller defers undecidable shifts to the exact pass; without one the plain fp32 decision stands)
  // bit 15 of the record's flags: the parent lies behind a wall it sits on, word 2 of its list is that wall's REACH
  // cstar = |delta| / Epsilon instead of entries (near_lists.h, ownWall): the wall itself is not listed
  const bool behind = (bits >> 15) & 1u;
  const float cosWo = dot(ph.parentN, dProj);
  // (a segment that leaves within cstar of grazing meets the own wall's plane at t >= Epsilon: the exact pass decides; 1.2e-3:
  // the parent's normal against the triangle's, ownWall's parallel test.  Decided BEFORE the visibility loop: the reach is
  // not carried across it)
  const bool ownAmb = behind && cosWo > 0.f && cosWo <= __uint_as_float(ph.nl2) + 1.2e-3f;
  const int vis = shadowBlocked<FULLVIS>(a, ldsTri, ph.nl0, ph.nl1, behind ? 0xFFFFFFFFu : ph.nl2, ph.parentPos, dProj, eps, vmax);
  bool good = vis == GVPM_TRI_MISS;
#ifdef GVPM_DBG_SHIFT2  // (probe builds, on a single pair: scripts/probes_py/vpm_bisect.py)
  printf("shiftDiffuse vis %d ownAmb %d behind %d cosWo %g lProj %.9g vmax %.9g lists %08x %08x %08x parent %.9g %.9g %.9g dir %.9g %.9g %.9g\n", vis,
         (int)ownAmb, (int)behind, cosWo, lProj, vmax, ph.nl0, ph.nl1, ph.nl2, ph.parentPos.x, ph.parentPos.y, ph.parentPos.z, dProj.x, dProj.y,
         dProj.z);
#endif
  // (the sign / cosine tests below flip within fp32 rounding of a grazing direction)
  if (amb)
    *amb = (((vis & GVPM_TRI_AMB) || ownAmb) ? 16u : 0u) |
           ((GVPM_PF_PARENT_TYPE(bits) != GVPM_PARENT_MEDIUM && fabsf(cosWo) <= 2e-6f) ? 32u : 0u);
  // surface / emitter parents: the offset direction must leave on the side the photon left (sign of
  // dot(n, dProj) / dot(n, -wi))
  const bool isMedium = ptype == GVPM_PARENT_MEDIUM, isGlossy = ptype == GVPM_PARENT_SURFACE_BSDF;
  const bool isSurface = ptype == GVPM_PARENT_SURFACE || isGlossy;
  good = good && (isMedium || cosWo * dot(ph.parentN, -ph.wi) >= 0.f);
  // eval / pdf of the parent towards the offset position (diffuse.cpp:110-127, phase eval, area.cpp:132-150)
  const float cosWi = dot(ph.parentN, ph.parentWi);
  // eval/pdf = 0 or the shading-normal reject; a glossy parent may have been met from the other side (a transmitted photon of a
  // rough dielectric: glossyParentEval decides)
  good = good && (!isSurface || (cosWo > 0.f && (isGlossy ? cosWi != 0.f : cosWi > 0.f)));
  const float lam = INV_PI_F * fmaxf(cosWo, 0.f);
  const float pMed = phaseEval(ph.parentG, ph.parentWi, dProj);
  float pdfValue = isMedium ? pMed : lam;
  f3 thr = isSurface ? ph.parentScat * lam : (isMedium ? ph.parentScat * pMed : mk3(lam));
  bool pdfTiny = false;  // (glossyParentEval: the pdf underflowed HERE, not in the reference's double)
  if (isGlossy) {
    // (a branch of its own: scenes without glossy walls pay one wave-uniform test)
    uint32_t gst = 0u;
    if (!glossyParentEval<MIX>(a, ph.parentG, ph.parentScat, ph.parentN, ph.parentWi, dProj, cosWi, cosWo, thr, pdfValue, &gst)) good = false;
    pdfTiny = (gst & 1u) != 0u;
    if (amb && (gst & 2u)) *amb |= 32u;
  }
  const float gop = frcp(l2Proj);
  float sPdf = pdfValue * gop;
  good = good && ph.parentPdf != 0.f;
  thr = thr * (gop * ph.parentRR * frcp(ph.parentPdf));
  if (GVPM_PF_EDGE_IN_MEDIUM(bits)) {
    f3 tr;
    float pdfSuccess;
    mediumEval(a.med, lProj, tr, pdfSuccess);
    sPdf *= pdfSuccess;
    thr = thr * tr * frcp(ph.edgePdf);
  }
  good = good && (sPdf != 0.f || pdfTiny);
  const f3 photonWeight = ph.prefixW * thr;
  const f3 sigS = mk3(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]);
  const f3 contrib = sigS * photonWeight * phaseEval(a.med.g, -dProj, -sh.d);
  float w = 0.5f;
  bool misOk = true;
  if (cfgFlag<CFG::FIXED, CFG::USE_MIS>(a.cfg.use_mis)) {
    const float basePdf = pdfBaseRay * ph.parentPdf * ph.edgePdf;
    const float offsetPdf = sPdf * pdfShiftRay;
    misOk = !((offsetPdf == 0.f && !(pdfTiny && pdfShiftRay != 0.f)) || basePdf == 0.f);
    // (sensorMisPre: the caller's per-(shift, beam) value, when it keeps one)
    const float v = (sensorMisPre >= 0.f ? sensorMisPre : sensorMIS(sh, base, edge)) * fdiv(offsetPdf, basePdf);
    w = cfgFlag<CFG::FIXED, CFG::POWER_HEURISTIC>(a.cfg.power_heuristic) ? frcp(1.f + v * v) : frcp(1.f + v);
  }
  // a failed MIS keeps the flux it computed and takes weight 1 (shift_volume_photon.cpp:463-470)
  shiftedFlux = good ? trShift * contrib * sh.eye : mk3(0.f);  // jacobian == 1
  ok = good && misOk;
  return ok ? w : 1.f;
}

// A shift that needs the manifold walk (shiftPhotonManifold, shift_volume_photon.cpp:160-295): what the walk reads goes
// to the host's request list, what the device needs to finish the shift once the host has answered (:217-279) stays beside
// it.  Rare and register hungry: not inlined -- and handed the list BY VALUE: a `const GatherArgs &` here makes the kernel
// keep its whole argument block in scratch (a 600-byte frame, every a.field a scratch load).  False: the list is full --
// a failed shift.
struct ReqSink {
  gvpm_shift_request *host;
  float4 *ctx;
  uint32_t *count;
  uint32_t cap;
  const uint32_t *origIdx;
};
__device__ __forceinline__ ReqSink reqSink(const GatherArgs &a) { return ReqSink{a.reqHost, a.reqCtx, a.reqCount, a.reqCap, a.origIdx}; }

static __device__ __noinline__ bool recordShiftRequest(ReqSink a, float radius, uint32_t pidx, uint32_t set, int i, f3 offsetPos, f3 basePt,
                                                       f3 shiftPt, float tPrime, float tr, float pdfCam, float pdfShiftPos, float sMIS,
                                                       float scale, f3 bc, f3 shD, f3 eye, uint32_t pix) {
  const uint32_t slot = atomicAdd(a.count, 1u);
  if (slot >= a.cap) return false;
  gvpm_shift_request rq;
  rq.photon = a.origIdx[pidx];
  rq.set = set;
  rq.shift = (uint32_t)i;
  rq.reserved = 0u;
  rq.offset_pos[0] = offsetPos.x; rq.offset_pos[1] = offsetPos.y; rq.offset_pos[2] = offsetPos.z;
  rq.radius = radius;  // (G-VPM: the pixel's own radius)
  rq.base_point[0] = basePt.x; rq.base_point[1] = basePt.y; rq.base_point[2] = basePt.z;
  rq.t = tPrime;
  rq.shift_point[0] = shiftPt.x; rq.shift_point[1] = shiftPt.y; rq.shift_point[2] = shiftPt.z;
  rq.reserved2 = 0.f;
  a.host[slot] = rq;
  float4 *c = a.ctx + 4 * (size_t)slot;
  c[0] = make_float4(tr, pdfCam, pdfShiftPos, sMIS);
  c[1] = make_float4(scale, bc.x, bc.y, bc.z);
  c[2] = make_float4(shD.x, shD.y, shD.z, __uint_as_float(pix));
  c[3] = make_float4(eye.x, eye.y, eye.z, __uint_as_float((uint32_t)i));
  return true;
}

// computeVolumeContribution (gvpm/shift/shift_utilities.h:231-253) and the debugShift filter
// (shift_volume_photon.cpp:680-687) depend only on the photon and the configuration: fold
// them into bit 6 of the hot record.
__device__ __forceinline__ bool photonContributes(uint32_t flags, const gvpm_params &cfg) {
  const int mode = cfg.lighting_interaction_mode;
  const uint32_t ptype = GVPM_PF_PARENT_TYPE(flags);
  if (!((mode & GVPM_SURF2MEDIA) && (mode & GVPM_MEDIA2MEDIA))) {
    if (ptype == GVPM_PARENT_MEDIUM && !(mode & GVPM_MEDIA2MEDIA)) return false;
    if (ptype != GVPM_PARENT_MEDIUM && !(mode & GVPM_SURF2MEDIA)) return false;
  }
  const int compo = (int)GVPM_PF_PREV_COMPONENT(flags);
  if (cfg.bsdf_interaction_mode != GVPM_BSDF_ALL && compo > 0 && !(compo & cfg.bsdf_interaction_mode)) return false;
  if (cfg.debug_shift != GVPM_SHIFT_ALL && cfg.debug_shift != GVPM_SHIFT_NULL) {
    int st;
    switch (GVPM_PF_SHIFT_TYPE(flags)) {
      case 1: st = GVPM_SHIFT_DIFFUSE; break;
      case 2: st = GVPM_SHIFT_MEDIUM; break;
      case 3: st = GVPM_SHIFT_MANIFOLD; break;
      default: st = GVPM_SHIFT_INVALID; break;
    }
    if (cfg.debug_shift != st) return false;
  }
  return true;
}

}  // namespace gvpm
