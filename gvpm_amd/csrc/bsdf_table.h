// The table of gvpm_upload_bsdfs (include/gvpm_hip.h, gvpm_bsdf), once: how many raw entries follow a head, how a head is
// packed into the four 16-byte rows the device reads, which lane of which row holds which field, and the rules a table
// must obey.  Plain C++17 without HIP types, so that the host library includes it too; the readers are templates over any row
// type with members x, y, z, w (the device's float4).  A new kind is added HERE first: writer and readers on one screen.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/gvpm_hip.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GVPM_TBL __host__ __device__ __forceinline__
#else
#define GVPM_TBL inline
#endif

namespace gvpm {

GVPM_TBL uint32_t bsdfBits(float v) {
  uint32_t b;
  __builtin_memcpy(&b, &v, 4);
  return b;
}
GVPM_TBL float bsdfWord(int32_t i) {
  float v;
  __builtin_memcpy(&v, &i, 4);
  return v;
}

// ---- raw entries behind a head ----
// A rough-plastic head is followed by its transmittance slice (GVPM_RTRANS_KNOTS floats, then zero words), an anisotropic
// head by its frame entry ({tangent, alphaV}, then zero words); photons name head indices only.
GVPM_TBL int bsdfTailEntries(int kind) {
  if (kind == GVPM_BSDF_ROUGHPLASTIC) return GVPM_RTRANS_ENTRIES;
  return (kind == GVPM_BSDF_WARD_ANISO || kind == GVPM_BSDF_ROUGHCONDUCTOR_ANISO) ? GVPM_ANISO_ENTRIES : 0;
}
// +0 or a NORMAL float (not -0, a subnormal, NaN or inf): a raw entry's first word must never read as a kind
GVPM_TBL bool bsdfRawWordValid(float v) { return bsdfBits(v) == 0u || (std::fabs(v) >= FLT_MIN && std::fabs(v) <= FLT_MAX); }
// word j of the raw entries behind a head of `kind`: slice values lie in [0, 1], frame words are signed, the padding is +0
GVPM_TBL bool bsdfTailWordValid(int kind, int j, float v) {
  const bool slice = kind == GVPM_BSDF_ROUGHPLASTIC;
  if (j >= (slice ? GVPM_RTRANS_KNOTS : 4)) return bsdfBits(v) == 0u;
  return bsdfRawWordValid(v) && (!slice || (v >= 0.f && v <= 1.f));
}

// ---- rules shared by the kinds ----
GVPM_TBL bool bsdfWeightValid(float w) { return w >= 0.f && w <= 1.f; }
GVPM_TBL bool bsdfAlphaValid(float alpha) { return alpha >= 1e-4f; }  // (the microfacet constructor's clamp, microfacet.h:88-90)
GVPM_TBL bool bsdfMicrofacetValid(const gvpm_bsdf &b) {
  return b.distribution == GVPM_MICROFACET_BECKMANN || b.distribution == GVPM_MICROFACET_GGX || b.distribution == GVPM_MICROFACET_PHONG;
}
// (the Phong / Ashikhmin-Shirley distribution has no visible-normal sampling: the reference forces it off, microfacet.h:140-144)
GVPM_TBL bool bsdfSampleVisibleValid(const gvpm_bsdf &b) { return b.distribution != GVPM_MICROFACET_PHONG || b.sample_visible == 0; }
// (Ward: the variant rides in sample_visible, and both components only)
GVPM_TBL bool bsdfWardVariantValid(const gvpm_bsdf &b) {
  return b.sample_visible >= GVPM_WARD_WARD && b.sample_visible <= GVPM_WARD_BALANCED && b.distribution == 0;
}

// the rough dielectric's relative index as seen from wi's side: finite, within [0.2, 5] (either side of any real glass)
GVPM_TBL bool bsdfDielectricEtaValid(float eta) { return eta >= 0.2f && eta <= 5.f; }
GVPM_TBL bool bsdfChannelValid(float c) { return c >= 0.f && c <= 1.f; }
// every word the rough dielectric leaves unused is +0
GVPM_TBL bool bsdfDielectricZerosValid(const gvpm_bsdf &b) {
  return (bsdfBits(b.eta[1]) | bsdfBits(b.eta[2]) | bsdfBits(b.specular_sampling_weight) | bsdfBits(b.reserved[0]) | bsdfBits(b.reserved[1])) == 0u;
}

// the mixture: a weight is finite and not negative (their sum > 0 is the caller's test); a child word is GVPM_MIXTURE_CHILD_DIFFUSE,
// GVPM_MIXTURE_CHILD_ABSENT or a table index below n, as an integer-valued float; every word the kind leaves unused is +0
GVPM_TBL bool bsdfMixtureWeightValid(float w) { return w >= 0.f && w <= FLT_MAX; }
GVPM_TBL bool bsdfMixtureChildValid(float c, uint32_t n) {
  return c == (float)GVPM_MIXTURE_CHILD_DIFFUSE || c == (float)GVPM_MIXTURE_CHILD_ABSENT ||
         (bsdfBits(c) == 0u || (c > 0.f && c < (float)n && c == (float)(uint32_t)c));
}
GVPM_TBL bool bsdfMixtureZerosValid(const gvpm_bsdf &b) {
  return (bsdfBits(b.specular[2]) | bsdfBits(b.exponent) | bsdfBits(b.specular_sampling_weight) | (uint32_t)b.sample_visible |
          bsdfBits(b.eta[2]) | bsdfBits(b.k[0]) | bsdfBits(b.k[1]) | bsdfBits(b.k[2]) | bsdfBits(b.reserved[0]) | bsdfBits(b.reserved[1])) == 0u;
}

// ---- a head's four rows ----
//   row 0  {kind, specular.rgb}
//   row 1  {exponent | alpha (alphaU), sampling weight, distribution | Phong component, sample_visible | Ward variant}
//   row 2  {eta.rgb, k.r}         plastics: {eta, Fdr, -, component met}
//   row 3  {k.g, k.b, 0, 0}       plastics: {nonlinear, ...}
//   rough dielectric: row 2 {eta seen from wi's side, 0, 0, transmittance.r}, row 3 {transmittance.g, transmittance.b, 0, 0}
//   mixture: row 0 {kind, w_0, w_1, 0}, row 1 {0, 0, sampled component + 1, 0}, row 2 {child 0, child 1, 0, 0}
// The integers travel as their bit patterns, the plastics' component and nonlinear flag as the floats they are in gvpm_bsdf.
// The readers return a lane as it is stored and leave `!= 0` / `(int)` to the caller where the caller had them: moving such a
// conversion into the reader changed the kernels' register allocation (NOTEBOOK.md, "one home for the BSDF table").
inline void bsdfPackRows(const gvpm_bsdf &b, float rows[16]) {
  const float r[16] = {bsdfWord(b.kind), b.specular[0], b.specular[1], b.specular[2],
                       b.exponent, b.specular_sampling_weight, bsdfWord(b.distribution), bsdfWord(b.sample_visible),
                       b.eta[0], b.eta[1], b.eta[2], b.k[0],
                       b.k[1], b.k[2], 0.f, 0.f};
  memcpy(rows, r, sizeof r);
}
// row 0
template <class R> GVPM_TBL int bsdfKind(const R &r0) { return (int)bsdfBits(r0.x); }
template <int C, class R> GVPM_TBL float bsdfSpecular(const R &r0) { return C == 0 ? r0.y : (C == 1 ? r0.z : r0.w); }
// row 1
template <class R> GVPM_TBL float bsdfExponent(const R &r1) { return r1.x; }  // Phong
template <class R> GVPM_TBL float bsdfAlpha(const R &r1) { return r1.x; }     // every other kind; alphaU of the anisotropic ones
template <class R> GVPM_TBL float bsdfSamplingWeight(const R &r1) { return r1.y; }
template <class R> GVPM_TBL int bsdfPhongComponent(const R &r1) { return (int)bsdfBits(r1.z); }  // 0 both, 1 specular, 2 diffuse
template <class R> GVPM_TBL int bsdfDistribution(const R &r1) { return (int)bsdfBits(r1.z); }    // GVPM_MICROFACET_*
template <class R> GVPM_TBL int bsdfSampleVisible(const R &r1) { return (int)bsdfBits(r1.w); }  // != 0: the pdf's visible-normals form
template <class R> GVPM_TBL int bsdfWardVariant(const R &r1) { return (int)bsdfBits(r1.w); }  // GVPM_WARD_*
// rows 2 and 3, rough conductor: channel C of eta and k
template <int C, class R> GVPM_TBL float bsdfConductorEta(const R &r2) { return C == 0 ? r2.x : (C == 1 ? r2.y : r2.z); }
template <int C, class R> GVPM_TBL float bsdfConductorK(const R &r2, const R &r3) { return C == 0 ? r2.w : (C == 1 ? r3.x : r3.y); }
// rows 2 and 3, the plastics
template <class R> GVPM_TBL float bsdfPlasticEta(const R &r2) { return r2.x; }
template <class R> GVPM_TBL float bsdfPlasticFdr(const R &r2) { return r2.y; }
template <class R> GVPM_TBL float bsdfPlasticComponent(const R &r2) { return r2.w; }  // 0.f both, 1.f glossy, 2.f diffuse
template <class R> GVPM_TBL bool bsdfPlasticNonlinear(const R &r3) { return r3.x != 0.f; }
// rows 2 and 3, the rough dielectric: the relative index seen from wi's side, channel C of the specular transmittance
template <class R> GVPM_TBL float bsdfDielectricEta(const R &r2) { return r2.x; }
template <int C, class R> GVPM_TBL float bsdfTransmittance(const R &r2, const R &r3) { return C == 0 ? r2.w : (C == 1 ? r3.x : r3.y); }
// the mixture: weight and child word I (0 or 1), the component met
template <int I, class R> GVPM_TBL float bsdfMixtureWeight(const R &r0) { return I == 0 ? r0.y : r0.z; }
template <int I, class R> GVPM_TBL float bsdfMixtureChild(const R &r2) { return I == 0 ? r2.x : r2.y; }
template <class R> GVPM_TBL int bsdfMixtureComponent(const R &r1) { return (int)bsdfBits(r1.z); }  // 0 both, 1 child 0, 2 child 1
// the frame entry behind an anisotropic head, as one row: {tangent.xyz, alphaV}
template <class R> GVPM_TBL float bsdfFrameAlphaV(const R &fr) { return fr.w; }

}  // namespace gvpm
