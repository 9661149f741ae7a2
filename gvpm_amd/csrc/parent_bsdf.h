// The BSDF models of a glossy surface parent (GVPM_PARENT_SURFACE_BSDF): microfacet distributions, Fresnel terms, the rough
// transmittance and the evaluation of one entry of the table of gvpm_upload_bsdfs, whose rows bsdf_table.h lays out.
#pragma once
#include <hip/hip_runtime.h>

#include "bsdf_table.h"
#include "device_types.h"
#include "vec.h"

namespace gvpm {

#define PI_F 3.14159265358979323846f
#define INV_PI_F 0.31830988618379067154f
#define INV_TWOPI_F 0.15915494309189533577f
#define INV_FOURPI_F 0.07957747154594766788f

// MicrofacetDistribution, isotropic (src/bsdfs/microfacet.h): D of a half vector with cosine cH to the normal (:191-232) and
// Smith's G1 of a direction with cosine cV to the normal and vDotH to the half vector (:477-518).
// The Phong / Ashikhmin-Shirley distribution (GVPM_MICROFACET_PHONG) has the exponent max(2 / alpha^2 - 2, 0) (:700-704) and
// D = (e + 2) / (2 pi) cos^e; the power is formed as the Phong kind forms its lobe.  Its G1 is Beckmann's, with alpha (:489-501).
__device__ __forceinline__ float phongExponent(float alpha) { return fmaxf(fdiv(2.f, alpha * alpha) - 2.f, 0.f); }
__device__ __forceinline__ float microfacetD(int dist, float alpha, float cH) {
  if (cH <= 0.f) return 0.f;
  const float c2 = cH * cH;
  const float e = fdiv(fmaxf(1.f - c2, 0.f), alpha * alpha * c2);  // tan^2 / alpha^2: Beckmann's and GGX's; the Phong arm does not read it
  float r;
  if (dist == GVPM_MICROFACET_GGX) {
    const float root = (1.f + e) * c2;
    r = frcp(PI_F * alpha * alpha * root * root);
  } else if (dist != GVPM_MICROFACET_PHONG) {
    r = fdiv(__expf(-e), PI_F * alpha * alpha * c2 * c2);
  } else {
    const float ex = phongExponent(alpha);  // (the Phong EXPONENT, not `e` above)
    r = (ex + 2.f) * INV_TWOPI_F * __builtin_exp2f(ex * __builtin_log2f(cH));  // std::pow(cos(theta_m), exponent)
  }
  return r * cH < 1e-20f ? 0.f : r;
}
__device__ __forceinline__ float microfacetG1(int dist, float alpha, float cV, float vDotH) {
  if (vDotH * cV <= 0.f) return 0.f;
  const float t2 = 1.f - cV * cV;
  if (t2 <= 0.f) return 1.f;  // perpendicular incidence
  const float tanT = fabsf(fdiv(fsqrt(t2), cV));
  if (dist == GVPM_MICROFACET_GGX) {
    const float root = alpha * tanT;
    return fdiv(2.f, 1.f + fsqrt(1.f + root * root));
  }
  const float a = frcp(alpha * tanT);
  if (a >= 1.6f) return 1.f;
  const float a2 = a * a;
  return fdiv(3.535f * a + 2.181f * a2, 1.f + 2.276f * a + 2.577f * a2);
}
// The anisotropic kinds (GVPM_BSDF_WARD_ANISO, GVPM_BSDF_ROUGHCONDUCTOR_ANISO): the frame entry behind the head carries the
// surface's tangent s and alphaV; with the record's parent normal n, s' = normalize(s - n (n . s)) and t = n x s' stand for the
// shading frame's s and t.  Only SQUARES of the tangential components enter the formulas, so neither the sign of s nor the
// handedness of (s', t, n) matters.  False: the tangent is parallel to the normal -- a failed shift.
__device__ __forceinline__ bool anisoFrame(const float4 fr, f3 n, f3 &s, f3 &t) {
  s = mk3(fr.x, fr.y, fr.z);
  s = s - n * dot(n, s);
  const float ss = dot(s, s);
  if (ss < 1e-12f) return false;
  s = s * frsq(ss);
  t = cross(n, s);
  return true;
}
// MicrofacetDistribution::eval with alphaU != alphaV (microfacet.h:191-232): mx, my, cH = the unit half vector in the frame
// Ashikhmin-Shirley (GVPM_MICROFACET_PHONG): the exponent interpolated between eU and eV by the half vector's azimuth
// (interpolatePhongExponent, :553-565: eU where alphaU == alphaV or sin^2(theta_m) <= RCPOVERFLOW), D = sqrt((eU + 2)(eV + 2)) /
// (2 pi) cos^e
__device__ __forceinline__ float microfacetDAniso(int dist, float au, float av, float mx, float my, float cH) {
  if (cH <= 0.f) return 0.f;
  const float c2 = cH * cH, ux = fdiv(mx, au), uy = fdiv(my, av);
  const float e = fdiv(ux * ux + uy * uy, c2);  // (Beckmann's and GGX's; the Phong arm reads neither it nor ux, uy)
  float r;
  if (dist == GVPM_MICROFACET_GGX) {
    const float root = (1.f + e) * c2;
    r = frcp(PI_F * au * av * root * root);
  } else if (dist != GVPM_MICROFACET_PHONG) {
    r = fdiv(__expf(-e), PI_F * au * av * c2 * c2);
  } else {
    const float eU = phongExponent(au), eV = phongExponent(av), s2 = 1.f - c2;
    const float ex = (au == av || s2 <= 0x1p-128f) ? eU : fdiv(eU * (mx * mx) + eV * (my * my), s2);
    r = fsqrt((eU + 2.f) * (eV + 2.f)) * INV_TWOPI_F * __builtin_exp2f(ex * __builtin_log2f(cH));
  }
  return r * cH < 1e-20f ? 0.f : r;
}
// projectRoughness (microfacet.h:541-551) of a unit direction with tangential components vx, vy and cosine cV; at
// perpendicular incidence (sin^2 <= 0) the value is not used: microfacetG1 returns 1 before it reads alpha (:484-488)
__device__ __forceinline__ float projectRoughness(float au, float av, float vx, float vy, float cV) {
  return fsqrt(fdiv(vx * vx * (au * au) + vy * vy * (av * av), 1.f - cV * cV));
}
// fresnelConductorExact, one channel (src/libcore/util.cpp:747-769)
__device__ __forceinline__ float fresnelConductor(float cI, float eta, float k) {
  const float c2 = cI * cI, s2 = 1.f - c2, s4 = s2 * s2;
  const float t1 = eta * eta - k * k - s2;
  const float a2pb2 = fsqrt(fmaxf(t1 * t1 + k * k * eta * eta * 4.f, 0.f));
  const float aa = fsqrt(fmaxf((a2pb2 + t1) * 0.5f, 0.f));
  const float term1 = a2pb2 + c2, term2 = aa * (2.f * cI);
  const float Rs2 = fdiv(term1 - term2, term1 + term2);
  const float term3 = a2pb2 * c2 + s4, term4 = term2 * s2;
  const float Rp2 = Rs2 * fdiv(term3 - term4, term3 + term4);
  return 0.5f * (Rp2 + Rs2);
}
// fresnelDielectricExt for a cosine >= 0 and eta >= 1 (src/libcore/util.cpp:659-689): exactly 0 at eta == 1; no total internal
// reflection from the rarer side
__device__ __forceinline__ float fresnelDielectric(float cI, float eta) {
  if (eta == 1.f) return 0.f;
  const float ie = frcp(eta);
  const float cT = fsqrt(fmaxf(1.f - (1.f - cI * cI) * (ie * ie), 0.f));
  const float Rs = fdiv(cI - eta * cT, cI + eta * cT), Rp = fdiv(eta * cI - cT, eta * cI + cT);
  return 0.5f * (Rs * Rs + Rp * Rp);
}
// RoughTransmittance::eval with eta and alpha fixed (src/bsdfs/rtrans.h:183-236): evalCubicInterp1D (libcore/spline.cpp:23-60)
// of the 100 values `t` over cos^(1/4) in [0, 1] -- Catmull-Rom, one-sided differences at the ends, left knot
// min(floor(x), 98) -- clamped to [0, 1].  c > 0 is the caller's test; a cosine that rounding left above 1 is looked up at 1.
__device__ __forceinline__ float roughTransmittance(const float *__restrict__ t, float c) {
  const float x = fsqrt(fsqrt(fminf(c, 1.f))) * (float)(GVPM_RTRANS_KNOTS - 1);
  const int k = min((int)x, GVPM_RTRANS_KNOTS - 2);
  const float f0 = t[k], f1 = t[k + 1];
  const float fm = t[max(k - 1, 0)], f2 = t[min(k + 2, GVPM_RTRANS_KNOTS - 1)];
  const float d0 = k > 0 ? 0.5f * (f1 - fm) : f1 - f0;
  const float d1 = k + 2 < GVPM_RTRANS_KNOTS ? 0.5f * (f2 - f0) : f1 - f0;
  const float u = x - (float)k, u2 = u * u, u3 = u2 * u;
  const float r = (2.f * u3 - 3.f * u2 + 1.f) * f0 + (-2.f * u3 + 3.f * u2) * f1 + (u3 - 2.f * u2 + u) * d0 + (u3 - u2) * d1;
  return fminf(fmaxf(r, 0.f), 1.f);
}

// fresnelDielectricExt for a cosine of either sign and any eta > 0 (src/libcore/util.cpp:659-689): a negative cosine meets the
// inverse index; total internal reflection (cos^2(theta_T) <= 0) gives 1
__device__ __forceinline__ float fresnelDielectricExt(float cI, float eta) {
  if (eta == 1.f) return 0.f;
  const float e = cI > 0.f ? eta : frcp(eta), c = fabsf(cI), ie = frcp(e);
  if (1.f - (1.f - c * c) * (ie * ie) <= 0.f) return 1.f;
  return fresnelDielectric(c, e);
}

// a head's specular reflectance (bsdf_table.h, row 0)
__device__ __forceinline__ f3 bsdfSpecular3(const float4 b0) { return mk3(bsdfSpecular<0>(b0), bsdfSpecular<1>(b0), bsdfSpecular<2>(b0)); }

// The rough dielectric (GVPM_BSDF_ROUGHDIELECTRIC; src/bsdfs/roughdielectric.cpp:270-422, include/gvpm_hip.h), the one kind that
// transmits.  `n` is the record's normal, on the side the photon LEFT (cosWo > 0 is the caller's test): cosWi > 0 is reflection,
// cosWi < 0 transmission.  Everything in wi's frame: nI = n sign(cosWi), ci = |cosWi|, co = +-cosWo, eta = the entry's index
// behind the surface over the index on wi's side.  Returns {eval.rgb, pdf}; pdf < 0: |wi + wo eta|^2 < 1e-12, no half vector -- a
// failed shift.  Inlined, and dispatched LAST in glossyParentEval: as a __noinline__ function handed everything by value it cost
// seven to ten evaluation kernels scratch, inlined but dispatched first five (NOTEBOOK.md, "Rough-dielectric parents").
__device__ __forceinline__ float4 roughDielectricEval(const float4 *__restrict__ e, f3 n, f3 wi, f3 wo, float cosWi, float cosWo) {
  const float4 b0 = e[0], b1 = e[1], b2 = e[2], b3 = e[3];
  const float sgn = cosWi > 0.f ? 1.f : -1.f, ci = fabsf(cosWi), co = cosWo * sgn;
  const bool reflect = cosWi > 0.f;
  const float eta = bsdfDielectricEta(b2), alpha = bsdfAlpha(b1);
  const int dist = bsdfDistribution(b1), vis = bsdfSampleVisible(b1) != 0;
  f3 H = reflect ? wi + wo : wi + wo * eta;
  const float HH = dot(H, H);
  if (HH < 1e-12f) return make_float4(0.f, 0.f, 0.f, -1.f);
  H = H * frsq(HH);
  float cH = dot(H, n) * sgn;  // (the half vector in nI's hemisphere, :300-302)
  if (cH < 0.f) {
    H = -H;
    cH = -cH;
  }
  const float wiH = dot(wi, H), woH = dot(wo, H);
  // D of the surface's alpha, and the D the half vector was sampled with: the same for visible normals, else at the alpha Walter's
  // trick scaled (:406-414) with its own `D' cos_H < 1e-20` cut.  D == 0 gives eval = 0 (:315-316) -- and pdf = 0 only if D' is
  // zero too: RoughDielectric::pdf does not look at D, so a half vector in the band between the two cuts is a shift that
  // SUCCEEDS with zero flux (the products below are 0 x finite)
  const float D = microfacetD(dist, alpha, cH);
  const float Ds = vis ? D : microfacetD(dist, alpha * (1.2f - 0.2f * fsqrt(ci)), cH);
  if (D == 0.f && Ds == 0.f) return make_float4(0.f, 0.f, 0.f, 0.f);
  const float F = fresnelDielectricExt(wiH, eta);
  const float G1i = microfacetG1(dist, alpha, ci, wiH), G1o = microfacetG1(dist, alpha, co, woH);
  f3 f;
  float dwh;
  if (reflect) {
    f = bsdfSpecular3(b0) * fdiv(F * D * G1i * G1o, 4.f * ci);
    dwh = frcp(4.f * woH);
  } else {
    const float sD = wiH + eta * woH, e2 = fdiv(eta * eta, sD * sD);
    // (EImportance: no solid-angle compression factor, :339-343)
    f = mk3(bsdfTransmittance<0>(b2, b3), bsdfTransmittance<1>(b2, b3), bsdfTransmittance<2>(b2, b3)) *
        fabsf(fdiv((1.f - F) * D * G1i * G1o * e2 * wiH * woH, ci));
    dwh = e2 * woH;
  }
  // the sampling density of the half vector: visible normals, or all normals
  const float prob = vis ? fdiv(D * G1i * fabsf(wiH), ci) : Ds * cH;
  return make_float4(f.x, f.y, f.z, fabsf(prob * dwh) * (reflect ? F : 1.f - F));
}

// The rough conductor (GVPM_BSDF_ROUGHCONDUCTOR, GVPM_BSDF_ROUGHCONDUCTOR_ANISO; src/bsdfs/roughconductor.cpp:257-319, include/gvpm_hip.h)
// of head `bi`, whose first two rows the caller has read: eval = F D G / (4 cos_i), pdf = D G1(wi) / (4 cos_i) or D cos_H / (4 |wo . H|).
// Once, for the kind's own arm of glossyParentEval and for the children of a mixture.  f and pdf arrive zero and stay zero where
// D == 0 (pdfAll = D cos_H, pdfVisible = D G1 ...).  False: the anisotropic frame is rejected -- a failed shift.
__device__ __forceinline__ bool roughConductorEval(const GatherArgs &a, uint32_t bi, const float4 b0, const float4 b1, int kind, f3 n, f3 wi,
                                                   f3 wo, float cosWi, float cosWo, f3 &f, float &pdf) {
  const float4 b2 = a.bsdfs[4 * bi + 2], b3 = a.bsdfs[4 * bi + 3];
  const float alpha = bsdfAlpha(b1);
  const int dist = bsdfDistribution(b1), vis = bsdfSampleVisible(b1) != 0;
  f3 H = wi + wo;
  H = H * frsq(dot(H, H));
  const float cH = dot(H, n), wiH = dot(wi, H), woH = dot(wo, H);
  float D, alI = alpha, alO = alpha;  // (anisotropic: alphaU = the head's alpha, the roughness projected on wi and on wo)
  if (kind == GVPM_BSDF_ROUGHCONDUCTOR) {
    D = microfacetD(dist, alpha, cH);
  } else {
    const float4 fr = a.bsdfs[4 * (bi + 1)];
    f3 s, t;
    if (!anisoFrame(fr, n, s, t)) return false;
    D = microfacetDAniso(dist, alpha, bsdfFrameAlphaV(fr), dot(H, s), dot(H, t), cH);
    if (D != 0.f) {
      alI = projectRoughness(alpha, bsdfFrameAlphaV(fr), dot(wi, s), dot(wi, t), cosWi);
      alO = projectRoughness(alpha, bsdfFrameAlphaV(fr), dot(wo, s), dot(wo, t), cosWo);
    }
  }
  if (D == 0.f) return true;  // eval and pdf both zero
  const float G1i = microfacetG1(dist, alI, cosWi, wiH), G1o = microfacetG1(dist, alO, cosWo, woH);
  const float model = fdiv(D * G1i * G1o, 4.f * cosWi);
  f = mk3(fresnelConductor(wiH, bsdfConductorEta<0>(b2), bsdfConductorK<0>(b2, b3)) * bsdfSpecular<0>(b0),
          fresnelConductor(wiH, bsdfConductorEta<1>(b2), bsdfConductorK<1>(b2, b3)) * bsdfSpecular<1>(b0),
          fresnelConductor(wiH, bsdfConductorEta<2>(b2), bsdfConductorK<2>(b2, b3)) * bsdfSpecular<2>(b0)) * model;
  pdf = vis ? fdiv(D * G1i, 4.f * cosWi) : fdiv(D * cH, 4.f * fabsf(woH));
  return true;
}

// One conductor child of a mixture: `child` = its word of the head (bsdf_table.h); a word that names no head of a rough conductor --
// gvpm_upload_bsdfs lets none through -- fails the shift like any unknown index.  f and pdf arrive zero.
__device__ __forceinline__ bool mixtureChildEval(const GatherArgs &a, float child, f3 n, f3 wi, f3 wo, float cosWi, float cosWo, f3 &f,
                                                 float &pdf) {
  const uint32_t ci = (uint32_t)child;
  if (ci >= a.nbsdfs) return false;
  const float4 c0 = a.bsdfs[4 * ci], c1 = a.bsdfs[4 * ci + 1];
  const int ck = bsdfKind(c0);
  if (ck != GVPM_BSDF_ROUGHCONDUCTOR && ck != GVPM_BSDF_ROUGHCONDUCTOR_ANISO) return false;
  return roughConductorEval(a, ci, c0, c1, ck, n, wi, wo, cosWi, cosWo, f, pdf);
}

// The two-component mixture (GVPM_BSDF_MIXTURE; src/bsdfs/mixturebsdf.cpp:177-209,316-319, include/gvpm_hip.h): eval = sum w_i eval_i,
// pdf = sum p_i pdf_i, p_i = w_i / (w_0 + w_1), over both children or over the one the vertex was sampled through (pdf_c times
// pdfComponent = p_c: the same term).  A child is the Lambertian (reflectance = the record's kd), the head of a rough conductor, or
// absent, which contributes nothing (gvpm_upload_bsdfs refuses it where the entry selects it).  A conductor child with D == 0
// contributes zero and the other child still counts; one whose frame is rejected fails the shift.  STRAIGHT-LINE, child 0's conductor,
// child 1's, the Lambertian last, and the head's rows read again between them so that nothing but n, wi, wo and the sums lives
// across a conductor: as a run-time loop over the children it cost the G-BRE evaluation 190 to 280 bytes of scratch per lane, as a
// __noinline__ function 380 (NOTEBOOK.md, "Mixture parents").
__device__ __forceinline__ bool mixtureEval(const GatherArgs &a, uint32_t bi, f3 kd, f3 n, f3 wi, f3 wo, float cosWi, float cosWo, f3 &f,
                                            float &pdf) {
  {
    const float child = bsdfMixtureChild<0>(a.bsdfs[4 * bi + 2]);
    if (bsdfMixtureComponent(a.bsdfs[4 * bi + 1]) != 2 && child >= 0.f && !mixtureChildEval(a, child, n, wi, wo, cosWi, cosWo, f, pdf))
      return false;
  }
  const float4 m0 = a.bsdfs[4 * bi], m1 = a.bsdfs[4 * bi + 1], m2 = a.bsdfs[4 * bi + 2];
  const int comp = bsdfMixtureComponent(m1);  // 0 both, 1 child 0 alone, 2 child 1 alone
  const float w0 = bsdfMixtureWeight<0>(m0), w1 = bsdfMixtureWeight<1>(m0), ip = frcp(w0 + w1);
  f = f * w0;
  pdf *= w0 * ip;
  const float child1 = bsdfMixtureChild<1>(m2);
  if (comp != 1 && child1 >= 0.f) {
    f3 fc = mk3(0.f);
    float pc = 0.f;
    if (!mixtureChildEval(a, child1, n, wi, wo, dot(n, wi), dot(n, wo), fc, pc)) return false;
    const float4 r0 = a.bsdfs[4 * bi];
    f = f + fc * bsdfMixtureWeight<1>(r0);
    pdf += pc * (bsdfMixtureWeight<1>(r0) * frcp(bsdfMixtureWeight<0>(r0) + bsdfMixtureWeight<1>(r0)));
  }
  // the Lambertian child in play (at most one: two are refused), diffuse.cpp:110-127
  const float wl = (comp != 2 && bsdfMixtureChild<0>(m2) == (float)GVPM_MIXTURE_CHILD_DIFFUSE)
                       ? w0
                       : ((comp != 1 && child1 == (float)GVPM_MIXTURE_CHILD_DIFFUSE) ? w1 : 0.f);
  f = f + kd * (INV_PI_F * cosWo * wl);
  pdf += INV_PI_F * cosWo * (wl * ip);
  return true;
}

// A glossy surface parent (GVPM_PARENT_SURFACE_BSDF): BSDF::eval and BSDF::pdf * pdfComponent of the table entry the
// record names, towards the new direction `wo` (shift_diffuse.cpp:25-41 with bRec.component = -1).  Phong, src/bsdfs/
// phong.cpp:121-186: eval = (ks (e + 2) / 2pi alpha^e + kd / pi) cos_o, pdf = w alpha^e (e + 1) / 2pi + (1 - w) cos_o / pi,
// alpha = wo . reflect(wi).  Rough conductor, src/bsdfs/roughconductor.cpp:257-319: eval = F D G / (4 cos_i), pdf = D G1(wi)
// / (4 cos_i) or D cos_H / (4 |wo . H|) (include/gvpm_hip.h).  cosWo > 0 and cosWi != 0 is the caller's test; cosWi < 0 (the
// light arrived on the other side: a transmitted photon) is the rough dielectric's alone, every other kind fails the shift.
// False: no such entry (a failed shift).
// MIX: the kernel evaluates mixture entries (GVPM_BSDF_MIXTURE), dispatched LAST.  Everywhere but in the G-BRE evaluation, whose
// kernels exist in both forms: the one without reads such an entry as no kind, and is launched only where the table holds none
// (gather_bre_eval.hip, launch_evaluate_bre) -- with the arm inlined the kernel of a plain benchmark run spilled 15 VGPRs where it spills 7.
// state (optional out, round 5): bit 0 -- the pdf is POSITIVE in double precision although it underflowed here (the
// specular component of a Phong wall alone, exponent ~1000: alpha^e leaves fp32 below alpha ~ 0.94 and fp64 only below ~0.6;
// with pdf == 0 the reference fails the shift, with a positive one -- however small -- it succeeds, with weight 1 and a
// flux that rounds to zero: only the counter tells them apart); bit 1 -- within rounding of the double's own underflow:
// the exact pass decides, with the lobe in fp64 (phongEvalD).
template <bool MIX = true>
__device__ __forceinline__ bool glossyParentEval(const GatherArgs &a, float index, f3 kd, f3 n, f3 wi, f3 wo, float cosWi,
                                                 float cosWo, f3 &f, float &pdf, uint32_t *state = nullptr) {
  const uint32_t bi = (uint32_t)index;
  f = mk3(0.f);
  pdf = 0.f;
  if (state) *state = 0u;
  if (!(index >= 0.f) || bi >= a.nbsdfs) return false;
  const float4 b0 = a.bsdfs[4 * bi], b1 = a.bsdfs[4 * bi + 1];
  // (a record met from behind, cosWi <= 0, reads as no kind unless its entry is the rough dielectric's: a failed shift)
  const int kind = (cosWi > 0.f || bsdfKind(b0) == GVPM_BSDF_ROUGHDIELECTRIC) ? bsdfKind(b0) : 0;
  if (kind == GVPM_BSDF_PHONG) {
    // (the sampling weight is read as the lane it is: through bsdfSamplingWeight the compiler swaps the operands of a mask
    // `and` in the G-VPM kernels, and this change leaves every instruction where it was -- NOTEBOOK.md)
    const float e = bsdfExponent(b1), w = b1.y;
    const f3 refl = n * (2.f * cosWi) - wi;
    const float alpha = dot(wo, refl);
    const float l2 = alpha > 0.f ? e * __builtin_log2f(alpha) : -INFINITY;
    float lobe = alpha > 0.f ? __builtin_exp2f(l2) : 0.f;  // std::pow(alpha, exponent)
    // (the entry's component: 0 both, 1 the specular lobe alone, 2 the diffuse one alone -- bRec.component + 1; a component's
    // pdf times its pdfComponent IS its term of the mixture, phong.cpp:157-186,331-342)
    const int comp = bsdfPhongComponent(b1);
    const float dOn = comp == 1 ? 0.f : 1.f;
    if (comp == 2) lobe = 0.f;
    f = (bsdfSpecular3(b0) * ((e + 2.f) * INV_TWOPI_F * lobe) + kd * (INV_PI_F * dOn)) * cosWo;
    pdf = w * (lobe * (e + 1.f) * INV_TWOPI_F) + (1.f - w) * (INV_PI_F * cosWo * dOn);
    if (state && comp == 1 && pdf == 0.f && w > 0.f) {
      // the double's lobe is zero below 2^-1074; the factors beside it (w (e + 1) / 2 pi, 1 / l^2, the medium's pdf) move the
      // product's own underflow by a few tens of binades: a band of +-64 around it, and |alpha| within rounding of zero
      *state = (l2 > -1010.f ? 1u : 0u) | ((l2 > -1138.f && l2 <= -1010.f) || fabsf(alpha) <= 1e-6f ? 2u : 0u);
    }
    return true;
  }
  if (kind == GVPM_BSDF_WARD || kind == GVPM_BSDF_WARD_ANISO) {
    // src/bsdfs/ward.cpp:178-266, both components (roughness >= 0.05); H NOT normalised in eval, as the reference has it; the
    // variant rides in the field the rough conductor uses for its pdf's form.  Isotropic: alphaU == alphaV = the head's alpha.
    // Anisotropic: alphaU = the head's alpha, alphaV and the tangent in the frame entry behind the head; alphaU alphaV stands where
    // alpha^2 stood, and the exponent -((H.x / alphaU)^2 + (H.y / alphaV)^2) / H.z^2 is scale-free in H: eval and pdf share it
    const float w = bsdfSamplingWeight(b1);
    const int variant = bsdfWardVariant(b1);
    const f3 H = wi + wo;
    const float HH = dot(H, H), Hz = cosWi + cosWo;
    float ia2, ex;
    if (kind == GVPM_BSDF_WARD) {
      ia2 = frcp(bsdfAlpha(b1) * bsdfAlpha(b1));
      ex = -(HH - Hz * Hz) * frcp(Hz * Hz) * ia2;
    } else {
      const float4 fr = a.bsdfs[4 * (bi + 1)];
      f3 s, t;
      if (!anisoFrame(fr, n, s, t)) return false;
      const float ux = fdiv(dot(H, s), bsdfAlpha(b1)), uy = fdiv(dot(H, t), bsdfFrameAlphaV(fr));
      ia2 = frcp(bsdfAlpha(b1) * bsdfFrameAlphaV(fr));
      ex = -(ux * ux + uy * uy) * frcp(Hz * Hz);
    }
    const float E = __expf(ex);
    float factor1;
    if (variant == GVPM_WARD_WARD) factor1 = INV_FOURPI_F * ia2 * frsq(cosWi * cosWo);
    else if (variant == GVPM_WARD_DUER) factor1 = INV_FOURPI_F * ia2 * frcp(cosWi * cosWo);
    else factor1 = HH * INV_PI_F * ia2 * frcp(Hz * Hz * Hz * Hz);
    const float specRef = factor1 * E;
    f = (bsdfSpecular3(b0) * (specRef > 1e-10f ? specRef : 0.f) + kd * INV_PI_F) * cosWo;
    // pdf: the normalised half vector; Hn . wi = (1 + wi . wo) / |H|, cos(theta_Hn) = Hz / |H|
    const float iH = frsq(HH), cH = Hz * iH, wiH = dot(wi, H) * iH;
    pdf = w * (INV_FOURPI_F * ia2 * E * frcp(wiH * cH * cH * cH)) + (1.f - w) * (INV_PI_F * cosWo);
    return true;
  }
  if (kind == GVPM_BSDF_ROUGHCONDUCTOR || kind == GVPM_BSDF_ROUGHCONDUCTOR_ANISO)
    return roughConductorEval(a, bi, b0, b1, kind, n, wi, wo, cosWi, cosWo, f, pdf);
  if (kind == GVPM_BSDF_ROUGHPLASTIC || kind == GVPM_BSDF_PLASTIC) {
    // src/bsdfs/roughplastic.cpp:326-437,566-586 and the diffuse component of src/bsdfs/plastic.cpp:245-307,451-477
    // (include/gvpm_hip.h): row 2 = {eta, Fdr, -, component met}, row 3 = {nonlinear, ...}; a rough-plastic head is followed by
    // its transmittance slice, 100 contiguous floats (gvpm_upload_bsdfs checked that they are there)
    const float4 b2 = a.bsdfs[4 * bi + 2], b3 = a.bsdfs[4 * bi + 3];
    const float w = bsdfSamplingWeight(b1), eta = bsdfPlasticEta(b2), Fdr = bsdfPlasticFdr(b2);
    const int comp = (int)bsdfPlasticComponent(b2);  // 0 both, 1 the glossy component alone, 2 the diffuse one alone
    float Ti, To, spec = 0.f, pdfM = 0.f;
    if (kind == GVPM_BSDF_ROUGHPLASTIC) {
      const float *slice = reinterpret_cast<const float *>(a.bsdfs + 4 * (bi + 1));
      Ti = roughTransmittance(slice, cosWi);
      To = roughTransmittance(slice, cosWo);
      const float alpha = bsdfAlpha(b1);
      const int dist = bsdfDistribution(b1), vis = bsdfSampleVisible(b1) != 0;
      f3 H = wi + wo;
      H = H * frsq(dot(H, H));
      const float cH = dot(H, n), wiH = dot(wi, H), woH = dot(wo, H);
      const float D = microfacetD(dist, alpha, cH);
      if (D != 0.f && comp != 2) {
        const float G1i = microfacetG1(dist, alpha, cosWi, wiH), G1o = microfacetG1(dist, alpha, cosWo, woH);
        spec = fresnelDielectric(wiH, eta) * fdiv(D * G1i * G1o, 4.f * cosWi);
        pdfM = vis ? fdiv(D * G1i, 4.f * cosWi) : fdiv(D * cH, 4.f * fabsf(woH));
      }
    } else {
      Ti = 1.f - fresnelDielectric(cosWi, eta);
      To = 1.f - fresnelDielectric(cosWo, eta);
    }
    // the probability of the glossy component: 0 / 0 (T = 0 with w = 0, T = 1 with w = 1) is NaN in the reference -- a failed shift
    const float p = 1.f - Ti, den = p * w + (1.f - p) * (1.f - w);
    if (!(den > 0.f)) return false;
    const float pS = fdiv(p * w, den);
    const float dOn = comp == 1 ? 0.f : 1.f;
    const bool nl = bsdfPlasticNonlinear(b3);  // kd / (1 - kd Fdr) per channel, else kd / (1 - Fdr)
    const f3 kdp = mk3(fdiv(kd.x, 1.f - (nl ? kd.x : 1.f) * Fdr), fdiv(kd.y, 1.f - (nl ? kd.y : 1.f) * Fdr),
                       fdiv(kd.z, 1.f - (nl ? kd.z : 1.f) * Fdr));
    const float ie = frcp(eta);
    f = bsdfSpecular3(b0) * spec + kdp * (INV_PI_F * cosWo * Ti * To * (ie * ie) * dOn);
    pdf = pS * pdfM + (1.f - pS) * (INV_PI_F * cosWo * dOn);
    return true;
  }
  if (kind == GVPM_BSDF_ROUGHDIELECTRIC) {
    const float4 r = roughDielectricEval(a.bsdfs + 4 * bi, n, wi, wo, cosWi, cosWo);
    if (r.w < 0.f) return false;
    f = mk3(r.x, r.y, r.z);
    pdf = r.w;
    return true;
  }
  if constexpr (MIX) {
    if (kind == GVPM_BSDF_MIXTURE) return mixtureEval(a, bi, kd, n, wi, wo, cosWi, cosWo, f, pdf);
  }
  return false;
}

// Phong::eval (x cos) and Phong::pdf x pdfComponent of a table entry in fp64 (phong.cpp:121-186,331-342): what the exact
// passes and the fp64 transcription of G-Beams evaluate a Phong parent with -- a lobe of exponent ~1000 lives where fp32 has
// no numbers.  False: not a Phong entry.
__device__ __forceinline__ bool phongEvalD(const GatherArgs &a, float index, d3 kd, d3 n, d3 wi, d3 wo, double cosWi, double cosWo,
                                           d3 &f, double &pdf) {
  const uint32_t bi = (uint32_t)index;
  if (!(index >= 0.f) || bi >= a.nbsdfs) return false;
  const float4 b0 = a.bsdfs[4 * bi], b1 = a.bsdfs[4 * bi + 1];
  if (bsdfKind(b0) != GVPM_BSDF_PHONG || !(cosWi > 0)) return false;  // (cosWi <= 0: glossyParentEval fails the shift)
  const double INV_PI = 0.31830988618379067154, INV_TWOPI = 0.15915494309189533577;
  const double e = bsdfExponent(b1), w = bsdfSamplingWeight(b1);
  const int comp = bsdfPhongComponent(b1);  // 0 both, 1 specular only, 2 diffuse only (gvpm_hip.h, gvpm_bsdf)
  const d3 refl = n * (2.0 * cosWi) - wi;
  const double alpha = dot(wo, refl);
  const double lobe = (alpha > 0 && comp != 2) ? pow(alpha, e) : 0.0, dOn = comp == 1 ? 0.0 : 1.0;
  f = (mkd(bsdfSpecular<0>(b0), bsdfSpecular<1>(b0), bsdfSpecular<2>(b0)) * ((e + 2.0) * INV_TWOPI * lobe) + kd * (INV_PI * dOn)) * cosWo;
  pdf = w * (lobe * (e + 1.0) * INV_TWOPI) + (1.0 - w) * (INV_PI * cosWo * dOn);
  return true;
}

}  // namespace gvpm
