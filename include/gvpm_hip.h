/*
 * gvpm_hip.h -- C ABI of libgvpm_hip.so: the MI355X (gfx950) photon-gather +
 * gradient-domain shift path of the `gvpm` integrator.
 *
 * This is the seam a Mitsuba-side `gvpm` Integrator shim binds instead of the
 * `switch (m_config.volTechnique)` at
 *   src/integrators/photonmapper/gvpm/gvpm.cpp:456-474
 * (computeVolumeGradientPhoton / ...PhotonBRE / ...Beams / ...Planes), and of
 * the per-pixel assembly that follows it (gvpm.cpp:480-532, 1205-1306).
 * All citations below are relative to the reference tree
 * (gvpm/ = src/integrators/photonmapper/gvpm/).
 *
 * Conventions
 *  - plain C, plain pointers and sizes, no torch / HIP types in any signature;
 *  - every call returns int: 0 = GVPM_OK, negative = gvpm_status; the text of
 *    the last failure of a handle is available through gvpm_last_error();
 *    nothing throws or aborts (Mitsuba's SLog(EError) throws; a shim converts);
 *  - the caller owns every host buffer passed in; the library copies during
 *    the call (uploads are synchronous with respect to the host buffer), with
 *    one exception: a buffer in PINNED host memory (gvpm_host_alloc*) is copied
 *    asynchronously on the handle's copy stream and must stay untouched until
 *    the gvpm_gather that consumes it has returned (G-BRE) or, for the other
 *    techniques, until gvpm_synchronize / a download has returned;
 *  - a handle is single-owner (call it from the RenderJob thread only);
 *    kernels are stream-ordered; gvpm_download_* block until results are ready;
 *  - the `_dev` variants take DEVICE pointers (already resident in HBM, e.g.
 *    a torch tensor's data_ptr()) and do no PCIe traffic.  They are BORROWED:
 *    kernels of up to three consecutive steps are in flight at a time (build of
 *    N+2, traversal of N+1, evaluation of N), so a borrowed buffer must stay
 *    untouched until gvpm_synchronize has returned or the SECOND gvpm_gather
 *    after the one that consumed it has returned.
 *
 * All floating-point payload is fp32 (the reference's SCons default
 * SINGLE_PRECISION build, build/config-linux-gcc.py:7); the device computes in
 * fp32.
 */
#ifndef GVPM_HIP_H
#define GVPM_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVPM_ABI_VERSION 3  /* 2: gvpm_bsdf grew to 64 bytes (rough conductor), round 4; 3: gvpm_devgen_scene carries the
                              sensor's rotation (cam_to_world), round 5.  Table kinds and entry points are ADDITIONS and
                              do not bump it (GVPM_BSDF_ROUGHPLASTIC, GVPM_BSDF_PLASTIC, the two _ANISO kinds, GVPM_BSDF_ROUGHDIELECTRIC, GVPM_BSDF_MIXTURE: same 64-byte gvpm_bsdf) */

/* ---- status codes --------------------------------------------------------*/
typedef enum gvpm_status {
  GVPM_OK = 0,
  GVPM_ERR_INVALID_ARG = -1,  /* null pointer, bad enum, inconsistent sizes   */
  GVPM_ERR_NO_DEVICE = -2,    /* no gfx950 device / HIP runtime failure       */
  GVPM_ERR_HIP = -3,          /* a HIP call failed (see gvpm_last_error)      */
  GVPM_ERR_STATE = -4,        /* call order violated (e.g. gather w/o photons)*/
  GVPM_ERR_UNSUPPORTED = -5,  /* flag combination the reference itself rejects
                                 (GPMConfig::load SLog(EError) cases,
                                 gvpm/gvpm_struct.h:291-331) or a branch that
                                 is host-only (manifold shift)                */
  GVPM_ERR_COMM = -6          /* RCCL failure                                 */
} gvpm_status;

/* ---- enums mirrored from the reference -----------------------------------*/
/* EVolumeTechnique, src/integrators/volume_utils.h:12-21 (same order).      */
typedef enum gvpm_technique {
  GVPM_VOL_BRE2D = 0,
  GVPM_VOL_BRE3D = 1,
  GVPM_DISTANCE = 2,          /* G-VPM, 3D point kernel                       */
  GVPM_BEAM_BEAM_1D = 3,
  GVPM_BEAM_BEAM_3D_NAIVE = 4,
  GVPM_BEAM_BEAM_3D_EGSR = 5,
  GVPM_BEAM_BEAM_3D_OPTIMIZED = 6,
  GVPM_VOL_PLANE0D = 7
} gvpm_technique;

/* EPixel, gvpm/gvpm_struct.h:354-359; offsets from generateOffsetPos,
 * gvpm/shift/shift_utilities.h:255-261: L=(-1,0) R=(+1,0) T=(0,+1) B=(0,-1). */
enum { GVPM_LEFT = 0, GVPM_RIGHT = 1, GVPM_TOP = 2, GVPM_BOTTOM = 3 };

/* ELightShiftType, gvpm/gvpm_struct.h:30-37 (values kept).                   */
enum {
  GVPM_SHIFT_ALL = 0,
  GVPM_SHIFT_DIFFUSE = 1 << 1,
  GVPM_SHIFT_MANIFOLD = 1 << 2,
  GVPM_SHIFT_NULL = 1 << 4,
  GVPM_SHIFT_MEDIUM = 1 << 5,
  GVPM_SHIFT_INVALID = 1 << 6
};

/* ELightingEffects, src/integrators/volume_utils.h:94-103.                   */
enum {
  GVPM_SURF2SURF = 1 << 1,
  GVPM_SURF2MEDIA = 1 << 2,
  GVPM_MEDIA2SURF = 1 << 3,
  GVPM_MEDIA2MEDIA = 1 << 4
};

/* BSDF::EBSDFType bits used by bsdfInteractionMode
 * (include/mitsuba/render/bsdf.h; parse in volume_utils.h:120-151).          */
enum {
  GVPM_BSDF_DIFFUSE_REFLECTION = 0x00002,
  GVPM_BSDF_ALL = 0x1FFFF
};

/* ---- photon record flags (one uint32 per photon) -------------------------*/
/* parent = light-path vertex (vertexId-1), the vertex the photon is
 * re-connected from (gvpm/shift/shift_volume_photon.cpp:389-390).            */
#define GVPM_PARENT_EMITTER 0u  /* PathVertex::EEmitterSample (area light)    */
#define GVPM_PARENT_SURFACE 1u  /* ESurfaceInteraction, Lambertian closed set */
#define GVPM_PARENT_MEDIUM 2u   /* EMediumInteraction                         */
#define GVPM_PARENT_SURFACE_BSDF 3u /* ESurfaceInteraction whose BSDF is entry
                                   (uint32_t) parent_g of the table of
                                   gvpm_upload_bsdfs (a glossy parent, round 4);
                                   parent_scat = its diffuse reflectance       */
#define GVPM_PF_PARENT_TYPE(f) ((f) & 3u)
/* result of getTypeShift() (gvpm/shift/shift_utilities.h:112-136) -- a pure
 * function of the light path, evaluated by the host at flattening time:
 * 0 invalid, 1 diffuse, 2 medium, 3 manifold                                 */
#define GVPM_PF_SHIFT_TYPE(f) (((f) >> 2) & 7u)
#define GVPM_PF_EDGE_IN_MEDIUM(f) (((f) >> 5) & 1u) /* edge(vertexId-1)->medium != 0 */
#define GVPM_PF_DEPTH(f) (((f) >> 8) & 0xFFu)        /* vertexId - 1            */
/* getVertexComponentType(vPrev) (shift_utilities.h:219-229), low 16 bits of
 * BSDF::EBSDFType                                                            */
#define GVPM_PF_PREV_COMPONENT(f) (((f) >> 16) & 0xFFFFu)
#define GVPM_PF_MAKE(parent, shift, edge_medium, depth, comp)                  \
  (((uint32_t)(parent) & 3u) | (((uint32_t)(shift) & 7u) << 2) |               \
   (((uint32_t)(edge_medium) & 1u) << 5) | (((uint32_t)(depth) & 0xFFu) << 8) | \
   (((uint32_t)(comp) & 0xFFFFu) << 16))

/* ---- configuration: the GPMConfig flags the kernels read -----------------*/
/* gvpm/gvpm_struct.h:107-333 (same names, snake_case).                       */
typedef struct gvpm_params {
  int32_t abi_version;          /* = GVPM_ABI_VERSION                          */
  int32_t width, height;        /* film crop size                              */
  int32_t vol_technique;        /* gvpm_technique                              */
  int32_t max_depth;            /* maxDepth; <= 0: no limit (the functors test
                                   `config.maxDepth > 0`)                      */
  int32_t min_depth;            /* minDepth                                    */
  int32_t use_mis;              /* useMIS: 1 "area", 0 "none"                  */
  int32_t use_shift_null;       /* useShiftNull                                */
  int32_t path_set;             /* pathSet                                     */
  int32_t power_heuristic;      /* powerHeuristic                              */
  int32_t no_medium_shift;      /* noMediumShift (must be 1: shiftPhotonMedium
                                   is SAssert(false), shift_volume_photon.cpp:307) */
  int32_t use_manifold;         /* useManifold: manifold shifts are host-only;
                                   the device treats them as the reference does
                                   with useManifold=false (failed shift)       */
  int32_t debug_shift;          /* debugShift, ELightShiftType value           */
  int32_t lighting_interaction_mode; /* ELightingEffects bits                 */
  int32_t bsdf_interaction_mode;     /* BSDF type mask, GVPM_BSDF_ALL = "all"  */
  int32_t nb_camera_samples;    /* nbCameraSamples (G-VPM)                     */
  int32_t visibility_as_written;/* 1: shadow ray maxt = lProj*ShadowEpsilon as
                                   written at shift_volume_photon.cpp:396;
                                   0: lProj*(1-ShadowEpsilon)                  */
  float alpha;                  /* alpha (radius reduction), in (0, 1]         */
  float initial_scale_volume;   /* initialScaleVolume                          */
  float bsphere_radius;         /* m_smokeAABB.getBSphere().radius             */
  float epsilon;                /* Epsilon, include/mitsuba/core/constants.h   */
  float shadow_epsilon;         /* ShadowEpsilon                               */
  int32_t reserved[8];
} gvpm_params;

/* ---- medium (homogeneous, "balance" strategy) ----------------------------*/
/* src/medium/homogeneous.cpp:432-513, src/phase/{isotropic,hg}.cpp.          */
/* gvpm_upload_medium accepts: every field finite; sigma_t equal across the
 * channels (else GVPM_ERR_UNSUPPORTED) and > 0; 0 <= sigma_s[c] <= sigma_t[c]
 * (sigma_s may differ per channel); |g| < 1; medium_sampling_weight in (0, 1].
 * Anything else is GVPM_ERR_INVALID_ARG.  No kernel writes a non-finite value
 * for an accepted medium, however thick: a transmittance below 1e-20 is 0 as
 * in the reference, and so is whatever is divided by it.                     */
typedef struct gvpm_medium {
  float sigma_a[3];
  float sigma_s[3];             /* in [0, sigma_t[c]]                          */
  float sigma_t[3];             /* must be equal across channels (:196-200), > 0 */
  float g;                      /* HG mean cosine in (-1, 1), 0 = isotropic    */
  float medium_sampling_weight; /* in (0, 1]; 1 after
                                   computeOnlyVolumeInteraction()              */
  float reserved[5];
} gvpm_medium;

/* ---- glossy surface parents ------------------------------*/
/* diffuseReconnection re-evaluates the BSDF of the vertex a photon is re-connected from towards the offset position
 * (gvpm/shift/operation/shift_diffuse.cpp:25-47: BSDF::eval, BSDF::pdf * pdfComponent with
 * bRec.component = parent->sampledComponentIndex).  The device's closed set: the Lambertian of GVPM_PARENT_SURFACE
 * (src/bsdfs/diffuse.cpp:110-127) and the BSDFs of this table, named by photons of parent type
 * GVPM_PARENT_SURFACE_BSDF through parent_g (an index, stored as a float).
 *   GVPM_BSDF_PHONG  the modified Phong model of src/bsdfs/phong.cpp with BOTH components, i.e. a vertex whose
 *     sampledComponentIndex is -1 -- what PathVertex::sampleNext records for every Phong surface of roughness
 *     sqrt(2 / (2 + exponent)) >= 0.05 (exponent <= 798; vertex.cpp:160-165 with Phong::sampleComponent, phong.cpp:311-330):
 *       eval(wi, wo) = (specular (exponent + 2) / (2 pi) alpha^exponent [alpha > 0] + diffuse / pi) cos(theta_o)   :121-150
 *       pdf(wi, wo)  = w alpha^exponent (exponent + 1) / (2 pi) [alpha > 0] + (1 - w) cos(theta_o) / pi          :157-186
 *     with alpha = wo . reflect(wi), w = specular_sampling_weight, both zero unless cos(theta_i), cos(theta_o) > 0;
 *     pdfComponent = 1.  Such a vertex classifies as DIFFUSE for every roughness above bounceRoughness (default 0.001,
 *     gvpm_struct.h:66-100,232-236): its photons are re-connected through it like through a Lambertian wall.
 *     ONE component (round 5): below roughness 0.05 (exponent > 798) sampleNext picks a component first
 *     (Phong::sampleComponent, phong.cpp:308-329: 0 = the specular lobe with probability w, 1 = the diffuse one) and the
 *     reconnection evaluates THAT component (bRec.component = sampledComponentIndex): eval = its term alone, pdf = its pdf
 *     times pdfComponent (w or 1 - w, :331-342) -- which is the matching term of the mixture above.  Such a vertex names an
 *     entry whose `distribution` field holds component + 1 (0: both, the entries of round 4; 1: specular only; 2: diffuse
 *     only): a surface that can be met both ways has one entry per way.  gvpm_upload_bsdfs does not range-check the field for this
 *     kind: any value other than 1 and 2 reads as both components (GVPM_MICROFACET_PHONG = 3 among them: it is NOT read as a
 *     microfacet distribution here, and is accepted).
 *   GVPM_BSDF_ROUGHCONDUCTOR  src/bsdfs/roughconductor.cpp with an ISOTROPIC Beckmann, GGX or Phong distribution (alphaU == alphaV:
 *     the photon record carries the parent's normal, not its tangent frame) -- one component, EGlossyReflection:
 *       H = normalize(wi + wo), D = MicrofacetDistribution::eval (microfacet.h:191-232), G = smithG1(wi, H) smithG1(wo, H)
 *       (:477-522), F = fresnelConductorExact(wi . H, eta, k) * specular (libcore/util.cpp:747-769)
 *       eval(wi, wo) = F D G / (4 cos(theta_i))                                                                 :257-293
 *       pdf(wi, wo)  = D smithG1(wi, H) / (4 cos(theta_i))  [sample_visible]   or   D cos(theta_H) / (4 |wo . H|)  :295-319
 *     both zero unless cos(theta_i), cos(theta_o) > 0; pdfComponent = 1.  `exponent` carries alpha (after the constructor's
 *     clamp to >= 1e-4, microfacet.h:135-136).  Classified like any vertex by its roughness alpha against bounceRoughness.
 *     THE PHONG DISTRIBUTION (GVPM_MICROFACET_PHONG; the same for every kind that has a `distribution`): with the exponent
 *     e(alpha) = max(2 / alpha^2 - 2, 0) (microfacet.h:700-704),
 *       D(m) = (e + 2) / (2 pi) cos(theta_m)^e,  0 for cos(theta_m) <= 0;  D cos(theta_m) < 1e-20 -> D = 0          (:191-232)
 *       smithG1 = Beckmann's rational form, with alpha and not the exponent                                          (:489-501)
 *     and the pdf is the all-normals form alone: the reference forces sampleVisible off for this distribution (:140-144), and
 *     `sample_visible` != 0 with it is refused (GVPM_ERR_INVALID_ARG).
 *   GVPM_BSDF_WARD (round 5)  src/bsdfs/ward.cpp with alphaU == alphaV (isotropic: the photon record carries the parent's normal,
 *     not its tangent frame) and roughness alpha >= 0.05, i.e. BOTH components (Ward::sampleComponent, ward.cpp:370-389): with
 *     H = wi + wo (NOT normalised, as the reference has it), tan2 = (|H|^2 - H.z^2) / H.z^2, E = exp(-tan2 / alpha^2),
 *       eval = (specular * factor1 * E [if factor1 * E > 1e-10] + diffuse / pi) cos(theta_o)                            :178-228
 *         factor1 = 1 / (4 pi alpha^2 sqrt(cos_i cos_o))      variant 0, "ward"
 *                 = 1 / (4 pi alpha^2 cos_i cos_o)            variant 1, "ward-duer"
 *                 = |H|^2 / (pi alpha^2 H.z^4)                variant 2, "balanced" (the plugin's default)
 *       pdf  = w E / (4 pi alpha^2 (Hn . wi) cos^3(theta_Hn)) + (1 - w) cos(theta_o) / pi,  Hn = H / |H|                :230-266
 *     `exponent` carries alpha, `sample_visible` the variant, `specular_sampling_weight` w; pdfComponent = 1.
 *   GVPM_BSDF_ROUGHPLASTIC  src/bsdfs/roughplastic.cpp:326-437,532-586 with an isotropic, untextured Beckmann, GGX or Phong distribution:
 *     a dielectric coating (component 0, EGlossyReflection) over a diffuse base (component 1, EDiffuseReflection).  With
 *     H = normalize(wi + wo), D, G as for the rough conductor, F = fresnelDielectricExt(wi . H, eta) (libcore/util.cpp:659-689),
 *     T(c) = the external rough transmittance at the surface's eta and alpha (rtrans.h:183-236 after setEta / setAlpha: 100
 *     values over c^(1/4) in [0, 1], evalCubicInterp1D of libcore/spline.cpp:23-60, clamped to [0, 1]) and
 *     Fdr = 1 - the internal diffuse transmittance:
 *       eval(wi, wo) = specular F D G / (4 cos(theta_i)) + kd' / pi cos(theta_o) T(cos_i) T(cos_o) / eta^2
 *         kd' = kd / (1 - kd Fdr) per channel [nonlinear] or kd / (1 - Fdr); kd = the photon's parent_scat
 *       pS = p w / (p w + (1 - p) (1 - w)),  p = 1 - T(cos_i),  w = specular_sampling_weight
 *       pdf(wi, wo)  = pS pdf_m + (1 - pS) cos(theta_o) / pi,  pdf_m = the rough conductor's pdf (either form)
 *     both zero unless cos(theta_i), cos(theta_o) > 0.  Below roughness 0.05 sampleNext picks ONE component (sampleComponent,
 *     :532-564) and the reconnection evaluates that component: eval = its term alone, pdf * pdfComponent = its term of the
 *     mixture above (pdfComponent = pS or 1 - pS, :566-586).  With GVPM_MICROFACET_PHONG, D and G are the rough conductor's for that
 *     distribution, pdf_m = D cos(theta_H) / (4 |wo . H|), and the slice is the one of data/microfacet/phong.dat.  Fields: `specular`, `exponent` = alpha (>= 1e-4), `distribution`,
 *     `sample_visible`, `specular_sampling_weight` as for the rough conductor; eta[0] = eta (>= 1), eta[1] = Fdr (in [0, 1)),
 *     k[0] = the component met, as a float: 0 both, 1 the glossy one alone, 2 the diffuse one alone (sampledComponentIndex + 1);
 *     k[1] = 1 for `nonlinear`, else 0; the rest zero.  THE SLICE follows the entry in the table: the 7 entries behind a
 *     rough-plastic head are raw -- 100 floats T_0..T_99 contiguous (knot j at c^(1/4) = j / 99), then 12 zero words -- and
 *     belong to it: gvpm_upload_bsdfs refuses a head without them and any slice value that is not a normal float or zero in
 *     [0, 1]; photons name HEAD indices only (a raw entry read as a head shows 0 or a word >= 2^23 as its kind: such a photon's
 *     shift fails like any unknown index).  pS = 0 / 0 (T(cos_i) = 0 with w = 0, or T(cos_i) = 1 with w = 1: NaN in the
 *     reference) is a failed shift here.  A cosine that rounding left above 1 is looked up at 1.
 *   GVPM_BSDF_PLASTIC  src/bsdfs/plastic.cpp:245-307,451-477, always met one component at a time.  Its Dirac component is a
 *     specular vertex (nothing reconnects through it); this kind is its DIFFUSE component (k[0] must be 2):
 *       eval = kd' / pi cos(theta_o) (1 - F(cos_i)) (1 - F(cos_o)) / eta^2,  F = fresnelDielectricExt(., eta), kd' as above
 *       pdf * pdfComponent = cos(theta_o) / pi (1 - pS),  pS = F(cos_i) w / (F(cos_i) w + (1 - F(cos_i)) (1 - w))
 *     Fields: eta[0], eta[1] = Fdr (the plugin's closed-form m_fdrInt), k[0] = 2, k[1] = nonlinear,
 *     `specular_sampling_weight`; no slice.
 *   GVPM_BSDF_WARD_ANISO, GVPM_BSDF_ROUGHCONDUCTOR_ANISO  the anisotropic forms of GVPM_BSDF_WARD and GVPM_BSDF_ROUGHCONDUCTOR
 *     (alphaU != alphaV allowed) on a PLANAR surface.  The photon record carries the parent's normal n and no tangent: the
 *     tangent travels per surface in the table.  A head of either kind has the fields of its isotropic sibling, `exponent` =
 *     alphaU, and is followed by ONE raw entry, the frame entry: words 0..2 = s, the world-space tangent of the surface (the
 *     `s` of the intersection's shading frame, the direction alphaU belongs to), word 3 = alphaV, words 4..15 zero.  The
 *     device forms  s' = normalize(s - n (n . s)),  t = n x s'  and, for a vector v,  v.x = v . s', v.y = v . t, v.z = v . n;
 *     only SQUARES of the tangential components enter the formulas below, so neither the sign of s nor the handedness of
 *     (s', t, n) matters.  |s - n (n . s)|^2 < 1e-12 (a tangent parallel to the normal) is a failed shift.
 *       Ward (ward.cpp:178-264): with H = wi + wo (not normalised),  E = exp(-((H.x / alphaU)^2 + (H.y / alphaV)^2) / H.z^2)
 *       (scale-free in H: eval and pdf use the same value), eval and pdf are those of GVPM_BSDF_WARD with alphaU alphaV in
 *       the place of alpha^2 in factor1 and in the pdf; the `factor1 * E > 1e-10` rule is kept.
 *       Rough conductor (roughconductor.cpp:257-319): with m = normalize(wi + wo),
 *         D = exp(-e) / (pi alphaU alphaV cos^4(theta_m))  [Beckmann]   or   1 / (pi alphaU alphaV ((1 + e) cos^2(theta_m))^2)  [GGX],
 *         e = (m.x^2 / alphaU^2 + m.y^2 / alphaV^2) / cos^2(theta_m);  D cos(theta_m) < 1e-20 -> D = 0           (microfacet.h:191-232)
 *         smithG1(v, m) with alpha = projectRoughness(v) = sqrt((v.x^2 alphaU^2 + v.y^2 alphaV^2) / sin^2(theta_v))    (:477-522, :541-551)
 *         (perpendicular incidence returns 1 before the projection), Fresnel and both forms of the pdf as for the isotropic kind.
 *         D = sqrt((eU + 2)(eV + 2)) / (2 pi) cos(theta_m)^e  [GVPM_MICROFACET_PHONG: Ashikhmin-Shirley], eU = e(alphaU), eV = e(alphaV),
 *         e = eU where alphaU == alphaV or sin^2(theta_m) <= 2^-128 (RCPOVERFLOW, constants.h:58), else
 *         e = (eU m.x^2 + eV m.y^2) / sin^2(theta_m) (:553-565); the same cut; smithG1 is Beckmann's at the projected roughness;
 *         the all-normals pdf alone.
 *     gvpm_upload_bsdfs refuses, before anything is copied (GVPM_ERR_INVALID_ARG): a head without its frame entry; a frame
 *     word that is not +0 or a normal float (-0, subnormals, NaN, inf: a raw entry read as a head then shows 0 or a word
 *     >= 2^23 as its kind, never a valid one); | |s| - 1 | > 1e-3; alphaU or alphaV < 1e-4 (the microfacet constructor's clamp,
 *     microfacet.h:88-90; for Ward, whose plugin has no clamp, it is THIS LIBRARY's own limit); Ward: 0.5 (alphaU + alphaV) <
 *     0.05 (Ward::getRoughness, ward.cpp:365, against sampleComponent, :370-389: below it one component is sampled), a
 *     sampling weight outside [0, 1]; GVPM_ERR_UNSUPPORTED: a Ward variant outside 0..2 or `distribution` != 0, a conductor
 *     whose distribution is not Beckmann, GGX or Phong / Ashikhmin-Shirley.  alphaU == alphaV is legal: the isotropic
 *     kind, whatever the tangent.  Photons name HEAD indices only.  GVPM_ANISO_ENTRIES = the raw entries behind such a head.
 *     (7 is not a kind.)
 *   GVPM_BSDF_ROUGHDIELECTRIC  src/bsdfs/roughdielectric.cpp:270-422 with an isotropic, untextured Beckmann, GGX or Phong distribution: the
 *     one kind that TRANSMITS.  RoughDielectric::sampleComponent returns -1 and pdfComponent 1 at every roughness (:647-657), so
 *     there is no entry per component: reflection and transmission are both in play at every vertex.  Two conventions:
 *     (1) THE RECORD'S NORMAL POINTS TO THE SIDE THE PHOTON LEFT: for a record that names an entry of this kind, parent_n is the
 *     surface normal oriented so that dot(parent_n, pos - parent_pos) > 0 (a host that has the shading normal flips it where the
 *     photon was transmitted).  Admissible offset directions then satisfy cos(theta_o) = parent_n . wo > 0 as for every other
 *     surface parent (the reference's sign test, shift_volume_photon.cpp:404-412, keeps the shifted direction on the base's
 *     side), and the photon's class is read off the record: cos(theta_i) = parent_n . parent_wi > 0 is REFLECTION, < 0 is
 *     TRANSMISSION, == 0 gives eval = 0 (:271), a failed shift.
 *     (2) ONE ENTRY PER SIDE OF INCIDENCE: eval and pdf depend on the surface's orientation only through the index wi lies in,
 *     so eta[0] = the index BEHIND the surface divided by the index ON wi's SIDE -- m_eta where the light arrived on the outside,
 *     m_invEta where it arrived inside.  A surface that can be met both ways has two entries; the photon names the entry of the
 *     side it was met from.
 *     With nI = parent_n sign(cos(theta_i)) (the normal on wi's side), ci = |cos(theta_i)|, eta = eta[0] and cosines taken
 *     against nI (cos_o = +-parent_n . wo):
 *       reflection (:279-286, 324-329, 365-375):  H = normalize(wi + wo),
 *         eval = specular F D G / (4 ci),  dwh_dwo = 1 / (4 wo . H)
 *       transmission (:287-298, 330-347, 376-391):  H = normalize(wi + wo eta), flipped into nI's hemisphere,
 *         sD = wi . H + eta wo . H,
 *         eval = k |(1 - F) D G eta^2 (wi . H)(wo . H) / (ci sD^2)|   (mode EImportance: factor = 1),
 *         dwh_dwo = eta^2 (wo . H) / sD^2
 *       F = fresnelDielectricExt(wi . H, eta) (libcore/util.cpp:659-689; wi . H > 0 in wi's frame; total internal reflection: 1),
 *       D = MicrofacetDistribution::eval(H) (microfacet.h:191-232), G = smithG1(wi, H) smithG1(wo, H) with signed cosines
 *       (:477-522: dot(v, m) cosTheta(v) <= 0 gives 0),
 *       pdf = |prob dwh_dwo| (reflection: F, transmission: 1 - F)                                                   (:350-422)
 *         prob = D smithG1(wi, H) |wi . H| / ci  [sample_visible]   or   D' cos(theta_H), D' = the distribution at alpha scaled by
 *         1.2 - 0.2 sqrt(ci) (:406-414), with its own D' cos(theta_H) < 1e-20 -> 0 cut.  GVPM_MICROFACET_PHONG: D as for the rough
 *         conductor, prob = D' cos(theta_H) alone, D' with the exponent recomputed from the scaled alpha (scaleAlpha, microfacet.h:178-183).
 *     D == 0 gives eval = 0, and pdf = 0 with visible normals; without them the pdf is D''s (RoughDielectric::pdf does not look at
 *     D): a half vector between the two cuts is a shift that succeeds with zero flux.  The same holds where G = 0 (a direction no
 *     facet reaches, a facet seen from behind): eval = 0, pdf > 0.  |wi + wo eta|^2 < 1e-12 (no half vector) is a failed shift.
 *     Fields: `specular` = m_specularReflectance, k[0..2] = m_specularTransmittance (both after ensureEnergyConservation),
 *     `exponent` = alpha (>= 1e-4), `distribution`, `sample_visible` as for the rough conductor, eta[0] as above; eta[1], eta[2],
 *     `specular_sampling_weight` and `reserved` zero.  No raw entries behind the head.  gvpm_upload_bsdfs refuses, before anything
 *     is copied (GVPM_ERR_INVALID_ARG): alpha < 1e-4, eta[0] not finite or outside [0.2, 5], a reflectance or transmittance
 *     channel outside [0, 1], a non-zero word where zero is asked, `sample_visible` != 0 with
 *     GVPM_MICROFACET_PHONG; GVPM_ERR_UNSUPPORTED: a distribution that is not Beckmann, GGX or Phong.
 *   GVPM_BSDF_MIXTURE  src/bsdfs/mixturebsdf.cpp as the reference has it: TWO children of one component each (:144-149, :301-314) --
 *     the ordinary way to a glossy-diffuse wall out of single-component plugins, or a blend of two metals.  The children that can
 *     occur are the Lambertian, the rough conductor (isotropic or anisotropic, any distribution) and the smooth conductor (a Dirac
 *     vertex: nothing reconnects through it); Phong, Ward, the plastics and the rough dielectric have two components and the
 *     reference refuses them.  With the weights w_0, w_1 (m_weights AFTER the constructor's rescale where ensureEnergyConservation is
 *     on and they sum above 1, :130-142) and p_i = w_i / (w_0 + w_1) (m_pdf, :171-173):
 *       component -1, both children of roughness >= 0.05:  eval = w_0 eval_0 + w_1 eval_1,  pdf = p_0 pdf_0 + p_1 pdf_1   :177-209
 *       component c, picked by sampleNext where a child is smoother than 0.05 (vertex.cpp:160-180):
 *         eval = w_c eval_c,  pdf * pdfComponent = pdf_c p_c                                                              :316-319
 *     One 64-byte head, no raw entries behind it: specular[0], specular[1] = w_0, w_1 (specular[2] zero); `distribution` = the sampled
 *     component + 1 as for the Phong kind (0 both, 1 child 0 alone, 2 child 1 alone: a surface that can be met both ways has one
 *     head per way); eta[0], eta[1] = the two children; every other word +0.  The device derives p_i from the weights.  A CHILD
 *     WORD is the table index of a GVPM_BSDF_ROUGHCONDUCTOR or GVPM_BSDF_ROUGHCONDUCTOR_ANISO head, as an integer-valued float (as
 *     parent_g carries one; anywhere in the table, before or after the mixture, and it may be shared), or
 *     GVPM_MIXTURE_CHILD_DIFFUSE = -1, the Lambertian (diffuse.cpp:110-127), whose reflectance is the record's parent_scat,
 *     UNWEIGHTED -- the device applies w --, contributing kd / pi cos(theta_o) and cos(theta_o) / pi, or
 *     GVPM_MIXTURE_CHILD_ABSENT = -2, a child the device cannot evaluate (the smooth conductor), legal only where `distribution`
 *     selects the OTHER child.  A conductor child contributes what its own head gives alone (its frame entry, its distribution and
 *     its form of the pdf included); D = 0 there is a zero contribution and the other child still counts; an anisotropic child
 *     whose tangent is parallel to the normal fails the whole shift, as alone.  cos(theta_i) <= 0 is a failed shift.  A vertex with
 *     component -1 is classified by child 0's roughness (gvpm_struct.h:57-64), >= 0.05 then: diffuse at the default bounceRoughness.
 *     gvpm_upload_bsdfs refuses, before anything is copied (GVPM_ERR_INVALID_ARG): a weight that is negative or not finite,
 *     w_0 + w_1 <= 0, `distribution` outside 0..2, a child word that is not -1, -2 or a non-negative integer below the table's
 *     length, a child index that names a raw entry, -2 for a child `distribution` selects or with `distribution` 0, an unused word
 *     that is not +0; GVPM_ERR_UNSUPPORTED: a child head of any other kind (the two-component kinds, a mixture), and BOTH children
 *     -1 -- legal in the reference, but the pdf is cos / pi either way: the host folds it into a plain GVPM_PARENT_SURFACE record of
 *     reflectance w_0 kd_0 + w_1 kd_1.
 *   A record of any OTHER kind with cos(theta_i) <= 0 fails its shift, as ever.
 * A surface parent outside the closed set stays what it was: the host flags the photon's shift type 0 (failed shift).   */
enum { GVPM_BSDF_PHONG = 1, GVPM_BSDF_ROUGHCONDUCTOR = 2, GVPM_BSDF_WARD = 3, GVPM_BSDF_ROUGHPLASTIC = 4, GVPM_BSDF_PLASTIC = 5,
       GVPM_BSDF_WARD_ANISO = 6, GVPM_BSDF_ROUGHCONDUCTOR_ANISO = 8, GVPM_BSDF_ROUGHDIELECTRIC = 9, GVPM_BSDF_MIXTURE = 10 };
#define GVPM_MIXTURE_CHILD_DIFFUSE (-1) /* a mixture's child word: the Lambertian, reflectance = the record's parent_scat    */
#define GVPM_MIXTURE_CHILD_ABSENT (-2)  /* a mixture's child word: not evaluable on the device (the smooth conductor)        */
#define GVPM_ANISO_ENTRIES 1           /* raw table entries behind an anisotropic head (the frame entry)            */
#define GVPM_RTRANS_KNOTS 100          /* values of a rough-plastic slice                                          */
#define GVPM_RTRANS_ENTRIES 7          /* raw table entries behind a rough-plastic head (448 bytes)                */
enum { GVPM_WARD_WARD = 0, GVPM_WARD_DUER = 1, GVPM_WARD_BALANCED = 2 };
/* GVPM_MICROFACET_PHONG: the Phong distribution and, with alphaU != alphaV, Ashikhmin-Shirley's (MicrofacetDistribution::EPhong is 2
 * in microfacet.h:56: the binding maps it).  (2 is not a distribution: gvpm_upload_bsdfs refuses it, GVPM_ERR_UNSUPPORTED.) */
enum { GVPM_MICROFACET_BECKMANN = 0, GVPM_MICROFACET_GGX = 1, GVPM_MICROFACET_PHONG = 3 };
typedef struct gvpm_bsdf {    /* 64 bytes */
  int32_t kind;               /* GVPM_BSDF_*                                                            */
  float specular[3];          /* m_specularReflectance (Phong: after ensureEnergyConservation, phong.cpp:86-91);
                                 mixture: specular[0], specular[1] = the weights w_0, w_1 after the rescale */
  float exponent;             /* Phong: m_exponent; rough conductor, Ward: alpha (the _ANISO kinds: alphaU) */
  float specular_sampling_weight; /* Phong, Ward: m_specularSamplingWeight, phong.cpp:93-97, ward.cpp:158-162 */
  int32_t distribution;       /* rough conductor: GVPM_MICROFACET_*; Phong, mixture: sampled component + 1 (0 = both) */
  int32_t sample_visible;     /* rough conductor: m_sampleVisible (the pdf's form); Ward: GVPM_WARD_* variant */
  float eta[3], k[3];         /* rough conductor: m_eta, m_k (relative to the exterior, roughconductor.cpp:181-191);
                                 plastics: eta[0] = eta, eta[1] = Fdr, k[0] = component met (0 / 1 / 2), k[1] = nonlinear;
                                 rough dielectric: eta[0] = relative index seen from wi's side, k = m_specularTransmittance;
                                 mixture: eta[0], eta[1] = the children (a head index, GVPM_MIXTURE_CHILD_DIFFUSE or _ABSENT) */
  float reserved[2];
} gvpm_bsdf;

/* ---- scene occluders for scene->rayIntersect(Ray) ------------------------*/
/* call sites shift_volume_photon.cpp:398, shift_volume_beams.cpp:421.
 * Triangle i = (v0, v0+e1, v0+e2); arrays of 3*n floats.                     */
typedef struct gvpm_triangles {
  const float *v0, *e1, *e2;
  uint32_t n;
} gvpm_triangles;

/* ---- volume photons: one record per stored light-path vertex -------------*/
/* Host-side flattening of GPhotonNodeData + the Path it points to
 * (gvpm/gvpm_accel.h:17-65,119-199). SoA, n elements per array, 3-vectors
 * packed xyz.  c = vertexId, parent = vertex(c-1).                            */
typedef struct gvpm_photon_soa {
  const float *pos;         /* 3n  vertex(c) position                          */
  const float *wi;          /* 3n  -edge(c-1)->d  (towards the parent)         */
  const float *flux;        /* 3n  GPhotonNodeData::weight                     */
  const float *parent_pos;  /* 3n  vertex(c-1) position                        */
  const float *parent_n;    /* 3n  geometric (= shading) normal of a surface or
                                   emitter parent; ignored for a medium parent */
  const float *prefix_w;    /* 3n  prod_{i<c-1} v_i.weight*v_i.rrWeight*e_i.weight
                                   (shift_volume_photon.cpp:415-422)           */
  const float *parent_scat; /* 3n  surface: diffuse reflectance; medium: sigma_s */
  const float *parent_wi;   /* 3n  unit direction parent -> vertex(c-2)        */
  const float *parent_pdf;  /* n   vertex(c-1)->pdf[EImportance] (area measure) */
  const float *edge_pdf;    /* n   edge(c-1)->pdf[EImportance]                 */
  const float *parent_rr;   /* n   vertex(c-1)->rrWeight                       */
  const float *parent_g;    /* n   HG g of the parent's medium (medium parent) */
  const uint32_t *flags;    /* n   GVPM_PF_*                                   */
  const uint32_t *path_id;  /* n   GPhotonNodeData::pathID                     */
  uint64_t n;
} gvpm_photon_soa;

/* ---- camera beams ---------------------------------------------------------*/
/* One gvpm_camera_ray = one medium edge of a camera path (base, or the same
 * edge of the path re-traced through an offset pixel by
 * ShiftGatherPoint::generate, gvpm/shift/shift_cameraPath.h:29-133), with the
 * SVertexPDF cache entries the functors read (gvpm/gvpm_struct.h:361-370,
 * 585-631).  64 bytes.  A beam SET = 5 consecutive rays: base, L, R, T, B.   */
typedef struct gvpm_camera_ray {
  float o[3];        /* vertex(e) position                                     */
  float len;         /* edge(e)->length                                        */
  float d[3];        /* -edge(e)->d, unit, pointing away from the camera       */
  float pdf;         /* getVertexInfo(e).pdf                                   */
  float eye[3];      /* getWeightBeam(e-1) * getWeightVertex(e)                */
  float jacobian;    /* getVertexInfo(e).jacobian                              */
  float gop;         /* GOp(e) = geometryOpposingTerm(path, e, e+1)            */
  uint32_t info;     /* bit0: validVolumeEdge(e, medium) (always 1 for base);
                        bits 8..15: edge index e                               */
  float rand;        /* base ray only: the sampler->next1D() of this beam
                        (gvpm.cpp:1042 BRE; :1156 VPM)                         */
  uint32_t pixel;    /* base ray only: px | py << 16                           */
} gvpm_camera_ray;

#define GVPM_RAY_VALID(info) ((info) & 1u)
#define GVPM_RAY_EDGE(info) (((info) >> 8) & 0xFFu)
#define GVPM_RAY_INFO(valid, edge) (((uint32_t)(valid) & 1u) | (((uint32_t)(edge) & 0xFFu) << 8))

/* G-VPM only: one record per camera sample (gvpm.cpp:1143-1180).  The host keeps the
 * per-path part of the loop -- the CDF over the medium edges of the pixel's camera path
 * (selBeam, :1117-1129) and sampleReuse (:1148) -- and hands over, per sample, which beam
 * set was selected, the re-used random number that drives sampleDistance(EDistanceAlwaysValid)
 * (:1168) and the selection probability selBeam[sampleIndex].  Samples of one pixel must be
 * consecutive (they are summed in order).                                                  */
typedef struct gvpm_vpm_sample {
  uint32_t set;      /* index of the beam set (pixel, medium edge) in the uploaded rays      */
  float rand;        /* randSample after sampleReuse                                        */
  float pdf_sel;     /* selBeam[sampleIndex]                                                */
  uint32_t reserved;
} gvpm_vpm_sample;

/* ---- per-pixel accumulators (what GatherPoint keeps across iterations) ---*/
/* gvpm/gvpm_struct.h:429-441: mediumFlux, shiftedMediumFlux[4],
 * weightedMediumFlux[4]; each RGB => 27 floats per pixel, row-major pixels.   */
#define GVPM_ACCUM_FLOATS 27

typedef struct gvpm_stats {
  uint64_t evaluations;   /* functor invocations that produced a base
                             contribution + 4 shift attempts       */
  uint64_t candidates;    /* (beam, photon) pairs tested geometrically         */
  uint64_t null_shifts, diffuse_shifts, failed_shifts;
  uint64_t dropped_pairs; /* (photon, beam) pairs the traversal could not store: must be 0 -- gvpm_get_stats returns
                             GVPM_ERR_STATE otherwise (the image would be biased)  */
  uint64_t reserved[2];   /* [0]: G-BRE, the last build's photon cells: kind << 56 | count (low 32 bits); kind 0 = uniform
                             3D grid, 1 = cells over the (u, v) plane of a single-origin ray bundle;
                             bits 32-55: steps whose traversal + evaluation were queued before the planner's counters were
                             known and had to be queued again (a diagnostic, not an error);
                             [1]: packed photon records whose material index lay beyond the uploaded table (decoded with a
                             black parent): must be 0 -- gvpm_get_stats returns GVPM_ERR_STATE otherwise           */
} gvpm_stats;

typedef struct gvpm_context gvpm_context;

/* ---- lifecycle ------------------------------------------------------------*/
/* device: HIP device ordinal.  *out receives the handle.                     */
int gvpm_create(const gvpm_params *params, int device, gvpm_context **out);
int gvpm_destroy(gvpm_context *h);
const char *gvpm_last_error(const gvpm_context *h);
int gvpm_abi_version(void);

/* Reset per-pixel accumulators and the APA radius scale to
 * initialScaleVolume (GPMIntegrator::render, gvpm.cpp:272-291).              */
int gvpm_reset(gvpm_context *h);

/* Decisions.  Every decision of a shift -- null shift or reconnection, the mirror step of getShiftPos, the triangle tests of
 * the shadow segment, the sign / cosine tests of the reconnection -- is taken in fp32 WITH a rigorous error margin; a shift
 * with a comparison inside its margin (~1e-5 of them; for a parent that position rounding left behind the wall it sits
 * on, the reconnections within a few degrees of grazing) is evaluated by the EXACT PASS instead: the reference's statement
 * in fp64 on the same fp32 inputs (csrc/exact_shift.hip for G-BRE and G-VPM, run when the sums are read and every few
 * gathers; csrc/gather_beams.hip exact_beams_kernel for G-Beams, behind every evaluation), so the shift counters of
 * gvpm_stats equal those of a double-precision evaluation of the same inputs exactly (all four techniques; limits:
 * DESIGN.md section 2).  evaluated: shifts the exact passes have taken since gvpm_reset; lost: shifts that did not fit
 * their list (also reported as dropped_pairs: gvpm_get_stats then fails).                                               */
int gvpm_get_exact_shift_count(gvpm_context *h, uint64_t *evaluated, uint64_t *lost);


/* ---- uploads --------------------------------------------------------------*/
int gvpm_upload_scene(gvpm_context *h, const gvpm_triangles *tris);
int gvpm_upload_medium(gvpm_context *h, const gvpm_medium *medium);
/* the BSDF table of the scene's glossy surfaces (once per scene, before the first gather that meets a photon of parent
 * type GVPM_PARENT_SURFACE_BSDF; such a photon with an index beyond the table is a failed shift)                       */
int gvpm_upload_bsdfs(gvpm_context *h, const gvpm_bsdf *table, uint32_t n);
/* per iteration: replaces the proc->getPhotonVolumeMap() of gvpm.cpp:450-454  */
int gvpm_upload_photons(gvpm_context *h, const gvpm_photon_soa *photons);
/* G-Beams, per iteration: replaces proc->getBeamMap() (gvpm.cpp:449).  One record per LTPhotonBeam
 * (gvpm/gvpm_beams.h:18-43), i.e. per medium edge i of a light path, in the photon SoA re-read as:
 *   pos = vertex(i+1) (beam end), parent_* = vertex(i) (beam origin), wi = -edge(i)->d,
 *   flux = LTPhotonBeam::flux (without the transmittance of edge i), prefix_w = prod_{k<i},
 *   parent_pdf = vertex(i)->pdf[EImportance], flags: depth = i, shift type = getTypeShift(path, i+1),
 *   path_id = LTPhotonBeam::pathID;
 * end_n: 3 floats per beam, geometric normal of vertex(i+1), all zero when it is a medium interaction.
 * The beam radius is R*0.01*globalScaleVolume (gvpm.cpp:391,881), kept by the handle.
 * Per-hit randoms (v and w samples of the 3D kernel) are Philox4x32-10 with
 * key = {bits(base ray rand), 0x6265616d}, counter = {beam index, 0, 0, 0}.                    */
int gvpm_upload_beams(gvpm_context *h, const gvpm_photon_soa *beams, const float *end_n);
int gvpm_upload_beams_dev(gvpm_context *h, const gvpm_photon_soa *beams_dev, const float *end_n_dev);
/* G-Planes (0D kernel), per iteration: replaces the LTPhotonPlane list of gvpm.cpp:790-800.  One
 * plane per photon beam (same SoA reading as gvpm_upload_beams: ori = parent_pos, w0 length0 =
 * pos - parent_pos, flux, flags depth = edgeID) plus the second edge drawn by
 * LTPhotonPlane::transformBeam (gvpm/gvpm_plane.h:53-73): w1 (3 floats, unit) and len1 (1 float)
 * per plane.  Preconditions of the reference hold: sensor inside the medium (gvpm.cpp:784-788,
 * i.e. camera rays with medium edge 1), min_depth >= 2 (gvpm.cpp:163-166), no null shift.       */
int gvpm_upload_planes(gvpm_context *h, const gvpm_photon_soa *beams, const float *w1, const float *len1);
int gvpm_upload_planes_dev(gvpm_context *h, const gvpm_photon_soa *beams_dev, const float *w1_dev,
                           const float *len1_dev);
/* per iteration: n_sets beam sets (5 rays each). Replaces GatherPoint[] +
 * ShiftGatherPoint[4] for the medium edges of every pixel.  Sets may come in
 * any order; several sets may address the same pixel (several medium edges). */
int gvpm_upload_camera_beams(gvpm_context *h, const gvpm_camera_ray *rays,
                             uint64_t n_sets);
/* G-VPM: the camera samples of this iteration (n = pixels_with_medium * nbCameraSamples)   */
int gvpm_upload_vpm_samples(gvpm_context *h, const gvpm_vpm_sample *samples, uint64_t n);
/* the same, source buffers already in device memory                          */
int gvpm_upload_photons_dev(gvpm_context *h, const gvpm_photon_soa *photons_dev);
int gvpm_upload_camera_beams_dev(gvpm_context *h,
                                 const gvpm_camera_ray *rays_dev,
                                 uint64_t n_sets);
int gvpm_upload_vpm_samples_dev(gvpm_context *h, const gvpm_vpm_sample *samples_dev, uint64_t n);

/* ---- pipelined uploads -----------------------------------------------------*/
/* Pinned host memory for producers (hipHostMalloc).  gvpm_host_alloc_photons lays ONE block out as the 14 arrays
 * of a photon SoA in the struct's order and returns the view: an upload from it is a single packed copy.           */
int gvpm_host_alloc(uint64_t bytes, void **out);
int gvpm_host_alloc_photons(uint64_t n, gvpm_photon_soa *view, void **block);
int gvpm_host_free(void *p);
/* Start copying the inputs of the step AFTER the coming gvpm_gather (pinned memory only): the copy runs on the copy
 * stream while that gather's kernels run, and the set becomes the current input when that gather returns -- as if
 * gvpm_upload_* had been called at that point.  One pending set per kind.  Loop of a pipelined host:
 *   upload(1); for N: prefetch(N+1); gather(N).                                                                     */
int gvpm_prefetch_photons(gvpm_context *h, const gvpm_photon_soa *photons);
int gvpm_prefetch_camera_beams(gvpm_context *h, const gvpm_camera_ray *rays, uint64_t n_sets);
/* The same for the other techniques' inputs: photon beams with their end normals (G-Beams), photon planes with their second
 * edges (G-Planes), the camera samples of G-VPM.  The side arrays (end_n; w1, len1) travel in the staging slot of their beam
 * records and the samples in a ring of three slots of their own, all copied on the copy stream: an upload from pinned memory
 * is left in flight, one from pageable memory is complete when the call returns.  A prefetched set becomes current when the
 * coming gvpm_gather or gvpm_gather_primal returns.  One pending set per kind (beams, planes and photons are ONE kind: they
 * share the photon slots); at most 2^24 - 1 beams or planes (G-Beams' beam index).
 * Lifetime of a pinned buffer handed to ANY upload or prefetch, side arrays and samples included: untouched until the gather
 * that consumes it has returned, or gvpm_synchronize has.                                                              */
int gvpm_prefetch_beams(gvpm_context *h, const gvpm_photon_soa *beams, const float *end_n);
int gvpm_prefetch_planes(gvpm_context *h, const gvpm_photon_soa *beams, const float *w1, const float *len1);
int gvpm_prefetch_vpm_samples(gvpm_context *h, const gvpm_vpm_sample *samples, uint64_t n);

/* ---- packed uploads (round 3) ----------------------------------------------*/
/* The SoA entry points above move 120 bytes a photon and 320 a beam set over PCIe -- at C2 2.9 times the duration of the
 * step they feed.  These records carry the same inputs in 76 and 272 bytes:
 *   photons  -- wi is not sent: the device forms normalize(parent_pos - pos) (in fp64, rounded once), which is what
 *               -edge(c-1)->d is -- to the rounding of the two fp32 positions: for a photon at distance L from its parent
 *               the derived direction is off by up to ~1e-7 / L rad (L ~ 1e-4, one photon in a thousand at C2: 1e-3 to
 *               1e-2 rad; tests/test_packed_upload.py bounds it).  A host that cannot accept that keeps the SoA upload
 *               (the shim: GVPM_HIP_UPLOAD=soa); parent_n and parent_wi travel as octahedral 2 x snorm16 (axis-aligned vectors are exact,
 *               others are off by <= 4.8e-5 rad (parent_n; parent_wi 5.8e-5): in general position -- tests/test_rotated_gpu.py -- the film's L2
 *               against the fp64 oracle is 8e-6 with packed records, 9e-8 with SoA; a zero vector stays zero); parent_scat and parent_g become an index into a
 *               table of the scene's materials (gvpm_upload_materials); path_id travels as the one bit the gather reads
 *               of it (checkerboard parity, gvpm.cpp:1020-1030) in bit 7 of flags.  Positions, flux, prefix_w and the three
 *               pdfs / weights stay fp32: evaluation counts are those of the SoA upload, bit for bit.
 *   beam set -- the base ray as it is, the four shifted rays without the fields only the base carries (rand, pixel) and
 *               with `info` folded away: valid = !signbit(len), edge = the base ray's.  Lossless.
 * gvpm_pack_* / gvpm_unpack_* are plain host functions (no GPU): a producer packs straight into pinned memory
 * (gvpm_host_alloc), and what a packed upload means is DEFINED by gvpm_unpack_photons -- the device decodes with the same
 * arithmetic, operation for operation.  Reference seam: gvpm/gvpm_accel.h:31-59,119-199 (the fields read back there).     */
typedef struct gvpm_material {
  float scat[3];            /* parent_scat: diffuse reflectance of a surface, sigma_s of a medium */
  float g;                  /* parent_g                                                            */
} gvpm_material;
typedef struct gvpm_photon_packed { /* 76 bytes */
  float pos[3];
  float parent_pdf;
  float parent_pos[3];
  float edge_pdf;
  float flux[3];
  float parent_rr;
  float prefix_w[3];
  uint32_t parent_n_oct;    /* x | y << 16, snorm16 each; 0x80008000: the zero vector            */
  uint32_t parent_wi_oct;
  uint32_t flags;           /* GVPM_PF_* with bit 7 = path_id & 1                                 */
  uint32_t material;        /* index into the table of gvpm_upload_materials                      */
} gvpm_photon_packed;
typedef struct gvpm_ray_packed {    /* 52 bytes: a shifted ray of a beam set */
  float o[3];
  float len;                /* sign bit set: !validVolumeEdge (the magnitude is still the length) */
  float d[3];
  float pdf;
  float eye[3];
  float jacobian;
  float gop;
} gvpm_ray_packed;
typedef struct gvpm_beam_set_packed { /* 272 bytes */
  gvpm_camera_ray base;
  gvpm_ray_packed shifted[4];
} gvpm_beam_set_packed;
/* table / table_n: the materials met so far (in/out, appended to; at most table_cap <= 65536 entries --
 * GVPM_ERR_INVALID_ARG beyond, e.g. a textured scene: such a host keeps the SoA upload).                                  */
int gvpm_pack_photons(const gvpm_photon_soa *src, gvpm_photon_packed *dst, gvpm_material *table, uint32_t table_cap,
                      uint32_t *table_n);
/* dst: 14 writable arrays of src_n elements (the pointers of a gvpm_photon_soa, cast)                                    */
int gvpm_unpack_photons(const gvpm_photon_packed *src, uint64_t n, const gvpm_material *table, uint32_t table_n,
                        const gvpm_photon_soa *dst);
/* GVPM_ERR_INVALID_ARG when a shifted ray's edge index differs from its base ray's                                       */
int gvpm_pack_camera_beams(const gvpm_camera_ray *rays, uint64_t n_sets, gvpm_beam_set_packed *dst);
int gvpm_unpack_camera_beams(const gvpm_beam_set_packed *src, uint64_t n_sets, gvpm_camera_ray *dst);
/* The table may be re-uploaded at any time with MORE entries behind an unchanged prefix (what gvpm_pack_photons' appending
 * produces): that never waits.  Changing existing entries, or growing beyond the allocated capacity, first waits for all
 * work of the handle.  A gather that consumes packed photons without a table fails with GVPM_ERR_STATE.                   */
int gvpm_upload_materials(gvpm_context *h, const gvpm_material *table, uint32_t n);
/* as gvpm_upload_photons / gvpm_prefetch_photons (pageable or pinned memory; prefetch: pinned only)                       */
int gvpm_upload_photons_packed(gvpm_context *h, const gvpm_photon_packed *photons, uint64_t n);
int gvpm_prefetch_photons_packed(gvpm_context *h, const gvpm_photon_packed *photons, uint64_t n);

/* ---- linked photon records (round 6) ---------------------------------------*/
/* The photons of one light path are CONSECUTIVE vertices (GPhotonMap::tryAppend walks the path, gvpm/gvpm_accel.h:119-199):
 * most of what a 76-byte record carries of its parent is already on the wire.  Three record kinds, chosen per photon by the
 * packer, which VERIFIES each choice against the SoA source (a photon that does not fit a short kind travels as a full one):
 *   chain (40 bytes) -- the parent is the medium vertex that IS the previous photon of the upload (same path, MEDIUM parent):
 *                       parent_pos = pos[i-1], prefix_w = flux[i-1] (the path weight up to the parent, bit for bit),
 *                       parent_wi = the previous photon's wi, parent_n = 0, parent_scat / parent_g = entry `component field of
 *                       flags` of the material table; the record keeps pos, flux, the three pdfs / weights, flags;
 *   emit  (48 bytes) -- the parent is an emitter vertex: prefix_w, parent_rr, parent_n, parent_g from entry `component field
 *                       of flags` of the blob's EMITTER table (32 bytes an entry: one per emitter triangle and power),
 *                       parent_scat = 0, parent_wi = (1, 0, 0) as tryAppend leaves them; the record keeps pos, parent_pos,
 *                       flux, parent_pdf, edge_pdf, flags;
 *   full  (76 bytes) -- gvpm_photon_packed, as above.
 * In both short kinds the component field of flags is free (such a parent's component type is always
 * GVPM_BSDF_DIFFUSE_REFLECTION -- verified) and carries the table index.  wi is derived as in the packed records; a chain
 * record's parent_wi is derived from the two positions before it (to the rounding of fp32 positions: tighter than the
 * octahedral code of a full record).  S-cbox / S-fogroom: 28 % chain, 58 % emit, 14 % full = 49.6 bytes a photon.
 * The records travel as ONE blob (one copy): header, 2-bit kinds, per-64-photon bases, emitter table, the three record
 * arrays.  What a blob means is DEFINED by gvpm_unpack_photons_linked; the device decodes with the same arithmetic.  */
typedef struct gvpm_emitter_entry { /* 32 bytes */
  float prefix_w[3];
  float parent_rr;
  float parent_n[3];
  float parent_g;
} gvpm_emitter_entry;
typedef struct gvpm_photon_emit { /* 48 bytes */
  float pos[3];
  float parent_pdf;
  float parent_pos[3];
  float edge_pdf;
  float flux[3];
  uint32_t flags;             /* GVPM_PF_* with bit 7 = path_id & 1; bits 16-31: index into the blob's emitter table */
} gvpm_photon_emit;
typedef struct gvpm_photon_chain { /* 40 bytes */
  float pos[3];
  float parent_pdf;
  float flux[3];
  float edge_pdf;
  float parent_rr;
  uint32_t flags;             /* ... bits 16-31: index into the table of gvpm_upload_materials (the medium parent's) */
} gvpm_photon_chain;
#define GVPM_LINKED_MAGIC 0x4C4E4B31u /* "LNK1" */
#define GVPM_LINKED_FULL 0u
#define GVPM_LINKED_EMIT 1u
#define GVPM_LINKED_CHAIN 2u
typedef struct gvpm_linked_header { /* 64 bytes, at the start of the blob; offsets in bytes from it, 16-byte aligned */
  uint32_t magic, n, n_full, n_emit, n_chain, n_emitters;
  uint32_t off_kinds;         /* ceil(n / 16) words, photon i: bits 2 (i % 16) .. +1                                    */
  uint32_t off_groups;        /* ceil(n / 64) x {full records, emit records before photon 64 g}                         */
  uint32_t off_emitters, off_full, off_emit, off_chain;
  uint32_t bytes;             /* of the whole blob                                                                      */
  uint32_t reserved[3];
} gvpm_linked_header;
/* bytes a blob of n photons can need at most (every photon full, 65536 emitter entries never reached in practice: 1024) */
size_t gvpm_linked_photons_bound(uint64_t n);
/* packs into `blob` (capacity `cap` bytes, e.g. pinned memory of gvpm_linked_photons_bound(n) bytes); the material table grows
 * as in gvpm_pack_photons; *bytes: the blob's size.  GVPM_ERR_INVALID_ARG: capacity or a table exhausted.               */
int gvpm_pack_photons_linked(const gvpm_photon_soa *src, void *blob, size_t cap, gvpm_material *table, uint32_t table_cap,
                             uint32_t *table_n, size_t *bytes);
int gvpm_unpack_photons_linked(const void *blob, size_t bytes, const gvpm_material *table, uint32_t table_n,
                               const gvpm_photon_soa *dst);
int gvpm_upload_photons_linked(gvpm_context *h, const void *blob, size_t bytes);
int gvpm_prefetch_photons_linked(gvpm_context *h, const void *blob, size_t bytes);
int gvpm_upload_camera_beams_packed(gvpm_context *h, const gvpm_beam_set_packed *sets, uint64_t n_sets);
int gvpm_prefetch_camera_beams_packed(gvpm_context *h, const gvpm_beam_set_packed *sets, uint64_t n_sets);

/* ---- compact camera-beam sets (round 4) ------------------------------------*/
/* The beam sets of a frame are most of a step's upload (272 of every 348 bytes at one set per photon-free pixel; 71 of
 * C2's 143.6 MB).  For the FIRST medium edge of a camera path of a perspective sensor nearly all of a set is a function
 * of the sensor: every ray starts on the line through the sensor's origin and its film position, the five film positions
 * share their fractional offset (src/libbidir/vertex.cpp:345-346), eyeContrib = getWeightBeam(e-1) * getWeightVertex(e)
 * is 1 (importance-sampled pinhole, null boundary), and the SVertexPDF entries enter the gather only through
 * GatherPoint::sensorMIS (gvpm/gvpm_struct.h:608-631) = (pdf_s / pdf_b) * jacobian_s, where ShiftGatherPoint::trace /
 * generate DEFINE jacobian_s as the reciprocal of that pdf ratio (shift_cameraPath.h:76-116,191-242: jacobian = pdf1/pdf2 *
 * GOpBase/GOpNew against pdf = pdf2 * GOpNew; pdf2 == 0 replaces pdf2 by pdf1 in BOTH) -- the product is 1.  Such a set
 * travels as 60 bytes: pixel, the sample's fractional film offset, the base ray's random number, a validity mask, and per
 * ray the distance from the sensor's origin to the start of the edge (0 when the sensor sits in the medium) and the edge's
 * length.  The device rebuilds the five rays from the sensor (gvpm_upload_sensor); deeper edges (behind a mirror or a
 * rough vertex: their eye weight, origin and Jacobians are the path's) keep the full 272-byte records and ride along in the
 * same upload.  What a compact set MEANS is defined by gvpm_unpack_camera_beams_compact, with which the device agrees bit
 * for bit (fp64, no contraction).  Against the producer's own fp32 rays the decoded ones differ by rounding only: d is the
 * sensor direction rounded once; o = fp32(origin + t0 * d) moves along the ray by the rounding of t0 (<= 6e-8 relative)
 * and off it by half an ulp, as the producer's own fp32 o does against the exact ray; pdf = jacobian = gop = 1 carry the
 * product above exactly where the producer's fp32 factors carry it to a few ulp.                                           */
typedef struct gvpm_sensor {
  double pos[3];            /* sensor origin, world space                                                                 */
  double to_world[9];       /* row-major rotation camera -> world; camera space looks along -z, +x to the right of the
                               film, +y towards larger pixel rows (a shim folds Mitsuba's flips into it)                  */
  double tan_half_fov_x, tan_half_fov_y;
  int32_t width, height;    /* film size in pixels                                                                        */
  int32_t reserved[4];
} gvpm_sensor;
/* direction through film position (sx, sy), in pixels:
 *   c = ((2 sx / width - 1) tan_half_fov_x, (2 sy / height - 1) tan_half_fov_y, -1);  d = to_world * (c / |c|)          */
typedef struct gvpm_beam_set_compact { /* 60 bytes */
  uint32_t pixel;           /* px | py << 16 of the base path                                                             */
  float jitter[2];          /* film position of the base sample minus (px, py), in [0, 1); shifted path k samples
                               (px, py) + offset_k + jitter, offsets L R T B = (-1,0) (+1,0) (0,+1) (0,-1)                */
  float rand;               /* the base ray's `rand`                                                                      */
  uint32_t info;            /* bit k (0 base, 1..4 L R T B): validVolumeEdge of ray k; bits 8..15: edge index e           */
  float t0[5];              /* |vertex(e) - sensor origin| per ray                                                        */
  float len[5];             /* edge(e)->length per ray                                                                    */
} gvpm_beam_set_compact;
int gvpm_upload_sensor(gvpm_context *h, const gvpm_sensor *sensor);
/* Splits n_sets beam sets (5 rays each) into compact records and full packed records.  jitter: 2 floats per set.  A set
 * goes to `compact` iff its decode reproduces the five rays (o, d within 4 ulp of their magnitude, len, validity and edge
 * exactly), every eye weight is 1 and every valid shifted ray has |pdf_s / pdf_b * jacobian_s - 1| <= 1e-4; otherwise to
 * `full`.  Both outputs need room for n_sets records.  new_index (n_sets entries, may be NULL): the index a set has in the
 * upload made of the two lists -- compact sets first, in input order, then the full ones (G-VPM samples and shift
 * requests name sets by that index).                                                                                     */
int gvpm_pack_camera_beams_compact(const gvpm_sensor *sensor, const gvpm_camera_ray *rays, const float *jitter,
                                   uint64_t n_sets, gvpm_beam_set_compact *compact, uint64_t *n_compact,
                                   gvpm_beam_set_packed *full, uint64_t *n_full, uint32_t *new_index);
/* dst: 5 * n_compact rays                                                                                                */
int gvpm_unpack_camera_beams_compact(const gvpm_sensor *sensor, const gvpm_beam_set_compact *src, uint64_t n_compact,
                                     gvpm_camera_ray *dst);
/* as gvpm_upload_camera_beams_packed / gvpm_prefetch_camera_beams_packed: the upload holds n_compact + n_full sets       */
int gvpm_upload_camera_beams_compact(gvpm_context *h, const gvpm_beam_set_compact *compact, uint64_t n_compact,
                                     const gvpm_beam_set_packed *full, uint64_t n_full);
int gvpm_prefetch_camera_beams_compact(gvpm_context *h, const gvpm_beam_set_compact *compact, uint64_t n_compact,
                                       const gvpm_beam_set_packed *full, uint64_t n_full);

/* ---- packed photon beams, photon planes and G-VPM samples ------------------------------------------------------------*/
/* Photon beams and planes are photon SoAs re-read (gvpm_upload_beams): gvpm_pack_photons_linked packs them as they stand --
 * it verifies every short record against the source, the gathers read `path_id & 1` only, and a beam's wi IS
 * normalize(parent_pos - pos), which the decoder derives.  What a blob means is gvpm_unpack_photons_linked's.
 *   beams  -- the end normals travel as one octahedral code per beam (the code of parent_n_oct: 2 x snorm16; 0x80008000 is
 *             the zero vector a medium end vertex carries; axis-aligned normals are exact, others within 4.8e-5 rad:
 *             gvpm_pack_normals_oct picks the nearest of the four codes around a normal, 4.3e-5 rad at worst).  What
 *             the codes mean is DEFINED by gvpm_unpack_normals_oct; the device decodes with the same arithmetic.
 *   planes -- w1 and len1 stay fp32 (lossless); only the beam records are packed.
 *   G-VPM samples -- the samples of a pixel are consecutive and share `set` and `pdf_sel`: they travel as RUNS plus one
 *             `float rand` per sample.  Sample first + k (k < count) of a run is {set, rands[first + k], pdf_sel, 0}; the
 *             runs are contiguous from sample 0 (first of run r + 1 = first + count of run r), none is empty, and their
 *             counts sum to n.  Lossless; 4 + 16 / nb_camera_samples bytes a sample where a pixel has one medium edge.
 *             gvpm_pack_vpm_samples forms maximal runs of equal `set` and bit-equal `pdf_sel` (runs_cap entries of room:
 *             n always suffice) and refuses a sample whose `reserved` is not 0; gvpm_unpack_vpm_samples DEFINES the
 *             meaning and refuses a run list that breaks the rules above; the uploads run the same check on the host
 *             before anything is copied (GVPM_ERR_INVALID_ARG: the previous samples stay in force).
 * The prefetch twins take pinned memory only, as gvpm_prefetch_photons.                                                  */
typedef struct gvpm_vpm_run { /* 16 bytes */
  uint32_t set;
  float pdf_sel;
  uint32_t first;             /* index of the run's first sample                                                          */
  uint32_t count;
} gvpm_vpm_run;
int gvpm_pack_normals_oct(const float *normals, uint64_t n, uint32_t *codes);     /* 3 floats -> 1 code, n times            */
int gvpm_unpack_normals_oct(const uint32_t *codes, uint64_t n, float *normals);
int gvpm_pack_vpm_samples(const gvpm_vpm_sample *samples, uint64_t n, gvpm_vpm_run *runs, uint64_t runs_cap,
                          uint64_t *n_runs, float *rands);
int gvpm_unpack_vpm_samples(const gvpm_vpm_run *runs, uint64_t n_runs, const float *rands, uint64_t n,
                            gvpm_vpm_sample *dst);
int gvpm_upload_beams_linked(gvpm_context *h, const void *blob, size_t bytes, const uint32_t *end_n_oct);
int gvpm_prefetch_beams_linked(gvpm_context *h, const void *blob, size_t bytes, const uint32_t *end_n_oct);
int gvpm_upload_planes_linked(gvpm_context *h, const void *blob, size_t bytes, const float *w1, const float *len1);
int gvpm_prefetch_planes_linked(gvpm_context *h, const void *blob, size_t bytes, const float *w1, const float *len1);
int gvpm_upload_vpm_samples_packed(gvpm_context *h, const gvpm_vpm_run *runs, uint64_t n_runs, const float *rands,
                                   uint64_t n);
int gvpm_prefetch_vpm_samples_packed(gvpm_context *h, const gvpm_vpm_run *runs, uint64_t n_runs, const float *rands,
                                     uint64_t n);

/* ---- read-back of decoded inputs (for tests and debugging; not part of a render loop) --------------------------------*/
/* What the LAST gather read, as the device decoded it, before the next upload into the same staging slot.  Both wait for
 * every stream of the handle, then copy.  GVPM_ERR_STATE before the first gather.
 * gvpm_download_photons: the photon SoA in upload order; dst holds 14 writable host arrays of dst->n elements, and dst->n
 *   must be that gather's photon count (GVPM_ERR_INVALID_ARG otherwise).
 * gvpm_download_camera_beams: the camera rays, five per set, in the device's set order (compact sets first, then the full
 *   ones: new_index of gvpm_pack_camera_beams_compact); min(cap, *n) sets are copied, *n = the gather's set count.       */
int gvpm_download_photons(gvpm_context *h, const gvpm_photon_soa *dst);
int gvpm_download_camera_beams(gvpm_context *h, gvpm_camera_ray *dst, uint64_t cap, uint64_t *n);
/* gvpm_download_beam_sides: the side arrays of that gather's beams, one entry per photon of gvpm_download_photons --
 *   after a G-Beams gather the end normals into vec3_out (3 floats a beam; len1_out is not touched and may be NULL), after
 *   a G-Planes gather w1 into vec3_out and len1 into len1_out.  GVPM_ERR_STATE after a gather of another technique.
 * gvpm_download_vpm_samples: the G-VPM samples; min(cap, *n) are copied, *n = the gather's sample count (GVPM_ERR_STATE
 *   when the last gather was not a G-VPM one).                                                                           */
int gvpm_download_beam_sides(gvpm_context *h, float *vec3_out, float *len1_out);
int gvpm_download_vpm_samples(gvpm_context *h, gvpm_vpm_sample *dst, uint64_t cap, uint64_t *n);

/* ---- manifold shifts through the host (first slice) ----------------------------------------*/
/* A photon whose shift type is 3 (EManifoldShift: a specular chain between the photon and the vertex it can be re-connected
 * from) needs the manifold walk of shiftPhotonManifold (shift_volume_photon.cpp:160-295: generateShiftPathME + ShiftME,
 * shift/operation/shift_ME.cpp:13-142, SpecularManifold::det, src/libbidir/mut_manifold.cpp:1310-1410) -- Newton iterations
 * over Mitsuba's Path / BSDF objects that stay on the host.  With use_manifold = 0 such a shift is a failed shift (weight 1),
 * as in the reference.  With use_manifold = 1 and gvpm_enable_host_shifts(h, capacity > 0), a G-BRE, (round 4) G-VPM
 * (VolumeGradientPositionQuery reaches the same dispatch, shift_volume_photon.cpp:489-655 -> :49-117) or G-Beams gather
 * (shiftBeamME, shift_volume_beams.cpp:601-746; see the request's and the answer's G-Beams notes) instead RECORDS
 * one request per (photon, beam, shifted pixel) that reaches shiftPhotonManifold -- everything the walk takes as input -- and
 * adds nothing for it; the host runs the walk for each request and hands the results back; the device then applies
 * shift_volume_photon.cpp:217-279 (contribution, Jacobian, MIS weight) and adds the terms to the iteration:
 *     gvpm_gather(it) -> gvpm_download_shift_requests -> [host: manifold walks] -> gvpm_upload_host_shifts
 * Requests the host never answers (the next gvpm_gather or download comes first), and requests beyond `capacity`, count as
 * failed shifts.                                                                                                          */
typedef struct gvpm_shift_request { /* 64 bytes */
  uint32_t photon;          /* index into this iteration's photon (G-Beams: beam) upload: lightPath / vertexId = c of the
                               walk (G-Beams: beam->path, c = edgeID + 1)                                                 */
  uint32_t set;             /* beam set (upload order) and ...                                                            */
  uint32_t shift;           /* ... which of its shifted rays: 0..3 = L R T B                                              */
  uint32_t reserved;        /* G-Beams: the bits of the float kRec.pdf() (pdfEdgeFailure * pdfKernel), the pdf
                               cacheSourcePath gives the re-cut last edge of the source path (shift_volume_beams.cpp:574)  */
  float offset_pos[3];      /* offsetPos (getShiftPos, :858-896; G-Beams: newPos): where vertex c of the proposal lies    */
  float radius;             /* photonRadius (the host multiplies by its config.relaxME); G-VPM: the pixel's own radius   */
  float base_point[3];      /* baseRay(baseRay.maxt); G-Beams: baseCameraRay(shiftW - mint), as generateShiftPathME is
                               handed it (shift_volume_beams.cpp:627)                                                     */
  float t;                  /* baseRay.maxt = shiftRay.maxt = t'; G-Beams: shiftW = kRec.w                                */
  float shift_point[3];     /* shiftRay(shiftRay.maxt); G-Beams: shiftRay(shiftW - mint) (:628)                           */
  float reserved2;          /* G-Beams: kRec.v, the kernel's place on the beam (cacheSourcePath moves vertex c there)      */
} gvpm_shift_request;
typedef struct gvpm_host_shift {    /* 40 bytes */
  uint32_t ok;              /* generateShiftPathME && ShiftME succeeded                                                    */
  float throughput[3];      /* sRecME.throughtput                                                                          */
  float wi[3];              /* normalize(proposal.vertex(c-1)->getPosition() - offsetPos); G-Beams: NOT normalised --
                               proposal.vertex(c-1)->getPosition() - newPos, i.e. -edge(c-1)->d * edge(c-1)->length: kernelPDF
                               (shift_volume_beams.cpp:653-656) needs the proposal's last edge whole                       */
  float pdf;                /* sRecME.pdf                                                                                  */
  float det_ratio;          /* manifold->det(proposal, b, c) / manifold->det(source, b, c) (G-Beams: of the cached source) */
  float base_pdf;           /* prod_{i=b}^{c-1} source.vertex(i)->pdf[EImportance] * source.edge(i)->pdf[EImportance]      */
} gvpm_host_shift;
int gvpm_enable_host_shifts(gvpm_context *h, uint64_t capacity);   /* 0: off (the default)                                 */
/* waits for the gather; *n = requests recorded (at most capacity), the first min(*n, cap) of them copied to `out`        */
int gvpm_download_shift_requests(gvpm_context *h, gvpm_shift_request *out, uint64_t cap, uint64_t *n);
/* results[k] answers request k; n must be the number of recorded requests                                                */
int gvpm_upload_host_shifts(gvpm_context *h, const gvpm_host_shift *results, uint64_t n);

/* ---- the hot path ---------------------------------------------------------*/
/* One SPPM iteration of computeVolumeGradientPhotonBRE (gvpm.cpp:988-1079;
 * vol_technique BRE2D/BRE3D): builds the acceleration structure over the
 * uploaded photons, gathers every uploaded beam set, normalises by nb_paths,
 * folds the result into the APA running mean with iteration `it` (1-based) and
 * applies scaleVolumeAPA(it) (gvpm.cpp:181-215).
 * vol_technique DISTANCE: computeVolumeGradientPhoton (gvpm.cpp:1081-1203):
 * gathers every uploaded camera sample with the per-pixel radius
 * R*0.01*scaleVol, ADDS the result (x 1/nbCameraSamples) to the accumulators
 * (plain sums; gvpm_download_film divides by the total emitted path count as
 * gvpm.cpp:489-492 does) and applies the per-pixel SPPM update of scaleVol /
 * NVol (:1191-1195).
 * vol_technique BEAM_BEAM_1D / BEAM_BEAM_3D_OPTIMIZED: computeVolumeGradientBeams
 * (gvpm.cpp:880-986) over the uploaded photon beams (APA fold as for BRE).
 * Asynchronous on the handle's stream.                                        */
int gvpm_gather(gvpm_context *h, int it, uint64_t nb_paths);

/* ---- primal estimators (second half) -----------------------*/
/* One iteration of the PRIMAL volume pass of the reference's `sppm` integrator (src/integrators/photonmapper/sppm.cpp) for
 * the handle's vol_technique, over the SAME uploads, grids, planners and traversals as gvpm_gather -- the primal estimators
 * are the gradient functors' base terms with the conventions below -- with GatherPoint::fluxVol as the result: the first
 * three of a pixel's 27 accumulators (gvpm_download_accum; the other 24 stay zero).  Inputs re-read as:
 *   photons  pos, wi = -Photon::getDirection(), flux = Photon::getPower() (what Mitsuba's compressed record DEcodes to,
 *            include/mitsuba/render/photon.h:86-135), flags depth = Photon::getDepth(); the parent fields are not read;
 *   beams    (gvpm_upload_beams) as for gvpm_gather: PhotonBeam origin / end / flux / depth;
 *   camera   the BASE ray of each set = one Beam{p1, p2, weight, depth} of a gather point: o = p1, d, len = |p2 - p1|,
 *            eye = beam.weight, edge = beam.depth, rand, pixel (sppm.cpp:949-981); the four shifted rays are ignored.
 * BRE2D / BRE3D  volumePhotonPassBRE (sppm.cpp:882-1000) with BeamRadianceEstimator::query (bre.cpp:166-254) on the
 *   estimator built with cameraHeuristic = true (sppm.cpp:927: the gradient pass's uniform radius): per hit
 *     Tr(t') * power * phase(wi, -d) / kernelVolume * (1 / nb_paths) [* max(2 deltaT, 1e-4), 3D] * beam.weight
 *   on the ray re-based at r(mint), WITHOUT the sigma_s factor of the gradient functor, one random number PER HIT for the
 *   3D kernel -- Philox4x32-10, key = {bits(base ray rand), 0x70726d6c}, counter = {bits(pos.x), bits(pos.y), bits(pos.z),
 *   0} of the photon (the reference draws from a stateful per-thread sampler in traversal order) -- and a far check for the
 *   2D kernel (:240-242).  APA fold of sppm.cpp:986 and scaleVolumeAPA(it) (sppm.cpp:255-285 = gvpm.cpp:181-215).
 * DISTANCE  the point estimate (sppm.cpp:1040-1126) with PhotonMap::estimateVolumeRadiance (librender/photonmap.cpp:277-330)
 *   per camera sample of gvpm_upload_vpm_samples: sum(power * phase) * beam.weight * Tr / (pdfSuccess * sel) * MCNorm /
 *   kernelVolume added to fluxVol (plain sums, as gvpm_gather does for this technique), M = the photons that pass the
 *   radius AND the depth test (`maxDepth > 0 &&`: a bound of zero or less filters nothing, as written), then the SPPM
 *   update of scaleVol / NVol (:1116-1120).
 * BEAM_BEAM_1D / BEAM_BEAM_3D_OPTIMIZED  volumePhotonPassBeams (sppm.cpp:762-880) with BeamRadianceQuery (pm/beams.h:29-223):
 *   the gradient pass's kernel record (shift_volume_beams.h:157-290) with the camera transmittance over [Epsilon, w]
 *   instead of [0, w]; the per-hit random numbers are gvpm_upload_beams' Philox stand-in; APA fold as for BRE.
 * max_depth filters as the queries' maxDepth = m_maxDepth - beam.depth does.  GVPM_ERR_UNSUPPORTED when the handle carries a
 * filter the primal passes do not have (path_set, debug_shift, min_depth, interaction modes) and for PLANE0D / the _NAIVE /
 * _EGSR beam kernels.  gvpm_stats.evaluations counts the accepted pairs.                                              */
int gvpm_gather_primal(gvpm_context *h, int it, uint64_t nb_paths);

/* current kernel radius R*0.01*globalScaleVolume (gvpm.cpp:989)              */
int gvpm_get_radius(gvpm_context *h, float *radius);
int gvpm_set_global_scale(gvpm_context *h, float global_scale_volume);
int gvpm_get_stats(gvpm_context *h, gvpm_stats *out);
/* G-VPM per-pixel SPPM state (GatherPoint::scaleVol / NVol), width*height floats each */
int gvpm_download_vpm_state(gvpm_context *h, float *scale_vol, float *n_vol);
/* average duration in ms of the gather kernel launches since the last call,
 * measured with HIP events on the handle's stream, and their number          */
int gvpm_get_kernel_time(gvpm_context *h, float *avg_ms, uint32_t *launches);
/* the same for one phase of gvpm_gather: 0 = dominant kernel (as above; G-BRE: the evaluation
 * kernel), 1 = G-BRE traversal kernel, 2 = build (photon grid, beam sort, planner)             */
int gvpm_get_phase_time(gvpm_context *h, int phase, float *avg_ms, uint32_t *launches);

/* ---- results --------------------------------------------------------------*/
/* 27 floats per pixel (GVPM_ACCUM_FLOATS), width*height pixels               */
int gvpm_download_accum(gvpm_context *h, float *accum);
/* the same into DEVICE memory (e.g. a tensor that torch.distributed all-reduces) */
int gvpm_download_accum_dev(gvpm_context *h, float *accum_dev);
/* throughput (gvpm.cpp:480-500 with reusePrimal :503-532 when reuse_primal)
 * and the gradient images of computeGradient (gvpm.cpp:1205-1306), each
 * width*height*3 floats; emission may be NULL (else added as emission/it).   */
int gvpm_download_film(gvpm_context *h, int it, int reuse_primal,
                       const float *emission, float *throughput, float *dx,
                       float *dy);
/* the same three images, back to back (throughput | dx | dy, 9*width*height
 * floats) in DEVICE memory on the context's stream: what an image-sharded rank
 * hands to the film all-reduce and gvpm_poisson_solve_dev.  emission_dev may
 * be NULL.  Asynchronous: film_dev must not be in flight on another stream, and
 * gvpm_synchronize orders it before a consumer on one.                         */
int gvpm_download_film_dev(gvpm_context *h, int it, int reuse_primal,
                           const float *emission_dev, float *film_dev);
int gvpm_synchronize(gvpm_context *h);

/* ---- reconstruction -----------------------------------*/
/* Screened-Poisson reconstruction of the final image from throughput + gradients: replaces
 * poisson::Solver as gvpm.cpp:610-690 drives it (importImagesMTS, setupBackend, solveIndirect,
 * exportImagesMTS; src/integrators/poisson_solver/Solver.cpp:376-497, Backend.cpp:154-384).
 * The fields are Solver::Params' solver configuration (Solver.hpp:81-88); cg_precond must be 0
 * (no preset of the reference enables the preconditioner).                                    */
typedef struct gvpm_poisson_params {
  float alpha;               /* weight of the primal image, reconstructAlpha (0.2)   */
  int32_t irls_iter_max;     /* 1 = L2, > 1 = L1 by IRLS                              */
  float irls_reg_init;
  float irls_reg_iter;
  int32_t cg_iter_max;
  int32_t cg_iter_check;
  int32_t cg_precond;
  float cg_tolerance;
} gvpm_poisson_params;
/* Solver::Params::setConfigPreset (Solver.cpp:91-164): "L1D", "L1Q", "L1L", "L2D", "L2Q";
 * alpha is set to the reference's default 0.2.  GVPM_ERR_INVALID_ARG for an unknown preset.   */
int gvpm_poisson_preset(const char *preset, gvpm_poisson_params *out);
/* dx, dy, throughput, direct (may be NULL), out: width*height*3 floats, RGB triplets, row major.
 * out = reconstruction (+ direct), i.e. what exportImagesMTS returns.                          */
int gvpm_poisson_solve(gvpm_context *h, const gvpm_poisson_params *params, int width, int height,
                       const float *dx, const float *dy, const float *throughput, const float *direct,
                       float *out);
/* the same with every image in device memory (a device-side producer)      */
int gvpm_poisson_solve_dev(gvpm_context *h, const gvpm_poisson_params *params, int width, int height,
                           const float *dx, const float *dy, const float *throughput,
                           const float *direct, float *out);

/* ---- device-side producers for closed-form scenes -------*/
/* Photon shooting (GPMIntegrator's photon pass: gvpm_proc.cpp:125-209,278-350 with GPhotonMap::tryAppend /
 * LTBeamMap::tryAppendLT flattening) and camera-beam generation (randomWalkFromPixelToFirstDiffuse +
 * ShiftGatherPoint::generate, gvpm_gatherpoint.h:22-170, shift_cameraPath.h:29-133) on the GPU for scenes the
 * device can intersect itself: a triangle list, the materials of the host generators (Lambertian / index-matched / mirror
 * through gvpm_devgen_create, every glossy kind through gvpm_devgen_create_ex), one quad area light, one homogeneous medium, a
 * pinhole sensor.  The outputs are device-resident and go straight into
 * gvpm_upload_photons_dev / gvpm_upload_beams_dev / gvpm_upload_camera_beams_dev: nothing crosses PCIe.
 * Same counter-based streams as the host generators of gvpm_amd/host (keyed by path / pixel index), so the
 * device reproduces the sequential host loop: same photon count, same path count, same order.              */
typedef struct gvpm_devgen_scene {
  uint32_t n_tris, n_mats;
  const double *tris;        /* 12 per triangle: v0, e1, e2, geometric normal   */
  const int32_t *tri_mat;    /* material index per triangle                      */
  const int32_t *mat_kind;   /* 0 Lambertian, 1 index-matched medium boundary, 2 mirror; 3..11 with gvpm_devgen_create_ex */
  const double *mat_albedo;  /* 3 per material                                   */
  double light_c[3], light_u[3], light_v[3], light_n[3], radiance[3], light_area;
  gvpm_medium medium;
  double cam_pos[3], tan_half_fov_x;
  int32_t width, height;
  uint32_t seed;
  int32_t camera_inside;     /* sensor inside the medium: edge 1 is the medium edge */
  int32_t max_depth, rr_depth, min_depth;  /* GPMConfig maxDepth, rrDepth, minDepth */
  double camera_sphere;      /* world units (gvpm.cpp:162)                        */
  double cam_to_world[9];    /* row-major rotation camera -> world (camera space looks along -z, +x to the right of the
                                film, +y towards larger pixel rows: gvpm_sensor's to_world); ALL ZERO = identity (ABI 3) */
} gvpm_devgen_scene;
typedef struct gvpm_devgen gvpm_devgen;
/* gvpm_devgen_create walks the closed set Lambertian (0) / index-matched boundary (1) / mirror (2) and refuses every other
 * mat_kind with GVPM_ERR_UNSUPPORTED; scene and kinds are validated on the host before the device is touched.            */
int gvpm_devgen_create(const gvpm_devgen_scene *scene, int device, gvpm_devgen **out);
/* What a material carries beyond its kind and albedo (scene->mat_kind, scene->mat_albedo): the parameters of the glossy kinds, so that
 * the device generators walk every material the host generators of gvpm_amd/host walk.  mat_kind may then be any kind of the host
 * walk: 3 Phong, 4 rough conductor, 5 Ward, 6 rough plastic, 7 plastic, 8 anisotropic Ward, 9 anisotropic rough conductor, 10 rough
 * dielectric, 11 two-child mixture.  Each sampler follows the reference lines quoted here (and, with the arithmetic, in
 * gvpm_amd/host/synth_core.h); component selection is PathVertex::sampleNext's (vertex.cpp:160-180) for every kind.
 *   spec         Phong (phong.cpp:188-247), Ward (ward.cpp:268-327), conductor (roughconductor.cpp:321-389), plastics (roughplastic.cpp:
 *                439-501, plastic.cpp:451-466): the specular reflectance; rough dielectric (roughdielectric.cpp:513-617): the specular
 *                reflectance
 *   exponent     Phong: the exponent (one component per bounce where sqrt(2 / (2 + exponent)) < 0.05, phong.cpp:293-329); every
 *                other kind: alpha, alphaU of the anisotropic kinds; mixture: the smaller of its children's roughnesses
 *   spec_weight  m_specularSamplingWeight (phong.cpp:93-97, ward.cpp, roughplastic.cpp:532-564, plastic.cpp:451-466)
 *   bsdf         index of the material's first head in the table of gvpm_upload_bsdfs (-1: none): what the records' parent_g name.
 *                Phong / rough plastic / mixture below roughness 0.05: a head per component met; rough dielectric: bsdf = met
 *                from the front, the next head = met from the back
 *   eta, k       conductor: the complex index per channel (fresnelConductorExact, util.cpp:747-769); rough dielectric: k = the
 *                specular transmittance
 *   distribution the microfacet kinds: GVPM_MICROFACET_* (MicrofacetDistribution::sampleAll, microfacet.h:287-375, without
 *                visible normals); Ward: GVPM_WARD_* (ward.cpp:230-266)
 *   coat_eta     plastics: the coating's relative index; rough dielectric: m_eta, the index below the front over the index above
 *   fdr          plastics: Fdr (rough: with its slice, roughplastic.cpp:439-501; smooth: m_fdrInt, plastic.cpp); nonlinear: m_nonlinear
 *   rtrans       rough plastic: its transmittance slice, GVPM_RTRANS_KNOTS values in [0, 1] (RoughTransmittance::eval at fixed eta
 *                and alpha, rtrans.h:183-236); read during the call and copied to device memory the generator owns; NULL for
 *                every other kind
 *   alpha_v, tangent   the anisotropic kinds: alphaV and the surface's unit tangent in world space, the direction alphaU belongs to
 *                (ward.cpp:289-306, microfacet.h:287-347); the rules of the table's frame entry hold
 *   child, mix_w the mixture (mixturebsdf.cpp:247-314): two materials of this scene out of Lambertian / rough conductor of either
 *                form, and their weights after the constructor's rescale
 *   reserved     zero
 * gvpm_devgen_create_ex validates scene and materials on the host BEFORE the device is touched, so every refusal is reached on a
 * machine without a GPU, where a well-formed scene returns GVPM_ERR_NO_DEVICE.  GVPM_ERR_INVALID_ARG: n_mats != scene->n_mats, an
 * unknown kind, a non-zero reserved word, a rough plastic without its slice or with a slice value outside [0, 1] or not finite, an
 * anisotropic kind whose tangent is not a unit vector to 1e-3 or whose alphaU / alphaV is below 1e-4, a mixture child index out of
 * range, mixture weights that are negative, not finite or sum to zero, a `bsdf` below -1.  GVPM_ERR_UNSUPPORTED: a microfacet `distribution` that is not Beckmann, GGX or Phong, a Ward variant outside
 * GVPM_WARD_*, a mixture child that is not Lambertian or a rough conductor of either form.  gvpm_devgen_last_error() names the
 * refusal of the calling thread's last gvpm_devgen_create / _ex ("" after a success).
 * A generator made here launches the closed-set kernels when no material is above kind 2 -- bit for bit gvpm_devgen_create's output --
 * and the glossy unit's kernels otherwise.                                                                                          */
typedef struct gvpm_devgen_material {
  double spec[3];
  double exponent, spec_weight;
  double eta[3], k[3];
  double coat_eta, fdr;
  double alpha_v, tangent[3];
  double mix_w[2];
  const float *rtrans;
  int32_t bsdf, distribution, nonlinear;
  int32_t child[2];
  int32_t reserved[3];
} gvpm_devgen_material;
int gvpm_devgen_create_ex(const gvpm_devgen_scene *scene, const gvpm_devgen_material *mats, uint32_t n_mats, int device,
                          gvpm_devgen **out);
const char *gvpm_devgen_last_error(void);
int gvpm_devgen_destroy(gvpm_devgen *g);
/* shoots light paths 0, 1, 2, ... of `iteration` until `capacity` photons are stored; *dev_soa receives device
 * pointers owned by the generator, *nb_paths the number of paths shot.  The generator rotates THREE output sets per
 * kind (photons / beams, camera rays): an output stays untouched during the two following calls of its kind, which
 * is what the borrowing rule of the `_dev` uploads needs (kernels of three steps in flight)                       */
int gvpm_devgen_shoot_photons(gvpm_devgen *g, int iteration, uint64_t capacity, gvpm_photon_soa *dev_soa,
                              uint64_t *nb_paths);
/* photon beams (one record per medium edge, see gvpm_upload_beams) + the end normals                           */
int gvpm_devgen_shoot_beams(gvpm_devgen *g, int iteration, uint64_t capacity, gvpm_photon_soa *dev_soa,
                            const float **end_n_dev, uint64_t *nb_paths);
/* beam sets (5 rays each) of the pixels whose 4x4 tile t has t % tile_mod == tile_rem (1, 0: the whole frame),
 * row-major pixel order; *rays_dev is owned by the generator (one of three buffers used in turn, see above)        */
int gvpm_devgen_camera_beams(gvpm_devgen *g, int iteration, int tile_mod, int tile_rem,
                             const gvpm_camera_ray **rays_dev, uint64_t *n_sets);
/* copies `bytes` of a generator output back to the host (inspection, tests)                                     */
int gvpm_devgen_read(gvpm_devgen *g, const void *dev, void *host, uint64_t bytes);

/* ---- multi-GPU (image-tile sharding) --------------------------*/
/* Each rank gathers only the beam sets of its own pixels; before
 * reconstruction the 27-float accumulators (disjoint supports) are summed
 * across ranks.  comm_id is the 128-byte ncclUniqueId produced on rank 0 by
 * gvpm_comm_unique_id and distributed by the host (e.g. torch.distributed).  */
int gvpm_comm_unique_id(void *id128);
int gvpm_comm_init(gvpm_context *h, const void *id128, int rank, int world);
int gvpm_allreduce_accum(gvpm_context *h);
/* SURVEY 8e's collective: sum the 3 film planes (gvpm_download_film_dev's
 * layout, 9*width*height floats) in place.  computeGradient adds one term from
 * the pixel and one from its +x / +y neighbour (gvpm.cpp:1223,1266), so the sum
 * of the ranks' partial films is bit-identical to the single-GPU film for dx, dy
 * and throughput; with reuse_primal the throughput's 8-term sum is associated
 * differently (a few ulp).  A third of gvpm_allreduce_accum's bytes.            */
int gvpm_allreduce_film(gvpm_context *h, float *film_dev);

#ifdef __cplusplus
}
#endif
#endif /* GVPM_HIP_H */
