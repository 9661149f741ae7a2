/* C ABI of libgvpm_host.so: synthetic hosts (scene, light paths, camera beams)
 * and the GPMIntegrator mirror.  Used by bench.py / tests through ctypes and
 * by C++ callers directly. */
#ifndef GVPM_HOST_API_H
#define GVPM_HOST_API_H
#include "../../include/gvpm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct gvpm_synth gvpm_synth;
gvpm_synth *gvpm_synth_create(const char *scene, int width, int height, uint32_t seed);
void gvpm_synth_destroy(gvpm_synth *s);
/* the scene as the device-side generators take it (gvpm_devgen_create, include/gvpm_hip.h); the arrays stay owned by `s` */
int gvpm_synth_devgen_scene(gvpm_synth *s, gvpm_devgen_scene *out);
/* GPMConfig minDepth of the light-path walk (0 at create): the photon flattening stores path vertices from index max(minDepth + 1, 2),
 * the beam flattening edges from index max(minDepth, 1) (GPhotonMap::tryAppend, LTBeamMap::tryAppendLT) -- at 2 no record is reconnected
 * from the emitter.  Host generators, gvpm_synth_params and gvpm_synth_devgen_scene all carry it.  GVPM_ERR_INVALID_ARG outside
 * [0, maxDepth). */
int gvpm_synth_set_min_depth(gvpm_synth *s, int min_depth);
/* the scene's materials beyond kind and albedo, as gvpm_devgen_create_ex takes them: `n` = the scene's material count (n_mats of
 * gvpm_synth_devgen_scene; GVPM_ERR_INVALID_ARG otherwise); a slice pointer stays owned by `s`.  GVPM_ERR_STATE, and nothing written,
 * when a rough-plastic material has no transmittance slice yet (gvpm_synth_set_rtrans) -- where the shoot calls fail too */
int gvpm_synth_devgen_materials(const gvpm_synth *s, gvpm_devgen_material *out, uint32_t n);
int gvpm_synth_params(const gvpm_synth *s, gvpm_params *out);
int gvpm_synth_medium(const gvpm_synth *s, gvpm_medium *out);
int gvpm_synth_triangles(gvpm_synth *s, gvpm_triangles *out);
/* shoots light paths of iteration `it` until `capacity` photons are stored;
 * *out points into buffers owned by `s` (valid until the next shoot) */
uint64_t gvpm_synth_shoot(gvpm_synth *s, int it, uint64_t capacity, gvpm_photon_soa *out,
                          uint64_t *nb_paths);
/* (both shoot calls return UINT64_MAX, and store nothing, when a rough-plastic material of the scene has no transmittance
 * slice yet: gvpm_synth_set_rtrans) */
/* photon beams of iteration `it` (see gvpm_upload_beams); *end_n: 3 floats per beam */
uint64_t gvpm_synth_shoot_beams(gvpm_synth *s, int it, uint64_t capacity, gvpm_photon_soa *out,
                                const float **end_n, uint64_t *nb_paths);
/* the beam sets of the 4x4-pixel tiles t with t % tile_mod == tile_rem, whole frame (image-sharded ranks) */
uint64_t gvpm_synth_beams_interleaved(gvpm_synth *s, int it, int tile_mod, int tile_rem, const gvpm_camera_ray **out);
/* photon planes for the beams of the LAST gvpm_synth_shoot_beams call (see gvpm_upload_planes) */
uint64_t gvpm_synth_planes(gvpm_synth *s, int it, const float **w1, const float **len1);
/* camera beam sets of the pixel rectangle; returns the number of sets */
uint64_t gvpm_synth_beams(gvpm_synth *s, int it, int x0, int y0, int x1, int y1,
                          const gvpm_camera_ray **out);
/* rough-plastic materials (scenes cbox_roughplastic*): the material indices, in table order (at most cap written; returns
 * their number), and the setter of a material's transmittance slice -- n = GVPM_RTRANS_KNOTS values in [0, 1] over
 * cos^(1/4) -- and Fdr (include/gvpm_hip.h, GVPM_BSDF_ROUGHPLASTIC).  The slice is derived from the reference renderer's data
 * files and comes from the caller.  GVPM_ERR_INVALID_ARG: not such a material, n or a value out of range. */
uint32_t gvpm_synth_rtrans_materials(const gvpm_synth *s, int32_t *mats, int32_t *distribution, float *alpha, float *eta, uint32_t cap);
int gvpm_synth_set_rtrans(gvpm_synth *s, int mat, const float *values, int n, float fdr);
/* A TEST HOOK, not something a renderer needs: it lets the chi-square tests drive the walk's own sampling code instead of a
 * copy of it.  One bounce off plastic material `mat` exactly as the light-path walk takes it (synth_core.h samplePlastic): unit normal n,
 * unit wi (towards the previous vertex), the vertex's two random numbers.  Returns 1 and wo, weight (eval / pdf), pdf
 * (solid angle; discrete for the Dirac component, *component = 0 then) and the sampled component (-1: both were in play),
 * 0 when the sample is lost, GVPM_ERR_INVALID_ARG for another kind of material or a missing slice. */
int gvpm_synth_sample_plastic(const gvpm_synth *s, int mat, const double *n, const double *wi, double u1, double u2, double *wo,
                              double *weight, double *pdf, int *component);
/* A TEST HOOK like gvpm_synth_sample_plastic, for the isotropic rough-conductor materials (scenes cbox_conductor,
 * cbox_conductor_phong; synth_core.h sampleConductor).  Returns 1 and wo, weight (eval / pdf), pdf (solid angle), 0 when the
 * sample is lost, GVPM_ERR_INVALID_ARG for another kind of material. */
int gvpm_synth_sample_conductor(const gvpm_synth *s, int mat, const double *n, const double *wi, double u1, double u2, double *wo,
                                double *weight, double *pdf);
/* A TEST HOOK like gvpm_synth_sample_plastic, for the anisotropic Ward / rough-conductor materials (scenes cbox_ward_aniso,
 * cbox_conductor_aniso; synth_core.h sampleAniso): one bounce with the material's own tangent and alphas.  Returns 1 and wo,
 * weight (eval / pdf), pdf (solid angle), 0 when the sample is lost (a tangent parallel to n among the reasons),
 * GVPM_ERR_INVALID_ARG for another kind of material. */
int gvpm_synth_sample_aniso(const gvpm_synth *s, int mat, const double *n, const double *wi, double u1, double u2, double *wo,
                            double *weight, double *pdf);
/* A TEST HOOK like gvpm_synth_sample_plastic, for the rough-dielectric material (scenes cbox_roughglass*; synth_core.h
 * sampleDielectric): one bounce off or through the surface whose FRONT normal is n, wi on either side of it; u3 = the random
 * number of the reflect / transmit choice.  Returns 1 and wo, weight, pdf (solid angle), *component = the sampled type
 * (0x8 EGlossyReflection, 0x10 EGlossyTransmission); 0 when the sample is lost; GVPM_ERR_INVALID_ARG for another kind of material. */
int gvpm_synth_sample_dielectric(const gvpm_synth *s, int mat, const double *n, const double *wi, double u1, double u2, double u3,
                                 double *wo, double *weight, double *pdf, int *component);
/* A TEST HOOK like gvpm_synth_sample_plastic, for the mixture materials (scenes cbox_mixture*; synth_core.h sampleMixture): one bounce
 * as the light-path walk takes it, component selection included.  Returns 1 and wo, weight, pdf (solid angle, pdfComponent in it),
 * *component = the child the vertex was sampled through (-1: both were in play), *type = the sampled lobe's type (0x2
 * EDiffuseReflection, 0x8 EGlossyReflection); 0 when the sample is lost; GVPM_ERR_INVALID_ARG for another kind of material. */
int gvpm_synth_sample_mixture(const gvpm_synth *s, int mat, const double *n, const double *wi, double u1, double u2, double *wo,
                              double *weight, double *pdf, int *component, int *type);
/* the two children (material indices) and weights of mixture material `mat`; returns the index of its first table entry, or
 * GVPM_ERR_INVALID_ARG for another kind of material */
int gvpm_synth_mixture(const gvpm_synth *s, int mat, int32_t *children, double *weights);
/* the BSDF table of the scene's glossy walls (a rough-plastic head is followed by the raw entries of its slice, an anisotropic head by its
 * frame entry), in the order the photons' parent_g name them (gvpm_upload_bsdfs);
 * returns the number of entries (at most cap are written) */
uint32_t gvpm_synth_bsdfs(const gvpm_synth *s, gvpm_bsdf *out, uint32_t cap);
/* self-check of the streaming flattening the device generator uses (StreamPath, synth_core.h) against flattenPath /
 * flattenBeams on the same `n_paths` light paths of `iteration`: the number of paths whose records differ in any bit
 * (0 = identical); *n_records: records compared */
uint64_t gvpm_synth_stream_check(gvpm_synth *s, int iteration, uint64_t n_paths, int beams, uint64_t *n_records);
/* the scene's pinhole sensor as the compact beam sets take it (gvpm_upload_sensor, include/gvpm_hip.h) */
int gvpm_synth_sensor(const gvpm_synth *s, gvpm_sensor *out);
/* the fractional film offsets (2 floats per set) the base paths of `rays` (5 per set) of iteration `it` were sampled at:
 * the first two draws of the pixel's stream (cameraBeamSets, synth_core.h) -- what a Mitsuba host reads off its sample
 * position; the second argument of gvpm_pack_camera_beams_compact */
int gvpm_synth_jitter(const gvpm_synth *s, int it, const gvpm_camera_ray *rays, uint64_t n_sets, float *out);
/* G-VPM camera samples for the beam sets of the LAST gvpm_synth_beams call */
uint64_t gvpm_synth_vpm_samples(gvpm_synth *s, int it, int nb_camera_samples, const gvpm_vpm_sample **out);
#ifdef __cplusplus
}
#endif
#endif
