// Device-side producers for the closed-form synthetic scenes: photon shooting and camera-beam
// generation on the GPU, so that an iteration's inputs never cross PCIe (204 MB per iteration at C2, about twice
// the gather's step time).  The per-path / per-pixel logic is the host generator's, compiled from the same source
// (host/synth_core.h); here it runs one light path or one pixel per lane.
//
// Order.  The host loop appends the photons of path 0, 1, 2, ... until `capacity` is reached (GPhotonMap::tryAppend
// semantics, gvpm_proc.cpp:278-350) and reports how many paths it shot.  The device reproduces exactly that: a batch
// of paths is walked once to COUNT its photons, an exclusive scan gives every path its slot, a one-lane search finds
// the path at which the capacity is reached, and the batch is walked again to WRITE (recomputing a path is cheaper
// than parking ~4 KB of records per lane).  Camera beam sets are compacted the same way (pixels in row-major order).
// The output is the C ABI's device-resident SoA (gvpm_upload_photons_dev / gvpm_upload_camera_beams_dev).
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "../../include/gvpm_hip.h"
#include "../host/synth_core.h"
#include "device_types.h"
#include "scan_sort.h"
#include "synth_device_launch.h"

// the walk and camera-beam kernels of the closed set (Lambertian / index-matched / mirror) and their launchers; the same text with
// the glossy materials compiled in is synth_device_glossy.hip's
#define GVPM_SYNTH_K(name) GVPM_SYNTH_PLAIN(name)
#include "synth_walk_kernels.inc"

namespace gvpm {

namespace {

template <typename T> struct Buf {
  T *p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct PhotonOut {
  float *v3[8];  // pos wi flux parent_pos parent_n prefix_w parent_scat parent_wi
  float *f1[4];  // parent_pdf edge_pdf parent_rr parent_g
  uint32_t *flags, *pathId;
  float *endN;
};

// ctl: [0] photons stored before this batch, [1] paths counted before, [2] paths with photons before,
//      [3] (out) paths of this batch that the host loop would have processed
__global__ void synth_stop_kernel(const uint32_t *counts, const uint32_t *offs, const uint32_t *countedOffs,
                                  const uint32_t *counted, const uint32_t *neOffs, const uint32_t *nonEmpty, uint32_t m,
                                  uint64_t capacity, uint32_t *ctl) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint64_t before = ctl[0];
  // first k with before + offs[k] + counts[k] >= capacity
  uint32_t lo = 0, hi = m;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (before + offs[mid] + counts[mid] >= capacity) hi = mid;
    else lo = mid + 1;
  }
  const uint32_t processed = lo < m ? lo + 1u : m;
  const uint32_t last = processed - 1u;
  ctl[3] = processed;
  const uint64_t stored = before + offs[last] + counts[last];
  ctl[4] = (uint32_t)(stored < capacity ? stored : capacity);
  ctl[5] = ctl[1] + countedOffs[last] + counted[last];
  ctl[6] = ctl[2] + neOffs[last] + nonEmpty[last];
}

// one lane per (path, record slot): the parked records of the paths the host loop would have processed -> the output
__global__ __launch_bounds__(256) void synth_place_kernel(const float *__restrict__ park, int stride, const uint32_t *__restrict__ counts,
                                                          const uint32_t *__restrict__ offs, const uint32_t *__restrict__ neOffs,
                                                          const uint32_t *__restrict__ ctl, uint32_t m, uint64_t capacity, PhotonOut o) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t k = t / (uint32_t)stride, q = t % (uint32_t)stride;
  if (k >= m || k >= ctl[3] || q >= counts[k]) return;
  const uint64_t i = (uint64_t)ctl[0] + offs[k] + q;
  if (i >= capacity) return;
  const float *d = park + ((size_t)k * stride + q) * PARK_WORDS;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    o.v3[a][3 * i] = d[3 * a];
    o.v3[a][3 * i + 1] = d[3 * a + 1];
    o.v3[a][3 * i + 2] = d[3 * a + 2];
  }
  if (o.endN) {
    o.endN[3 * i] = d[24];
    o.endN[3 * i + 1] = d[25];
    o.endN[3 * i + 2] = d[26];
  }
  o.f1[0][i] = d[27];
  o.f1[1][i] = d[28];
  o.f1[2][i] = d[29];
  o.f1[3][i] = d[30];
  o.flags[i] = __float_as_uint(d[31]);
  o.pathId[i] = ctl[2] + neOffs[k];
}


}  // namespace
}  // namespace gvpm

#include "synth_camera_kernels.inc"

using namespace gvpm;

struct gvpm_devgen {
  int device = 0;
  hipStream_t stream = nullptr;
  SceneView view;
  Buf<SynthTri> tris;
  Buf<SynthMat> mats;
  Buf<float> slices;    // the rough plastics' transmittance slices, GVPM_RTRANS_KNOTS floats each: what the device SynthMats' rtrans point at
  bool glossy = false;  // a material above MAT_MIRROR: the glossy unit's kernels (synth_device_glossy.hip)
  Buf<uint32_t> counts, counted, nonEmpty, offs, countedOffs, neOffs, ctl;
  Buf<float> park;  // parked records of a batch's paths (synth_walk_kernel)
  // Outputs are BORROWED by the gather context (gvpm_upload_*_dev), whose kernels of up to three consecutive steps are
  // in flight: three output sets per kind, used in turn, so that a call never writes what the two steps before it read.
  struct PhotonOut {
    Buf<float> f3[8], f1[4], endN;
    Buf<uint32_t> flags, pathId;
  } pout[3];
  int poutIdx = 0, raysIdx = 0;
  PhotonOut &po() { return pout[poutIdx]; }
  Buf<uint32_t> pixFlag, pixOffs;
  Buf<gvpm_camera_ray> raysOut[3];
  SortTemp scanTmp;
  uint32_t *pinned = nullptr;  // 8 words, mapped host memory
  double pathsPerPhoton = 0.0;  // light paths walked per stored photon in the last shoot
};

#define SY_TRY(expr)                         \
  do {                                       \
    hipError_t _e = (expr);                  \
    if (_e != hipSuccess) return GVPM_ERR_HIP; \
  } while (0)

extern "C" {

// ---- create: everything is validated on the host before the device is touched ----
static thread_local const char *devgenError = "";
static int refuse(int rc, const char *msg) {
  devgenError = msg;
  return rc;
}
const char *gvpm_devgen_last_error(void) { return devgenError; }

// the scene's own rules (both entry points)
static int checkScene(const gvpm_devgen_scene *sc, gvpm_devgen **out) {
  if (!sc || !out) return refuse(GVPM_ERR_INVALID_ARG, "null scene or output pointer");
  if (sc->n_tris && (!sc->tris || !sc->tri_mat)) return refuse(GVPM_ERR_INVALID_ARG, "null triangle arrays");
  if (sc->n_mats && (!sc->mat_kind || !sc->mat_albedo)) return refuse(GVPM_ERR_INVALID_ARG, "null material arrays");
  if (sc->max_depth + 1 > GVPM_SYNTH_MAXV || sc->width <= 0 || sc->height <= 0)
    return refuse(GVPM_ERR_INVALID_ARG, "max_depth beyond the walk's vertex limit, or an empty frame");
  for (uint32_t i = 0; i < sc->n_tris; ++i)
    if (sc->tri_mat[i] < 0 || (uint32_t)sc->tri_mat[i] >= sc->n_mats) return refuse(GVPM_ERR_INVALID_ARG, "a triangle's material index is out of range");
  return GVPM_OK;
}

// One material of gvpm_devgen_create_ex (include/gvpm_hip.h): the rules, in the order they are reported -- what the table of
// gvpm_upload_bsdfs asks of the same kinds (bsdf_table.h), in its words.
static int checkMaterial(const gvpm_devgen_scene *sc, const gvpm_devgen_material *mats, uint32_t i) {
  const int kind = sc->mat_kind[i];
  const gvpm_devgen_material &m = mats[i];
  if (kind < MAT_LAMBERT || kind > MAT_MIXTURE) return refuse(GVPM_ERR_INVALID_ARG, "material kind outside the generators' set (0 .. 11)");
  if (m.reserved[0] | m.reserved[1] | m.reserved[2]) return refuse(GVPM_ERR_INVALID_ARG, "material: the reserved words are zero");
  if (kind == MAT_ROUGHPLASTIC) {
    if (!m.rtrans) return refuse(GVPM_ERR_INVALID_ARG, "rough plastic: the transmittance slice is missing");
    for (int j = 0; j < GVPM_RTRANS_KNOTS; ++j)
      if (!(m.rtrans[j] >= 0.f && m.rtrans[j] <= 1.f)) return refuse(GVPM_ERR_INVALID_ARG, "rough plastic: slice values are finite and in [0, 1]");
  }
  if (kind == MAT_WARD_ANISO || kind == MAT_ROUGHCONDUCTOR_ANISO) {
    const double sl = std::sqrt(m.tangent[0] * m.tangent[0] + m.tangent[1] * m.tangent[1] + m.tangent[2] * m.tangent[2]);
    if (!(std::fabs(sl - 1.0) <= 1e-3)) return refuse(GVPM_ERR_INVALID_ARG, "anisotropic Ward / rough conductor: the tangent is a unit vector (to 1e-3)");
    if (!bsdfAlphaValid((float)m.exponent) || !bsdfAlphaValid((float)m.alpha_v))
      return refuse(GVPM_ERR_INVALID_ARG, "anisotropic Ward / rough conductor: alphaU, alphaV >= 1e-4");
  }
  if (kind == MAT_WARD || kind == MAT_WARD_ANISO) {
    if (m.distribution < GVPM_WARD_WARD || m.distribution > GVPM_WARD_BALANCED) return refuse(GVPM_ERR_UNSUPPORTED, "Ward: variant ward / ward-duer / balanced");
  } else if (kind == MAT_ROUGHCONDUCTOR || kind == MAT_ROUGHCONDUCTOR_ANISO || kind == MAT_ROUGHPLASTIC || kind == MAT_ROUGHDIELECTRIC) {
    if (m.distribution != GVPM_MICROFACET_BECKMANN && m.distribution != GVPM_MICROFACET_GGX && m.distribution != GVPM_MICROFACET_PHONG)
      return refuse(GVPM_ERR_UNSUPPORTED, kind == MAT_ROUGHPLASTIC      ? "rough plastic: Beckmann, GGX or Phong"
                                          : kind == MAT_ROUGHDIELECTRIC ? "rough dielectric: Beckmann, GGX or Phong"
                                                                        : "rough conductor: Beckmann, GGX or Phong / Ashikhmin-Shirley");
  }
  if (m.bsdf < -1) return refuse(GVPM_ERR_INVALID_ARG, "material: bsdf is -1 (no table entry) or the index of the material's first head");
  if (kind == MAT_MIXTURE) {
    // (sampleMixture divides by w_0 + w_1: the table's rule for the weights)
    if (!(m.mix_w[0] >= 0.0 && m.mix_w[0] <= FLT_MAX) || !(m.mix_w[1] >= 0.0 && m.mix_w[1] <= FLT_MAX) || !(m.mix_w[0] + m.mix_w[1] > 0.0))
      return refuse(GVPM_ERR_INVALID_ARG, "mixture: weights finite and >= 0, their sum > 0");
    for (int c = 0; c < 2; ++c)
      if (m.child[c] < 0 || (uint32_t)m.child[c] >= sc->n_mats) return refuse(GVPM_ERR_INVALID_ARG, "mixture: a child is the index of a material of the scene");
    for (int c = 0; c < 2; ++c) {
      const int ck = sc->mat_kind[m.child[c]];
      if (ck != MAT_LAMBERT && ck != MAT_ROUGHCONDUCTOR && ck != MAT_ROUGHCONDUCTOR_ANISO)
        return refuse(GVPM_ERR_UNSUPPORTED, "mixture: a child is the Lambertian or a rough conductor (one component each; no mixture as a child)");
    }
  }
  return GVPM_OK;
}

// `dm`: the materials beyond kind and albedo (null: the closed set, every kind above MAT_MIRROR has been refused)
static int createCommon(const gvpm_devgen_scene *sc, const gvpm_devgen_material *dm, int device, gvpm_devgen **out) {
  if (hipSetDevice(device) != hipSuccess) return refuse(GVPM_ERR_NO_DEVICE, "no such HIP device");
  gvpm_devgen *g = new (std::nothrow) gvpm_devgen();
  if (!g) return refuse(GVPM_ERR_HIP, "out of host memory");
  g->device = device;
  auto bail = [&](int rc) {
    gvpm_devgen_destroy(g);
    return refuse(rc, "a HIP call failed while the generator was set up");
  };
  if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) return bail(GVPM_ERR_HIP);
  std::vector<SynthTri> tris(sc->n_tris);
  for (uint32_t i = 0; i < sc->n_tris; ++i) {
    const double *t = sc->tris + 12 * (size_t)i;
    tris[i].v0 = V3(t[0], t[1], t[2]);
    tris[i].e1 = V3(t[3], t[4], t[5]);
    tris[i].e2 = V3(t[6], t[7], t[8]);
    tris[i].n = V3(t[9], t[10], t[11]);
    tris[i].mat = sc->tri_mat[i];
  }
  // the rough plastics' slices, one after the other in device memory the generator owns
  std::vector<float> slices;
  std::vector<SynthMat> mats(sc->n_mats);
  for (uint32_t i = 0; i < sc->n_mats; ++i) {
    mats[i].kind = sc->mat_kind[i];
    mats[i].albedo = V3(sc->mat_albedo[3 * i], sc->mat_albedo[3 * i + 1], sc->mat_albedo[3 * i + 2]);
    mats[i].spec = V3(0.0);
    mats[i].exponent = mats[i].specWeight = 0.0;
    mats[i].bsdf = -1;
    if (!dm) continue;
    const gvpm_devgen_material &m = dm[i];
    SynthMat &o = mats[i];
    o.spec = V3(m.spec[0], m.spec[1], m.spec[2]);
    o.exponent = m.exponent;
    o.specWeight = m.spec_weight;
    o.bsdf = m.bsdf;
    o.eta = V3(m.eta[0], m.eta[1], m.eta[2]);
    o.k = V3(m.k[0], m.k[1], m.k[2]);
    o.distribution = m.distribution;
    o.coatEta = m.coat_eta;
    o.fdr = m.fdr;
    o.nonlinear = m.nonlinear;
    o.alphaV = m.alpha_v;
    o.tangent = V3(m.tangent[0], m.tangent[1], m.tangent[2]);
    for (int c = 0; c < 2; ++c) {
      o.child[c] = m.child[c];
      o.mixW[c] = m.mix_w[c];
    }
    if (o.kind == MAT_ROUGHPLASTIC) slices.insert(slices.end(), m.rtrans, m.rtrans + GVPM_RTRANS_KNOTS);
    if (o.kind > MAT_MIRROR) g->glossy = true;
  }
  if (!slices.empty()) {
    if (g->slices.ensure(slices.size()) != hipSuccess ||
        hipMemcpy(g->slices.p, slices.data(), slices.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      return bail(GVPM_ERR_HIP);
    size_t at = 0;
    for (auto &o : mats)
      if (o.kind == MAT_ROUGHPLASTIC) {
        o.rtrans = g->slices.p + at;  // (a device address: the host never reads through it)
        at += GVPM_RTRANS_KNOTS;
      }
  }
  if (g->tris.ensure(tris.size() + 1) != hipSuccess || g->mats.ensure(mats.size() + 1) != hipSuccess) return bail(GVPM_ERR_HIP);
  if (!tris.empty() && hipMemcpy(g->tris.p, tris.data(), tris.size() * sizeof(SynthTri), hipMemcpyHostToDevice) != hipSuccess)
    return bail(GVPM_ERR_HIP);
  if (!mats.empty() && hipMemcpy(g->mats.p, mats.data(), mats.size() * sizeof(SynthMat), hipMemcpyHostToDevice) != hipSuccess)
    return bail(GVPM_ERR_HIP);
  if (hipHostMalloc((void **)&g->pinned, 64, hipHostMallocMapped) != hipSuccess) return bail(GVPM_ERR_HIP);
  SceneView &v = g->view;
  v.tris = g->tris.p;
  v.ntri = (int)sc->n_tris;
  v.mats = g->mats.p;
  v.nmats = (int)sc->n_mats;
  v.lightC = V3(sc->light_c[0], sc->light_c[1], sc->light_c[2]);
  v.lightU = V3(sc->light_u[0], sc->light_u[1], sc->light_u[2]);
  v.lightV = V3(sc->light_v[0], sc->light_v[1], sc->light_v[2]);
  v.lightN = V3(sc->light_n[0], sc->light_n[1], sc->light_n[2]);
  v.radiance = V3(sc->radiance[0], sc->radiance[1], sc->radiance[2]);
  v.lightArea = sc->light_area;
  v.medium = sc->medium;
  v.camPos = V3(sc->cam_pos[0], sc->cam_pos[1], sc->cam_pos[2]);
  {
    const double *m = sc->cam_to_world;
    bool zero = true;
    for (int k = 0; k < 9; ++k) zero = zero && m[k] == 0.0;
    v.camX = zero ? V3(1, 0, 0) : V3(m[0], m[3], m[6]);
    v.camY = zero ? V3(0, 1, 0) : V3(m[1], m[4], m[7]);
    v.camZ = zero ? V3(0, 0, 1) : V3(m[2], m[5], m[8]);
  }
  v.tanHalfFovX = sc->tan_half_fov_x;
  v.width = sc->width;
  v.height = sc->height;
  v.seed = sc->seed;
  v.cameraInside = sc->camera_inside != 0;
  v.maxDepth = sc->max_depth;
  v.rrDepth = sc->rr_depth;
  v.minDepth = sc->min_depth;
  v.cameraSphere = sc->camera_sphere;
  *out = g;
  devgenError = "";
  return GVPM_OK;
}

int gvpm_devgen_create(const gvpm_devgen_scene *sc, int device, gvpm_devgen **out) {
  if (int rc = checkScene(sc, out)) return rc;
  // (the closed set: Lambertian, index-matched boundary, mirror -- a glossy wall's parameters do not travel in gvpm_devgen_scene:
  // gvpm_devgen_create_ex takes them)
  auto bail = [](int rc) {
    return refuse(rc, "material kind outside gvpm_devgen_create's closed set (Lambertian, index-matched, mirror): gvpm_devgen_create_ex");
  };
  for (uint32_t i = 0; i < sc->n_mats; ++i) {
    const int kind = sc->mat_kind[i];
    if (kind < 0 || kind > MAT_MIRROR) return bail(GVPM_ERR_UNSUPPORTED);
  }
  return createCommon(sc, nullptr, device, out);
}

int gvpm_devgen_create_ex(const gvpm_devgen_scene *sc, const gvpm_devgen_material *mats, uint32_t n_mats, int device, gvpm_devgen **out) {
  if (int rc = checkScene(sc, out)) return rc;
  if (n_mats != sc->n_mats || (n_mats && !mats)) return refuse(GVPM_ERR_INVALID_ARG, "one gvpm_devgen_material per material of the scene");
  for (uint32_t i = 0; i < n_mats; ++i)
    if (int rc = checkMaterial(sc, mats, i)) return rc;
  return createCommon(sc, mats, device, out);
}

int gvpm_devgen_destroy(gvpm_devgen *g) {
  if (!g) return GVPM_ERR_INVALID_ARG;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  g->tris.release(); g->mats.release(); g->slices.release();
  g->counts.release(); g->counted.release(); g->nonEmpty.release(); g->offs.release(); g->countedOffs.release();
  g->neOffs.release(); g->ctl.release(); g->park.release();
  for (auto &o : g->pout) {
    for (auto &b : o.f3) b.release();
    for (auto &b : o.f1) b.release();
    o.endN.release(); o.flags.release(); o.pathId.release();
  }
  g->pixFlag.release(); g->pixOffs.release();
  for (auto &b : g->raysOut) b.release();
  if (g->scanTmp.d) (void)hipFree(g->scanTmp.d);
  if (g->pinned) (void)hipHostFree(g->pinned);
  if (g->stream) (void)hipStreamDestroy(g->stream);
  delete g;
  return GVPM_OK;
}

// beams != 0: photon beams (one record per medium edge, LTBeamMap::tryAppendLT) + end normals
static int shootCommon(gvpm_devgen *g, int iteration, uint64_t capacity, int beams, gvpm_photon_soa *soa, const float **endN,
                       uint64_t *nbPaths) {
  if (!g || !soa || !nbPaths || capacity == 0 || capacity > 0x7FFFFFF0ull) return GVPM_ERR_INVALID_ARG;
  (void)hipSetDevice(g->device);
  hipStream_t s = g->stream;
  g->poutIdx = (g->poutIdx + 1) % 3;
  for (auto &b : g->po().f3) SY_TRY(b.ensure(capacity * 3 + 4));
  for (auto &b : g->po().f1) SY_TRY(b.ensure(capacity + 4));
  SY_TRY(g->po().flags.ensure(capacity + 4));
  SY_TRY(g->po().pathId.ensure(capacity + 4));
  if (beams) SY_TRY(g->po().endN.ensure(capacity * 3 + 4));
  // paths per batch: what the previous shoot needed per stored photon plus a margin, so that one batch (one
  // count pass + one write pass) usually suffices; `capacity` paths the first time
  const double perPhoton = g->pathsPerPhoton > 0.0 ? g->pathsPerPhoton * 1.06 : 1.0;
  const uint32_t m = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((uint64_t)((double)capacity * perPhoton) + 64, 4096), 1u << 22);
  Buf<uint32_t> *scratch[] = {&g->counts, &g->counted, &g->nonEmpty, &g->offs, &g->countedOffs, &g->neOffs};
  for (auto *b : scratch) SY_TRY(b->ensure((size_t)m + 1));
  SY_TRY(g->ctl.ensure(8));
  SY_TRY(hipMemsetAsync(g->ctl.p, 0, 8 * sizeof(uint32_t), s));
  // a path stores at most one record per vertex beyond the emitter sample
  const int stride = std::max(1, std::min(GVPM_SYNTH_MAXV, g->view.maxDepth));
  SY_TRY(g->park.ensure((size_t)m * stride * PARK_WORDS + 64));
  PhotonOut o;
  for (int a = 0; a < 8; ++a) o.v3[a] = g->po().f3[a].p;
  for (int a = 0; a < 4; ++a) o.f1[a] = g->po().f1[a].p;
  o.flags = g->po().flags.p;
  o.pathId = g->po().pathId.p;
  o.endN = beams ? g->po().endN.p : nullptr;
  uint64_t base = 0, stored = 0, paths = 0;
  for (int batch = 0; stored < capacity; ++batch) {
    if (batch > 4096) return GVPM_ERR_STATE;  // a scene that stores nothing
    // one round of waves (two per SIMD at this kernel's registers), each walking its share of the batch with refill
    const uint32_t chunk = std::max(64u, (((m + 2047u) / 2048u) + 63u) & ~63u);  // (1024 / 4096 / 8192 shares: the same)
    const unsigned nb = (m + chunk - 1) / chunk;
    (g->glossy ? synthLaunchWalk_glossy : synthLaunchWalk)(s, nb, g->view, iteration, base, m, chunk, beams, g->park.p, stride, g->counts.p,
                                                           g->counted.p, g->nonEmpty.p);
    SY_TRY(exclusiveSumU32(g->scanTmp, g->counts.p, g->offs.p, m, s));
    SY_TRY(exclusiveSumU32(g->scanTmp, g->counted.p, g->countedOffs.p, m, s));
    SY_TRY(exclusiveSumU32(g->scanTmp, g->nonEmpty.p, g->neOffs.p, m, s));
    hipLaunchKernelGGL(synth_stop_kernel, dim3(1), dim3(1), 0, s, g->counts.p, g->offs.p, g->countedOffs.p, g->counted.p,
                       g->neOffs.p, g->nonEmpty.p, m, capacity, g->ctl.p);
    {
      const uint64_t slots = (uint64_t)m * (uint64_t)stride;
      hipLaunchKernelGGL(synth_place_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, g->park.p, stride, g->counts.p,
                         g->offs.p, g->neOffs.p, g->ctl.p, m, capacity, o);
    }
    uint32_t c[8];
    SY_TRY(hipMemcpyAsync(c, g->ctl.p, sizeof(c), hipMemcpyDeviceToHost, s));
    SY_TRY(hipStreamSynchronize(s));
    SY_TRY(hipGetLastError());
    base += c[3];
    stored = c[4];
    paths = c[5];
    // next batch continues from the totals
    const uint32_t next[3] = {c[4], c[5], c[6]};
    SY_TRY(hipMemcpyAsync(g->ctl.p, next, sizeof(next), hipMemcpyHostToDevice, s));
    SY_TRY(hipStreamSynchronize(s));
  }
  soa->pos = g->po().f3[0].p; soa->wi = g->po().f3[1].p; soa->flux = g->po().f3[2].p; soa->parent_pos = g->po().f3[3].p;
  soa->parent_n = g->po().f3[4].p; soa->prefix_w = g->po().f3[5].p; soa->parent_scat = g->po().f3[6].p; soa->parent_wi = g->po().f3[7].p;
  soa->parent_pdf = g->po().f1[0].p; soa->edge_pdf = g->po().f1[1].p; soa->parent_rr = g->po().f1[2].p; soa->parent_g = g->po().f1[3].p;
  soa->flags = g->po().flags.p;
  soa->path_id = g->po().pathId.p;
  soa->n = stored;
  if (endN) *endN = beams ? g->po().endN.p : nullptr;
  *nbPaths = paths;
  if (stored) g->pathsPerPhoton = (double)base / (double)stored;
  return GVPM_OK;
}

int gvpm_devgen_shoot_photons(gvpm_devgen *g, int iteration, uint64_t capacity, gvpm_photon_soa *dev_soa, uint64_t *nb_paths) {
  return shootCommon(g, iteration, capacity, 0, dev_soa, nullptr, nb_paths);
}

int gvpm_devgen_shoot_beams(gvpm_devgen *g, int iteration, uint64_t capacity, gvpm_photon_soa *dev_soa, const float **end_n_dev,
                           uint64_t *nb_paths) {
  if (!end_n_dev) return GVPM_ERR_INVALID_ARG;
  return shootCommon(g, iteration, capacity, 1, dev_soa, end_n_dev, nb_paths);
}

int gvpm_devgen_read(gvpm_devgen *g, const void *dev, void *host, uint64_t bytes) {
  if (!g || (bytes && (!dev || !host))) return GVPM_ERR_INVALID_ARG;
  (void)hipSetDevice(g->device);
  if (bytes) SY_TRY(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
  return GVPM_OK;
}

int gvpm_devgen_camera_beams(gvpm_devgen *g, int iteration, int tile_mod, int tile_rem, const gvpm_camera_ray **rays_dev,
                            uint64_t *n_sets) {
  if (!g || !rays_dev || !n_sets || tile_mod < 1 || tile_rem < 0 || tile_rem >= tile_mod) return GVPM_ERR_INVALID_ARG;
  (void)hipSetDevice(g->device);
  hipStream_t s = g->stream;
  const uint32_t npix = (uint32_t)g->view.width * (uint32_t)g->view.height;
  SY_TRY(g->pixFlag.ensure((size_t)npix + 1));
  SY_TRY(g->pixOffs.ensure((size_t)npix + 1));
  const unsigned nb = (npix + 63) / 64;
  SY_TRY(hipMemsetAsync(g->pixFlag.p + npix, 0, 4, s));
  (g->glossy ? synthLaunchBeamFlag_glossy : synthLaunchBeamFlag)(s, nb, g->view, iteration, tile_mod, tile_rem, npix, g->pixFlag.p);
  SY_TRY(exclusiveSumU32(g->scanTmp, g->pixFlag.p, g->pixOffs.p, npix + 1, s));
  uint32_t total = 0;
  SY_TRY(hipMemcpyAsync(&total, g->pixOffs.p + npix, 4, hipMemcpyDeviceToHost, s));
  SY_TRY(hipStreamSynchronize(s));
  g->raysIdx = (g->raysIdx + 1) % 3;
  SY_TRY(g->raysOut[g->raysIdx].ensure((size_t)total * 5 + 5));
  (g->glossy ? synthLaunchBeamWrite_glossy : synthLaunchBeamWrite)(s, nb, g->view, iteration, npix, g->pixFlag.p, g->pixOffs.p,
                                                                   g->raysOut[g->raysIdx].p);
  SY_TRY(hipStreamSynchronize(s));
  SY_TRY(hipGetLastError());
  *rays_dev = g->raysOut[g->raysIdx].p;
  *n_sets = total;
  return GVPM_OK;
}

}  // extern "C"
