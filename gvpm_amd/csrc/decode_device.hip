// The device decoders of the packed inputs: packed / linked photon records, packed / compact camera-beam sets, octahedral end
// normals and run-packed G-VPM samples into what the SoA uploads put in the staging slots.  pack_codec.h defines the bytes, for these kernels and for the host unpackers
// (pack_host.hip) from one text; the consuming gather launches them at the head of its build chain (uploads.hip, stagingHead).
#include "context.h"
#include "pack_codec.h"

namespace {

// ---- packed records -> what the SoA uploads put in the slots (pack_codec.h) ----------------
__global__ __launch_bounds__(256) void unpack_photons_kernel(const gvpm_photon_packed *__restrict__ src, uint32_t n,
                                                             const gvpm_material *__restrict__ table, uint32_t table_n,
                                                             gvpm_photon_soa dst, unsigned long long *bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    // gvpm_unpack_photons refuses such a record; here it decodes as a black parent and is REPORTED (gvpm_get_stats fails)
    if (src[i].material >= table_n) atomicAdd(bad, 1ull);
    unpackPhoton(src[i], table, table_n, dst, i);
  }
}
__global__ __launch_bounds__(256) void unpack_rays_kernel(const gvpm_beam_set_packed *__restrict__ src, uint32_t nsets,
                                                          gvpm_camera_ray *__restrict__ dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nsets * 5u) dst[i] = unpackRay(src[i / 5u], (int)(i % 5u));
}

__global__ __launch_bounds__(256) void unpack_compact_rays_kernel(gvpm_sensor sensor, const gvpm_beam_set_compact *__restrict__ src,
                                                                  uint32_t nsets, gvpm_camera_ray *__restrict__ dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nsets * 5u) dst[i] = unpackCompactRay(sensor, src[i / 5u], (int)(i % 5u));
}

// linked records (pack_codec.h): first pass -- a wave takes 64 consecutive photons; the index of a photon's record within
// its kind's array is the group's base + the lanes of that kind below it.  The header was checked on the host
// (linkedHeaderOk); the body is not trusted: a kind 3, or a group whose bases are not the running counts -- base + its
// records of the kind = the next group's base (the last group's: the header's count), bases of group 0 zero -- is
// REPORTED (gvpm_get_stats fails, as gvpm_unpack_photons_linked refuses the blob) and decodes as a zero record; no record
// index at or beyond its kind's count is ever read, whatever the bytes say
__global__ __launch_bounds__(256) void unpack_linked_kernel(const unsigned char *__restrict__ blob, const gvpm_material *__restrict__ table,
                                                            uint32_t table_n, gvpm_photon_soa dst, unsigned long long *bad) {
  const gvpm_linked_header hd = *reinterpret_cast<const gvpm_linked_header *>(blob);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < hd.n;
  const uint32_t *kinds = reinterpret_cast<const uint32_t *>(blob + hd.off_kinds);
  const uint32_t kind = live ? linkedKind(kinds, i) : 3u;
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long mF = __ballot(kind == GVPM_LINKED_FULL), mE = __ballot(kind == GVPM_LINKED_EMIT), mC = __ballot(kind == GVPM_LINKED_CHAIN);
  if (!live) return;
  const uint2 *groups = reinterpret_cast<const uint2 *>(blob + hd.off_groups);
  const uint32_t g = i >> 6, first = i & ~63u;
  const uint2 base = groups[g];
  const uint2 next = g + 1u < (hd.n + 63u) >> 6 ? groups[g + 1u] : make_uint2(hd.n_full, hd.n_emit);
  const bool groupOk = (uint64_t)base.x + (uint64_t)__popcll(mF) == next.x && (uint64_t)base.y + (uint64_t)__popcll(mE) == next.y &&
                       (uint64_t)base.x + base.y <= first;
  bool ok = groupOk;
  if (kind == GVPM_LINKED_FULL) {
    const uint32_t j = base.x + (uint32_t)__popcll(mF & below);
    ok = ok && j < hd.n_full;
    gvpm_photon_packed r{};
    if (ok) r = reinterpret_cast<const gvpm_photon_packed *>(blob + hd.off_full)[j];
    if (!ok || r.material >= table_n) atomicAdd(bad, 1ull);
    unpackPhoton(r, table, table_n, dst, i);
  } else if (kind == GVPM_LINKED_EMIT) {
    const uint32_t j = base.y + (uint32_t)__popcll(mE & below);
    ok = ok && j < hd.n_emit;
    gvpm_photon_emit r{};
    if (ok) r = reinterpret_cast<const gvpm_photon_emit *>(blob + hd.off_emit)[j];
    if (!ok || (r.flags >> 16) >= hd.n_emitters) atomicAdd(bad, 1ull);
    unpackEmit(r, reinterpret_cast<const gvpm_emitter_entry *>(blob + hd.off_emitters), hd.n_emitters, dst, i);
  } else {
    // (kind 3 included: its chain index would collide with a real chain record's)
    const uint32_t j = first - base.x - base.y + (uint32_t)__popcll(mC & below);
    ok = ok && kind == GVPM_LINKED_CHAIN && j < hd.n_chain;
    gvpm_photon_chain r{};
    if (ok) r = reinterpret_cast<const gvpm_photon_chain *>(blob + hd.off_chain)[j];
    if (!ok || (r.flags >> 16) >= table_n || i == 0u) atomicAdd(bad, 1ull);
    unpackChainOwn(r, table, table_n, dst, i);
  }
}
// ... second pass: the chain records' links
__global__ __launch_bounds__(256) void link_linked_kernel(const unsigned char *__restrict__ blob, gvpm_photon_soa dst) {
  const gvpm_linked_header hd = *reinterpret_cast<const gvpm_linked_header *>(blob);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0u || i >= hd.n) return;
  const uint32_t *kinds = reinterpret_cast<const uint32_t *>(blob + hd.off_kinds);
  if (linkedKind(kinds, i) != GVPM_LINKED_CHAIN) return;
  linkChain(dst, i, i >= 2u && linkedKind(kinds, i - 1u) == GVPM_LINKED_CHAIN);
}

// ---- side inputs: end normals as octahedral codes, G-VPM samples as runs (pack_codec.h) ----
__global__ __launch_bounds__(256) void unpack_normals_oct_kernel(const uint32_t *__restrict__ codes, uint32_t n, float *__restrict__ dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v[3];
  octDecode(codes[i], v);
  dst[3 * (size_t)i] = v[0];
  dst[3 * (size_t)i + 1] = v[1];
  dst[3 * (size_t)i + 2] = v[2];
}
// one sample a lane, whatever the runs' lengths: each finds its run by bisection over the runs' first samples (the host has
// checked that they ascend from 0 and end at n: vpmRunsOk), so a run of 1, of 64 or of 10 000 samples is the same code
__global__ __launch_bounds__(256) void expand_vpm_runs_kernel(const gvpm_vpm_run *__restrict__ runs, uint32_t nruns,
                                                              const float *__restrict__ rands, uint32_t n,
                                                              gvpm_vpm_sample *__restrict__ dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = expandVpmSample(runs, nruns, rands, i);
}

}  // namespace

namespace gvpm {
void launch_unpack_normals_oct(const uint32_t *codes, uint32_t n, float *dst, hipStream_t s) {
  if (n) hipLaunchKernelGGL(unpack_normals_oct_kernel, dim3((n + 255) / 256), dim3(256), 0, s, codes, n, dst);
}
void launch_expand_vpm_runs(const uint32_t *packed, uint32_t nruns, uint32_t n, gvpm_vpm_sample *dst, hipStream_t s) {
  if (n && nruns)
    hipLaunchKernelGGL(expand_vpm_runs_kernel, dim3((n + 255) / 256), dim3(256), 0, s, reinterpret_cast<const gvpm_vpm_run *>(packed),
                       nruns, reinterpret_cast<const float *>(packed + (size_t)nruns * 4), n, dst);
}
void launch_unpack_linked(const uint32_t *blob, uint32_t n, const gvpm_material *table, uint32_t table_n, const gvpm_photon_soa &dst,
                          unsigned long long *bad, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(unpack_linked_kernel, dim3((n + 255) / 256), dim3(256), 0, s, reinterpret_cast<const unsigned char *>(blob), table,
                     table_n, dst, bad);
  hipLaunchKernelGGL(link_linked_kernel, dim3((n + 255) / 256), dim3(256), 0, s, reinterpret_cast<const unsigned char *>(blob), dst);
}
void launch_unpack_compact_rays(const gvpm_sensor &sensor, const uint32_t *compact, uint32_t ncompact, gvpm_camera_ray *dst,
                                hipStream_t s) {
  if (ncompact)
    hipLaunchKernelGGL(unpack_compact_rays_kernel, dim3((ncompact * 5u + 255) / 256), dim3(256), 0, s, sensor,
                       reinterpret_cast<const gvpm_beam_set_compact *>(compact), ncompact, dst);
}
void launch_unpack_photons(const uint32_t *packed, uint32_t n, const gvpm_material *table, uint32_t table_n,
                           const gvpm_photon_soa &dst, unsigned long long *bad, hipStream_t s) {
  if (n)
    hipLaunchKernelGGL(unpack_photons_kernel, dim3((n + 255) / 256), dim3(256), 0, s,
                       reinterpret_cast<const gvpm_photon_packed *>(packed), n, table, table_n, dst, bad);
}
void launch_unpack_rays(const uint32_t *packed, uint32_t nsets, gvpm_camera_ray *dst, hipStream_t s) {
  if (nsets)
    hipLaunchKernelGGL(unpack_rays_kernel, dim3((nsets * 5u + 255) / 256), dim3(256), 0, s,
                       reinterpret_cast<const gvpm_beam_set_packed *>(packed), nsets, dst);
}
}  // namespace gvpm
