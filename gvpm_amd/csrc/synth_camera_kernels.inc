// The device generators' camera-beam kernels, written once and compiled by two units: synth_device.hip (the closed set Lambertian /
// index-matched / mirror, GVPM_SYNTH_GLOSSY 0 in its device pass) and synth_device_glossy.hip (every material of the host walk).  The
// including unit defines GVPM_SYNTH_K(name): the kernels' and launchers' names in that unit.  Each unit is a code object of its own
// (no relocatable device code), so one instantiation costs the other nothing (host/synth_core.h, at MatKind).
namespace gvpm {
namespace {

// ---- camera beams ----
__device__ __forceinline__ bool ownedPixel(const SceneView &sc, uint32_t p, int tileMod, int tileRem, int &px, int &py) {
  px = (int)(p % (uint32_t)sc.width);
  py = (int)(p / (uint32_t)sc.width);
  const int tilesX = (sc.width + 3) / 4;
  return !(tileMod > 1 && ((py / 4) * tilesX + px / 4) % tileMod != tileRem);
}
__global__ __launch_bounds__(64) void GVPM_SYNTH_K(synth_beam_flag_kernel)(SceneView sc, int iteration, int tileMod, int tileRem,
                                                             uint32_t npix, uint32_t *flag) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  int px, py;
  uint32_t f = 0;
  if (ownedPixel(sc, p, tileMod, tileRem, px, py)) {
    // the number of sets (medium edges of the base path: 0, 1, or 2 behind a mirror)
    gvpm_camera_ray sets[2][5];
    float w[2];
    f = (uint32_t)cameraBeamSets(sc, iteration, px, py, sets, w);
  }
  flag[p] = f;
}
__global__ __launch_bounds__(64) void GVPM_SYNTH_K(synth_beam_write_kernel)(SceneView sc, int iteration, uint32_t npix,
                                                              const uint32_t *flag, const uint32_t *offs,
                                                              gvpm_camera_ray *out) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix || !flag[p]) return;
  const int px = (int)(p % (uint32_t)sc.width), py = (int)(p / (uint32_t)sc.width);
  gvpm_camera_ray sets[2][5];
  float w[2];
  const int n = cameraBeamSets(sc, iteration, px, py, sets, w);
  gvpm_camera_ray *dst = out + (size_t)offs[p] * 5;
  for (int q = 0; q < n; ++q)
    for (int k = 0; k < 5; ++k) dst[5 * q + k] = sets[q][k];
}

}  // namespace

// the launchers synth_device.hip's drivers call (synth_device_launch.h)
void GVPM_SYNTH_K(synthLaunchBeamFlag)(hipStream_t s, unsigned nb, const SceneView &sc, int iteration, int tileMod, int tileRem, uint32_t npix,
                                       uint32_t *flag) {
  hipLaunchKernelGGL(GVPM_SYNTH_K(synth_beam_flag_kernel), dim3(nb), dim3(64), 0, s, sc, iteration, tileMod, tileRem, npix, flag);
}
void GVPM_SYNTH_K(synthLaunchBeamWrite)(hipStream_t s, unsigned nb, const SceneView &sc, int iteration, uint32_t npix, const uint32_t *flag,
                                        const uint32_t *offs, gvpm_camera_ray *out) {
  hipLaunchKernelGGL(GVPM_SYNTH_K(synth_beam_write_kernel), dim3(nb), dim3(64), 0, s, sc, iteration, npix, flag, offs, out);
}

}  // namespace gvpm
