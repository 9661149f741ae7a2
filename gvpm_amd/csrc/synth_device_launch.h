// The launchers of the device generators' two kernel families (synth_walk_kernels.inc, synth_camera_kernels.inc): the closed set of synth_device.hip and
// the glossy unit's, synth_device_glossy.hip.  The drivers (synth_device.hip) pick a family per generator.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gvpm_hip.h"
#include "../host/synth_core.h"

namespace gvpm {

// words of a parked record (ParkSink, synth_walk_kernels.inc; synth_place_kernel reads them)
constexpr int PARK_WORDS = 32;

#define GVPM_SYNTH_LAUNCHERS(K)                                                                                                              \
  void K(synthLaunchWalk)(hipStream_t s, unsigned nb, const SceneView &sc, int iteration, uint64_t base, uint32_t m, uint32_t chunk, int beams, \
                          float *park, int stride, uint32_t *counts, uint32_t *counted, uint32_t *nonEmpty);                                  \
  void K(synthLaunchBeamFlag)(hipStream_t s, unsigned nb, const SceneView &sc, int iteration, int tileMod, int tileRem, uint32_t npix,         \
                              uint32_t *flag);                                                                                                \
  void K(synthLaunchBeamWrite)(hipStream_t s, unsigned nb, const SceneView &sc, int iteration, uint32_t npix, const uint32_t *flag,            \
                               const uint32_t *offs, gvpm_camera_ray *out);
#define GVPM_SYNTH_PLAIN(name) name
#define GVPM_SYNTH_GLOSSY_NAME(name) name##_glossy
GVPM_SYNTH_LAUNCHERS(GVPM_SYNTH_PLAIN)
GVPM_SYNTH_LAUNCHERS(GVPM_SYNTH_GLOSSY_NAME)

}  // namespace gvpm
