// The device generators' kernels with the glossy materials compiled in (gvpm_devgen_create_ex, include/gvpm_hip.h): the walk and
// the camera-beam kernels of synth_walk_kernels.inc and synth_camera_kernels.inc once more, under names of their own, with host/synth_core.h's
// GVPM_SYNTH_GLOSSY regions in the device pass -- Phong, Ward, the rough conductor, the plastics, the anisotropic kinds, the rough
// dielectric and the two-child mixture, sampled by the very text the host generators run.  A unit of its own, as
// gather_bre_eval.inc's units are: the fp64 pow / atan / log chains cost registers (NOTEBOOK.md, "device generators walk glossy
// scenes"), and synth_device.hip's closed-set kernels must not pay for them.  The camera walk has no glossy region today -- a
// camera path ends on a glossy wall as it does on a Lambertian one -- so the camera kernels here compute what the closed set's do;
// they live here so that a generator launches one family.
#define GVPM_SYNTH_DEVICE_GLOSSY 1
#include <hip/hip_runtime.h>

#include "../../include/gvpm_hip.h"
#include "../host/synth_core.h"
#include "synth_device_launch.h"

#define GVPM_SYNTH_K(name) GVPM_SYNTH_GLOSSY_NAME(name)
#include "synth_walk_kernels.inc"
#include "synth_camera_kernels.inc"
