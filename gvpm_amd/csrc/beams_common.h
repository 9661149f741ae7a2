// What the G-Beams units share and nothing more: the sub-beam count (the grid build, the traversal and both evaluations must
// cut a beam the same way), the traversal's fp32 ownership prefilter, the run lengths of the evaluation front ends and the
// launchers' dispatch over the tile width.  The traversal unit (gather_beams_trav.hip) includes this and neither evaluation.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_types.h"
#include "shift_device.h"
#include "vec.h"

// blocks of 64 pairs an evaluation wave reserves at a time (guided: evaluate_beams2_kernel, gather_beams.hip)
#ifndef GVPM_BEAMS_RUN  // (probe builds)
#define GVPM_BEAMS_RUN 256
#endif
#ifndef GVPM_BEAMS_RUN_MIN
#define GVPM_BEAMS_RUN_MIN 16
#endif

namespace gvpm {

// number of sub-beams of a beam of length len for target length ls (shared with the grid build)
__device__ __forceinline__ uint32_t subBeamCount(float len, float ls) {
  const float n = ceilf(len / ls);
  return (uint32_t)fminf(fmaxf(n, 1.f), 255.f);
}

// fp32 necessary condition for evaluateBeam to produce anything for (camera ray, sub-beam): the two lines pass
// within the kernel radius and the parameter that decides ownership (3D: where the beam enters the camera ray's
// capped cylinder, shift_volume_beams.h:213-220; 1D: the closest approach, beams_struct.h:297-299) falls in this
// sub-beam's range, fattened by a margin that covers the fp32 error.  Everything is measured from the sub-beam's
// centre, which the sphere test already placed within radius + half a sub-beam of the ray, so the operands are small
// and well conditioned; near-parallel pairs are passed through.  The fp64 evaluation that follows repeats the
// reference's tests exactly: the prefilter only removes pairs it would reject (~7 of 8: each beam crosses the ray's
// neighbourhood with several sub-beams and exactly one owns the pair).
__device__ __forceinline__ bool beamPrefilter(const RayReg &base, f3 C, f3 bd, float ls, uint32_t sub, float r, float eps,
                                              int technique) {
  const f3 co = C - base.o;
  const float sC = dot(co, base.d);
  const f3 D0 = co - base.d * sC;  // centre relative to its projection on the camera line
  const float bdd = dot(bd, base.d);
  const float sin2 = fmaxf(1.f - bdd * bdd, 0.f);
  if (sin2 < 1e-5f) return true;
  const float inv = frcp(sin2);
  const float tau0 = -(dot(D0, bd) - dot(D0, base.d) * bdd) * inv;  // closest approach, from the centre
  const f3 cr = cross(bd, base.d);
  const float ad = dot(D0, cr);
  const float dmin2 = ad * ad * inv;
  if (dmin2 >= r * r * 1.002f) return false;
  const float delta = 0.01f * ls + 1e-5f * (r + ls) * inv;
  const float half = 0.5f * ls;
  float tau;
  if (technique == GVPM_BEAM_BEAM_1D) {
    // the sub-beam that contains the geometric closest approach speaks for the beam (beamOwner1D; the first one also
    // for an approach before the beam's origin -- one beyond either end can only be accepted through the reference's
    // rounding, and then by no candidate of this traversal: the bounded difference DESIGN.md states)
    tau = tau0;
    return tau < half + delta && (sub == 0u || tau > -half - delta);
  }
  const float hw = fsqrt(fmaxf(r * r - dmin2, 0.f) * inv);
  float tN = tau0 - hw, tF = tau0 + hw;
  // caps of the camera ray's cylinder [mint, maxt] (cylinderIntersection, beams_3d_intersections.h:118-137)
  const float lMax = base.len - 2.f * eps;
  const float zc = sC - eps;
  const float zN = zc + tN * bdd, zF = zc + tF * bdd;
  const float zmarg = 1e-4f * (fabsf(zc) + r);
  if (zN < 0.f) {
    if (zF < -zmarg) return false;
    if (zN != zF) tN = tN + (tF - tN) * fminf(fmaxf(zN / (zN - zF), 0.f), 1.f);
  } else if (zN > lMax) {
    if (zF > lMax + zmarg) return false;
    if (zN != zF) tN = tN + (tF - tN) * fminf(fmaxf((zN - lMax) / (zN - zF), 0.f), 1.f);
  }
  tau = tN;
  // owner: tmin < tN < tmax, or the first sub-beam when the ray's cylinder already contains the beam's origin
  if (tau > -half - delta && tau < half + delta) return true;
  return sub == 0u && tau < -half + delta;
}

// The launchers' one switch: f(std::integral_constant<int, B>) for the tile width B of this context -- 64, 32, and the
// 16-wide kernels for anything else.
template <typename F> inline void forBeamsPerWave(int beamsPerWave, F &&f) {
  switch (beamsPerWave) {
    case 64: f(std::integral_constant<int, 64>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
  }
}

}  // namespace gvpm
