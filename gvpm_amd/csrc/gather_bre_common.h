// What the two units of the G-BRE gather share: gather_bre.hip (planner, traversal, primal estimate, host-shift tail) and
// gather_bre_eval.hip (the gradient evaluation, built without the SLP vectoriser: DESIGN section 4).
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "vec.h"

namespace gvpm {

constexpr uint32_t EVAL_LDS_TRIS = 64;  // occluders staged in the evaluation kernel's LDS when the scene has no more

// the fp32 error band of the hit test: E bounds |disk - disk_exact|, band |d2 - d2_exact| for the
// difference vector wv = photon - ray origin and disk = wv . d
__device__ __forceinline__ void hitBand(f3 wv, float disk, float r, float r2f, float &E, float &band) {
  E = 6e-7f * (fabsf(wv.x) + fabsf(wv.y) + fabsf(wv.z) + fabsf(disk));
  band = 4.f * r * E + r2f * 2e-6f;
}

// The photon's own sphere box [p - r, p + r] against the ray segment [mint, maxt] (ownBoxHit: what every ancestor box of the
// reference's BVH implies) with fp32 error bands: 1 the slab test surely passes, 0 surely fails, 2 undecidable.  Only asked
// for photons that project at or beyond the beam's END (about one candidate in a thousand): between the ends the point of
// closest approach lies in the sphere, hence in the box, and the test passes by construction.
__device__ __forceinline__ int ownBoxBand(f3 p, f3 o, f3 d, float r, float mint, float maxt) {
  float nearT = -INFINITY, farT = INFINITY, eN = 0.f, eF = 0.f;
  bool open = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float pk = comp(p, k), ok = comp(o, k), dk = comp(d, k);
    if (dk == 0.f) open = true;  // (the reference branches on an exactly zero component: the exact pass decides)
    const float rc = frcp(dk);
    float t1 = ((pk - r) - ok) * rc, t2 = ((pk + r) - ok) * rc;
    const float lo = fminf(t1, t2), hi = fmaxf(t1, t2);
    // numerators good to ~3 eps (|p| + |o| + r), the reciprocal to 1 ulp, the product to half an ulp
    const float e = 4e-7f * (fabsf(pk) + fabsf(ok) + r) * fabsf(rc) + 2e-7f * (fabsf(lo) + fabsf(hi));
    if (lo > nearT) { nearT = lo; eN = e; } else if (lo + e > nearT - eN) { eN = fmaxf(eN, e + (nearT - lo)); }
    if (hi < farT) { farT = hi; eF = e; } else if (hi - e < farT + eF) { eF = fmaxf(eF, e + (hi - farT)); }
  }
  if (open || !(nearT == nearT) || !(farT == farT)) return 2;
  const float mE = 2e-7f * (maxt + mint);
  const bool fail = nearT - eN > farT + eF || farT + eF < mint - mE || nearT - eN > maxt + mE;
  const bool pass = nearT + eN < farT - eF && farT - eF > mint + mE && nearT + eN < maxt - mE;
  return pass ? 1 : (fail ? 0 : 2);
}

__device__ __forceinline__ void borderRule(const GatherArgs &a, uint32_t pix, int i, float &w) {
  // no reverse shift at the right and top borders, shift_volume_photon.cpp:843-846
  const int px = (int)(pix & 0xFFFFu), py = (int)(pix >> 16);
  if ((i == GVPM_RIGHT && px == a.cfg.width - 1) || (i == GVPM_TOP && py == a.cfg.height - 1)) w = 1.f;
}

// LDS accesses of ONE wave are executed in order; what has to be stopped is the compiler moving them
__device__ __forceinline__ void waveLdsSync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Work units of the evaluation (round 6).  The planner balances the TRAVERSAL (items of equal staged photons); the pairs an
// item yields vary by more than ten (C2: mean 450, the items in front of the light 4 500+), and the evaluation took one item per
// wave at a time in index order: with ~7 items a wave the last one decided when a wave ended -- the waves finished anywhere
// between 0.47 and 1.19 ms of a 1.19 ms kernel (probe build), mean 0.75: a third of the wave-time was the tail.  The
// traversal now files every item's pairs as parts of at most EVAL_UNIT pairs in two lists -- parts above EVAL_UNIT_SMALL
// pairs, and the small ones -- and the evaluation's queue serves the large list first: the units that end the kernel are small.
#ifndef GVPM_EVAL_UNIT
#define GVPM_EVAL_UNIT 1280
#endif
#ifndef GVPM_EVAL_UNIT_SMALL
#define GVPM_EVAL_UNIT_SMALL 256
#endif
constexpr uint32_t EVAL_UNIT = GVPM_EVAL_UNIT, EVAL_UNIT_SMALL = GVPM_EVAL_UNIT_SMALL;

// waves per SIMD the evaluation is compiled for, and an attribute slot for probe builds (gather_bre_eval.hip)
#ifndef GVPM_EVAL_MINW
#define GVPM_EVAL_MINW 3
#endif
#ifndef GVPM_EVAL_ATTR
#define GVPM_EVAL_ATTR
#endif

}  // namespace gvpm
