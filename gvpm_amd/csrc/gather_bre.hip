// G-BRE gather + gradient-domain shift for gfx950 (CDNA4), hand-written HIP.
//
// Replaces, for one SPPM iteration, the body of
//   GPMIntegrator::computeVolumeGradientPhotonBRE   gvpm/gvpm.cpp:988-1079
//   GradientBeamRadianceEstimator::query            gvpm/gvpm_accel.h:268-312
//   VolumeGradientBREQuery::operator()              gvpm/shift/shift_volume_photon.cpp:658-856
//   shiftNull / shiftPhoton / shiftPhotonDiffuse    shift_volume_photon.cpp:49-158,382-486
//   diffuseReconnection                             gvpm/shift/operation/shift_diffuse.cpp:11-134
//   getShiftPos                                     shift_volume_photon.cpp:858-896
//   GatherPoint::sensorMIS                          gvpm/gvpm_struct.h:608-631
//   HomogeneousMedium::eval, phase eval             src/medium/homogeneous.cpp:432-513, src/phase/*.cpp
//
// Execution model (64-lane waves that share nothing but staged occluders, no MFMA: gather / divergent math):
//   * a TILE is a bundle of B camera-beam sets (B = 16/32/64, 64/B lanes per beam) that the
//     tile sort made spatially coherent (8x8 / 8x4 / 4x4 pixel tiles);
//   * the photon map is a uniform grid (all photons share one radius, gvpm.cpp:989) sorted by
//     cell with x fastest; a tile walks the grid in thick slabs along its major axis,
//     wave-reduces the fattened footprint of its beams into a cell box and turns the box into
//     x-contiguous photon ranges;
//   * plan_kernel walks every tile once WITHOUT touching photons (cellStart differences only) and
//     cuts it into work items of roughly equal candidate count -- the load balancer that replaces
//     BlockScheduler's dynamic image blocks (photonmapper/utilities/block_sched.h:87-113);
//   * traverse_bre_kernel (one workgroup per item, or persistent waves pulling items from an atomic
//     queue: GVPM_PERSISTENT) holds no evaluation state, so it runs at high occupancy: for each slab step the 16-byte hot photon
//     records of the ranges are copied coalesced into an LDS stage and every lane tests them
//     against its own beam (LDS broadcast reads) with a CONSERVATIVE fp32 test (error band on the
//     safe side) plus the exact integer filters (depth, interaction mode, checkerboard parity).
//     Survivors are compacted with __ballot / popcount and appended to the list of their beam in
//     the item's region of the pair buffer (sized by the planner's upper bound; 4 bytes per pair);
//   * evaluate_bre_kernel (gather_bre_eval.hip; persistent, four waves per workgroup) cuts the concatenated per-beam lists
//     of an item into 64 equal chunks, one per lane, walked in segments of 16 steps.  Every pair is first DECIDED: the fp32 test with a rigorous error
//     band, the reference predicate in uncontracted fp64 only when the band could change the
//     decision (~1e-5 of the pairs), so the evaluated set equals the fp64 oracle's bit for bit.
//     Then phase 1 (base contribution + null shifts, 27 sums in registers) and, in a loop of its
//     own, phase 2 (offset-path reconnections with shadow ray, Jacobian, MIS weight); the sums go
//     to per-beam LDS accumulators and are flushed with global atomics at the end of the item.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "device_types.h"
#include "gather_bre_common.h"
#include "shift_device.h"
#include "tile_walk.h"
#include "vec.h"

namespace gvpm {

// ---- exact predicate (fp64, no contraction): gvpm_accel.h:279-301 + aabb.h:310-340 ----
struct HitGeom {
  double disk, distSqr;
};

// diskDistance / distSqr of gvpm_accel.h:296-299 in the reference's operation order
__device__ __forceinline__ HitGeom hitGeom(f3 pf, f3 of, f3 df) {
#pragma clang fp contract(off)
  const double px = pf.x, py = pf.y, pz = pf.z;
  const double ox = of.x, oy = of.y, oz = of.z;
  const double dx = df.x, dy = df.y, dz = df.z;
  const double cx = px - ox, cy = py - oy, cz = pz - oz;
  HitGeom g;
  g.disk = cx * dx + cy * dy + cz * dz;
  const double qx = ox + dx * g.disk, qy = oy + dy * g.disk, qz = oz + dz * g.disk;
  const double vx = qx - px, vy = qy - py, vz = qz - pz;
  g.distSqr = vx * vx + vy * vy + vz * vz;
  return g;
}

// own sphere box vs ray segment: what every ancestor AABB of the reference BVH implies
__device__ __forceinline__ bool ownBoxHit(f3 pf, f3 of, f3 df, d3 rcp, double mint, double maxt, double radius) {
#pragma clang fp contract(off)
  double nearT = -INFINITY, farT = INFINITY;
  const double o3[3] = {of.x, of.y, of.z}, dd[3] = {df.x, df.y, df.z}, c3[3] = {pf.x, pf.y, pf.z};
  const double r3[3] = {rcp.x, rcp.y, rcp.z};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double minVal = c3[i] - radius, maxVal = c3[i] + radius;
    if (dd[i] == 0.0) {
      if (o3[i] < minVal || o3[i] > maxVal) return false;
    } else {
      double t1 = (minVal - o3[i]) * r3[i];
      double t2 = (maxVal - o3[i]) * r3[i];
      if (t1 > t2) { double t = t1; t1 = t2; t2 = t; }
      nearT = fmax(t1, nearT);
      farT = fmin(t2, farT);
      if (!(nearT <= farT)) return false;
    }
  }
  return !(farT < mint || nearT > maxt);
}

// 3D-kernel resample of the camera distance, shift_volume_photon.cpp:707-726
__device__ __forceinline__ bool resample3D(const HitGeom &g, double radius, double rnd, double mint, double edgeLen,
                                           double &tPrime, double &deltaT) {
#pragma clang fp contract(off)
  deltaT = sqrt(fmax(0.0, radius * radius - g.distSqr));
  const double tminKernel = g.disk - deltaT;
  tPrime = tminKernel + (deltaT * 2) * rnd;
  return !(tPrime < mint || tPrime > edgeLen);
}

// The reference's hit decision for one (photon, beam) candidate, in its own operation order.  Rare
// (only candidates inside the fp32 error band get here) and register hungry (fp64 divisions and
// square root), hence not inlined into the traversal loop.
static __device__ __noinline__ bool exactHit(f3 p, f3 o, f3 d, float len, float r, float rnd, float eps, bool use3D) {
  const double mintD = (double)eps, maxtD = (double)len - (double)eps;
  const d3 rcpD = mkd(1.0 / (double)d.x, 1.0 / (double)d.y, 1.0 / (double)d.z);
  const HitGeom g = hitGeom(p, o, d);
  if (!(g.disk > mintD && g.distSqr < (double)r * (double)r && ownBoxHit(p, o, d, rcpD, mintD, maxtD, (double)r)))
    return false;
  if (!use3D) return true;
  double tp, dt;
  return resample3D(g, (double)r, (double)rnd, mintD, (double)len, tp, dt);
}

// The rest of shiftPhotonManifold for the recorded requests, once the host has run the walks (results == nullptr: it has
// not -- every request is a failed shift): shift_volume_photon.cpp:205-279, then the accumulation of :843-853.
__global__ __launch_bounds__(256) void apply_host_shifts_kernel(GatherArgs a, const gvpm_host_shift *__restrict__ results, uint32_t n) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t ok = 0, bad = 0;
  if (k < n) {
    const float4 c0 = a.reqCtx[4 * (size_t)k], c1 = a.reqCtx[4 * (size_t)k + 1], c2 = a.reqCtx[4 * (size_t)k + 2],
                 c3 = a.reqCtx[4 * (size_t)k + 3];
    const float tr = c0.x, pdfCam = c0.y, pdfShiftPos = c0.z, sMIS = c0.w, scale = c1.x;
    const f3 bc = mk3(c1.y, c1.z, c1.w), shD = mk3(c2.x, c2.y, c2.z), eye = mk3(c3.x, c3.y, c3.z);
    const uint32_t pix = __float_as_uint(c2.w);
    const int i = (int)__float_as_uint(c3.w);
    float w = 1.f;
    f3 sflux = mk3(0.f);
    bool good = false;
    if (results && results[k].ok) {
      const gvpm_host_shift r = results[k];
      // result.jacobian *= sRecME.jacobian (1) * additionalJacobian (1); *= detProposed / detSource
      const float jac = r.det_ratio;
      if (jac > 0.f && isfinite(jac)) {
        good = true;
        const f3 photonWeight = mk3(r.throughput[0], r.throughput[1], r.throughput[2]);
        const f3 wi = mk3(r.wi[0], r.wi[1], r.wi[2]);
        const f3 sigS = mk3(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]);
        const f3 contrib = (sigS * photonWeight) * phaseEval(a.med.g, wi, -shD);
        sflux = contrib * eye * (tr * jac);
        w = 0.5f;
        const float offsetPdf = r.pdf * pdfShiftPos;
        if (offsetPdf == 0.f) {
          w = 1.f;
          sflux = mk3(0.f);
        }
        if (a.cfg.use_mis) {
          const float basePdf = pdfCam * r.base_pdf;
          if (basePdf == 0.f) {
            w = 0.f;
          } else if (a.cfg.power_heuristic) {
            const float v = sMIS * jac * (offsetPdf / basePdf);
            w = 1.f / (1.f + v * v);
          } else {
            w = 1.f / (1.f + sMIS * offsetPdf * jac / basePdf);
          }
        }
      }
    }
    borderRule(a, pix, i, w);
    const size_t p = (size_t)(pix >> 16) * a.cfg.width + (pix & 0xFFFFu);
    const float ws = w * scale * a.iterScale, wbS = w * a.iterScale;
    float *dst = a.iter + p * 27;
    if (ws != 0.f) {
      atomicAdd(&dst[3 + 3 * i + 0], sflux.x * ws);
      atomicAdd(&dst[3 + 3 * i + 1], sflux.y * ws);
      atomicAdd(&dst[3 + 3 * i + 2], sflux.z * ws);
    }
    atomicAdd(&dst[15 + 3 * i + 0], bc.x * wbS);
    atomicAdd(&dst[15 + 3 * i + 1], bc.y * wbS);
    atomicAdd(&dst[15 + 3 * i + 2], bc.z * wbS);
    ok = good ? 1u : 0u;
    bad = good ? 0u : 1u;
  }
  // statistics: a manifold shift that succeeded counts with the reconnections, the others are failed shifts
  const uint32_t nOk = (uint32_t)__popcll(__ballot(ok != 0u)), nBad = (uint32_t)__popcll(__ballot(bad != 0u));
  if ((threadIdx.x & 63) == 0 && (nOk | nBad)) {
    unsigned long long *row = a.stats + 8 * (size_t)(blockIdx.x % GVPM_STAT_ROWS);
    atomicAdd(&row[3], (unsigned long long)nOk);
    atomicAdd(&row[4], (unsigned long long)nBad);
  }
}
void launch_apply_host_shifts(const GatherArgs &a, const gvpm_host_shift *results, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(apply_host_shifts_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, results, n);
}

// ------------------------------------------------------------------------------------------
// traversal: persistent waves pulling work items, (photon, beam) pairs out
// ------------------------------------------------------------------------------------------
#ifndef GVPM_TRAV_WPB
#define GVPM_TRAV_WPB 1
#endif
// waves per traversal workgroup: they share nothing (a slice of LDS each, wave-local synchronisation); one
// workgroup of 4 waves costs the dispatcher what a workgroup of one wave does, and 22 000 single-wave workgroups per
// launch were dispatch-bound (2.4 resident waves per SIMD on average where registers and LDS allow 5)
constexpr int TRAV_WPB = GVPM_TRAV_WPB;
// waves per SIMD the traversal is compiled for: the hand-off instantiation (the C2 path) needs 95 VGPRs with nothing spilled
// and takes 5 (round 8: 6 -- 80 -- spills 2); the own-walk one keeps 4 (127 VGPRs; 5 spills 36).  Round 6, one kernel for
// both paths: 3 -- 147 -- was 2 % slower on the pipelined C2 step than 4 -- 128; 5 -- 96, 60 spilled -- equal
#ifndef GVPM_TRAV_MINW
#define GVPM_TRAV_MINW 5
#endif
#ifndef GVPM_TRAV_OWN_MINW
#define GVPM_TRAV_OWN_MINW 4
#endif
// the staged photons, one array per component: a lane tests FOUR consecutive photons against its beam, read with four
// ds_read_b128 issued together, two photons per packed-fp32 instruction
struct alignas(16) TravLds {
  float x[STAGE], y[STAGE], z[STAGE];
  uint32_t bits[STAGE];
  uint32_t stageIdx[STAGE];
  float4 cyl[3];  // the tile's cylinder: {axis point, R^2} {axis direction, s0} {s1}
};
typedef float v2f __attribute__((ext_vector_type(2)));

// OWN_WALK: the kernel computes each slab step's cell box from its own beams (slabBox), as the planner did; only when the
// planner hands no boxes over (GatherArgs::planBoxes null: GVPM_PLAN_BOXES=0, or a grid dimension of 1024 or more).  The
// hand-off instantiation keeps none of TileWalk's per-lane walk state past the set-up (round 8: 95 VGPRs against the own
// walk's 127, at B = 16).
template <int B, bool OWN_WALK>
__global__ __launch_bounds__(64 * TRAV_WPB) __attribute__((amdgpu_waves_per_eu(OWN_WALK ? GVPM_TRAV_OWN_MINW : GVPM_TRAV_MINW))) void traverse_bre_kernel(GatherArgs a, const uint4 *__restrict__ items,
                                                          const uint2 *__restrict__ itemOff,
                                                          const uint32_t *__restrict__ itemCount, uint32_t *queueHead,
                                                          uint32_t *__restrict__ pairs, uint32_t *__restrict__ pairCnt,
                                                          uint32_t persistent, uint2 *__restrict__ units, uint32_t *unitCtl,
                                                          uint32_t unitCap) {
  constexpr int LPB = 64 / B;
  __shared__ TravLds sAll[TRAV_WPB];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (the compiler must see it is wave-uniform)
  TravLds &s = sAll[wv];
  const int lane = threadIdx.x & 63;
  if (itemCount[7] != 0u) return;  // an optimistic step whose buffers were too small (build_chain.hip, TailArgs): queued again
  const uint32_t nItems = *itemCount;
  const int b = lane % B, sub = lane / B;
  const float r = a.radius;
  const float r2f = r * r;
  const float eps = a.cfg.epsilon;
  const uint32_t coalesceAt = a.cfg.reserved[3] ? (uint32_t)a.cfg.reserved[3] : 512u;  // photons in a box row set
  unsigned long long nCand = 0;  // wave-uniform
  uint32_t nOver = 0;

  // One item per wave (the grid is the item count: the hardware dispatcher balances the load and, at every workgroup
  // boundary, lets the other streams' kernels in by priority -- persistent waves hold their registers until the whole
  // kernel ends, which stretched the next step's build, a chain of twenty small kernels, from 0.55 to 1.3 ms).
  // `persistent` (GVPM_PERSISTENT=1): waves loop over items; the first is the wave's own index, a shared counter
  // (one address: ~11 ns per atomic whatever the number of waves) serves the rest.
  bool firstItem = true;
  for (;;) {
    uint32_t it = blockIdx.x * TRAV_WPB + (uint32_t)wv;
    if (!firstItem) {
      // (a grid that covers the items -- the usual case of an optimistic step, whose grid is a guess -- asks the queue nothing)
      if (!persistent || gridDim.x * TRAV_WPB >= nItems) break;
      if (lane == 0) it = gridDim.x * TRAV_WPB + atomicAdd(queueHead, 1u);
      it = __shfl(it, 0, 64);
    }
    firstItem = false;
    it = (uint32_t)__builtin_amdgcn_readfirstlane((int)it);  // (wave-uniform: the item's record and region in scalar registers)
    if (it >= nItems) break;
    const uint4 item = items[it];
    const uint32_t setBase = item.x, nb = item.y & 0xFFu, chunk = item.y >> 8;
    if (nb == 0) continue;
    // the item's region: one list of up to `cap` photon indices per beam of the tile
    const uint2 reg = itemOff[it];
    const uint32_t cap = reg.y;
    // (a wave-uniform base and a 32-bit offset per lane, not a 64-bit pointer per lane)
    uint32_t *const outBase = pairs + (size_t)reg.x * 64u;
    const uint32_t outOff = (uint32_t)b * cap;
    uint32_t mine = 0;  // hits of this lane's beam so far (equal in the LPB lanes of the beam)
    BaseInfo bi;
    const RayReg base = loadBaseDirect<B>(a, setBase, nb, lane, bi);
    TileWalk w;
    tileSetupFrom(a, base, base.valid, w);
    const bool beamValid = w.beamValid;
    // the walk's wave-uniform bounds (the hand-off instantiation needs nothing else of TileWalk past this point)
    const int cA0 = __builtin_amdgcn_readfirstlane(w.cA0), K = __builtin_amdgcn_readfirstlane(w.K);
    const float mint = eps, maxt = base.len - eps;
    // depth + edge within [minDepth, maxDepth] (shift_volume_photon.cpp:670-673) as a window on the photon's depth
    const int dmax = a.cfg.max_depth > 0 ? a.cfg.max_depth - (int)bi.edge : 0x7FFFFFFF;
    const int dmin = a.cfg.min_depth != 0 ? a.cfg.min_depth - (int)bi.edge : -0x7FFFFFFF;
    const uint32_t pixParity = ((bi.pix & 0xFFFFu) + (bi.pix >> 16)) & 1u;
    const uint32_t fmask = 0x40u | (a.cfg.path_set ? (1u << GVPM_HOT_PARITY_BIT) : 0u);
    const uint32_t fwant = 0x40u | (a.cfg.path_set ? (pixParity << GVPM_HOT_PARITY_BIT) : 0u);
    const bool depthWindow = a.cfg.max_depth > 0 || a.cfg.min_depth != 0;  // wave-uniform
    int dlo = max(dmin, 0), dhi = min(dmax, 255);
    if (dhi < dlo) dlo = dhi = 256;  // nothing passes
    const uint32_t dspan = (uint32_t)(dhi - dlo);
    // thresholds of the conservative test.  The fp32 error of disk is below 6e-7 (|wv|_1 + |disk|) (hitBand) with
    // wv = photon - origin and |disk| <= |wv|_1.  Only pairs the reference accepts must pass, and for those the photon
    // lies within 3 r of the beam's segment: |wv|_1 <= sqrt(3) (len + 3 r), whatever the grid or the other photons are
    const float wv1 = 1.7321f * (fmaxf(base.len, 0.f) + 3.f * r);
    const float Emax = 1.25e-6f * wv1;
    const float thrD2 = beamValid ? r2f + (4.f * r * Emax + r2f * 2e-6f) : -1.f;
    const float thrLo = mint - Emax, thrHi = maxt + 2.f * r;
    // The box of a slab step holds ~3 x the photons of the tile's bounding cylinder (tile_walk.h tileCylinder): a staged
    // window is compacted to the cylinder's photons before the 16-beam pass tests it (GVPM_TRAV_PREFILTER=0: as staged).
    const bool prefilter = !(a.cfg.reserved[0] & 128);
    bool cylOk = false;
    if (prefilter) {
      // foot points of accepted photons have ray parameters in [thrLo, thrHi]; an accepted photon is within
      // sqrt(thrD2) <= r (1 + 1e-6) + 2 Emax of its foot point
      const TileCyl c = tileCylinder(base, beamValid, fminf(thrLo, 0.f) - r, thrHi + r, r, 2.f * Emax);
      cylOk = c.ok;
      // (nine wave-uniform numbers used once per staged window: parked in LDS rather than held in registers beside the
      // test loop -- the kernel's register budget is what lets the build's kernels run beside it)
      waveLdsSync();
      if (lane == 0) {
        s.cyl[0] = make_float4(c.o.x, c.o.y, c.o.z, c.R2);
        s.cyl[1] = make_float4(c.d.x, c.d.y, c.d.z, c.s0);
        s.cyl[2] = make_float4(c.s1, 0.f, 0.f, 0.f);
      }
      waveLdsSync();
    }
    const bool haveCyl = prefilter && __builtin_amdgcn_readfirstlane((int)cylOk);
    unsigned long long tested = 0;  // wave-uniform
    auto putStage = [&](uint32_t k, float4 v, uint32_t gi) {
      s.x[k] = v.x;
      s.y[k] = v.y;
      s.z[k] = v.z;
      s.bits[k] = __float_as_uint(v.w);
      s.stageIdx[k] = gi;
    };

    // (bundle cells: a heavy item is split into parts that take its staging windows round-robin, tile_walk.h)
    const bool bundle = a.grid.mode == 1;
    const uint32_t part = bundle ? (item.z >> 8) & 0xFFFu : 0u, parts = bundle ? max(item.z >> 20, 1u) : 1u;
    uint32_t winNo = 0;
    const int cBeg = max((int)(bundle ? item.z & 0xFFu : item.z), cA0),
              cEnd = min((int)item.w, __builtin_amdgcn_readfirstlane(w.cA1));
    for (int cA = cBeg; cA <= cEnd; cA += K) {
      const int cAe = min(cA + K - 1, cEnd);
      CellBox bx;
      if constexpr (OWN_WALK) {
        if (!slabBox(a, w, cA, cAe, bx)) continue;
      } else {
        // the slab's cell box: the planner's (it reduced the tile's footprints to count the box's photons), one load
        // instead of a footprint per lane, four wave reductions and the cell arithmetic per slab step.  The driver sizes
        // the boxes for every step a chunk can have: a step beyond them is counted as dropped pairs (an error, not a skip)
        const uint32_t stepIdx = (uint32_t)(cA - cA0) / (uint32_t)K;
        if (stepIdx >= a.planBoxStride) {
          nOver += lane == 0 ? 1u : 0u;
          continue;
        }
        if (!unpackCellBox(a.planBoxes[(size_t)chunk * a.planBoxStride + stepIdx], bx)) continue;
      }
      const int nranges = (bx.by1 - bx.by0 + 1) * (bx.bz1 - bx.bz0 + 1);
      for (int rbase = 0; rbase < nranges; rbase += 64) {
        uint32_t start, count;
        boxRange(a, bx, rbase + lane, nranges, start, count);
        const uint32_t incl = wave_scan_incl(count, lane);
        const uint32_t excl = incl - count;
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);  // (wave-uniform: the window loop in SGPRs)
        for (uint32_t win = 0; win < total; win += STAGE) {
          if (parts > 1u && (winNo++ % parts) != part) continue;
          // stage [win, win + STAGE) of the concatenated ranges
          waveLdsSync();
          const uint32_t nst = min((uint32_t)STAGE, total - win);
          if (total >= coalesceAt) {
            // dense boxes (C4: 4 M photons): consecutive LANES take consecutive entries of the window (the range an
            // entry falls in: a 6-step search over the exclusive scan, through ds_bpermute), so a load instruction
            // reads a few contiguous runs of records instead of 64 separate ones
#pragma unroll
            for (uint32_t k = (uint32_t)lane; k < (uint32_t)STAGE; k += 64u) {
              const uint32_t e = win + k;
              uint32_t rr = 0;
#pragma unroll
              for (uint32_t step = 32; step; step >>= 1) {
                const uint32_t cand = rr + step;
                const uint32_t v = (uint32_t)__shfl((int)excl, (int)(cand & 63u), 64);
                if (v <= e) rr = cand;
              }
              const uint32_t rStart = (uint32_t)__shfl((int)start, (int)rr, 64), rExcl = (uint32_t)__shfl((int)excl, (int)rr, 64);
              if (k < nst) {
                const uint32_t gi = rStart + (e - rExcl);
                putStage(k, a.hot[gi], gi);
              }
            }
          } else
          {
            const uint32_t lo_i = max(excl, win), hi_i = min(excl + count, win + STAGE);
            uint32_t i = lo_i;
            // (one record per lane and trip: four loads in flight per lane, as this loop had them, cost 44 VGPRs -- a
            // wave per SIMD -- and the kernel a fifth of its speed)
            for (; i < hi_i; ++i) {
              const uint32_t gi = start + (i - excl);
              putStage(i - win, a.hot[gi], gi);
            }
          }
          waveLdsSync();
          uint32_t nkeep = nst;
          if (haveCyl) {
            // compaction in place, 64 entries a round: a round's survivors go to slots at or below the round's own (every
            // lane holds its entry in registers before anything is written; later rounds' slots are not touched)
            nkeep = 0;
            const float4 c0 = s.cyl[0], c1 = s.cyl[1];
            const float cS1 = s.cyl[2].x;
            const f3 axO = mk3(c0.x, c0.y, c0.z), axD = mk3(c1.x, c1.y, c1.z);
            const float cylR2 = c0.w, cylS0 = c1.w, cylS1 = cS1;
            for (uint32_t k0 = 0; k0 < nst; k0 += 64u) {
              const uint32_t k = k0 + (uint32_t)lane;
              const bool live = k < nst;
              const float px = live ? s.x[k] : 0.f, py = live ? s.y[k] : 0.f, pz = live ? s.z[k] : 0.f;
              const uint32_t pb = live ? s.bits[k] : 0u, pi = live ? s.stageIdx[k] : 0u;
              const f3 wv = mk3(px, py, pz) - axO;
              const float sq = dot(wv, axD);
              const float d2 = dot(wv, wv) - sq * sq;
              const bool keep = live && d2 < cylR2 && sq > cylS0 && sq < cylS1 && (pb & 0x40u);
              const unsigned long long m = __ballot(keep);
              waveLdsSync();
              if (keep) {
                const uint32_t dst = nkeep + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                s.x[dst] = px; s.y[dst] = py; s.z[dst] = pz; s.bits[dst] = pb; s.stageIdx[dst] = pi;
              }
              nkeep += (uint32_t)__popcll(m);
            }
            waveLdsSync();
          }
          // the slots between the last photon and the next multiple of 16 hold photons no beam can meet
          if (lane < 16 && nkeep + (uint32_t)lane < ((nkeep + 15u) & ~15u)) s.x[nkeep + lane] = 3.0e38f;
          waveLdsSync();
          tested += nkeep;
          // groups of G * LPB staged photons: sub-lane `sub` of a beam takes G consecutive ones.  A branch-free pass
          // marks the candidates, then the wave appends them one per lane and round.
          constexpr uint32_t G = 4;
          static_assert(STAGE % (G * LPB) == 0 && G == 4, "a lane reads four consecutive photons with one b128 per component");
          for (uint32_t jb = 0; jb < nkeep; jb += G * LPB) {  // wave-uniform trip count: the append below is collective
            const uint32_t j0 = jb + (uint32_t)sub * G;
            const float4 X = *reinterpret_cast<const float4 *>(&s.x[j0]);
            const float4 Y = *reinterpret_cast<const float4 *>(&s.y[j0]);
            const float4 Z = *reinterpret_cast<const float4 *>(&s.z[j0]);
            const uint4 Bt = *reinterpret_cast<const uint4 *>(&s.bits[j0]);
            uint32_t cm = 0;
            {
              const v2f ox = {base.o.x, base.o.x}, oy = {base.o.y, base.o.y}, oz = {base.o.z, base.o.z};
              const v2f dx = {base.d.x, base.d.x}, dy = {base.d.y, base.d.y}, dz = {base.d.z, base.d.z};
              const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
              const uint32_t bs[4] = {Bt.x, Bt.y, Bt.z, Bt.w};
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const v2f wx = (v2f){xs[2 * h], xs[2 * h + 1]} - ox, wy = (v2f){ys[2 * h], ys[2 * h + 1]} - oy,
                          wz = (v2f){zs[2 * h], zs[2 * h + 1]} - oz;
                const v2f disk = wx * dx + (wy * dy + wz * dz);
                const v2f vx = wx - dx * disk, vy = wy - dy * disk, vz = wz - dz * disk;
                const v2f d2 = vx * vx + (vy * vy + vz * vz);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                  const int u = 2 * h + e;
                  // conservative: every pair the reference accepts passes (its disk test within the band -- folded into
                  // the thresholds, from the largest |photon - origin| the grid allows; beyond the beam end the
                  // own-box test admits diskDistance up to maxt + sqrt(3) r)
                  uint32_t ok = (uint32_t)(d2[e] < thrD2) & (uint32_t)(disk[e] > thrLo) & (uint32_t)(disk[e] < thrHi);
                  // the exact filters, shift_volume_photon.cpp:670-697: computeVolumeContribution + debugShift (bit 6,
                  // folded by reorderBody), checkerboard parity (bit 7), depth window
                  ok &= (uint32_t)((bs[u] & fmask) == fwant);
                  if (depthWindow) ok &= (uint32_t)((uint32_t)((int)GVPM_PF_DEPTH(bs[u]) - dlo) <= dspan);
                  cm |= ok << u;
                }
              }
            }
            if (__ballot(cm != 0u)) {
              // append: the LPB sub-lanes of a beam (lanes b, b + B, ...) write their candidates behind one another.
              // (consecutive photons are neighbours in space, so one lane often holds several of a beam's hits: a
              // collective round per hit would cost the whole wave a round for each)
              const uint32_t c = (uint32_t)__popc(cm);
              uint32_t before = 0, total = c;
              if (B <= 32) {
                const uint32_t t = (uint32_t)__shfl_xor((int)total, 32, 64);
                before += (lane & 32) ? t : 0u;
                total += t;
              }
              if (B == 16) {
                const uint32_t t = (uint32_t)__shfl_xor((int)c, 16, 64);
                // lanes with bit 4 set come after their partner; the pair with bit 5 set after the pair without
                const uint32_t pairSum = c + t;
                const uint32_t t2 = (uint32_t)__shfl_xor((int)pairSum, 32, 64);
                before = ((lane & 16) ? t : 0u) + ((lane & 32) ? t2 : 0u);
                total = pairSum + t2;
              }
              uint32_t off = mine + before;
              while (cm) {
                const uint32_t u = (uint32_t)__ffs(cm) - 1u;
                cm &= cm - 1u;
                if (off < cap) outBase[outOff + off] = s.stageIdx[j0 + u];
                else nOver++;
                ++off;
              }
              mine += total;
            }
          }
        }
      }
    }
    if (sub == 0) pairCnt[(size_t)it * B + b] = (uint32_t)b < nb ? min(mine, cap) : 0u;
    if (units) {
      // the evaluation's WORK UNITS (round 6): this item's pairs, cut into parts of at most EVAL_UNIT -- see evaluate_bre_kernel
      uint32_t tot = (sub == 0 && (uint32_t)b < nb) ? min(mine, cap) : 0u;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) tot += (uint32_t)__shfl_xor((int)tot, o, 64);
      tot = (uint32_t)__builtin_amdgcn_readfirstlane((int)tot);
      if (tot) {
        const uint32_t parts = (tot + EVAL_UNIT - 1u) / EVAL_UNIT;
        const uint32_t cls = (tot + parts - 1u) / parts > EVAL_UNIT_SMALL ? 0u : 1u;
        uint32_t slot = 0;
        if (lane == 0) slot = atomicAdd(&unitCtl[cls], parts);
        slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);
        for (uint32_t pp = (uint32_t)lane; pp < parts; pp += 64u) {
          if (slot + pp < unitCap) units[(size_t)cls * unitCap + slot + pp] = make_uint2(it, pp | (parts << 16));
          else nOver++;
        }
      }
    }
    nCand += tested * nb;  // (pairs the 16-beam pass tested)
  }
  {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nOver += (uint32_t)__shfl_xor((int)nOver, o, 64);
    if (lane == 0 && (nCand | nOver)) {
      unsigned long long *row = statRow(a);
      atomicAdd(&row[1], nCand);
      if (nOver) atomicAdd(&row[7], (unsigned long long)nOver);  // must stay 0: the planner's bound is exact
    }
  }
}

// (evaluate_bre_kernel, its helpers and its launcher: gather_bre_eval.hip, a unit of its own with its own compiler flags)

// ------------------------------------------------------------------------------------------
// The PRIMAL beam radiance estimate (second half): BeamRadianceEstimator::query,
// src/integrators/photonmapper/bre.cpp:166-254, as SPPMIntegrator::volumePhotonPassBRE drives it (sppm.cpp:882-1000,
// cameraHeuristic = true: the gradient pass's uniform radius).  A strict subset of the gradient gather: same grid, planner,
// traversal and pair lists; this kernel walks an item's lists like evaluate_bre_kernel but evaluates the primal query's
// term only -- re-based ray (:168), stored power without sigma_s, one random number PER HIT for the 3D kernel (Philox keyed
// by the beam's `rand` and the photon's position bits: the reference's comes from a stateful sampler in traversal order),
// a far check for the 2D kernel (:240-242), no checkerboard, no shifts.  The hit decision is the reference's own, in
// uncontracted fp64 in its operation order (this is not the headline kernel: no banded fp32 fast path), so the evaluated
// set equals the fp64 oracle's (oracle/gvpm_oracle_primal.hpp); radiometry fp32.
// ------------------------------------------------------------------------------------------
template <int B> struct PrimalLds : RayTile<B> {
  double acc[3][B];
  uint32_t boff[B + 1];
};

__device__ __forceinline__ float primalHitRandom(float setRand, f3 pos) {
  uint32_t k0 = __float_as_uint(setRand), k1 = 0x70726d6cu;
  uint32_t c0 = __float_as_uint(pos.x), c1 = __float_as_uint(pos.y), c2 = __float_as_uint(pos.z), c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return (float)(c0 >> 8) * (1.0f / 16777216.0f);
}

// bre.cpp:168-223 / :240-242 for one (photon, beam) pair: accepted?  tR: the distance the transmittance is taken over
// (on the re-based ray), deltaT: half the kernel's chord.
__device__ __forceinline__ bool primalDecide(f3 pf, f3 of, f3 df, float len, float r, float eps, float setRand, bool use3D,
                                             double &tR, double &deltaT) {
#pragma clang fp contract(off)
  const double mint = (double)eps, maxtRay = (double)len - (double)eps;
  const double dx = df.x, dy = df.y, dz = df.z;
  // ray = Ray(r(r.mint), r.d, 0, r.maxt - r.mint)
  const double ox = (double)of.x + dx * mint, oy = (double)of.y + dy * mint, oz = (double)of.z + dz * mint;
  const double maxt = maxtRay - mint;
  const double px = pf.x, py = pf.y, pz = pf.z;
  const double cx = px - ox, cy = py - oy, cz = pz - oz;
  const double disk = cx * dx + cy * dy + cz * dz;
  const double qx = ox + dx * disk, qy = oy + dy * disk, qz = oz + dz * disk;
  const double vx = qx - px, vy = qy - py, vz = qz - pz;
  const double distSqr = vx * vx + vy * vy + vz * vz;
  const double radius = (double)r, radSqr = radius * radius;
  tR = disk;
  deltaT = 0.0;
  if (!(disk > 0 && distSqr < radSqr)) return false;
  if (use3D) {
    if (disk - (radius * 2) > maxt) return false;
    deltaT = sqrt(radSqr - distSqr);
    const double tminKernel = disk - deltaT;
    tR = tminKernel + 2 * deltaT * (double)primalHitRandom(setRand, pf);
    return !(tR < 0 || tR > maxt);
  }
  return !(disk > maxt);
}

template <int B>
__global__ __launch_bounds__(64) void evaluate_primal_kernel(GatherArgs a, const uint4 *__restrict__ items,
                                                             const uint2 *__restrict__ itemOff,
                                                             const uint32_t *__restrict__ itemCount, uint32_t *queueHead,
                                                             const uint32_t *__restrict__ pairs,
                                                             const uint32_t *__restrict__ pairCnt) {
  __shared__ PrimalLds<B> s;
  const int lane = threadIdx.x;
  const uint32_t nItems = *itemCount;
  const bool use3D = a.cfg.vol_technique == GVPM_VOL_BRE3D;
  const float r = a.radius;
  const float kernelVol = use3D ? (4.0f / 3.0f) * 3.14159265358979323846f * r * r * r : 3.14159265358979323846f * r * r;
  const float weight = 1.f / kernelVol;
  unsigned long long nEval = 0;
  bool firstItem = true;
  for (;;) {
    uint32_t it = blockIdx.x;
    if (!firstItem) {
      if (lane == 0) it = gridDim.x + atomicAdd(queueHead, 1u);
      it = __shfl(it, 0, 64);
    }
    firstItem = false;
    if (it >= nItems) break;
    const uint4 item = items[it];
    const uint32_t setBase = item.x, nb = item.y & 0xFFu;
    if (nb == 0) continue;
    const uint32_t cntb = (uint32_t)lane < nb ? pairCnt[(size_t)it * B + lane] : 0u;
    const uint32_t incl = wave_scan_incl(cntb, lane);
    const uint32_t total = __shfl(incl, 63, 64);
    if (total == 0) continue;
    const uint2 reg = itemOff[it];
    const uint32_t *lists = pairs + (size_t)reg.x * 64u;
    const uint32_t cap = reg.y;
    __syncthreads();
    if (lane < B) s.boff[lane + 1] = incl;
    if (lane == 0) s.boff[0] = 0u;
    loadTileRaysNoSync<B>(a, s, setBase, nb, lane);
    for (int idx = lane; idx < 3 * B; idx += 64) (&s.acc[0][0])[idx] = 0.0;
    __syncthreads();
    const uint32_t chunk = (total + 63u) / 64u;
    const uint32_t g0 = min(total, (uint32_t)lane * chunk), g1 = min(total, g0 + chunk);
    uint32_t cur = 0;
    if (g0 < g1)
      while (s.boff[cur + 1] <= g0) cur++;
    f3 sum = mk3(0.f);
    bool dirty = false;
    for (uint32_t g = g0; g < g1; ++g) {
      uint32_t b = cur;
      while (s.boff[b + 1] <= g) b++;
      if (b != cur) {
        if (dirty) {
          atomicAdd(&s.acc[0][cur], (double)sum.x);
          atomicAdd(&s.acc[1][cur], (double)sum.y);
          atomicAdd(&s.acc[2][cur], (double)sum.z);
        }
        sum = mk3(0.f);
        dirty = false;
        cur = b;
      }
      const uint32_t pidx = lists[(size_t)b * cap + (g - s.boff[b])];
      const PhotonFront ph = loadFront(a, pidx);
      const RayReg base = loadRay(s, 0, cur);
      double tR, deltaT;
      if (!primalDecide(ph.pos, base.o, base.d, base.len, r, a.cfg.epsilon, s.rnd[cur], use3D, tR, deltaT)) continue;
      // result += Tr * power * phase(wi, -d) * (weight * scaleFactor) [* max(2 deltaT, 1e-4)]; * beam.weight (sppm.cpp:976-981)
      f3 trT;
      float dummy;
      mediumEval(a.med, (float)tR, trT, dummy);
      const float inv = use3D ? fmaxf(2.f * (float)deltaT, 0.0001f) : 1.f;
      sum = sum + ph.flux * base.eye * (trT.x * phaseEval(a.med.g, ph.wi, -base.d) * weight * inv);
      dirty = true;
      nEval++;
    }
    if (dirty) {
      atomicAdd(&s.acc[0][cur], (double)sum.x);
      atomicAdd(&s.acc[1][cur], (double)sum.y);
      atomicAdd(&s.acc[2][cur], (double)sum.z);
    }
    __syncthreads();
    for (int idx = lane; idx < 3 * B; idx += 64) {
      const int k = idx / B, bb = idx % B;
      if ((uint32_t)bb < nb) {
        const float v = (float)s.acc[k][bb];
        if (v != 0.f) {
          const uint32_t pv = s.pix[bb];
          atomicAdd(&a.iter[((size_t)(pv >> 16) * a.cfg.width + (pv & 0xFFFFu)) * 27 + k], v * a.iterScale);
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nEval += __shfl_xor(nEval, o, 64);
  if (lane == 0 && nEval) atomicAdd(&statRow(a)[0], nEval);
}

void launch_evaluate_primal(const GatherArgs &a, int beamsPerWave, const uint4 *items, const uint2 *itemOff,
                            const uint32_t *itemCount, uint32_t *queueHead, const uint32_t *pairs, const uint32_t *pairCnt,
                            uint32_t nwaves, hipStream_t stream) {
  if (a.nsets == 0 || nwaves == 0) return;
  switch (beamsPerWave) {
    case 64: hipLaunchKernelGGL(evaluate_primal_kernel<64>, dim3(nwaves), dim3(64), 0, stream, a, items, itemOff, itemCount, queueHead, pairs, pairCnt); break;
    case 32: hipLaunchKernelGGL(evaluate_primal_kernel<32>, dim3(nwaves), dim3(64), 0, stream, a, items, itemOff, itemCount, queueHead, pairs, pairCnt); break;
    default: hipLaunchKernelGGL(evaluate_primal_kernel<16>, dim3(nwaves), dim3(64), 0, stream, a, items, itemOff, itemCount, queueHead, pairs, pairCnt); break;
  }
}

// itemCount / blockTotal must be zero on entry (memset on the same stream)
void launch_plan_bre(const GatherArgs &a, int beamsPerWave, uint32_t ntiles, uint32_t target, uint4 *items,
                     uint32_t *itemCount, uint2 *itemOff, uint32_t *blockTotal, uint32_t itemCap, hipStream_t stream) {
  if (a.nsets == 0 || ntiles == 0) return;
  // waves stride over the tiles; the stride is prime because image-sharded input owns every N-th tile, and a
  // stride that is a multiple of N would leave all the work to 1/N of the blocks
  const uint32_t nwg = ntiles < 4093u ? ntiles : 4093u;
  switch (beamsPerWave) {
    case 64: hipLaunchKernelGGL(plan_kernel<64>, dim3(nwg), dim3(64), 0, stream, a, ntiles, target, items, itemCount, itemOff, blockTotal, itemCap); break;
    case 32: hipLaunchKernelGGL(plan_kernel<32>, dim3(nwg), dim3(64), 0, stream, a, ntiles, target, items, itemCount, itemOff, blockTotal, itemCap); break;
    default: hipLaunchKernelGGL(plan_kernel<16>, dim3(nwg), dim3(64), 0, stream, a, ntiles, target, items, itemCount, itemOff, blockTotal, itemCap); break;
  }
}

// queueHead must be zero on entry
void launch_traverse_bre(const GatherArgs &a, int beamsPerWave, const uint4 *items, const uint2 *itemOff,
                         const uint32_t *itemCount, uint32_t *queueHead, uint32_t *pairs, uint32_t *pairCnt,
                         uint32_t nwaves, bool persistent, hipStream_t stream, uint2 *units, uint32_t *unitCtl, uint32_t unitCap) {
  if (a.nsets == 0 || nwaves == 0) return;
  const uint32_t persist = persistent ? 1u : 0u;
  const dim3 grid((nwaves + TRAV_WPB - 1) / TRAV_WPB), block(64 * TRAV_WPB);
#define GVPM_LAUNCH_TRAV(BB, OWN) \
  hipLaunchKernelGGL((traverse_bre_kernel<BB, OWN>), grid, block, 0, stream, a, items, itemOff, itemCount, queueHead, pairs, pairCnt, \
                     persist, units, unitCtl, unitCap)
  // (the driver hands the planner's boxes over whenever it can size them, drivers_bre.hip)
  const bool own = a.planBoxes == nullptr;
  switch (beamsPerWave) {
    case 64: if (own) GVPM_LAUNCH_TRAV(64, true); else GVPM_LAUNCH_TRAV(64, false); break;
    case 32: if (own) GVPM_LAUNCH_TRAV(32, true); else GVPM_LAUNCH_TRAV(32, false); break;
    default: if (own) GVPM_LAUNCH_TRAV(16, true); else GVPM_LAUNCH_TRAV(16, false); break;
  }
#undef GVPM_LAUNCH_TRAV
}

uint32_t plan_items_capacity(uint32_t nsets, uint32_t ntiles, int beamsPerWave) {
  return (ntiles + nsets / (uint32_t)beamsPerWave + 1u) * (uint32_t)PLAN_MAX_ITEMS;
}

}  // namespace gvpm
