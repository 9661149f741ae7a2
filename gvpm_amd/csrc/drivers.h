// What the host-only driver units share: drivers_build.hip (photon grid, beam sort), drivers_bre.hip, drivers_beams.hip,
// drivers_vpm.hip (one technique's step each) and gather_drivers.hip (the helpers below, G-Planes, the host-shift C ABI and
// gvpm_gather).  No device code in any of them.
#pragma once
#include "context.h"

using EventPair = std::pair<hipEvent_t, hipEvent_t>;

static inline int ilog2ceil(uint32_t v) {
  int b = 0;
  while ((1ull << b) < v) ++b;
  return b;
}

// A driver that builds on another stream than the gather stream holds one of these: h->bstream goes back to the gather
// stream on every exit, the early returns of HIP_TRY included.
struct BuildStreamGuard {
  gvpm_context *h;
  BuildStreamGuard(gvpm_context *h_, hipStream_t s) : h(h_) { h->bstream = s; }
  ~BuildStreamGuard() { h->bstream = h->stream; }
  BuildStreamGuard(const BuildStreamGuard &) = delete;
  BuildStreamGuard &operator=(const BuildStreamGuard &) = delete;
};

// G-BRE's build as one chain of launches (build_chain.hip, launch_build_chain): buildGrid / sortBeams then only size the
// buffers and the grid and leave here what the chain's launcher needs.
struct ChainPrep {
  bool on = false;
  float dmax = 0.f;
  bool wantOrig = false;
  uint32_t *sub = nullptr;
  uint32_t nkeys = 0, tileShift = 0;  // the beam sort's key space (sortBeams)
  int tw = 4, th = 4;
};

// how buildGrid gets the photons' bounds and which cells it may choose
struct GridBuild {
  bool deferred = false;            // G-BRE: the previous photon set's bounds when there are any, this set's left in flight (pinB6)
  bool force3D = false;             // G-BRE: no bundle cells for this build
  const float *knownB6 = nullptr;   // the bounds, already on the host (the caller read them back with something else)
  ChainPrep *chain = nullptr;       // G-BRE: size only, the build chain does the launches
};

// ---- drivers_build.hip (everything on h->bstream) ----
// tile shape and key space of the beam sort for `beamsPerWave` sets per wave
void beamTiling(const gvpm_context *h, int beamsPerWave, int &tw, int &th, uint32_t &ntiles, int &tileShift);
// uniform grid over the photons for kernel radius r
int buildGrid(gvpm_context *h, float r, const GridBuild &how = GridBuild{});
int sortBeams(gvpm_context *h, int beamsPerWave = 0, const ChainPrep *cp = nullptr);

// ---- gather_drivers.hip ----
void fillArgs(const gvpm_context *h, GatherArgs &a, float r);
// shadow rays through the occluder BVH instead of the per-photon near-occluder lists
bool needFullVis(const gvpm_context *h);
// before a gather that can defer shifts to the exact pass: the lists exist; after its kernels have been queued: the cadence
int exactPrepare(gvpm_context *h);
int exactAfterGather(gvpm_context *h);
// the next event pair of phase 0 = dominant kernel, 1 = traversal, 2 = build (gvpm_get_phase_time)
int nextEvents(gvpm_context *h, EventPair **ev, int phase = 0);
// the pinned words the build kernels report through: pinB6 (bounds) and pinCtl (counters)
int ensurePinned(gvpm_context *h);
// Manifold-typed shifts are recorded for the host (gvpm_download_shift_requests) instead of failing: the request buffers
// into `a` (ctxStride float4 of context a request; origIdx where requests name photons), zeroed on `s`, and a copy of `a`
// that adds the answered terms to `iter` with weight `iterScale` kept for the apply kernel (beams: the G-Beams one).
int armHostShiftRequests(gvpm_context *h, GatherArgs &a, int ctxStride, bool wantOrigIdx, float *iter, float iterScale, bool beams,
                         hipStream_t s);
// scaleVolumeAPA(it), gvpm.cpp:181-215 (m_independentScale = false, forceAPA empty): the radius for the next iteration
void scaleVolumeAPA(gvpm_context *h, int it);

// ---- one technique each ----
int gatherBRE(gvpm_context *h, int it, uint64_t nb_paths, bool primal);    // drivers_bre.hip
int gatherBeams(gvpm_context *h, int it, uint64_t nb_paths, bool primal);  // drivers_beams.hip
int gatherVPM(gvpm_context *h, int it, uint64_t nb_paths, bool primal);    // drivers_vpm.hip
