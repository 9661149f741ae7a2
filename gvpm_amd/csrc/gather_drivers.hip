// gvpm_gather (C ABI, include/gvpm_hip.h) and what its per-technique drivers share: the kernel arguments, the exact pass's
// cadence, the phase events, the host-shift requests and the APA radius update; the G-Planes step; the host-shift C ABI.
// The other techniques' steps are drivers_bre.hip, drivers_beams.hip and drivers_vpm.hip, their builds drivers_build.hip.
// Mirrors GPMIntegrator::photonMapPass and the computeVolumeGradient* drivers (gvpm/gvpm.cpp:383-500, 880-1180).
#include "drivers.h"
#include "staging.h"

float currentRadius(const gvpm_context *h) {
  // breInitSize = bsphere.radius * globalScaleVolume * POURCENTAGE_BS, gvpm.cpp:989 (Float = float)
  return h->cfg.bsphere_radius * h->globalScaleVolume * 0.01f;
}

bool needFullVis(const gvpm_context *h) {
  return !h->cfg.visibility_as_written || h->nearOverflow;
}

void fillArgs(const gvpm_context *h, GatherArgs &a, float r) {
  memset(&a, 0, sizeof(a));
  a.hot = h->bs->hot.p;
  a.cold = h->bs->cold.p;
  a.cellStart = h->bs->cellStart.p;
  a.nearExt = h->bs->nearExt.p;
  a.sat = h->bs->sat.p;
  a.nph = h->nph;
  a.grid = h->bs->grid;
  a.rays = h->raysDev;
  a.setPerm = h->bs->setPerm.p;
  a.tileStart = h->bs->tileStart.p;
  a.nsets = h->nsets;
  a.tri4 = h->tri4.p;
  a.bvh = h->bvh.p;
  a.ntri = h->ntri;
  a.triAbs1 = 0.f;
  if (h->ntri)
    for (int c = 0; c < 3; ++c) a.triAbs1 += fmaxf(fabsf(h->triMin[c]), fabsf(h->triMax[c]));
  for (int c = 0; c < 3; ++c) {
    a.med.sigmaS[c] = h->medium.sigma_s[c];
    a.med.sigmaT[c] = h->medium.sigma_t[c];
  }
  a.med.g = h->medium.g;
  a.med.msw = h->medium.medium_sampling_weight;
  a.cfg = h->cfg;
  if (h->bsdfMixtures) a.cfg.reserved[0] |= GVPM_TABLE_HAS_MIXTURE;  // (gather_bre_eval.hip, launch_evaluate_bre)
  a.radius = r;
  a.iter = h->iter.p;
  a.stats = h->stats.p;
  a.samples = h->samplesDev;
  a.nsamples = h->nsamples;
  a.scaleVol = h->scaleVol.p;
  a.mvol = h->mvol.p;
  a.kernelRadius = r;
  a.subLen = 0.f;
  a.nbeams = 0;
  a.bsdfs = h->bsdfs.p;
  a.nbsdfs = h->nbsdfs;
  a.vpmOrder = nullptr;
  a.vpmOrderN = 0;
  a.vpmCostKey = a.vpmCostVal = nullptr;
  a.exPay = h->exPay.p;
  a.exPayCount = h->exPayCount.p;
  a.exPayCap = h->exPay.p ? h->exPayCap : 0u;
  a.exOvf = h->exOvf.p;
  a.exOvfCount = h->exOvfCount.p;
  a.exOvfCap = a.exOvf ? h->exOvfCap : 0u;
}

// The exact pass over the shifts the gathers deferred (exact_shift.hip): on the gather stream, when a reader asks
// (gvpm_join_exact) or every exFlushEvery gathers.
// whatever reads or rescales the sums on the gather stream waits for the last readers of every build set
int joinEvalStreams(gvpm_context *h) {
  if (h->streamA2)
    for (BuildSet &b : h->sets)
      if (b.lastUseValid && b.lastUse) HIP_TRY(h, hipStreamWaitEvent(h->stream, b.lastUse, 0));
  return GVPM_OK;
}
int gvpm_join_exact(gvpm_context *h) {
  {
    const int rcj = joinEvalStreams(h);
    if (rcj != GVPM_OK) return rcj;
  }
  if (h->exSince == 0) return GVPM_OK;
  GatherArgs a;
  fillArgs(h, a, 0.f);
  a.hot = a.cold = nullptr;
  a.rays = nullptr;
  a.iter = h->accum.p;
  launch_exact_pass(a, h->exTotals.p, h->pinExact, h->stream);
  HIP_TRY(h, hipGetLastError());
  // (the pass empties the handle's entry list: the capture kernels of later evaluations come after it on this stream)
  h->exSinceAtLast = h->exSince;
  h->exSince = 0;
  return GVPM_OK;
}
int exactPrepare(gvpm_context *h) {
  // (the list starts at 2^17 entries -- 64 MB, not 512 -- and is regrown, with the pass that empties it in front,
  // when a pass has found it more than a quarter full; the measured rate is ~1e-5 of the shifts)
  if (h->exPay.p && h->pinExact && h->pinExact[0] != 0xFFFFFFFFu && h->pinExact[0] > h->exPayCap / 4u && h->exPayCap < (1u << 22)) {
    const int rcj = gvpm_join_exact(h);
    if (rcj != GVPM_OK) return rcj;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->streamA2) HIP_TRY(h, hipStreamSynchronize(h->streamA2));
    h->exPay.release();
    h->exPayCap *= 4u;
    h->pinExact[0] = 0u;
  }
  HIP_TRY(h, h->exPay.reserveExact(h->exPayCap));
  HIP_TRY(h, h->exOvf.reserveExact(h->exOvfCap));
  if (!h->pinExact) {
    HIP_TRY(h, hipHostMalloc((void **)&h->pinExact, 64, hipHostMallocMapped));
    h->pinExact[0] = 0xFFFFFFFFu;  // (no pass has reported yet)
  }
  return GVPM_OK;
}
int exactAfterGather(gvpm_context *h) {
  if (!h->exFlushFixed && h->pinExact[0] != 0xFFFFFFFFu) {
    // what the last pass found per gather it covered (read without waiting: a stale number only delays the adjustment)
    const uint32_t perGather = h->pinExact[0] / std::max(1u, h->exSinceAtLast) + 1u;
    h->exFlushEvery = std::max(1u, std::min(256u, (h->exPayCap / 4u) / perGather));
    if (h->trace & TRACE_EXACT) fprintf(stderr, "[exact] last pass found %u entries over %u gathers -> a pass every %u gathers (since %u)\n", h->pinExact[0], h->exSinceAtLast, h->exFlushEvery, h->exSince);
  }
  if (++h->exSince >= h->exFlushEvery) return gvpm_join_exact(h);
  return GVPM_OK;
}
int nextEvents(gvpm_context *h, EventPair **ev, int phase) {
  // HIP events on the handle's stream bracket the dominant kernel (roofline.achieved) and the other phases
  // a ring of at most GVPM_EVENT_RING pairs per phase: a host that never polls gvpm_get_phase_time keeps the timings of
  // its last launches instead of growing the pool by three pairs per step
  constexpr size_t GVPM_EVENT_RING = 256;
  if (h->eventsHead[phase] == h->events[phase].size()) {
    if (h->events[phase].size() >= GVPM_EVENT_RING) {
      h->eventsHead[phase] = 0;  // overwrite the oldest
    } else {
      hipEvent_t e0, e1;
      HIP_TRY(h, hipEventCreate(&e0));
      HIP_TRY(h, hipEventCreate(&e1));
      h->events[phase].emplace_back(e0, e1);
    }
  }
  *ev = &h->events[phase][h->eventsHead[phase]++];
  h->eventsCount[phase] = std::min(h->eventsCount[phase] + 1, GVPM_EVENT_RING);
  return GVPM_OK;
}

int ensurePinned(gvpm_context *h) {
  if (h->pinB6) return GVPM_OK;
  HIP_TRY(h, hipHostMalloc((void **)&h->pinB6, 256, hipHostMallocMapped));
  memset(h->pinB6, 0, 256);
  h->pinCtl = reinterpret_cast<uint32_t *>(h->pinB6 + 8);
  return GVPM_OK;
}

int armHostShiftRequests(gvpm_context *h, GatherArgs &a, int ctxStride, bool wantOrigIdx, float *iter, float iterScale, bool beams,
                         hipStream_t s) {
  HIP_TRY(h, h->reqHost.ensure(h->reqCap));
  HIP_TRY(h, h->reqCtx.ensure((size_t)ctxStride * h->reqCap));
  HIP_TRY(h, h->reqCount.ensure(2));
  HIP_TRY(h, hipMemsetAsync(h->reqCount.p, 0, 8, s));
  a.reqHost = h->reqHost.p;
  a.reqCtx = h->reqCtx.p;
  a.reqCount = h->reqCount.p;
  a.reqCap = (uint32_t)h->reqCap;
  if (wantOrigIdx) a.origIdx = h->bs->origIdx.p;
  h->reqArgs = a;
  h->reqArgs.iter = iter;
  h->reqArgs.iterScale = iterScale;
  h->reqOutstanding = true;
  h->reqBeams = beams;
  return GVPM_OK;
}

void scaleVolumeAPA(gvpm_context *h, int it) {
  // the exponent follows the kernel's dimension (gvpm.cpp:195-201): cube root for the 3D kernels, square root for the 2D
  // one, the ratio itself for the 1D beam kernel and the plane estimator
  const double ratio = ((it - 1) + (double)h->cfg.alpha) / ((it - 1) + 1);
  double f = std::cbrt(ratio);
  if (h->cfg.vol_technique == GVPM_VOL_BRE2D) f = std::sqrt(ratio);
  else if (h->cfg.vol_technique == GVPM_BEAM_BEAM_1D || h->cfg.vol_technique == GVPM_VOL_PLANE0D) f = ratio;
  h->globalScaleVolume = (float)(h->globalScaleVolume * f);
}

// computeVolumeGradientPlanes, gvpm.cpp:782-878
static int gatherPlanes(gvpm_context *h, int it, uint64_t nb_paths) {
  if (!h->havePlanes) return fail(h, GVPM_ERR_STATE, "G-Planes gather needs gvpm_upload_planes");
  PlaneArgs pa;
  pa.ori = h->rawDev.parent_pos;
  pa.end = h->rawDev.pos;
  pa.flux = h->rawDev.flux;
  pa.flags = h->rawDev.flags;
  pa.w1 = h->w1Dev;
  pa.len1 = h->len1Dev;
  pa.nplanes = h->nph;
  pa.planesPerItem = h->nph;
  if (h->photonsDirty) {
    HIP_TRY(h, h->planeTest.ensure((size_t)h->nph * 3 + 1));
    pa.test = h->planeTest.p;
    launch_plane_records(pa, h->planeTest.p, h->stream);
    h->photonsDirty = false;
    h->bs->builtRadius = -1.f;
  }
  pa.test = h->planeTest.p;
  if (h->beamsDirty) {
    int rc = sortBeams(h, 64);  // one camera ray per lane: 8x8 pixel tiles
    if (rc != GVPM_OK) return rc;
    h->beamsDirty = false;
  }
  h->iterClean = false;
  HIP_TRY(h, hipMemsetAsync(h->iter.p, 0, h->npix * 27 * sizeof(float), h->stream));
  GatherArgs a;
  fillArgs(h, a, 0.f);
  // enough (tile, plane chunk) items to fill the chip; chunks of at least 256 planes
  uint32_t nchunks = 1;
  if (h->bs->ntiles && h->nph) {
    nchunks = (4u * h->nwaves + h->bs->ntiles - 1) / h->bs->ntiles;
    nchunks = std::max(1u, std::min(nchunks, (h->nph + 255u) / 256u));
    nchunks = std::min(nchunks, 65535u);
    pa.planesPerItem = (h->nph + nchunks - 1) / nchunks;
    nchunks = (h->nph + pa.planesPerItem - 1) / pa.planesPerItem;
  }
  EventPair *ev;
  int rc = nextEvents(h, &ev);
  if (rc != GVPM_OK) return rc;
  HIP_TRY(h, hipEventRecord(ev->first, h->stream));
  launch_gather_planes(a, pa, h->bs->ntiles, nchunks, h->stream);
  HIP_TRY(h, hipEventRecord(ev->second, h->stream));
  launch_finalize(h->accum.p, h->iter.p, h->npix * 27, it, nb_paths, h->stream);
  HIP_TRY(h, hipGetLastError());
  scaleVolumeAPA(h, it);
  return GVPM_OK;
}

// ---- manifold shifts through the host (include/gvpm_hip.h) --------------------------------------------------------------
static int requestCount(gvpm_context *h, uint32_t *n) {
  uint32_t c = 0;
  HIP_TRY(h, hipMemcpyAsync(&c, h->reqCount.p, 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  *n = (uint32_t)std::min<uint64_t>(c, h->reqCap);
  return GVPM_OK;
}
int flushHostShifts(gvpm_context *h) {
  if (!h->reqOutstanding) return GVPM_OK;
  h->reqOutstanding = false;
  uint32_t n = 0;
  const int rc = requestCount(h, &n);
  if (rc != GVPM_OK) return rc;
  if (h->reqBeams) launch_apply_host_shifts_beams(h->reqArgs, nullptr, n, h->stream);
  else launch_apply_host_shifts(h->reqArgs, nullptr, n, h->stream);
  HIP_TRY(h, hipGetLastError());
  return GVPM_OK;
}

extern "C" {

int gvpm_enable_host_shifts(gvpm_context *h, uint64_t capacity) {
  CHECK_H(h);
  if (capacity > 0x7FFFFFF0ull) return fail(h, GVPM_ERR_INVALID_ARG, "host-shift capacity too large");
  const int rc = flushHostShifts(h);
  if (rc != GVPM_OK) return rc;
  h->reqCap = capacity;
  h->photonsDirty = true;  // (the next build writes the upload index of every photon)
  return GVPM_OK;
}

int gvpm_download_shift_requests(gvpm_context *h, gvpm_shift_request *out, uint64_t cap, uint64_t *n) {
  CHECK_H(h);
  if (!n || (cap && !out)) return GVPM_ERR_INVALID_ARG;
  *n = 0;
  if (!h->reqOutstanding) return GVPM_OK;
  uint32_t c = 0;
  const int rc = requestCount(h, &c);
  if (rc != GVPM_OK) return rc;
  *n = c;
  const size_t m = (size_t)std::min<uint64_t>(c, cap);
  if (m) HIP_TRY(h, hipMemcpy(out, h->reqHost.p, m * sizeof(gvpm_shift_request), hipMemcpyDeviceToHost));
  return GVPM_OK;
}

int gvpm_upload_host_shifts(gvpm_context *h, const gvpm_host_shift *results, uint64_t n) {
  CHECK_H(h);
  if (!h->reqOutstanding) return n == 0 ? GVPM_OK : fail(h, GVPM_ERR_STATE, "no shift requests are waiting for results");
  if (n && !results) return fail(h, GVPM_ERR_INVALID_ARG, "null host shifts");
  uint32_t c = 0;
  const int rc = requestCount(h, &c);
  if (rc != GVPM_OK) return rc;
  if (n != c) return fail(h, GVPM_ERR_INVALID_ARG, "gvpm_upload_host_shifts: one result per recorded request");
  h->reqOutstanding = false;
  if (!c) return GVPM_OK;
  HIP_TRY(h, h->reqResults.ensure(c));
  HIP_TRY(h, hipMemcpyAsync(h->reqResults.p, results, (size_t)c * sizeof(gvpm_host_shift), hipMemcpyHostToDevice, h->stream));
  if (h->reqBeams) launch_apply_host_shifts_beams(h->reqArgs, h->reqResults.p, c, h->stream);
  else launch_apply_host_shifts(h->reqArgs, h->reqResults.p, c, h->stream);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (the caller may reuse `results`)
  return GVPM_OK;
}

static int gatherEntry(gvpm_context *h, int it, uint64_t nb_paths, bool primal);
int gvpm_gather(gvpm_context *h, int it, uint64_t nb_paths) {
  CHECK_H(h);
  return gatherEntry(h, it, nb_paths, false);
}
int gvpm_gather_primal(gvpm_context *h, int it, uint64_t nb_paths) {
  CHECK_H(h);
  const gvpm_params &c = h->cfg;
  if (c.vol_technique == GVPM_VOL_PLANE0D || c.vol_technique == GVPM_BEAM_BEAM_3D_NAIVE || c.vol_technique == GVPM_BEAM_BEAM_3D_EGSR)
    return fail(h, GVPM_ERR_UNSUPPORTED, "gvpm_gather_primal: built for BRE 2D / 3D, DISTANCE, BEAM_BEAM_1D and BEAM_BEAM_3D_OPTIMIZED");
  // the primal pass has none of the gradient pass's filters (sppm.cpp:882-1000): the handle must not carry them
  if (c.path_set || c.debug_shift != GVPM_SHIFT_ALL || c.min_depth != 0 || c.bsdf_interaction_mode != GVPM_BSDF_ALL ||
      !((c.lighting_interaction_mode & GVPM_SURF2MEDIA) && (c.lighting_interaction_mode & GVPM_MEDIA2MEDIA)))
    return fail(h, GVPM_ERR_UNSUPPORTED, "gvpm_gather_primal: path_set, debug_shift, min_depth and the interaction modes must be neutral");
  return gatherEntry(h, it, nb_paths, true);
}
static int gatherEntry(gvpm_context *h, int it, uint64_t nb_paths, bool primal) {
  if (it < 1 || nb_paths == 0) return fail(h, GVPM_ERR_INVALID_ARG, "it must be >= 1 and nb_paths > 0");
  if (!h->haveMedium || !h->havePhotons || !h->haveBeams)
    return fail(h, GVPM_ERR_STATE, "gather needs medium, photons and camera beams uploaded");
  h->useAll = false;
  h->bstream = h->stream;
  {
    const int rcf = flushHostShifts(h);
    if (rcf != GVPM_OK) return rcf;
  }
  // the streams that read this step's host-uploaded inputs wait for their copies (copy stream)
  // (packed records are decoded here, at the head of the chain that reads them: G-BRE builds on the build stream)
  const bool breTech = h->cfg.vol_technique == GVPM_VOL_BRE2D || h->cfg.vol_technique == GVPM_VOL_BRE3D;
  {
    // G-BRE and G-VPM keep plain sums: the exact pass may add its terms whenever it runs.  The beam / plane gathers fold
    // iter[] into running means on the gather stream: entries that wait are taken first.
    const bool sums = (breTech || h->cfg.vol_technique == GVPM_DISTANCE) && !primal;
    if (!sums) {
      const int rcj = gvpm_join_exact(h);
      if (rcj != GVPM_OK) return rcj;
    }
  }
  hipStream_t us = breTech && h->pipeline ? h->streamB : h->stream, other = us == h->stream ? h->streamB : h->stream;
  if (int rcs = stagingHead(h, us, other)) return rcs;
  h->gatheredPh = h->rawDev;
  h->gatheredPh.n = h->nph;
  h->gatheredRays = h->raysDev;
  h->gatheredSets = h->nsets;
  h->haveGathered = true;
  {
    const int t = h->cfg.vol_technique;
    h->gatheredSide = t == GVPM_VOL_PLANE0D ? gvpm_context::SIDE_PLANES
                      : (t == GVPM_BEAM_BEAM_1D || t == GVPM_BEAM_BEAM_3D_OPTIMIZED) ? gvpm_context::SIDE_BEAMS : gvpm_context::SIDE_NONE;
    h->gatheredEndN = h->endNDev;
    h->gatheredW1 = h->w1Dev;
    h->gatheredLen1 = h->len1Dev;
    h->gatheredVpm = t == GVPM_DISTANCE;
    h->gatheredSamples = h->samplesDev;
    h->gatheredNSamples = h->gatheredVpm ? h->nsamples : 0u;
  }
  int rc;
  switch (h->cfg.vol_technique) {
    case GVPM_VOL_BRE2D:
    case GVPM_VOL_BRE3D: rc = gatherBRE(h, it, nb_paths, primal); break;
    case GVPM_DISTANCE: rc = gatherVPM(h, it, nb_paths, primal); break;
    case GVPM_BEAM_BEAM_1D:
    case GVPM_BEAM_BEAM_3D_OPTIMIZED: rc = gatherBeams(h, it, nb_paths, primal); break;
    case GVPM_VOL_PLANE0D: rc = gatherPlanes(h, it, nb_paths); break;
    default: return fail(h, GVPM_ERR_UNSUPPORTED, "vol_technique not built in this library yet");
  }
  if (rc != GVPM_OK) return rc;
  // the kernels just queued are the last readers of the staged inputs; prefetched inputs become the current ones
  return stagingTail(h);
}
}  // extern "C"
