// The G-VPM step: computeVolumeGradientPhoton, gvpm.cpp:1081-1203.  Host code only.
#include "drivers.h"

// The bound on the largest per-pixel scale and, when the photons or the cell size it gives have changed, the grid -- built on
// the build stream into the other build set (pipelined) or on the gather stream.  rmax: the radius the cells were sized for.
static int boundScaleAndRebuild(gvpm_context *h, float &rmax) {
  // grid cell = the largest per-pixel radius R * 0.01 * max(scaleVol) -- or anything above it.
  // Round 6: the step no longer waits for the one before it.  (1) The scale: a pixel's scale only shrinks (ratio <= 1 in the
  // SPPM update), so the largest scale of ANY earlier iteration bounds this one's: the host keeps such a bound -- the initial
  // scale at gvpm_reset, then whatever the iterations' last kernels have exported to pinned memory by now, one or two steps
  // stale -- and the cells are that much larger than they need to be.  (2) The photons' bounds and the grid on the BUILD stream,
  // into the other build set, while the gather of the step before still runs on the gather stream: the host waits for the
  // bounds of THIS upload only (a 10 us reduction that depends on nothing else), then for the near lists' overflow word behind
  // the build.  Until round 6 both waits stood behind the previous gather, the GPU idle for ~25 us of a 0.45 ms step, and the
  // build's nine small launches (~70 us) ran between two gathers instead of beside one.
  {
    const int rcp = ensurePinned(h);
    if (rcp != GVPM_OK) return rcp;
  }
  {
    const uint32_t bits = reinterpret_cast<volatile uint32_t *>(h->pinCtl)[32];
    float e;
    memcpy(&e, &bits, 4);
    if (bits != 0u && e > 0.f && e < h->vpmScaleBound) h->vpmScaleBound = e;
  }
  const float maxScale = h->vpmScaleBound;
  if (!(maxScale > 0.f)) return fail(h, GVPM_ERR_STATE, "G-VPM gather: no scale bound (gvpm_reset sets it)");
  rmax = (h->cfg.bsphere_radius * 0.01f) * maxScale;
  const bool pipe = h->pipeline && h->vpmPipeline && h->streamB;
  const BuildStreamGuard onBuildStream(h, pipe ? h->streamB : h->stream);
  if (h->photonsDirty || rmax != h->bs->builtRadius) {
    if (pipe) {
      // the other set; wait (on the build stream) until the gather that last read it is done
      h->setIdx = (h->setIdx + 1) % 2;
      h->bs = &h->sets[h->setIdx];
      if (h->bs->lastUseValid) HIP_TRY(h, hipStreamWaitEvent(h->bstream, h->bs->lastUse, 0));
    }
    const bool wantBounds = h->nph > 0;
    if (wantBounds) {
      HIP_TRY(h, h->bs->boundsPartial.ensure(1024 * 6));
      HIP_TRY(h, h->bs->bounds6.ensure(32));
      launch_bounds(h->rawDev.pos, h->nph, h->bs->boundsPartial.p, 1024, h->bs->bounds6.p, h->pinB6, h->bstream, nullptr, nullptr);
      HIP_TRY(h, hipStreamSynchronize(h->bstream));
    }
    GridBuild how;
    how.knownB6 = wantBounds ? h->pinB6 : nullptr;
    const int rc = buildGrid(h, rmax, how);
    if (rc != GVPM_OK) return rc;
    h->photonsDirty = false;
    h->bs->builtRadius = rmax;
    if (pipe) {
      HIP_TRY(h, hipEventRecord(h->bs->traversed, h->bstream));  // (this set's spare event: the build is done)
      HIP_TRY(h, hipStreamWaitEvent(h->stream, h->bs->traversed, 0));
    }
  }
  return GVPM_OK;
}

// The evaluation as three kernels (gather_vpm.hip): the walk and the evaluation on the gather stream, the redo of the heavy
// batches beside the evaluation on streamA2 (pipelined; else on the gather stream too), joined back by an event.
static int evaluateSplit(gvpm_context *h, const GatherArgs &a, uint32_t nBatches) {
  VpmSplit sp;
  // the pool: four chunks a batch (four pairs a sample) unless GVPM_VPM_POOL says otherwise; a step that needs more sends the
  // batches that find it exhausted through the fused code
  const uint32_t shardChunks = std::max<uint32_t>(4u, (uint32_t)(((uint64_t)h->vpmPoolPerBatch * nBatches + VPM_SHARDS - 1) / VPM_SHARDS));
  HIP_TRY(h, h->vpmPairs.ensure((size_t)shardChunks * VPM_SHARDS * 64));
  HIP_TRY(h, h->vpmChunkMeta.ensure((size_t)shardChunks * VPM_SHARDS));
  HIP_TRY(h, h->vpmStatus.ensure(nBatches));
  HIP_TRY(h, h->vpmState.ensure(h->nsamples));
  HIP_TRY(h, h->vpmRedo.ensure(nBatches));
  HIP_TRY(h, h->vpmCtl.ensure(VPM_CTL_REDO + 32));
  HIP_TRY(h, hipMemsetAsync(h->vpmCtl.p, 0, (VPM_CTL_REDO + 32) * sizeof(uint32_t), h->stream));
  sp.pairs = h->vpmPairs.p;
  sp.chunkMeta = h->vpmChunkMeta.p;
  sp.ctl = h->vpmCtl.p;
  sp.status = h->vpmStatus.p;
  sp.redo = h->vpmRedo.p;
  sp.state = h->vpmState.p;
  sp.shardChunks = shardChunks;
  sp.nBatches = nBatches;
  if (!h->vpmFound) {
    HIP_TRY(h, hipEventCreateWithFlags(&h->vpmFound, hipEventDisableTiming));
    HIP_TRY(h, hipEventCreateWithFlags(&h->vpmRedone, hipEventDisableTiming));
  }
  sp.zeroWord = h->maxScaleBits.p;  // (read through the host at the top; the iteration's last kernel reduces the new maximum into it)
  launch_vpm_find(a, sp, h->stream);
  const bool side = h->pipeline && h->streamA2;
  hipStream_t rs = side ? h->streamA2 : h->stream;
  if (side) {
    HIP_TRY(h, hipEventRecord(h->vpmFound, h->stream));
    HIP_TRY(h, hipStreamWaitEvent(rs, h->vpmFound, 0));
  }
  launch_vpm_redo(a, sp, needFullVis(h), h->vpmRedoWaves, rs);
  launch_vpm_eval(a, sp, needFullVis(h), std::max(1u, h->vpmEvalWaves / VPM_SHARDS), h->stream);
  if (side) {
    HIP_TRY(h, hipEventRecord(h->vpmRedone, rs));
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->vpmRedone, 0));
  }
  return GVPM_OK;
}

// computeVolumeGradientPhoton (G-VPM), gvpm.cpp:1081-1203
int gatherVPM(gvpm_context *h, int it, uint64_t nb_paths, bool primal) {
  (void)it;
  if (!h->haveSamples) return fail(h, GVPM_ERR_STATE, "G-VPM gather needs gvpm_upload_vpm_samples");
  if (h->cfg.nb_camera_samples <= 0) return fail(h, GVPM_ERR_INVALID_ARG, "nb_camera_samples must be positive");
  float rmax = 0.f;
  int rc = boundScaleAndRebuild(h, rmax);
  if (rc != GVPM_OK) return rc;
  // (the previous G-VPM gather zeroed `iter` and `mvol` as it folded them, and zeroes the largest-scale word before its update:
  // accumulate_kernel / vpm_update_kernel; anything else in between -- another technique, a failed gather -- and they are cleared here)
  if (!h->iterClean) {
    HIP_TRY(h, hipMemsetAsync(h->iter.p, 0, h->npix * 27 * sizeof(float), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->mvol.p, 0, h->npix * sizeof(float), h->stream));
  }
  h->iterClean = false;
  {
    const int rcx = exactPrepare(h);
    if (rcx != GVPM_OK) return rcx;
  }
  GatherArgs a;
  fillArgs(h, a, rmax);
  EventPair *ev;
  rc = nextEvents(h, &ev);
  if (rc != GVPM_OK) return rc;
  if (!primal && h->reqCap > 0 && h->cfg.use_manifold && h->bs->origIdx.p) {
    // manifold-typed shifts are recorded for the host (gvpm_download_shift_requests) instead of failing; the answered
    // terms are added straight to the accumulators (plain sums: this iteration's buffer is folded right below)
    rc = armHostShiftRequests(h, a, 4, true, h->accum.p, 1.f, false, h->stream);
    if (rc != GVPM_OK) return rc;
  }
  // Heaviest batches first.  A wave's time follows its candidate count (correlation 0.99, scripts/vpm_timing.py) and the
  // counts are heavy-tailed (C1: median 159, maximum 6 500 -- the pixels that look at the light): in sample order the last
  // heavy wave started when the others were done, and the kernel ran 160 of its 560 us on a handful of waves.  The batches
  // hold the same pixels every iteration, so the last launch's counts order this one.
  const uint32_t nBatches = (h->nsamples + 63u) / 64u;
  if (h->blockValB.cap < (size_t)nBatches + 1) h->vpmOrderN = 0;  // (a regrown buffer has lost the order)
  for (DevBuf<uint32_t> *b : {&h->blockKeyA, &h->blockKeyB, &h->blockValA, &h->blockValB}) HIP_TRY(h, b->ensure(nBatches + 1));
  a.vpmCostKey = h->blockKeyA.p;
  a.vpmCostVal = h->blockValA.p;
  // (a launch of another size: the permutation's slots, then the batches it does not know, in order; see the kernel)
  const bool haveOrder = h->vpmOrderN != 0 && !h->vpmNoOrder && h->vpmOrderN <= 2u * nBatches && nBatches <= 2u * h->vpmOrderN;
  a.vpmOrder = haveOrder ? h->blockValB.p : nullptr;
  a.vpmOrderN = haveOrder ? h->vpmOrderN : 0u;
  HIP_TRY(h, hipEventRecord(ev->first, h->stream));
  if (h->vpmSplit && !primal) {
    rc = evaluateSplit(h, a, nBatches);
    if (rc != GVPM_OK) return rc;
  } else {
    HIP_TRY(h, hipMemsetAsync(h->maxScaleBits.p, 0, 4, h->stream));
    launch_gather_vpm(a, needFullVis(h), primal, h->stream);
  }
  HIP_TRY(h, hipEventRecord(ev->second, h->stream));
  // the shifts the kernel could not decide in fp32: into the handle's list (before the radii of this iteration are updated),
  // where they wait for the exact pass -- which adds to the plain sums whenever it runs
  if (!primal) {
    launch_capture_notes(a, h->stream, 32);  // (a hundred notes an iteration at C1: 256 workgroups spent 8 us on their own hand-off)
    rc = exactAfterGather(h);
    if (rc != GVPM_OK) return rc;
  }
  // (re-sorted every fourth launch: the heavy pixels stay where they are while the radii shrink)
  if (!h->vpmNoOrder && nBatches > 1024u && (!haveOrder || (h->vpmLaunches & 3u) == 0u)) {
    HIP_TRY(h, sortPairsU32(h->bs->sortTmp, h->blockKeyA.p, h->blockKeyB.p, h->blockValA.p, h->blockValB.p, nBatches, 20, h->stream));
    h->vpmOrderN = nBatches;
  }
  h->vpmLaunches++;
  HIP_TRY(h, hipEventRecord(h->bs->lastUse, h->stream));  // (the kernels above are the last readers of this build set)
  h->bs->lastUseValid = true;
  launch_vpm_finish(h->accum.p, h->iter.p, h->scaleVol.p, h->nVol.p, h->mvol.p, h->npix, h->cfg.alpha, h->maxScaleBits.p, h->stream);
  // the new largest scale to pinned memory: a later gather's bound (above)
  launch_export_u32(h->maxScaleBits.p, nullptr, nullptr, nullptr, nullptr, h->pinCtl + 32, h->stream);
  HIP_TRY(h, hipGetLastError());
  h->iterClean = true;
  h->totalEmitted += (double)nb_paths;  // m_totalEmittedVolume, gvpm.cpp:434
  return GVPM_OK;
}
