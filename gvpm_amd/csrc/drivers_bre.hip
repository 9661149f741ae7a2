// The G-BRE step: computeVolumeGradientPhotonBRE, gvpm.cpp:988-1079.  Host code only.
// Pipeline: the build of this step (grid, beam sort, planner) runs on the build stream into a build set the previous
// steps are NOT reading, so it overlaps their traversal and evaluation; the host waits once (planner counters) and --
// unless an optimistic step had them queued behind the build already -- then queues traversal + evaluation.
#include "drivers.h"

namespace {

// One step's state, handed from stage to stage (gatherBRE at the bottom is the sequence).
struct BreStep {
  gvpm_context *h;
  int it;
  uint64_t nbPaths;
  bool primal;
  float r;                      // this step's kernel radius
  EventPair *evBuild = nullptr, *evTrav = nullptr, *evEval = nullptr;
  GatherArgs a;
  uint32_t itemCap = 0;         // the planner's bound on its work items
  uint32_t blocks = 0, nItems = 0;  // what the planner found: pair blocks, work items (after the host's wait)
  ChainPrep cp;
  int attempt = 0;              // 1: the step again on the 3D grid, after a ray outside the bundle the cells were keyed for
  bool force3D = false;
  bool rebuilt = false;         // this attempt built a set (else: re-planned the current one in place)
  bool chainRan = false;        // ... through the build chain
  bool queued = false;          // traversal + evaluation of this step are in their streams already (optimistic step)
  bool prevOverflow = false;    // h->nearOverflow of the last build: what an optimistic step picks its evaluation kernel by
  std::chrono::steady_clock::time_point T0;

  // GVPM_TRACE_HOST: host time since the last lap
  void lap(const char *what) {
    if (!(h->trace & TRACE_HOST)) return;
    auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[host] it=%d %-10s %8.1f us\n", it, what, std::chrono::duration<double, std::micro>(t - T0).count());
    T0 = t;
  }
  bool threeStage() const { return h->pipeline && h->travStream; }
};

// Gather stream.  The evaluation adds this iteration's estimate (1 / nb_paths per partial sum) straight into the running
// sum; an iteration that is not the successor of the last one rescales the sum first.
int foldRunningSum(gvpm_context *h, int it) {
  h->sumMode = true;
  if (h->sumIt != 0 && it - 1 != h->sumIt) {
    // the reference's fold (mean * (it - 1) + v) / it then weighs the old mean by (it - 1) / it, i.e. the sum by (it - 1) / last
    const int rc = gvpm_join_exact(h);
    if (rc != GVPM_OK) return rc;
    launch_scale(h->accum.p, h->accum.p, h->npix * 27, (float)((double)(it - 1) / (double)h->sumIt), h->stream);
  }
  h->sumIt = it;
  return GVPM_OK;
}

// Build stream (h->bstream).  New photons, beams or radius: rotate to the next build set, wait for its last readers, size
// (or, without the chain, launch) the grid and the beam sort.  Otherwise the current set is re-planned in place.
int buildOrWait(BreStep &s) {
  gvpm_context *h = s.h;
  s.rebuilt = false;
  s.cp = ChainPrep{};
  if (h->photonsDirty || h->beamsDirty || s.r != h->bs->builtRadius) {
    // the other set; wait until the kernels that last read it are done
    h->setIdx = (h->setIdx + 1) % (s.threeStage() ? 3 : 2);
    h->bs = &h->sets[h->setIdx];
    if (h->bs->used) HIP_TRY(h, hipStreamWaitEvent(h->bstream, h->bs->lastUse, 0));
    HIP_TRY(h, hipEventRecord(s.evBuild->first, h->bstream));
    s.lap("waitevent");
    {
      // the beam sort's key space rides behind the cells in the chain's counter array: known before the grid is sized
      int tileShift;
      uint32_t ntilesAll;
      beamTiling(h, h->beamsPerWave, s.cp.tw, s.cp.th, ntilesAll, tileShift);
      tileShift -= 3;  // (the chain's keys carry no edge bits: the sets of one pixel keep no order among themselves)
      const uint64_t nkeys = (uint64_t)ntilesAll << tileShift;
      s.cp.on = h->buildChain && h->nph > 0 && h->nsets > 0 && nkeys <= 0x3FFFFFF0ull;
      s.cp.nkeys = (uint32_t)nkeys;
      s.cp.tileShift = (uint32_t)tileShift;
    }
    GridBuild how;
    how.deferred = true;
    how.force3D = s.force3D;
    how.chain = &s.cp;
    int rc = buildGrid(h, s.r, how);
    s.lap("buildGrid");
    if (rc == GVPM_OK) rc = sortBeams(h, 0, &s.cp);
    s.lap("sortBeams");
    if (rc != GVPM_OK) return rc;
    h->photonsDirty = false;
    h->beamsDirty = false;
    h->bs->builtRadius = s.r;
    s.rebuilt = h->nph > 0;
  } else {
    // same inputs, same radius: the set is re-planned and re-traversed in place, once the evaluation kernel that still
    // reads its items and pair lists is done (the traversal stream waits too)
    if (h->bs->used) HIP_TRY(h, hipStreamWaitEvent(h->bstream, h->bs->lastUse, 0));
    if (h->bs->used && s.threeStage()) HIP_TRY(h, hipStreamWaitEvent(h->streamC, h->bs->lastUse, 0));
    HIP_TRY(h, hipEventRecord(s.evBuild->first, h->bstream));
  }
  return GVPM_OK;
}

// No launches: the kernel arguments of the built set, the item list and the planner's slab boxes at their bounds.
int sizeItemsAndBoxes(BreStep &s) {
  gvpm_context *h = s.h;
  GatherArgs &a = s.a;
  fillArgs(h, a, s.r);
  a.iter = h->accum.p;
  a.iterScale = 1.0f / (float)s.nbPaths;
  // slab thickness along y / z: 8 layers with the 1.5-radius cells of maps up to 2 M photons (round 3, with the traversal's
  // cylinder filter: -4 % on the C2 step, three alternating runs on one box), 6 with the one-radius cells above (a rank's
  // share of C4: 2.9 ms against 3.1)
  if (!a.cfg.reserved[1] && h->cellScale <= 0.f && h->nph <= 2000000u) a.cfg.reserved[1] = 8;
  s.itemCap = plan_items_capacity(h->nsets, h->bs->ntiles, h->beamsPerWave);
  HIP_TRY(h, h->bs->items.ensure(s.itemCap));
  HIP_TRY(h, h->bs->itemOff.ensure(s.itemCap));
  if (h->planBoxHandOff) {
    // one box per slab step and tile chunk: steps <= dim / (thinnest slab) + 1, chunks < nsets / B + ntiles + 1 (< 2^24)
    const Grid &g = h->bs->grid;
    const int kmin = std::max(1, std::min(a.cfg.reserved[2] ? a.cfg.reserved[2] : 8, a.cfg.reserved[1] ? a.cfg.reserved[1] : 6));
    // (sized for the finest grid the cell rule allows, as the cell arrays: a regrowth is a device-wide sync)
    const uint32_t stride = (uint32_t)(std::max(386, std::max(g.dim[0], std::max(g.dim[1], g.dim[2]))) / kmin + 2);
    const size_t chunks = (size_t)h->nsets / (size_t)h->beamsPerWave + h->bs->ntiles + 2;
    if (chunks < (1u << 24) && std::max(g.dim[0], std::max(g.dim[1], g.dim[2])) < 1024) {
      HIP_TRY(h, h->bs->planBoxes.ensure(chunks * stride));
      a.planBoxes = h->bs->planBoxes.p;
      a.planBoxStride = stride;
    }
  }
  HIP_TRY(h, h->bs->queueCtl.ensure(8));
  a.bundleFlag = h->bs->queueCtl.p + 4;
  // the planner's bound on (photon, beam) pairs sizes the pair buffer (grow only), read back in the step's one host sync,
  // with the photon bounds and the near-list overflow count
  return ensurePinned(h);
}

// Traversal + evaluation of the built set, for `blocks` pair blocks and `nItems` work items.  The traversal goes to the
// traversal stream (three-stage pipeline: the build of the NEXT step, which starts on the build stream as soon as this call
// returns, overlaps it), to the build stream (two stages) or to the gather stream (GVPM_PIPELINE=0); the evaluation and the
// note capture to the gather stream, behind the traversal by an event.  optimistic: queued before the host has seen the
// planner's counters -- nothing may be regrown (a regrowth is a device-wide sync), the traversal's grid is a guess (its waves
// take what lies beyond it from the queue), and the kernels wait for the build by an event.
int queueGather(BreStep &s, uint32_t blocks, uint32_t nItems, bool optimistic, bool fullVis) {
  gvpm_context *h = s.h;
  GatherArgs &a = s.a;
  const bool primal = s.primal;
  if (!optimistic) {
    HIP_TRY(h, h->bs->pairs.ensure((size_t)blocks * 64u + 64u));
    HIP_TRY(h, h->bs->pairCnt.ensure((size_t)s.itemCap * h->beamsPerWave));
  }
  int rc = nextEvents(h, &s.evTrav, 1);
  if (rc == GVPM_OK) rc = nextEvents(h, &s.evEval, 0);
  if (rc != GVPM_OK) return rc;
  const hipStream_t ts = !h->pipeline ? h->stream : (h->travStream ? h->streamC : h->streamB), es = h->stream;
  // the evaluation's work units (gather_bre_common.h, EVAL_UNIT): an item yields at most staged x beams pairs, i.e. at most
  // blocks_i * 64 / unit + 1 parts; their counters are queueCtl[5..6] (zeroed with the queue heads)
  uint2 *units = nullptr;
  uint32_t unitCap = 0;
  if (h->evalUnits && h->persistentEval && !primal) {
    if (optimistic) {
      unitCap = (uint32_t)std::min<size_t>(h->bs->units.cap / 2u, 0x3FFFFFFFu);
      units = unitCap ? h->bs->units.p : nullptr;
    } else {
      const uint64_t capU = (uint64_t)blocks * 64u / eval_unit_pairs() + nItems + 64u;
      if (capU < 0x3FFFFFFFull) {
        HIP_TRY(h, h->bs->units.ensure((size_t)capU * 2u));
        unitCap = (uint32_t)std::min<size_t>(h->bs->units.cap / 2u, 0x3FFFFFFFu);
        units = h->bs->units.p;
      }
    }
  }
  if (!primal) {
    // this set's own note list (exact_shift.hip)
    if (!h->bs->notes.p) {
      HIP_TRY(h, h->bs->notes.reserveExact(h->exOvfCap));
      HIP_TRY(h, h->bs->notesCount.ensure(4));
      HIP_TRY(h, hipMemsetAsync(h->bs->notesCount.p, 0, 4 * sizeof(uint32_t), es));
    }
    a.exOvf = h->bs->notes.p;
    a.exOvfCount = h->bs->notesCount.p;
    a.exOvfCap = h->exOvfCap;
  }
  if (optimistic && ts != h->bstream) HIP_TRY(h, hipStreamWaitEvent(ts, s.evBuild->second, 0));
  HIP_TRY(h, hipEventRecord(s.evTrav->first, ts));
  launch_traverse_bre(a, h->beamsPerWave, h->bs->items.p, h->bs->itemOff.p, h->bs->queueCtl.p, h->bs->queueCtl.p + 1,
                      h->bs->pairs.p, h->bs->pairCnt.p, h->persistentTrav ? h->nwavesTrav : nItems, h->persistentTrav || optimistic, ts,
                      units, h->bs->queueCtl.p + 5, unitCap);
  HIP_TRY(h, hipEventRecord(s.evTrav->second, ts));
  HIP_TRY(h, hipEventRecord(h->bs->traversed, ts));
  HIP_TRY(h, hipStreamWaitEvent(es, h->bs->traversed, 0));
  // maps beyond 2 M photons: the evaluation is the stage the pipelined step waits for (its records no longer fit the
  // Infinity Cache), so it gets its third wave per SIMD; below, the other stages need the room more (measured: +6 % on a
  // rank's step at C4 with 12 waves per CU, -3 % at C2)
  // (... when the evaluation is the long stage: a rank that holds an eighth of the frame evaluates for 1.3 ms beside a build of
  // 1.0 -- with 12 waves per CU the build starves.  C4, rank 0 of N emulated, 8 / 12 waves: N = 2: 7.14 / 6.91 ms per step,
  // N = 4: 3.94 / 3.93, N = 8: 2.33 / 2.47)
  const bool smallShare = h->nsets > 0 && (size_t)h->nsets * 6u <= h->npix;
  const uint32_t nwEval = (h->pipeline && !h->nwavesFromEnv && h->ncu && h->nph > 2000000u && !smallShare)
                              ? std::min<uint32_t>(h->ncu * 12u, GVPM_STAT_ROWS) : h->nwaves;
  if (!primal && h->reqCap > 0 && h->cfg.use_manifold && h->bs->origIdx.p) {
    rc = armHostShiftRequests(h, a, 4, true, a.iter, a.iterScale, false, es);
    if (rc != GVPM_OK) return rc;
  }
  HIP_TRY(h, hipEventRecord(s.evEval->first, es));
  if (primal)
    // the primal beam radiance estimate over the same items and pair lists (gather_bre.hip, evaluate_primal_kernel)
    launch_evaluate_primal(a, h->beamsPerWave, h->bs->items.p, h->bs->itemOff.p, h->bs->queueCtl.p, h->bs->queueCtl.p + 2,
                           h->bs->pairs.p, h->bs->pairCnt.p, std::max<uint32_t>(1u, std::min<uint32_t>(nItems, h->ncu * 16u)), es);
  else
    launch_evaluate_bre(a, h->beamsPerWave, fullVis, h->bs->items.p, h->bs->itemOff.p, h->bs->queueCtl.p,
                        h->bs->queueCtl.p + 2, h->bs->pairs.p, h->bs->pairCnt.p, h->persistentEval ? nwEval : nItems, h->persistentEval,
                        es, units, h->bs->queueCtl.p + 5, unitCap);
  HIP_TRY(h, hipEventRecord(s.evEval->second, es));
  // the shifts and pairs the evaluation could not decide in fp32: their records and rays into the handle's list, where they
  // wait for the exact pass
  if (!primal) launch_capture_notes(a, es);
  HIP_TRY(h, hipEventRecord(h->bs->lastUse, es));
  h->bs->lastUseValid = true;
  if (!primal) return exactAfterGather(h);  // (a pass it starts waits for this evaluation too: after the event above)
  return GVPM_OK;
}

// Build stream.  A rebuilt set with the chain on: the whole build -- cells, beam sort, summed-volume table, planner beside
// the photon scatter -- in six launches, and, for an optimistic step, traversal + evaluation behind it (queueGather's
// streams).  Otherwise the planner and the export of its counters as two launches.  Either way the counters land in pinCtl.
int launchBuildAndPlan(BreStep &s) {
  gvpm_context *h = s.h;
  const ChainPrep &cp = s.cp;
  if (cp.on && s.rebuilt) {
    if (!h->chainCtl.p) {
      HIP_TRY(h, h->chainCtl.ensure(192));
      HIP_TRY(h, hipMemsetAsync(h->chainCtl.p, 0, h->chainCtl.cap * sizeof(uint32_t), h->bstream));
    }
    ChainArgs c{};
    c.pos = h->rawDev.pos;
    c.n = h->nph;
    c.g = h->bs->grid;
    c.keys = h->bs->keysA.p;
    c.rank = h->bs->valsA.p;
    c.counts = h->bs->cellCount.p;
    c.starts = h->bs->cellStart.p;
    c.beamOff = h->bs->grid.ncells + 1u;
    c.scanLen = c.beamOff + cp.nkeys + 1u;
    c.sub = cp.sub;
    HIP_TRY(h, h->bs->chainBuckets.ensure(768));
    c.buckets = h->bs->chainBuckets.p;
    c.out6 = h->bs->bounds6.p;
    c.hostB6 = h->pinB6;
    c.rays = h->raysDev;
    c.nsets = h->nsets;
    c.width = h->cfg.width;
    c.tw = cp.tw;
    c.th = cp.th;
    c.tileShift = cp.tileShift;
    c.ntiles = h->bs->ntiles;
    c.bKeys = h->bs->bKeysA.p;
    c.bRank = h->bs->bValsA.p;
    c.setPerm = h->bs->setPerm.p;
    c.tileStart = h->bs->tileStart.p;
    c.blockSum = reinterpret_cast<uint32_t *>(h->bs->sortTmp.d);
    c.ctl = h->chainCtl.p;
    c.queueCtl = h->bs->queueCtl.p;
    c.overflowCtr = h->bs->overflowCtr.p;
    c.nearExt = h->bs->nearExt.p;
    c.sat = h->bs->sat.p;
    h->boundsPending = h->haveCachedBounds;  // (the chain's bounds land in pinB6 with the counters)
    // An OPTIMISTIC step: the pair buffer and the unit lists as the last steps left them (the radius shrinks: what held the
    // last step holds this one), the traversal's grid from the last item count, the evaluation kernel by the last build's
    // near lists.  The build's last block checks all of it against what the planner found.
    const bool optimistic = h->optimistic && h->pipeline && s.attempt == 0 && !s.primal && h->persistentEval && h->lastItems > 0 &&
                            h->bs->pairs.cap >= 128u && h->bs->pairCnt.cap >= (size_t)s.itemCap * h->beamsPerWave &&
                            (!h->evalUnits || h->bs->units.cap >= 2u);
    const bool fullVisOpt = !h->cfg.visibility_as_written || s.prevOverflow;
    // (tests: GVPM_OPTIMISTIC_REFUSE=n makes the guard refuse every n-th optimistic step -- a pair buffer of zero blocks)
    const bool refuse = optimistic && h->optRefuseEvery > 0 && (++h->optSteps % h->optRefuseEvery) == 0;
    launch_build_chain(c, s.a, h->rawDev, h->beamsPerWave, h->planTarget, h->bs->items.p, h->bs->itemOff.p, s.itemCap, cp.dmax, h->nearGrid,
                       (uint32_t)std::min<size_t>(h->bs->nearExt.cap, 0xFFFFFF00u), cp.wantOrig ? h->bs->origIdx.p : nullptr, h->pinCtl,
                       !h->bs->bucketsInit, h->bstream,
                       optimistic ? (refuse ? 0u : (uint32_t)std::min<size_t>((h->bs->pairs.cap - 64u) / 64u, 0xFFFFFFF0u)) : 0xFFFFFFFFu,
                       optimistic && h->evalUnits ? (uint32_t)std::min<size_t>(h->bs->units.cap / 2u, 0x3FFFFFFFu) : 0u, eval_unit_pairs(),
                       fullVisOpt, h->planGroups, h->nearScalar);
    h->bs->bucketsInit = true;
    s.chainRan = true;
    if (optimistic) {
      HIP_TRY(h, hipEventRecord(s.evBuild->second, h->bstream));
      const uint32_t guess = std::min<uint32_t>(s.itemCap, h->lastItems + h->lastItems / 8u + 256u);
      const int rc = queueGather(s, 0u, guess, true, fullVisOpt);
      if (rc != GVPM_OK) return rc;
      s.queued = true;
    }
  } else {
    HIP_TRY(h, hipMemsetAsync(h->bs->queueCtl.p, 0, 8 * sizeof(uint32_t), h->bstream));
    launch_plan_bre(s.a, h->beamsPerWave, h->bs->ntiles, h->planTarget, h->bs->items.p, h->bs->queueCtl.p, h->bs->itemOff.p,
                    h->bs->queueCtl.p + 3, s.itemCap, h->bstream);
    launch_export_u32(h->bs->queueCtl.p + 3, s.rebuilt ? h->bs->overflowCtr.p : nullptr, s.rebuilt ? h->bs->nearExt.p : nullptr,
                      h->bs->queueCtl.p, h->bs->queueCtl.p + 4, h->pinCtl, h->bstream);
  }
  if (!s.queued) HIP_TRY(h, hipEventRecord(s.evBuild->second, h->bstream));
  s.lap("plan");
  return GVPM_OK;
}

// The step's one host wait, on the build stream; then the planner's counters.  An optimistic step the build's guard refused
// is un-queued here (waits on the gather and traversal streams, two memsets on the build stream).  retry: the planner met a
// ray outside the bundle the cells were keyed for -- the caller runs the build stages again, on the 3D grid.
int readCounters(BreStep &s, bool &retry) {
  gvpm_context *h = s.h;
  retry = false;
  HIP_TRY(h, hipStreamSynchronize(h->bstream));
  s.lap("syncB");
  s.blocks = h->pinCtl[0];
  s.nItems = h->pinCtl[3];
  if (s.queued && h->pinCtl[5] != 0u) {
    // the guess was wrong: both kernels have returned at once (or will); wait for them, then the caller queues them again, sized
    if (h->trace & TRACE_PLAN) fprintf(stderr, "[plan] optimistic step refused by the build (status %u): queued again\n", h->pinCtl[5]);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (s.threeStage()) HIP_TRY(h, hipStreamSynchronize(h->streamC));
    HIP_TRY(h, hipMemsetAsync(h->bs->queueCtl.p + 1, 0, 2 * sizeof(uint32_t), h->bstream));
    HIP_TRY(h, hipMemsetAsync(h->bs->queueCtl.p + 5, 0, 3 * sizeof(uint32_t), h->bstream));
    HIP_TRY(h, hipStreamSynchronize(h->bstream));
    s.queued = false;
    h->optRefused++;
  }
  if (s.a.grid.mode == 1 && h->pinCtl[4] != 0u && s.attempt == 0) {
    // not the bundle the cells were keyed for (another sensor, or later edges of the camera paths among the beams):
    // this step again on the 3D grid; the frame is fitted anew at the next build, a few times
    h->bundleState = ++h->bundleViolations > 3 ? -1 : 0;
    h->photonsDirty = true;
    h->boundsPending = false;
    s.force3D = true;
    retry = true;
  }
  return GVPM_OK;
}

// No launches (GVPM_TRACE_PLAN reads the queue words back): what the counters say about this build is kept for the next
// one -- grid kind, near-list overflow and wants, the photons' and the camera beams' bounds, the item count.
int recordBuild(BreStep &s) {
  gvpm_context *h = s.h;
  h->lastGridMode = s.a.grid.mode;
  h->lastGridCells = s.a.grid.ncells;
  if (s.nItems > s.itemCap) return fail(h, GVPM_ERR_STATE, "G-BRE planner produced more work items than its bound");
  if (h->trace & TRACE_PLAN) {
    uint32_t q[4] = {0, 0, 0, 0};
    (void)hipMemcpy(q, h->bs->queueCtl.p, sizeof(q), hipMemcpyDeviceToHost);
    fprintf(stderr, "[plan] items %u staged blocks %u tiles %u sets %u; photons %u, %s %d x %d x %d cells of %g (radius %g)\n", q[0],
            s.blocks, h->bs->ntiles, h->nsets, h->nph, h->bs->grid.mode == 1 ? "bundle cells" : "grid", h->bs->grid.dim[0],
            h->bs->grid.dim[1], h->bs->grid.dim[2], (double)h->bs->grid.cell, (double)s.r);
  }
  if (s.rebuilt) {
    h->nearOverflow = h->cfg.visibility_as_written && h->pinCtl[1] != 0;
    // what the extension lists asked for (the cursor keeps counting past the capacity): sizes the next build's
    h->nearExtWant = std::max<size_t>(h->nearExtWant, (size_t)h->pinCtl[2] + h->pinCtl[2] / 4);
    if (h->trace & TRACE_VIS)
      fprintf(stderr, "[vis] ntri %u photons %u: %u lists overflowed, extension cursor %u of %zu, fullvis %d\n", h->ntri, h->nph,
              h->pinCtl[1], h->pinCtl[2], h->bs->nearExt.cap, (int)needFullVis(h));
  }
  if (h->boundsPending) {
    h->boundsPending = false;
    for (int c = 0; c < 6; ++c)
      if (!std::isfinite(h->pinB6[c])) return fail(h, GVPM_ERR_INVALID_ARG, "non-finite photon position");
    memcpy(h->cachedB6, h->pinB6, sizeof(h->cachedB6));
  }
  if (s.rebuilt && s.chainRan) {
    // the camera beams' bounds of this step clip the next step's grid
    bool ok = true;
    for (int c = 0; c < 6; ++c) ok = ok && std::isfinite(h->pinB6[16 + c]);
    h->haveBeamBounds = ok;
    if (ok) memcpy(h->beamB6, h->pinB6 + 16, sizeof(h->beamB6));
  }
  h->lastItems = s.nItems;
  return GVPM_OK;
}

// No launches: the first step of a run gives the build sets that have not run yet the capacities of the one that has, so
// that the second step does not stop for gigabytes of hipMalloc in the middle of the pipeline.
int mirrorSets(gvpm_context *h) {
  if (h->pipeline) {
    for (int k = 0; k < (h->travStream ? 3 : 2); ++k) {
      BuildSet &other = h->sets[k];
      if (&other != h->bs && !other.used && !h->bs->used) HIP_TRY(h, other.mirrorFrom(*h->bs));
    }
  }
  h->bs->used = true;
  return GVPM_OK;
}

// everything that goes to the build stream, up to the host's one wait and what it read
int buildAndPlan(BreStep &s) {
  gvpm_context *h = s.h;
  const BuildStreamGuard onBuildStream(h, h->pipeline ? h->streamB : h->stream);
  int rc = foldRunningSum(h, s.it);
  if (rc == GVPM_OK) rc = exactPrepare(h);
  // (a second pass only when the planner met a ray outside the bundle the grid was keyed for: rebuilt in 3D)
  for (s.attempt = 0; rc == GVPM_OK && s.attempt < 2; ++s.attempt) {
    bool retry = false;
    rc = buildOrWait(s);
    if (rc == GVPM_OK) rc = sizeItemsAndBoxes(s);
    if (rc == GVPM_OK) rc = launchBuildAndPlan(s);
    if (rc == GVPM_OK) rc = readCounters(s, retry);
    if (!retry) break;
  }
  if (rc == GVPM_OK) rc = recordBuild(s);
  return rc;
}

}  // namespace

int gatherBRE(gvpm_context *h, int it, uint64_t nb_paths, bool primal) {
  BreStep s{h, it, nb_paths, primal, currentRadius(h)};
  s.prevOverflow = h->nearOverflow;
  s.T0 = std::chrono::steady_clock::now();
  int rc = nextEvents(h, &s.evBuild, 2);
  if (rc == GVPM_OK) rc = buildAndPlan(s);
  if (rc == GVPM_OK && !s.queued) rc = queueGather(s, s.blocks, s.nItems, false, needFullVis(h));
  if (rc == GVPM_OK) rc = mirrorSets(h);
  if (rc != GVPM_OK) return rc;
  HIP_TRY(h, hipGetLastError());
  s.lap("launchK");
  scaleVolumeAPA(h, it);
  return GVPM_OK;
}
