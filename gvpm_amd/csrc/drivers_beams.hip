// The G-Beams step: computeVolumeGradientBeams, gvpm.cpp:880-986, and its sub-beam grid.  Host code only; one stream.
#include "drivers.h"

// sub-beam grid for photon beams of kernel radius r
static int buildBeamGrid(gvpm_context *h, float r) {
  const uint32_t n = h->nph;
  h->nsub = 0;
  h->maxSubLen = 0.f;
  HIP_TRY(h, h->bs->cold.ensure((size_t)(n + 1) * GVPM_REC_QUADS));
  if (n == 0) {
    h->bs->grid = Grid{{0, 0, 0}, 1.f, 1.f, {1, 1, 1}, 1};
    HIP_TRY(h, h->bs->cellStart.ensure(2));
    HIP_TRY(h, hipMemsetAsync(h->bs->cellStart.p, 0, 2 * sizeof(uint32_t), h->stream));
    h->subLen = r;
    return GVPM_OK;
  }
  // bounds of the beam end points and origins
  const int nblocks = 1024;  // (four workgroups per CU: 256 left this bandwidth-bound pass latency-bound, 58 us for 24 MB)
  HIP_TRY(h, h->bs->boundsPartial.ensure(nblocks * 6));
  HIP_TRY(h, h->bs->bounds6.ensure(32));
  // (what the host reads back in this build -- bounds, sub-beam count -- and after the traversal is written by the kernels
  // into pinned memory, as in the G-BRE build: a D2H copy is a runtime kernel of its own with ~20 us of latency around it)
  if (!h->pinBeams) HIP_TRY(h, hipHostMalloc((void **)&h->pinBeams, 256, hipHostMallocMapped));
  uint32_t *pinU = reinterpret_cast<uint32_t *>(h->pinBeams + 16);
  launch_bounds(h->rawDev.pos, n, h->bs->boundsPartial.p, nblocks, h->bs->bounds6.p, h->pinBeams, h->stream);
  launch_bounds(h->rawDev.parent_pos, n, h->bs->boundsPartial.p, nblocks, h->bs->bounds6.p + 6, h->pinBeams + 8, h->stream);
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  float b12[12];
  memcpy(b12, h->pinBeams, 6 * sizeof(float));
  memcpy(b12 + 6, h->pinBeams + 8, 6 * sizeof(float));
  float b6[6], ext = 0.f;
  for (int c = 0; c < 3; ++c) {
    b6[c] = fminf(b12[c], b12[6 + c]);
    b6[3 + c] = fmaxf(b12[3 + c], b12[9 + c]);
    if (!std::isfinite(b6[c]) || !std::isfinite(b6[3 + c])) return fail(h, GVPM_ERR_INVALID_ARG, "non-finite beam position");
    ext = fmaxf(ext, b6[3 + c] - b6[c]);
  }
  Grid g{};
  // sub-beams (and cells) of 3/4 of the kernel radius: the traversal cost follows the number of sphere tests, which
  // shrinks with the cell until the ext/256 floor (measured: 34 ms at 1.5 r, 23.5 ms at 0.75 r and below)
  // (round 3, measured at C3 with the round's evaluation: sub-beams and cells of 1.5 r -- 24 M sub-beams instead of 47 M,
  // build 6.4 -> 4.2 ms, traversal 10.2 -> 9.9 -- and, with them, work items of 4096 staged sub-beams: traversal -> 7.9 ms.
  // Round 2 had measured the opposite (23.5 ms at 0.75 r against 34 at 1.5 r) on a traversal that resolved its candidates
  // one per lane and round: the cost followed the sphere tests then, the walk and the staging now.)
  // (end of round 4, with the build's kernels cheaper per sub-beam and the traversal's parity partition: 2.25 r -- GVPM_CELL_SCALE
  // 2 / 2.5 / 3 / 3.5 / 4 at C3: 23.19 / 22.80 / 22.72 / 23.15 / 24.0 ms per step)
  float cell = fmaxf(0.75f * (h->cellScale > 0.f ? h->cellScale : 3.0f) * r, ext / 256.f);
  if (!(cell > 0.f)) cell = 1.f;
  g.cell = cell;
  g.invCell = 1.f / cell;
  uint64_t nc = 1;
  for (int c = 0; c < 3; ++c) {
    g.org[c] = b6[c] - 0.5f * cell;
    g.dim[c] = (int)floorf((b6[3 + c] - g.org[c]) * g.invCell) + 2;
    nc *= (uint64_t)g.dim[c];
  }
  if (nc > 0x7FFFFFFFull) return fail(h, GVPM_ERR_INVALID_ARG, "grid too large");
  g.ncells = (uint32_t)nc;
  h->bs->grid = g;
  h->subLen = cell;
  // cut the beams into sub-beams of about one cell
  HIP_TRY(h, h->subCounts.ensure(n + 1));
  HIP_TRY(h, h->subOffsets.ensure(n + 1));
  HIP_TRY(h, h->beamCtl.ensure(4));
  HIP_TRY(h, hipMemsetAsync(h->beamCtl.p, 0, 4 * sizeof(uint32_t), h->stream));
  launch_beam_subcount(h->rawDev.pos, h->rawDev.parent_pos, n, h->subLen, h->subCounts.p, h->beamCtl.p, h->stream);
  HIP_TRY(h, exclusiveSumU32(h->bs->sortTmp, h->subCounts.p, h->subOffsets.p, n, h->stream));
  launch_export_u32(h->subOffsets.p + (n - 1), h->subCounts.p + (n - 1), h->beamCtl.p, nullptr, nullptr, pinU, h->stream);
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const uint32_t lastOff = pinU[0], lastCnt = pinU[1], maxBits = pinU[2];
  const uint64_t S = (uint64_t)lastOff + lastCnt;
  if (S > 0x7FFFFFF0ull) return fail(h, GVPM_ERR_INVALID_ARG, "too many sub-beams");
  h->nsub = (uint32_t)S;
  memcpy(&h->maxSubLen, &maxBits, 4);
  HIP_TRY(h, h->bs->keysA.ensure(S));
  HIP_TRY(h, h->bs->keysB.ensure(S));
  HIP_TRY(h, h->bs->valsA.ensure(S));
  HIP_TRY(h, h->bs->valsB.ensure(S));
  HIP_TRY(h, h->bs->hot.ensure(2 * S));
  HIP_TRY(h, h->subFlags.ensure(S + 1));
  HIP_TRY(h, h->bs->cellStart.ensure((size_t)g.ncells + 2));
  launch_beam_expand(h->rawDev.pos, h->rawDev.parent_pos, n, h->subCounts.p, h->subOffsets.p, g, h->bs->keysA.p,
                     h->bs->valsA.p, h->stream);
  HIP_TRY(h, sortPairsU32(h->bs->sortTmp, h->bs->keysA.p, h->bs->keysB.p, h->bs->valsA.p, h->bs->valsB.p, h->nsub,
                          ilog2ceil(g.ncells + 1), h->stream));
  HIP_TRY(h, h->beamAux.ensure(2 * (size_t)n + 2));
  launch_beam_cold(h->rawDev, h->endNDev, n, h->cfg, h->subCounts.p, h->bs->cold.p, h->beamAux.p, h->stream);
  launch_sub_hot(h->bs->valsB.p, h->nsub, h->beamAux.p, h->bs->hot.p, h->subFlags.p, h->stream);
  launch_segment_start(h->bs->keysB.p, h->nsub, g.ncells, 0, h->bs->cellStart.p, h->stream);
  {
    const size_t satCells = (size_t)(g.dim[0] + 1) * (g.dim[1] + 1) * (g.dim[2] + 1);
    HIP_TRY(h, h->bs->sat.ensure(satCells));
    launch_sat(h->bs->cellStart.p, g, h->bs->sat.p, h->stream);
  }
  HIP_TRY(h, hipGetLastError());
  return GVPM_OK;
}

// What is stale of the build, for kernel radius r: the sub-beam grid and the beam records, the camera-beam sort, the beams'
// near-occluder lists.
static int refreshBuild(gvpm_context *h, float r) {
  if (h->photonsDirty || r != h->bs->builtRadius) {
    int rc = buildBeamGrid(h, r);
    if (rc != GVPM_OK) return rc;
    h->photonsDirty = false;
    h->bs->builtRadius = r;
    h->beamNearStale = true;  // new records (or a new radius): the near-occluder lists are rebuilt below
  }
  bool nearDirty = false;
  if (h->beamsDirty) {
    int rc = sortBeams(h);
    if (rc != GVPM_OK) return rc;
    h->beamsDirty = false;
    // how far a shifted camera ray strays from its base ray, over all uploaded sets (beam_near_kernel's delta)
    HIP_TRY(h, h->shiftExtent.ensure(1));
    launch_shift_extent(h->raysDev, h->nsets, h->shiftExtent.p, h->stream);
    nearDirty = true;
  }
  if (nearDirty || h->beamNearStale) {
    HIP_TRY(h, h->shiftExtent.ensure(1));
    HIP_TRY(h, h->beamClear.ensure((size_t)h->nph + 1));
    launch_beam_near(h->bs->cold.p, h->nph, h->tri4.p, h->ntri, r, h->cfg.epsilon, h->shiftExtent.p, h->beamClear.p, h->beamsFreeCone, h->stream);
    if (h->trace & TRACE_BEAMS) {
      DevBuf<uint32_t> hist;
      uint32_t hh[21] = {0}, ext = 0;
      if (hist.ensure(24) == hipSuccess && hipMemsetAsync(hist.p, 0, 96, h->stream) == hipSuccess) {
        launch_beam_near_hist(h->bs->cold.p, h->nph, h->ntri, hist.p, h->stream);
        (void)hipMemcpyAsync(hh, hist.p, sizeof(hh), hipMemcpyDeviceToHost, h->stream);
        (void)hipMemcpyAsync(&ext, h->shiftExtent.p, 4, hipMemcpyDeviceToHost, h->stream);
        (void)hipStreamSynchronize(h->stream);
        float extf;
        memcpy(&extf, &ext, 4);
        fprintf(stderr, "[beams] near lists (delta = 4 x %g + %g, %u occluders): lengths 0..19:", (double)r, (double)extf, h->ntri);
        for (int k = 0; k <= 19; ++k) fprintf(stderr, " %u", hh[k]);
        fprintf(stderr, "; overflowed %u\n", hh[20]);
      }
      hist.release();
    }
    h->beamNearStale = false;
  }
  return GVPM_OK;
}

// Plan, traverse into the pair list, wait for the counts -- again with longer lists while either has overflowed.  npairs:
// the pairs the traversal wrote (blocks of 64).  evTrav: the phase's event pair, around all passes.
static int planAndTraverse(gvpm_context *h, const GatherArgs &a, float r, EventPair *evTrav, uint32_t &npairs) {
  // The planner splits heavy items into as many as 512 parts (tile_walk.h), so its own bound (items per tile chunk) is
  // not a bound on the list: the list starts at that bound plus room for the parts and, when the planner reports more
  // (it counts what it could not write, and the traversal never reads past the capacity), is regrown to the count and
  // the plan repeated -- as the pair list below.
  uint32_t itemCap = h->beamItemsInit ? h->beamItemsInit
                                      : plan_items_capacity(h->nsets, h->bs->ntiles, h->beamsPerWave) + h->nsub / 256u + 4096u;
  itemCap = std::max(itemCap, h->beamItemCap);
  HIP_TRY(h, h->bs->queueCtl.ensure(8));
  // traversal -> pair list (blocks of 64) -> evaluation.  The list has no useful a-priori bound (the planner's is
  // sub-beams x rays per slab box, ~100x the survivors): it starts at 16 M pairs and, when the traversal reports
  // more than fit, is regrown to what it counted and the traversal repeated (deterministic, first iterations only).
  // queueCtl: [0] items, [1] item queue head, [2] pairs (multiple of 64), [3] block queue head
  if (h->beamPairs.cap == 0) HIP_TRY(h, h->beamPairs.ensure(h->beamPairsInit));
  npairs = 0;
  bool planned = false;
  HIP_TRY(h, hipEventRecord(evTrav->first, h->stream));
  for (int attempt = 0;; ++attempt) {
    if (!planned) {
      HIP_TRY(h, h->bs->items.ensure(itemCap));
      HIP_TRY(h, hipMemsetAsync(h->bs->queueCtl.p, 0, 8 * sizeof(uint32_t), h->stream));
      // (work items of 6144 staged sub-beams: 4096 / 6144 / 8192 / 12288 at C3 with cells of 2.25 r: 22.73 / 22.45 / 22.43 / 22.51 ms)
      launch_plan_bre(a, h->beamsPerWave, h->bs->ntiles, h->planTargetSet ? h->planTarget : 6144u, h->bs->items.p, h->bs->queueCtl.p, nullptr, nullptr,
                      itemCap, h->stream);
      planned = true;
    }
    const uint32_t cap = (uint32_t)std::min<size_t>(h->beamPairs.cap, 0xFFFFFFC0u);
    const size_t nblkCap = cap / 64u + 1u;
    for (DevBuf<uint32_t> *b : {&h->blockKeyA, &h->blockKeyB, &h->blockValA, &h->blockValB}) HIP_TRY(h, b->ensure(nblkCap));
    launch_traverse_beams(a, h->subFlags.p, h->beamsPerWave, h->bs->items.p, h->bs->queueCtl.p, itemCap, h->bs->queueCtl.p + 1,
                          h->beamPairs.p, h->bs->queueCtl.p + 2, cap, h->blockKeyA.p, h->blockValA.p, h->nwavesTrav, h->stream);
    if (!h->pinBeams) HIP_TRY(h, hipHostMalloc((void **)&h->pinBeams, 256, hipHostMallocMapped));
    uint32_t *pinU = reinterpret_cast<uint32_t *>(h->pinBeams + 16) + 8;
    launch_export_u32(h->bs->queueCtl.p, h->bs->queueCtl.p + 1, h->bs->queueCtl.p + 2, nullptr, nullptr, pinU, h->stream);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const uint32_t ctl[3] = {pinU[0], pinU[1], pinU[2]};
    npairs = ctl[2];
    if (h->trace & TRACE_BEAMS) {
      uint32_t q[4];
      (void)hipMemcpy(q, h->bs->queueCtl.p, sizeof(q), hipMemcpyDeviceToHost);
      fprintf(stderr, "[beams] items %u (cap %u) pairs %u (cap %u) nsub %u nsets %u tiles %u cell %.3f r %.3f dims %d %d %d\n", q[0],
              itemCap, npairs, cap, h->nsub, h->nsets, h->bs->ntiles, h->bs->grid.cell, r, h->bs->grid.dim[0], h->bs->grid.dim[1],
              h->bs->grid.dim[2]);
    }
    const bool itemsOver = ctl[0] > itemCap, pairsOver = npairs > cap;
    if (!itemsOver && !pairsOver) break;
    if (attempt >= 3) return fail(h, GVPM_ERR_HIP, "G-Beams item / pair lists overflowed after being regrown");
    if (itemsOver) {
      // (the pass over the truncated list is discarded whole)
      itemCap = ctl[0] + (ctl[0] >> 2) + 64u;
      h->beamItemCap = itemCap;
      planned = false;
    } else {
      HIP_TRY(h, h->beamPairs.ensure((size_t)npairs + (npairs >> 2) + 64));
      HIP_TRY(h, hipMemsetAsync(h->bs->queueCtl.p + 1, 0, 2 * sizeof(uint32_t), h->stream));
    }
    // the candidate count of the discarded pass
    HIP_TRY(h, hipMemset2DAsync(a.stats + 1, 8 * sizeof(unsigned long long), 0, sizeof(unsigned long long), GVPM_STAT_ROWS,
                                h->stream));
  }
  HIP_TRY(h, hipEventRecord(evTrav->second, h->stream));
  return GVPM_OK;
}

// The pair blocks sorted by tile, the evaluation over them (host-shift requests armed when enabled), and behind it the fp64
// pass over what it left undecided.  ev: the evaluation's event pair.
static int evaluatePairs(gvpm_context *h, GatherArgs &a, uint32_t npairs, int it, uint64_t nb_paths, bool primal, EventPair *ev) {
  HIP_TRY(h, hipEventRecord(ev->first, h->stream));
  // blocks of 64 pairs, sorted by tile: the evaluation loads a tile's rays once per run of its blocks
  const uint32_t nBlocks = npairs / 64u;
  if (nBlocks)
    HIP_TRY(h, sortPairsU32(h->bs->sortTmp, h->blockKeyA.p, h->blockKeyB.p, h->blockValA.p, h->blockValB.p, nBlocks,
                            ilog2ceil(h->nsets + 1), h->stream));
  if (!primal && !h->beamsExact) {
    // the notes of the shifts the fp32 evaluation cannot decide (exact_beams_kernel, behind it): ~1.2e-3 of the PAIRS at C3, and
    // a block holds 64 pairs -- room for four notes a block, i.e. 6 % of the pairs, fifty times that rate (a
    // quarter of the block count was three times the rate, not twenty), and never less than the handle's default; S-laser's plate
    // had 2.8 % undecided segments before triHitFine.  Beyond it gvpm_get_stats still fails loudly (the counter keeps counting).
    const size_t need = std::max<size_t>(h->exOvfCap, (size_t)nBlocks * 4u);
    if (need > 0xFFFFFF00ull) return fail(h, GVPM_ERR_INVALID_ARG, "too many pair blocks for the note list");
    HIP_TRY(h, h->exOvf.reserveExact(need));
    a.exOvf = h->exOvf.p;
    a.exOvfCap = (uint32_t)need;
  }
  if (!primal && !h->beamsExact && h->reqCap > 0 && h->cfg.use_manifold) {
    // manifold-typed shifts (shiftBeamME) are recorded for the host instead of failing; the answered terms go straight into
    // the running mean: this iteration's buffer is folded right below, with weight 1 / (nb_paths * it)
    const int rcq = armHostShiftRequests(h, a, 5, false, h->accum.p, (float)(1.0 / ((double)nb_paths * (double)it)), true, h->stream);
    if (rcq != GVPM_OK) return rcq;
  }
  if (h->beamsSplit && !primal && !h->beamsExact && !a.reqHost && h->beamsPerWave == 16 && nBlocks) {
    // (experiment: phase 1 and phase 2 as two kernels, the reconnection entries through HBM -- gather_beams.hip)
    const size_t nEnt = (size_t)nBlocks * 256u;
    if (nEnt > 0xFFFFFF00ull) return fail(h, GVPM_ERR_INVALID_ARG, "too many blocks for the split evaluation");
    HIP_TRY(h, h->splitId.ensure(nEnt));
    HIP_TRY(h, h->splitMeta.ensure(nEnt));
    HIP_TRY(h, h->splitK.ensure(nEnt));
    HIP_TRY(h, h->splitU.ensure(nEnt));
    HIP_TRY(h, h->splitBlkCnt.ensure((size_t)nBlocks + 1));
    HIP_TRY(h, h->splitRuns.ensure((size_t)nBlocks / 16u + (size_t)h->ncu * 12u + 64u));
    HIP_TRY(h, h->splitCtl.ensure(4));
    HIP_TRY(h, hipMemsetAsync(h->splitCtl.p, 0, 16, h->stream));
    launch_evaluate_beams_split(a, h->splitId.p, h->splitMeta.p, h->splitK.p, h->splitU.p, h->splitBlkCnt.p, h->splitRuns.p,
                                h->splitCtl.p, h->beamPairs.p, h->blockKeyB.p, h->blockValB.p, nBlocks, h->bs->queueCtl.p + 3,
                                h->ncu, h->stream);
  } else
    launch_evaluate_beams(a, h->beamsPerWave, h->beamsExact && !primal, h->beamPairs.p, h->blockKeyB.p, h->blockValB.p, nBlocks,
                          h->bs->queueCtl.p + 3, h->nwaves, h->stream);
  HIP_TRY(h, hipEventRecord(ev->second, h->stream));
  // the shifts the fp32 evaluation left undecided (gather_beams.hip, exact_beams_kernel): in fp64, behind it, every gather
  if (!primal && !h->beamsExact) {
    launch_exact_beams(a, h->exTotals.p, h->stream);
    if (h->trace & TRACE_EXACT) {
      unsigned long long v[20];
      HIP_TRY(h, hipMemcpyAsync(v, h->exTotals.p, sizeof(v), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      fprintf(stderr, "[exact beams] so far %llu evaluated, %llu lost, longest list %llu; by cause 0..9:", v[0], v[1], v[2]);
      for (int k = 0; k < 10; ++k) fprintf(stderr, " %llu", v[4 + k]);
      fprintf(stderr, "\n");
    }
  }
  return GVPM_OK;
}

// computeVolumeGradientBeams, gvpm.cpp:880-986.  Everything on the gather stream.
int gatherBeams(gvpm_context *h, int it, uint64_t nb_paths, bool primal) {
  if (!h->haveBeamsMap) return fail(h, GVPM_ERR_STATE, "G-Beams gather needs gvpm_upload_beams");
  h->vpmOrderN = 0;  // (the block-sort buffers below also hold G-VPM's batch order)
  const float r = currentRadius(h);  // beamInitSize, gvpm.cpp:881
  // phases as for G-BRE (gvpm_get_phase_time): 2 = build (sub-beam grid, beam records, camera-beam sort, near lists),
  // 1 = plan + traversal, 0 = the evaluation (block sort + evaluate_beams2_kernel)
  EventPair *evBuild, *evTrav, *ev;
  int rc = nextEvents(h, &evBuild, 2);
  if (rc == GVPM_OK) rc = nextEvents(h, &evTrav, 1);
  if (rc != GVPM_OK) return rc;
  HIP_TRY(h, hipEventRecord(evBuild->first, h->stream));
  rc = refreshBuild(h, r);
  if (rc != GVPM_OK) return rc;
  h->iterClean = false;  // (this gather leaves `iter` written)
  HIP_TRY(h, hipMemsetAsync(h->iter.p, 0, h->npix * 27 * sizeof(float), h->stream));
  HIP_TRY(h, hipEventRecord(evBuild->second, h->stream));
  GatherArgs a;
  fillArgs(h, a, r);
  a.kernelRadius = r;
  // one cell layer per slab step (the box of a thicker slab grows with the tile's perspective spread, and the
  // traversal cost follows the number of sphere tests: 5.1 ms at 1 layer, 6.2 at 2, 8.9 at 4/6)
  if (!a.cfg.reserved[1]) a.cfg.reserved[1] = 1;
  if (!a.cfg.reserved[2]) a.cfg.reserved[2] = 1;
  a.radius = r + 0.5f * h->maxSubLen * 1.001f + 1e-6f;  // traversal radius: sub-beams are binned by their centre
  a.subLen = h->subLen;
  a.nbeams = h->nph;
  a.nph = h->nsub;
  a.beamClear = h->beamClear.p;
  a.cfg.reserved[5] = primal ? 1 : 0;  // the evaluation stops after the kernel record's base term
  rc = nextEvents(h, &ev);
  if (rc != GVPM_OK) return rc;
  uint32_t npairs = 0;
  rc = planAndTraverse(h, a, r, evTrav, npairs);
  if (rc != GVPM_OK) return rc;
  rc = evaluatePairs(h, a, npairs, it, nb_paths, primal, ev);
  if (rc != GVPM_OK) return rc;
  if (primal) {
    // BeamRadianceQuery takes the camera ray's transmittance over [Epsilon, w] (pm/beams.h:57-61,189-193) where the gradient
    // pass's kernel record takes it over [0, w] (shift_volume_beams.h:167,262): one factor exp(sigma_t Epsilon) on every term
    // (sigma_t is equal across the channels, gvpm_upload_medium)
    const float f = (float)std::exp((double)h->medium.sigma_t[0] * (double)h->cfg.epsilon);
    launch_scale(h->iter.p, h->iter.p, h->npix * 27, f, h->stream);
  }
  launch_finalize(h->accum.p, h->iter.p, h->npix * 27, it, nb_paths, h->stream);
  HIP_TRY(h, hipGetLastError());
  scaleVolumeAPA(h, it);
  return GVPM_OK;
}
