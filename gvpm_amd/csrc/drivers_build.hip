// The device builds the drivers share: the uniform grid over the photons (or the bundle cells), the occluder grid of the
// near-occluder lists and the counting sort of the camera-beam sets.  Host code only; every launch goes to h->bstream.
#include "drivers.h"

// tile shape and key space of the beam sort for `beamsPerWave` sets per wave
void beamTiling(const gvpm_context *h, int beamsPerWave, int &tw, int &th, uint32_t &ntiles, int &tileShift) {
  tw = 8;
  th = 4;
  if (beamsPerWave == 64) th = 8;
  if (beamsPerWave == 16) tw = 4;
  const uint32_t tilesX = (h->cfg.width + tw - 1) / tw, tilesY = (h->cfg.height + th - 1) / th;
  ntiles = tilesX * tilesY;
  tileShift = ilog2ceil(tw * th) + 3;
}

// The occluder grid of the near-occluder lists (grid_build.hip: near_grid_kernel; near_lists.h: nearVisit): count, scan, fill.  Once per
// scene: the one host read-back (the number of entries) stalls nothing that matters.
static int buildNearGrid(gvpm_context *h, float reach) {
  NearGrid g{};
  float ext[3], vol = 1.f;
  for (int c = 0; c < 3; ++c) {
    ext[c] = std::max(h->triMax[c] - h->triMin[c] + 2.02f * reach, 1e-6f);
    vol *= ext[c];
  }
  // about 64^3 cells, cubic ones: per axis extent / cell, cell = (volume / 64^3)^(1/3), at least 1, at most 256
  const float cell = std::cbrt(vol / 262144.f);
  size_t ncells = 1;
  for (int c = 0; c < 3; ++c) {
    g.dim[c] = std::max(1, std::min(256, (int)std::ceil(ext[c] / std::max(cell, 1e-9f))));
    g.org[c] = h->triMin[c] - 1.01f * reach;
    g.inv[c] = (float)g.dim[c] / ext[c];
    ncells *= (size_t)g.dim[c];
  }
  hipStream_t st = h->bstream;
  HIP_TRY(h, h->nearGridStart.ensure(ncells + 1));
  HIP_TRY(h, h->nearGridCount.ensure(ncells + 1));
  HIP_TRY(h, hipMemsetAsync(h->nearGridCount.p, 0, (ncells + 1) * sizeof(uint32_t), st));
  launch_near_grid(h->tri4.p, h->ntri, g, reach, h->nearGridCount.p, nullptr, 0, st);
  HIP_TRY(h, exclusiveSumU32(h->bs->sortTmp, h->nearGridCount.p, h->nearGridStart.p, (uint32_t)ncells + 1, st));
  uint32_t total = 0;
  HIP_TRY(h, hipMemcpyAsync(&total, h->nearGridStart.p + ncells, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipStreamSynchronize(st));
  HIP_TRY(h, h->nearGridTris.ensure((size_t)total + 1));
  HIP_TRY(h, hipMemsetAsync(h->nearGridCount.p, 0, (ncells + 1) * sizeof(uint32_t), st));
  g.start = h->nearGridStart.p;
  g.tris = h->nearGridTris.p;
  launch_near_grid(h->tri4.p, h->ntri, g, reach, h->nearGridCount.p, h->nearGridTris.p, 1, st);
  HIP_TRY(h, hipGetLastError());
  h->nearGrid = g;
  h->nearGridReach = reach;
  return GVPM_OK;
}

// The frame of the camera beams' bundle: common origin, mean direction, (u, v) range.  Two small reductions and a host
// wait, once; afterwards every planner run checks its rays against the frame (GatherArgs::bundleFlag).
static int fitBundle(gvpm_context *h) {
  h->bundleState = -1;
  if (!h->nsets || !h->raysDev) return GVPM_OK;
  HIP_TRY(h, h->bs->bounds6.ensure(32));
  double *dev = reinterpret_cast<double *>(h->bs->bounds6.p);
  double o[13];
  Grid g{};
  launch_bundle_fit(h->raysDev, h->nsets, 0, g, dev, h->bstream);
  HIP_TRY(h, hipMemcpyAsync(o, dev, sizeof(o), hipMemcpyDeviceToHost, h->bstream));
  HIP_TRY(h, hipStreamSynchronize(h->bstream));
  for (int k = 0; k < 13; ++k)
    if (!std::isfinite(o[k])) return GVPM_OK;
  const double cnt = o[12];
  if (!(cnt >= 1.0)) return GVPM_OK;
  // C = M^-1 b, M symmetric (adjugate); rays of one direction only (an orthographic sensor) leave M singular
  const double xx = o[0], xy = o[1], xz = o[2], yy = o[3], yz = o[4], zz = o[5];
  const double c00 = yy * zz - yz * yz, c01 = xz * yz - xy * zz, c02 = xy * yz - xz * yy;
  const double c11 = xx * zz - xz * xz, c12 = xy * xz - xx * yz, c22 = xx * yy - xy * xy;
  const double det = xx * c00 + xy * c01 + xz * c02;
  if (!(det > 1e-9 * cnt * cnt * cnt)) return GVPM_OK;
  const double C[3] = {(c00 * o[6] + c01 * o[7] + c02 * o[8]) / det, (c01 * o[6] + c11 * o[7] + c12 * o[8]) / det,
                       (c02 * o[6] + c12 * o[7] + c22 * o[8]) / det};
  double A[3] = {o[9], o[10], o[11]};
  const double len = std::sqrt(A[0] * A[0] + A[1] * A[1] + A[2] * A[2]);
  if (!(len > 0.2 * cnt)) return GVPM_OK;  // directions all over the sphere
  int sm = 0;
  for (int c = 0; c < 3; ++c) {
    A[c] /= len;
    if (fabs(A[c]) < fabs(A[sm])) sm = c;
  }
  double E[3] = {0, 0, 0}, U[3], V[3];
  E[sm] = 1.0;
  U[0] = A[1] * E[2] - A[2] * E[1]; U[1] = A[2] * E[0] - A[0] * E[2]; U[2] = A[0] * E[1] - A[1] * E[0];
  const double ul = std::sqrt(U[0] * U[0] + U[1] * U[1] + U[2] * U[2]);
  for (int c = 0; c < 3; ++c) U[c] /= ul;
  V[0] = A[1] * U[2] - A[2] * U[1]; V[1] = A[2] * U[0] - A[0] * U[2]; V[2] = A[0] * U[1] - A[1] * U[0];
  double c1 = 0;
  for (int c = 0; c < 3; ++c) {
    g.bo[c] = (float)C[c];
    g.ba[c] = (float)A[c];
    g.bu[c] = (float)U[c];
    g.bv[c] = (float)V[c];
    c1 += fabs(C[c]);
  }
  launch_bundle_fit(h->raysDev, h->nsets, 1, g, dev, h->bstream);
  HIP_TRY(h, hipMemcpyAsync(o, dev, sizeof(o), hipMemcpyDeviceToHost, h->bstream));
  HIP_TRY(h, hipStreamSynchronize(h->bstream));
  for (int k = 0; k < 8; ++k)
    if (!std::isfinite(o[k])) return GVPM_OK;
  if (!(o[4] > 0.15)) return GVPM_OK;  // a field of view near 180 degrees: (u, v) is no parametrisation for it
  // the lines must pass the point to fp32 rounding of positions of this size, and the point must not lie ahead of a start
  const double scale = 1.0 + c1 + fabs(o[6]) + fabs(o[7]);
  const double res = std::sqrt(std::max(o[5], 0.0));
  if (res > 4e-6 * scale || o[6] < -4e-6 * scale) return GVPM_OK;
  g.lineTol = (float)(2.0 * res + 4e-6 * scale);
  // the next uploads are the same sensor with other sub-pixel offsets: two pixels of margin
  const double px = std::max(o[1] - o[0], o[3] - o[2]) / (double)std::max(1, std::min(h->cfg.width, h->cfg.height));
  const double pad = 2.0 * px + 1e-5 * (1.0 + fabs(o[0]) + fabs(o[1]) + fabs(o[2]) + fabs(o[3]));
  g.uMin = (float)(o[0] - pad); g.uMax = (float)(o[1] + pad);
  g.vMin = (float)(o[2] - pad); g.vMax = (float)(o[3] + pad);
  g.mode = 1;
  h->bundleGrid = g;
  h->bundleState = 1;
  return GVPM_OK;
}

// cells of the bundle grid for this build: level-0 cells of 1 / bundleDiv of a tile's width
static Grid bundleCells(const gvpm_context *h, float r, int tileW) {
  Grid g = h->bundleGrid;
  const float range = fmaxf(g.uMax - g.uMin, g.vMax - g.vMin);
  const float tile = range * (float)tileW / (float)std::max(1, std::max(h->cfg.width, h->cfg.height));
  int G = 8;
  while (G < 512 && range / (float)G > tile / h->bundleDiv) G *= 2;
  int levels = 1;
  while ((1 << (levels - 1)) < G) ++levels;  // log2(G) + 1: the last level is one cell
  g.dim[0] = g.dim[1] = G;
  g.dim[2] = 2;
  g.levels = levels;
  g.ncells = (uint32_t)G * (uint32_t)G * 2u;
  g.s0 = range / (float)G;
  g.invS0 = 1.f / g.s0;
  g.radius = r;
  g.org[0] = g.org[1] = g.org[2] = 0.f;
  g.cell = g.s0;
  g.invCell = g.invS0;
  return g;
}

// buildGrid, first stage: the photons' bounds into b6 and their largest extent into ext -- the caller's, the previous set's
// (this set's then stay in flight, h->boundsPending) or reduced and read back here, with a host wait.
static int photonBounds(gvpm_context *h, const GridBuild &how, bool chain, float b6[6], float &ext) {
  const uint32_t n = h->nph;
  const bool deferred = how.deferred;
  const float *knownB6 = how.knownB6;
  const int nblocks = 1024;
  HIP_TRY(h, h->bs->boundsPartial.ensure(nblocks * 6));
  HIP_TRY(h, h->bs->bounds6.ensure(32));
  {
    const int rcp = ensurePinned(h);
    if (rcp != GVPM_OK) return rcp;
  }
  const bool defer = deferred && h->haveCachedBounds;
  if (!knownB6 && !(chain && defer))  // (the chain reduces the bounds in its own first two launches)
    launch_bounds(h->rawDev.pos, n, h->bs->boundsPartial.p, nblocks, h->bs->bounds6.p, defer ? h->pinB6 : nullptr,
                  h->bstream);
  if (knownB6) {
    memcpy(b6, knownB6, 6 * sizeof(float));
    memcpy(h->cachedB6, b6, 6 * sizeof(float));
    h->haveCachedBounds = true;
  } else if (defer) {
    h->boundsPending = true;
    memcpy(b6, h->cachedB6, 6 * sizeof(float));
  } else {
    HIP_TRY(h, hipMemcpyAsync(b6, h->bs->bounds6.p, 6 * sizeof(float), hipMemcpyDeviceToHost, h->bstream));
    HIP_TRY(h, hipStreamSynchronize(h->bstream));
    memcpy(h->cachedB6, b6, 6 * sizeof(float));
    h->haveCachedBounds = true;
  }
  ext = 0.f;
  for (int c = 0; c < 3; ++c) {
    if (!std::isfinite(b6[c]) || !std::isfinite(b6[3 + c])) return fail(h, GVPM_ERR_INVALID_ARG, "non-finite photon position");
    ext = fmaxf(ext, b6[3 + c] - b6[c]);
  }
  return GVPM_OK;
}

// buildGrid, second stage: the cells for kernel radius r over bounds b6 (clipped in place to what the camera beams can
// reach) -- the 3D grid, or G-BRE's bundle cells, whose frame is fitted here when it is not yet (a host wait, once).
static int sizeGrid(gvpm_context *h, float r, const GridBuild &how, float b6[6], float ext, Grid &g) {
  const uint32_t n = h->nph;
  const bool deferred = how.deferred;
  const float cellScale0 = h->cellScale > 0.f ? h->cellScale : (deferred && n <= 2000000u ? 1.5f : 1.0f);
  if (deferred && h->clipGrid && h->haveBeamBounds) {
    // G-BRE (round 6): the grid covers what the camera beams can reach, not what the photons fill.  An open scene's photons
    // fly far (S-cbox: extents of 2-5 times the box from step to step, 1.5-16 M cells), the beams end on its surfaces: the
    // cell arrays, their scan and the summed-volume table shrink to the box.  Photons outside sit (clamped) in the border cells,
    // as photons outside LAST step's bounds always have -- the binning and the footprints clamp alike, so the evaluated set
    // does not depend on where the grid ends; two cells of margin keep the beams' footprints off those border cells.  The
    // beams' bounds are the last step's (reduced by its build), like the photons'.
    float lo[3], hi[3], cell = cellScale0 * r;
    for (int pass = 0; pass < 2; ++pass) {
      const float pad = 1.01f * r + 2.f * cell;
      float e = 0.f;
      for (int c = 0; c < 3; ++c) {
        lo[c] = fmaxf(b6[c], h->beamB6[c] - pad);
        hi[c] = fminf(b6[3 + c], h->beamB6[3 + c] + pad);
        if (!(lo[c] <= hi[c])) lo[c] = hi[c] = fminf(fmaxf(h->beamB6[c], b6[c]), b6[3 + c]);  // (no photon near the beams)
        e = fmaxf(e, hi[c] - lo[c]);
      }
      cell = fmaxf(cellScale0 * r, e / 384.f);
      ext = e;
    }
    for (int c = 0; c < 3; ++c) {
      b6[c] = lo[c];
      b6[3 + c] = hi[c];
    }
  }
  g = Grid{};
  // cell edge in radii.  G-BRE with maps up to 2 M photons: 1.5 -- the cell arrays (memset, scan, summed-volume table:
  // ~135 of the build's 575 us at C2 with cells of one radius) shrink 3.4x, and there the build is the stage the
  // pipelined step waits for; the traversal tests 1.3x the photons per hit.  Measured at C2: 1.51 -> 1.43-1.445 ms per
  // step.  At C4 (4 M photons) the evaluation is the long stage and the larger cells cost the traversal 1 % of the step.
  const float cellScale = cellScale0;
  float cell = fmaxf(cellScale * r, ext / 384.f);
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
  // (round 6: the automatic choice is OFF -- with the grid clipped to the beams' reach and the planner walking four chunks a wave
  // the 3D grid is the faster one for a rank's share too: C4, rank 0 of 8 / of 4: 2.36-2.39 / 3.90 ms a step against 2.47 /
  // 4.02 with the bundle cells, alternating runs.  GVPM_BUNDLE=1 forces them, GVPM_BUNDLE_AUTO=1 restores the choice.)
  if (deferred && !h->bundleFromEnv && h->bundleAuto) {
    // "a rank's share of an image-sharded frame": the beam sets cover at most half of the pixels.  With hysteresis (ADVICE
    // round 4): a frame whose medium covers about half the pixels must not flip the cell kind -- and the planner's tuning with
    // it -- from step to step; the kind is left only beyond 0.6 / below 0.4 of the frame.
    const size_t twice = (size_t)h->nsets * 2u;
    const bool sharded = h->nsets > 0 && (h->bundleEnabled ? twice * 5u <= h->npix * 6u : twice * 5u <= h->npix * 4u);
    if (sharded != h->bundleEnabled) {
      h->bundleEnabled = sharded;
      if (sharded && h->bundleState < 0) h->bundleState = 0;  // (a frame that failed earlier is tried again, a few times)
    }
  }
  if (deferred && h->bundleEnabled && h->bundleState >= 0 && !how.force3D) {
    // G-BRE: the camera beams of a pinhole sensor leave one point -- cells over the bundle's (u, v) plane instead
    if (h->bundleState == 0) {
      const int rcf = fitBundle(h);
      if (rcf != GVPM_OK) return rcf;
    }
    if (h->bundleState == 1) g = bundleCells(h, r, h->beamsPerWave == 16 ? 4 : 8);
  }
  return GVPM_OK;
}

// buildGrid, third stage: the photon and cell arrays for grid g, their counters zeroed; without the chain also the count,
// the scan and G-BRE's summed-volume table.  sub: the striped counters of bundle cells (null for the 3D grid).
static int cellArrays(gvpm_context *h, const Grid &g, bool deferred, bool chain, const ChainPrep *cp, uint32_t *&sub) {
  const uint32_t n = h->nph;
  // counting sort by cell (x fastest): count + rank, exclusive scan, scatter
  HIP_TRY(h, h->bs->keysA.ensure(n));
  HIP_TRY(h, h->bs->valsA.ensure(n));
  HIP_TRY(h, h->bs->hot.ensure(n));
  HIP_TRY(h, h->bs->cold.ensure((size_t)n * GVPM_REC_QUADS));
  // the radius shrinks every iteration, so the grid grows: size the cell arrays (and the scan's temporary)
  // for the finest grid the cell rule allows (386^3 cells, 230 MB each) once -- a regrowth is a hipFree,
  // i.e. a device-wide sync in the middle of the pipeline
  const size_t worstCells = (size_t)386 * 386 * 386 + 2;
  // (the chain counts and scans the beam sets' tile keys behind the cells, in the same two arrays)
  const size_t keyRoom = chain ? (size_t)cp->nkeys + 4u : 0u;
  {
    const uint32_t *was = h->bs->cellCount.p;
    HIP_TRY(h, h->bs->cellCount.ensure(std::max((size_t)g.ncells + 2, worstCells) + keyRoom));
    if (h->bs->cellCount.p != was) h->bs->countsClean = false;
  }
  HIP_TRY(h, h->bs->cellStart.ensure(std::max((size_t)g.ncells + 2, worstCells) + keyRoom));
  if (!h->bs->scanSized || (chain && !h->bs->scanSizedChain)) {
    HIP_TRY(h, reserveScanTemp(h->bs->sortTmp, (uint32_t)std::min<size_t>(worstCells + keyRoom, 0x7FFFFFF0u)));
    h->bs->scanSized = true;
    h->bs->scanSizedChain = chain;
  }
  if (chain) {
    // the chain hands its counters back zeroed: one memset when the array is new, or was last used by the separate launches
    if (!h->bs->countsClean) HIP_TRY(h, hipMemsetAsync(h->bs->cellCount.p, 0, h->bs->cellCount.cap * sizeof(uint32_t), h->bstream));
    h->bs->countsClean = true;
  } else {
    HIP_TRY(h, hipMemsetAsync(h->bs->cellCount.p, 0, ((size_t)g.ncells + 1) * sizeof(uint32_t), h->bstream));
    h->bs->countsClean = false;
  }
  // (bundle cells: striped counters, grid_build.hip cell_count_kernel)
  sub = nullptr;
  if (g.mode == 1) {
    // (the chain: counters + their prefixes, and the counters are handed back zeroed -- one memset when the array is new, has
    // another size or was last used by the separate launches)
    const size_t subWords = (size_t)cell_stripes() * g.ncells;
    const uint32_t *was = h->bs->cellSub.p;
    HIP_TRY(h, h->bs->cellSub.ensure(subWords * (chain ? 2u : 1u)));
    if (!chain || h->bs->cellSub.p != was || h->bs->subCleanWords != subWords)
      HIP_TRY(h, hipMemsetAsync(h->bs->cellSub.p, 0, subWords * sizeof(uint32_t), h->bstream));
    h->bs->subCleanWords = chain ? subWords : 0u;
    sub = h->bs->cellSub.p;
  }
  // extension lists of the near-occluder lists: sized once per set for the largest photon count (grow only); word 0 is the
  // allocation cursor.  The count kernel starts it at 1 and the lists' overflow counter at 0 (two memsets less per build).
  HIP_TRY(h, h->bs->overflowCtr.ensure(2));
  const size_t extWant = std::min<size_t>(std::max<size_t>((size_t)n * 8u + 4096u, h->nearExtWant), 0xFFFFFF00u);
  HIP_TRY(h, h->bs->nearExt.ensure(extWant));
  if (!chain) {
    launch_cell_count(h->rawDev.pos, n, g, h->bs->keysA.p, h->bs->valsA.p, h->bs->cellCount.p, sub, h->bstream, h->bs->overflowCtr.p,
                      h->bs->nearExt.p);
    HIP_TRY(h, exclusiveSumU32(h->bs->sortTmp, h->bs->cellCount.p, h->bs->cellStart.p, g.ncells + 1, h->bstream));
  }
  if (deferred) {
    // G-BRE: summed-volume table for the planner (sized once for the finest grid, like the cell arrays)
    const size_t satCells = (size_t)(g.dim[0] + 1) * (g.dim[1] + 1) * (g.dim[2] + 1);
    HIP_TRY(h, h->bs->sat.ensure(std::max(satCells, (size_t)387 * 387 * 387)));
    if (!chain) launch_sat(h->bs->cellStart.p, g, h->bs->sat.p, h->bstream);
  }
  return GVPM_OK;
}

// uniform grid over the photons for kernel radius r (GridBuild in drivers.h: where the bounds come from, which cells)
int buildGrid(gvpm_context *h, float r, const GridBuild &how) {
  const uint32_t n = h->nph;
  const bool deferred = how.deferred;
  ChainPrep *cp = how.chain;
  h->boundsPending = false;
  const bool chain = cp && cp->on && n > 0;
  if (cp) cp->on = chain;
  if (n == 0) {
    h->bs->grid = Grid{{0, 0, 0}, 1.f, 1.f, {1, 1, 1}, 1};
    HIP_TRY(h, h->bs->cellStart.ensure(2));
    HIP_TRY(h, hipMemsetAsync(h->bs->cellStart.p, 0, 2 * sizeof(uint32_t), h->bstream));
    return GVPM_OK;
  }
  float b6[6], ext = 0.f;
  Grid g{};
  uint32_t *sub = nullptr;
  int rc = photonBounds(h, how, chain, b6, ext);
  if (rc == GVPM_OK) rc = sizeGrid(h, r, how, b6, ext, g);
  if (rc != GVPM_OK) return rc;
  h->bs->grid = g;
  rc = cellArrays(h, g, deferred, chain, cp, sub);
  if (rc != GVPM_OK) return rc;
  // longest possible reconnection segment: diagonal of (occluders U photons), generously padded
  float diag2 = 0.f;
  for (int c = 0; c < 3; ++c) {
    const float lo = fminf(b6[c], h->ntri ? h->triMin[c] : b6[c]), hi = fmaxf(b6[3 + c], h->ntri ? h->triMax[c] : b6[3 + c]);
    diag2 += (hi - lo) * (hi - lo);
  }
  const float lmax = 1.25f * sqrtf(diag2) + 8.f * r + 1e-3f;
  const float dmax = h->cfg.shadow_epsilon * lmax * 1.01f + 1e-6f;
  if (h->ntri > 64u && h->useNearGrid && !(dmax <= h->nearGridReach)) {
    // (the occluder grid belongs to the handle, not to a build set: a gather that still reads it on the other stream ends first)
    if (h->bstream != h->stream) HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->streamA2) HIP_TRY(h, hipStreamSynchronize(h->streamA2));
    const int rcg = buildNearGrid(h, dmax * 1.5f);
    if (rcg != GVPM_OK) return rcg;
  }
  const bool wantOrig = h->reqCap > 0 && h->cfg.use_manifold;  // (host-shift requests name photons by their place in the upload)
  if (wantOrig) HIP_TRY(h, h->bs->origIdx.ensure((size_t)n + 1));
  if (chain) {
    cp->dmax = dmax;
    cp->wantOrig = wantOrig;
    cp->sub = sub;
    h->nearOverflow = false;
    return GVPM_OK;
  }
  launch_reorder(h->rawDev, h->bs->keysA.p, h->bs->valsA.p, h->bs->cellStart.p, n, h->cfg, h->bvh.p, h->tri4.p, h->ntri, dmax,
                 h->nearGrid, h->bs->nearExt.p, (uint32_t)std::min<size_t>(h->bs->nearExt.cap, 0xFFFFFF00u), h->bs->hot.p,
                 h->bs->cold.p, h->bs->overflowCtr.p, wantOrig ? h->bs->origIdx.p : nullptr, sub, g.ncells, h->bstream, h->nearScalar);
  HIP_TRY(h, hipGetLastError());
  h->nearOverflow = false;
  if (!deferred && h->cfg.visibility_as_written) {
    launch_export_u32(h->bs->overflowCtr.p, nullptr, nullptr, nullptr, nullptr, h->pinCtl, h->bstream);
    HIP_TRY(h, hipStreamSynchronize(h->bstream));
    h->nearOverflow = h->pinCtl[0] != 0;
  }
  return GVPM_OK;
}

int sortBeams(gvpm_context *h, int beamsPerWave, const ChainPrep *cp) {
  const uint32_t n = h->nsets;
  if (!beamsPerWave) beamsPerWave = h->beamsPerWave;
  int tw, th, tileShift;
  uint32_t ntilesAll;
  beamTiling(h, beamsPerWave, tw, th, ntilesAll, tileShift);
  h->bs->ntiles = ntilesAll;
  h->bs->tileW = tw;
  h->bs->tileH = th;
  HIP_TRY(h, h->bs->tileStart.ensure((size_t)h->bs->ntiles + 2));
  HIP_TRY(h, h->bs->bKeysA.ensure(n + 1));
  HIP_TRY(h, h->bs->bValsA.ensure(n + 1));
  HIP_TRY(h, h->bs->setPerm.ensure(n + 1));
  if (cp && cp->on) return GVPM_OK;  // (counted, scanned and scattered by the build chain)
  if (n) {
    // counting sort by (tile, pixel in tile, edge): count + rank, exclusive scan, scatter
    const uint64_t nkeys = (uint64_t)h->bs->ntiles << tileShift;
    if (nkeys > 0x7FFFFFF0ull) return fail(h, GVPM_ERR_INVALID_ARG, "film too large for the beam sort");
    HIP_TRY(h, h->bs->beamCount.ensure(nkeys + 2));
    HIP_TRY(h, h->bs->beamStart.ensure(nkeys + 2));
    HIP_TRY(h, hipMemsetAsync(h->bs->beamCount.p, 0, (nkeys + 1) * sizeof(uint32_t), h->bstream));
    launch_beam_count(h->raysDev, n, h->cfg.width, tw, th, h->bs->bKeysA.p, h->bs->bValsA.p, h->bs->beamCount.p, h->bstream);
    HIP_TRY(h, exclusiveSumU32(h->bs->sortTmp, h->bs->beamCount.p, h->bs->beamStart.p, (uint32_t)nkeys + 1, h->bstream));
    launch_beam_scatter(h->bs->bKeysA.p, h->bs->bValsA.p, h->bs->beamStart.p, n, h->bs->setPerm.p, h->bstream);
    launch_tile_start(h->bs->beamStart.p, h->bs->ntiles, (uint32_t)tileShift, h->bs->tileStart.p, h->bstream);
  } else {
    HIP_TRY(h, hipMemsetAsync(h->bs->tileStart.p, 0, ((size_t)h->bs->ntiles + 1) * sizeof(uint32_t), h->bstream));
  }
  HIP_TRY(h, hipGetLastError());
  return GVPM_OK;
}
