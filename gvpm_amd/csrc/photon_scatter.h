// The photon scatter: an uploaded photon (SoA) -> its hot record, its 128-byte cold record and its near-occluder list.
// Included by grid_build.hip (reorder_kernel), build_chain.hip (chain_tail_kernel) and beams_build.hip (RawPhotons, ld3).
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "grid_cells.h"
#include "near_lists.h"
#include "shift_device.h"
#include "vec.h"

namespace gvpm {

// ---- the SoA upload layout ------------------------------------------------------------------
struct RawPhotons {
  const float *pos, *wi, *flux, *parent_pos, *parent_n, *prefix_w, *parent_scat, *parent_wi;
  const float *parent_pdf, *edge_pdf, *parent_rr, *parent_g;
  const uint32_t *flags, *path_id;
};
inline RawPhotons rawOf(const gvpm_photon_soa &s) {
  return RawPhotons{s.pos,       s.wi,         s.flux,     s.parent_pos, s.parent_n, s.prefix_w, s.parent_scat,
                    s.parent_wi, s.parent_pdf, s.edge_pdf, s.parent_rr,  s.parent_g, s.flags,    s.path_id};
}

__device__ __forceinline__ float4 ld3(const float *p, uint32_t i, float w) {
  return make_float4(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2], w);
}

// counting sort, pass 3: photon `src` (reads in upload order: coalesced) goes to slot cellStart[key] + rank
// (whole 128-byte records: full-line writes)
struct ReorderLds {
  float4 stg[64][GVPM_REC_QUADS / 2 + 1];  // half a record a pass; +1: odd stride against bank conflicts (5 KB: one wave a block)
  uint32_t dstIdx[64];
};
// bid: which 64 photons of the upload this wave takes (the kernel's block index, or the block's index among the reorder
// blocks of the build chain's tail kernel)
template <int MODE>
__device__ __forceinline__ void reorderBody(const RawPhotons &r, const uint32_t *__restrict__ keys,
                                            const uint32_t *__restrict__ rank,
                                            const uint32_t *__restrict__ cellStart, uint32_t n,
                                            const gvpm_params &cfg, const float4 *bvh, const float4 *tri4,
                                            uint32_t ntri, float dmax, const NearGrid &ng, uint32_t *nearExt,
                                            uint32_t extCap, float4 *hot, float4 *cold, uint32_t *overflow,
                                            uint32_t *origIdx, const uint32_t *__restrict__ sub, uint32_t ncells, uint32_t bid,
                                            uint32_t *counts, uint32_t *subCount, ReorderLds &L) {
  // The record is assembled in LDS and written by EIGHT lanes (one 16-byte quad each): a store instruction then
  // covers whole 64-byte halves of eight records instead of sixty-four 16-byte pieces of sixty-four lines.  Two passes of four
  // quads (round 6: 5 KB of LDS a wave instead of 9.5 -- the kernel runs beside the evaluation and the traversal).
  auto &stg = L.stg;
  auto &dstIdx = L.dstIdx;
  const uint32_t src = bid * 64u + threadIdx.x;
  const int t = threadIdx.x;
  constexpr int HALF = GVPM_REC_QUADS / 2;
  dstIdx[t] = 0xFFFFFFFFu;
  float4 q4 = make_float4(0.f, 0.f, 0.f, 0.f), q5 = q4, q6 = q4, q7 = q4;
  const bool live = src < n && (counts || rank[src] != 0xFFFFFFFFu);  // (0xFFFFFFFF: outside the bundle, cell_count_kernel)
  if (live) {
    // (sub: the photon's rank counts within its stripe of the cell, cell_count_kernel)
    // (counts: the build chain -- no ranks were taken when the cells were counted; the counter is counted back down here)
    // (subCount: the chain with bundle cells -- the stripe's counter is counted back down, its prefix within the cell is in `sub`)
    uint32_t i;
    if (counts) i = cellStart[keys[src]] + (atomicSub(&counts[keys[src]], 1u) - 1u);
    else if (subCount) {
      const size_t sk = (size_t)(src % CELL_STRIPES) * ncells + keys[src];
      i = cellStart[keys[src]] + sub[sk] + (atomicSub(&subCount[sk], 1u) - 1u);
    } else i = cellStart[keys[src]] + rank[src] + (sub ? sub[(size_t)(src % CELL_STRIPES) * ncells + keys[src]] : 0u);
    uint32_t bits = r.flags[src] & ~((1u << 6) | (1u << GVPM_HOT_PARITY_BIT));
    if (photonContributes(bits, cfg)) bits |= 1u << 6;
    bits |= (r.path_id[src] & 1u) << GVPM_HOT_PARITY_BIT;
    const float4 h0 = ld3(r.pos, src, __uint_as_float(bits));
    hot[i] = h0;
    if (origIdx) origIdx[i] = src;  // (host-shift requests name photons by their place in the upload)
    // one 128-byte record per photon: an evaluation touches exactly one cache line
    stg[t][0] = h0;
    stg[t][1] = ld3(r.wi, src, r.parent_pdf[src]);
    stg[t][2] = ld3(r.flux, src, r.edge_pdf[src]);
    stg[t][3] = ld3(r.parent_pos, src, r.parent_rr[src]);
    q4 = ld3(r.parent_n, src, r.parent_g[src]);
    const f3 P = mk3(r.parent_pos[3 * (size_t)src], r.parent_pos[3 * (size_t)src + 1], r.parent_pos[3 * (size_t)src + 2]);
    const f3 PN = mk3(q4.x, q4.y, q4.z);
    const NearList nl = nearOccluders<MODE>(P, PN, bvh, tri4, ntri, dmax, ng, nearExt, extCap, cfg.epsilon);
    const uint32_t w0 = nl.w0, w1 = nl.w1, w2 = nl.w2;
    const float cstar = nl.cstar;
    if ((w0 >> 24) == 0xFEu) atomicAdd(overflow, 1u);
    // (bit 15 of the COLD record's flags only -- the depth field's top bit, which the evaluation does not read: "word 2 of the
    // near list is the reach of the wall the parent sits behind"; the hot record the traversal filters by keeps the flags)
    stg[t][0].w = __uint_as_float((bits & ~(1u << 15)) | (cstar > 0.f ? 1u << 15 : 0u));
    q5 = ld3(r.prefix_w, src, __uint_as_float(w0));
    q6 = ld3(r.parent_scat, src, __uint_as_float(w1));
    q7 = ld3(r.parent_wi, src, __uint_as_float(w2));
    dstIdx[t] = i;
  }
  __syncthreads();
  for (int e = t; e < 64 * HALF; e += 64) {
    const int rec = e / HALF, part = e % HALF;
    const uint32_t i = dstIdx[rec];
    if (i != 0xFFFFFFFFu) cold[(size_t)i * GVPM_REC_QUADS + part] = stg[rec][part];
  }
  __syncthreads();
  if (live) {
    stg[t][0] = q4;
    stg[t][1] = q5;
    stg[t][2] = q6;
    stg[t][3] = q7;
  }
  __syncthreads();
  for (int e = t; e < 64 * HALF; e += 64) {
    const int rec = e / HALF, part = e % HALF;
    const uint32_t i = dstIdx[rec];
    if (i != 0xFFFFFFFFu) cold[(size_t)i * GVPM_REC_QUADS + HALF + part] = stg[rec][part];
  }
}

}  // namespace gvpm
