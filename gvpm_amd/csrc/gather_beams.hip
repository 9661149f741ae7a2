// G-Beams (beam x beam) gather + gradient-domain shift for gfx950, hand-written HIP: the evaluation and the sub-beam build.
//
// Replaces, for one SPPM iteration, the body of
//   GPMIntegrator::computeVolumeGradientBeams     gvpm/gvpm.cpp:880-986
// in three units: this one cuts the photon beams into sub-beams for the grid (at the end of the file) and evaluates the
// (camera ray, sub-beam) pairs -- the default fp32 kernel, then the literal fp64 evaluation and the exact pass;
// gather_beams_trav.hip lists the pairs (the reference's SubBeamBVH query); gather_beams_split.hip is the fp32 evaluation as two
// kernels (opt-in).  The reference's functions the evaluation re-derives are listed with their transcription
// (beams_eval_f64.h).
// The kernels of this file stay in ONE module, in this order: compiled apart, or with the fused kernel's <B, true>
// instantiations elsewhere, their instructions are no longer the ones measured (NOTEBOOK.md, round 11).
//
// The evaluation runs in fp32 in a local frame (beams_eval_f32.h, beams_shift_f32.h), in two
// phases (base + null shifts, then the queued reconnections); the literal fp64 transcription of the
// reference with its float intermediates settles the ownership decisions that fall inside the fp32 error band
// (beamKernelExact), and the shifts with whose own decisions fp32 cannot be trusted are noted for exact_beams_kernel.
#include <hip/hip_runtime.h>

#include "beams_common.h"
#include "beams_eval_f32.h"
#include "beams_shift_f32.h"
#include "device_types.h"
#include "dmath.h"
#include "shift_device.h"
#include "tile_walk.h"
#include "vec.h"

namespace gvpm {

#ifdef GVPM_BEAMS_AUDIT
// probe builds only: the audit log beamBase keeps (beams_shift_f32.h), as this unit's kernels wrote it
extern "C" int gvpm_debug_beams_audit(unsigned int *count, float *log, float *ratio) {
  if (hipMemcpyFromSymbol(count, HIP_SYMBOL(gvpmAuditCount), 4) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(log, HIP_SYMBOL(gvpmAuditLog), sizeof(float) * 256 * 16) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(ratio, HIP_SYMBOL(gvpmAuditRatio), 32) != hipSuccess) return -1;
  return 0;
}
#endif

// The rest of shiftBeamME once the host has run the walks (results == nullptr: it has not -- every request is a failed shift):
// kernelPDF of the proposal's last edge against the shifted ray (:653-663), Jacobian (:665-686), the shifted camera terms
// (:688-703), MIS (:705-733), then the accumulation of BeamGradRadianceQuery::operator() (:330-350).  For G-Beams the answer's
// `wi` is the proposal's last edge as a VECTOR from the new vertex to its predecessor (direction and length).
__global__ __launch_bounds__(256) void apply_host_shifts_beams_kernel(GatherArgs a, const gvpm_host_shift *__restrict__ results, uint32_t n) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t ok = 0, bad = 0;
  if (k < n) {
    const float4 c0 = a.reqCtx[5 * (size_t)k], c1 = a.reqCtx[5 * (size_t)k + 1], c2 = a.reqCtx[5 * (size_t)k + 2],
                 c3 = a.reqCtx[5 * (size_t)k + 3], c4 = a.reqCtx[5 * (size_t)k + 4];
    const f3 bcv = mk3(c2.x, c2.y, c2.z), eye = mk3(c3.x, c3.y, c3.z);
    const float shiftW = c1.w, wkrr = c2.w, sMIS = c3.w, radius = c4.x;
    const uint32_t pix = __float_as_uint(c4.y);
    const int i = (int)__float_as_uint(c4.z);
    float w = 1.f;
    f3 sflux = mk3(0.f);
    bool good = false;
    if (results && results[k].ok) {
      const gvpm_host_shift r = results[k];
      const gvpm_shift_request rq = a.reqHost[k];
      const d3 wiV = mkd(r.wi[0], r.wi[1], r.wi[2]);
      const double newLen = sqrt(len2(wiV));
      const double jac = (double)r.det_ratio;
      if (newLen > 0.0) {
        const d3 edgeD = wiV * (-1.0 / newLen);  // proposal.edge(c - 1)->d
        const d3 newPos = mkd(rq.offset_pos[0], rq.offset_pos[1], rq.offset_pos[2]);
        const d3 orgBeam = newPos + wiV;         // proposal.vertex(c - 1)
        KRecD kr;
        kr.radius = (double)radius;
        const RayD shRay{mkd(c0.x, c0.y, c0.z), mkd(c1.x, c1.y, c1.z), (double)a.cfg.epsilon, (double)c0.w};
        const double shiftKernelPDF = kernelPDF(kr, a.cfg.vol_technique, shRay, orgBeam, edgeD, newLen);
        if (shiftKernelPDF != 0.0 && jac > 0.0 && isfinite(jac)) {
          good = true;
          const float tr = mediumEvalF(a.med, shiftW).tr;
          const f3 sigS = mk3(a.med.sigmaS[0], a.med.sigmaS[1], a.med.sigmaS[2]);
          const f3 shD = mk3(c1.x, c1.y, c1.z);
          const float phaseTerm = phaseEval(a.med.g, tof(edgeD) * -1.f, -shD);
          sflux = mk3(r.throughput[0], r.throughput[1], r.throughput[2]) * sigS * (tr * phaseTerm) * eye * (float)jac;
          w = 0.5f;
          if (a.cfg.use_mis) {
            const double offsetPdf = (double)r.pdf * shiftKernelPDF, basePdf = (double)r.base_pdf;
            if (basePdf == 0.0) {
              w = 0.f;
            } else if (offsetPdf == 0.0) {
              w = 1.f;
            } else {
              const double x = (double)sMIS * jac * (offsetPdf / basePdf);
              w = (float)(a.cfg.power_heuristic ? 1.0 / (1.0 + x * x) : 1.0 / (1.0 + x));
            }
          }
        }
      }
    }
    if (beamBorder(a, pix, i)) w = 1.f;
    const size_t p = (size_t)(pix >> 16) * a.cfg.width + (pix & 0xFFFFu);
    float *dst = a.iter + p * 27;
    const float ws = w * wkrr * a.iterScale, wb = w * a.iterScale;
    if (sflux.x != 0.f || sflux.y != 0.f || sflux.z != 0.f) {
      atomicAdd(&dst[3 + 3 * i + 0], sflux.x * ws);
      atomicAdd(&dst[3 + 3 * i + 1], sflux.y * ws);
      atomicAdd(&dst[3 + 3 * i + 2], sflux.z * ws);
    }
    atomicAdd(&dst[15 + 3 * i + 0], bcv.x * wb);
    atomicAdd(&dst[15 + 3 * i + 1], bcv.y * wb);
    atomicAdd(&dst[15 + 3 * i + 2], bcv.z * wb);
    ok = good ? 1u : 0u;
    bad = good ? 0u : 1u;
  }
  const uint32_t nOk = (uint32_t)__popcll(__ballot(ok != 0u)), nBad = (uint32_t)__popcll(__ballot(bad != 0u));
  if ((threadIdx.x & 63) == 0 && (nOk | nBad)) {
    atomicAdd(&statRow(a)[3], (unsigned long long)nOk);
    atomicAdd(&statRow(a)[4], (unsigned long long)nBad);
  }
}
void launch_apply_host_shifts_beams(const GatherArgs &a, const gvpm_host_shift *results, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(apply_host_shifts_beams_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, results, n);
}

// ---- evaluation, fp32 path: two phases ----------------------------------------------------------------------------
// As the fp64 evaluation (below: blocks of 64 pairs sorted by tile, RUN blocks per reservation), but a block
// goes through phase 1 only (beamBase + beamShift1: kernel record, base contribution, null shifts); the reconnections it needs are appended to
// a wave-wide LDS ring (ballot + popcount; 40 bytes each) and run 64 at a time through phase 2 (beamShift2) whenever
// the ring holds a full wave of them, and completely before the tile's accumulators are flushed.
// The reconnections waiting for phase 2 and the ones the first round deferred share ONE pool of entries, as two stacks
// growing towards each other (the order of the reconnections is free: they only add to the accumulators): a block appends at
// most 4 x 64 to at most 63 that wait from the block before, and at most 63 deferred ones wait beside them -- 382; a drain moves
// entries from the lower stack to the upper one, never more.  (Until round 4 two rings of 320 + 128 entries: the 1.8 KB this
// saves are what takes the kernel from 7 to 8 resident waves per CU at B = 16.)

#ifdef GVPM_EVAL_TIMING
// probe builds only: per wave of the last launch, shader-clock ticks in [0] beamBase [1] beamShift1 + push [2] phase 2
// [3] tile change (flush, rays) [7] lifetime; [4] blocks [5] pairs alive after beamBase [6] reconnections
__device__ unsigned long long gvpmBeamsLog[8 * 16384];
extern "C" int gvpm_debug_beams_timing(unsigned long long *out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(gvpmBeamsLog), sizeof(gvpmBeamsLog)) == hipSuccess ? 0 : -1;
}
__device__ __forceinline__ unsigned long long beamsTick() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
  return t;
}
#define BTICK() beamsTick()
#else
#define BTICK() 0ull
#endif

template <int B, bool HS = false>
__global__ __launch_bounds__(64, B == 64 ? 1 : 2) void evaluate_beams2_kernel(GatherArgs a, const uint2 *__restrict__ pairs,
                                                                             const uint32_t *__restrict__ sortedKey,
                                                                             const uint32_t *__restrict__ sortedBlock,
                                                                             uint32_t nBlocks, uint32_t *queueHead) {
  constexpr uint32_t RUN = GVPM_BEAMS_RUN, RUN_MIN = GVPM_BEAMS_RUN_MIN;
  __shared__ BeamEvalLds<B> s;
  extern __shared__ float4 sceneTri[];  // occluders of a small scene (dynamic: 48 bytes each, none for larger scenes)
  const int lane = threadIdx.x;
  const float4 *ldsTri = nullptr;
  if (a.ntri <= BEAM_LDS_TRIS) {
    for (uint32_t i = lane; i < 3u * a.ntri; i += 64u) sceneTri[i] = a.tri4[i];
    ldsTri = sceneTri;
    __syncthreads();
  }
  uint32_t nEval = 0, nNull = 0, nDiff = 0, nFail = 0;
  uint32_t curBase = 0xFFFFFFFFu, curNb = 0;
  uint32_t qCount = 0;  // the lower stack of the pool, wave-uniform
  [[maybe_unused]] unsigned long long bt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  [[maybe_unused]] const unsigned long long btStart = BTICK();
  uint32_t vCount = 0;  // the deferred ones: the upper stack, wave-uniform
  auto drainVis = [&](uint32_t n) __attribute__((always_inline)) {  // n <= 64 deferred reconnections through the any-hit loop
    __syncthreads();
    if ((uint32_t)lane < n) {
      const uint32_t e = (uint32_t)BPOOL - vCount + (uint32_t)lane;  // the last n pushed
      BeamPQ q;
      q.id = s.qid[e];
      q.meta = s.qmeta[e];
      q.k = s.qk[e];
      q.u = s.qu[e];
      bool defer;
      beamShift2<B, HS>(a, s, q, ldsTri, true, defer, nDiff, nFail, curBase);
    }
    vCount -= n;
  };
  auto drain = [&](uint32_t n) __attribute__((always_inline)) {   // n <= 64 entries of the ring through phase 2 (first round)
    [[maybe_unused]] const unsigned long long d0 = BTICK();
    bt[6] += n;
    __syncthreads();
    bool defer = false;
    BeamPQ q = {};
    if ((uint32_t)lane < n) {
      const uint32_t e = qCount - n + (uint32_t)lane;  // the last n pushed
      q.id = s.qid[e];
      q.meta = s.qmeta[e];
      q.k = s.qk[e];
      q.u = s.qu[e];
      beamShift2<B, HS>(a, s, q, ldsTri, false, defer, nDiff, nFail, curBase);
    }
    qCount -= n;
    const unsigned long long dm = __ballot(defer);
    if (dm) {
      // (one wave per workgroup: every lane has read its entry before any lane pushes -- the upper stack may grow into the
      // slots just popped)
      if (defer) {
        const uint32_t slot = (uint32_t)BPOOL - 1u - vCount - (uint32_t)__popcll(dm & ((1ull << lane) - 1ull));
        s.qid[slot] = q.id;
        s.qmeta[slot] = q.meta;
        s.qk[slot] = q.k;
        s.qu[slot] = q.u;
      }
      vCount += (uint32_t)__popcll(dm);
      if (vCount >= 64u) drainVis(64u);
    }
    bt[2] += BTICK() - d0;
  };
  auto flushTile = [&]() __attribute__((always_inline)) {
    while (qCount) drain(min(qCount, 64u));
    while (vCount) drainVis(min(vCount, 64u));
    __syncthreads();
    if (curBase != 0xFFFFFFFFu) {
      for (int idx = lane; idx < 27 * B; idx += 64) {
        const int k = idx / B, bb = idx % B;
        if ((uint32_t)bb < curNb) {
          const float v = (float)s.acc[k][bb];
          if (v != 0.f) {
            const uint32_t pv = s.pix[bb];
            const size_t p = (size_t)(pv >> 16) * a.cfg.width + (pv & 0xFFFFu);
            atomicAdd(&a.iter[p * 27 + k], v);
          }
        }
      }
    }
    __syncthreads();
  };
  // Runs of blocks, guided: a run ends with the tile's flush (27 x B film atomics, the next tile's rays), so runs are long (at
  // C3 a tile has ~134 blocks: runs of 8 spent 11 % of the kernel in tile changes, 18.1 ms; runs of 32: 16.7; guided from 256
  // down to 16: 16.2) and shrink towards the end of the list, so that the waves still finish together.
  bool firstItem = true;
  const uint32_t run0 = min(RUN, max(RUN_MIN, nBlocks / (4u * gridDim.x)));  // the first run of every wave is its own
  const uint32_t firstDyn = gridDim.x * run0;
  for (;;) {
    uint32_t b0 = blockIdx.x * run0, cnt = run0;
    if (!firstItem) {
      if (lane == 0) {
        const uint32_t seen = firstDyn + __hip_atomic_load(queueHead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t rem = seen < nBlocks ? nBlocks - seen : 0u;
        cnt = min(RUN, max(RUN_MIN, rem / (2u * gridDim.x)));
        b0 = firstDyn + atomicAdd(queueHead, cnt);
      }
      b0 = __shfl(b0, 0, 64);
      cnt = __shfl(cnt, 0, 64);
    }
    // (wave-uniform, and said so: the run's bounds, the blocks' keys and the tile's base then live in scalar registers)
    b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
    cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt);
    firstItem = false;
    if (b0 >= nBlocks) break;
    const uint32_t b1 = min(nBlocks, b0 + cnt);
    for (uint32_t bi = b0; bi < b1; ++bi) {
      const uint32_t setBase = sortedKey[bi];
      [[maybe_unused]] const unsigned long long c0 = BTICK(), dr0 = bt[2];
      if (setBase != curBase) {
        flushTile();
        curBase = setBase;
        curNb = min((uint32_t)B, a.nsets - setBase);
        loadTileRays<B>(a, s, setBase, curNb, lane);
        for (int idx = lane; idx < 27 * B; idx += 64) (&s.acc[0][0])[idx] = 0.0;
        relToBase<B>(s, lane);
        __syncthreads();
      }
      [[maybe_unused]] const unsigned long long c1 = BTICK();
      bt[3] += (c1 - c0) - (bt[2] - dr0);
      const uint2 e = pairs[(size_t)sortedBlock[bi] * 64u + lane];
      const bool live = e.x != 0xFFFFFFFFu && e.y >= setBase && e.y - setBase < curNb;
      const uint32_t bIdx = e.y - setBase;
      BeamP1 st;
      const bool alive = live && beamBase<B>(a, s, e.x, bIdx, st);
      if (alive && st.st != 0xFFu) nEval++;  // (debugShift mismatch: base contribution kept, not an evaluation -- as the reference returns)
#ifdef GVPM_EVAL_TIMING
      asm volatile("" :: "v"((int)alive));
      const unsigned long long c2 = BTICK();
      bt[0] += c2 - c1;
      bt[4] += 1;
      bt[5] += (unsigned long long)__popcll(__ballot(alive));
#endif
      // (primal: the sppm integrator's beam pass -- BeamRadianceQuery, pm/beams.h:29-223 -- is the kernel record's base term
      // alone: no shifts.  cfg.reserved[5], set by gvpm_gather_primal's driver)
      const bool primal = a.cfg.reserved[5] != 0;
#pragma unroll 1
      for (int i = 0; i < 4; ++i) {
        bool rec = false;
        if (alive && !primal) beamShift1<B, HS>(a, s, st, bIdx, i, rec, nNull, nFail, setBase);
        const unsigned long long m = __ballot(rec);
        if (rec) {
          const uint32_t slot = qCount + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
          s.qid[slot] = st.id;
          s.qmeta[slot] = bIdx | ((uint32_t)i << 8);
          // base.eye * k.contrib * weightKernel * rr = (base.eye * flux * sigS) * (sc * weightKernel * rr): the scalar is carried
          s.qk[slot] = make_float4(st.k.tauV, st.k.sigmaW, st.k.pdfEdgeFailure * st.k.pdfKernel, st.k.sc * st.k.weightKernel * st.rr);
          s.qu[slot] = st.k.u;
        }
        qCount += (uint32_t)__popcll(m);
      }
#ifdef GVPM_EVAL_TIMING
      bt[1] += BTICK() - c2;
#endif
      while (qCount >= 64u) drain(64u);
    }
    {
      [[maybe_unused]] const unsigned long long f0 = BTICK(), dr0 = bt[2];
      flushTile();
      bt[3] += (BTICK() - f0) - (bt[2] - dr0);
    }
    curBase = 0xFFFFFFFFu;
  }
#ifdef GVPM_EVAL_TIMING
  bt[7] = BTICK() - btStart;
  if (lane == 0 && blockIdx.x < 16384u)
    for (int k = 0; k < 8; ++k) gvpmBeamsLog[8 * blockIdx.x + k] = bt[k];
#endif
  {
    unsigned long long ev = nEval, nu = nNull, di = nDiff, fa = nFail;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ev += __shfl_xor(ev, o, 64);
      nu += __shfl_xor(nu, o, 64);
      di += __shfl_xor(di, o, 64);
      fa += __shfl_xor(fa, o, 64);
    }
    if (lane == 0 && ev) {
      atomicAdd(&statRow(a)[0], ev);
      atomicAdd(&statRow(a)[2], nu);
      atomicAdd(&statRow(a)[3], di);
      atomicAdd(&statRow(a)[4], fa);
    }
  }
}

// the literal fp64 evaluation, below
void launch_evaluate_beams_exact(const GatherArgs &a, int beamsPerWave, const uint2 *pairs, const uint32_t *sortedKey,
                                 const uint32_t *sortedBlock, uint32_t nBlocks, uint32_t *queueHead, uint32_t nwaves,
                                 hipStream_t stream);

void launch_evaluate_beams(const GatherArgs &a, int beamsPerWave, bool exact, const uint2 *pairs, const uint32_t *sortedKey,
                           const uint32_t *sortedBlock, uint32_t nBlocks, uint32_t *queueHead, uint32_t nwaves,
                           hipStream_t stream) {
  if (a.nsets == 0 || nBlocks == 0) return;
  if (exact) {
    launch_evaluate_beams_exact(a, beamsPerWave, pairs, sortedKey, sortedBlock, nBlocks, queueHead, nwaves, stream);
    return;
  }
  const size_t dyn = a.ntri <= BEAM_LDS_TRIS ? (size_t)a.ntri * 48u : 0u;
  forBeamsPerWave(beamsPerWave, [&](auto b) {
    constexpr int B = decltype(b)::value;
    // manifold-typed shifts go to the host's request list (an instantiation of its own: the default keeps its registers)
    if (a.reqHost)
      hipLaunchKernelGGL((evaluate_beams2_kernel<B, true>), dim3(nwaves), dim3(64), dyn, stream, a, pairs, sortedKey, sortedBlock,
                         nBlocks, queueHead);
    else
      hipLaunchKernelGGL((evaluate_beams2_kernel<B>), dim3(nwaves), dim3(64), dyn, stream, a, pairs, sortedKey, sortedBlock,
                         nBlocks, queueHead);
  });
}

// ---- evaluation, literal fp64 path (GVPM_BEAMS_FP64=1: the on-device cross-check) ------------------------------
// One pair per lane, blocks of 64 pairs of one tile.  The block's camera-beam sets (at most B consecutive sorted
// sets) are loaded into LDS, the lanes evaluate their pairs (evaluateBeam: the reference transcribed in fp64) into
// the block's LDS accumulators, and the touched accumulators go to the film with one global atomic each.
// The blocks arrive sorted by tile (radix sort of the block keys on the host side of the launch), and a wave takes
// RUN consecutive blocks at a time: the tile's rays are loaded, the accumulators zeroed and flushed once per tile
// and run instead of once per block (that bookkeeping was 3.2 of the kernel's 5.9 ms at the probe).
template <int B>
__global__ __launch_bounds__(64, 1) void evaluate_beams_exact_kernel(GatherArgs a, const uint2 *__restrict__ pairs,
                                                                     const uint32_t *__restrict__ sortedKey,
                                                                     const uint32_t *__restrict__ sortedBlock,
                                                                     uint32_t nBlocks, uint32_t *queueHead) {
  constexpr uint32_t RUN = GVPM_BEAMS_RUN, RUN_MIN = GVPM_BEAMS_RUN_MIN;
  __shared__ TileLds<B> s;
  const int lane = threadIdx.x;
  uint32_t nEval = 0, nNull = 0, nDiff = 0, nFail = 0;
  uint32_t curBase = 0xFFFFFFFFu, curNb = 0;
  auto flushTile = [&]() __attribute__((always_inline)) {
    __syncthreads();
    if (curBase != 0xFFFFFFFFu) {
      for (int idx = lane; idx < 27 * B; idx += 64) {
        const int k = idx / B, bb = idx % B;
        if ((uint32_t)bb < curNb) {
          const float v = (float)s.acc[k][bb];
          if (v != 0.f) {
            const uint32_t pv = s.pix[bb];
            const size_t p = (size_t)(pv >> 16) * a.cfg.width + (pv & 0xFFFFu);
            atomicAdd(&a.iter[p * 27 + k], v);
          }
        }
      }
    }
    __syncthreads();
  };
  // the first item of every wave is its own index; the shared counter (one address: ~11 ns per atomic whatever the
  // number of waves) serves the rest
  // (guided runs of blocks, as in evaluate_beams2_kernel above)
  bool firstItem = true;
  const uint32_t run0 = min(RUN, max(RUN_MIN, nBlocks / (4u * gridDim.x)));  // the first run of every wave is its own
  const uint32_t firstDyn = gridDim.x * run0;
  for (;;) {
    uint32_t b0 = blockIdx.x * run0, cnt = run0;
    if (!firstItem) {
      if (lane == 0) {
        const uint32_t seen = firstDyn + __hip_atomic_load(queueHead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t rem = seen < nBlocks ? nBlocks - seen : 0u;
        cnt = min(RUN, max(RUN_MIN, rem / (2u * gridDim.x)));
        b0 = firstDyn + atomicAdd(queueHead, cnt);
      }
      b0 = __shfl(b0, 0, 64);
      cnt = __shfl(cnt, 0, 64);
    }
    firstItem = false;
    if (b0 >= nBlocks) break;
    const uint32_t b1 = min(nBlocks, b0 + cnt);
    for (uint32_t bi = b0; bi < b1; ++bi) {
      const uint32_t setBase = sortedKey[bi];
      if (setBase != curBase) {
        flushTile();
        curBase = setBase;
        curNb = min((uint32_t)B, a.nsets - setBase);
        loadTileRays<B>(a, s, setBase, curNb, lane);
        for (int idx = lane; idx < 27 * B; idx += 64) (&s.acc[0][0])[idx] = 0.0;
        __syncthreads();
      }
      const uint2 e = pairs[(size_t)sortedBlock[bi] * 64u + lane];
      const bool live = e.x != 0xFFFFFFFFu && e.y >= setBase && e.y - setBase < curNb;
      if (live) {
        // (EXV: the shadow segments through anyHitExact, every triangle test in fp64 as the exact pass takes them.  With the plain
        // fp32 test the cross-check was literal only where no parent self-hits: in a room 256 wide 1400 from the origin, Epsilon
        // at the ulp of a coordinate, 34 of 145 000 shifts went the other way -- found by the `centimetres` transform,
        // tests/test_similarity_gpu.py)
        if (evaluateBeam<B, true>(a, s, e.x, e.y - setBase, nNull, nDiff, nFail)) nEval++;
      }
    }
    flushTile();
    curBase = 0xFFFFFFFFu;
  }
  {
    unsigned long long ev = nEval, nu = nNull, di = nDiff, fa = nFail;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ev += __shfl_xor(ev, o, 64);
      nu += __shfl_xor(nu, o, 64);
      di += __shfl_xor(di, o, 64);
      fa += __shfl_xor(fa, o, 64);
    }
    if (lane == 0 && ev) {
      atomicAdd(&statRow(a)[0], ev);
      atomicAdd(&statRow(a)[2], nu);
      atomicAdd(&statRow(a)[3], di);
      atomicAdd(&statRow(a)[4], fa);
    }
  }
}

// (the `exact` branch of launch_evaluate_beams, which has returned already for an empty list)
void launch_evaluate_beams_exact(const GatherArgs &a, int beamsPerWave, const uint2 *pairs, const uint32_t *sortedKey,
                                 const uint32_t *sortedBlock, uint32_t nBlocks, uint32_t *queueHead, uint32_t nwaves,
                                 hipStream_t stream) {
  forBeamsPerWave(beamsPerWave, [&](auto b) {
    hipLaunchKernelGGL((evaluate_beams_exact_kernel<decltype(b)::value>), dim3(nwaves), dim3(64), 0, stream, a, pairs, sortedKey,
                       sortedBlock, nBlocks, queueHead);
  });
}

// ---- the exact pass of G-Beams (round 5) ------------------------------------------------------------------------------------
// The shifts the fp32 evaluation could not decide (beamShift1 / beamShift2: a decision inside its band) were noted --
// {beam set, beam | sub << 24, GVPM_EX_KIND_BEAMS | shift << 8 | cause << 16} in a.exOvf -- and added nothing.  This kernel
// runs BEHIND the evaluation on the same stream, every gather (the beams' build is not pipelined: nothing the notes refer to
// has moved): a lane per note, the reference's statements in fp64 (evaluateBeam, beams_eval_f64.h, with the triangle tests of the shadow
// segment in fp64 too), the shift's terms to the iteration's sums, its counter to the statistics.  A lane's rays and sums
// live in ITS column of a 64-wide tile.
__global__ __launch_bounds__(64) void exact_beams_kernel(GatherArgs a, unsigned long long *totals) {
  __shared__ TileLds<64> s;
  const int lane = threadIdx.x;
  const uint32_t total = *a.exOvfCount, n = min(total, a.exOvfCap);
  uint32_t nNull = 0, nDiff = 0, nFail = 0;
  for (uint32_t j0 = blockIdx.x * 64u; j0 < n; j0 += gridDim.x * 64u) {
    const uint32_t j = j0 + (uint32_t)lane;
    const bool have = j < n;
    const uint4 note = have ? a.exOvf[j] : make_uint4(0u, 0u, 0u, 0u);
    uint32_t pix = 0u;
    for (int k = 0; k < 5; ++k) {
      float4 q0 = make_float4(0.f, 0.f, 0.f, -1e-30f), q1 = make_float4(0.f, 0.f, 1.f, 0.f), q2 = make_float4(0.f, 0.f, 0.f, 0.f),
             q3 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (have) {
        const gvpm_camera_ray *ray = a.rays + (size_t)note.x * 5 + k;
        const float4 *rp = reinterpret_cast<const float4 *>(ray);
        q0 = rp[0]; q1 = rp[1]; q2 = rp[2]; q3 = rp[3];
        const float l = fabsf(q0.w);
        q0.w = GVPM_RAY_VALID(ray->info) != 0 ? l : -fmaxf(l, 1e-30f);  // (the valid bit rides on the sign of len, tile_walk.h)
      }
      s.ray4[k][0][lane] = q0;
      s.ray4[k][1][lane] = q1;
      s.ray4[k][2][lane] = q2;
      s.gop[k][lane] = q3.x;
      if (k == 0) {
        s.rnd[lane] = q3.z;
        s.pix[lane] = pix = __float_as_uint(q3.w);
        s.edge[lane] = GVPM_RAY_EDGE(__float_as_uint(q3.y));
      }
    }
    for (int k = 0; k < 27; ++k) s.acc[k][lane] = 0.0;
    __syncthreads();
    if (have) {
      if (totals) atomicAdd(&totals[4 + min((note.z >> 16) & 0xFFu, 15u)], 1ull);
      evaluateBeam<64, true>(a, s, note.y, (uint32_t)lane, nNull, nDiff, nFail, (int)((note.z >> 8) & 0xFFu));
      const size_t p = (size_t)(pix >> 16) * a.cfg.width + (pix & 0xFFFFu);
      for (int k = 3; k < 27; ++k) {
        const float v = (float)s.acc[k][lane];
        if (v != 0.f) atomicAdd(&a.iter[p * 27 + k], v);
      }
    }
    __syncthreads();
  }
  if (nNull) atomicAdd(&statRow(a)[2], (unsigned long long)nNull);
  if (nDiff) atomicAdd(&statRow(a)[3], (unsigned long long)nDiff);
  if (nFail) atomicAdd(&statRow(a)[4], (unsigned long long)nFail);
}
// the list is empty again; totals: {evaluated, lost, largest list} as exact_pass_kernel keeps them (exact_shift.hip)
__global__ void exact_beams_done_kernel(GatherArgs a, unsigned long long *totals) {
  const uint32_t total = *a.exOvfCount, n = min(total, a.exOvfCap);
  if (totals) {
    totals[0] += n;
    if (total > n) totals[1] += total - n;
    if (totals[2] < total) totals[2] = total;
  }
  if (total > n) atomicAdd(&a.stats[7], (unsigned long long)(total - n));  // dropped (gvpm_stats::dropped_pairs): gvpm_get_stats fails
  *a.exOvfCount = 0u;
}
void launch_exact_beams(const GatherArgs &a, unsigned long long *totals, hipStream_t stream) {
  // (a wave per workgroup, 37 KB of LDS each: four per CU resident; the empty ones leave at once)
  hipLaunchKernelGGL(exact_beams_kernel, dim3(2048), dim3(64), 0, stream, a, totals);
  hipLaunchKernelGGL(exact_beams_done_kernel, dim3(1), dim3(1), 0, stream, a, totals);
}

// ---- grid build helpers for sub-beams ------------------------------------------------------
// counts[i] = number of sub-beams of beam i; maxLs = longest sub-beam (float bits, atomicMax)
__global__ __launch_bounds__(256) void beam_subcount_kernel(const float *__restrict__ p2, const float *__restrict__ p1,
                                                            uint32_t n, float ls, uint32_t *counts, uint32_t *maxLs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  float sub = 0.f;
  if (i < n) {
    const double dx = (double)p2[3 * (size_t)i] - (double)p1[3 * (size_t)i];
    const double dy = (double)p2[3 * (size_t)i + 1] - (double)p1[3 * (size_t)i + 1];
    const double dz = (double)p2[3 * (size_t)i + 2] - (double)p1[3 * (size_t)i + 2];
    const float len = (float)sqrt(dx * dx + dy * dy + dz * dz);
    const uint32_t c = subBeamCount(len, ls);
    counts[i] = c;
    sub = len / (float)c;
  }
  sub = wave_max(sub);
  // (one address: atomics on it retire ~11 ns apart -- 31 k waves of them were 0.34 of this kernel's 0.36 ms -- so a wave
  // first looks whether it would raise the maximum at all)
  if ((threadIdx.x & 63) == 0 && __float_as_uint(sub) > __hip_atomic_load(maxLs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(maxLs, __float_as_uint(sub));
}

// for every sub-beam j = offsets[beam] + sub: keys[j] = the grid cell of its centre, vals[j] = beam | sub << 24 -- the pair
// the sort takes (until round 4: centres and ids written here, a key kernel over the centres, the sort carrying indices and
// sub_hot_kernel gathering ids[order[j]]: 16 bytes a sub-beam more traffic and one dependent gather more).
// A wave expands 64 beams TOGETHER: their sub-beams laid end to end, consecutive lanes take consecutive ones (the beam an
// element belongs to: a 6-step search over the wave's exclusive scan), so the stores are whole lines -- a lane looping over
// its own beam's ~12 sub-beams wrote 64 scattered pieces per instruction (0.25 ms at C3 for 0.2 GB).
__global__ __launch_bounds__(256) void beam_expand_kernel(const float *__restrict__ p2, const float *__restrict__ p1,
                                                          uint32_t n, const uint32_t *__restrict__ counts,
                                                          const uint32_t *__restrict__ offsets, Grid g, uint32_t *keys,
                                                          uint32_t *vals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool have = i < n;
  const uint32_t c = have ? counts[i] : 0u, o = have ? offsets[i] : 0u;
  const f3 a = have ? mk3(p1[3 * (size_t)i], p1[3 * (size_t)i + 1], p1[3 * (size_t)i + 2]) : mk3(0.f);
  const f3 b = have ? mk3(p2[3 * (size_t)i], p2[3 * (size_t)i + 1], p2[3 * (size_t)i + 2]) : mk3(0.f);
  const uint32_t incl = wave_scan_incl(c, lane), excl = incl - c;
  const uint32_t total = __shfl(incl, 63, 64);
  const uint32_t base = __shfl(o, 0, 64);  // (offsets are the exclusive scan of counts: the wave's elements are contiguous)
  for (uint32_t e0 = 0; e0 < total; e0 += 64u) {
    const uint32_t e = e0 + (uint32_t)lane;
    uint32_t r = 0;
#pragma unroll
    for (uint32_t step = 32; step; step >>= 1) {
      const uint32_t cand = r + step;
      const uint32_t v = (uint32_t)__shfl((int)excl, (int)(cand & 63u), 64);
      if (cand < 64u && v <= e) r = cand;
    }
    const uint32_t rc = (uint32_t)__shfl((int)c, (int)r, 64), rx = (uint32_t)__shfl((int)excl, (int)r, 64);
    const f3 ra = mk3(__shfl(a.x, (int)r, 64), __shfl(a.y, (int)r, 64), __shfl(a.z, (int)r, 64));
    const f3 rb = mk3(__shfl(b.x, (int)r, 64), __shfl(b.y, (int)r, 64), __shfl(b.z, (int)r, 64));
    if (e < total) {
      const uint32_t k = e - rx;
      const float t = ((float)k + 0.5f) / (float)rc;
      const f3 m = ra + (rb - ra) * t;
      const int cx = cellCoord(m.x, g.org[0], g.invCell, g.dim[0]);
      const int cy = cellCoord(m.y, g.org[1], g.invCell, g.dim[1]);
      const int cz = cellCoord(m.z, g.org[2], g.invCell, g.dim[2]);
      keys[base + e] = ((uint32_t)cz * g.dim[1] + cy) * g.dim[0] + cx;
      vals[base + e] = (blockIdx.x * blockDim.x + (threadIdx.x & ~63u) + r) | (k << 24);
    }
  }
}

// sorted sub-beam records for the traversal: {centre, beam | sub << 24} {beam direction, sub-beam length} and the
// beam's filter bits (cold word 7.w: contribution, parity, depth).  The length is the evaluation's (fp64 norm
// rounded to float), so that sub-beam ranges agree.
__global__ __launch_bounds__(256) void sub_hot_kernel(const uint32_t *__restrict__ sortedIds, uint32_t n,
                                                      const float4 *__restrict__ aux, float4 *hot, uint32_t *hotFlags) {
  // (the two quads of a record go through LDS: consecutive lanes then write consecutive quads -- whole lines -- instead
  // of every lane its two halves of a 32-byte record)
  __shared__ float4 stg[256][2];
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = threadIdx.x;
  if (j < n) {
    const uint32_t id = sortedIds[j], beam = id & 0xFFFFFFu, sub = id >> 24;
    // {p1, bits} {direction, sub-beam length} of the beam (beam_cold_kernel): one 32-byte gather; the centre is computed,
    // not gathered (to a few ulp the one beam_expand_kernel binned: every test downstream carries a margin)
    const float4 a0 = aux[2 * (size_t)beam], a1 = aux[2 * (size_t)beam + 1];
    const float tt = a1.w * ((float)sub + 0.5f);
    stg[t][0] = make_float4(a0.x + a1.x * tt, a0.y + a1.y * tt, a0.z + a1.z * tt, __uint_as_float(id));
    stg[t][1] = a1;
    hotFlags[j] = __float_as_uint(a0.w);
  }
  __syncthreads();
  const size_t base = 2 * (size_t)blockIdx.x * blockDim.x;
  const float4 *flat = &stg[0][0];
#pragma unroll
  for (int e = t; e < 512; e += 256)
    if (base + (size_t)e < 2 * (size_t)n) hot[base + e] = flat[e];
}

void launch_beam_subcount(const float *p2, const float *p1, uint32_t n, float ls, uint32_t *counts, uint32_t *maxLs,
                          hipStream_t s) {
  hipLaunchKernelGGL(beam_subcount_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p2, p1, n, ls, counts, maxLs);
}
void launch_beam_expand(const float *p2, const float *p1, uint32_t n, const uint32_t *counts, const uint32_t *offsets,
                        const Grid &g, uint32_t *keys, uint32_t *vals, hipStream_t s) {
  hipLaunchKernelGGL(beam_expand_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p2, p1, n, counts, offsets, g, keys, vals);
}
void launch_sub_hot(const uint32_t *sortedIds, uint32_t n, const float4 *aux, float4 *hot, uint32_t *hotFlags, hipStream_t s) {
  hipLaunchKernelGGL(sub_hot_kernel, dim3((n + 255) / 256), dim3(256), 0, s, sortedIds, n, aux, hot, hotFlags);
}

}  // namespace gvpm
