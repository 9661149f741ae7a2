// G-Beams traversal for gfx950, hand-written HIP: the (camera ray, sub-beam) pair list.
//
// Replaces, for one SPPM iteration, the query of
//   SubBeamBVH (build + query)                    pm/beams_accel.h:82-267
// (pm/ = src/integrators/photonmapper/).
//
// Acceleration structure: like the reference, every photon beam is cut into sub-beams (here of
// about one grid cell) and each sub-beam is binned ONCE, by its centre, into the same sorted
// uniform grid the photon kernels use; the camera tile walks the grid with the kernel radius
// inflated by half a sub-beam.  A (camera ray, beam) pair is evaluated by the one sub-beam that
// owns the intersection -- the reference's own rule (1D: v in (t1,t2], beams_struct.h:297-299;
// 3D: tNear in (t1,t2), shift_volume_beams.h:213-220) -- so the result does not depend on how
// beams are cut.  Traversal, LDS staging, ballot compaction and the work queue are those of the
// BRE kernel (tile_walk.h).  The sub-beams are cut and keyed by gather_beams.hip (beam_subcount_kernel,
// beam_expand_kernel, sub_hot_kernel), which also evaluates the pairs (or gather_beams_split.hip does); this unit needs nothing
// of either evaluation.
#include <hip/hip_runtime.h>

#include "beams_common.h"
#include "device_types.h"
#include "shift_device.h"
#include "tile_walk.h"
#include "vec.h"

#ifndef GVPM_BSTAGE
#define GVPM_BSTAGE 128
#endif

namespace gvpm {

// ---- traversal: (camera ray, sub-beam) pairs that survive the sphere test and the fp32 prefilter ---------------
// Persistent waves over the planner's items (tile_walk.h), built like the BRE traversal: the sub-beam records of a
// slab box -- {centre, beam | sub << 24} {direction, sub-beam length} + the beam's filter bits, 36 bytes -- are
// staged in LDS; every lane (ray b = lane % B, slot = lane / B) sphere-tests G staged records branch-free, then the
// wave resolves the marked ones one per lane and round: flag filters (contribution, checkerboard parity, depth) and
// the ownership prefilter, straight from LDS and the lane's own ray registers.  Survivors are compacted by ballot
// into an LDS ring and appended to the global pair list 64 at a time (one atomic per 64 pairs; the tail of an item
// is padded with empty pairs so that a block of 64 never mixes tiles).  pair = {beam | sub << 24, sorted set index}.
// (a stage of 128: the one-layer slab boxes hold ~100 sub-beams, and 6 KB of LDS per wave instead of 10 leaves room
// for more resident waves, which is what hides the per-slab latency chain)
constexpr int BSTAGE = GVPM_BSTAGE;
constexpr int BCQ = 512;  // sphere-test survivors waiting for the prefilter (a group adds at most 4 x 64, 63 wait; power of 2)
typedef float v2fb __attribute__((ext_vector_type(2)));
struct alignas(16) BeamTravLds {
  float4 st0[BSTAGE], st1[BSTAGE];
  // the centres and the filter bits once more, one array per component: the sphere test reads FOUR consecutive staged
  // sub-beams with four ds_read_b128 issued together and tests two at a time in packed fp32 (as the G-BRE traversal)
  float sx[BSTAGE], sy[BSTAGE], sz[BSTAGE];
  uint32_t stF[BSTAGE];
  uint2 outq[QCAP];
  float4 rayO[64], rayD[64];  // the tile's base rays {o, len} {d, -}: a candidate is resolved by ANY lane
  uint16_t candq[BCQ];        // staged record | ray << 8
};

#ifdef GVPM_TRAV_TIMING
// probe builds only: per wave of the last launch {start, end (wall clock, 100 MHz), items, candidates}
__device__ unsigned long long gvpmBeamTravLog[4 * 8192];
extern "C" int gvpm_debug_beamtrav_timing(unsigned long long *out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(gvpmBeamTravLog), sizeof(gvpmBeamTravLog)) == hipSuccess ? 0 : -1;
}
#endif
template <int B>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void traverse_beams_kernel(GatherArgs a, const uint32_t *__restrict__ hotFlags,
                                                            const uint4 *__restrict__ items,
                                                            const uint32_t *__restrict__ itemCount, uint32_t itemCap, uint32_t *queueHead,
                                                            uint2 *__restrict__ pairs, uint32_t *pairCount,
                                                            uint32_t pairCap, uint32_t *__restrict__ blockKey,
                                                            uint32_t *__restrict__ blockVal) {
  constexpr int LPB = 64 / B;
  __shared__ BeamTravLds s;
  const int lane = threadIdx.x;
  const int technique = a.cfg.vol_technique;
  // (the planner counts the items it had no room to write: never read past the list; the host regrows it and repeats)
  const uint32_t nItems = min(*itemCount, itemCap);
  const int b = lane % B, sub = lane / B;
  const float rT = a.radius;  // test radius = kernel radius + half a sub-beam
  const float r = a.kernelRadius;
  const float eps = a.cfg.epsilon;
  const bool pathSet = a.cfg.path_set != 0;
  const int maxDepth = a.cfg.max_depth;
  unsigned long long nCand = 0;
#ifdef GVPM_TRAV_TIMING
  const unsigned long long tw0 = wall_clock64();
  unsigned long long nIt = 0;
#endif
  // Blocks of the pair list are reserved RESERVE at a time: atomics on one address retire at ~11 ns each on this
  // part whatever the number of waves (scripts/probes/atomics_bench.hip), so one atomic per block (~260 k per pass)
  // bounded the kernel at 3 ms.  What a wave has left over at the end is written as empty blocks of its last tile.
  constexpr uint32_t RESERVE = 8u;
  uint32_t resSlot = 0, resLeft = 0, lastSet = 0;

  // the first item of every wave is its own index; the shared counter (one address: ~11 ns per atomic whatever the
  // number of waves) serves the rest
  bool firstItem = true;
  for (;;) {
    uint32_t it = blockIdx.x;
    if (!firstItem) {
      if (lane == 0) it = gridDim.x + atomicAdd(queueHead, 1u);
      it = __shfl(it, 0, 64);
    }
    firstItem = false;
    it = (uint32_t)__builtin_amdgcn_readfirstlane((int)it);  // (wave-uniform: the item's record in scalar registers)
    if (it >= nItems) break;
#ifdef GVPM_TRAV_TIMING
    nIt++;
#endif
    const uint4 item = items[it];
    // a heavy item comes as `parts` items that take its staging windows round-robin (plan_kernel)
    const uint32_t setBase = item.x, nb = item.y & 0xFFu, part = (item.y >> 8) & 0xFFFu, parts = max(item.y >> 20, 1u);
    if (nb == 0) continue;
    uint32_t winIdx = 0;  // staging windows of the item so far (wave-uniform)
    BaseInfo bi;
    const RayReg base = loadBaseDirect<B>(a, setBase, nb, lane, bi);
    TileWalk w;
    tileSetupFrom(a, base, base.valid, w);
    const bool beamValid = w.beamValid;
    const float mint = eps, maxt = base.len - eps;
    const uint32_t pixParity = ((bi.pix & 0xFFFFu) + (bi.pix >> 16)) & 1u;
    const int edge = (int)bi.edge;
    // the sphere test's thresholds (an invalid beam set passes nothing) and filter words
    // (plus the fp32 error of the test itself, bounded as in the G-BRE traversal by the beam's own length: a centre that
    // passes the exact test lies within rT of the segment)
    const float eT = 1.25e-6f * 1.7321f * (fmaxf(base.len, 0.f) + 3.f * rT);
    const float thrD2 = beamValid ? rT * rT * 1.001f + 4.f * rT * eT : -1.f, thrLo = mint - rT * 1.001f - eT,
                thrHi = maxt + rT * 1.001f + eT;
    const uint32_t fmask = 0x40u | (pathSet ? (1u << GVPM_HOT_PARITY_BIT) : 0u);
    const uint32_t fwant = 0x40u | (pathSet ? (pixParity << GVPM_HOT_PARITY_BIT) : 0u);
    const int dmaxB = maxDepth - edge;
    // the tile's bounding cylinder (tile_walk.h tileCylinder; round 3): sub-beams whose centre lies outside it are not
    // staged at all -- the box of a slab step holds about three times the centres any of the tile's rays can accept
    const bool prefilter = !(a.cfg.reserved[0] & 128);
    TileCyl cyl;
    cyl.ok = false;
    if (prefilter) cyl = tileCylinder(base, beamValid, fminf(thrLo, 0.f) - rT, thrHi + rT, rT * 1.0005f, 2.f * eT);
    const bool haveCyl = prefilter && __builtin_amdgcn_readfirstlane((int)cyl.ok);
    uint32_t qHead = 0, qCount = 0;
    auto emit = [&](uint32_t n) __attribute__((always_inline)) {  // n <= 64 pairs of the ring -> one block of 64 in the global list
      if (resLeft == 0u) {
        if (lane == 0) resSlot = atomicAdd(pairCount, 64u * RESERVE);
        resSlot = __shfl(resSlot, 0, 64);
        resLeft = RESERVE;
      }
      const uint32_t slot = resSlot;
      resSlot += 64u;
      resLeft--;
      lastSet = setBase;
      const uint2 e = (uint32_t)lane < n ? s.outq[(qHead + lane) % QCAP] : make_uint2(0xFFFFFFFFu, 0u);
      if (slot + 64u <= pairCap) {  // past the capacity: counted, not written (host regrows)
        pairs[slot + lane] = e;
        if (lane == 0) {
          // the block's tile (first sorted set of its item): the evaluation takes the blocks tile by tile
          blockKey[slot / 64u] = setBase;
          blockVal[slot / 64u] = slot / 64u;
        }
      }
      qHead = (qHead + n) % QCAP;
      qCount -= n;
    };
    __syncthreads();
    if (sub == 0) {
      s.rayO[b] = make_float4(base.o.x, base.o.y, base.o.z, base.len);
      s.rayD[b] = make_float4(base.d.x, base.d.y, base.d.z, 0.f);
    }
    __syncthreads();
    uint32_t cHead = 0, cCount = 0;  // candidate ring, wave-uniform
    auto resolve = [&](uint32_t n) __attribute__((always_inline)) {  // n <= 64 candidates: ownership prefilter, survivors -> the pair ring
      __syncthreads();
      bool keep = false;
      uint32_t id = 0, rb = 0;
      if ((uint32_t)lane < n) {
        const uint32_t c = s.candq[(cHead + (uint32_t)lane) % BCQ];
        const uint32_t j = c & 0xFFu;
        rb = c >> 8;
        const float4 h0 = s.st0[j], h1 = s.st1[j], ro = s.rayO[rb], rd = s.rayD[rb];
        id = __float_as_uint(h0.w);
        RayReg ray;
        ray.o = mk3(ro.x, ro.y, ro.z);
        ray.d = mk3(rd.x, rd.y, rd.z);
        ray.len = ro.w;
        keep = beamPrefilter(ray, mk3(h0.x, h0.y, h0.z), mk3(h1.x, h1.y, h1.z), h1.w, id >> 24, r, eps, technique);
      }
      nCand += n;
      cHead = (cHead + n) % BCQ;
      cCount -= n;
      const unsigned long long km = __ballot(keep);
      if (km) {
        if (keep)
          s.outq[(qHead + qCount + (uint32_t)__popcll(km & ((1ull << lane) - 1ull))) % QCAP] = make_uint2(id, setBase + rb);
        qCount += (uint32_t)__popcll(km);
        if (qCount >= 64u) {
          __syncthreads();
          emit(64u);
          __syncthreads();
        }
      }
    };
    const int cBeg = max((int)item.z, w.cA0), cEnd = min((int)item.w, w.cA1);
    for (int cA = cBeg; cA <= cEnd; cA += w.K) {
      const int cAe = min(cA + w.K - 1, cEnd);
      CellBox bx;
      if (!slabBox(a, w, cA, cAe, bx)) continue;
      const int nranges = (bx.by1 - bx.by0 + 1) * (bx.bz1 - bx.bz0 + 1);
      for (int rbase = 0; rbase < nranges; rbase += 64) {
        uint32_t start, count;
        boxRange(a, bx, rbase + lane, nranges, start, count);
        const uint32_t incl = wave_scan_incl(count, lane);
        const uint32_t excl = incl - count;
        const uint32_t total = __shfl(incl, 63, 64);
        for (uint32_t win = 0; win < total; win += BSTAGE) {
          if (winIdx++ % parts != part) continue;
          __syncthreads();
          const uint32_t nwin = min((uint32_t)BSTAGE, total - win);
          // staged so far (wave-uniform): the window's entries inside the tile's cylinder whose beam contributes at all,
          // compacted -- and, with the checkerboard (pathSet), PARTITIONED by the beam's parity: parity 0 from slot 0 upwards,
          // parity 1 from the last slot downwards.  A ray only meets beams of its pixel's parity (shift_volume_beams.cpp:
          // 142-184), so its lanes walk their own half: half the sphere tests (round 4; the filter bits are still tested --
          // where the halves' last groups of 16 overlap, a lane reads entries of the other parity)
          uint32_t n0 = 0, n1 = 0;
          // Staging: entry k of the window is element win + k of the concatenated ranges.  Consecutive LANES take
          // consecutive entries (the range an entry falls in is found by a 6-step search over the exclusive scan,
          // through ds_bpermute), so a load instruction reads a few contiguous runs of records instead of 64
          // separate ones -- with ~80 sub-beams per range (C3: 47 M sub-beams) the per-lane copy loops had made the
          // staging alone 58 of the traversal's 104 ms.
#pragma unroll
          for (uint32_t k = (uint32_t)lane; k < (uint32_t)BSTAGE; k += 64u) {
            const uint32_t e = win + k;
            uint32_t rr = 0;
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1) {
              const uint32_t cand = rr + step;
              const uint32_t v = (uint32_t)__shfl((int)excl, (int)(cand & 63u), 64);
              if (v <= e) rr = cand;
            }
            const uint32_t rStart = (uint32_t)__shfl((int)start, (int)rr, 64), rExcl = (uint32_t)__shfl((int)excl, (int)rr, 64);
            const uint32_t gi = rStart + (e - rExcl);
            float4 c0 = make_float4(0.f, 0.f, 0.f, 0.f);
            uint32_t fl = 0;
            bool keep = k < nwin;
            if (keep) {
              c0 = a.hot[2 * (size_t)gi];
              fl = hotFlags[gi];
              keep = (fl & 0x40u) && (!haveCyl || insideCylinder(cyl, mk3(c0.x, c0.y, c0.z)));
            }
            const bool up = keep && pathSet && ((fl >> GVPM_HOT_PARITY_BIT) & 1u);
            const unsigned long long km = __ballot(keep), um = __ballot(up), lm = km & ~um;
            if (keep) {
              const unsigned long long below = (1ull << lane) - 1ull;
              const uint32_t dst = up ? (uint32_t)BSTAGE - 1u - n1 - (uint32_t)__popcll(um & below) : n0 + (uint32_t)__popcll(lm & below);
              s.st0[dst] = c0;
              s.st1[dst] = a.hot[2 * (size_t)gi + 1];
              s.sx[dst] = c0.x;
              s.sy[dst] = c0.y;
              s.sz[dst] = c0.z;
              s.stF[dst] = fl;
            }
            n0 += (uint32_t)__popcll(lm);
            n1 += (uint32_t)__popcll(um);
          }
          // the FREE slots up to each half's next multiple of 16 hold centres no ray can meet
          {
            const uint32_t free0 = n0, free1 = (uint32_t)BSTAGE - n1;  // the free slots: [free0, free1)
            const uint32_t lo = n0 + (uint32_t)lane, hi = free1 - 1u - (uint32_t)lane;
            if (lane < 16 && lo < ((n0 + 15u) & ~15u) && lo < free1) s.sx[lo] = 3.0e38f;
            if (lane < 16 && (uint32_t)lane < (((n1 + 15u) & ~15u) - n1) && free1 >= free0 + 1u + (uint32_t)lane) s.sx[hi] = 3.0e38f;
          }
          __syncthreads();
          constexpr uint32_t G = 4;
          static_assert(BSTAGE % (G * LPB) == 0, "a lane reads four consecutive staged sub-beams with one b128 per component");
          // (wave-uniform trip count: the longer half; a lane whose own half is exhausted marks nothing -- the slots it
          // reads then hold the other half or an earlier window)
          const uint32_t nmax = max(n0, n1);
          const bool upper = pathSet && pixParity != 0u;
          const uint32_t nMine = upper ? n1 : n0;
          for (uint32_t jb = 0; jb < nmax; jb += G * LPB) {
            const uint32_t j0 = (upper ? (uint32_t)BSTAGE - (uint32_t)(G * LPB) - jb : jb) + (uint32_t)sub * G;
            uint32_t cm = 0;
            if (jb < nMine)
            {
              const float4 X = *reinterpret_cast<const float4 *>(&s.sx[j0]);
              const float4 Y = *reinterpret_cast<const float4 *>(&s.sy[j0]);
              const float4 Z = *reinterpret_cast<const float4 *>(&s.sz[j0]);
              const uint4 Ft = *reinterpret_cast<const uint4 *>(&s.stF[j0]);
              const v2fb ox = {base.o.x, base.o.x}, oy = {base.o.y, base.o.y}, oz = {base.o.z, base.o.z};
              const v2fb dx = {base.d.x, base.d.x}, dy = {base.d.y, base.d.y}, dz = {base.d.z, base.d.z};
              const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
              const uint32_t fs[4] = {Ft.x, Ft.y, Ft.z, Ft.w};
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const v2fb wx = (v2fb){xs[2 * h], xs[2 * h + 1]} - ox, wy = (v2fb){ys[2 * h], ys[2 * h + 1]} - oy,
                           wz = (v2fb){zs[2 * h], zs[2 * h + 1]} - oz;
                const v2fb disk = wx * dx + (wy * dy + wz * dz);
                const v2fb vx = wx - dx * disk, vy = wy - dy * disk, vz = wz - dz * disk;
                const v2fb d2 = vx * vx + (vy * vy + vz * vz);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                  const int u = 2 * h + e;
                  // conservative: sub-beam centre within (kernel radius + half sub-beam) of the ray segment; the
                  // beam's filter bits (contribution, checkerboard parity, depth) are tested here too: they halve
                  // the pairs that reach the ownership prefilter
                  uint32_t ok = (uint32_t)(d2[e] < thrD2) & (uint32_t)(disk[e] > thrLo) & (uint32_t)(disk[e] < thrHi);
                  ok &= (uint32_t)((fs[u] & fmask) == fwant);
                  if (maxDepth > 0) ok &= (uint32_t)((int)GVPM_PF_DEPTH(fs[u]) <= dmaxB);
                  cm |= ok << u;
                }
              }
            }
            // the survivors (a few per cent of the tests, scattered over the lanes) are compacted into a candidate
            // ring and go through the ownership prefilter 64 at a time, one per lane whatever ray they belong to:
            // resolved in place -- every lane looping over its own marks -- a round ran the ~100 instructions of
            // the prefilter for the one lane in ten that had a mark
#pragma unroll
            for (uint32_t u = 0; u < G; ++u) {
              const bool bit = (cm >> u) & 1u;
              const unsigned long long m = __ballot(bit);
              if (bit)
                s.candq[(cHead + cCount + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))) % BCQ] =
                    (uint16_t)((j0 + u) | ((uint32_t)b << 8));
              cCount += (uint32_t)__popcll(m);
            }
            while (cCount >= 64u) resolve(64u);
          }
          // the stage is about to be overwritten: the candidates that refer to it go first
          while (cCount) resolve(min(cCount, 64u));
        }
      }
    }
    __syncthreads();
    if (qCount) emit(qCount);
    __syncthreads();
  }
  for (; resLeft; --resLeft, resSlot += 64u) {
    if (resSlot + 64u <= pairCap) {
      pairs[resSlot + lane] = make_uint2(0xFFFFFFFFu, 0u);
      if (lane == 0) {
        blockKey[resSlot / 64u] = lastSet;
        blockVal[resSlot / 64u] = resSlot / 64u;
      }
    }
  }
  if (lane == 0 && nCand) atomicAdd(&statRow(a)[1], nCand);
#ifdef GVPM_TRAV_TIMING
  if (lane == 0 && blockIdx.x < 8192u) {
    gvpmBeamTravLog[4 * blockIdx.x] = tw0;
    gvpmBeamTravLog[4 * blockIdx.x + 1] = wall_clock64();
    gvpmBeamTravLog[4 * blockIdx.x + 2] = nIt;
    gvpmBeamTravLog[4 * blockIdx.x + 3] = nCand;
  }
#endif
}

void launch_traverse_beams(const GatherArgs &a, const uint32_t *hotFlags, int beamsPerWave, const uint4 *items,
                           const uint32_t *itemCount, uint32_t itemCap, uint32_t *queueHead, uint2 *pairs, uint32_t *pairCount,
                           uint32_t pairCap, uint32_t *blockKey, uint32_t *blockVal, uint32_t nwaves, hipStream_t stream) {
  if (a.nsets == 0) return;
  forBeamsPerWave(beamsPerWave, [&](auto b) {
    hipLaunchKernelGGL(traverse_beams_kernel<decltype(b)::value>, dim3(nwaves), dim3(64), 0, stream, a, hotFlags, items, itemCount,
                       itemCap, queueHead, pairs, pairCount, pairCap, blockKey, blockVal);
  });
}

}  // namespace gvpm
