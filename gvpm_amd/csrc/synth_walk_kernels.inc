// The device generators' light-path walk kernel, written once and compiled by two units: synth_device.hip (the closed set Lambertian /
// index-matched / mirror, GVPM_SYNTH_GLOSSY 0 in its device pass) and synth_device_glossy.hip (every material of the host walk).  The
// including unit defines GVPM_SYNTH_K(name): the kernels' and launchers' names in that unit.  Each unit is a code object of its own
// (no relocatable device code), so one instantiation costs the other nothing (host/synth_core.h, at MatKind).
namespace gvpm {
namespace {

// the sinks of flattenPath / flattenBeams (synth_core.h): the count pass keeps a number, the write pass stores each record
// where it belongs -- neither holds the path's records in (scratch) memory
struct CountSink {
  int n;
  __device__ CountSink() : n(0) {}
  __device__ void clear() { n = 0; }
  __device__ bool empty() const { return n == 0; }
  __device__ void push_back(const PhotonRec &) {
    if (n < GVPM_SYNTH_MAXV) ++n;
  }
};
// The walk runs ONCE (round 3; it ran twice: count, then write): its records are parked at a slot that depends on the path
// alone -- path k, record n at (k * stride + n) -- and a copy kernel moves them to their place in the output once the
// scans have said where that is.  32 words a record; with 288 GB of HBM the 1-2 GB of parking space are affordable, a
// second walk of 0.85 M light paths in fp64 (1.5 ms) was not.
struct ParkSink {
  float *park;  // this path's slots
  int n, stride;
  __device__ void clear() { n = 0; }
  __device__ bool empty() const { return n == 0; }
  __device__ void push_back(const PhotonRec &r) {
    if (n >= stride) return;
    float *d = park + (size_t)n * PARK_WORDS;
    ++n;
    const V3 v[9] = {r.pos, r.wi, r.flux, r.parentPos, r.parentN, r.prefixW, r.parentScat, r.parentWi, r.endN};
#pragma unroll
    for (int a = 0; a < 9; ++a) {
      d[3 * a] = (float)v[a].x;
      d[3 * a + 1] = (float)v[a].y;
      d[3 * a + 2] = (float)v[a].z;
    }
    d[27] = r.parentPdf;
    d[28] = r.edgePdf;
    d[29] = r.parentRR;
    d[30] = r.parentG;
    d[31] = __uint_as_float(r.flags);
  }
};

// A wave owns `chunk` consecutive paths of the batch and its lanes REFILL: a lane whose path has ended takes the wave's next
// path while its neighbours walk on (walkBegin / walkStep, synth_core.h).  With one path per lane a wave ran until its
// longest path ended -- twelve bounces with the mean near five: less than half of the lane-steps did work.  Where a path's
// records are parked depends on the path alone, so which lane walks it changes nothing.
template <bool BEAMS>
__device__ __forceinline__ void walkChunk(const SceneView &sc, int iteration, uint64_t base, uint32_t k0, uint32_t k1, float *park,
                                          int stride, uint32_t *counts, uint32_t *counted, uint32_t *nonEmpty) {
  const int lane = threadIdx.x & 63;
  ParkSink recs;
  recs.park = park;
  recs.stride = stride;
  recs.n = 0;
  StreamPath<ParkSink, BEAMS> path(sc, recs);
  Philox rng(sc.seed, 0x11ffu, (uint32_t)iteration, 0u, 0u);
  V3 throughput(1.0);
  uint32_t next = k0;  // wave-uniform
  uint32_t k = 0;
  int i = 0;
  bool active = false;
  for (;;) {
    // refill: the idle lanes take the next paths, in lane order
    const unsigned long long idle = __ballot(!active);
    if (idle && next < k1) {
      const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
      if (!active && next + rank < k1) {
        k = next + rank;
        const uint64_t idx = base + k;
        rng = Philox(sc.seed, 0x11ffu, (uint32_t)iteration, (uint32_t)idx, (uint32_t)(idx >> 32));
        recs.park = park + (size_t)k * stride * PARK_WORDS;
        walkBegin(sc, rng, path, throughput);
        i = 1;
        active = true;
      }
      next = min(k1, next + (uint32_t)__popcll(idle));
    }
    if (!__ballot(active)) break;
    if (active) {
      if (i >= sc.maxDepth || !walkStep(sc, rng, path, throughput, i)) {
        const bool c = path.finish();
        counts[k] = (uint32_t)recs.n;
        counted[k] = c ? 1u : 0u;
        nonEmpty[k] = recs.n ? 1u : 0u;
        active = false;
      } else {
        ++i;
      }
    }
  }
}

__global__ __launch_bounds__(64) void GVPM_SYNTH_K(synth_walk_kernel)(SceneView sc, int iteration, uint64_t base, uint32_t m, uint32_t chunk, int beams,
                                                        float *park, int stride, uint32_t *counts, uint32_t *counted,
                                                        uint32_t *nonEmpty) {
  const uint32_t k0 = blockIdx.x * chunk;
  if (k0 >= m) return;
  const uint32_t k1 = min(m, k0 + chunk);
  if (beams) walkChunk<true>(sc, iteration, base, k0, k1, park, stride, counts, counted, nonEmpty);
  else walkChunk<false>(sc, iteration, base, k0, k1, park, stride, counts, counted, nonEmpty);
}

}  // namespace

// the launcher synth_device.hip's drivers call (synth_device_launch.h)
void GVPM_SYNTH_K(synthLaunchWalk)(hipStream_t s, unsigned nb, const SceneView &sc, int iteration, uint64_t base, uint32_t m, uint32_t chunk,
                                   int beams, float *park, int stride, uint32_t *counts, uint32_t *counted, uint32_t *nonEmpty) {
  hipLaunchKernelGGL(GVPM_SYNTH_K(synth_walk_kernel), dim3(nb), dim3(64), 0, s, sc, iteration, base, m, chunk, beams, park, stride, counts,
                     counted, nonEmpty);
}

}  // namespace gvpm
