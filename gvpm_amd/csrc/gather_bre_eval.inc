// The G-BRE evaluation kernel, included by gather_bre_eval.hip once per form: GVPM_EVAL_KERNEL = its name, GVPM_EVAL_MIX = whether it
// evaluates mixture parents (GVPM_BSDF_MIXTURE; parent_bsdf.h, glossyParentEval<MIX>).  The text is the kernel's own, unchanged: as a
// __forceinline__ body shared by two __global__ wrappers every instantiation's assembly moved (NOTEBOOK.md, "Mixture parents").
// CFG (shift_device.h): EvalCfgGeneric reads the integrator configuration from a.cfg; a fixed one compiles its dead paths out.
template <int B, bool FULLVIS, bool PF, bool HS = false, typename CFG = EvalCfgGeneric>
__global__ __launch_bounds__(64 * SegCfg<B>::WPB, GVPM_EVAL_MINW * SegCfg<B>::WPB / 4 > 0 ? GVPM_EVAL_MINW * SegCfg<B>::WPB / 4 : 1) GVPM_EVAL_ATTR
void GVPM_EVAL_KERNEL(GatherArgs a, const uint4 *__restrict__ items, const uint2 *__restrict__ itemOff,
                             const uint32_t *__restrict__ itemCount, uint32_t *queueHead,
                             const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ pairCnt,
                             uint32_t persistent, const uint2 *__restrict__ units, const uint32_t *__restrict__ unitCtl,
                             uint32_t unitCap) {
  constexpr int WPB = SegCfg<B>::WPB;
  constexpr int BB = SegCfg<B>::BEAM_BITS;
  using Entry = typename SegCfg<B>::Entry;
  __shared__ SegLds<B> sAll[WPB];
  extern __shared__ float4 sceneTri[];  // the occluders of a small scene (48 bytes each), shared by the waves
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (itemCount[7] != 0u) return;  // (see traverse_bre_kernel)
  SegLds<B> &s = sAll[wv];
  const float4 *ldsTri = nullptr;
  if (!FULLVIS && a.ntri <= EVAL_LDS_TRIS && !(a.cfg.reserved[0] & 16)) {
    for (uint32_t i = threadIdx.x; i < 3u * a.ntri; i += 64u * WPB) sceneTri[i] = a.tri4[i];
    ldsTri = sceneTri;
  }
  __syncthreads();  // the only workgroup barrier: from here on the waves run independently
  const uint32_t nItems = *itemCount;
  const uint32_t waveId = blockIdx.x * WPB + wv, nWaves = gridDim.x * WPB;
  uint32_t nEval = 0, nNull = 0, nDiff = 0, nFail = 0;
  [[maybe_unused]] unsigned long long tk[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  [[maybe_unused]] const unsigned long long tStart = TICK();
  [[maybe_unused]] unsigned long long tItemMax = 0;
#ifdef GVPM_EVAL_TIMING
  const unsigned long long wStart = wall_clock64();
  unsigned long long wLastStart = 0, lastN = 0, lastUk = 0, wLastEnd = 0, tkLast[6] = {0, 0, 0, 0, 0, 0}, suLast[4] = {0, 0, 0, 0};
#endif

  // (Measured in round 6 and dropped, as round 3 had for whole items: asking the queue for the NEXT entry while the current one
  // is evaluated -- the returning atomic is a quarter of a unit's set-up -- leaves every wave sitting on a reserved unit when
  // the queue runs dry: single stream 0.593 -> 0.636 ms, the waves' end times 0.55-1.09 ms instead of 0.58-0.99.)
  bool firstItem = true;
  for (;;) {
    [[maybe_unused]] const unsigned long long tItem = TICK();
    uint32_t it = waveId;
    if (!firstItem) {
      if (!persistent) break;  // one item per wave (see traverse_bre_kernel)
      if (lane == 0) it = nWaves + atomicAdd(queueHead, 1u);
      it = __shfl(it, 0, 64);
    }
    firstItem = false;
    // (wave-uniform, and SAID so: the item's record, its pair region and everything derived from them then live in scalar
    // registers -- as vector registers they were ten of the values this kernel spills around its hot loop, round 5)
    it = (uint32_t)__builtin_amdgcn_readfirstlane((int)it);
    uint32_t part = 0u, parts = 1u;
    if (units) {
      // entry `it` of the unit queue: the list of large parts, then the small ones (see EVAL_UNIT)
      const uint32_t c0 = min(unitCtl[0], unitCap), c1 = min(unitCtl[1], unitCap);
      if (it >= c0 + c1) break;
      const uint2 u = it < c0 ? units[it] : units[(size_t)unitCap + (it - c0)];
      it = u.x;
      part = u.y & 0xFFFFu;
      parts = u.y >> 16;
    }
    if (it >= nItems) break;
    const uint4 item = items[it];
    const uint32_t setBase = item.x, nb = item.y & 0xFFu;
    if (nb == 0) continue;
    const uint32_t cntb = (uint32_t)lane < nb ? pairCnt[(size_t)it * B + lane] : 0u;
    const uint32_t incl = wave_scan_incl(cntb, lane);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (total == 0) continue;
    // the wave's share [r0, r0 + n) of the item's concatenated lists
    const uint32_t per = (total + parts - 1u) / parts;
    const uint32_t r0 = part * per;
    if (r0 >= total) continue;
    const uint32_t n = min(per, total - r0);
#ifdef GVPM_EVAL_TIMING
    wLastStart = wall_clock64();
    lastN = n;
    lastUk = it;
    for (int k = 1; k <= 5; ++k) tkLast[k] = tk[k];  // ([1]: this unit's setup is added after this point)
    const unsigned long long su0 = TICK();
#endif
    const uint2 reg = itemOff[it];
    const uint32_t *lists = pairs + (size_t)reg.x * 64u;
    const uint32_t cap = reg.y;
    waveLdsSync();
    if (lane < B) s.boff[lane + 1] = incl;
    if (lane == 0) s.boff[0] = 0u;
    if (lane == 0) s.setBase = setBase;
#ifdef GVPM_EVAL_TIMING
    const unsigned long long su1 = TICK();
#endif
    loadTileRaysNoSync<B>(a, s, setBase, nb, lane);
#ifdef GVPM_EVAL_TIMING
    const unsigned long long su2 = TICK();
#endif
    for (int idx = lane; idx < 27 * B; idx += 64) (&s.acc[0][0])[idx] = 0.0;
    waveLdsSync();
    relToBase<B>(s, lane);
    waveLdsSync();
#ifdef GVPM_EVAL_TIMING
    suLast[0] = su0 - tItem; suLast[1] = su1 - su0; suLast[2] = su2 - su1; suLast[3] = TICK() - su2;
#endif
    [[maybe_unused]] unsigned long long tMark = TICK();
    tk[1] += tMark - tItem;
    tk[6] += 1;

    const bool use3D = cfgFlag<CFG::FIXED, CFG::USE3D>(a.cfg.vol_technique == GVPM_VOL_BRE3D);
    // my chunk [g0, g1) of the concatenated per-beam lists (lane l of ANY wave position: g0 = min(total, l * chunk))
    const uint32_t chunk = (n + 63u) / 64u;
    const uint32_t g0 = r0 + min(n, (uint32_t)lane * chunk), g1 = min(r0 + n, g0 + chunk);
    uint32_t cur = 0;  // current beam
    if (g0 < g1)
      while (s.boff[cur + 1] <= g0) cur++;

    for (uint32_t tSeg = 0; tSeg < chunk;) {
      // One pass per segment (round 5): a pair whose HIT the fp32 bands cannot decide (decidePair: ~1e-5 of the candidates)
      // goes to the exact pass behind this kernel (exact_shift.hip, GVPM_EX_KIND_BRE_PAIR: the reference predicate, the base
      // term and the four shifts in fp64) instead of through an fp64 predicate and a second round of both loops in here.
      {
        // ---- decision + phase 1 ----
        uint32_t qn = 0;  // wave-uniform
        Acc27 acc;
#pragma unroll
        for (int k = 0; k < 27; ++k) acc.v[k] = 0.f;
        bool dirty = false;  // acc holds sums of beam `cur`
        const uint32_t tLim = chunk;
        uint32_t t = tSeg;
        // the pair of a lane at step tt: entry g of the concatenated lists, its beam, its photon index.
        // The index of step t + 1 is fetched while step t computes: one dependent global load less per step.
        auto locate = [&](uint32_t tt, uint32_t from, bool &hv, uint32_t &gg, uint32_t &bb, uint32_t &pi) {
          gg = g0 + tt;
          hv = gg < g1 && tt < tLim;
          bb = from;  // (a lane's own pairs come in ascending beam order)
          pi = 0u;
          if (hv) {
            while (s.boff[bb + 1] <= gg) bb++;
            pi = lists[(size_t)bb * cap + (gg - s.boff[bb])];
          }
        };
        // PF (maps beyond the Infinity Cache): the photon INDEX of step t + 2 and the RECORD (its first 48 bytes) of step
        // t + 1 are in flight while step t computes; otherwise the index of step t + 1 only
        bool haveN = false, haveB = false;
        uint32_t gN = 0, bN = 0, pidxN = 0, gB = 0, bB = 0, pidxB = 0;
        locate(t, cur, haveN, gN, bN, pidxN);
        PhotonFront phN = {};
        if (PF) {
          locate(t + 1u, bN, haveB, gB, bB, pidxB);
          phN = loadFront(a, pidxN);  // (index 0 when the lane has no pair: a valid record, not used)
        }
        for (; t < tLim && t - tSeg < (uint32_t)SEG_STEPS && qn + 256u <= (uint32_t)SEG_QCAP; ++t) {
          [[maybe_unused]] const unsigned long long l0 = LTICK();
          const bool have = haveN;
          const uint32_t b = bN, pidx = pidxN;
          const PhotonFront phCur = phN;
          if (PF) {
            haveN = haveB; gN = gB; bN = bB; pidxN = pidxB;
            phN = loadFront(a, pidxN);
            locate(t + 2u, bN, haveB, gB, bB, pidxB);
          } else {
            locate(t + 1u, b, haveN, gN, bN, pidxN);
          }
          [[maybe_unused]] const unsigned long long l1 = LTICK();
          tk[7] += l1 - l0;
          uint32_t qMask = 0;
          [[maybe_unused]] unsigned long long l2 = l1, l3 = l1;
          if (have) {
            if (b != cur) {
              if (dirty) flushAcc<B>(s, acc, cur);
              dirty = false;
              cur = b;
            }
            l2 = LTICK();
            const PhotonFront ph = PF ? phCur : loadFront(a, pidx);
            const RayReg base = loadRay(s, 0, cur);
            int dec = decidePair<CFG>(ph.pos, base, s.rnd[cur], a.radius, a.cfg.epsilon, use3D);
            if (dec == 2) dec = decidePairFine<CFG>(ph.pos, base, s.rnd[cur], a.radius, a.cfg.epsilon, use3D);
#ifdef GVPM_EVAL_TIMING
            asm volatile("" :: "v"(dec));
            l3 = LTICK();
#endif
            if (dec == 1) {
              evalPhase1<B, HS, CFG>(a, s, ph, base, cur, acc, nNull, nFail, qMask);
              dirty = true;
              nEval++;
            } else if (dec == 2) {
              // the bands cannot decide this pair: the exact pass takes it whole (predicate, base term, four shifts)
              deferNote(a, GVPM_EX_KIND_BRE_PAIR, a.setPerm[s.setBase + cur], pidx, 0u, 1u);
            }
          }
          const uint32_t ent = ((t - tSeg) << (8 + BB)) | ((uint32_t)lane << (2 + BB)) | cur;
#pragma unroll
          for (uint32_t i = 0; i < 4u; ++i) {
            const bool qd = (qMask >> i) & 1u;
            const unsigned long long m = __ballot(qd);
            if (qd) s.q[qn + __popcll(m & ((1ull << lane) - 1ull))] = (Entry)(ent | (i << BB));
            qn += (uint32_t)__popcll(m);
          }
#ifdef GVPM_EVAL_TIMING
          { const unsigned long long l5 = LTICK(); tk[8] += l2 - l1; tk[9] += l3 - l2; tk[10] += l5 - l3; tk[11] += 1; }
#endif
        }
        if (dirty) flushAcc<B>(s, acc, cur);
        const uint32_t tEnd = t;  // first step of the next segment
        waveLdsSync();
        { [[maybe_unused]] const unsigned long long tn = TICK(); tk[2] += tn - tMark; tMark = tn; }
        // ---- phase 2 over the queue: lane l takes entries [l * cq, (l + 1) * cq) ----
        const uint32_t cq = (qn + 63u) / 64u;
        const uint32_t e0 = min(qn, (uint32_t)lane * cq), e1 = min(qn, e0 + cq);
        uint32_t key = 0xFFFFFFFFu;
        f3 rs = mk3(0.f), rw = mk3(0.f);
        // (the photon index of entry j + 1 is fetched while entry j computes)
        auto entry = [&](uint32_t j, bool &hv, uint32_t &k2o, uint32_t &pi, uint32_t &bo, uint32_t &io) {
          hv = j < cq && e0 + j < e1;
          k2o = 0xFFFFFFFFu;
          pi = bo = io = 0u;
          if (hv) {
            const uint32_t e = s.q[e0 + j];
            bo = e & ((1u << BB) - 1u);
            io = (e >> BB) & 3u;
            const uint32_t ln = (e >> (2 + BB)) & 63u, ts = e >> (8 + BB);
            const uint32_t g = r0 + min(n, ln * chunk) + tSeg + ts;
            pi = lists[(size_t)bo * cap + (g - s.boff[bo])];
            k2o = (bo << 2) | io;
          }
        };
        bool haveE = false, haveF = false;
        uint32_t k2E = 0, pidxE = 0, bE = 0, iE = 0, k2F = 0, pidxF = 0, bF = 0, iF = 0;
        entry(0u, haveE, k2E, pidxE, bE, iE);
        if (PF) entry(1u, haveF, k2F, pidxF, bF, iF);
        for (uint32_t j = 0; j <= cq; ++j) {
          const bool have = haveE;
          const uint32_t k2 = k2E, pidx = pidxE, b = bE, i = iE;
          [[maybe_unused]] float warm = 0.f;
          if (PF) {
            // the index of entry j + 2 in flight, and one word of the record of entry j + 1 touched: the line (the whole
            // 128-byte record) is on its way from HBM while entry j computes
            haveE = haveF; k2E = k2F; pidxE = pidxF; bE = bF; iE = iF;
            warm = reinterpret_cast<const float *>(a.cold + (size_t)pidxE * GVPM_REC_QUADS)[0];
            entry(j + 2u, haveF, k2F, pidxF, bF, iF);
          } else {
            entry(j + 1u, haveE, k2E, pidxE, bE, iE);
          }
          if (k2 != key && key != 0xFFFFFFFFu) {
            // the run of one (beam, shift) ended: its 6 sums go to the LDS accumulators
            const uint32_t kb = key >> 2, ki = key & 3u;
            atomicAdd(&s.acc[3 + 3 * ki + 0][kb], (double)rs.x);
            atomicAdd(&s.acc[3 + 3 * ki + 1][kb], (double)rs.y);
            atomicAdd(&s.acc[3 + 3 * ki + 2][kb], (double)rs.z);
            atomicAdd(&s.acc[15 + 3 * ki + 0][kb], (double)rw.x);
            atomicAdd(&s.acc[15 + 3 * ki + 1][kb], (double)rw.y);
            atomicAdd(&s.acc[15 + 3 * ki + 2][kb], (double)rw.z);
            rs = rw = mk3(0.f);
          }
          key = k2;
          if (have) {
            f3 sf, wb;
            evalPhase2Core<B, FULLVIS, HS, GVPM_EVAL_MIX, CFG>(a, s, pidx, b, (int)i, sf, wb, nDiff, nFail, ldsTri);
            rs = rs + sf;
            rw = rw + wb;
          }
          if (PF) asm volatile("" ::"v"(warm));
        }
        waveLdsSync();
        { [[maybe_unused]] const unsigned long long tn = TICK(); tk[3] += tn - tMark; tMark = tn; }
        tSeg = tEnd;
      }
    }
    // ---- write out: 27 partial sums per beam set into the running sum ----
    // sum index fastest: one wave-instruction adds 64 consecutive words of the pixels' 27-float rows (beam index fastest
    // added 4-word pieces of 16 rows: scattered float atomics run far below contiguous ones)
    for (uint32_t idx = lane; idx < 27u * min(nb, (uint32_t)B); idx += 64u) {
      const uint32_t bb = idx / 27u, k = idx - 27u * bb;
      const float v = (float)s.acc[k][bb];
      if (v != 0.f) {
        const uint32_t pv = s.pix[bb];
        const size_t p = (size_t)(pv >> 16) * a.cfg.width + (pv & 0xFFFFu);
        atomicAdd(&a.iter[p * 27 + k], v * a.iterScale);
      }
    }
    { [[maybe_unused]] const unsigned long long tn = TICK(); tk[5] += tn - tMark; if (tn - tItem > tItemMax) tItemMax = tn - tItem; }
#ifdef GVPM_EVAL_TIMING
    wLastEnd = wall_clock64();
#endif
  }
#ifdef GVPM_EVAL_TIMING
  tk[0] = TICK() - tStart;
  if (lane == 0)
  {
#if GVPM_EVAL_TIMING > 1  // (same-address atomics of thousands of ending waves stall the loads of the waves still running)
    for (int k = 0; k < 12; ++k) atomicAdd(&gvpmEvalTiming[k], tk[k]);
    atomicMax(&gvpmEvalTiming[12], tk[0]);
    atomicMax(&gvpmEvalTiming[13], tItemMax);
    atomicAdd(&gvpmEvalTiming[14], 1ull);
#endif
    if (waveId < 16384u) {
      unsigned long long *lg = gvpmEvalWaveLog + 16 * waveId;
      for (int k = 0; k < 4; ++k) lg[12 + k] = suLast[k];
      lg[0] = wStart;
      lg[1] = wall_clock64();
      lg[2] = tk[6];
      lg[3] = wLastStart;
      lg[4] = lastN;
      lg[5] = lastUk;
      for (int k = 1; k <= 5; ++k) lg[5 + k] = tk[k] - tkLast[k];
      lg[11] = wLastEnd;
    }
  }
#endif
  // ---- statistics ----
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
      unsigned long long *row = a.stats + 8 * (size_t)(waveId % GVPM_STAT_ROWS);
      atomicAdd(&row[0], ev);
      atomicAdd(&row[2], nu);
      atomicAdd(&row[3], di);
      atomicAdd(&row[4], fa);
    }
  }
}
