// Staging of the per-iteration inputs (C ABI, include/gvpm_hip.h): photon maps, photon beams / planes, camera beams and
// G-VPM samples, from pageable or pinned host memory (copy stream, three slots each, prefetch) or borrowed device memory.
// The ring's protocol is written once, below; the record formats are pack_host.hip (host) and decode_device.hip (device).
// Reference seam: the flattening of GPhotonNodeData + Path at gvpm/gvpm_accel.h:31-59,119-199.
#include "pack_codec.h"
#include "staging.h"

using PhotonSlot = gvpm_context::PhotonSlot;
using RaySlot = gvpm_context::RaySlot;
using SampleSlot = gvpm_context::SampleSlot;
using PhotonRing = gvpm_context::StagingRing<PhotonSlot>;
using RayRing = gvpm_context::StagingRing<RaySlot>;
using SampleRing = gvpm_context::StagingRing<SampleSlot>;

static bool isPinnedHost(const void *ptr) {
  hipPointerAttribute_t attr;
  if (!ptr || hipPointerGetAttributes(&attr, ptr) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory is reported as an error: not one of ours
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

// ---- the staging ring (context.h), each step once for both kinds of slot ---------------------------------------------------
// What the kinds differ in: the events of a slot's last readers, and what the handle reads of the current slot.
static int waitForReaders(gvpm_context *h, PhotonSlot &ps) {
  // the kernels of the gathers that last read this slot (its build; the G-Planes gather) may still be running
  HIP_TRY(h, hipStreamWaitEvent(h->copyStream, ps.consumed, 0));
  HIP_TRY(h, hipStreamWaitEvent(h->copyStream, ps.consumedB, 0));
  return GVPM_OK;
}
static int waitForReaders(gvpm_context *h, RaySlot &rs) {
  // the evaluation kernel of the step that last used this slot may still be reading it
  HIP_TRY(h, hipStreamWaitEvent(h->copyStream, rs.freed, 0));
  return GVPM_OK;
}
static int waitForReaders(gvpm_context *h, SampleSlot &ss) {
  // G-VPM's kernels read the samples (the redo on its side stream is joined back before the gather's tail)
  HIP_TRY(h, hipStreamWaitEvent(h->copyStream, ss.freed, 0));
  return GVPM_OK;
}
static void makeCurrent(gvpm_context *h, PhotonRing &r, int slot) {
  r.cur = slot;
  r.wait = r.ownedCur = true;
  const PhotonSlot &ps = r.slot[slot];
  h->rawDev = ps.dev;
  h->nph = (uint32_t)h->rawDev.n;
  h->havePhotons = h->photonsDirty = true;
  // the side arrays the slot carries (a plain photon upload carries none: the techniques that need them keep what they had)
  if (ps.side == gvpm_context::SIDE_BEAMS) {
    h->endNDev = ps.endN.p;
    h->haveBeamsMap = true;
  } else if (ps.side == gvpm_context::SIDE_PLANES) {
    h->w1Dev = ps.w1.p;
    h->len1Dev = ps.len1.p;
    h->havePlanes = true;
  }
}
static void makeCurrent(gvpm_context *h, SampleRing &r, int slot) {
  r.cur = slot;
  r.wait = r.ownedCur = true;
  h->samplesDev = r.slot[slot].smp.p;
  h->nsamples = r.slot[slot].n;
  h->haveSamples = true;
}
static void makeCurrent(gvpm_context *h, RayRing &r, int slot) {
  r.cur = slot;
  r.wait = r.ownedCur = true;
  h->raysDev = r.slot[slot].rays.p;
  h->nsets = r.slot[slot].nsets;
  h->haveBeams = h->beamsDirty = true;
}

// The refusals of a prefetch (from pageable memory; a second one pending), then the slot that is neither current nor
// pending, with the copy stream behind its last readers.
template <typename Slot>
static int acquireSlot(gvpm_context *h, gvpm_context::StagingRing<Slot> &r, bool prefetch, bool pinned, const char *needsPinned,
                       const char *alreadyPending, Slot **out) {
  if (prefetch && !pinned) return fail(h, GVPM_ERR_INVALID_ARG, needsPinned);
  if (prefetch && r.pending >= 0) return fail(h, GVPM_ERR_STATE, alreadyPending);
  int slot = (r.cur + 1) % 3;
  if (slot == r.pending) slot = (r.cur + 2) % 3;
  Slot &s = r.slot[slot];
  if (s.read)
    if (int rc = waitForReaders(h, s)) return rc;
  s.read = false;
  *out = &s;
  return GVPM_OK;
}
static const char *const PHOTONS_PENDING = "a prefetched photon set is already pending";
static const char *const BEAMS_PENDING = "a prefetched camera-beam list is already pending";
static const char *const SAMPLES_PENDING = "a prefetched set of vpm samples is already pending";

// Before a slot's buffers are regrown: regrowing frees the old ones, which a build or a decode on either compute stream, or
// a copy, may still be using.  All three streams whatever the format: DevBuf::ensure's hipFree is a device-wide sync as it is,
// so the wider wait only adds ordering to a path that already stalls.
static int syncBeforeRegrow(gvpm_context *h) {
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->streamB));
  HIP_TRY(h, hipStreamSynchronize(h->copyStream));
  return GVPM_OK;
}

// Behind a slot's copies: `copied`, then the slot is parked as pending (prefetch) or becomes the current input.
template <typename Slot>
static int finishSlot(gvpm_context *h, gvpm_context::StagingRing<Slot> &r, Slot *s, bool pinned, bool prefetch) {
  HIP_TRY(h, hipEventRecord(s->copied, h->copyStream));
  // pageable memory: the caller may reuse its buffers when this returns (one pageable array makes the runtime stage that copy
  // itself; the header's contract: the library copies during the call).  Pinned memory (gvpm_host_alloc*): the copy is left
  // in flight; the buffer must stay untouched until the gather that consumes it has returned (copyDoneAtTail) or the handle
  // was synchronised
  if (!pinned) HIP_TRY(h, hipStreamSynchronize(h->copyStream));
  const int slot = (int)(s - r.slot);
  if (prefetch) r.pending = slot;
  else makeCurrent(h, r, slot);
  return GVPM_OK;
}

// The consumer's side: both compute streams wait for the current slot's copy; a packed slot is decoded on `us`
// (`decode` launches the kernels) and the other stream waits for that.
template <typename Slot, typename Decode>
static int awaitCurrent(gvpm_context *h, gvpm_context::StagingRing<Slot> &r, hipStream_t us, hipStream_t other, Decode decode) {
  if (!r.wait) return GVPM_OK;
  Slot &s = r.slot[r.cur];
  HIP_TRY(h, hipStreamWaitEvent(h->stream, s.copied, 0));
  HIP_TRY(h, hipStreamWaitEvent(h->streamB, s.copied, 0));
  if (s.needUnpack) {
    if (int rc = decode(s)) return rc;
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(s.unpacked, us));
    HIP_TRY(h, hipStreamWaitEvent(other, s.unpacked, 0));
    s.needUnpack = false;
  }
  r.wait = false;
  r.fresh = true;
  return GVPM_OK;
}
// The header's lifetime rule for pinned buffers -- untouched until the gather that consumes them has returned -- holds by
// itself where the gather waits on the host for a kernel behind the copy (G-BRE's build, G-Beams' bounds).  G-Planes and
// G-VPM's samples have no such wait: the gather's tail waits for the copy it has just consumed (long complete: its kernels
// are queued behind it).  G-BRE's tail does not pay for the call.
template <typename Ring> static int copyDoneAtTail(gvpm_context *h, Ring &r, bool wait) {
  if (r.fresh && wait && r.ownedCur) HIP_TRY(h, hipEventSynchronize(r.slot[r.cur].copied));
  r.fresh = false;
  return GVPM_OK;
}
// prefetched inputs (gvpm_prefetch_*) become the current ones: what an upload at this point would have done
template <typename Ring> static void promotePending(gvpm_context *h, Ring &r) {
  if (r.pending < 0) return;
  const int slot = r.pending;
  r.pending = -1;
  makeCurrent(h, r, slot);
}

int stagingHead(gvpm_context *h, hipStream_t us, hipStream_t other) {
  int rc = awaitCurrent(h, h->ph, us, other, [&](PhotonSlot &ps) {
    // (a packed record names its parent's material by index: without a table every parent would decode as black)
    if (h->nmaterials == 0)
      return fail(h, GVPM_ERR_STATE, "packed photons were uploaded but no material table (gvpm_upload_materials)");
    if (ps.linked) launch_unpack_linked(ps.packed.p, (uint32_t)ps.dev.n, h->materials.p, h->nmaterials, ps.dev, h->stats.p + 6, us);
    else launch_unpack_photons(ps.packed.p, (uint32_t)ps.dev.n, h->materials.p, h->nmaterials, ps.dev, h->stats.p + 6, us);
    if (ps.octNormals) launch_unpack_normals_oct(ps.endNOct.p, (uint32_t)ps.dev.n, ps.endN.p, us);
    return (int)GVPM_OK;
  });
  if (rc != GVPM_OK) return rc;
  rc = awaitCurrent(h, h->smp, us, other, [&](SampleSlot &ss) {
    launch_expand_vpm_runs(ss.packed.p, ss.nruns, ss.n, ss.smp.p, us);
    return (int)GVPM_OK;
  });
  if (rc != GVPM_OK) return rc;
  return awaitCurrent(h, h->ray, us, other, [&](RaySlot &rs) {
    if (rs.ncompact) {
      if (!h->haveSensor) return fail(h, GVPM_ERR_STATE, "compact beam sets were uploaded but no sensor (gvpm_upload_sensor)");
      launch_unpack_compact_rays(h->sensor, rs.compact.p, rs.ncompact, rs.rays.p, us);
    }
    launch_unpack_rays(rs.packed.p, rs.nsets - rs.ncompact, rs.rays.p + (size_t)rs.ncompact * 5, us);
    return (int)GVPM_OK;
  });
}

int stagingTail(gvpm_context *h) {
  // the kernels just queued on the gather stream are the last readers of this step's camera rays
  if (h->ray.ownedCur) {
    RaySlot &rs = h->ray.slot[h->ray.cur];
    HIP_TRY(h, hipEventRecord(rs.freed, h->stream));
    rs.read = true;
  }
  // ... of G-VPM's samples
  if (h->smp.ownedCur) {
    SampleSlot &ss = h->smp.slot[h->smp.cur];
    HIP_TRY(h, hipEventRecord(ss.freed, h->stream));
    ss.read = true;
  }
  // ... and of the staged photon arrays (the build on either stream; G-Planes reads them in the gather itself)
  const bool breTech = h->cfg.vol_technique == GVPM_VOL_BRE2D || h->cfg.vol_technique == GVPM_VOL_BRE3D;
  if (int rc = copyDoneAtTail(h, h->ph, !breTech)) return rc;
  if (int rc = copyDoneAtTail(h, h->ray, !breTech)) return rc;
  if (int rc = copyDoneAtTail(h, h->smp, !breTech)) return rc;
  if (h->ph.ownedCur) {
    // G-BRE reads them in its build only (reorder_kernel), and gatherBRE has waited for that build on the host (the
    // planner's counters): nothing of it is in flight here.  An event behind the whole gather made the prefetched copy
    // of step N+2 wait for the EVALUATION of step N: the PCIe-inclusive step went from 3.6 to 5.8 ms.  The other
    // techniques read them on the gather stream (their builds; G-Planes in the gather kernel itself).
    PhotonSlot &ps = h->ph.slot[h->ph.cur];
    const bool bre = h->cfg.vol_technique == GVPM_VOL_BRE2D || h->cfg.vol_technique == GVPM_VOL_BRE3D;
    if (!bre) {
      HIP_TRY(h, hipEventRecord(ps.consumed, h->stream));
      HIP_TRY(h, hipEventRecord(ps.consumedB, h->streamB));
      ps.read = true;
    }
  }
  promotePending(h, h->ph);
  promotePending(h, h->ray);
  promotePending(h, h->smp);
  return GVPM_OK;
}

// ---- the uploads into the ring: each its argument checks, its capacity needs and its copies --------------------------------
// The per-beam side arrays that ride in a photon slot beside its beam records: end normals (fp32, or one octahedral code a
// beam) for G-Beams, the second plane edges for G-Planes.  Host pointers.
struct SideArrays {
  int kind = gvpm_context::SIDE_NONE;
  const float *endN = nullptr;
  const uint32_t *endNOct = nullptr;
  const float *w1 = nullptr, *len1 = nullptr;
  const char *needsPinned = nullptr;  // the refusal of a prefetch from pageable memory, in the entry point's name
};
static bool sidePinned(const SideArrays &sd) {
  for (const void *q : {(const void *)sd.endN, (const void *)sd.endNOct, (const void *)sd.w1, (const void *)sd.len1})
    if (q && !isPinnedHost(q)) return false;
  return true;
}
static bool sideFits(const PhotonSlot &ps, const SideArrays &sd, size_t n) {
  if (sd.kind == gvpm_context::SIDE_BEAMS) return ps.endN.cap >= n * 3 + 4 && (!sd.endNOct || ps.endNOct.cap >= n + 4);
  if (sd.kind == gvpm_context::SIDE_PLANES) return ps.w1.cap >= n * 3 + 4 && ps.len1.cap >= n + 4;
  return true;
}
// (after syncBeforeRegrow)
static int growSide(gvpm_context *h, PhotonSlot &ps, const SideArrays &sd, size_t n) {
  if (sd.kind == gvpm_context::SIDE_BEAMS) {
    HIP_TRY(h, ps.endN.ensure(n * 3 + 4));
    if (sd.endNOct) HIP_TRY(h, ps.endNOct.ensure(n + 4));
  } else if (sd.kind == gvpm_context::SIDE_PLANES) {
    HIP_TRY(h, ps.w1.ensure(n * 3 + 4));
    HIP_TRY(h, ps.len1.ensure(n + 4));
  }
  return GVPM_OK;
}
// on the copy stream, behind the slot's beam records and in front of its `copied`
static int copySide(gvpm_context *h, PhotonSlot &ps, const SideArrays &sd, size_t n) {
  ps.side = sd.kind;
  ps.octNormals = n > 0 && sd.endNOct != nullptr;
  if (!n) return GVPM_OK;
  if (sd.endNOct) HIP_TRY(h, hipMemcpyAsync(ps.endNOct.p, sd.endNOct, n * 4, hipMemcpyHostToDevice, h->copyStream));
  else if (sd.endN) HIP_TRY(h, hipMemcpyAsync(ps.endN.p, sd.endN, n * 12, hipMemcpyHostToDevice, h->copyStream));
  if (sd.w1) HIP_TRY(h, hipMemcpyAsync(ps.w1.p, sd.w1, n * 12, hipMemcpyHostToDevice, h->copyStream));
  if (sd.len1) HIP_TRY(h, hipMemcpyAsync(ps.len1.p, sd.len1, n * 4, hipMemcpyHostToDevice, h->copyStream));
  return GVPM_OK;
}

static int uploadPhotonsCommon(gvpm_context *h, const gvpm_photon_soa *p, bool fromDevice, bool prefetch = false,
                               const SideArrays &sd = SideArrays()) {
  if (!p) return fail(h, GVPM_ERR_INVALID_ARG, "null photon soa");
  if (p->n > 0x7FFFFFF0ull) return fail(h, GVPM_ERR_INVALID_ARG, "too many photons");
  const uint32_t n = (uint32_t)p->n;
  const PhotonArrayPtrs src(*p);
  for (const void *q : src.p)
    if (n && !q) return fail(h, GVPM_ERR_INVALID_ARG, "null photon array");
  if (fromDevice) {
    if (prefetch) return fail(h, GVPM_ERR_INVALID_ARG, "prefetch takes host buffers");
    h->rawDev = *p;
    h->ph.wait = h->ph.ownedCur = false;
    h->nph = n;
    h->havePhotons = h->photonsDirty = true;
    return GVPM_OK;
  }
  // one block in the ABI's order (gvpm_host_alloc_photons) is one allocation and one copy: its first array speaks for all
  bool oneBlock = n > 0;
  size_t words = 0;
  for (int k = 0; k < PHOTON_ARRAYS && oneBlock; ++k) {
    oneBlock = (const char *)src.p[k] == (const char *)src.p[0] + words * 4;
    words += (size_t)n * photonArrayWords(k);
  }
  // pinned only if EVERY array is
  bool pinned = n > 0;
  for (int k = 0; k < (oneBlock ? 1 : PHOTON_ARRAYS) && pinned; ++k) pinned = isPinnedHost(src.p[k]);
  // (an EMPTY beam / plane set may be prefetched like any other: its pointers, where given, say where it comes from)
  if (n == 0 && sd.kind != gvpm_context::SIDE_NONE) pinned = src.p[0] && isPinnedHost(src.p[0]);
  pinned = pinned && sidePinned(sd);
  PhotonSlot *ps;
  if (int rc = acquireSlot(h, h->ph, prefetch, pinned,
                           sd.needsPinned ? sd.needsPinned : "gvpm_prefetch_photons needs pinned host memory (gvpm_host_alloc*)",
                           PHOTONS_PENDING, &ps))
    return rc;
  if (ps->raw.cap < (size_t)n * PHOTON_WORDS + 8 || !sideFits(*ps, sd, n)) {
    if (int rc = syncBeforeRegrow(h)) return rc;
    HIP_TRY(h, ps->raw.ensure((size_t)n * PHOTON_WORDS + 8));
    if (int rc = growSide(h, *ps, sd, n)) return rc;
  }
  photonArraysInBlock(ps->dev, ps->raw.p, n);
  ps->needUnpack = ps->linked = false;
  if (oneBlock) HIP_TRY(h, hipMemcpyAsync(ps->raw.p, src.p[0], (size_t)n * PHOTON_WORDS * 4, hipMemcpyHostToDevice, h->copyStream));
  uint32_t *to = ps->raw.p;
  for (int k = 0; k < PHOTON_ARRAYS && n && !oneBlock; ++k) {
    HIP_TRY(h, hipMemcpyAsync(to, src.p[k], (size_t)n * photonArrayWords(k) * 4, hipMemcpyHostToDevice, h->copyStream));
    to += (size_t)n * photonArrayWords(k);
  }
  if (int rc = copySide(h, *ps, sd, n)) return rc;
  return finishSlot(h, h->ph, ps, pinned, prefetch);
}

// the packed twin of uploadPhotonsCommon: one copy of 76 n bytes into the slot.  The decode into the slot's SoA arrays is
// left to the gather that consumes the slot, at the head of its build (stagingHead): a kernel on the copy stream would
// sit between two copies and wait for compute units behind the gather kernels of the step in flight -- measured at C2,
// 4.7 ms a step that way against 3.6 for the SoA upload it was to beat
// (linkedBytes != 0: `src` is a blob of linked records of that size, n64 its photon count)
static int uploadPhotonsPacked(gvpm_context *h, const gvpm_photon_packed *src, uint64_t n64, bool prefetch, size_t linkedBytes = 0,
                               const SideArrays &sd = SideArrays()) {
  if (n64 && !src) return fail(h, GVPM_ERR_INVALID_ARG, "null packed photons");
  if (n64 > 0x7FFFFFF0ull) return fail(h, GVPM_ERR_INVALID_ARG, "too many photons");
  const uint32_t n = (uint32_t)n64;
  bool pinned = n > 0 && isPinnedHost(src);
  if (n == 0 && sd.kind != gvpm_context::SIDE_NONE) pinned = src && isPinnedHost(src);  // (an empty beam / plane set: uploadPhotonsCommon)
  pinned = pinned && sidePinned(sd);
  PhotonSlot *ps;
  if (int rc = acquireSlot(h, h->ph, prefetch, pinned,
                           sd.needsPinned ? sd.needsPinned : "gvpm_prefetch_photons_packed needs pinned host memory (gvpm_host_alloc)",
                           PHOTONS_PENDING, &ps))
    return rc;
  constexpr size_t RW = sizeof(gvpm_photon_packed) / 4;
  const size_t packedWords = linkedBytes ? (linkedBytes + 3u) / 4u + 8u : (size_t)n * RW + 8;
  if (ps->raw.cap < (size_t)n * PHOTON_WORDS + 8 || ps->packed.cap < packedWords || !sideFits(*ps, sd, n)) {
    if (int rc = syncBeforeRegrow(h)) return rc;
    HIP_TRY(h, ps->raw.ensure((size_t)n * PHOTON_WORDS + 8));
    if (int rc = growSide(h, *ps, sd, n)) return rc;
    // (a blob of linked records is never larger than the packed records of its photons + its tables: sized for those, so that
    // blobs of varying size do not regrow the slot)
    HIP_TRY(h, ps->packed.ensure(std::max(packedWords, (size_t)n * RW + 8 + 16384u)));
  }
  photonArraysInBlock(ps->dev, ps->raw.p, n);
  ps->needUnpack = n > 0;
  ps->linked = linkedBytes != 0;
  if (n) HIP_TRY(h, hipMemcpyAsync(ps->packed.p, src, linkedBytes ? linkedBytes : (size_t)n * sizeof(gvpm_photon_packed), hipMemcpyHostToDevice, h->copyStream));
  if (int rc = copySide(h, *ps, sd, n)) return rc;
  return finishSlot(h, h->ph, ps, pinned, prefetch);
}

static int uploadLinked(gvpm_context *h, const void *blob, size_t bytes, bool prefetch, const SideArrays &sd = SideArrays()) {
  if (!blob || bytes < sizeof(gvpm_linked_header)) return fail(h, GVPM_ERR_INVALID_ARG, "null or short blob of linked photon records");
  gvpm_linked_header hd;
  memcpy(&hd, blob, sizeof(hd));
  if (sd.kind != gvpm_context::SIDE_NONE && hd.n > 0xFFFFFFu) return fail(h, GVPM_ERR_INVALID_ARG, "too many beams (24-bit beam index)");
  if (!linkedHeaderOk(hd, bytes)) return fail(h, GVPM_ERR_INVALID_ARG, "not a blob of gvpm_pack_photons_linked (header / sizes)");
  // (an empty blob of beams keeps its pointer: it says whether the set comes from pinned memory)
  if (hd.n == 0u) return uploadPhotonsPacked(h, sd.kind != gvpm_context::SIDE_NONE ? static_cast<const gvpm_photon_packed *>(blob) : nullptr, 0, prefetch, 0, sd);
  return uploadPhotonsPacked(h, static_cast<const gvpm_photon_packed *>(blob), hd.n, prefetch, hd.bytes, sd);
}

// Photon beams and planes: a photon upload whose slot also carries the side arrays (host memory), or borrowed device memory
static const char *const BEAMS_NEED_PINNED = "gvpm_prefetch_beams* needs pinned host memory (gvpm_host_alloc*), end normals included";
static const char *const PLANES_NEED_PINNED = "gvpm_prefetch_planes* needs pinned host memory (gvpm_host_alloc*), w1 and len1 included";
static int uploadPhotonBeamsCommon(gvpm_context *h, const gvpm_photon_soa *b, const float *end_n, bool fromDevice, bool prefetch = false) {
  if (b && b->n && !end_n) return fail(h, GVPM_ERR_INVALID_ARG, "null end_n");
  if (b && b->n > 0xFFFFFFull) return fail(h, GVPM_ERR_INVALID_ARG, "too many beams (24-bit beam index)");
  SideArrays sd;
  sd.kind = gvpm_context::SIDE_BEAMS;
  sd.endN = end_n;
  sd.needsPinned = BEAMS_NEED_PINNED;
  if (int rc = uploadPhotonsCommon(h, b, fromDevice, prefetch, sd)) return rc;
  if (fromDevice) {
    h->endNDev = end_n;
    h->haveBeamsMap = true;
  }
  return GVPM_OK;
}

static int uploadPlanesCommon(gvpm_context *h, const gvpm_photon_soa *b, const float *w1, const float *len1, bool fromDevice,
                              bool prefetch = false) {
  if (b && b->n && (!w1 || !len1)) return fail(h, GVPM_ERR_INVALID_ARG, "null w1 / len1");
  // (the synchronous entry points never had G-Beams' limit; the prefetch ones state it)
  if (prefetch && b && b->n > 0xFFFFFFull) return fail(h, GVPM_ERR_INVALID_ARG, "too many planes (24-bit beam index)");
  SideArrays sd;
  sd.kind = gvpm_context::SIDE_PLANES;
  sd.w1 = w1;
  sd.len1 = len1;
  sd.needsPinned = PLANES_NEED_PINNED;
  if (int rc = uploadPhotonsCommon(h, b, fromDevice, prefetch, sd)) return rc;
  if (fromDevice) {
    h->w1Dev = w1;
    h->len1Dev = len1;
    h->havePlanes = true;
  }
  return GVPM_OK;
}

static int uploadBeamsLinked(gvpm_context *h, const void *blob, size_t bytes, const uint32_t *end_n_oct, bool prefetch) {
  SideArrays sd;
  sd.kind = gvpm_context::SIDE_BEAMS;
  sd.endNOct = end_n_oct;
  sd.needsPinned = BEAMS_NEED_PINNED;
  if (blob && bytes >= sizeof(gvpm_linked_header)) {
    gvpm_linked_header hd;
    memcpy(&hd, blob, sizeof(hd));
    if (hd.n && hd.n <= 0xFFFFFFu && !end_n_oct) return fail(h, GVPM_ERR_INVALID_ARG, "null end_n_oct");
  }
  return uploadLinked(h, blob, bytes, prefetch, sd);
}
static int uploadPlanesLinked(gvpm_context *h, const void *blob, size_t bytes, const float *w1, const float *len1, bool prefetch) {
  SideArrays sd;
  sd.kind = gvpm_context::SIDE_PLANES;
  sd.w1 = w1;
  sd.len1 = len1;
  sd.needsPinned = PLANES_NEED_PINNED;
  if (blob && bytes >= sizeof(gvpm_linked_header)) {
    gvpm_linked_header hd;
    memcpy(&hd, blob, sizeof(hd));
    if (hd.n && hd.n <= 0xFFFFFFu && (!w1 || !len1)) return fail(h, GVPM_ERR_INVALID_ARG, "null w1 / len1");
  }
  return uploadLinked(h, blob, bytes, prefetch, sd);
}

static int uploadBeamsCommon(gvpm_context *h, const gvpm_camera_ray *rays, uint64_t nsets, bool fromDevice,
                             bool prefetch = false) {
  if (nsets && !rays) return fail(h, GVPM_ERR_INVALID_ARG, "null camera rays");
  if (nsets > 0x0FFFFFFFull) return fail(h, GVPM_ERR_INVALID_ARG, "too many beam sets");
  if (fromDevice) {
    if (prefetch) return fail(h, GVPM_ERR_INVALID_ARG, "prefetch takes host buffers");
    h->raysDev = rays;
    h->ray.wait = h->ray.ownedCur = false;
    h->nsets = (uint32_t)nsets;
    h->haveBeams = h->beamsDirty = true;
    return GVPM_OK;
  }
  const bool pinned = nsets && isPinnedHost(rays);
  RaySlot *rs;
  if (int rc = acquireSlot(h, h->ray, prefetch, pinned, "gvpm_prefetch_camera_beams needs pinned host memory (gvpm_host_alloc)", BEAMS_PENDING, &rs))
    return rc;
  if (rs->rays.cap < (size_t)nsets * 5 + 1) {
    if (int rc = syncBeforeRegrow(h)) return rc;
    HIP_TRY(h, rs->rays.ensure((size_t)nsets * 5 + 1));
  }
  rs->nsets = (uint32_t)nsets;
  rs->ncompact = 0;
  rs->needUnpack = false;
  if (nsets) HIP_TRY(h, hipMemcpyAsync(rs->rays.p, rays, (size_t)nsets * 5 * sizeof(gvpm_camera_ray), hipMemcpyHostToDevice, h->copyStream));
  return finishSlot(h, h->ray, rs, pinned, prefetch);
}

static int uploadBeamsPacked(gvpm_context *h, const gvpm_beam_set_packed *src, uint64_t nsets, bool prefetch) {
  if (nsets && !src) return fail(h, GVPM_ERR_INVALID_ARG, "null packed beam sets");
  if (nsets > 0x0FFFFFFFull) return fail(h, GVPM_ERR_INVALID_ARG, "too many beam sets");
  const bool pinned = nsets && isPinnedHost(src);
  RaySlot *rs;
  if (int rc = acquireSlot(h, h->ray, prefetch, pinned, "gvpm_prefetch_camera_beams_packed needs pinned host memory (gvpm_host_alloc)", BEAMS_PENDING, &rs))
    return rc;
  constexpr size_t SW = sizeof(gvpm_beam_set_packed) / 4;
  if (rs->rays.cap < (size_t)nsets * 5 + 1 || rs->packed.cap < (size_t)nsets * SW + 8) {
    if (int rc = syncBeforeRegrow(h)) return rc;
    HIP_TRY(h, rs->rays.ensure((size_t)nsets * 5 + 1));
    HIP_TRY(h, rs->packed.ensure((size_t)nsets * SW + 8));
  }
  rs->nsets = (uint32_t)nsets;
  rs->ncompact = 0;
  rs->needUnpack = nsets > 0;
  if (nsets) HIP_TRY(h, hipMemcpyAsync(rs->packed.p, src, (size_t)nsets * sizeof(gvpm_beam_set_packed), hipMemcpyHostToDevice, h->copyStream));
  return finishSlot(h, h->ray, rs, pinned, prefetch);
}

// compact sets (60 bytes, rebuilt from the sensor) + the full packed sets of deeper edges: two copies into the slot,
// decoded by the consuming gather like the packed records
static int uploadBeamsCompact(gvpm_context *h, const gvpm_beam_set_compact *compact, uint64_t ncompact,
                              const gvpm_beam_set_packed *full, uint64_t nfull, bool prefetch) {
  if ((ncompact && !compact) || (nfull && !full)) return fail(h, GVPM_ERR_INVALID_ARG, "null compact / full beam sets");
  const uint64_t nsets = ncompact + nfull;
  if (nsets > 0x0FFFFFFFull) return fail(h, GVPM_ERR_INVALID_ARG, "too many beam sets");
  if (ncompact && !h->haveSensor) return fail(h, GVPM_ERR_STATE, "compact beam sets need gvpm_upload_sensor first");
  const bool pinned = nsets && (!ncompact || isPinnedHost(compact)) && (!nfull || isPinnedHost(full));
  RaySlot *rs;
  if (int rc = acquireSlot(h, h->ray, prefetch, pinned, "gvpm_prefetch_camera_beams_compact needs pinned host memory (gvpm_host_alloc)", BEAMS_PENDING, &rs))
    return rc;
  constexpr size_t SW = sizeof(gvpm_beam_set_packed) / 4, CW = sizeof(gvpm_beam_set_compact) / 4;
  if (rs->rays.cap < (size_t)nsets * 5 + 1 || rs->packed.cap < (size_t)nfull * SW + 8 || rs->compact.cap < (size_t)ncompact * CW + 8) {
    if (int rc = syncBeforeRegrow(h)) return rc;
    HIP_TRY(h, rs->rays.ensure((size_t)nsets * 5 + 1));
    HIP_TRY(h, rs->packed.ensure((size_t)nfull * SW + 8));
    HIP_TRY(h, rs->compact.ensure((size_t)ncompact * CW + 8));
  }
  rs->nsets = (uint32_t)nsets;
  rs->ncompact = (uint32_t)ncompact;
  rs->needUnpack = nsets > 0;
  if (ncompact)
    HIP_TRY(h, hipMemcpyAsync(rs->compact.p, compact, (size_t)ncompact * sizeof(gvpm_beam_set_compact), hipMemcpyHostToDevice, h->copyStream));
  if (nfull)
    HIP_TRY(h, hipMemcpyAsync(rs->packed.p, full, (size_t)nfull * sizeof(gvpm_beam_set_packed), hipMemcpyHostToDevice, h->copyStream));
  return finishSlot(h, h->ray, rs, pinned, prefetch);
}

static int uploadSamplesCommon(gvpm_context *h, const gvpm_vpm_sample *smp, uint64_t n, bool fromDevice, bool prefetch = false) {
  if (n && !smp) return fail(h, GVPM_ERR_INVALID_ARG, "null vpm samples");
  if (n > 0x7FFFFFF0ull) return fail(h, GVPM_ERR_INVALID_ARG, "too many vpm samples");
  if (fromDevice) {
    if (prefetch) return fail(h, GVPM_ERR_INVALID_ARG, "prefetch takes host buffers");
    h->samplesDev = smp;
    h->smp.wait = h->smp.ownedCur = false;
    h->nsamples = (uint32_t)n;
    h->haveSamples = true;
    return GVPM_OK;
  }
  const bool pinned = n && isPinnedHost(smp);
  SampleSlot *ss;
  if (int rc = acquireSlot(h, h->smp, prefetch, pinned, "gvpm_prefetch_vpm_samples needs pinned host memory (gvpm_host_alloc)", SAMPLES_PENDING, &ss))
    return rc;
  if (ss->smp.cap < (size_t)n + 1) {
    if (int rc = syncBeforeRegrow(h)) return rc;
    HIP_TRY(h, ss->smp.ensure((size_t)n + 1));
  }
  ss->n = (uint32_t)n;
  ss->nruns = 0;
  ss->needUnpack = false;
  if (n) HIP_TRY(h, hipMemcpyAsync(ss->smp.p, smp, (size_t)n * sizeof(gvpm_vpm_sample), hipMemcpyHostToDevice, h->copyStream));
  return finishSlot(h, h->smp, ss, pinned, prefetch);
}

// the run-packed twin: the runs and one rand a sample land in the slot's `packed`, expanded by the consuming gather
static int uploadSamplesPacked(gvpm_context *h, const gvpm_vpm_run *runs, uint64_t nruns, const float *rands, uint64_t n, bool prefetch) {
  if (n > 0x7FFFFFF0ull) return fail(h, GVPM_ERR_INVALID_ARG, "too many vpm samples");
  if (n && !rands) return fail(h, GVPM_ERR_INVALID_ARG, "null rands");
  if (!vpmRunsOk(runs, nruns, n))
    return fail(h, GVPM_ERR_INVALID_ARG, "vpm sample runs: contiguous from sample 0, none empty, counts summing to n (gvpm_unpack_vpm_samples)");
  const bool pinned = n && isPinnedHost(runs) && isPinnedHost(rands);
  SampleSlot *ss;
  if (int rc = acquireSlot(h, h->smp, prefetch, pinned, "gvpm_prefetch_vpm_samples_packed needs pinned host memory (gvpm_host_alloc)", SAMPLES_PENDING, &ss))
    return rc;
  const size_t words = (size_t)nruns * 4 + (size_t)n + 8;
  if (ss->smp.cap < (size_t)n + 1 || ss->packed.cap < words) {
    if (int rc = syncBeforeRegrow(h)) return rc;
    HIP_TRY(h, ss->smp.ensure((size_t)n + 1));
    // (room for a run every fourth sample: lists of varying length seldom regrow the slot)
    HIP_TRY(h, ss->packed.ensure(std::max(words, (size_t)n * 2 + 8)));
  }
  ss->n = (uint32_t)n;
  ss->nruns = (uint32_t)nruns;
  ss->needUnpack = n > 0;
  if (n) {
    HIP_TRY(h, hipMemcpyAsync(ss->packed.p, runs, (size_t)nruns * sizeof(gvpm_vpm_run), hipMemcpyHostToDevice, h->copyStream));
    HIP_TRY(h, hipMemcpyAsync(ss->packed.p + (size_t)nruns * 4, rands, (size_t)n * 4, hipMemcpyHostToDevice, h->copyStream));
  }
  return finishSlot(h, h->smp, ss, pinned, prefetch);
}

// ---- read-back of what the last gather decoded (tests and debugging) ----
static int syncAllStreams(gvpm_context *h) {
  for (hipStream_t s : {h->copyStream, h->stream, h->streamB, h->streamC, h->streamA2})
    if (s) HIP_TRY(h, hipStreamSynchronize(s));
  return GVPM_OK;
}

extern "C" {

int gvpm_upload_materials(gvpm_context *h, const gvpm_material *table, uint32_t n) {
  CHECK_H(h);
  if (n && !table) return fail(h, GVPM_ERR_INVALID_ARG, "null material table");
  if (n > 65536u) return fail(h, GVPM_ERR_INVALID_ARG, "more than 65536 materials");
  // The unpack kernels that read the table run at the head of a gather's build chain (gather stream or build stream) and
  // may be in flight.  A table that only GROWS (the usual case: gvpm_pack_photons appends) is safe to extend under them --
  // no record in flight names an entry beyond the old count; an edit of existing entries, or a regrowth (which frees the
  // old buffer), first waits for every stream of the handle.
  const bool prefixSame = n >= h->nmaterials && h->nmaterials == (uint32_t)h->materialsHost.size() &&
                          (h->nmaterials == 0 || memcmp(h->materialsHost.data(), table, (size_t)h->nmaterials * sizeof(gvpm_material)) == 0);
  const bool regrow = h->materials.cap < (size_t)n + 1;
  if (regrow || !prefixSame)
    if (int rc = syncBeforeRegrow(h)) return rc;
  if (regrow) HIP_TRY(h, h->materials.ensure(std::max<size_t>((size_t)n + 1, 64)));
  const uint32_t first = (regrow || !prefixSame) ? 0u : h->nmaterials;
  if (n > first)
    HIP_TRY(h, hipMemcpy(h->materials.p + first, table + first, (size_t)(n - first) * sizeof(gvpm_material), hipMemcpyHostToDevice));
  h->materialsHost.assign(table, table + n);
  h->nmaterials = n;
  return GVPM_OK;
}

int gvpm_host_alloc(uint64_t bytes, void **out) {
  if (!out || bytes == 0) return GVPM_ERR_INVALID_ARG;
  return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? GVPM_OK : GVPM_ERR_HIP;
}
int gvpm_host_free(void *p) { return hipHostFree(p) == hipSuccess ? GVPM_OK : GVPM_ERR_HIP; }
int gvpm_host_alloc_photons(uint64_t n, gvpm_photon_soa *view, void **block) {
  if (!view || !block || n == 0 || n > 0x7FFFFFF0ull) return GVPM_ERR_INVALID_ARG;
  if (hipHostMalloc(block, (size_t)n * PHOTON_WORDS * 4, hipHostMallocDefault) != hipSuccess) return GVPM_ERR_HIP;
  photonArraysInBlock(*view, (const uint32_t *)*block, n);
  return GVPM_OK;
}

int gvpm_upload_photons(gvpm_context *h, const gvpm_photon_soa *p) {
  CHECK_H(h);
  return uploadPhotonsCommon(h, p, false);
}
int gvpm_upload_photons_dev(gvpm_context *h, const gvpm_photon_soa *p) {
  CHECK_H(h);
  return uploadPhotonsCommon(h, p, true);
}
int gvpm_prefetch_photons(gvpm_context *h, const gvpm_photon_soa *p) {
  CHECK_H(h);
  return uploadPhotonsCommon(h, p, false, true);
}
int gvpm_upload_photons_packed(gvpm_context *h, const gvpm_photon_packed *photons, uint64_t n) {
  CHECK_H(h);
  return uploadPhotonsPacked(h, photons, n, false);
}
int gvpm_prefetch_photons_packed(gvpm_context *h, const gvpm_photon_packed *photons, uint64_t n) {
  CHECK_H(h);
  return uploadPhotonsPacked(h, photons, n, true);
}
int gvpm_upload_photons_linked(gvpm_context *h, const void *blob, size_t bytes) {
  CHECK_H(h);
  return uploadLinked(h, blob, bytes, false);
}
int gvpm_prefetch_photons_linked(gvpm_context *h, const void *blob, size_t bytes) {
  CHECK_H(h);
  return uploadLinked(h, blob, bytes, true);
}

int gvpm_upload_planes(gvpm_context *h, const gvpm_photon_soa *beams, const float *w1, const float *len1) {
  CHECK_H(h);
  return uploadPlanesCommon(h, beams, w1, len1, false);
}
int gvpm_upload_planes_dev(gvpm_context *h, const gvpm_photon_soa *beams, const float *w1, const float *len1) {
  CHECK_H(h);
  return uploadPlanesCommon(h, beams, w1, len1, true);
}
int gvpm_upload_beams(gvpm_context *h, const gvpm_photon_soa *beams, const float *end_n) {
  CHECK_H(h);
  return uploadPhotonBeamsCommon(h, beams, end_n, false);
}
int gvpm_upload_beams_dev(gvpm_context *h, const gvpm_photon_soa *beams, const float *end_n) {
  CHECK_H(h);
  return uploadPhotonBeamsCommon(h, beams, end_n, true);
}

int gvpm_prefetch_beams(gvpm_context *h, const gvpm_photon_soa *beams, const float *end_n) {
  CHECK_H(h);
  return uploadPhotonBeamsCommon(h, beams, end_n, false, true);
}
int gvpm_prefetch_planes(gvpm_context *h, const gvpm_photon_soa *beams, const float *w1, const float *len1) {
  CHECK_H(h);
  return uploadPlanesCommon(h, beams, w1, len1, false, true);
}
int gvpm_upload_beams_linked(gvpm_context *h, const void *blob, size_t bytes, const uint32_t *end_n_oct) {
  CHECK_H(h);
  return uploadBeamsLinked(h, blob, bytes, end_n_oct, false);
}
int gvpm_prefetch_beams_linked(gvpm_context *h, const void *blob, size_t bytes, const uint32_t *end_n_oct) {
  CHECK_H(h);
  return uploadBeamsLinked(h, blob, bytes, end_n_oct, true);
}
int gvpm_upload_planes_linked(gvpm_context *h, const void *blob, size_t bytes, const float *w1, const float *len1) {
  CHECK_H(h);
  return uploadPlanesLinked(h, blob, bytes, w1, len1, false);
}
int gvpm_prefetch_planes_linked(gvpm_context *h, const void *blob, size_t bytes, const float *w1, const float *len1) {
  CHECK_H(h);
  return uploadPlanesLinked(h, blob, bytes, w1, len1, true);
}

int gvpm_upload_sensor(gvpm_context *h, const gvpm_sensor *sensor) {
  CHECK_H(h);
  if (!sensor) return fail(h, GVPM_ERR_INVALID_ARG, "null sensor");
  if (sensor->width < 1 || sensor->height < 1 || sensor->width > 65535 || sensor->height > 65535 ||
      !(sensor->tan_half_fov_x > 0.0) || !(sensor->tan_half_fov_y > 0.0))
    return fail(h, GVPM_ERR_INVALID_ARG, "sensor: film size in 1..65535 and positive field of view");
  for (int k = 0; k < 3; ++k) {
    // rows of a rotation: unit length, mutually orthogonal (a sheared or scaled transform is not a pinhole this format covers)
    const double *r = sensor->to_world + 3 * k, *q = sensor->to_world + 3 * ((k + 1) % 3);
    if (std::fabs(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] - 1.0) > 1e-9 || std::fabs(r[0] * q[0] + r[1] * q[1] + r[2] * q[2]) > 1e-9)
      return fail(h, GVPM_ERR_INVALID_ARG, "sensor: to_world must be a rotation");
  }
  // (the decode kernel takes the sensor by value at launch: nothing on the device to order against)
  h->sensor = *sensor;
  h->haveSensor = true;
  return GVPM_OK;
}

int gvpm_upload_camera_beams(gvpm_context *h, const gvpm_camera_ray *rays, uint64_t n_sets) {
  CHECK_H(h);
  return uploadBeamsCommon(h, rays, n_sets, false);
}
int gvpm_upload_camera_beams_dev(gvpm_context *h, const gvpm_camera_ray *rays, uint64_t n_sets) {
  CHECK_H(h);
  return uploadBeamsCommon(h, rays, n_sets, true);
}
int gvpm_prefetch_camera_beams(gvpm_context *h, const gvpm_camera_ray *rays, uint64_t n_sets) {
  CHECK_H(h);
  return uploadBeamsCommon(h, rays, n_sets, false, true);
}
int gvpm_upload_camera_beams_packed(gvpm_context *h, const gvpm_beam_set_packed *sets, uint64_t n_sets) {
  CHECK_H(h);
  return uploadBeamsPacked(h, sets, n_sets, false);
}
int gvpm_prefetch_camera_beams_packed(gvpm_context *h, const gvpm_beam_set_packed *sets, uint64_t n_sets) {
  CHECK_H(h);
  return uploadBeamsPacked(h, sets, n_sets, true);
}
int gvpm_upload_camera_beams_compact(gvpm_context *h, const gvpm_beam_set_compact *compact, uint64_t n_compact,
                                     const gvpm_beam_set_packed *full, uint64_t n_full) {
  CHECK_H(h);
  return uploadBeamsCompact(h, compact, n_compact, full, n_full, false);
}
int gvpm_prefetch_camera_beams_compact(gvpm_context *h, const gvpm_beam_set_compact *compact, uint64_t n_compact,
                                       const gvpm_beam_set_packed *full, uint64_t n_full) {
  CHECK_H(h);
  return uploadBeamsCompact(h, compact, n_compact, full, n_full, true);
}

int gvpm_upload_vpm_samples(gvpm_context *h, const gvpm_vpm_sample *samples, uint64_t n) {
  CHECK_H(h);
  return uploadSamplesCommon(h, samples, n, false);
}
int gvpm_upload_vpm_samples_dev(gvpm_context *h, const gvpm_vpm_sample *samples, uint64_t n) {
  CHECK_H(h);
  return uploadSamplesCommon(h, samples, n, true);
}

int gvpm_prefetch_vpm_samples(gvpm_context *h, const gvpm_vpm_sample *samples, uint64_t n) {
  CHECK_H(h);
  return uploadSamplesCommon(h, samples, n, false, true);
}
int gvpm_upload_vpm_samples_packed(gvpm_context *h, const gvpm_vpm_run *runs, uint64_t n_runs, const float *rands, uint64_t n) {
  CHECK_H(h);
  return uploadSamplesPacked(h, runs, n_runs, rands, n, false);
}
int gvpm_prefetch_vpm_samples_packed(gvpm_context *h, const gvpm_vpm_run *runs, uint64_t n_runs, const float *rands, uint64_t n) {
  CHECK_H(h);
  return uploadSamplesPacked(h, runs, n_runs, rands, n, true);
}

int gvpm_download_beam_sides(gvpm_context *h, float *vec3_out, float *len1_out) {
  CHECK_H(h);
  if (!h->haveGathered) return fail(h, GVPM_ERR_STATE, "gvpm_download_beam_sides: no gather yet");
  const bool planes = h->gatheredSide == gvpm_context::SIDE_PLANES;
  if (!planes && h->gatheredSide != gvpm_context::SIDE_BEAMS)
    return fail(h, GVPM_ERR_STATE, "gvpm_download_beam_sides: the last gather was neither G-Beams nor G-Planes");
  const size_t n = (size_t)h->gatheredPh.n;
  if (n && (!vec3_out || (planes && !len1_out))) return fail(h, GVPM_ERR_INVALID_ARG, "gvpm_download_beam_sides: null destination array");
  if (n && !(planes ? h->gatheredW1 && h->gatheredLen1 : h->gatheredEndN != nullptr))
    return fail(h, GVPM_ERR_STATE, "gvpm_download_beam_sides: that gather had no side arrays (it failed)");
  if (int rc = syncAllStreams(h)) return rc;
  if (n) HIP_TRY(h, hipMemcpy(vec3_out, planes ? h->gatheredW1 : h->gatheredEndN, n * 12, hipMemcpyDeviceToHost));
  if (n && planes) HIP_TRY(h, hipMemcpy(len1_out, h->gatheredLen1, n * 4, hipMemcpyDeviceToHost));
  return GVPM_OK;
}

int gvpm_download_vpm_samples(gvpm_context *h, gvpm_vpm_sample *dst, uint64_t cap, uint64_t *n) {
  CHECK_H(h);
  if (!h->haveGathered) return fail(h, GVPM_ERR_STATE, "gvpm_download_vpm_samples: no gather yet");
  if (!h->gatheredVpm) return fail(h, GVPM_ERR_STATE, "gvpm_download_vpm_samples: the last gather was not a G-VPM one");
  if (!n || (cap && !dst)) return fail(h, GVPM_ERR_INVALID_ARG, "gvpm_download_vpm_samples: null n or dst");
  *n = h->gatheredNSamples;
  const uint64_t m = std::min<uint64_t>(cap, h->gatheredNSamples);
  if (int rc = syncAllStreams(h)) return rc;
  if (m) HIP_TRY(h, hipMemcpy(dst, h->gatheredSamples, (size_t)m * sizeof(gvpm_vpm_sample), hipMemcpyDeviceToHost));
  return GVPM_OK;
}

int gvpm_download_photons(gvpm_context *h, const gvpm_photon_soa *dst) {
  CHECK_H(h);
  if (!h->haveGathered) return fail(h, GVPM_ERR_STATE, "gvpm_download_photons: no gather yet");
  const gvpm_photon_soa &s = h->gatheredPh;
  if (!dst || dst->n != s.n) return fail(h, GVPM_ERR_INVALID_ARG, "gvpm_download_photons: dst->n must be the gathered photon count");
  const PhotonArrayPtrs from(s), to(*dst);
  for (const void *q : to.p)
    if (s.n && !q) return fail(h, GVPM_ERR_INVALID_ARG, "gvpm_download_photons: null destination array");
  if (int rc = syncAllStreams(h)) return rc;
  for (int k = 0; k < PHOTON_ARRAYS && s.n; ++k)
    HIP_TRY(h, hipMemcpy(const_cast<void *>(to.p[k]), from.p[k], (size_t)s.n * photonArrayWords(k) * 4, hipMemcpyDeviceToHost));
  return GVPM_OK;
}

int gvpm_download_camera_beams(gvpm_context *h, gvpm_camera_ray *dst, uint64_t cap, uint64_t *n) {
  CHECK_H(h);
  if (!h->haveGathered) return fail(h, GVPM_ERR_STATE, "gvpm_download_camera_beams: no gather yet");
  if (!n || (cap && !dst)) return fail(h, GVPM_ERR_INVALID_ARG, "gvpm_download_camera_beams: null n or dst");
  *n = h->gatheredSets;
  const uint64_t m = std::min<uint64_t>(cap, h->gatheredSets);
  if (int rc = syncAllStreams(h)) return rc;
  if (m) HIP_TRY(h, hipMemcpy(dst, h->gatheredRays, (size_t)m * 5 * sizeof(gvpm_camera_ray), hipMemcpyDeviceToHost));
  return GVPM_OK;
}

}  // extern "C"
