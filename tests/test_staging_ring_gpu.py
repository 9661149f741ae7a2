"""The staging ring (uploads.hip, staging.h) with its slots reused ACROSS formats: seven consecutive G-BRE iterations whose
photon format cycles SoA from pageable memory -> SoA from one pinned block -> packed -> linked and whose ray format cycles
SoA -> packed -> compact.  Three slots, cycles of 4 and 3: every slot holds at least two formats in turn, and the photon
count grows by 500 a step, so slots regrow while older ones are still referenced.  Once with plain uploads and once with
the inputs of step N+1 prefetched from pinned memory before gather N (pageable SoA photons cannot be: uploaded in their
turn).  The reference is the same seven steps fed by plain pageable SoA uploads of the HOST-unpacked arrays (gvpm_unpack_*;
compact sets in the order the compact upload gives them): what every gather read (gvpm_download_photons /
gvpm_download_camera_beams) must equal the reference's bit for bit, the evaluation counts must be equal and the final
accumulators agree to rtol 2e-6 (float atomics: the bar of test_prefetched_pinned_uploads_equal_plain_uploads)."""
import ctypes as C

import numpy as np
import pytest

import cases
from gvpm_amd import abi, hip

pytestmark = pytest.mark.gpu
STEPS = 7
PHOTON_FORMATS = ("soa_pageable", "soa_pinned", "packed", "linked")
RAY_FORMATS = ("soa", "packed", "compact")
PHOTON_ARRAYS = abi.PHOTON_VEC3 + abi.PHOTON_F1 + abi.PHOTON_U1


class Step:
    """One iteration's inputs in its formats, and the host-unpacked arrays the reference uploads"""

    def __init__(self, c, k, table):
        it = k + 1
        self.it = it
        self.pfmt, self.rfmt = PHOTON_FORMATS[k % 4], RAY_FORMATS[k % 3]
        self.ph, self.nb = c.sc.shoot_photons(it, 6000 + 500 * k)
        self.rays = c.sc.camera_beams(it)
        sensor = c.sc.sensor()
        jitter = c.sc.jitter(it, self.rays)
        # pageable records ...
        self.packed = hip.pack_photons(self.ph, table)
        self.blob = hip.pack_photons_linked(self.ph, table)
        self.rpacked = hip.pack_camera_beams(self.rays)
        self.comp, self.full, _ = hip.pack_camera_beams_compact(sensor, self.rays, jitter)
        # ... and the same in pinned memory (the table holds every material by now: the records are the same)
        self.pin_ph = hip.PinnedPhotons(self.ph.n).fill(self.ph)
        self.pin_rays = hip.PinnedRays(self.rays)
        self.pin = hip.PinnedPacked(self.ph, self.rays, table, sensor=sensor if self.rfmt == "compact" else None,
                                    jitter=jitter if self.rfmt == "compact" else None, linked=self.pfmt == "linked")
        self.ref_ph = {"packed": lambda: hip.unpack_photons(self.packed, table),
                       "linked": lambda: hip.unpack_photons_linked(self.blob, table)}.get(self.pfmt, lambda: self.ph)()
        self.ref_rays = {"soa": lambda: self.rays, "packed": lambda: hip.unpack_camera_beams(self.rpacked),
                         "compact": lambda: np.concatenate([hip.unpack_camera_beams_compact(sensor, self.comp),
                                                            hip.unpack_camera_beams(self.full)])}[self.rfmt]()

    def close(self):
        for p in (self.pin_ph, self.pin_rays, self.pin):
            p.close()


def upload_photons(ctx, s, prefetch):
    L, h = hip.lib(), ctx._h
    if s.pfmt == "soa_pageable":
        assert not prefetch
        ctx.upload_photons(s.ph)
    elif s.pfmt == "soa_pinned":
        ctx.prefetch(photons=s.pin_ph) if prefetch else ctx.upload_pinned(photons=s.pin_ph)
    elif s.pfmt == "packed":
        if prefetch:
            ctx._check(L.gvpm_prefetch_photons_packed(h, s.pin._pp, s.pin.n))
        else:
            ctx.upload_photons_packed(s.packed)
    elif prefetch:
        ctx._check(L.gvpm_prefetch_photons_linked(h, s.pin._pp, s.pin.photon_bytes))
    else:
        ctx.upload_photons_linked(s.blob)


def upload_rays(ctx, s, prefetch):
    L, h = hip.lib(), ctx._h
    if s.rfmt == "soa":
        ctx.prefetch(rays=s.pin_rays) if prefetch else ctx.upload_camera_beams(s.rays)
    elif s.rfmt == "packed":
        if prefetch:
            ctx._check(L.gvpm_prefetch_camera_beams_packed(h, s.pin._pr, s.pin.nsets))
        else:
            ctx.upload_camera_beams_packed(s.rpacked)
    elif prefetch:
        ctx._check(L.gvpm_prefetch_camera_beams_compact(h, s.pin._pc if s.pin.ncompact else None, s.pin.ncompact,
                                                        s.pin._pr if s.pin.nfull else None, s.pin.nfull))
    else:
        ctx.upload_camera_beams_compact(s.comp, s.full)


def run(c, steps, table, mode):
    """-> ([(photons, rays) every gather read], statistics, accumulators)"""
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ctx.upload_sensor(c.sc.sensor())
    ctx.upload_materials(table)
    read = []
    prefetched = [False, False]   # the coming step's photons / rays are parked in the ring
    for k, s in enumerate(steps):
        if mode == "reference":
            ctx.upload_photons(s.ref_ph)
            ctx.upload_camera_beams(s.ref_rays)
        else:
            if not prefetched[0]:
                upload_photons(ctx, s, False)
            if not prefetched[1]:
                upload_rays(ctx, s, False)
            prefetched = [False, False]
            if mode == "prefetch" and k + 1 < len(steps):
                nxt = steps[k + 1]
                if nxt.pfmt != "soa_pageable":
                    upload_photons(ctx, nxt, True)
                    prefetched[0] = True
                upload_rays(ctx, nxt, True)
                prefetched[1] = True
        ctx.gather(s.it, s.nb)
        read.append((ctx.download_photons(s.ph.n), ctx.download_camera_beams()))
    st, acc = ctx.stats(), ctx.download_accum()
    ctx.close()
    return read, st, acc


@pytest.fixture(scope="module")
def ring_case():
    c = cases.make_case("cbox", 24, 20, 6000, 3.0)
    table = hip.MaterialTable()
    for k in range(STEPS):   # every step's materials first: later packs of the same photons then give the same records
        hip.pack_photons(c.sc.shoot_photons(k + 1, 6000 + 500 * k)[0], table)
    steps = [Step(c, k, table) for k in range(STEPS)]
    assert [s.ph.n for s in steps] == sorted(s.ph.n for s in steps) and steps[-1].ph.n > steps[0].ph.n + 2000
    assert all(s.comp.size > 0 for s in steps)
    ref = run(c, steps, table, "reference")
    yield c, steps, table, ref
    for s in steps:
        s.close()


@pytest.mark.parametrize("mode", ["plain", "prefetch"])
def test_slots_reused_across_formats_read_what_the_host_unpackers_give(ring_case, mode):
    c, steps, table, (ref_read, ref_st, ref_acc) = ring_case
    read, st, acc = run(c, steps, table, mode)
    for s, (ph, rays), (rph, rrays) in zip(steps, read, ref_read):
        for name in PHOTON_ARRAYS:
            a, b = np.ascontiguousarray(getattr(ph, name)), np.ascontiguousarray(getattr(rph, name))
            assert a.tobytes() == b.tobytes(), (mode, s.it, s.pfmt, name)
        assert rays.shape == rrays.shape and rays.tobytes() == rrays.tobytes(), (mode, s.it, s.rfmt)
    print(mode, "evaluations", st["evaluations"], ref_st["evaluations"], "max rel",
          float(np.max(np.abs(acc - ref_acc) / np.maximum(np.abs(ref_acc), 1e-30))))
    assert st["evaluations"] == ref_st["evaluations"] > 0
    assert np.allclose(acc, ref_acc, rtol=2e-6, atol=0)


def test_the_two_refusals_of_a_prefetch_for_every_format(ring_case):
    """gvpm_prefetch_* from pageable memory is an argument error, a second prefetch before the gather that consumes the first
    a call-order error, for every format; neither disturbs the ring: the parked inputs are what the next-but-one gather reads."""
    c, steps, table, (ref_read, _, _) = ring_case
    s, L = steps[3], hip.lib()   # (linked photons, SoA rays; its pinned copies serve the other formats' second prefetch)
    ctx = hip.Context(c.p, device=0)
    h = ctx._h
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ctx.upload_sensor(c.sc.sensor())
    ctx.upload_materials(table)
    soa = s.ph.soa()
    photon_calls = [lambda: L.gvpm_prefetch_photons(h, C.byref(soa)),
                    lambda: L.gvpm_prefetch_photons_packed(h, s.packed.ctypes.data, s.packed.size),
                    lambda: L.gvpm_prefetch_photons_linked(h, s.blob.ctypes.data, s.blob.size)]
    ray_calls = [lambda: L.gvpm_prefetch_camera_beams(h, s.rays.ctypes.data, s.rays.shape[0]),
                 lambda: L.gvpm_prefetch_camera_beams_packed(h, s.rpacked.ctypes.data, s.rpacked.shape[0]),
                 lambda: L.gvpm_prefetch_camera_beams_compact(h, s.comp.ctypes.data, s.comp.size, None, 0)]
    for call in photon_calls + ray_calls:
        assert call() == abi.GVPM_ERR_INVALID_ARG
    upload_photons(ctx, steps[0], False)
    upload_rays(ctx, steps[0], False)
    upload_photons(ctx, s, True)
    upload_rays(ctx, s, True)
    pinned_again = [lambda: L.gvpm_prefetch_photons(h, C.byref(s.pin_ph.soa)),
                    lambda: L.gvpm_prefetch_photons_packed(h, s.pin._pp, s.pin.n),
                    lambda: L.gvpm_prefetch_photons_linked(h, s.pin._pp, s.pin.photon_bytes),
                    lambda: L.gvpm_prefetch_camera_beams(h, s.pin_rays.ptr, s.pin_rays.nsets),
                    lambda: L.gvpm_prefetch_camera_beams_packed(h, s.pin._pr, s.pin.nsets)]
    for call in pinned_again + photon_calls + ray_calls:   # (pageable AND pending: the argument error comes first)
        assert call() == (abi.GVPM_ERR_STATE if call in pinned_again else abi.GVPM_ERR_INVALID_ARG)
    ctx.gather(1, steps[0].nb)
    ctx.gather(2, s.nb)
    ph, rays = ctx.download_photons(s.ph.n), ctx.download_camera_beams()
    ctx.close()
    for name in PHOTON_ARRAYS:
        assert np.ascontiguousarray(getattr(ph, name)).tobytes() == np.ascontiguousarray(getattr(ref_read[3][0], name)).tobytes(), name
    assert rays.tobytes() == ref_read[3][1].tobytes()
