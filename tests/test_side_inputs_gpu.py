"""The side inputs of G-Beams, G-Planes and G-VPM through the staging ring (uploads.hip): end normals, second plane edges and
camera samples from pageable memory, from pinned memory, prefetched, and in their packed forms (linked beam records +
octahedral end normals; run-packed samples).  The reference of every test is the synchronous entry points fed the
HOST-unpacked arrays (gvpm_unpack_photons_linked, gvpm_unpack_normals_oct, gvpm_unpack_vpm_samples): what every gather read
(gvpm_download_photons / _beam_sides / _vpm_samples) must equal it bit for bit, the evaluation and shift counters must be
equal, and the accumulators agree within rtol 2e-6 (float atomics: the bar of test_staging_ring_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import cases
from gvpm_amd import abi, hip
from test_oracle_beams import make_beam_case
from test_oracle_planes import make_plane_case
from test_oracle_vpm import make_vpm_case
from test_side_inputs import malformed_run_lists

pytestmark = pytest.mark.gpu
STEPS = 7
FORMATS = ("pageable", "pinned", "packed")
PHOTON_ARRAYS = abi.PHOTON_VEC3 + abi.PHOTON_F1 + abi.PHOTON_U1
COUNTERS = ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts")
B1D, B3D = abi.GVPM_BEAM_BEAM_1D, abi.GVPM_BEAM_BEAM_3D_OPTIMIZED


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_photons(a, b):
    return a.n == b.n and all(same_bytes(getattr(a, k), getattr(b, k)) for k in PHOTON_ARRAYS)


class Inputs:
    """One iteration's photon-side inputs of a technique ("beams", "planes" or "vpm") in every form: pageable arrays, pinned
    holders, packed; and `ref`, the host-unpacked arrays of form `fmt` that the synchronous reference uploads"""

    def __init__(self, kind, fmt, table, ph, end_n=None, w1=None, len1=None, samples=None):
        self.kind, self.fmt, self.ph = kind, fmt, ph
        self.end_n, self.w1, self.len1, self.samples = end_n, w1, len1, samples
        self.pin_ph = self.pin = self.pin_smp = None
        if kind == "vpm":
            self.pin_ph = hip.PinnedPhotons(ph.n).fill(ph)
            self.pin_smp = hip.PinnedSamples(samples)
            self.runs, self.rands = hip.pack_vpm_samples(samples)
            self.ref = (ph, hip.unpack_vpm_samples(self.runs, self.rands) if fmt == "packed" else samples)
            return
        self.pin = hip.PinnedBeams(ph, end_n=end_n, w1=w1, len1=len1, table=table)
        self.blob = hip.pack_photons_linked(ph, table)
        ref_ph = hip.unpack_photons_linked(self.blob, table) if fmt == "packed" else ph
        if kind == "beams":
            self.codes = hip.pack_normals_oct(end_n)
            self.ref = (ref_ph, hip.unpack_normals_oct(self.codes) if fmt == "packed" else end_n)
        else:
            self.ref = (ref_ph, w1, len1)

    def close(self):
        for p in (self.pin_ph, self.pin, self.pin_smp):
            if p is not None:
                p.close()


def feed(ctx, x, prefetch):
    """x's inputs in its own format; prefetch: for the step after the coming gather"""
    if x.kind == "vpm":
        if x.fmt == "pageable":
            assert not prefetch
            ctx.upload_photons(x.ph)
            ctx.upload_vpm_samples(x.samples)
        else:
            ctx.prefetch(photons=x.pin_ph) if prefetch else ctx.upload_pinned(photons=x.pin_ph)
            ctx.upload_pinned_vpm_samples(x.pin_smp, prefetch=prefetch, packed=x.fmt == "packed")
    elif x.fmt == "pageable":
        assert not prefetch
        if x.kind == "beams":
            ctx.upload_beams(x.ph, x.end_n)
        else:
            ctx.upload_planes(x.ph, x.w1, x.len1)
    else:
        ctx.upload_pinned_beams(x.pin, prefetch=prefetch, packed=x.fmt == "packed")


def feed_reference(ctx, x):
    if x.kind == "vpm":
        ctx.upload_photons(x.ref[0])
        ctx.upload_vpm_samples(x.ref[1])
    elif x.kind == "beams":
        ctx.upload_beams(*x.ref)
    else:
        ctx.upload_planes(*x.ref)


def read_back(ctx, x):
    ph = ctx.download_photons(x.ph.n)
    if x.kind == "vpm":
        return ph, ctx.download_vpm_samples()
    sides = ctx.download_beam_sides(x.ph.n)
    return (ph,) + (sides if x.kind == "planes" else (sides,))


def same_inputs(got, want):
    return same_photons(got[0], want[0]) and all(same_bytes(a, b) for a, b in zip(got[1:], want[1:], strict=True))


def open_context(c, table):
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    cases.upload_bsdfs(ctx, c)
    ctx.upload_materials(table)
    return ctx


# ---- equivalence over seven steps ------------------------------------------------------------------------------------------
class Session:
    """Seven iterations of one technique: formats cycling pageable -> pinned -> packed, 500 more photons / beams a step"""

    def __init__(self, name):
        self.name = name
        kind = self.kind = {"vpm": "vpm", "beams1d": "beams", "beams3d": "beams", "planes": "planes"}[name]
        if kind == "vpm":
            c, n0 = make_vpm_case("cbox", 24, 20, 30000, 5.0, nb=8), 30000
        elif kind == "beams":
            c, n0 = make_beam_case("cbox", 32, 28, 12000, 2.5, technique=B1D if name == "beams1d" else B3D), 12000
        else:
            c, n0 = make_plane_case("cbox_in", 32, 28, 6000), 6000
        self.c, self.table = c, hip.MaterialTable()
        raw = []
        for k in range(STEPS):
            it, n = k + 1, n0 + 500 * k
            if kind == "vpm":
                ph, nb = c.sc.shoot_photons(it, n)
                rays, smp = c.sc.camera_beams_and_vpm_samples(it, 8)
                raw.append((nb, rays, dict(ph=ph, samples=smp)))
            elif kind == "beams":
                ph, en, nb = c.sc.shoot_beams(it, n)
                raw.append((nb, c.sc.camera_beams(it), dict(ph=ph, end_n=en)))
            else:
                ph, _, w1, len1, nb = c.sc.shoot_planes(it, n)
                raw.append((nb, c.sc.camera_beams(it), dict(ph=ph, w1=w1, len1=len1)))
            hip.pack_photons_linked(raw[-1][2]["ph"], self.table)   # (every step's materials first: the blobs then agree)
        self.nb = [r[0] for r in raw]
        self.rays = [r[1] for r in raw]
        self.pin_rays = [hip.PinnedRays(r[1]) for r in raw]
        self.steps = [Inputs(kind, FORMATS[k % 3], self.table, **r[2]) for k, r in enumerate(raw)]
        sizes = [x.ph.n for x in self.steps]
        assert sizes == sorted(sizes) and sizes[-1] >= sizes[0] + 2000
        self.ref = self.run("reference")
        self.ref2 = None

    def run(self, mode):
        """-> ([what every gather read], statistics, accumulators, G-VPM state)"""
        ctx = open_context(self.c, self.table)
        read, parked = [], False
        for k, x in enumerate(self.steps):
            if mode == "reference":
                feed_reference(ctx, x)
                ctx.upload_camera_beams(self.rays[k])
            else:
                if not parked:
                    feed(ctx, x, False)
                    if x.fmt == "pageable":
                        ctx.upload_camera_beams(self.rays[k])
                    else:
                        ctx.upload_pinned(rays=self.pin_rays[k])
                parked = False
                if mode == "prefetch" and k + 1 < STEPS and self.steps[k + 1].fmt != "pageable":
                    feed(ctx, self.steps[k + 1], True)
                    ctx.prefetch(rays=self.pin_rays[k + 1])
                    parked = True
            ctx.gather(k + 1, self.nb[k])
            read.append(read_back(ctx, x))
        out = read, ctx.stats(), ctx.download_accum(), (ctx.download_vpm_state() if self.kind == "vpm" else None)
        ctx.close()
        return out

    def close(self):
        for p in self.steps + self.pin_rays:
            p.close()


@pytest.fixture(scope="module", params=["vpm", "beams1d", "beams3d", "planes"])
def session(request):
    s = Session(request.param)
    yield s
    s.close()


def rel_spread(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


@pytest.mark.parametrize("mode", ["plain", "prefetch"])
def test_seven_steps_equal_the_synchronous_uploads_of_the_unpacked_arrays(session, mode):
    s = session
    ref_read, ref_st, ref_acc, ref_state = s.ref
    read, st, acc, state = s.run(mode)
    for k, (x, got, want) in enumerate(zip(s.steps, read, ref_read)):
        assert same_inputs(want, x.ref), (s.name, "reference", k)
        assert same_inputs(got, want), (s.name, mode, k, x.fmt)
    print(s.name, mode, {k: st[k] for k in COUNTERS}, "accumulators: max rel", rel_spread(acc, ref_acc))
    for k in COUNTERS:
        assert st[k] == ref_st[k], (k, st, ref_st)
    assert st["evaluations"] > 0
    if state is not None:
        print(s.name, mode, "scale_vol / n_vol: max rel", rel_spread(state[0], ref_state[0]), rel_spread(state[1], ref_state[1]))
        assert np.allclose(state[0], ref_state[0], rtol=1e-6, atol=0) and np.allclose(state[1], ref_state[1], rtol=1e-6, atol=0)
    assert np.allclose(acc, ref_acc, rtol=2e-6, atol=0)


def test_two_synchronous_runs_agree_within_the_bar(session):
    """The bar itself: two runs of the reference (the synchronous entry points, whose kernels this feature leaves alone) differ
    by less than the 2e-6 the equivalence test allows the new paths."""
    s = session
    again = s.run("reference")
    print(s.name, "two reference runs: max rel", rel_spread(again[2], s.ref[2]))
    assert all(again[1][k] == s.ref[1][k] for k in COUNTERS)
    assert np.allclose(again[2], s.ref[2], rtol=2e-6, atol=0)


# ---- decode parity at the sizes where the decoders change path ---------------------------------------------------------------
def run_sequence(ctx, items, nb):
    """items: [(Inputs, "pageable" | "pinned" | "prefetched")], consumed by consecutive gathers; a prefetched item is handed over
    before the gather of the item in front of it.  -> what every gather read"""
    read, parked = [], False
    for k, (x, how) in enumerate(items):
        if not parked:
            assert how != "prefetched"
            if how == "pageable":   # the packed records from pageable memory: the synchronous packed entry points
                if x.kind == "beams":
                    ctx.upload_beams_linked(x.blob, x.codes)
                elif x.kind == "planes":
                    ctx.upload_planes_linked(x.blob, x.w1, x.len1)
                else:
                    ctx.upload_vpm_samples_packed(x.runs, x.rands)
            else:
                feed_side(ctx, x, False)
        parked = False
        if k + 1 < len(items) and items[k + 1][1] == "prefetched":
            feed_side(ctx, items[k + 1][0], True)
            parked = True
        ctx.gather(k + 1, nb)
        read.append(read_back(ctx, x))
    return read


def feed_side(ctx, x, prefetch):
    """the packed form from pinned memory (G-VPM: the samples alone; the photons stay)"""
    if x.kind == "vpm":
        ctx.upload_pinned_vpm_samples(x.pin_smp, prefetch=prefetch, packed=True)
    else:
        ctx.upload_pinned_beams(x.pin, prefetch=prefetch, packed=True)


@pytest.mark.parametrize("kind", ["beams", "planes"])
def test_packed_beams_decode_as_the_host_unpackers_say(kind):
    """0, 1, 63, 64, 65 and 12 000 beams (a wave of the linked decoder takes 64 records; more than one workgroup), each from
    pageable memory, from pinned memory and prefetched"""
    if kind == "beams":
        c = make_beam_case("cbox", 16, 12, 12000, 2.5)
        arrays = dict(end_n=c.end_n)
    else:
        c = make_plane_case("cbox_in", 16, 12, 12000)
        arrays = dict(w1=c.w1, len1=c.len1)
    assert c.beams.n == 12000
    table = hip.MaterialTable()
    hip.pack_photons_linked(c.beams, table)
    items = []
    for n in (0, 1, 63, 64, 65, 12000):
        x = Inputs(kind, "packed", table, c.beams.subset(np.arange(n)), **{k: v[:n] for k, v in arrays.items()})
        items += [(x, "pageable"), (x, "pinned"), (x, "prefetched")]
    ctx = open_context(c, table)
    ctx.upload_camera_beams(c.rays)
    read = run_sequence(ctx, items, c.nb)
    st = ctx.stats()
    ctx.close()
    for (x, how), got in zip(items, read):
        assert same_inputs(got, x.ref), (kind, x.ph.n, how)
    assert st["evaluations"] > 0
    for x in {id(x): x for x, _ in items}.values():
        x.close()


@pytest.mark.parametrize("nb", [1, 8, 64, 70])
def test_run_packed_samples_expand_as_the_host_unpacker_says(nb):
    """runs of 1, 8, 64 and 70 samples (below, at and above a wave), each from pageable memory, from pinned memory and prefetched"""
    c = make_vpm_case("cbox", 12, 10, 4000, 5.0, nb=nb)
    table = hip.MaterialTable()
    x = Inputs("vpm", "packed", table, c.ph, samples=c.samples)
    assert x.runs["count"].max() == nb and x.runs.size > 64
    empty = Inputs("vpm", "packed", table, c.ph, samples=c.samples[:0])
    one = Inputs("vpm", "packed", table, c.ph, samples=c.samples[:1])
    ctx = open_context(c, table)
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(c.rays)
    items = [(x, "pageable"), (x, "pinned"), (x, "prefetched"), (empty, "pageable"), (one, "pinned"), (empty, "pinned"), (one, "prefetched")]
    read = run_sequence(ctx, items, c.nb)
    ctx.close()
    for (y, how), got in zip(items, read):
        assert same_bytes(got[1], y.ref[1]), (nb, y.samples.size, how)
    for y in (x, empty, one):
        y.close()


# ---- gvpm_gather_primal consumes a prefetched beam set the same way ------------------------------------------------------------
def test_primal_gather_consumes_a_prefetched_beam_set():
    c = make_beam_case("cbox", 32, 28, 3000, 2.5, technique=B3D, path_set=0)
    table = hip.MaterialTable()
    b2, en2, nb2 = c.sc.shoot_beams(2, 3500)
    for b in (c.beams, b2):
        hip.pack_photons_linked(b, table)
    first, second = Inputs("beams", "pinned", table, c.beams, end_n=c.end_n), Inputs("beams", "packed", table, b2, end_n=en2)
    out = []
    for mode in ("reference", "prefetch"):
        ctx = open_context(c, table)
        ctx.upload_camera_beams(c.rays)
        if mode == "reference":
            feed_reference(ctx, first)
            ctx.gather_primal(1, c.nb)
            feed_reference(ctx, second)
        else:
            feed(ctx, first, False)
            feed(ctx, second, True)
            ctx.gather_primal(1, c.nb)
        ctx.gather_primal(2, nb2)
        out.append((read_back(ctx, second), ctx.stats(), ctx.download_accum()))
        ctx.close()
    (ref_read, ref_st, ref_acc), (read, st, acc) = out
    assert same_inputs(ref_read, second.ref) and same_inputs(read, second.ref)
    assert st["evaluations"] == ref_st["evaluations"] > 0
    print("primal: max rel", rel_spread(acc, ref_acc))
    assert np.allclose(acc, ref_acc, rtol=2e-6, atol=0)
    first.close()
    second.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_new_entry_points():
    c = make_vpm_case("cbox", 12, 10, 2000, 5.0, nb=8)
    cb = make_beam_case("cbox", 12, 10, 500, 2.5)
    cp = make_plane_case("cbox_in", 12, 10, 500)
    table = hip.MaterialTable()
    beams = Inputs("beams", "packed", table, cb.beams, end_n=cb.end_n)
    planes = Inputs("planes", "packed", table, cp.beams, w1=cp.w1, len1=cp.len1)
    smp = Inputs("vpm", "packed", table, c.ph, samples=c.samples)
    L, INVALID, STATE = hip.lib(), abi.GVPM_ERR_INVALID_ARG, abi.GVPM_ERR_STATE
    ctx = open_context(c, table)
    h = ctx._h
    ptr = lambda a: np.ascontiguousarray(a).ctypes.data
    bsoa, psoa = cb.beams.soa(), cp.beams.soa()
    pageable = [lambda: L.gvpm_prefetch_beams(h, C.byref(bsoa), ptr(cb.end_n)),
                lambda: L.gvpm_prefetch_planes(h, C.byref(psoa), ptr(cp.w1), ptr(cp.len1)),
                lambda: L.gvpm_prefetch_beams_linked(h, ptr(beams.blob), beams.blob.size, ptr(beams.codes)),
                lambda: L.gvpm_prefetch_planes_linked(h, ptr(planes.blob), planes.blob.size, ptr(cp.w1), ptr(cp.len1)),
                lambda: L.gvpm_prefetch_vpm_samples(h, ptr(c.samples), c.samples.size),
                lambda: L.gvpm_prefetch_vpm_samples_packed(h, ptr(smp.runs), smp.runs.size, ptr(smp.rands), smp.rands.size),
                # pinned beam records, pageable side arrays: every array must be pinned
                lambda: L.gvpm_prefetch_beams(h, C.byref(beams.pin.soa), ptr(cb.end_n)),
                lambda: L.gvpm_prefetch_planes_linked(h, planes.pin.blob.ptr, planes.pin.blob.nbytes, planes.pin.w1.ptr, ptr(cp.len1))]
    for k, call in enumerate(pageable):
        assert call() == INVALID, k
    # a second pending set of a kind: beams, planes and photons share the photon slots; the samples have their own
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(c.rays)
    ctx.upload_vpm_samples(c.samples)
    ctx.upload_pinned_beams(beams.pin, prefetch=True)
    ctx.upload_pinned_vpm_samples(smp.pin_smp, prefetch=True)
    again = [lambda: L.gvpm_prefetch_beams(h, C.byref(beams.pin.soa), beams.pin.end_n.ptr),
             lambda: L.gvpm_prefetch_planes(h, C.byref(planes.pin.soa), planes.pin.w1.ptr, planes.pin.len1.ptr),
             lambda: L.gvpm_prefetch_beams_linked(h, beams.pin.blob.ptr, beams.pin.blob.nbytes, beams.pin.end_n_oct.ptr),
             lambda: L.gvpm_prefetch_planes_linked(h, planes.pin.blob.ptr, planes.pin.blob.nbytes, planes.pin.w1.ptr, planes.pin.len1.ptr),
             lambda: L.gvpm_prefetch_photons(h, C.byref(smp.pin_ph.soa)),
             lambda: L.gvpm_prefetch_vpm_samples(h, smp.pin_smp.samples.ptr, smp.pin_smp.n),
             lambda: L.gvpm_prefetch_vpm_samples_packed(h, smp.pin_smp.runs.ptr, smp.pin_smp.nruns, smp.pin_smp.rands.ptr, smp.pin_smp.n)]
    for k, call in enumerate(again):
        assert call() == STATE, k
    for k, call in enumerate(pageable):   # (pageable AND pending: the argument error comes first)
        assert call() == INVALID, k
    # the parked sets are what the next-but-one gather reads
    ctx.gather(1, c.nb)
    assert same_bytes(ctx.download_vpm_samples(), c.samples)
    ctx.upload_photons(c.ph)   # (the beams were parked in the photon slots: G-VPM gathers photons)
    # a malformed run list is refused before anything is copied: the samples in force stay
    good, bads = malformed_run_lists(int(c.samples.size))
    rands = np.ascontiguousarray(c.samples["rand"])
    for what, runs, n in bads:
        assert L.gvpm_upload_vpm_samples_packed(h, ptr(runs) if runs.size else None, runs.size, ptr(rands), n) == INVALID, what
    pr, pf = hip.PinnedArray(bads[1][1]), hip.PinnedArray(rands)
    assert L.gvpm_prefetch_vpm_samples_packed(h, pr.ptr, bads[1][1].size, pf.ptr, bads[1][2]) == INVALID
    ctx.gather(2, c.nb)
    assert same_bytes(ctx.download_vpm_samples(), smp.pin_smp.samples.view)
    # more than 2^24 - 1 beams: a forged count -- in a header-only blob, in the SoA's n -- is refused before anything is read
    blob = hip.pack_photons_linked(cb.beams.subset(np.zeros(0, np.int64)), table).copy()
    assert blob.size == 64
    blob.view(np.uint32)[1] = 1 << 24
    pinned_blob = hip.PinnedArray(blob)
    assert L.gvpm_upload_beams_linked(h, ptr(blob), blob.size, ptr(beams.codes)) == INVALID
    assert b"24-bit" in L.gvpm_last_error(h)
    assert L.gvpm_prefetch_beams_linked(h, pinned_blob.ptr, 64, beams.pin.end_n_oct.ptr) == INVALID
    assert L.gvpm_prefetch_planes_linked(h, pinned_blob.ptr, 64, planes.pin.w1.ptr, planes.pin.len1.ptr) == INVALID
    assert b"24-bit" in L.gvpm_last_error(h)
    forged = abi.PhotonSoA()
    C.memmove(C.byref(forged), C.byref(beams.pin.soa), C.sizeof(forged))
    forged.n = 1 << 24
    assert L.gvpm_prefetch_beams(h, C.byref(forged), beams.pin.end_n.ptr) == INVALID
    assert L.gvpm_prefetch_planes(h, C.byref(forged), planes.pin.w1.ptr, planes.pin.len1.ptr) == INVALID
    assert b"24-bit" in L.gvpm_last_error(h)
    # read-back before a gather of the technique
    assert L.gvpm_download_beam_sides(h, None, None) == STATE
    ctx.close()
    for p in (beams, planes, smp, pr, pf, pinned_blob):
        p.close()
