"""The four device decoders of decode_device.hip against the host definitions of the same bytes, BIT FOR BIT, every field:

    unpack_photons_kernel                          gvpm_unpack_photons
    unpack_linked_kernel + link_linked_kernel      gvpm_unpack_photons_linked
    unpack_rays_kernel                             gvpm_unpack_camera_beams
    unpack_compact_rays_kernel                     gvpm_unpack_camera_beams_compact

pack_codec.h compiles one text for both sides, fp64 without contraction, so no tolerance is taken anywhere.  Each input
is uploaded through its packed path, gathered once, and read back with gvpm_download_photons / gvpm_download_camera_beams.
The shapes sit where these kernels go wrong: photon counts around the 16-photon kinds words, the 64-photon ballot groups
and the 256-thread blocks, plus a map of about a million photons; linked blobs made of real light paths with every record
pattern the decoder treats apart (asserted from the header and the kinds words); beam-set counts whose 5 n rays straddle
the 256-thread block (5 n = 255, 260) and the fifth block (5 n = 1275, 1280, 1285 -- 5 n is never 256 or 1280 +- 1), with
invalid shifted rays and a -0 length; the pageable and the pinned / prefetched uploads.

The last part uploads the malformed blobs of test_linked_malformed.py: the device must refuse what the host definition
refuses -- header defects at upload, body defects through gvpm_get_stats -- and leave nothing behind on the handle."""
import numpy as np
import pytest

import cases
from gvpm_amd import abi, hip
import test_linked_malformed as M

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 255, 256, 257, 4097)
LARGE = (1 << 20) - 3  # about a million photons, neither a multiple of 16 nor of 64
SET_COUNTS = (1, 51, 52, 255, 256, 257)
FIELDS = abi.PHOTON_VEC3 + abi.PHOTON_F1 + abi.PHOTON_U1
OCT_ZERO = 0x80008000


def assert_photons_bits(got, want, what):
    assert got.n == want.n, what
    for k in FIELDS:
        g = np.ascontiguousarray(getattr(got, k)).view(np.uint32).reshape(got.n, -1)
        w = np.ascontiguousarray(getattr(want, k)).view(np.uint32).reshape(want.n, -1)
        bad = np.nonzero((g != w).any(1))[0]
        assert bad.size == 0, f"{what}: {k} differs at photons {bad[:8].tolist()} (of {bad.size})"


def assert_rays_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g = np.ascontiguousarray(got).view(np.uint32).reshape(got.shape[0], -1)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(want.shape[0], -1)
    bad = np.nonzero((g != w).any(1))[0]
    if bad.size:
        fields = [k for k in abi.CAMERA_RAY_DTYPE.names
                  if not np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32))]
        raise AssertionError(f"{what}: sets {bad[:8].tolist()} (of {bad.size}) differ in {fields}")


@pytest.fixture(scope="module")
def big():
    """one light-path map of LARGE photons (cbox) as the source of every photon window"""
    return cases.make_case("cbox", 16, 12, LARGE, 3.0)


@pytest.fixture(scope="module")
def frame():
    """camera beam sets of a 48 x 40 frame behind a mirror: compact-eligible sets and deeper (full) ones"""
    return cases.make_case("cbox_mirror", 48, 40, 2000, 3.0)


def new_ctx(c):
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    return ctx


def window(ph, n, salt):
    off = (salt * 7919) % (ph.n - n + 1)
    return ph.subset(np.arange(off, off + n))


# ---- photons ---------------------------------------------------------------------------------------------------------

def test_packed_photon_records(big):
    t = hip.MaterialTable()
    hip.pack_photons(big.ph.subset(np.arange(20000)), t)
    ctx = new_ctx(big)
    for it, n in enumerate(COUNTS + (LARGE,), 1):
        ph = window(big.ph, n, it)
        pk = hip.pack_photons(ph, t)
        ctx.upload_materials(t)
        ctx.upload_photons_packed(pk)
        ctx.upload_camera_beams(big.rays)
        ctx.gather(it, big.nb)
        assert_photons_bits(ctx.download_photons(n), hip.unpack_photons(pk, t), f"packed records, n = {n}")
    # (the large map holds both parities and zero normals)
    assert set(np.unique(pk["flags"] >> 7 & 1)) == {0, 1} and (pk["parent_n_oct"] == OCT_ZERO).any()
    ctx.stats()  # nothing reported
    ctx.close()


def kinds_of(blob):
    return M.blob_views(blob)[3]


def linked_patterns(big):
    """{name: (photons, check(blob, table))}: windows and subsets of real light paths that put each record pattern of the
    linked decoder in place; check() asserts from the blob itself that the pattern is there"""
    bigblob = hip.pack_photons_linked(big.ph, hip.MaterialTable())
    kind = kinds_of(bigblob)
    F, E, CH = abi.GVPM_LINKED_FULL, abi.GVPM_LINKED_EMIT, abi.GVPM_LINKED_CHAIN
    out = {}

    def counts(blob):
        hd = hip.linked_header(blob)
        return hd["n"], hd["n_full"], hd["n_emit"], hd["n_chain"]

    def records(blob):
        hd = hip.linked_header(blob)
        full = np.frombuffer(blob[hd["off_full"]:hd["off_full"] + 76 * hd["n_full"]].tobytes(), abi.PHOTON_PACKED_DTYPE)
        emit = np.frombuffer(blob[hd["off_emit"]:hd["off_emit"] + 48 * hd["n_emit"]].tobytes(), abi.PHOTON_EMIT_DTYPE)
        chain = np.frombuffer(blob[hd["off_chain"]:hd["off_chain"] + 40 * hd["n_chain"]].tobytes(), abi.PHOTON_CHAIN_DTYPE)
        return hd, full, emit, chain

    for n in COUNTS:
        out[f"window {n}"] = (window(big.ph, n, n), None)
    out["window large"] = (big.ph.subset(np.arange(LARGE)), None)

    # every photon full: parents that are not emitters, shuffled (no photon follows its parent); zero normals (medium parents)
    rng = np.random.default_rng(11)
    idx = np.nonzero((big.ph.flags & 3) != abi.GVPM_PARENT_EMITTER)[0]
    out["all full"] = (big.ph.subset(rng.permutation(idx)[:5000]),
                       lambda b, t: counts(b)[1] == counts(b)[0] and (records(b)[1]["parent_n_oct"] == OCT_ZERO).any())
    # every photon an emit record
    out["all emit"] = (big.ph.subset(np.nonzero(kind == E)[0][:5000]), lambda b, t: counts(b)[2] == counts(b)[0])

    # chain-dominated: every chain photon with the photon before it (so that it still chains)
    keep = np.nonzero((kind == CH) | (np.roll(kind, -1) == CH))[0][:9001]
    out["chain dominated"] = (big.ph.subset(keep), lambda b, t: 2 * counts(b)[3] > counts(b)[0])

    # a chain at photon 1, chains straddling 63 / 64 and 255 / 256, each behind a chain (parent_wi from two positions)
    cc = set((np.nonzero((kind[1:] == CH) & (kind[:-1] == CH))[0] + 1).tolist())
    a = next(i - 64 for i in sorted(cc) if i >= 64 and i - 64 + 256 in cc and kind[i - 64 + 1] == CH)

    def straddle(b, t):
        k = kinds_of(b)
        return k[1] == CH and k[63] == CH and k[64] == CH and k[255] == CH and k[256] == CH
    out["chains at 1, 63/64, 255/256"] = (big.ph.subset(np.arange(a, a + 301)), straddle)

    # two scenes' light paths in one blob: emitter index n_emitters - 1, material index table_n - 1 (both the second scene's)
    other = cases.make_case("laser", 16, 12, 4000, 3.0).ph
    both = abi.Photons(0)
    both.n = 6000
    for k in FIELDS:
        setattr(both, k, np.ascontiguousarray(np.concatenate([getattr(big.ph, k)[:3000], getattr(other, k)[:3000]])))

    def last_entries(b, t):
        hd, full, emit, chain = records(b)
        return (hd["n_emitters"] >= 2 and ((emit["flags"] >> 16) == hd["n_emitters"] - 1).any()
                and (((chain["flags"] >> 16) == t.n - 1).any() or (full["material"] == t.n - 1).any()))
    out["two scenes"] = (both, last_entries)
    return out


def test_linked_records(big):
    t = hip.MaterialTable()
    hip.pack_photons_linked(big.ph.subset(np.arange(20000)), t)  # (a table for the blobs without a material of their own)
    ctx = new_ctx(big)
    for it, (name, (ph, check)) in enumerate(linked_patterns(big).items(), 1):
        blob = hip.pack_photons_linked(ph, t)
        if check is not None:
            assert check(blob, t), f"{name}: the pattern is not in the blob"
        if name == "window large":
            # the path_id bit rides in the flags of every record kind: both values of it, in each
            hd = hip.linked_header(blob)
            for off, cnt, dt in (("off_full", "n_full", abi.PHOTON_PACKED_DTYPE), ("off_emit", "n_emit", abi.PHOTON_EMIT_DTYPE),
                                 ("off_chain", "n_chain", abi.PHOTON_CHAIN_DTYPE)):
                r = np.frombuffer(blob[hd[off]:hd[off] + dt.itemsize * hd[cnt]].tobytes(), dt)
                assert set(np.unique(r["flags"] >> 7 & 1)) == {0, 1}, cnt
        ctx.upload_materials(t)
        ctx.upload_photons_linked(blob)
        ctx.upload_camera_beams(big.rays)
        ctx.gather(it, big.nb)
        assert_photons_bits(ctx.download_photons(ph.n), hip.unpack_photons_linked(blob, t), f"linked records, {name}")
    ctx.stats()  # nothing reported
    ctx.close()


# ---- camera beam sets ------------------------------------------------------------------------------------------------

def with_invalid_rays(rays):
    """invalid shifted rays, some of them of length 0 (packed: a -0 length)"""
    r = rays.copy()
    r["info"][3::7, 2] &= ~np.uint32(1)
    r["info"][5::11, 4] &= ~np.uint32(1)
    r["len"][5::11, 4] = 0.0
    return r


def small_photons(c):
    return c.ph.subset(np.arange(min(c.ph.n, 500)))


def test_packed_beam_sets(frame):
    rays_all = with_invalid_rays(frame.rays)
    assert rays_all.shape[0] > 1000
    ctx = new_ctx(frame)
    for it, n in enumerate(SET_COUNTS + (rays_all.shape[0],), 1):
        rays = rays_all[:n]
        pk = hip.pack_camera_beams(rays)
        if n > 5:
            assert (pk.view(np.uint8).reshape(n, 272)[:, 64:].view(abi.RAY_PACKED_DTYPE)["len"].view(np.uint32) == 0x80000000).any()
        ctx.upload_photons(small_photons(frame))
        ctx.upload_camera_beams_packed(pk)
        ctx.gather(it, frame.nb)
        assert_rays_bits(ctx.download_camera_beams(), hip.unpack_camera_beams(pk), f"packed sets, n = {n}")
    ctx.close()


def compact_sets(c, rays):
    """compact + full records of `rays` (some sets forced full: no base ray), and what the host makes of them in the
    device's set order, and new_index"""
    rays = rays.copy()
    rays["info"][::13, 0] &= ~np.uint32(1)  # a set without a base ray travels full
    sensor = c.sc.sensor()
    comp, full, idx = hip.pack_camera_beams_compact(sensor, rays, c.sc.jitter(c.it, rays))
    return sensor, comp, full, idx


def host_compact_in_input_order(sensor, comp, full, idx):
    dec = np.concatenate([hip.unpack_camera_beams_compact(sensor, comp), hip.unpack_camera_beams(full)])
    return dec[idx]


def test_compact_beam_sets(frame):
    rays_all = with_invalid_rays(frame.rays)
    ctx = new_ctx(frame)
    ctx.upload_sensor(frame.sc.sensor())
    for it, n in enumerate(SET_COUNTS + (rays_all.shape[0],), 1):
        sensor, comp, full, idx = compact_sets(frame, rays_all[:n])
        if n > 52:
            assert comp.size > 0 and full.shape[0] > 0  # a mixed slot
        ctx.upload_photons(small_photons(frame))
        ctx.upload_camera_beams_compact(comp, full)
        ctx.gather(it, frame.nb)
        dev = ctx.download_camera_beams()
        assert dev.shape[0] == n
        # the device's set order mapped back to the input's through new_index
        assert_rays_bits(dev[idx], host_compact_in_input_order(sensor, comp, full, idx), f"compact sets, n = {n}")
    ctx.close()


# ---- pinned memory, prefetched ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["packed", "linked", "compact"])
def test_pinned_and_prefetched_uploads(big, frame, mode):
    """a pinned upload decoded by the first gather, a prefetched one by the second: each read back after its gather"""
    t = hip.MaterialTable()
    rays_all = with_invalid_rays(frame.rays)
    steps = [(window(big.ph, 4097, 1), rays_all[:257]), (window(big.ph, 257, 2), rays_all[:52])]
    sensor = frame.sc.sensor()
    pins, want = [], []
    for ph, rays in steps:
        kw = {}
        if mode == "compact":
            rays = rays.copy()
            rays["info"][::13, 0] &= ~np.uint32(1)
            kw = dict(sensor=sensor, jitter=frame.sc.jitter(frame.it, rays))
        pk = hip.PinnedPacked(ph, rays, t, linked=mode == "linked", **kw)
        pins.append(pk)
        if mode == "linked":
            wp = hip.unpack_photons_linked(hip.pack_photons_linked(ph, t), t)
        else:
            wp = hip.unpack_photons(hip.pack_photons(ph, t), t)
        if mode == "compact":
            s, comp, full, idx = sensor, *hip.pack_camera_beams_compact(sensor, rays, kw["jitter"])
            assert np.array_equal(idx, pk.new_index) and full.shape[0] > 0
            wr = (host_compact_in_input_order(s, comp, full, idx), idx)
        else:
            wr = (hip.unpack_camera_beams(hip.pack_camera_beams(rays)), None)
        want.append((wp, wr))
    ctx = new_ctx(frame)  # (the film the beam sets' pixels belong to)
    if mode == "compact":
        ctx.upload_sensor(sensor)
    ctx.upload_materials(t)
    ctx.upload_pinned_packed(pins[0])
    ctx.prefetch_packed(pins[1])
    for it in (1, 2):
        ctx.gather(it, frame.nb)
        wp, (wr, idx) = want[it - 1]
        assert_photons_bits(ctx.download_photons(wp.n), wp, f"{mode}, pinned step {it}")
        dev = ctx.download_camera_beams()
        assert_rays_bits(dev if idx is None else dev[idx], wr, f"{mode}, pinned step {it}")
    ctx.stats()
    ctx.close()
    for p in pins:
        p.close()


# ---- malformed linked blobs --------------------------------------------------------------------------------------------

BAD = ["kind3", "full_base+1", "full_base-1", "emit_base+1", "emit_base-1", "full_base_past_count", "n_chain_vs_kinds",
       "n_2^26_wrapped", "truncated"]


def run_valid(ctx, c, blob, t):
    ctx.upload_materials(t)
    ctx.upload_photons_linked(blob)
    ctx.upload_camera_beams(c.rays)
    ctx.gather(1, c.nb)
    n = hip.linked_header(blob)["n"]
    return ctx.download_accum().astype(np.float64), ctx.stats(), ctx.download_photons(n)


@pytest.mark.parametrize("name", BAD)
def test_device_refuses_what_the_host_definition_refuses(name):
    """header defects fail at upload (GVPM_ERR_INVALID_ARG); body defects make the next gvpm_get_stats fail
    (GVPM_ERR_STATE).  After a reset the handle gathers a valid blob exactly as a fresh one does."""
    c = cases.make_case("cbox", 16, 12, 3000, 3.0)
    blob, t = M.linked_case()
    bad, where = M.malformed_blobs(blob)[name]
    with pytest.raises(hip.GvpmError):
        M.host_unpack(bad, t)
    ctx = new_ctx(c)
    ctx.upload_materials(t)
    if where == "header":
        with pytest.raises(hip.GvpmError) as e:
            ctx.upload_photons_linked(bad)
        assert e.value.code == abi.GVPM_ERR_INVALID_ARG
    else:
        ctx.upload_photons_linked(bad)
        ctx.upload_camera_beams(c.rays)
        ctx.gather(1, c.nb)
        with pytest.raises(hip.GvpmError) as e:
            ctx.stats()
        assert e.value.code == abi.GVPM_ERR_STATE and "malformed" in str(e.value)
    ctx.reset()
    a1, s1, p1 = run_valid(ctx, c, blob, t)
    ctx.close()
    fresh = new_ctx(c)
    a2, s2, p2 = run_valid(fresh, c, blob, t)
    fresh.close()
    assert s1["evaluations"] > 0
    assert s1 == s2
    assert_photons_bits(p1, hip.unpack_photons_linked(blob, t), f"{name}: the valid blob after it")
    assert_photons_bits(p1, p2, f"{name}: against a fresh handle")
    assert np.abs(a1 - a2).max() <= 2e-5 * np.abs(a2).max()  # (the order of the atomics)
