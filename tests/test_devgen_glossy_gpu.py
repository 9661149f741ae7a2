"""The device generators over glossy scenes (gvpm_devgen_create_ex; csrc/synth_device_glossy.hip) against the host generators, which run
the same text (host/synth_core.h) sequentially: same photon count, same path count, same order; `flags` and `path_id` bit-equal -- so
every component selection, every sampled lobe type and every depth agree --, the float arrays (parent_g, the table index, among them)
equal up to the last bits of libm's pow / atan / exp / log / sin / cos, by the closed set's own tolerances (tests/test_devgen_gpu.py)."""
import numpy as np
import pytest

import cases
import devgen_glossy_cases as DG
import oracle_lib as O
from gvpm_amd import abi, hip
from test_devgen_gpu import close, photons_from_dev

pytestmark = pytest.mark.gpu


def assert_records_match(got, ref):
    assert np.array_equal(got.flags, ref.flags) and np.array_equal(got.path_id, ref.path_id)
    # (the table index travels as a float: equal as the integer it is)
    gl = (ref.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    assert np.array_equal(got.parent_g[gl], ref.parent_g[gl])
    for k in abi.PHOTON_VEC3 + abi.PHOTON_F1:
        assert close(getattr(got, k), getattr(ref, k)), k


@pytest.mark.parametrize("scene", DG.SCENES + DG.MIXTURES + DG.ROTATED)
def test_photons_match_the_host_generator(scene):
    sc = DG.scene(scene, 32, 24)
    g = hip.DeviceGenerator(sc, glossy=True)
    cap = 9000
    for it in (1, 3):
        ref, nb_ref = sc.shoot_photons(it, cap)
        soa, nb = g.shoot_photons(it, cap)
        assert int(soa.n) == ref.n == cap and nb == nb_ref
        assert ((ref.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF).sum() > 300
        assert_records_match(photons_from_dev(g, soa), ref)
    g.close()


@pytest.mark.parametrize("scene", [f[0] for f in DG.FAMILIES.values()] + ["cbox_mixture"])
def test_beams_and_end_normals_match_the_host_generator(scene):
    sc = DG.scene(scene, 32, 24)
    g = hip.DeviceGenerator(sc, glossy=True)
    cap = 5000
    for it in (1, 3):
        ref, en_ref, nb_ref = sc.shoot_beams(it, cap)
        soa, en_ptr, nb = g.shoot_beams(it, cap)
        assert int(soa.n) == ref.n and nb == nb_ref
        assert_records_match(photons_from_dev(g, soa), ref)
        assert close(g.read(en_ptr, 3 * ref.n, np.float32).reshape(-1, 3), en_ref)
    g.close()


@pytest.mark.parametrize("scene", ["cbox_conductor", "cbox_roughglass", "cbox_mixture"])
def test_min_depth_two_matches_the_host_generator(scene):
    """The walk's minDepth = 2 (SynthScene.set_min_depth -> gvpm_devgen_scene.min_depth), what the G-Beams unbiasedness cases shoot with:
    no record is reconnected from the emitter, and device and host agree as at minDepth = 0 -- beams + end normals, and photons."""
    sc = DG.scene(scene, 32, 24)
    sc.set_min_depth(2)
    assert sc.devgen_scene().min_depth == 2 and sc.params().min_depth == 2
    g = hip.DeviceGenerator(sc, glossy=True)
    ref, en_ref, nb_ref = sc.shoot_beams(2, 5000)
    soa, en_ptr, nb = g.shoot_beams(2, 5000)
    assert int(soa.n) == ref.n and nb == nb_ref
    assert ref.n > 1000 and ((ref.flags & 3) != abi.GVPM_PARENT_EMITTER).all()
    assert_records_match(photons_from_dev(g, soa), ref)
    assert close(g.read(en_ptr, 3 * ref.n, np.float32).reshape(-1, 3), en_ref)
    ref, nb_ref = sc.shoot_photons(2, 9000)
    soa, nb = g.shoot_photons(2, 9000)
    assert int(soa.n) == ref.n == 9000 and nb == nb_ref
    assert ((ref.flags & 3) != abi.GVPM_PARENT_EMITTER).all()
    assert_records_match(photons_from_dev(g, soa), ref)
    g.close()


@pytest.mark.parametrize("scene", ["cbox_phong", "cbox_roughglass", "cbox_mixture_rot"])
def test_camera_beams_match_the_host_generator(scene):
    sc = DG.scene(scene, 44, 36)
    g = hip.DeviceGenerator(sc, glossy=True)
    ref = sc.camera_beams(2)
    ptr, n = g.camera_beams(2)
    assert n == ref.shape[0] and n > 0
    got = g.read(ptr, n * 5, abi.CAMERA_RAY_DTYPE).reshape(n, 5)
    for name in abi.CAMERA_RAY_DTYPE.names:
        a, b = got[name], ref[name]
        if a.dtype.kind == "f":
            assert close(a, b), name
        else:
            assert np.array_equal(a, b), name
    g.close()


def test_gather_on_device_generated_conductor_inputs_matches_the_oracle():
    """End to end without PCIe over a kind the fp64 oracle states: device generators -> gvpm_upload_*_dev -> gvpm_upload_bsdfs -> gather;
    the oracle runs on the very inputs the device produced (downloaded): evaluations exact, the existing end-to-end test's L2 bar."""
    c = cases.make_case("cbox_conductor", 32, 28, 10, 3.0)
    g = hip.DeviceGenerator(c.sc, glossy=True)
    soa, nb = g.shoot_photons(1, 20000)
    rptr, nsets = g.camera_beams(1)
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ctx.upload_bsdfs(c.bsdfs)
    ctx.upload_photons_dev(soa)
    ctx.upload_camera_beams_dev(rptr, nsets)
    r = ctx.radius()
    ctx.gather(1, nb)
    acc = ctx.download_accum()
    st = ctx.stats()
    ctx.close()
    ph = photons_from_dev(g, soa)
    assert ((ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF).sum() > 1000
    rays = g.read(rptr, nsets * 5, abi.CAMERA_RAY_DTYPE).reshape(nsets, 5)
    ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, ph, rays, r, 1, nb, 64, use_accel=False)
    assert st["evaluations"] == cnt["evaluations"] > 1000
    lum = max(ref[..., 0:3].mean(), 1e-30)
    assert float(np.sqrt(((acc.astype(np.float64) - ref) ** 2).mean()) / lum) < 1e-4
    g.close()


def test_a_lambertian_scene_takes_the_closed_set_kernels():
    """glossy=True on plain cbox: no material above the mirror, so the generator launches the closed set's kernels -- outputs bit-equal to
    a generator made by gvpm_devgen_create."""
    from gvpm_amd.host import SynthScene
    sc = SynthScene("cbox", 32, 24)
    a, b = hip.DeviceGenerator(sc), hip.DeviceGenerator(sc, glossy=True)
    for shoot in ("photons", "beams"):
        outs = []
        for g in (a, b):
            if shoot == "photons":
                soa, nb = g.shoot_photons(2, 9000)
                en = None
            else:
                soa, en_ptr, nb = g.shoot_beams(2, 5000)
                en = g.read(en_ptr, 3 * int(soa.n), np.uint32)
            outs.append((photons_from_dev(g, soa), nb, en))
        (pa, na, ea), (pb, nb_, eb) = outs
        assert na == nb_ and pa.n == pb.n
        for k in abi.PHOTON_VEC3 + abi.PHOTON_F1 + abi.PHOTON_U1:
            assert np.array_equal(getattr(pa, k).view(np.uint32), getattr(pb, k).view(np.uint32)), k
        assert ea is None or np.array_equal(ea, eb)
    (pa, na), (pb, nb_) = a.camera_beams(2), b.camera_beams(2)
    assert na == nb_ > 0
    assert a.read(pa, na * 5 * 64, np.uint8).tobytes() == b.read(pb, nb_ * 5 * 64, np.uint8).tobytes()
    a.close()
    b.close()
