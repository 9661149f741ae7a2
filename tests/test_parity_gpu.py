"""Parity tests proper: the HIP path (through the C ABI) against the fp64 CPU oracle on the same
seeded inputs.  Run on the GPU box with `pytest -m gpu`.

Bars (BASELINE.md "Parity bar"):
  * evaluation count == oracle count exactly (the device evaluates the reference hit
    predicate in fp64 without contraction);
  * per-pixel L2 of the 27 accumulators / throughput / dx / dy against the fp64 oracle,
    normalised by the mean reference luminance, < 1e-3 (measured ~1e-6; asserted < 1e-4);
  * per entry of the 27 accumulators, where the device sees the oracle's inputs bit for bit (exact=True): exactly 0 wherever
    the fp64 oracle is, and p50 / p90 / p99 of the relative error within 4x / 4x / 8x of the fp32 oracle's own on the same
    inputs (entry_parity.py A and B; the tail bar C on the admitted inputs of test_entry_parity_gpu.py).
"""
import os

import numpy as np
import pytest

import cases
import oracle_lib as O
from entry_parity import assert_entry_parity
from gvpm_amd import abi, hip

pytestmark = pytest.mark.gpu
TOL = 1e-4
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def l2(a, ref, lum):
    return float(np.sqrt(((a.astype(np.float64) - ref) ** 2).mean()) / lum)


def device_gather(c, rays=None, ph=None, p=None, iters=None, beams_per_wave=None):
    """Returns (accum float32 [H,W,27], stats, film tuple) after running the case on the device."""
    p = c.p if p is None else p
    old = os.environ.get("GVPM_BEAMS_PER_WAVE")
    if beams_per_wave:
        os.environ["GVPM_BEAMS_PER_WAVE"] = str(beams_per_wave)
    try:
        ctx = hip.Context(p, device=0)
    finally:
        if beams_per_wave:
            if old is None:
                os.environ.pop("GVPM_BEAMS_PER_WAVE")
            else:
                os.environ["GVPM_BEAMS_PER_WAVE"] = old
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    cases.upload_bsdfs(ctx, c)
    ctx.upload_photons(c.ph if ph is None else ph)
    ctx.upload_camera_beams(c.rays if rays is None else rays)
    assert abs(ctx.radius() - c.r) == 0.0
    ctx.gather(c.it, c.nb)
    acc = ctx.download_accum()
    st = ctx.stats()
    film = ctx.download_film(c.it, True)
    ctx.close()
    return acc, st, film


def check(c, p=None, rays=None, ph=None, use_accel=False, exact=True, **kw):
    p = c.p if p is None else p
    acc, st, film = device_gather(c, rays=rays, ph=ph, p=p, **kw)
    ref, cnt, _ = O.gather_bre(p, c.m, c.tris, c.ph if ph is None else ph, c.rays if rays is None else rays, c.r,
                               c.it, c.nb, 64, use_accel=use_accel)
    lum = max(ref[..., 0:3].mean(), 1e-30)
    assert st["evaluations"] == cnt["evaluations"]
    # round 5: exact -- every decision of a shift is banded and the undecided shifts are evaluated in fp64 (exact_shift.hip).
    # exact=False keeps the bar of rounds 1-4 (which shift a borderline evaluation takes may flip with the fp32 re-derivation
    # of t': at most 2e-6 of the shifts) for callers that feed the device inputs the oracle does not see bit for bit
    for k in ("null_shifts", "diffuse_shifts", "failed_shifts"):
        assert abs(st[k] - cnt[k]) <= (0 if exact else max(2, 2e-6 * 4 * cnt["evaluations"])), (k, st, cnt)
    err = l2(acc, ref, lum)
    assert err < TOL, err
    if exact:
        # per entry, in units of the reference's own fp32 noise on these inputs (entry_parity.py): zeros and bulk; the tail bar
        # needs admitted inputs (entry_cases.py)
        r32, _, _ = O.gather_bre(p, c.m, c.tris, c.ph if ph is None else ph, c.rays if rays is None else rays, c.r, c.it, c.nb, 32,
                                 use_accel=use_accel)
        assert_entry_parity(acc, ref, r32, lum, tail=False, inputs=False)
    rthr, rdx, rdy = O.assemble(ref, c.it, True)
    for a, b in zip(film, (rthr, rdx, rdy)):
        assert l2(a, b, lum) < TOL
    return acc, ref, st


@pytest.fixture(scope="module")
def case():
    return cases.make_case("cbox", 40, 36, 30000, 2.5)


@pytest.mark.parametrize("scene", ["cbox", "cbox_hg"])
@pytest.mark.parametrize("bpw", [16, 32, 64])
def test_bre3d_matches_fp64_oracle(scene, bpw):
    c = cases.make_case(scene, 40, 36, 30000, 2.5)
    acc, ref, st = check(c, beams_per_wave=bpw)
    assert st["evaluations"] > 10000


def test_bre3d_matches_reference_bvh_walk(case):
    """Against the literal kd-tree -> BVH traversal of the reference (3D: same hit set)."""
    check(case, use_accel=True)


@pytest.mark.parametrize("kw", [
    dict(use_mis=0), dict(power_heuristic=1), dict(path_set=0), dict(use_shift_null=0),
    dict(visibility_as_written=0), dict(debug_shift=abi.GVPM_SHIFT_DIFFUSE), dict(debug_shift=abi.GVPM_SHIFT_NULL),
    dict(debug_shift=abi.GVPM_SHIFT_MANIFOLD), dict(max_depth=3), dict(min_depth=3), dict(max_depth=0),
    dict(lighting_interaction_mode=abi.GVPM_SURF2MEDIA), dict(lighting_interaction_mode=abi.GVPM_MEDIA2MEDIA),
    dict(bsdf_interaction_mode=0x00008),
])
def test_flag_sweep(case, kw):
    p = case.p.copy()
    for k, v in kw.items():
        setattr(p, k, v)
    check(case, p=p)


def test_bre2d_matches_own_box_oracle():
    c = cases.make_case("cbox", 40, 36, 30000, 2.5, vol_technique=abi.GVPM_VOL_BRE2D, use_shift_null=0)
    check(c, use_accel=False)
    # the reference BVH adds tree-dependent photons beyond the beam end (oracle header): bounded
    acc, st, _ = device_gather(c)
    ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=True)
    assert 0 <= cnt["evaluations"] - st["evaluations"] <= 0.01 * st["evaluations"]


@pytest.mark.parametrize("name", ["cbox_bre3d", "cbox_hg_bre3d", "cbox_bre2d"])
def test_golden_fixtures(name):
    import golden_io
    g = golden_io.load(os.path.join(GOLD, name + ".npz"))
    g.sc = None
    acc, st, _ = device_gather(g)
    assert st["evaluations"] == g.evaluations
    assert l2(acc, g.accum, g.accum[..., 0:3].mean()) < TOL


def test_three_iterations_apa_and_radius_schedule():
    c = cases.make_case("cbox", 32, 32, 20000, 3.0)
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ref = None
    scale = c.p.initial_scale_volume
    total = 0
    for it in (1, 2, 3):
        ph, nb = c.sc.shoot_photons(it, 20000)
        rays = c.sc.camera_beams(it)
        r = ctx.radius()
        assert r == cases.radius_of(c.p, np.float32(scale))
        ctx.upload_photons(ph)
        ctx.upload_camera_beams(rays)
        ctx.gather(it, nb)
        ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, ph, rays, r, it, nb, 64, use_accel=False, accum=ref)
        total += cnt["evaluations"]
        scale = np.float32(O.scale_volume_apa(float(scale), it, float(c.p.alpha), c.p.vol_technique))
    acc = ctx.download_accum()
    assert ctx.stats()["evaluations"] == total
    assert l2(acc, ref, ref[..., 0:3].mean()) < TOL
    ctx.reset()
    assert ctx.radius() == c.r and not ctx.download_accum().any()
    ctx.close()


def test_empty_and_ragged_inputs(case):
    c = case
    none = c.ph.subset(np.zeros(0, np.int64))
    acc, st, _ = device_gather(c, ph=none)
    assert st["evaluations"] == 0 and not acc.any()
    acc, st, _ = device_gather(c, rays=c.rays[:0])
    assert st["evaluations"] == 0 and not acc.any()
    # ragged: a handful of sets in random order, one pixel addressed by three sets, invalid shifted rays
    rng = np.random.default_rng(7)
    sel = rng.permutation(c.rays.shape[0])[:37]
    rays = c.rays[sel].copy()
    rays = np.concatenate([rays, rays[:1], rays[:1]])
    rays[3, 2]["info"] = abi.ray_info(0, 2)
    rays[5, 1:]["info"] = abi.ray_info(0, 2)
    check(c, rays=rays)
    # a single photon / a single beam
    check(c, ph=c.ph.subset(np.arange(1)))
    check(c, rays=c.rays[100:101])


def test_identical_shifted_beams_zero_gradient_on_device(case):
    c = case
    rays = cases.rays_shift_equals_base(c.rays)
    acc, ref, st = check(c, rays=rays)
    H, W = acc.shape[:2]
    flux, wt = acc[..., 0:3], acc[..., 15:27].reshape(H, W, 4, 3)
    assert np.allclose(wt[:-1, :-1], 0.5 * flux[:-1, :-1, None, :], rtol=1e-5, atol=1e-9)


def test_dev_upload_equals_host_upload(case):
    torch = pytest.importorskip("torch")
    c = case
    acc_host, st_host, _ = device_gather(c)
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    keep, soa = [], abi.PhotonSoA()
    for k in abi.PHOTON_VEC3 + abi.PHOTON_F1 + abi.PHOTON_U1:
        a = getattr(c.ph, k)
        t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        keep.append(t)
        setattr(soa, k, t.data_ptr())
    soa.n = c.ph.n
    rt = torch.from_numpy(c.rays.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    ctx.upload_photons_dev(soa)
    ctx.upload_camera_beams_dev(rt.data_ptr(), c.rays.shape[0])
    ctx.gather(1, c.nb)
    acc = ctx.download_accum()
    assert ctx.stats()["evaluations"] == st_host["evaluations"]
    # (float atomics: the order of a pixel's sums differs from run to run, ~sqrt(terms) ulp)
    np.testing.assert_allclose(acc, acc_host, rtol=5e-5, atol=1e-6 * float(np.abs(acc_host).max()))
    out = torch.zeros(acc.size, dtype=torch.float32, device="cuda")
    ctx.download_accum_dev(out.data_ptr())
    assert np.array_equal(out.cpu().numpy().reshape(acc.shape), acc)
    ctx.close()


def test_error_behaviour(case):
    c = case
    ctx = hip.Context(c.p, device=0)
    with pytest.raises(hip.GvpmError) as e:
        ctx.gather(1, 10)
    assert e.value.code == abi.GVPM_ERR_STATE
    ctx.upload_medium(c.m)
    bad = c.sc.medium()
    bad.sigma_t[0] = 2.0
    with pytest.raises(hip.GvpmError) as e:
        ctx.upload_medium(bad)
    assert e.value.code == abi.GVPM_ERR_UNSUPPORTED
    ctx.upload_scene(*c.tris)
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(c.rays)
    with pytest.raises(hip.GvpmError):
        ctx.gather(0, 10)
    ctx.close()
    p = c.p.copy()
    p.vol_technique = abi.GVPM_BEAM_BEAM_3D_NAIVE  # SAssert(false) in the reference's BeamKernelRecord::eval
    ctx = hip.Context(p, device=0)
    ctx.upload_medium(c.m)
    ctx.upload_scene(*c.tris)
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(c.rays)
    with pytest.raises(hip.GvpmError) as e:
        ctx.gather(1, 10)
    assert e.value.code == abi.GVPM_ERR_UNSUPPORTED
    ctx.close()


def bad_medium(c, **kw):
    m = c.sc.medium()
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(m, k)[v[0]] = v[1]
        else:
            setattr(m, k, v)
    return m


@pytest.mark.parametrize("kw", [
    dict(g=1.0), dict(g=-1.0), dict(g=1.5), dict(g=float("nan")), dict(g=float("inf")),
    dict(medium_sampling_weight=0.0), dict(medium_sampling_weight=-0.5), dict(medium_sampling_weight=1.5),
    dict(medium_sampling_weight=float("nan")),
    dict(sigma_s=(1, -0.25)), dict(sigma_s=(2, 1.5)), dict(sigma_s=(0, float("nan"))), dict(sigma_s=(1, float("inf"))),
    dict(sigma_a=(2, float("nan"))), dict(sigma_t=(1, float("nan"))), dict(sigma_t=(0, float("inf"))),
], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()).replace(" ", ""))
def test_upload_medium_refuses_out_of_range_fields(case, kw):
    """what the kernels divide by (pdfSuccess = sigma_t e msw, HG's 1 + g^2 + 2 g cos) and what no medium is"""
    ctx = hip.Context(case.p, device=0)
    try:
        with pytest.raises(hip.GvpmError) as e:
            ctx.upload_medium(bad_medium(case, **kw))
        assert e.value.code == abi.GVPM_ERR_INVALID_ARG, (kw, e.value)
        assert "medium" in str(e.value)
        with pytest.raises(hip.GvpmError) as e:      # (a refused medium is not kept)
            ctx.gather(1, 10)
        assert e.value.code == abi.GVPM_ERR_STATE
    finally:
        ctx.close()


def test_upload_medium_accepts_the_trial_media(case):
    import medium_cases
    ctx = hip.Context(case.p, device=0)
    try:
        for name in medium_cases.MEDIA:
            c = cases.Case()
            c.m = case.sc.medium()
            ctx.upload_medium(medium_cases.apply(c, name).m)
        ends = bad_medium(case, g=0.999, medium_sampling_weight=1e-3)   # the ends of the ranges; sigma_s = 0 and = sigma_t
        ends.sigma_s[0], ends.sigma_s[1] = 0.0, ends.sigma_t[1]
        ctx.upload_medium(ends)
    finally:
        ctx.close()


def test_full_size_properties():
    """BASELINE configs[1] size (512x512, 1M photons): size-independent properties + a windowed
    oracle comparison of the same frame."""
    c = cases.make_case("cbox", 512, 512, 1000000, 1.0)
    acc, st, _ = device_gather(c)
    assert st["evaluations"] > 10_000_000
    # (1) a 48x48 window of the same frame against the fp64 oracle (full photon map)
    px, py = cases.pixels_of(c.rays)
    sel = (px >= 232) & (px < 280) & (py >= 232) & (py < 280)
    ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, np.ascontiguousarray(c.rays[sel]), c.r, 1, c.nb, 64,
                               use_accel=True)
    win, rwin = acc[232:280, 232:280], ref[232:280, 232:280]
    assert l2(win, rwin, rwin[..., 0:3].mean()) < TOL
    # (2) run-to-run reproducibility
    acc2, st2, _ = device_gather(c)
    assert st2["evaluations"] == st["evaluations"]
    assert np.allclose(acc2, acc, rtol=2e-5, atol=1e-9)
    # (3) linearity in the photon flux
    ph2 = c.ph.subset(np.arange(c.ph.n))
    ph2.flux = ph2.flux * 2
    ph2.prefix_w = ph2.prefix_w * 2
    acc3, st3, _ = device_gather(c, ph=ph2)
    assert st3["evaluations"] == st["evaluations"]
    assert np.allclose(acc3, 2 * acc, rtol=2e-5, atol=1e-9)
    # (4) weights in [0,1]: 0 <= weighted <= flux
    H, W = acc.shape[:2]
    flux, wt = acc[..., 0:3], acc[..., 15:27].reshape(H, W, 4, 3)
    assert (wt >= 0).all() and (wt <= flux[:, :, None, :] * (1 + 1e-4) + 1e-12).all()
    # (5) border rule
    assert np.allclose(wt[H - 1, :, abi.GVPM_TOP], flux[H - 1], rtol=1e-4, atol=1e-12)


def test_grid_bounds_carried_from_previous_photon_set():
    """The grid of a step is sized by the previous step's photon bounds (one host sync per step):
    photons outside it sit in the border cells and must still be found, bit for bit."""
    c = cases.make_case("cbox", 32, 28, 20000, 3.0)
    pos = c.ph.pos
    small = np.nonzero((np.abs(pos[:, 0]) < 0.3) & (np.abs(pos[:, 1]) < 0.3) & (np.abs(pos[:, 2]) < 0.3))[0]
    assert 200 < small.size < c.ph.n // 2
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ctx.upload_camera_beams(c.rays)
    ctx.upload_photons(c.ph.subset(small))   # step 1: a small box in the middle -> small cached bounds
    ctx.gather(1, c.nb)
    ctx.reset()
    ctx.upload_photons(c.ph)                 # step 2: the full set, most of it outside the cached bounds
    ctx.gather(1, c.nb)
    acc = ctx.download_accum()
    st = ctx.stats()
    ctx.close()
    ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    assert st["evaluations"] == cnt["evaluations"]
    assert l2(acc, ref, max(ref[..., 0:3].mean(), 1e-30)) < TOL


@pytest.mark.parametrize("as_written", [1, 0])
def test_many_occluders_walk_the_bvh(as_written):
    """896 triangles tessellating the same box: more than 254 occluders (and the intended-visibility
    mode) send every shadow ray through the occluder BVH; the surface is unchanged, so the result
    must match the oracle on the coarse scene."""
    c = cases.make_case("cbox", 32, 28, 20000, 3.0, visibility_as_written=as_written)
    fine = cases.tessellate(c.tris, 3)
    assert fine[0].shape[0] > 254
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*fine)
    ctx.upload_medium(c.m)
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(c.rays)
    ctx.gather(1, c.nb)
    acc = ctx.download_accum()
    st = ctx.stats()
    ctx.close()
    ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    assert st["evaluations"] == cnt["evaluations"]
    # rays grazing the new interior edges may change a handful of shadow tests
    for k in ("diffuse_shifts", "failed_shifts"):
        assert abs(st[k] - cnt[k]) <= max(4, 2e-4 * cnt["diffuse_shifts"]), (k, st, cnt)
    assert l2(acc, ref, max(ref[..., 0:3].mean(), 1e-30)) < 1e-3


@pytest.mark.parametrize("levels,seps", [(1, 0.05), (3, 0.01), (3, 0.2), (7, 0.0002)])
def test_near_occluder_list_formats(levels, seps):
    """The as-written shadow segment (first ShadowEpsilon of the reconnection distance) is served by per-photon
    near-occluder lists: 8-bit indices up to 253 occluders, 16-bit beyond, extension lists when a list outgrows
    its inline slots.  A large ShadowEpsilon makes the lists long: extension lists in the narrow format (56
    occluders) and in the wide one (896), and at 0.2 more than the extension array holds, which sends the step
    through the BVH kernels; 229 376 occluders are beyond 16-bit indices (every list an extension list).  The result must stay the oracle's, which tests every occluder."""
    c = cases.make_case("cbox", 32, 28, 20000, 3.0, shadow_epsilon=seps)
    fine = cases.tessellate(c.tris, levels) if levels else c.tris
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*fine)
    ctx.upload_medium(c.m)
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(c.rays)
    ctx.gather(1, c.nb)
    acc = ctx.download_accum()
    st = ctx.stats()
    ctx.close()
    ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    assert st["evaluations"] == cnt["evaluations"]
    assert cnt["failed_shifts"] > 0
    for k in ("diffuse_shifts", "failed_shifts"):
        assert abs(st[k] - cnt[k]) <= max(4, 2e-4 * cnt["diffuse_shifts"]), (k, st, cnt)
    assert l2(acc, ref, max(ref[..., 0:3].mean(), 1e-30)) < 1e-3


def test_near_occluder_grid_finds_what_the_bvh_query_finds(monkeypatch):
    """Above 64 occluders the near-occluder lists come from the occluder grid (grid_build.hip: near_grid_kernel);
    GVPM_NEAR_GRID=0 keeps the BVH point query they came from before.  Same lists => the same shadow-ray outcomes: every
    counter equal and the accumulators equal up to the order of the float atomics."""
    c = cases.make_case("cbox", 32, 28, 20000, 3.0, shadow_epsilon=0.01)
    fine = cases.tessellate(c.tris, 3)  # 896 occluders: 16-bit lists
    out = []
    for flag in ("1", "0"):
        monkeypatch.setenv("GVPM_NEAR_GRID", flag)
        ctx = hip.Context(c.p, device=0)
        ctx.upload_scene(*fine)
        ctx.upload_medium(c.m)
        ctx.upload_photons(c.ph)
        ctx.upload_camera_beams(c.rays)
        ctx.gather(1, c.nb)
        out.append((ctx.download_accum(), ctx.stats()))
        ctx.close()
    (a1, s1), (a0, s0) = out
    for k in ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts"):
        assert s1[k] == s0[k], (k, s1, s0)
    assert s1["failed_shifts"] > 0
    np.testing.assert_allclose(a1, a0, rtol=5e-5, atol=1e-6 * float(np.abs(a0).max()))


def test_row_sharded_film_and_moving_shards():
    """A handle only clears / folds the film rows it has touched since the last reset (image-sharded ranks own
    a fraction of the frame): two shard handles must add up to the full-frame result, and a handle whose beam
    sets move to other rows must still apply the APA fold to the rows it left."""
    c = cases.make_case("cbox", 32, 28, 20000, 3.0)
    py = cases.pixels_of(c.rays)[1]
    top, bot = c.rays[py < 14], c.rays[py >= 14]
    full, _, _ = device_gather(c)
    a1, _, _ = device_gather(c, rays=top)
    a2, _, _ = device_gather(c, rays=bot)
    assert np.allclose(a1 + a2, full, rtol=1e-5, atol=1e-9)
    assert not a1[14:].any() and not a2[:14].any()
    # iteration 1 on the top rows, iteration 2 on the bottom rows, same handle
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(top)
    r1 = ctx.radius()
    ctx.gather(1, c.nb)
    ctx.upload_camera_beams(bot)
    r2 = ctx.radius()
    ctx.gather(2, c.nb)
    acc = ctx.download_accum()
    ctx.close()
    ref, _, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, top, r1, 1, c.nb, 64, use_accel=False)
    ref, _, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, bot, r2, 2, c.nb, 64, use_accel=False, accum=ref)
    assert l2(acc, ref, max(ref[..., 0:3].mean(), 1e-30)) < TOL
    assert np.allclose(acc[:14], 0.5 * a1[:14], rtol=1e-5, atol=1e-9)  # the rows left behind decayed by (it-1)/it


def test_partial_films_of_interleaved_shards_sum_to_the_frames_film():
    """SURVEY 8e's collective: every rank runs computeGradient over its own accumulators (zero elsewhere) and the
    3 film planes are summed.  dx, dy and the non-reusePrimal throughput add one term per rank at most twice per
    pixel, so the sum must be BIT-identical to the film of the summed accumulators."""
    import torch
    c = cases.make_case("cbox", 36, 28, 20000, 3.0)
    world, n = 3, 36 * 28 * 3
    accs, films = [], []
    for rank in range(world):
        rays = c.sc.camera_beams_interleaved(c.it, world, rank)
        ctx = hip.Context(c.p, device=0)
        ctx.upload_scene(*c.tris)
        ctx.upload_medium(c.m)
        ctx.upload_photons(c.ph)
        ctx.upload_camera_beams(rays)
        ctx.gather(c.it, c.nb)
        accs.append(ctx.download_accum())
        t = torch.zeros(3 * n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the film kernel on the context's
        ctx.download_film_dev(c.it, t.data_ptr(), reuse_primal=False)
        ctx.synchronize()
        films.append(t.cpu().numpy())
        ctx.close()
    yy, xx = np.mgrid[0:28, 0:36]
    owner = ((yy // 4) * 9 + xx // 4) % world
    for rank in range(world):
        assert not accs[rank][owner != rank].any() and accs[rank][owner == rank].any()
    total = accs[0] + accs[1] + accs[2]  # disjoint supports: exact
    # computeGradient in fp32 exactly as film_kernel associates it (gvpm.cpp:1223,1266); slots: 0 flux,
    # 1+i shifted, 5+i weighted, i = L R T B
    sh, wt = total[..., 3:15].reshape(28, 36, 4, 3), total[..., 15:27].reshape(28, 36, 4, 3)
    dx = sh[:, :, 1] - wt[:, :, 1]
    dx[:, :-1] += wt[:, 1:, 0] - sh[:, 1:, 0]
    dy = sh[:, :, 2] - wt[:, :, 2]
    dy[:-1] += wt[1:, :, 3] - sh[1:, :, 3]
    fsum = (films[0] + films[1]) + films[2]
    for k, ref in enumerate((total[..., 0:3], dx, dy)):
        got = fsum[k * n:(k + 1) * n].reshape(28, 36, 3)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (k, len(bad), bad[:6].tolist(), [(got[tuple(b)], ref[tuple(b)]) for b in bad[:6]])
    o = O.assemble(total, c.it, False)
    for k in range(3):
        # (fp32 sums of up to four terms against the fp64 assembly of the same accumulators)
        assert np.allclose(fsum[k * n:(k + 1) * n].reshape(28, 36, 3), o[k], rtol=1e-4, atol=1e-6 * np.abs(o[k]).max())


def test_non_consecutive_iteration_numbers_fold_like_the_reference():
    """The device keeps the running SUM over iterations; when `it` is not the successor of the previous call the
    reference's fold (mean * (it - 1) + v) / it weighs the old mean differently, and the sum has to be rescaled."""
    c = cases.make_case("cbox", 24, 20, 8000, 3.0)
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(c.rays)
    ref = None
    for it in (1, 3, 4, 9):
        r = ctx.radius()
        ctx.gather(it, c.nb)
        ref, _, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, r, it, c.nb, 64, use_accel=False, accum=ref)
    acc = ctx.download_accum()
    film = ctx.download_film(9, True)
    ctx.close()
    lum = max(ref[..., 0:3].mean(), 1e-30)
    assert l2(acc, ref, lum) < TOL
    for a, b in zip(film, O.assemble(ref, 9, True)):
        assert l2(a, b, lum) < TOL


def test_prefetched_pinned_uploads_equal_plain_uploads():
    """gvpm_host_alloc* + gvpm_prefetch_*: the copy of step N+1 is started before the gather of step N and becomes the
    current input when that gather returns -- four iterations that way must give the plain-upload accumulators, bit for
    bit (same kernels on the same inputs), and so must asynchronous uploads from pinned memory without prefetch."""
    c = cases.make_case("cbox", 40, 36, 20000, 2.5)
    data = []
    for it in range(1, 5):
        ph, nb = c.sc.shoot_photons(it, 20000 + 1000 * it)   # sizes differ: the staging slots regrow
        data.append((ph, nb, c.sc.camera_beams(it)))

    def run(mode):
        ctx = hip.Context(c.p, device=0)
        ctx.upload_scene(*c.tris)
        ctx.upload_medium(c.m)
        pinned = [(hip.PinnedPhotons(ph.n).fill(ph), nb, hip.PinnedRays(rays)) for ph, nb, rays in data] if mode != "plain" else None
        if mode == "prefetch":
            ctx.upload_pinned(pinned[0][0], pinned[0][2])
        for it, (ph, nb, rays) in enumerate(data, 1):
            if mode == "plain":
                ctx.upload_photons(ph)
                ctx.upload_camera_beams(rays)
            elif mode == "pinned":
                ctx.upload_pinned(pinned[it - 1][0], pinned[it - 1][2])
            elif it < len(data):
                ctx.prefetch(pinned[it][0], pinned[it][2])
            ctx.gather(it, nb)
        acc, st = ctx.download_accum(), ctx.stats()
        ctx.close()
        return acc, st

    ref, rst = run("plain")
    for mode in ("pinned", "prefetch"):
        acc, st = run(mode)
        assert st["evaluations"] == rst["evaluations"] > 10000
        assert np.allclose(acc, ref, rtol=2e-6, atol=0)   # (float atomics: the order of the partial sums is not fixed)
    # a second prefetch before the gather that consumes the first is a call-order error, pageable memory an argument error
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    pp, pr = hip.PinnedPhotons(data[0][0].n).fill(data[0][0]), hip.PinnedRays(data[0][2])
    ctx.prefetch(pp, pr)
    with pytest.raises(hip.GvpmError) as e:
        ctx.prefetch(pp, pr)
    assert e.value.code == abi.GVPM_ERR_STATE
    ctx.close()


@pytest.mark.parametrize("scene,W,H", [("cbox_mirror", 48, 40), ("cbox_mirror_side", 112, 84)])
@pytest.mark.parametrize("tech", [abi.GVPM_VOL_BRE3D, abi.GVPM_VOL_BRE2D])
def test_camera_paths_with_two_medium_edges(scene, W, H, tech):
    """pixels behind a mirror upload TWO beam sets (edge 1 and edge 2: eyeContrib != 1, its own GOp,
    the shifted path's half-vector-copied second edge, invalid where the offset path misses the mirror); light paths
    through the mirror carry manifold-type shifts (failed on the device as with useManifold=false)."""
    kw = dict(use_shift_null=0) if tech == abi.GVPM_VOL_BRE2D else {}
    c = cases.make_case(scene, W, H, 30000, 2.5, vol_technique=tech, **kw)
    e = (c.rays["info"][:, 0] >> 8) & 0xFF
    assert (e == 2).sum() > 40 and (e == 1).sum() > 1000
    sh2 = c.rays[e == 2][:, 1:]
    assert ((sh2["info"] & 1) == 0).any() and ((sh2["info"] & 1) == 1).any()
    acc, ref, st = check(c)
    assert st["failed_shifts"] > 100
    # the second edges alone: their share of the estimate
    only2 = np.ascontiguousarray(c.rays[e == 2])
    acc2, ref2, st2 = check(c, rays=only2)
    assert st2["evaluations"] > 150


def test_vpm_two_edge_camera_paths():
    from test_oracle_vpm import make_vpm_case
    from test_parity_vpm_gpu import device_vpm
    c = make_vpm_case("cbox_mirror", 48, 40, 40000, 5.0, nb=24)
    e = (c.rays["info"][:, 0] >> 8) & 0xFF
    on2 = np.isin(c.samples["set"], np.nonzero(e == 2)[0])
    assert on2.sum() > 100 and (c.samples["pdf_sel"][on2] < 0.5).all()   # the per-pixel edge CDF has two entries
    device_vpm(c, iters=2)


def test_optimistic_step_refused_by_the_build_is_queued_again(monkeypatch):
    """traversal and evaluation of a G-BRE step are queued behind its build BEFORE the host has seen the
    planner's counters; the build's last block compares them with the buffers' capacities and, when they do not fit,
    leaves a status word on which both kernels return at once -- the host then regrows and queues them again.
    GVPM_OPTIMISTIC_REFUSE=2 makes the guard see a pair buffer of zero blocks on every second optimistic step (the forced
    overflow VERDICT round 5 asked for): the iterations must come out as they do without it, and as the oracle's."""
    c = cases.make_case("cbox", 32, 24, 20000, 3.0)

    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = hip.Context(c.p, device=0)
        for k in env:
            monkeypatch.delenv(k)
        ctx.upload_scene(*c.tris)
        ctx.upload_medium(c.m)
        radii = []
        for it in range(1, 7):
            ph, nb = c.sc.shoot_photons(it, 20000)
            ctx.upload_photons(ph)
            ctx.upload_camera_beams(c.sc.camera_beams(it))
            radii.append(ctx.radius())
            ctx.gather(it, nb)
        acc = ctx.download_accum().astype(np.float64)
        st, refused = ctx.stats(), ctx.refused_steps()
        ctx.close()
        return acc, st, refused, radii

    acc0, st0, ref0, _ = run({})
    acc1, st1, ref1, radii = run({"GVPM_OPTIMISTIC_REFUSE": "2"})
    assert ref0 == 0 and ref1 >= 2, (ref0, ref1)  # (steps 2-6 are optimistic: the 2nd and the 4th of them are refused)
    for k in ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts"):
        assert st0[k] == st1[k], (k, st0, st1)
    lum = max(acc0[..., 0:3].mean(), 1e-30)
    assert l2(acc1, acc0, lum) < 1e-6
    # ... and against the oracle's APA fold over the same six iterations
    ref, ev = None, 0
    for it in range(1, 7):
        ph, nb = c.sc.shoot_photons(it, 20000)
        ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, ph, c.sc.camera_beams(it), radii[it - 1], it, nb, 64, use_accel=False, accum=ref)
        ev += cnt["evaluations"]
    assert st1["evaluations"] == ev
    assert l2(acc1, ref, max(ref[..., 0:3].mean(), 1e-30)) < TOL


@pytest.mark.parametrize("variant", ["replan", "bre2d", "GVPM_TRAV_STREAM=0", "GVPM_PIPELINE=0", "GVPM_BUILD_CHAIN=0", "GVPM_PLAN_GROUPS=0"])
def test_step_variants_that_no_other_test_reaches(variant, monkeypatch):
    """Branches of the G-BRE step (drivers_bre.hip) outside every other test's way, two iterations each against the
    oracle's fold: the same photons, beams and radius again (alpha = 1, nothing uploaded in between), which re-plans the
    built set in place with the planner as its own launch; a second BRE2D step, whose radius took the square-root
    exponent of scaleVolumeAPA; the two-stage pipeline, whose traversal runs on the build
    stream; everything on the gather stream; the build as separate launches instead of the chain; and the chain's planner
    walking one chunk of a tile's beams at a time (planBody in place of planBodyQ, build_chain.hip)."""
    replan, knob = variant == "replan", "=" in variant
    kw = dict(vol_technique=abi.GVPM_VOL_BRE2D, use_shift_null=0) if variant == "bre2d" else {}
    c = cases.make_case("cbox", 24, 20, 8000, 3.0, **kw)
    p = c.p.copy()
    if replan:
        p.alpha = 1.0
    if knob:
        monkeypatch.setenv(*variant.split("="))
    ctx = hip.Context(p, device=0)
    if knob:
        monkeypatch.delenv(variant.split("=")[0])
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ref, ev, scale = None, 0, p.initial_scale_volume
    for it in (1, 2):
        if it == 1 or not replan:
            ph, nb = c.sc.shoot_photons(it, 8000)
            rays = c.sc.camera_beams(it)
            ctx.upload_photons(ph)
            ctx.upload_camera_beams(rays)
        r = ctx.radius()
        assert r == cases.radius_of(p, np.float32(scale)) and (not replan or r == c.r)
        ctx.gather(it, nb)
        ref, cnt, _ = O.gather_bre(p, c.m, c.tris, ph, rays, r, it, nb, 64, use_accel=False, accum=ref)
        ev += cnt["evaluations"]
        scale = np.float32(O.scale_volume_apa(float(scale), it, float(p.alpha), p.vol_technique))
    acc = ctx.download_accum()
    st = ctx.stats()
    ctx.close()
    assert st["evaluations"] == ev > 1000
    assert l2(acc, ref, max(ref[..., 0:3].mean(), 1e-30)) < TOL
