"""G-BRE and G-VPM launch variants outside every other test's way.  The traversal and the evaluation of a G-BRE step are a matrix of
template instantiations (near lists or the occluder BVH, a plain table or one with mixture heads, host shifts, the record prefetch,
16 / 32 / 64 beams a wave) and dispatch modes (persistent or one wave an item, work units or not, the grid clipped to the beams'
reach or not, the planner's target, the waves per CU, the cell size, the slab thickness, the stream priorities), of which the suite
launched the default cell and a few named others; a mistake in an `if constexpr` arm or a dispatch branch shows only in the cell
that takes it.

Shape of test_parity_gpu.test_step_variants_that_no_other_test_reaches: cbox at 24 x 20 pixels with 8 000 photons, two iterations
under the shrinking radius against the oracle's fold -- the evaluation total exact and above 1 000, L2 / luminance below TOL = 1e-4 --
and beside it the default handle on the same inputs: the four counters equal, the accumulators equal up to the order of the float
atomics (rtol 5e-5, atol 1e-6 of the largest: the bar of test_near_occluder_grid_finds_what_the_bvh_query_finds).

Every value set below lies inside the range the library's parser accepts (gvpm_create, gvpm_api.hip: GVPM_PLAN_TARGET 64 .. 2^24,
GVPM_WAVES_PER_CU and GVPM_TRAV_WAVES_PER_CU 1 .. 32, GVPM_CELL_SCALE 0.25 .. 8, GVPM_PERSISTENT's two bits, GVPM_VPM_EVAL_WAVES
>= 64, GVPM_VPM_REDO_WAVES >= 1; the others are switches or plain integers), so the variant is in force without an observable of
its own.  The environment is set around hip.Context(...) only, where the library reads it."""
import numpy as np
import pytest

import cases
import mixture_cases as MC
import oracle_lib as O
import plastic_cases as PC
from gvpm_amd import abi, hip
from test_oracle_vpm import make_vpm_case
from test_parity_gpu import l2, TOL
from test_parity_vpm_gpu import device_vpm

pytestmark = pytest.mark.gpu
W, H, NPH, SCALE = 24, 20, 8000, 3.0
ITERS = (1, 2)
COUNTERS = ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts")
_inputs, _default = {}, {}


class Run:
    pass


def inputs(setting, **kw):
    """The photons, beams and radii of the two iterations and the oracle's fold over them, once per (setting, parameters).
    "mixture": cbox_conductor's records through mixtures {the wall's conductor, Lambertian} at weights (1, 0), which the oracle
    states as the plain conductor (tests/test_eval_specialised_gpu.py builds the same table)."""
    key = (setting, tuple(sorted(kw.items())))
    if key in _inputs:
        return _inputs[key]
    mix = setting == "mixture"
    c = cases.make_case("cbox_conductor" if mix else "cbox", W, H, NPH, SCALE, **kw)
    r = Run()
    r.key, r.c, r.p, r.table, mapping = key, c, c.p, c.bsdfs, None
    if mix:
        throwaway = cases.make_case("cbox_conductor", 8, 8, 100, 4.0)
        heads = MC.over_conductor(throwaway, (1.0, 0.0))
        r.table = throwaway.bsdfs
        assert (r.table["kind"][heads] == abi.GVPM_BSDF_MIXTURE).all()
        own = c.sc.bsdfs()
        mapping = np.zeros(own.size, np.int64)
        mapping[np.flatnonzero(abi.bsdf_heads(own))] = heads
    O.set_bsdfs(c.bsdfs)   # (the oracle reads the scene's own table and the records that name it)
    r.steps, r.radii, ref, ev, scale = [], [], None, 0, c.p.initial_scale_volume
    for it in ITERS:
        ph, nb = c.sc.shoot_photons(it, NPH)
        rays = c.sc.camera_beams(it)
        radius = cases.radius_of(c.p, np.float32(scale))
        ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, ph, rays, radius, it, nb, 64, use_accel=False, accum=ref)
        ev += cnt["evaluations"]
        r.steps.append((PC.relabelled(ph, mapping) if mix else ph, nb, rays))
        r.radii.append(radius)
        scale = np.float32(O.scale_volume_apa(float(scale), it, float(c.p.alpha), c.p.vol_technique))
    if mix:
        gl = (r.steps[0][0].flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
        assert gl.sum() > 200 and np.isin(r.steps[0][0].parent_g[gl].astype(np.int64), heads).all()
    r.ref, r.evaluations = ref, ev
    _inputs[key] = r
    return r


def device(r, monkeypatch, env=None, p=None, host_shifts=False):
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = hip.Context(r.p if p is None else p, device=0)
    for k in env:
        monkeypatch.delenv(k)
    ctx.upload_scene(*r.c.tris)
    ctx.upload_medium(r.c.m)
    if r.table.size:
        ctx.upload_bsdfs(r.table)
    if host_shifts:
        ctx.enable_host_shifts(1 << 16)
    for it, (ph, nb, rays), radius in zip(ITERS, r.steps, r.radii):
        assert ctx.radius() == radius
        ctx.upload_photons(ph)
        ctx.upload_camera_beams(rays)
        ctx.gather(it, nb)
    if host_shifts:
        ctx.download_shift_requests(1 << 16)   # (none is answered: failed shifts, as with use_manifold off)
    acc, st = ctx.download_accum(), ctx.stats()
    ctx.close()
    return acc, st


def default_handle(r, monkeypatch):
    if r.key not in _default:
        _default[r.key] = device(r, monkeypatch)
        matches_the_oracle(r, *_default[r.key], what=f"{r.key} default handle")
    return _default[r.key]


def matches_the_oracle(r, acc, st, what):
    err = l2(acc, r.ref, max(r.ref[..., 0:3].mean(), 1e-30))
    print(f"{what}: evaluations {st['evaluations']} / {r.evaluations}, L2 / lum {err:.3e}")
    assert st["evaluations"] == r.evaluations > 1000, (what, st, r.evaluations)
    assert err < TOL, (what, err)


def matches_the_default_handle(acc, st, acc0, st0, what):
    for k in COUNTERS:
        assert st[k] == st0[k], (what, k, st, st0)
    np.testing.assert_allclose(acc, acc0, rtol=5e-5, atol=1e-6 * float(np.abs(acc0).max()), err_msg=what)


def env_of(variant):
    return dict(kv.split("=", 1) for kv in variant.split())


VARIANTS = [
    "GVPM_PERSISTENT=0", "GVPM_PERSISTENT=2", "GVPM_PERSISTENT=3",   # bit 0: the evaluation's waves, bit 1: the traversal's (default 1)
    "GVPM_EVAL_UNITS=0",
    "GVPM_CLIP_GRID=0",
    "GVPM_PLAN_TARGET=64", "GVPM_PLAN_TARGET=1048576",
    "GVPM_WAVES_PER_CU=1", "GVPM_WAVES_PER_CU=32 GVPM_PIPELINE=0",
    "GVPM_TRAV_WAVES_PER_CU=1 GVPM_PERSISTENT=3",
    "GVPM_CELL_SCALE=0.25", "GVPM_CELL_SCALE=4",
    # slab layers per planner / traversal step (tile_walk.h tileSetupFrom: K = reserved[2] along x, reserved[1] along y and z; the
    # walk's steps are cA0 + k K clamped to cA1 and a step's box is staged in windows, so any K >= 1 is a valid cut; the box
    # hand-off's stride is sized from the smaller of the two, drivers_bre.hip).  The defaults are 6 and 8 -- and 8 for both with
    # maps of at most 2 M photons, as here: one below the smaller default, one below the larger
    "GVPM_SLAB_LAYERS=5", "GVPM_SLAB_LAYERS_X=7",
    "GVPM_STREAM_PRIORITIES=0,0,0",
]


@pytest.mark.parametrize("variant", VARIANTS)
def test_dispatch_variants_match_the_oracle_and_the_default_handle(variant, monkeypatch):
    r = inputs("cbox")
    acc0, st0 = default_handle(r, monkeypatch)
    acc, st = device(r, monkeypatch, env=env_of(variant))
    matches_the_oracle(r, acc, st, variant)
    matches_the_default_handle(acc, st, acc0, st0, variant)


# GVPM_RECORD_PREFETCH=1: the evaluation's next-record prefetch, by default on above 2 M photons only -- which the suite reaches at
# 4 M photons, 16 beams a wave, BVH visibility and a plain table.  Forced here on (a) the near-list kernel, (b) the occluder-BVH
# kernel, (c) a table with mixture heads, (d) 32 beams a wave; GVPM_RECORD_PREFETCH=0 once as the control.
PREFETCH = {
    "near lists": ("cbox", {}, {"GVPM_RECORD_PREFETCH": "1"}, {}),
    "full visibility": ("cbox", dict(visibility_as_written=0), {"GVPM_RECORD_PREFETCH": "1"}, {}),
    "mixture table": ("mixture", {}, {"GVPM_RECORD_PREFETCH": "1"}, {}),
    "32 beams a wave": ("cbox", {}, {"GVPM_RECORD_PREFETCH": "1", "GVPM_BEAMS_PER_WAVE": "32"}, {"GVPM_BEAMS_PER_WAVE": "32"}),
    "off (control)": ("cbox", {}, {"GVPM_RECORD_PREFETCH": "0"}, {}),
}


@pytest.mark.parametrize("which", list(PREFETCH))
def test_forced_record_prefetch(which, monkeypatch):
    setting, kw, env, env0 = PREFETCH[which]
    r = inputs(setting, **kw)
    acc0, st0 = device(r, monkeypatch, env=env0) if env0 else default_handle(r, monkeypatch)
    acc, st = device(r, monkeypatch, env=env)
    matches_the_oracle(r, acc, st, f"record prefetch, {which}")
    if env0:
        matches_the_oracle(r, acc0, st0, f"{which}, without the prefetch")
    matches_the_default_handle(acc, st, acc0, st0, which)
    assert st["diffuse_shifts"] > 1000   # (phase 2, where the records are read, ran)


@pytest.mark.parametrize("setting,kw", [("cbox", dict(visibility_as_written=0)), ("mixture", {})], ids=["full visibility", "mixture table"])
def test_host_shifts_with_full_visibility_and_with_a_mixture_table(setting, kw, monkeypatch):
    """The host-shift instantiations of the evaluation (use_manifold = 1 and gvpm_enable_host_shifts) with the occluder BVH and with a
    table that has mixture heads.  No request is answered, as in test_eval_specialised_gpu.FALLBACK["host shifts"]: the shifts fail
    as with use_manifold = 0, which is what the oracle's fold and the default handle were run with."""
    r = inputs(setting, **kw)
    acc0, st0 = default_handle(r, monkeypatch)
    p = r.p.copy()
    p.use_manifold = 1
    acc, st = device(r, monkeypatch, p=p, host_shifts=True)
    matches_the_oracle(r, acc, st, f"host shifts, {setting} {kw}")
    matches_the_default_handle(acc, st, acc0, st0, f"host shifts, {setting} {kw}")


# ---- G-VPM ------------------------------------------------------------------------------------------------------------------------
_vpm_default = {}


@pytest.mark.parametrize("knobs", ["GVPM_VPM_EVAL_WAVES=64", "GVPM_VPM_REDO_WAVES=1 GVPM_VPM_POOL=0"])
def test_vpm_launch_sizes_agree(knobs, monkeypatch):
    """In the shape of test_parity_vpm_gpu.test_vpm_kernel_paths_agree: the evaluation with the fewest persistent waves the parser
    allows (64 over the shards: every wave strides over many groups of chunks), and ONE persistent wave for the redo kernel with the
    pool of four chunks a shard (GVPM_VPM_POOL=0, as that test arranges), so that nearly every batch is on the redo list it walks."""
    c = make_vpm_case("cbox_hg", 32, 28, 40000, 5.0, nb=10)
    if "default" not in _vpm_default:
        _vpm_default["default"] = device_vpm(c, iters=4)
    acc0, _, st0 = _vpm_default["default"]
    for k, v in env_of(knobs).items():
        monkeypatch.setenv(k, v)
    acc1, ref, st1 = device_vpm(c, iters=4)   # (asserts the oracle's counters and L2 < TOL)
    for k in ("evaluations", "candidates", "null_shifts", "diffuse_shifts", "failed_shifts"):
        assert st0[k] == st1[k], (k, st0[k], st1[k])
    lum = max(ref[..., 0:3].mean(), 1e-30)
    print(f"{knobs}: L2 / lum against the oracle {l2(acc1, ref, lum):.3e}, against the default path {l2(acc1, acc0, lum):.3e}")
    assert l2(acc1, acc0, lum) < 1e-6


# ---- the grid clipped to STALE beam bounds ------------------------------------------------------------------------------------------
def test_grid_clipped_to_beam_bounds_carried_from_previous_beam_sets(monkeypatch):
    """Beside test_parity_gpu.test_grid_bounds_carried_from_previous_photon_set, for sizeGrid's clip (drivers_build.hip): the grid
    of a step covers what the LAST step's camera beams could reach.  Step 1 gathers with the beams of a 2 x 2 pixel window in a
    corner of a 32 x 28 frame; after a reset step 2 gathers the whole frame on the same handle: its grid is clipped to the window's
    reach, most beams and most photons lie outside it (clamped into the border cells) and every pair must still be found.  Against
    the oracle on the whole frame, and with GVPM_CLIP_GRID=0 (a value the parser accepts: the switch is in force) the counters must
    be the same."""
    c = cases.make_case("cbox", 32, 28, 20000, 3.0)
    px, py = cases.pixels_of(c.rays)
    corner = np.ascontiguousarray(c.rays[(px < 2) & (py < 2)])
    assert 1 <= corner.shape[0] <= 8 and c.rays.shape[0] > 100 * corner.shape[0]
    # the window's reach (its base rays' segments, padded as sizeGrid pads them) leaves most photons and most beams' ends outside
    o, d, ln = corner["o"][:, 0].astype(np.float64), corner["d"][:, 0].astype(np.float64), corner["len"][:, 0].astype(np.float64)
    ends = np.concatenate([o, o + d * ln[:, None]])
    pad = 1.01 * c.r + 2 * 1.5 * c.r
    lo, hi = ends.min(0) - pad, ends.max(0) + pad
    inside = ((c.ph.pos >= lo) & (c.ph.pos <= hi)).all(1)
    allo, alld, allln = c.rays["o"][:, 0].astype(np.float64), c.rays["d"][:, 0].astype(np.float64), c.rays["len"][:, 0].astype(np.float64)
    far = allo + alld * allln[:, None]
    beams_inside = ((far >= lo) & (far <= hi)).all(1)
    print(f"photons inside the window's reach {inside.sum()} of {c.ph.n}, beams ending inside it {beams_inside.sum()} of {len(far)}")
    assert inside.sum() < c.ph.n // 2 and beams_inside.sum() < len(far) // 2
    ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    lum = max(ref[..., 0:3].mean(), 1e-30)
    out = []
    for clip in ("1", "0"):
        monkeypatch.setenv("GVPM_CLIP_GRID", clip)
        ctx = hip.Context(c.p, device=0)
        monkeypatch.delenv("GVPM_CLIP_GRID")
        ctx.upload_scene(*c.tris)
        ctx.upload_medium(c.m)
        ctx.upload_photons(c.ph)
        ctx.upload_camera_beams(corner)      # step 1: a corner of the frame -> small cached beam bounds
        ctx.gather(1, c.nb)
        ctx.reset()
        ctx.upload_camera_beams(c.rays)      # step 2: the whole frame, most of it outside the cached bounds
        ctx.gather(1, c.nb)
        acc, st = ctx.download_accum(), ctx.stats()
        ctx.close()
        err = l2(acc, ref, lum)
        print(f"GVPM_CLIP_GRID={clip}: {[st[k] for k in COUNTERS]} oracle {[cnt[k] for k in COUNTERS]} L2 / lum {err:.3e}")
        for k in COUNTERS:
            assert st[k] == cnt[k], (clip, k, st, cnt)
        assert err < TOL, (clip, err)
        out.append(st)
    for k in COUNTERS:
        assert out[0][k] == out[1][k], (k, out)
