"""E[dx] = E[throughput(x + 1)] - E[throughput(x)] over BSDF parents, on the device (tests/unbiased.py has the statement, and
tests/test_unbiased_gpu.py the driver and the bars, imported here as they are: no pixel of D beyond 4.5 standard errors, slope within
1 % of one, relative L2 below max(1.5 x noise floor, 1e-3), more than 1500 pixel-channels tested).  The one test of the glossy
parents that owes nothing to anybody's reading of the reference: a wrong factor in a parent's eval or pdf, a wrong Jacobian through it,
weights that do not sum to one -- each biases dx against the finite difference of the throughput.

Inputs come from DeviceGenerator(sc, glossy=True), thousands of one-iteration renders of a 32 x 24 frame, alpha = 1,
visibility_as_written = 0, the scene's table through upload_bsdfs.

The filter.  With plain parameters 6 - 7 % of the records name a table entry (29 % in the rough-glass scenes): a wrong factor in one
kind would hide in the noise.  So every case runs with lighting_interaction_mode = GVPM_SURF2MEDIA (photonContributes drops the records
reconnected from a medium vertex) and without the records reconnected from the emitter.  G-BRE: the gather's min_depth at the smallest value that
removes them (devgen_glossy_cases.min_depth_without_emitter; the share of photons left is the 15 % / 39 % quoted below).  G-Beams: its
gather has no min_depth window (as the reference's has none), so the WALK takes minDepth = 2 (SynthScene.set_min_depth), the smallest value at which
LTBeamMap::tryAppendLT stores no beam that leaves the emitter (flattenBeams, host/synth_core.h), and the gather's parameters carry
the same 2; tests/test_devgen_glossy_gpu.py holds the device generator against the host's at that setting.  Both are
filters on the record, applied alike to throughput and gradients: the identity holds for the filtered estimator.  Each case asserts,
on its first iteration's records, that at least 35 % of those the gather takes have parent type GVPM_PARENT_SURFACE_BSDF -- a
condition, not a measurement: the host generator alone meets it (0.38 cbox_ward ... 0.79 cbox_mixture at 60 000 photons).

What it does not show: the filter leaves one record in six, so the renders carry more photons than the plain test's to keep more than
1500 lit pixel-channels; G-VPM and G-Planes are not run here."""
import numpy as np
import pytest

import devgen_glossy_cases as DG
import unbiased
from gvpm_amd import abi, hip
from test_devgen_gpu import photons_from_dev
from test_unbiased_gpu import TECH, H, W, check

pytestmark = pytest.mark.gpu
MIN_SHARE = 0.35


def estimate(scene, tech, n, nph, scale, **kw):
    sc = DG.scene(scene, W, H)
    beams = tech.startswith("beams")
    if beams:
        sc.set_min_depth(2)  # (the walk's minDepth: generator and params() carry it)
    gen = hip.DeviceGenerator(sc, glossy=True)
    p = sc.params()
    p.initial_scale_volume = scale
    p.alpha = 1.0
    p.visibility_as_written = 0
    p.vol_technique = TECH[tech]
    p.lighting_interaction_mode = abi.GVPM_SURF2MEDIA
    rptr, nsets = gen.camera_beams(1)
    rays = gen.read(rptr, nsets * 5, abi.CAMERA_RAY_DTYPE).reshape(nsets, 5)
    if not beams:
        p.min_depth = DG.min_depth_without_emitter(rays)
    assert p.min_depth == (2 if beams else 4)
    for k, v in kw.items():
        setattr(p, k, v)
    ctx = hip.Context(p, device=0)
    ctx.upload_scene(*sc.triangles())
    ctx.upload_medium(sc.medium())
    ctx.upload_bsdfs(sc.bsdfs())
    share = {}

    def step(k):
        it = k + 1
        ctx.reset()
        rptr, nsets = gen.camera_beams(it)
        if beams:
            soa, en, nb = gen.shoot_beams(it, nph)
            ctx.upload_beams_dev(soa, en)
            edge = None
        else:
            soa, nb = gen.shoot_photons(it, nph)
            ctx.upload_photons_dev(soa)
            edge = int((rays["info"][0, 0] >> 8) & 0xFF)
        if k == 0:
            rec = photons_from_dev(gen, soa)
            share["v"] = DG.table_parent_share(rec, p, edge)
            share["emitter"] = int((((rec.flags & 3) == abi.GVPM_PARENT_EMITTER) & DG.taken(rec, p, edge)).sum())
        ctx.upload_camera_beams_dev(rptr, nsets)
        ctx.gather(1, nb)
        return ctx.download_film(1, False)

    out = unbiased.run(step, n)
    st = ctx.stats()
    ctx.close()
    gen.close()
    assert share["emitter"] == 0  # (no record reconnected from the emitter reaches the estimator)
    return out, st, share["v"]


def run_case(scene, tech, n, nph, scale, **kw):
    out, st, (share, kept) = estimate(scene, tech, n, nph, scale, **kw)
    print(f"{scene} {tech} {kw}: {n} renders x {nph} records, {kept} kept in the first, share of table parents {share:.3f}")
    assert share >= MIN_SHARE, (scene, share)
    check(out, st, f"{scene} {tech} {kw}")


# Renders and records a render, with the time a case took on an MI355X.  The slope of this statistic sits below one by about the
# square of its noise floor at any finite render count (1 + sum(D ref) / sum(ref^2) with ref = g - D), so the 1 % bar needs a floor
# near 0.04: that, not the 1500 lit pixel-channels (2208 - 2232 are lit), sets the counts.
# G-BRE 3D: the filter keeps 15 % of the photons (39 % behind rough glass); 2 000 renders x 120 000 photons at scale 7: floor
# 0.029 - 0.038 (0.051 without MIS), 5.3 - 5.7 s a case, cbox_roughglass_rot 12.0 s (its tilted pane costs the walk twice the time).
BRE_RENDERS, BRE_PHOTONS, BRE_SCALE = 2000, 120000, 7.0
# G-Beams 3D: every stored beam passes the emitter filter, a third to a half passes SURF2MEDIA; 3 000 renders x 30 000 beams at the
# plain test's scale 2: floor 0.011 - 0.048, 4.7 - 5.1 s a case.
BEAM_RENDERS, BEAM_BEAMS, BEAM_SCALE = 3000, 30000, 2.0

# cbox_conductor, cbox_phong, cbox_ward: kinds the fp64 oracle states -- the control; the others: kinds no oracle covers
BRE_SCENES = ["cbox_conductor", "cbox_phong", "cbox_ward", "cbox_roughplastic", "cbox_plastic", "cbox_conductor_aniso", "cbox_ward_aniso",
              "cbox_roughglass", "cbox_conductor_phong", "cbox_mixture", "cbox_roughglass_rot"]


@pytest.mark.parametrize("scene", BRE_SCENES)
def test_bre3d_gradient_is_the_finite_difference_of_the_throughput(scene):
    run_case(scene, "bre3d", BRE_RENDERS, BRE_PHOTONS, BRE_SCALE)


def test_bre3d_without_mis():
    run_case("cbox_roughplastic", "bre3d", BRE_RENDERS, BRE_PHOTONS, BRE_SCALE, use_mis=0, path_set=0)


@pytest.mark.parametrize("scene", ["cbox_conductor", "cbox_roughglass", "cbox_mixture"])
def test_beams3d(scene):
    run_case(scene, "beams3d", BEAM_RENDERS, BEAM_BEAMS, BEAM_SCALE)
