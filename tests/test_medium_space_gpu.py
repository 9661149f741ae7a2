"""Device against the fp64 oracle over the trial media of tests/medium_cases.py, through the parity drivers of the four
techniques called unchanged: counters exact and the drivers' own L2 bars (G-BRE 1e-4, G-VPM 1e-4, G-Beams 2e-4, G-Planes 1e-5)
for chroma / msw / back / all / thick, plus the same bar on every colour channel by itself (the pooled metric hides a channel
that carries a few per cent of the luminance).  `opaque` has its own, stated, weaker counter rule (test_opaque)."""
import numpy as np
import pytest

import cases
import medium_cases
import oracle_lib as O
from gvpm_amd import abi, hip
from test_exact_pass_gpu import check_beams as exact_beams, check_bre as exact_bre, check_vpm as exact_vpm
from test_oracle_beams import make_beam_case, TECHS
from test_oracle_planes import make_plane_case
from test_oracle_vpm import make_vpm_case
from test_parity_beams_gpu import device_beams
from test_parity_gpu import check, l2, TOL
from test_parity_planes_gpu import device_planes
from test_parity_vpm_gpu import device_vpm
from test_primal_bre import primal_case
from test_primal_bre_gpu import check_primal

pytestmark = pytest.mark.gpu

# technique -> (case, driver, the L2 bar the driver asserts)
TECHNIQUES = {
    "bre3d": (lambda: cases.make_case("cbox", 40, 36, 30000, 2.5), check, TOL),
    "vpm": (lambda: make_vpm_case("cbox", 32, 28, 40000, 5.0, nb=10), device_vpm, TOL),
    "beams3d": (lambda: make_beam_case("cbox", 32, 28, 12000, 2.5, technique=TECHS[0]), device_beams, 2e-4),
    "beams1d": (lambda: make_beam_case("cbox", 32, 28, 12000, 2.5, technique=TECHS[1]), device_beams, 2e-4),
    "planes": (lambda: make_plane_case("cbox_in", 32, 28, 6000), device_planes, 1e-5),
}


def channels_within(acc, ref, bar):
    assert np.isfinite(acc).all()
    per = medium_cases.per_channel_l2(acc, ref)
    print("per-channel L2 (R, G, B):", per)
    assert max(per) < bar, per


@pytest.mark.parametrize("tech", list(TECHNIQUES))
@pytest.mark.parametrize("name", medium_cases.EXACT)
def test_medium(name, tech):
    make, driver, bar = TECHNIQUES[tech]
    c = medium_cases.apply(make(), name)
    acc, ref, st = driver(c)
    assert st["evaluations"] > 5000
    channels_within(acc, ref, bar)


# ---------------------------------------------------------------------------------------------------------------------
# `opaque` (sigma_t = 64): pdfSuccess = sigma_t exp(-sigma_t t) underflows in fp32 where fp64 still holds it, so a
# reconnection that fp64 counts with zero flux is a failed shift in fp32 (the fp32 oracle: 2 134 of 65 176 for this G-BRE
# case).  A migrated shift carries zero flux either way and the base terms beside it are cut to 0, so the sums keep their bar.
def run_opaque(tech, c):
    """-> (accum, stats, film, fp64 reference, its counters): the drivers' uploads and gathers without their assertions"""
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    cases.upload_bsdfs(ctx, c)
    rad = ctx.radius()
    if tech == "bre3d":
        ctx.upload_photons(c.ph)
        ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    elif tech == "vpm":
        ctx.upload_photons(c.ph)
        ctx.upload_vpm_samples(c.samples)
        ref, _, _, cnt, _ = O.gather_vpm(c.p, c.m, c.tris, c.ph, c.rays, c.samples, 64, use_accel=False)
    elif tech == "planes":
        ctx.upload_planes(c.beams, c.w1, c.len1)
        ref, cnt, _ = O.gather_planes(c.p, c.m, c.tris, c.beams, c.w1, c.len1, c.rays, 1, c.nb, 64)
    else:
        ctx.upload_beams(c.beams, c.end_n)
        ref, cnt, _ = O.gather_beams(c.p, c.m, c.tris, c.beams, c.end_n, c.rays, rad, 1, c.nb, 64)
    ctx.upload_camera_beams(c.rays)
    ctx.gather(1, c.nb)
    acc = ctx.download_accum()
    st = ctx.stats()
    film = ctx.download_film(1, True)
    ctx.close()
    return acc, st, film, ref, cnt


@pytest.mark.parametrize("tech", list(TECHNIQUES))
def test_opaque(tech):
    """Measured on an MI355X, device against fp64 oracle, L2 of the 27 accumulators: G-BRE 6.1e-7 (4 556 zero-flux reconnections
    counted as failed shifts), G-VPM 9.7e-8 (11 166), Beams 1D 1.9e-5 (dy 5.5e-5) and Planes 4.7e-7 (all four counters equal to the oracle's;
    so are Beams 3D's: the evaluated sets are the fp64 oracle's, 4 979 and 4 965 pairs, where the fp32 oracle evaluates 6 393).

    Beams 3D: accumulators 5.0e-5, the film's dy 1.5e-4 against 2e-4 -- nearly all of it ONE reconnection: pixel (14, 27),
    shifted[2] = 15.7588, 7 000x the mean luminance (exp(64 * 0.08) between the base beam's length and the new one's), so 1e-6
    of its own value is 7e-3 of the mean luminance in one of 2 688 film values.  With the lengths dist, v and w rounded to
    fp32 one by one (sigma_t times half an ulp: 1e-6 each) dy stood at 2.33e-4 and this case failed; beamShift2 now forms
    exp(-sigma_t (dist - v)) from the lengths' difference and w's depth in double (beams_shift_f32.h).  What is left is the
    offset position's own fp32 rounding in the local frame (1e-8 of a length, times sigma_t), which is of the same order: the
    1-D kernel's one outlier of the same pixel moved the other way with the same change (accumulators 1.0e-5 before)."""
    make, _, bar = TECHNIQUES[tech]
    c = medium_cases.apply(make(), "opaque")
    acc, st, film, ref, cnt = run_opaque(tech, c)
    print("device", st, "oracle", cnt)
    assert np.isfinite(acc).all() and all(np.isfinite(f).all() for f in film)
    assert np.isfinite(ref).all()
    assert st["evaluations"] == cnt["evaluations"] > 1000
    assert st["null_shifts"] == cnt["null_shifts"]
    assert st["diffuse_shifts"] + st["failed_shifts"] == cnt["diffuse_shifts"] + cnt["failed_shifts"], (st, cnt)
    # fp32 may turn a zero-flux reconnection into a failed one and never the reverse
    assert st["failed_shifts"] >= cnt["failed_shifts"], (st, cnt)
    lum = ref[..., 0:3].mean()
    err = l2(acc, ref, lum)
    print("L2", err)
    assert err < bar, err
    # (G-VPM's film divides by the emitted paths: device_vpm)
    rfilm, flum = (O.assemble(ref, 1, True, total_emitted=c.nb), lum / c.nb) if tech == "vpm" else (O.assemble(ref, 1, True), lum)
    errs = [l2(a, b, flum) for a, b in zip(film, rfilm)]
    print("film L2 (throughput, dx, dy)", errs)
    assert max(errs) < bar, errs


# ---------------------------------------------------------------------------------------------------------------------
# the other copies of sigS / mediumEvalD / phaseD, all under `all` (chromatic, msw = 0.3, g = -0.4)
def test_exact_pass_bre(monkeypatch):
    c = medium_cases.apply(cases.make_case("cbox", 40, 36, 30000, 2.5), "all")
    acc, ref, st = exact_bre(c, monkeypatch)
    channels_within(acc, ref, 2e-6)


def test_exact_pass_vpm(monkeypatch):
    c = medium_cases.apply(make_vpm_case("cbox", 32, 28, 40000, 5.0, nb=10), "all")
    acc, ref, st = exact_vpm(c, monkeypatch)
    channels_within(acc, ref, 2e-5)


@pytest.mark.parametrize("tech", TECHS)
def test_exact_pass_beams(tech, monkeypatch):
    c = medium_cases.apply(make_beam_case("cbox", 32, 28, 12000, 2.5, technique=tech), "all")
    acc, ref, st = exact_beams(c, monkeypatch)
    channels_within(acc, ref, 5e-5)


def test_occluders_and_rotation():
    c = medium_cases.apply(cases.make_case("fogroom_rot", 40, 36, 30000, 1.6), "all")
    acc, ref, st = check(c)
    assert st["evaluations"] > 5000 and st["diffuse_shifts"] > 5000
    channels_within(acc, ref, TOL)


def test_bre2d():
    c = medium_cases.apply(cases.make_case("cbox", 40, 36, 30000, 2.5, vol_technique=abi.GVPM_VOL_BRE2D, use_shift_null=0), "all")
    acc, ref, st = check(c, use_accel=False)
    assert st["evaluations"] > 5000
    channels_within(acc, ref, TOL)


@pytest.mark.parametrize("tech", [abi.GVPM_VOL_BRE3D, abi.GVPM_VOL_BRE2D])
def test_primal_gather_chromatic(tech):
    c = medium_cases.apply(primal_case("cbox", 40, 36, 30000, 2.5, vol_technique=tech, use_shift_null=0), "chroma")
    acc, ref, st = check_primal(c)
    for ch in range(3):   # (the primal pass fills the flux slots only)
        assert l2(acc[..., ch], ref[..., ch], ref[..., ch].mean()) < 1e-4
