"""The oracle against the independent numpy statements (tests/indep_statements.py) over the trial media of
tests/medium_cases.py: per-channel sigma_s, medium_sampling_weight < 1, backscatter, and media thick enough for the 1e-20
transmittance cut-off.  Every other test evaluates its cases under the grey, msw = 1, g in {0, 0.7} family the generators emit;
here the case is evaluated under another medium than the one its photons were shot in (as in similarity_cases.py: both sides
get the same arrays and the same gvpm_medium, and parity between them is what is asserted).  Sizes and bars are those of
test_indep_statements.py: counters equal, every one of the nine slot groups within 1e-9 of the mean luminance."""
import numpy as np
import pytest

import cases
import indep_statements as I
import medium_cases
import oracle_lib as O
from test_indep_statements import compare, compare_beams
from test_oracle_beams import make_beam_case, TECHS
from test_oracle_planes import make_plane_case
from test_oracle_vpm import make_vpm_case

NAMES = list(medium_cases.MEDIA)


def slots_agree(acc, ref, tol=1e-9):
    lum = ref[..., 0:3].mean()
    assert np.isfinite(ref).all() and np.isfinite(acc).all()
    for j in range(9):
        err = np.abs(acc[..., 3 * j:3 * j + 3] - ref[..., 3 * j:3 * j + 3]).max() / lum
        assert err < tol, (j, err)


@pytest.mark.parametrize("name", NAMES)
def test_bre3d(name):
    c = medium_cases.apply(cases.make_case("cbox", 20, 16, 4000, 4.0), name)
    cnt = compare(c)                       # (asserts evaluations > 100)
    assert cnt["diffuse_shifts"] > 50


@pytest.mark.parametrize("name", NAMES)
def test_vpm(name):
    c = medium_cases.apply(make_vpm_case("cbox", 12, 10, 6000, 8.0, 6), name)
    ref, rsv, rnv, cnt, _ = O.gather_vpm(c.p, c.m, c.tris, c.ph, c.rays, c.samples, 64, use_accel=True)
    acc, icnt, mvol = I.vpm_full(c)
    assert cnt["evaluations"] > 100 and cnt["diffuse_shifts"] > 50
    for k in ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts"):
        assert icnt[k] == cnt[k], (k, icnt, cnt)
    slots_agree(acc, ref)


@pytest.mark.parametrize("tech", TECHS)
@pytest.mark.parametrize("name", NAMES)
def test_beams(name, tech):
    c = medium_cases.apply(make_beam_case("cbox", 12, 10, 1500, 4.0, technique=tech), name)
    cnt = compare_beams(c)                 # (asserts evaluations > 100)
    assert cnt["diffuse_shifts"] > 50


@pytest.mark.parametrize("name", NAMES)
def test_planes(name):
    c = medium_cases.apply(make_plane_case("cbox_in", 16, 12, 1500), name)
    ref, cnt, _ = O.gather_planes(c.p, c.m, c.tris, c.beams, c.w1, c.len1, c.rays, 1, c.nb, 64)
    acc, icnt = I.planes_full(c)
    assert cnt["evaluations"] > 100 and cnt["diffuse_shifts"] > 50
    for k in ("evaluations", "diffuse_shifts", "failed_shifts"):
        assert icnt[k] == cnt[k], (k, icnt, cnt)
    slots_agree(acc, ref)


@pytest.mark.parametrize("name", ["thick", "opaque"])
def test_planes_behind_the_cut_off_carry_no_shifted_flux(name):
    """At the size the device test uses some planes are pierced further than 46 / sigma_t along an edge: the base
    transmittance is cut to 0, and the reference's ratio over it (shift_volume_planes.h:346-347) would be 0 / 0.  Oracle and
    independent statement agree that such a pair adds nothing, and everything stays finite."""
    c = medium_cases.apply(make_plane_case("cbox_in", 32, 28, 6000), name)
    sig_t = float(c.m.sigma_t[0])
    l0 = np.linalg.norm(c.beams.pos.astype(np.float64) - c.beams.parent_pos.astype(np.float64), axis=1)
    assert (np.maximum(l0, c.len1) * sig_t > -np.log(1e-20)).sum() > 100      # (edges long enough to reach the cut-off)
    ref, cnt, _ = O.gather_planes(c.p, c.m, c.tris, c.beams, c.w1, c.len1, c.rays, 1, c.nb, 64)
    acc, icnt = I.planes_full(c)
    for k in ("evaluations", "diffuse_shifts", "failed_shifts"):
        assert icnt[k] == cnt[k], (k, icnt, cnt)
    slots_agree(acc, ref)


def test_every_medium_moves_the_bre_reference():
    """the cases are sensitive: each trial medium moves the G-BRE reference by more than 0.1 x the mean luminance of the
    grey one (measured 1.9x .. 22x)"""
    c = cases.make_case("cbox", 20, 16, 4000, 4.0)
    grey, _, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    lum = grey[..., 0:3].mean()
    for name in NAMES:
        q = medium_cases.apply(cases.make_case("cbox", 20, 16, 4000, 4.0), name)
        ref, _, _ = O.gather_bre(q.p, q.m, q.tris, q.ph, q.rays, q.r, 1, q.nb, 64, use_accel=False)
        moved = np.sqrt(((ref - grey) ** 2).mean()) / lum
        assert moved > 0.1, (name, moved)


def test_thick_reaches_the_cut_off():
    """under `thick` at least one pixel that the grey medium lights has a flux of exactly 0: the 1e-20 cut-off is reached"""
    c = cases.make_case("cbox", 20, 16, 4000, 4.0)
    grey, _, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    medium_cases.apply(c, "thick")
    ref, _, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    lit = grey[..., 0:3].sum(-1) > 0
    assert (lit & (ref[..., 0:3].sum(-1) == 0)).sum() >= 1


def test_apply_sets_every_field():
    c = medium_cases.apply(cases.make_case("cbox", 8, 6, 100, 4.0), "all")
    s, t, g, w = medium_cases.MEDIA["all"]
    f = np.float32
    assert [c.m.sigma_s[k] for k in range(3)] == [f(x) for x in s] and [c.m.sigma_t[k] for k in range(3)] == [f(t)] * 3
    assert [c.m.sigma_a[k] for k in range(3)] == [f(t - x) for x in s]
    assert c.m.g == f(g) and c.m.medium_sampling_weight == f(w)
    assert c.sc.medium().g == 0.0 and c.sc.medium().medium_sampling_weight == 1.0    # (the scene's own medium is untouched)
