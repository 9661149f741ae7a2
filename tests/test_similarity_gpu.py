"""Parity AWAY FROM THE UNIT ROOM: the device against the fp64 oracle on scenes moved and resized by a similarity transform.

Every other scene of the suite is a room of half-width 1 at the origin, and the error bands behind which the device takes its
hit and shift decisions in fp32 were derived there.  tests/similarity_cases.py maps a case's positions by p' = s p + t; the
tests below run every technique through the transforms it names, with the harnesses of the parity files unchanged (their own
bars: 1e-4 G-BRE / G-VPM, 2e-4 G-Beams, 1e-5 G-Planes; evaluations and all shift counters equal to the oracle's):

  shifted      the room 3-5 widths from the origin              small   the room 1/64 wide
  large        64 wide, 200-300 from the origin                 far     the unit room 1000-2000 from the origin
  centimetres  256 wide, 700-1100 from the origin, Epsilon still 1e-4 -- a scene modelled in centimetres

Under `centimetres` and `far` Epsilon is below the ulp of a coordinate: parents land behind their own walls and self-hit in
the reference, which the own-wall rule, the near lists and the exact pass claim to reproduce -- with bands as wide as Epsilon
itself.  tests/test_similarity.py shows (on the CPU) that these inputs reach that regime.

Outcome: parity at the harnesses' bars for every technique under every transform; no note list overflowed.  The exact pass
takes 2.4 % of G-BRE 3D's shifts on the rotated fog room under `centimetres` (0.009 % untransformed), 2.3 % of G-VPM's, 70 % of
G-Beams 3D's ("Away from the unit room").  What the transforms found, fixed where it was: the reconnection vector
through an fp32 point (gather_bre.hip evalPhase2Core, gather_vpm.hip vpmPhase2: `far`), the free cone's own-wall sliver as a
constant angle (beams_build.hip beamClearTri: `centimetres`), plain fp32 shadow segments in the literal G-Beams path
(gather_beams.hip: `centimetres`).
"""
import os

import numpy as np
import pytest

import cases
import oracle_lib as O
import similarity_cases as S
from gvpm_amd import abi, hip
from test_bundle_grid_gpu import run as run_bundle
from test_oracle_beams import make_beam_case, TECHS
from test_oracle_planes import make_plane_case
from test_oracle_vpm import make_vpm_case
from test_parity_beams_gpu import device_beams
from test_parity_gpu import check, device_gather
from test_parity_planes_gpu import device_planes
from test_parity_vpm_gpu import device_vpm

pytestmark = pytest.mark.gpu
COUNTERS = ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts")
ALL = ["shifted", "small", "large", "centimetres", "far"]
B3D, B1D = abi.GVPM_BEAM_BEAM_3D_OPTIMIZED, abi.GVPM_BEAM_BEAM_1D
assert set(TECHS) == {B3D, B1D}


def bre_case(scene, name, **kw):
    return S.named(cases.make_case(scene, 40, 36, 30000, 1.6, **kw), name)


def vpm_case(scene, name):
    return S.named(make_vpm_case(scene, 32, 28, 40000, 3.1, nb=10), name)


def beam_case(scene, tech, name):
    return S.named(make_beam_case(scene, 32, 28, 12000, 1.6, technique=tech), name)


def plane_case(scene, name):
    return S.named(make_plane_case(scene, 32, 28, 6000), name)


# ---- G-BRE -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("scene", ["cbox", "fogroom_rot", "cbox_phong_rot"])
def test_bre3d(scene, name):
    acc, ref, st = check(bre_case(scene, name), exact=True)
    assert st["evaluations"] > 5000 and st["diffuse_shifts"] > 10000


def test_bre3d_centimetres_intended_visibility():
    check(bre_case("fogroom_rot", "centimetres", visibility_as_written=0), exact=True)


def test_bre3d_centimetres_reference_bvh_walk():
    check(bre_case("fogroom_rot", "centimetres"), use_accel=True, exact=True)


def test_bre3d_centimetres_bundle_cells():
    """the ray-bundle cells only select candidates: every counter but `candidates` equals the 3D grid's, and the oracle's"""
    c = bre_case("fogroom_rot", "centimetres")
    a3, s3, k3 = run_bundle(c, False)
    ab, sb, kb = run_bundle(c, True)
    assert k3 == [0] and kb == [1]
    for k in COUNTERS:
        assert sb[k] == s3[k], (k, sb, s3)
    lum = max(a3[..., 0:3].mean(), 1e-30)
    assert np.abs(ab.astype(np.float64) - a3).max() <= 2e-4 * max(np.abs(a3).max(), lum)
    ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, c.it, c.nb, 64)
    for k in COUNTERS:
        assert sb[k] == cnt[k], (k, sb, cnt)


@pytest.mark.parametrize("name", ["large", "centimetres"])
def test_bre2d(name):
    c = bre_case("cbox_rot", name, vol_technique=abi.GVPM_VOL_BRE2D, use_shift_null=0)
    check(c, use_accel=False, exact=True)


# ---- G-VPM -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("scene", ["cbox", "fogroom_rot"])
def test_vpm(scene, name):
    acc, ref, st = device_vpm(vpm_case(scene, name), exact=True)
    assert st["evaluations"] > 5000


# ---- G-Beams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["large", "centimetres"])
@pytest.mark.parametrize("tech", TECHS)
def test_beams(tech, name):
    acc, ref, st = device_beams(beam_case("cbox_rot", tech, name), exact=True)
    assert st["evaluations"] > 10000


@pytest.mark.parametrize("tech", TECHS)
@pytest.mark.parametrize("scene", ["laser_rot", "fogroom"])
def test_beams_centimetres(scene, tech):
    acc, ref, st = device_beams(beam_case(scene, tech, "centimetres"), exact=True)
    assert st["evaluations"] > 10000


def test_beams_small():
    device_beams(beam_case("cbox_rot", B3D, "small"), exact=True)


def test_beams_centimetres_literal_fp64_path(monkeypatch):
    """GVPM_BEAMS_FP64=1, the reference's statements with its float intermediates: the oracle's counters exactly -- which
    tells a band that is too narrow (the fast path alone is off) from an ownership problem (both are)"""
    monkeypatch.setenv("GVPM_BEAMS_FP64", "1")
    device_beams(beam_case("cbox_rot", B3D, "centimetres"), exact=True)


# ---- G-Planes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "large", "centimetres", "far"])
@pytest.mark.parametrize("scene", ["cbox_in", "cbox_in_rot"])
def test_planes(scene, name):
    acc, ref, st = device_planes(plane_case(scene, name), exact=True)
    assert st["evaluations"] > 20000


# ---- invariance on the device alone ------------------------------------------------------------------------------------------
def _counters(st):
    return {k: st[k] for k in COUNTERS}


def test_bre3d_counters_are_scale_invariant_on_the_device():
    """a power-of-two scale about the origin is exact in fp32: the device's own counters cannot move, oracle or no oracle"""
    c = cases.make_case("cbox", 40, 36, 30000, 1.6)
    _, st0, _ = device_gather(c)
    _, st1, _ = device_gather(S.transformed(c, *S.LARGE_AT_ORIGIN))
    assert st0["evaluations"] > 5000
    assert _counters(st1) == _counters(st0)


def _beams_stats(c):
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ctx.upload_beams(c.beams, c.end_n)
    ctx.upload_camera_beams(c.rays)
    ctx.gather(c.it, c.nb)
    st = ctx.stats()
    ctx.close()
    return st


def test_beams3d_counters_are_scale_invariant_on_the_device():
    c = make_beam_case("cbox", 32, 28, 12000, 1.6, technique=B3D)
    st0 = _beams_stats(c)
    st1 = _beams_stats(S.transformed(c, *S.LARGE_AT_ORIGIN))
    assert st0["evaluations"] > 10000
    assert _counters(st1) == _counters(st0)
