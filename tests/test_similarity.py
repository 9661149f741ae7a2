"""The similarity helper (tests/similarity_cases.py) against the fp64 oracle, on the CPU.

What a transform must and must not change is known without any device:

  * a power-of-two scale about the origin (with Epsilon scaled along) is exact in fp32 -- every input keeps its mantissa -- so
    the oracle's evaluated set and every shift decision are the untransformed case's, counter for counter.  A position or
    length field the helper forgot moves the counters by orders of magnitude; a constant of the reference's that is a
    length in disguise shows as a small difference and is named below;
  * a translation by a few room widths re-rounds every coordinate: the counters move by a handful of borderline pairs and
    the accumulators by the rounding of the inputs;
  * `centimetres` (a 256-wide room 1400 from the origin, Epsilon still 1e-4) and `far` (the unit room 2300 from the origin)
    put Epsilon below the ulp of a coordinate: parents land behind their own walls and self-hit, and the failed shifts of a
    scene with occluders rise well above the untransformed run's.  That is the regime tests/test_similarity_gpu.py is about.
"""
import functools

import numpy as np
import pytest

import cases
import oracle_lib as O
import similarity_cases as S
from gvpm_amd import abi
from test_oracle_beams import make_beam_case
from test_oracle_planes import make_plane_case
from test_oracle_vpm import make_vpm_case

COUNTERS = O.COUNTER_NAMES     # evaluations, candidates, null_shifts, diffuse_shifts, failed_shifts

# technique -> (builder at the shapes of test_similarity_gpu.py, Lambertian scene, rotated scene with occluders)
MAKE = {
    "bre3d": (lambda s: cases.make_case(s, 40, 36, 30000, 1.6), "cbox", "fogroom_rot"),
    "vpm": (lambda s: make_vpm_case(s, 32, 28, 40000, 3.1, nb=10), "cbox", "fogroom_rot"),
    "beams3d": (lambda s: make_beam_case(s, 32, 28, 12000, 1.6, technique=abi.GVPM_BEAM_BEAM_3D_OPTIMIZED), "cbox", "fogroom_rot"),
    "beams1d": (lambda s: make_beam_case(s, 32, 28, 12000, 1.6, technique=abi.GVPM_BEAM_BEAM_1D), "cbox", "fogroom_rot"),
    "planes": (lambda s: make_plane_case(s, 32, 28, 6000), "cbox_in", "cbox_in_rot"),
}
CASES = [(k, s) for k, (_, a, b) in MAKE.items() for s in (a, b)]
NAMED = dict(S.TRANSFORMS, large_at_origin=S.LARGE_AT_ORIGIN)


def oracle(kind, c):
    if kind == "bre3d":
        acc, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, c.it, c.nb, 64, use_accel=False)
    elif kind == "vpm":
        acc, _, _, cnt, _ = O.gather_vpm(c.p, c.m, c.tris, c.ph, c.rays, c.samples, 64, use_accel=False)
    elif kind in ("beams3d", "beams1d"):
        acc, cnt, _ = O.gather_beams(c.p, c.m, c.tris, c.beams, c.end_n, c.rays, c.r, c.it, c.nb, 64)
    else:
        acc, cnt, _ = O.gather_planes(c.p, c.m, c.tris, c.beams, c.w1, c.len1, c.rays, c.it, c.nb, 64)
    return acc, cnt


@functools.lru_cache(maxsize=None)
def base(kind, scene):
    """the untransformed case and its oracle run, computed once and shared (nothing below writes to them)"""
    c = MAKE[kind][0](scene)
    acc, cnt = oracle(kind, c)
    return c, acc, cnt


def run(kind, scene, name):
    c, _, _ = base(kind, scene)
    cases.use_bsdfs(c)
    return oracle(kind, S.transformed(c, *NAMED[name]))


# ---- the helper itself -----------------------------------------------------------------------------------------------------
def test_every_record_field_is_classified_and_an_unknown_one_raises(monkeypatch):
    assert set(S.PHOTON_FIELDS) == set(abi.PHOTON_VEC3 + abi.PHOTON_F1)
    assert set(S.RAY_FIELDS) == set(abi.CAMERA_RAY_DTYPE.names)
    assert S.RAY_FIELDS["eye"] == S.KEEP                                    # a weight, not a position
    c, _, _ = base("bre3d", "cbox")
    monkeypatch.setattr(abi, "PHOTON_F1", abi.PHOTON_F1 + ["a_field_added_later"])
    with pytest.raises(KeyError, match="a_field_added_later"):
        S.transform_records(c.ph, 2.0, (0, 0, 0))
    with pytest.raises(AssertionError):
        S.transformed(c, 3.0)                                               # not a power of two


def test_what_moves_and_what_does_not():
    s, t, _ = S.TRANSFORMS["large"]
    t64 = np.asarray(t, np.float64)
    for kind, scene in (("bre3d", "fogroom_rot"), ("vpm", "cbox"), ("beams3d", "cbox"), ("planes", "cbox_in_rot")):
        c, _, _ = base(kind, scene)
        q = S.transformed(c, s, t, True)
        recs = [(c.ph, q.ph)] + ([(c.beams, q.beams)] if hasattr(c, "beams") else [])
        for a, b in recs:
            for k in abi.PHOTON_VEC3 + abi.PHOTON_F1 + abi.PHOTON_U1:
                if k in ("pos", "parent_pos"):
                    assert np.array_equal(getattr(b, k), (getattr(a, k).astype(np.float64) * s + t64).astype(np.float32)), k
                    assert getattr(b, k).dtype == np.float32
                else:
                    assert np.array_equal(getattr(b, k), getattr(a, k)), k
        for k in abi.CAMERA_RAY_DTYPE.names:
            if k == "o":
                assert np.array_equal(q.rays[k], (c.rays[k].astype(np.float64) * s + t64).astype(np.float32))
            elif k == "len":
                assert np.array_equal(q.rays[k], c.rays[k] * np.float32(s))
            else:
                assert np.array_equal(q.rays[k], c.rays[k]), k
        assert np.array_equal(q.tris[0], (c.tris[0].astype(np.float64) * s + t64).astype(np.float32))
        assert np.array_equal(q.tris[1], c.tris[1] * np.float32(s)) and np.array_equal(q.tris[2], c.tris[2] * np.float32(s))
        assert q.p.bsphere_radius == c.p.bsphere_radius * s and q.p.epsilon == c.p.epsilon * s
        assert q.p.shadow_epsilon == c.p.shadow_epsilon                     # a ratio of the reconnection distance
        assert q.r == cases.radius_of(q.p) == c.r * s
        for k in ("sigma_a", "sigma_s", "sigma_t"):
            assert list(getattr(q.m, k)) == [v / s for v in getattr(c.m, k)]
        assert q.m.sigma_t[0] == q.m.sigma_t[1] == q.m.sigma_t[2] > 0         # what the medium upload insists on
        assert q.m.g == c.m.g and q.nb == c.nb and q.it == c.it
        if hasattr(c, "len1"):
            assert np.array_equal(q.len1, c.len1 * np.float32(s)) and np.array_equal(q.w1, c.w1)
        if hasattr(c, "end_n"):
            assert np.array_equal(q.end_n, c.end_n)
        if hasattr(c, "samples"):
            assert np.array_equal(q.samples, c.samples)
        # the original is left alone
        assert c.p.bsphere_radius * s == q.p.bsphere_radius and not np.array_equal(c.ph.pos, q.ph.pos)
    keep = S.transformed(c, 256.0, (1, 2, 3), False)
    assert keep.p.epsilon == c.p.epsilon and keep.p.bsphere_radius == c.p.bsphere_radius * 256


# ---- pure scales: exact -------------------------------------------------------------------------------------------------
# G-Planes, `small`: the reference's ray / parallelogram test refuses |det| < 1e-5 (pm/plane_struct.h:104-135) with
# det = e0 . (d x e1) over the plane's two FULL edges -- an area, which a scale s takes to s^2 det.  At s = 1 / 64 every pair
# with |det| < 1e-5 * 4096 in the room's own units is refused, 1.5 % of them; at s = 64 the threshold only loosens, and no
# pair of these cases lies under it.  So `small` drops pairs (and only drops them); everything else about it stays exact.
PLANE_DET_MIN = 1e-5


def plane_pairs_with_det_between(c, lo, hi):
    """pairs the 0D estimator evaluates (numpy statement of test_oracle_planes.numpy_plane0d_base) with lo <= |det| < hi"""
    ori = c.beams.parent_pos.astype(np.float64)
    e0 = c.beams.pos.astype(np.float64) - ori
    e1 = c.w1.astype(np.float64) * c.len1.astype(np.float64)[:, None]
    eps, n = float(c.p.epsilon), 0
    for s in range(c.rays.shape[0]):
        b = c.rays[s, 0]
        if not (int(b["info"]) & 1):
            continue
        o, d, L = b["o"].astype(np.float64), b["d"].astype(np.float64), float(b["len"])
        P = np.cross(d, e1)
        det = (e0 * P).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            T = o - ori
            t0 = (T * P).sum(1) * inv
            Q = np.cross(T, e0)
            t1 = (Q @ d) * inv
            tc = (e1 * Q).sum(1) * inv
        ok = (t0 >= 0) & (t0 <= 1) & (t1 >= 0) & (t1 <= 1) & (tc > eps) & (tc < L - eps)
        n += int((ok & (np.abs(det) >= lo) & (np.abs(det) < hi)).sum())
    return n


@pytest.mark.parametrize("name", ["small", "large_at_origin"])
@pytest.mark.parametrize("kind,scene", CASES)
def test_power_of_two_scale_keeps_every_counter(kind, scene, name):
    _, _, cnt0 = base(kind, scene)
    _, cnt = run(kind, scene, name)
    assert cnt0["evaluations"] > 5000 and cnt0["diffuse_shifts"] > 10000
    if kind == "planes" and name == "small":
        c, _, _ = base(kind, scene)
        lost = plane_pairs_with_det_between(c, PLANE_DET_MIN, PLANE_DET_MIN * 64 ** 2)
        assert 0.005 * cnt0["evaluations"] < lost < 0.03 * cnt0["evaluations"]
        # (the numpy statement forms det in plain doubles, the reference through float intermediates: +-2 as in test_oracle_planes)
        assert abs((cnt0["evaluations"] - cnt["evaluations"]) - lost) <= 2, (cnt0, cnt, lost)
        # every lost pair takes its four shifts along: at most 4 per pair, and nothing is gained
        for k in ("diffuse_shifts", "failed_shifts"):
            assert 0 <= cnt0[k] - cnt[k] <= 4 * (lost + 2), (k, cnt0, cnt)
        assert (cnt0["diffuse_shifts"] + cnt0["failed_shifts"]) - (cnt["diffuse_shifts"] + cnt["failed_shifts"]) \
            == 4 * (cnt0["evaluations"] - cnt["evaluations"])
        return
    for k in COUNTERS:
        assert cnt[k] == cnt0[k], (k, cnt, cnt0)


def test_shadow_epsilon_is_a_ratio_not_a_length():
    """What scaling ShadowEpsilon like a length does: lProj * ShadowEpsilon grows 64-fold relative to the reconnection and two
    shadow segments of fogroom_rot reach an occluder.  The helper leaves it alone; this keeps it from being 'fixed'."""
    c, _, cnt0 = base("bre3d", "fogroom_rot")
    cases.use_bsdfs(c)
    q = S.transformed(c, *S.LARGE_AT_ORIGIN)
    q.p.shadow_epsilon = c.p.shadow_epsilon * 64
    _, cnt = oracle("bre3d", q)
    assert cnt["evaluations"] == cnt0["evaluations"] and cnt["null_shifts"] == cnt0["null_shifts"]
    assert cnt["failed_shifts"] > cnt0["failed_shifts"]


@pytest.mark.parametrize("scene", ["cbox", "fogroom_rot", "cbox_phong_rot"])
def test_bre3d_scale_and_intended_visibility(scene):
    c = cases.make_case(scene, 40, 36, 30000, 1.6, visibility_as_written=0)
    _, cnt0 = oracle("bre3d", c)
    for xf in ((1.0 / 64, (0, 0, 0), True), S.LARGE_AT_ORIGIN):
        _, cnt = oracle("bre3d", S.transformed(c, *xf))
        for k in COUNTERS:
            assert cnt[k] == cnt0[k], (k, cnt, cnt0)


# ---- a translation by a few room widths ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,scene", CASES)
def test_shifted_room_gives_the_same_estimate(kind, scene):
    _, acc0, cnt0 = base(kind, scene)
    acc, cnt = run(kind, scene, "shifted")
    assert abs(cnt["evaluations"] - cnt0["evaluations"]) <= 1e-3 * cnt0["evaluations"], (cnt, cnt0)
    lum = acc0[..., 0:3].mean()
    err = float(np.sqrt(((acc - acc0) ** 2).mean()) / lum)
    print(f"{kind} {scene}: shifted vs none: evaluations {cnt['evaluations']} / {cnt0['evaluations']}, L2 / lum {err:.2e}")
    assert err < 1e-4, err


# ---- Epsilon below the ulp of a coordinate ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["centimetres", "far"])
@pytest.mark.parametrize("kind", ["bre3d", "vpm", "beams3d", "beams1d"])
def test_self_hit_regime_is_reached(kind, name):
    """fogroom_rot: parents rounded behind their own walls self-hit -- failed shifts well above the untransformed run's"""
    _, _, cnt0 = base(kind, "fogroom_rot")
    _, cnt = run(kind, "fogroom_rot", name)
    print(f"{kind} fogroom_rot {name}: failed shifts {cnt['failed_shifts']} against {cnt0['failed_shifts']}")
    assert cnt["failed_shifts"] > 1.5 * cnt0["failed_shifts"], (cnt, cnt0)
    assert abs(cnt["evaluations"] - cnt0["evaluations"]) <= 1e-3 * cnt0["evaluations"]
