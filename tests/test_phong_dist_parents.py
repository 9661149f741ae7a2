"""The Phong / Ashikhmin-Shirley microfacet distribution for glossy parents (GVPM_MICROFACET_PHONG; include/gvpm_hip.h), CPU side: the
constant and the layout, the numpy statement of tests/indep_phong_dist.py against what can be said in closed form (the exponent's
clamp, the normalisation, equal alphas, the pole), the host's two samplers against the statement's pdf (chi-square) and its
weight = eval / pdf for all four kinds that carry the distribution, the slices of the fixture, and the three synthetic scenes."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

import aniso_cases as AC
import cases
import dielectric_cases as DC
import indep_aniso as A
import indep_dielectric as D
import indep_phong_dist as PD
import indep_statements as I
import phong_dist_cases as C
import plastic_cases as PC
from gvpm_amd import abi
from test_plastic_parents import _chi_square, _dirs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
LUM = np.array([0.212671, 0.715160, 0.072169])


# ---- the constant and the layout -----------------------------------------------------------------------------------------------
def test_abi_constant_and_layout():
    header = open(os.path.join(ROOT, "include", "gvpm_hip.h")).read()
    enum = re.search(r"enum \{ GVPM_MICROFACET_BECKMANN = (\d+), GVPM_MICROFACET_GGX = (\d+), GVPM_MICROFACET_PHONG = (\d+) \};", header)
    assert enum and [int(x) for x in enum.groups()] == [0, 1, 3]
    assert (abi.GVPM_MICROFACET_BECKMANN, abi.GVPM_MICROFACET_GGX, abi.GVPM_MICROFACET_PHONG) == (0, 1, 3)
    assert "(2 is not a distribution" in header
    assert abi.BSDF_DTYPE.itemsize == 64 and abi.BSDF_DTYPE.fields["distribution"][1] == 24 and abi.BSDF_DTYPE.fields["sample_visible"][1] == 28
    assert int(re.search(r"#define GVPM_ABI_VERSION (\d+)", header).group(1)) == abi.GVPM_ABI_VERSION
    # the entries the builders make carry the value where the device reads it (row 1, lane z)
    for t in (C.conductor_entry(0.3), C.aniso_entry(0.35, 0.08, AC.SKEW[0]), C.rough_entry(0.1, 0.3, 0.4), C.glass_table(0.25)):
        assert t.view(np.int32).reshape(-1, 16)[0, 6] == 3 and t["sample_visible"][0] == 0


# ---- the statement against closed forms --------------------------------------------------------------------------------------------
def test_the_exponent_is_clamped_at_alpha_one():
    assert PD.exponent(1.0) == 0.0 and PD.exponent(1.2) == 0.0 and PD.exponent(7.0) == 0.0
    assert np.isclose(PD.exponent(0.03), 2.0 / 0.0009 - 2.0) and 2220 < PD.exponent(0.03) < 2221
    mz = np.array([1.0, 0.7, 0.2, 1e-3])
    d, _ = PD.distribution(1.2, 1.2, np.sqrt(1 - mz * mz), 0 * mz, mz)
    assert np.allclose(d, 1.0 / np.pi, rtol=1e-15)
    assert PD.distribution(0.3, 0.3, np.array([1.0]), np.array([0.0]), np.array([0.0]))[0][0] == 0.0      # the horizon
    assert PD.distribution(0.3, 0.3, np.array([0.6]), np.array([0.0]), np.array([-0.8]))[0][0] == 0.0     # below it


@pytest.mark.parametrize("alphas", [(0.03, 0.03), (0.3, 0.3), (1.2, 1.2), (0.12, 0.45)])
def test_the_distribution_is_normalised(alphas):
    """the integral of D cos(theta_m) over the hemisphere is 1: Gauss-Legendre in mu = cos(theta_m) (the integrand is mu^(e + 1) up to
    the azimuth's interpolation: 3 000 nodes cover exponent 2 220), the periodic rectangle rule in phi"""
    au, av = alphas
    x, w = np.polynomial.legendre.leggauss(3000)
    mu, w = 0.5 * (x + 1.0), 0.5 * w
    phi = (np.arange(512) + 0.5) * (2 * np.pi / 512)
    M, P = np.meshgrid(mu, phi, indexing="ij")
    s = np.sqrt(1 - M * M)
    d, raw = PD.distribution(au, av, s * np.cos(P), s * np.sin(P), M)
    total = (raw * w[:, None]).sum() * (2 * np.pi / 512)
    cut = ((raw - d * M) * w[:, None]).sum() * (2 * np.pi / 512)       # what the 1e-20 cut removes
    print(alphas, total, cut)
    assert abs(total - 1.0) < 1e-4 and 0 <= cut < 1e-15


def test_equal_alphas_are_the_isotropic_distribution_and_the_pole_returns_eu():
    rng = np.random.default_rng(3)
    m = _dirs(rng, 4000)
    for a in (0.03, 0.3, 0.9, 1.2):
        e = max(2.0 / (a * a) - 2.0, 0.0)
        d, raw = PD.distribution(a, a, m[:, 0], m[:, 1], m[:, 2])
        want = (e + 2.0) / (2 * np.pi) * m[:, 2] ** e
        want = np.where(want * m[:, 2] >= 1e-20, want, 0.0)
        assert np.abs(d - want).max() <= 1e-12 * want.max()
    # sin^2(theta_m) = 0 (and anything at or below 2^-128): eU, whatever the tangential components
    z = np.array([0.0])
    assert PD.interpolated_exponent(0.12, 0.45, z, z, z + 1.0)[0] == PD.exponent(0.12)
    # away from the pole the exponent runs from eU along the tangent to eV across it
    assert PD.interpolated_exponent(0.12, 0.45, z + 0.6, z, z + 0.8)[0] == pytest.approx(PD.exponent(0.12), rel=1e-14)
    assert PD.interpolated_exponent(0.12, 0.45, z, z + 0.6, z + 0.8)[0] == pytest.approx(PD.exponent(0.45), rel=1e-14)


def test_g1_is_beckmanns_with_alpha_not_the_exponent():
    """smithG1 switches on EPhong together with EBeckmann (microfacet.h:489-501): the statement's G1 equals indep_dielectric's Beckmann
    form at the same alpha"""
    rng = np.random.default_rng(4)
    v = _dirs(rng, 2000)
    vm = rng.random(2000) * 2 - 1
    for a in (0.03, 0.3, 1.2):
        g = PD.smith_g1(a, a, v[:, 0], v[:, 1], v[:, 2], vm)
        assert np.allclose(g, D.smith_g1(np.zeros(2000, bool), a, v[:, 2], vm), rtol=1e-13, atol=0)


def test_the_wrapper_hands_other_entries_on_untouched(monkeypatch):
    c = cases.make_case("cbox_conductor", 12, 10, 500, 4.0)
    table = np.concatenate([c.bsdfs, C.conductor_table(0.3)])
    rng = np.random.default_rng(6)
    wi, wo = _dirs(rng, 64), _dirs(rng, 64)
    n, kd = np.broadcast_to([0.0, 0.0, 1.0], (64, 3)), np.zeros((64, 3))
    I.set_bsdfs(table)
    base = I.phong_world(kd, np.zeros(64, np.int64), n, wi, wo)
    as_beckmann = I.phong_world(kd, np.full(64, 2), n, wi, wo)
    PD.install(monkeypatch)
    got = I.phong_world(kd, np.zeros(64, np.int64), n, wi, wo)
    assert all(np.array_equal(a, b) for a, b in zip(base, got))
    mine = I.phong_world(kd, np.full(64, 2), n, wi, wo)
    assert mine[2].all() and np.abs(mine[1] - as_beckmann[1]).max() > 1e-3      # (the unwrapped statement reads it as Beckmann)
    assert not I.phong_world(kd, np.full(64, 4), n, wi, wo)[2].any() and not I.phong_world(kd, np.full(64, -1), n, wi, wo)[2].any()
    cases.use_bsdfs(c)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def test_the_fixtures_slices():
    stored = np.load(C.GOLDEN)
    assert sorted(stored.files) == sorted(f"phong_eta1.5_alpha{a}" for a in ("0.1", "0.3", "0.03"))
    for k, v in stored.items():
        assert v.dtype == np.float32 and v.shape == (101,) and np.isfinite(v).all() and (v >= 0).all() and (v <= 1).all() and 0 <= v[100] < 1, k
        assert (v[:100] >= np.finfo(np.float32).tiny).all()     # (no subnormal word: gvpm_upload_bsdfs refuses them)
        assert v[99] > 0.9 and v[0] < v[99]
    # a rougher coating lets more through at grazing incidence; the three are different slices
    assert stored["phong_eta1.5_alpha0.03"][0] < stored["phong_eta1.5_alpha0.1"][0] < stored["phong_eta1.5_alpha0.3"][0]
    # where the reference's tables are at hand: the fixture is what its generator derives from them, bit for bit
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        spec = importlib.util.spec_from_file_location("make_rtrans_phong_golden", os.path.join(HERE, "golden", "make_rtrans_phong_golden.py"))
        G = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(G)
    finally:
        sys.path.remove(os.path.join(HERE, "golden"))
    if os.path.isdir(G.DATA_DIR):
        fresh = G.make()
        assert set(fresh) == set(stored.files)
        for k, v in fresh.items():
            assert np.array_equal(v.view(np.uint32), stored[k].view(np.uint32)), k


# ---- the scenes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ["", "_rot"])
@pytest.mark.parametrize("scene", C.SCENES)
def test_the_scenes_generate_and_their_photons_name_phong_distribution_heads(scene, rot):
    c = C.make_case(scene + rot, 20, 16, 20000, 4.0)
    heads = abi.bsdf_heads(c.bsdfs)
    mine = PD.is_phong_dist(c.bsdfs)
    assert mine.sum() == 2 and np.array_equal(mine, heads) and not c.bsdfs["sample_visible"][heads].any()
    kinds = {"cbox_conductor_phong": [abi.GVPM_BSDF_ROUGHCONDUCTOR, abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO],
             "cbox_roughplastic_phong": [abi.GVPM_BSDF_ROUGHPLASTIC] * 2, "cbox_roughglass_phong": [abi.GVPM_BSDF_ROUGHDIELECTRIC] * 2}[scene]
    assert list(c.bsdfs["kind"][heads]) == kinds
    gl = (c.ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    idx = c.ph.parent_g[gl].astype(np.int64)
    assert gl.sum() >= 1000 and mine[idx].all() and set(np.unique(idx)) == set(np.flatnonzero(heads))
    assert (((c.ph.flags[gl] >> 2) & 7) == 1).all()          # roughness above bounceRoughness: diffuse reconnections
    if scene == "cbox_conductor_phong":
        assert np.allclose(c.bsdfs["exponent"][heads], [0.3, 0.35]) and np.isclose(abi.frame_of(c.bsdfs, 1)[1], 0.08)
        s = abi.frame_of(c.bsdfs, 1)[0]
        assert abs(np.linalg.norm(s) - 1) < 1e-6
    elif scene == "cbox_roughplastic_phong":
        assert np.allclose(c.bsdfs["exponent"][heads], [0.1, 0.3]) and (c.bsdfs["k"][heads, 0] == 0).all()      # both components
        assert np.array_equal(abi.rtrans_of(c.bsdfs, 0), C.rtrans(1.5, 0.1)[0])
    else:
        assert np.allclose(c.bsdfs["exponent"][heads], DC.ALPHA) and np.allclose(c.bsdfs["eta"][heads, 0], [1.5, 1 / 1.5])
        tr, _ = D.is_transmitted(c.ph, c.bsdfs)
        assert tr.sum() > 300 and (gl & ~tr).sum() > 100
    cases.use_bsdfs(cases.make_case("cbox", 8, 8, 10, 4.0))


def test_the_plastic_scene_refuses_to_shoot_without_its_slices():
    from gvpm_amd.host import SynthScene
    sc = SynthScene("cbox_roughplastic_phong", 8, 8)
    assert [m[1:] for m in sc.rtrans_materials()] == [("phong", pytest.approx(0.1), 1.5), ("phong", pytest.approx(0.3), 1.5)]
    with pytest.raises(RuntimeError):
        sc.shoot_photons(1, 100)


# ---- the host's samplers -----------------------------------------------------------------------------------------------------------
def _material(sc, sampler):
    for mat in range(64):
        try:
            getattr(sc, sampler)(mat, (0.0, 0.0, 1.0), (0.0, 0.0, 1.0), 0.5, 0.5)
            return mat
        except ValueError:
            pass
    raise AssertionError(sampler)


TANGENT = np.array([0.9, 0.35, 0.25]) / np.linalg.norm([0.9, 0.35, 0.25])


def _conductor_statement(wall, n, wi, wo):
    """the two walls of cbox_conductor_phong with the host's own double-precision parameters (synth.cpp)"""
    k = len(wo)
    one = lambda x: np.broadcast_to(np.asarray(x, np.float64), (k, 3))
    if wall == 0:
        return PD.conductor_rows(one(1.0), 0.3, 0.3, PD.any_tangent(one(n)), one(C.CU[0]), one(C.CU[1]), one(n), one(wi), wo, count=False)
    return PD.conductor_rows(one(1.0), 0.35, 0.08, one(TANGENT), one(C.AL[0]), one(C.AL[1]), one(n), one(wi), wo, count=False)


@pytest.mark.parametrize("wall", [0, 1])
def test_sampling_matches_the_statements_pdf_chi_square(wall):
    """sampleAll of the distribution through the host's conductor bounce -- wall 0: isotropic (phi = 2 pi u2, cos = u1^(1 / (e + 2))),
    wall 1: Ashikhmin-Shirley's four quadrants -- against the statement's pdf, 10 x 20 bins at significance 0.01"""
    from gvpm_amd.host import SynthScene
    sc = SynthScene("cbox_conductor_phong", 8, 8)
    mat = _material(sc, "sample_conductor" if wall == 0 else "sample_aniso")
    n = AC.WALL_N[wall]
    rng = np.random.default_rng(61 + wall)
    u, v, _ = A.frame(np.array([[0.3, 0.5, 0.2]]), n[None, :])
    to_world = lambda d: d[..., 0:1] * u + d[..., 1:2] * v + d[..., 2:3] * n
    to_local = lambda d: np.stack([(d * u).sum(-1), (d * v).sum(-1), (d * n).sum(-1)], -1)
    bounce = sc.sample_conductor if wall == 0 else sc.sample_aniso

    def sample(wi_l, count):
        wi = to_world(wi_l)[0]
        res = [bounce(mat, n, wi, *rng.random(2)) for _ in range(count)]
        ok = [r for r in res if r is not None]
        return to_local(np.array([r[0] for r in ok])), len(res) - len(ok)

    def pdf_of(wi_l, dirs_l):
        return _conductor_statement(wall, n, to_world(wi_l)[0], to_world(dirs_l))[1]

    _chi_square(sample, pdf_of, rng, 6, 30000)


def test_conductor_weight_is_eval_over_pdf_to_1e9():
    from gvpm_amd.host import SynthScene
    sc = SynthScene("cbox_conductor_phong", 8, 8)
    rng = np.random.default_rng(71)
    for wall, sampler in enumerate(("sample_conductor", "sample_aniso")):
        mat, n = _material(sc, sampler), AC.WALL_N[wall]
        u, v, _ = A.frame(np.array([[0.3, 0.5, 0.2]]), n[None, :])
        wis = _dirs(rng, 600)
        wis = wis[:, 0:1] * u + wis[:, 1:2] * v + wis[:, 2:3] * n
        checked = 0
        for wi in wis:
            r = getattr(sc, sampler)(mat, n, wi, *rng.random(2))
            if r is None:
                continue
            wo, weight, pdf = r
            f, p, d = _conductor_statement(wall, n, wi, wo[None, :])
            assert d[0] and abs(p[0] - pdf) <= 1e-9 * pdf, (wall, p, pdf)
            assert np.allclose(f[0] / p[0], weight, rtol=1e-9, atol=1e-300)
            checked += 1
        assert checked > 250, (wall, checked)


def test_plastic_weight_is_eval_over_pdf_to_1e9():
    sc = C.scene("cbox_roughplastic_phong", 8, 8)
    n = np.array([0.0, 0.0, 1.0])
    rng = np.random.default_rng(72)
    host = [(0.1, (0.7, 0.7, 0.7), (1.0, 1.0, 0.9), False), (0.3, (0.6, 0.7, 0.9), (0.9, 0.9, 0.9), True)]
    for (mat, dist, _, _), (alpha, kd, ks, nonlinear) in zip(sc.rtrans_materials(), host):
        sl, fdr = C.rtrans(1.5, alpha)
        w = (LUM @ ks) / (LUM @ kd + LUM @ ks)
        checked = {0x0: 0}
        for wi in _dirs(rng, 500):
            r = sc.sample_plastic(mat, n, wi, *rng.random(2))
            if r is None:
                continue
            wo, weight, pdf, comp = r
            assert comp == -1
            one = lambda x: np.asarray(x, np.float64)[None]
            f, p, d = PD.plastic_rows(one(ks), alpha, w, 1.5, np.array([fdr]), np.array([0]), np.array([nonlinear]), sl.astype(np.float64)[None],
                                      one(kd), one(n), one(wi), one(wo), count=False)
            assert d[0] and abs(p[0] - pdf) <= 1e-9 * pdf
            assert np.allclose(f[0] / p[0], weight, rtol=1e-9, atol=1e-300)
            checked[0] += 1
        assert checked[0] > 300


def test_dielectric_weight_times_pdf_is_the_statements_eval():
    """all four classes (reflected / transmitted x wi outside / inside), 2 000 sampled directions each, to 1e-9"""
    from gvpm_amd.host import SynthScene
    sc = SynthScene("cbox_roughglass_phong", 8, 8)
    mat = DC.dielectric_material(sc)
    N = np.array([0.0, 0.0, 1.0])
    rng = np.random.default_rng(73)
    got = {(t, s): [] for t in (0x8, 0x10) for s in (1, -1)}
    while min(len(v) for v in got.values()) < 2000:
        side = 1 if rng.random() < 0.3 else -1
        z = 0.05 + 0.95 * rng.random() if side == 1 else 0.6 + 0.4 * rng.random()
        ph = 2 * np.pi * rng.random()
        wi = np.array([np.sqrt(1 - z * z) * np.cos(ph), np.sqrt(1 - z * z) * np.sin(ph), side * z])
        r = sc.sample_dielectric(mat, N, wi, *rng.random(3))
        if r is not None and len(got[(r[3], side)]) < 2000:
            got[(r[3], side)].append((wi, r[0], r[1], r[2]))
    for key, rows in got.items():
        wi, wo, weight, pdf = (np.array([r[j] for r in rows]) for j in range(4))
        k = len(rows)
        f, p, defined = PD.dielectric_rows(np.array(DC.KS), np.array(DC.KT), np.full(k, DC.ALPHA), np.full(k, DC.ETA),
                                           np.broadcast_to(N, wi.shape), wi, wo, count=False)
        assert defined.all() and (f > 0).all(), key
        assert np.abs(p / pdf - 1).max() < 1e-9, (key, np.abs(p / pdf - 1).max())
        assert np.abs(weight * pdf[:, None] / f - 1).max() < 1e-9, key


@pytest.mark.parametrize("scene", ["cbox_conductor_phong", "cbox_roughplastic_phong"])
def test_the_hosts_bounce_is_weight_times_pdf_equals_eval_in_the_records(scene):
    """flux = prefix * (f cos / pdf) * rr * (Tr / edgePdf) and pdf in solid angle = the stored area pdf * len^2 of the photons behind
    each wall, against the statement on the float32 table (the records are float32)"""
    c = C.make_case(scene, 20, 16, 20000, 4.0)
    all_gl = np.flatnonzero((c.ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF)
    for h in np.flatnonzero(abi.bsdf_heads(c.bsdfs)):
        gl = all_gl[c.ph.parent_g[all_gl] == h][:400]
        assert gl.size >= 10, (h, gl.size)
        d = c.ph.pos[gl].astype(np.float64) - c.ph.parent_pos[gl]
        ln = np.linalg.norm(d, axis=1)
        wo = d / ln[:, None]
        f, pdf, known = PD.phong_world_with_phong_dist(c.ph.parent_scat[gl].astype(np.float64), c.ph.parent_g[gl].astype(np.int64),
                                                       c.ph.parent_n[gl].astype(np.float64), c.ph.parent_wi[gl].astype(np.float64), wo)
        assert known.all() and (pdf > 0).all()
        assert np.allclose(pdf, c.ph.parent_pdf[gl] * ln * ln, rtol=4e-4), h
        tr = np.exp(-float(c.m.sigma_t[0]) * ln)
        want = c.ph.prefix_w[gl] * (f / pdf[:, None]) * c.ph.parent_rr[gl][:, None] * (tr / c.ph.edge_pdf[gl])[:, None]
        assert np.allclose(c.ph.flux[gl], want, rtol=6e-4), h
    cases.use_bsdfs(cases.make_case("cbox", 8, 8, 10, 4.0))
