"""Plastic surface parents (GVPM_BSDF_ROUGHPLASTIC, GVPM_BSDF_PLASTIC; include/gvpm_hip.h), CPU side: the transmittance fixture
and its generator, the numpy statement of the two BSDFs (tests/indep_plastic.py), and the two limits in which the frozen
fp64 oracle already states what they compute -- the Lambertian surface (eta = 1, Fdr = 0, T = 1) and the rough conductor
with k = 0 (glossy component alone, T = 0)."""
import importlib.util
import os

import numpy as np
import pytest

import cases
import indep_plastic as P
import indep_statements as I
import oracle_lib as O
import plastic_cases as PC
from gvpm_amd import abi
from test_oracle_beams import make_beam_case
from test_oracle_vpm import make_vpm_case

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["flux"] + [f"shifted[{i}]" for i in range(4)] + [f"weighted[{i}]" for i in range(4)]
COUNTERS = ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts")


def generator():
    spec = importlib.util.spec_from_file_location("make_rtrans_golden", os.path.join(HERE, "golden", "make_rtrans_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_its_generator_derives_from_the_reference_tables():
    G = generator()
    if not os.path.isdir(G.DATA_DIR):
        pytest.skip("the reference tree is not on this machine")
    fresh, stored = G.make(), np.load(PC.GOLDEN)
    assert set(fresh) == set(stored.files)
    for k, v in fresh.items():
        assert v.dtype == np.float32 and stored[k].dtype == np.float32 and np.array_equal(v.view(np.uint32), stored[k].view(np.uint32)), k


def test_fixture_anchors_and_ranges():
    """T(1), T(0) and Fdr of the two surfaces of cbox_roughplastic as an fp64 evaluation of the reference's tables gives them"""
    for (dist, alpha), (t1, t0, fdr) in {("beckmann", 0.1): (0.9600, 0.3680, 0.5952), ("ggx", 0.3): (0.9528, 0.6363, 0.5982)}.items():
        sl, f = PC.rtrans(dist, 1.5, alpha)
        assert abs(sl[99] - t1) < 5e-5 and abs(sl[0] - t0) < 5e-5 and abs(f - fdr) < 5e-5
    for k, v in np.load(PC.GOLDEN).items():
        assert v.shape == (101,) and np.isfinite(v).all() and (v >= 0).all() and (v <= 1).all() and 0 <= v[100] < 1, k
        assert (v[:100] >= np.finfo(np.float32).tiny).all()     # (no subnormal word: gvpm_upload_bsdfs refuses them)


def test_the_spline_is_the_cubic_hermite_spline_of_its_knot_derivatives():
    from scipy.interpolate import CubicHermiteSpline
    G = generator()
    sl, _ = PC.rtrans("ggx", 1.5, 0.3)
    v = sl.astype(np.float64)
    x = np.arange(100) / 99.0
    d = np.empty(100)
    d[1:-1] = 0.5 * (v[2:] - v[:-2])
    d[0], d[-1] = v[1] - v[0], v[-1] - v[-2]
    ref = CubicHermiteSpline(x, v, d * 99.0)
    q = np.concatenate([np.random.default_rng(5).random(4000), [0.0, 1.0, 0.5 / 99, 98.5 / 99]])
    for f in (P.catmull_rom, G.spline_eval):
        assert np.abs(f(v, q) - ref(q)).max() < 1e-14
        assert np.abs(f(v, x) - v).max() < 1e-14            # at the knots: the knots
    # the clamp and the warp: T(c) reads the spline at c^(1/4)
    c = np.linspace(0, 1, 1001)
    assert np.allclose(P.transmittance(v, c), np.clip(ref(c ** 0.25), 0, 1), atol=1e-14)


# ---- the statement ------------------------------------------------------------------------------------------------------------
def _dirs(rng, k):
    v = rng.normal(size=(k, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[:, 2] = np.abs(v[:, 2])
    return v


@pytest.mark.parametrize("which", ["rough", "rough1", "smooth"])
def test_reciprocity_positivity_and_the_component_probability(which):
    """f(wi, wo) = f cos / cos_o is symmetric in its arguments (both terms are: F D G / (4 ci co), and T(ci) T(co)); f >= 0;
    0 <= pS <= 1; one-component entries add up to the both-component entry"""
    table, heads = PC.plastic_tables(which)
    rng = np.random.default_rng(9)
    k = 4000
    n = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (k, 3))
    wi, wo = _dirs(rng, k), _dirs(rng, k)
    wi[:200, 2], wo[200:400, 2] = 1e-3, 1e-3    # grazing
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    kd = np.broadcast_to(np.array([0.5, 0.4, 0.3]), (k, 3))
    for h in heads:
        idx = np.full(k, h)
        f, pdf, ok = P.plastic_world(table, kd, idx, n, wi, wo)
        fr, _, _ = P.plastic_world(table, kd, idx, n, wo, wi)
        assert ok.all() and (f >= 0).all() and (pdf >= 0).all() and np.isfinite(f).all() and np.isfinite(pdf).all()
        a, b = f / wo[:, 2:3], fr / wi[:, 2:3]
        assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max()
        b_ = table[h]
        Ti = (P.transmittance(abi.rtrans_of(table, h), wi[:, 2]) if b_["kind"] == abi.GVPM_BSDF_ROUGHPLASTIC
              else 1 - P.fresnel_dielectric(wi[:, 2], float(b_["eta"][0])))
        pS = P.prob_specular(Ti, float(b_["specular_sampling_weight"]))
        assert (pS >= 0).all() and (pS <= 1).all()
    if which == "rough1":
        both = table.copy()
        both["k"][heads[0], 0] = 0
        f0, p0, _ = P.plastic_world(both, kd, np.full(k, heads[0]), n, wi, wo)
        f1, p1, _ = P.plastic_world(table, kd, np.full(k, heads[0]), n, wi, wo)
        f2, p2, _ = P.plastic_world(table, kd, np.full(k, heads[1]), n, wi, wo)
        assert np.allclose(f1 + f2, f0, rtol=1e-12) and np.allclose(p1 + p2, p0, rtol=1e-12) and (f1 > 0).any() and (f2 > 0).all()


def test_fresnel_vanishes_at_eta_one_and_the_conductors_at_k_zero():
    c = np.linspace(1e-3, 1, 100001)
    # (sqrt(c^2) against c: one rounding, over c >= 1e-3 and squared)
    assert (P.fresnel_dielectric(c, 1.0) < 1e-20).all()
    nn = 1.5 + 0j
    root = np.sqrt(nn * nn - (1 - c * c))
    F = 0.5 * (np.abs((c - root) / (c + root)) ** 2 + np.abs((nn * nn * c - root) / (nn * nn * c + root)) ** 2)
    assert np.abs(P.fresnel_dielectric(c, 1.5) / F - 1).max() < 1e-13


def test_the_wrapper_leaves_the_other_kinds_alone_and_fails_raw_entries(monkeypatch):
    c = cases.make_case("cbox_conductor", 12, 10, 500, 4.0)
    table = np.concatenate([PC.rough_entry("beckmann", 0.1, 0.3, 0.4), c.bsdfs])
    rng = np.random.default_rng(2)
    k = 64
    n, wi, wo, kd = np.broadcast_to([0.0, 0, 1], (k, 3)), _dirs(rng, k), _dirs(rng, k), np.full((k, 3), 0.4)
    I.set_bsdfs(c.bsdfs)
    f_c, p_c, _ = I.phong_world(kd, np.zeros(k, np.int64), n, wi, wo)
    I.set_bsdfs(table)
    P.install(monkeypatch)
    f, p, known = I.phong_world(kd, np.full(k, PC.E), n, wi, wo)
    assert known.all() and np.array_equal(f, f_c) and np.array_equal(p, p_c)
    for raw in range(1, PC.E):
        assert not I.phong_world(kd, np.full(k, raw), n, wi, wo)[2].any()
    f, p, known = I.phong_world(kd, np.zeros(k, np.int64), n, wi, wo)
    assert known.all() and (p > 0).all()
    assert not I.phong_world(kd, np.full(k, -1), n, wi, wo)[2].any() and not I.phong_world(kd, np.full(k, table.size), n, wi, wo)[2].any()


# ---- the limits the fp64 oracle states ----------------------------------------------------------------------------------------
def _same(acc, cnt, ref, rcnt, tol=1e-9):
    for k in COUNTERS:
        assert cnt[k] == rcnt[k], (k, cnt, rcnt)
    lum = ref[..., 0:3].mean()
    for j, name in enumerate(NAMES):
        err = np.abs(acc[..., 3 * j:3 * j + 3] - ref[..., 3 * j:3 * j + 3]).max() / lum
        assert err < tol, (name, err)


@pytest.mark.parametrize("kind", [abi.GVPM_BSDF_ROUGHPLASTIC, abi.GVPM_BSDF_PLASTIC])
def test_lambertian_limit_bre3d(kind, monkeypatch):
    """limit 1: a plain cbox whose Lambertian surface parents are re-labelled to name a plastic entry with eta = 1, Fdr = 0,
    T = 1 -- the statement with that table == the oracle on the untouched case, all 27 accumulators and the counters"""
    c = cases.make_case("cbox", 20, 16, 4000, 4.0)
    ref, rcnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    assert rcnt["diffuse_shifts"] > 300
    lam = ((c.ph.flags & 3) == abi.GVPM_PARENT_SURFACE).sum()
    c.ph = PC.relabelled(c.ph, None, lambertian_to=0)
    assert ((c.ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF).sum() == lam > 300
    PC.use_table(c, PC.limit1_table(kind))
    P.install(monkeypatch)
    acc, cnt = I.bre3d_full(c)
    _same(acc, cnt, ref, rcnt)
    # and with the unwrapped statement (or the oracle) the same photons fail: the table kind is what carries them
    O.set_bsdfs(c.bsdfs)
    _, cnt0, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    cases.use_bsdfs(c)
    assert cnt0["failed_shifts"] > rcnt["failed_shifts"] + 100


def test_conductor_limit_bre3d(monkeypatch):
    """limit 2: cbox_conductor with k = 0 == rough plastic met through its glossy component alone with T = 0 (pS = 1)"""
    c = cases.make_case("cbox_conductor", 20, 16, 20000, 4.0)
    cond, plastic, mapping = PC.limit2_tables(c.bsdfs)
    O.set_bsdfs(cond)
    ref, rcnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    assert rcnt["diffuse_shifts"] > 300
    c.ph = PC.relabelled(c.ph, mapping)
    PC.use_table(c, plastic)
    P.install(monkeypatch)
    acc, cnt = I.bre3d_full(c)
    _same(acc, cnt, ref, rcnt)


def test_conductor_limit_vpm(monkeypatch):
    c = make_vpm_case("cbox_conductor", 12, 10, 20000, 8.0, 6)
    cond, plastic, mapping = PC.limit2_tables(c.bsdfs)
    O.set_bsdfs(cond)
    ref, _, _, rcnt, _ = O.gather_vpm(c.p, c.m, c.tris, c.ph, c.rays, c.samples, 64, use_accel=True)
    assert rcnt["evaluations"] > 300
    c.ph = PC.relabelled(c.ph, mapping)
    PC.use_table(c, plastic)
    P.install(monkeypatch)
    acc, cnt, _ = I.vpm_full(c)
    _same(acc, cnt, ref, rcnt)


@pytest.mark.parametrize("kind", [abi.GVPM_BSDF_ROUGHPLASTIC, abi.GVPM_BSDF_PLASTIC])
def test_lambertian_limit_beams(kind, monkeypatch):
    c = make_beam_case("cbox", 12, 10, 1500, 4.0)
    ref, rcnt, _ = O.gather_beams(c.p, c.m, c.tris, c.beams, c.end_n, c.rays, c.r, 1, c.nb, 64)
    assert rcnt["diffuse_shifts"] > 50
    c.beams = PC.relabelled(c.beams, None, lambertian_to=0)
    assert ((c.beams.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF).sum() > 30
    PC.use_table(c, PC.limit1_table(kind))
    P.install(monkeypatch)
    acc, cnt = I.beams_full(c)
    _same(acc, cnt, ref, rcnt)


# ---- the synthetic scenes with plastic walls ------------------------------------------------------------------------------------
SCENES = ["cbox_roughplastic", "cbox_roughplastic1", "cbox_plastic"]
# the host walks with its materials' parameters in double, the table carries them as float32 (2^-24 relative; alpha enters a
# Beckmann lobe as exp(-tan^2 / alpha^2): times 2 tan^2 / alpha^2, up to ~100 where the lobe is still sampled)
PARAM_RTOL = 1e-5


def test_a_rough_plastic_scene_cannot_be_shot_before_its_slices_are_set():
    from gvpm_amd.host import SynthScene
    sc = SynthScene("cbox_roughplastic", 12, 10)
    assert [(d, round(a, 4), round(e, 4)) for _, d, a, e in sc.rtrans_materials()] == [("beckmann", 0.1, 1.5), ("ggx", 0.3, 1.5)]
    with pytest.raises(RuntimeError):
        sc.shoot_photons(1, 100)
    with pytest.raises(RuntimeError):
        sc.shoot_beams(1, 100)
    sl, fdr = PC.rtrans("beckmann", 1.5, 0.1)
    mat = sc.rtrans_materials()[0][0]
    for bad in (sl[:50], np.where(np.arange(100) == 7, 1.5, sl), np.where(np.arange(100) == 7, np.nan, sl)):
        with pytest.raises(ValueError):
            sc.set_rtrans(mat, bad, fdr)
    with pytest.raises(ValueError):
        sc.set_rtrans(0, sl, fdr)            # a Lambertian wall
    assert SynthScene("cbox_plastic", 12, 10).rtrans_materials() == [] and SynthScene("cbox", 12, 10).rtrans_materials() == []


@pytest.mark.parametrize("rot", ["", "_rot"])
@pytest.mark.parametrize("scene", SCENES)
def test_the_scenes_have_photons_behind_plastic_walls_and_a_table_for_them(scene, rot):
    c = PC.make_case(scene + rot, 40, 36, 30000, 2.5)
    heads = P.heads_of(c.bsdfs)
    kinds = c.bsdfs["kind"][heads]
    gl = (c.ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    idx = c.ph.parent_g[gl].astype(np.int64)
    assert gl.sum() >= 1000 and heads[idx].all() and set(np.unique(idx)) == set(np.flatnonzero(heads))
    assert (((c.ph.flags[gl] >> 2) & 7) == 1).all()              # diffuse reconnections
    lum = lambda v: v @ np.array([0.212671, 0.715160, 0.072169])
    for h in np.flatnonzero(heads):
        kd = c.ph.parent_scat[gl][idx == h][0]
        w = float(c.bsdfs["specular_sampling_weight"][h])
        assert 0 < w < 1 and np.isclose(w, lum(c.bsdfs["specular"][h]) / (lum(kd) + lum(c.bsdfs["specular"][h])), rtol=1e-6)
    ctype = c.ph.flags[gl] >> 16
    if scene == "cbox_roughplastic":
        assert c.bsdfs.size == 2 * PC.E and list(kinds) == [abi.GVPM_BSDF_ROUGHPLASTIC] * 2 and list(c.bsdfs["k"][heads, 0]) == [0, 0]
        assert list(c.bsdfs["distribution"][heads]) == [abi.GVPM_MICROFACET_BECKMANN, abi.GVPM_MICROFACET_GGX]
        assert np.allclose(c.bsdfs["exponent"][heads], [0.1, 0.3]) and set(np.unique(ctype)) == {0x2, 0x8}
        for h, (d, a) in zip((0, PC.E), (("beckmann", 0.1), ("ggx", 0.3))):
            sl, fdr = PC.rtrans(d, 1.5, a)
            assert np.array_equal(abi.rtrans_of(c.bsdfs, h), sl) and c.bsdfs["eta"][h, 1] == np.float32(fdr) and c.bsdfs["eta"][h, 0] == 1.5
    elif scene == "cbox_roughplastic1":
        # below alpha 0.05 a head per component met: glossy alone (EGlossyReflection), diffuse alone (EDiffuseReflection)
        assert c.bsdfs.size == 4 * PC.E and list(c.bsdfs["k"][heads, 0]) == [1, 2, 1, 2] and (c.bsdfs["exponent"][heads] < 0.05).all()
        comp = c.bsdfs["k"][idx, 0]
        assert (ctype[comp == 1] == 0x8).all() and (ctype[comp == 2] == 0x2).all()
    else:
        assert c.bsdfs.size == 2 and list(kinds) == [abi.GVPM_BSDF_PLASTIC] * 2 and list(c.bsdfs["k"][:, 0]) == [2, 2]
        assert (ctype == 0x2).all() and np.allclose(c.bsdfs["eta"][:, 1], PC.smooth_fdr_int(1.5), rtol=1e-6)
        # its Dirac bounces are specular vertices, as a mirror's: a surface parent whose component is not the diffuse one,
        # and a photon behind it does not reconnect there (shift type 0, or 3: a manifold shift further up the path)
        dirac = ((c.ph.flags & 3) == abi.GVPM_PARENT_SURFACE) & ((c.ph.flags >> 16) == 0x8)
        assert dirac.sum() > 50 and np.isin((c.ph.flags[dirac] >> 2) & 7, (0, 3)).all()


@pytest.mark.parametrize("scene", SCENES)
def test_the_hosts_plastic_bounce_is_weight_times_pdf_equals_eval(scene):
    """as for Phong and the conductor (test_glossy_parents.py): flux = prefix * (f cos / pdf) * rr * (Tr / edgePdf) and pdf in solid
    angle = the stored area pdf * len^2, against the numpy statement -- per kind and, for cbox_roughplastic1, per component
    (weight = eval_c / (pdf_c pdfComponent), pdf = pdf_c pdfComponent)"""
    c = PC.make_case(scene, 20, 16, 20000, 4.0)
    all_gl = np.flatnonzero((c.ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF)
    for h in np.flatnonzero(P.heads_of(c.bsdfs)):
        gl = all_gl[c.ph.parent_g[all_gl] == h][:400]
        assert gl.size >= 10, (h, gl.size)
        d = c.ph.pos[gl].astype(np.float64) - c.ph.parent_pos[gl]
        ln = np.linalg.norm(d, axis=1)
        wo = d / ln[:, None]
        f, pdf, known = P.phong_world_with_plastics(c.ph.parent_scat[gl].astype(np.float64), c.ph.parent_g[gl].astype(np.int64),
                                                    c.ph.parent_n[gl].astype(np.float64), c.ph.parent_wi[gl].astype(np.float64), wo)
        assert known.all() and (pdf > 0).all()
        assert np.allclose(pdf, c.ph.parent_pdf[gl] * ln * ln, rtol=2e-4), h
        tr = np.exp(-float(c.m.sigma_t[0]) * ln)
        want = c.ph.prefix_w[gl] * (f / pdf[:, None]) * c.ph.parent_rr[gl][:, None] * (tr / c.ph.edge_pdf[gl])[:, None]
        assert np.allclose(c.ph.flux[gl], want, rtol=4e-4), h


def _chi_square(sample, pdf_of, rng, n_wi, n_samples):
    """the protocol of test_glossy_parents.py (src/tests/test_chisquare.cpp): 10 x 20 (theta, phi) bins, the pdf integrated over
    the bins on a 16 x 16 sub-grid, bins with an expected frequency below 5 pooled, significance 0.01 with the Sidak correction"""
    from scipy import stats
    theta_bins, phi_bins, sub = 10, 20, 16
    alpha = 1.0 - (1.0 - 0.01) ** (1.0 / n_wi)
    th = (np.arange(theta_bins * sub) + 0.5) * (np.pi / (theta_bins * sub))
    phs = (np.arange(phi_bins * sub) + 0.5) * (2 * np.pi / (phi_bins * sub))
    T, Pm = np.meshgrid(th, phs, indexing="ij")
    dirs = np.stack([np.sin(T) * np.cos(Pm), np.sin(T) * np.sin(Pm), np.cos(T)], -1).reshape(-1, 3)
    cell = np.sin(T) * (np.pi / (theta_bins * sub)) * (2 * np.pi / (phi_bins * sub))
    for _ in range(n_wi):
        z = 0.1 + 0.9 * rng.random()
        ph = 2 * np.pi * rng.random()
        wi = np.array([np.sqrt(1 - z * z) * np.cos(ph), np.sqrt(1 - z * z) * np.sin(ph), z])
        wos, lost = sample(wi, n_samples)
        theta = np.arccos(np.clip(wos[:, 2], -1, 1))
        phi = np.arctan2(wos[:, 1], wos[:, 0]) % (2 * np.pi)
        obs, _, _ = np.histogram2d(theta, phi, bins=[theta_bins, phi_bins], range=[[0, np.pi], [0, 2 * np.pi]])
        pdf = pdf_of(wi, dirs).reshape(theta_bins * sub, phi_bins * sub)
        exp_ = (pdf * cell).reshape(theta_bins, sub, phi_bins, sub).sum((1, 3)) * (len(wos) + lost)
        assert abs(exp_.sum() - len(wos)) < 5 * np.sqrt(n_samples) + 0.01 * n_samples
        o, e = obs.ravel(), exp_.ravel()
        order = np.argsort(e)
        o, e = o[order], e[order]
        k = int(np.searchsorted(np.cumsum(e), 5.0)) + 1
        o = np.concatenate([[o[:k].sum()], o[k:]])
        e = np.concatenate([[e[:k].sum()], e[k:]])
        chi2 = ((o - e) ** 2 / e).sum()
        pval = 1 - stats.chi2.cdf(chi2, df=e.size - 1)
        assert pval > alpha, (wi, chi2, pval)


@pytest.mark.parametrize("wall", [0, 1])   # Beckmann alpha 0.1, GGX alpha 0.3
def test_rough_plastic_sampling_matches_its_pdf_chi_square(wall):
    """both components in play (alpha >= 0.05): the host's bounce against the numpy pdf; and the weight it returns IS eval / pdf"""
    sc = PC.scene("cbox_roughplastic", 8, 8)
    table = sc.bsdfs()
    mat = sc.rtrans_materials()[wall][0]
    head = wall * PC.E
    n = np.array([0.0, 0.0, 1.0])
    kd = np.array([[0.7, 0.7, 0.7], [0.6, 0.7, 0.9]])[wall]
    rng = np.random.default_rng(31 + wall)

    def sample(wi, count):
        res = [sc.sample_plastic(mat, n, wi, *rng.random(2)) for _ in range(count)]
        ok = [r for r in res if r is not None]
        for wo, weight, pdf, comp in ok[:50]:
            f, p, _ = P.plastic_world(table, kd[None, :], np.array([head]), n[None, :], wi[None, :], wo[None, :])
            assert comp == -1 and abs(p[0] - pdf) < PARAM_RTOL * pdf and np.allclose(f[0] / p[0], weight, rtol=PARAM_RTOL)
        return np.array([r[0] for r in ok]), len(res) - len(ok)

    def pdf_of(wi, dirs):
        return P.plastic_world(table, np.broadcast_to(kd, dirs.shape), np.full(len(dirs), head), np.broadcast_to(n, dirs.shape),
                               np.broadcast_to(wi, dirs.shape), dirs)[1]

    _chi_square(sample, pdf_of, rng, 6, 30000)


@pytest.mark.parametrize("scene,wall", [("cbox_roughplastic1", 0), ("cbox_roughplastic1", 1), ("cbox_plastic", 0)])
def test_one_component_sampling_chi_square_and_the_rescaling_as_written(scene, wall):
    """One component per bounce (alpha < 0.05, and the smooth plastic always).  The DIFFUSE component's sampler matches its
    pdf (the entry's pdf carries pdfComponent = 1 - pS: the sampler's density is the entry's pdf over it).  The GLOSSY
    component's does not, and provably so: RoughPlastic::sampleComponent rescales the sample it has just compared with pS by
    MULTIPLYING it (roughplastic.cpp:555-558, `sample.y *= probSpecular`), so the azimuth of the half vector, 2 pi sample.y,
    only covers [0, 2 pi pS^2) while the pdf is that of the full lobe.  That is the reference's behaviour and the host walk
    keeps it as written; weight * pdf == eval still holds for every sample (the reconnection only needs that), so the finding
    is pinned here instead of a chi-square of that component."""
    sc = PC.scene(scene, 8, 8)
    table = sc.bsdfs()
    heads = np.flatnonzero(P.heads_of(table))
    rough = scene != "cbox_plastic"
    mat = PC.plastic_materials(sc)[wall]
    h_spec, h_diff = (heads[2 * wall], heads[2 * wall + 1]) if rough else (None, heads[wall])
    n = np.array([0.0, 0.0, 1.0])
    kd = np.array([[0.7, 0.7, 0.7], [0.6, 0.7, 0.9]])[wall]
    rng = np.random.default_rng(41 + wall)
    seen = {0: 0, 1: 0}

    def sample(wi, count):
        res = [sc.sample_plastic(mat, n, wi, *rng.random(2)) for _ in range(count)]
        diff = [r for r in res if r is not None and r[3] == 1]
        spec = [r for r in res if r is not None and r[3] == 0]
        seen[0] += len(spec)
        seen[1] += len(diff)
        for wo, weight, pdf, comp in diff[:50]:
            f, p, _ = P.plastic_world(table, kd[None, :], np.array([h_diff]), n[None, :], wi[None, :], wo[None, :])
            assert abs(p[0] - pdf) < PARAM_RTOL * pdf and np.allclose(f[0] / p[0], weight, rtol=PARAM_RTOL)
        if rough and spec:
            b = table[h_spec]
            Ti = P.transmittance(abi.rtrans_of(table, h_spec), wi[2])
            pS = float(P.prob_specular(Ti, float(b["specular_sampling_weight"])))
            for wo, weight, pdf, comp in spec[:50]:
                f, p, _ = P.plastic_world(table, kd[None, :], np.array([h_spec]), n[None, :], wi[None, :], wo[None, :])
                assert abs(p[0] - pdf) < PARAM_RTOL * pdf and np.allclose(f[0] / p[0], weight, rtol=PARAM_RTOL)
            # the half vector's azimuth about the normal stays inside [0, 2 pi pS^2)
            hv = np.array([r[0] for r in spec]) + wi
            az = np.arctan2(hv[:, 1], hv[:, 0]) % (2 * np.pi)
            assert az.max() <= 2 * np.pi * pS * pS + 1e-9 < 2 * np.pi
        # (the diffuse histogram is conditional on the component: a sample that picked the other one counts as lost)
        return np.array([r[0] for r in diff]), len(res) - len(diff)

    def pdf_of(wi, dirs):
        return P.plastic_world(table, np.broadcast_to(kd, dirs.shape), np.full(len(dirs), h_diff), np.broadcast_to(n, dirs.shape),
                               np.broadcast_to(wi, dirs.shape), dirs)[1]

    _chi_square(sample, pdf_of, rng, 6, 30000)
    assert seen[0] > 1000 and seen[1] > 1000


@pytest.mark.parametrize("scene", SCENES)
def test_the_statement_counts_reconnections_the_oracle_fails(scene, monkeypatch):
    """the wrapped numpy statement on a plastic scene against the frozen oracle, which ignores the kinds it does not know: same
    evaluations, and the oracle's failed shifts through plastic parents are the statement's reconnections"""
    c = PC.make_case(scene, 20, 16, 6000, 4.0)
    _, ocnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    P.install(monkeypatch)
    acc, cnt = I.bre3d_full(c)
    assert cnt["evaluations"] == ocnt["evaluations"] and cnt["null_shifts"] == ocnt["null_shifts"]
    assert cnt["diffuse_shifts"] - ocnt["diffuse_shifts"] == ocnt["failed_shifts"] - cnt["failed_shifts"] > 100
