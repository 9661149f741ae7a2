"""Two-component mixture parents (GVPM_BSDF_MIXTURE; include/gvpm_hip.h), CPU side: the constants and the layout, the numpy statement of
tests/indep_mixture.py at degenerate weights against the sibling statements, the host's sampler (synth_core.h sampleMixture) against
the statement's pdf (chi-square) and its weight x pdf = eval, for both components together and for each selected component, and what
the three synthetic scenes flatten to."""
import os
import re

import numpy as np
import pytest

import aniso_cases as AC
import cases
import indep_aniso as A
import indep_mixture as M
import indep_phong_dist as PD
import indep_statements as I
import mixture_cases as C
from gvpm_amd import abi
from test_plastic_parents import _chi_square, _dirs

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
INNER = PD.phong_world_with_phong_dist
UP = np.array([0.0, 1.0, 0.0])         # the floor's normal
BACK = np.array([0.0, 0.0, 1.0])       # the back wall's


# ---- the constants and the layout ------------------------------------------------------------------------------------------------
def test_abi_constants_and_layout():
    header = open(os.path.join(ROOT, "include", "gvpm_hip.h")).read()
    assert re.search(r"GVPM_BSDF_ROUGHDIELECTRIC = 9, GVPM_BSDF_MIXTURE = 10 \};", header)
    assert re.search(r"#define GVPM_MIXTURE_CHILD_DIFFUSE \(-1\)", header) and re.search(r"#define GVPM_MIXTURE_CHILD_ABSENT \(-2\)", header)
    assert (abi.GVPM_BSDF_MIXTURE, abi.GVPM_MIXTURE_CHILD_DIFFUSE, abi.GVPM_MIXTURE_CHILD_ABSENT) == (10, -1, -2)
    assert abi.BSDF_DTYPE.itemsize == 64 and abi.bsdf_tail_entries(abi.GVPM_BSDF_MIXTURE) == 0
    assert int(re.search(r"#define GVPM_ABI_VERSION (\d+)", header).group(1)) == abi.GVPM_ABI_VERSION
    e = abi.mixture_entry((0.6, 0.4), (abi.GVPM_MIXTURE_CHILD_DIFFUSE, 5), 2)
    words, ints = e.view(np.float32).reshape(16), e.view(np.int32).reshape(16)
    # row 0 {kind, w_0, w_1, 0}, row 1 {0, 0, component + 1, 0}, row 2 {child 0, child 1, 0, 0}; every other word +0
    assert ints[0] == 10 and ints[6] == 2 and np.allclose(words[1:3], [0.6, 0.4]) and list(words[8:10]) == [-1.0, 5.0]
    rest = np.delete(ints, [0, 1, 2, 6, 8, 9])
    assert not rest.any()
    table = np.concatenate([C.conductor_entry(0.3), e, C.aniso_entry(0.1, 0.2, AC.SKEW[0])])
    assert list(abi.bsdf_heads(table)) == [True, True, True, False] and list(M.is_mixture(table)) == [False, True, False, False]


# ---- the statement at degenerate weights is the sibling statements ------------------------------------------------------------------
def _rows(rng, k, n):
    u, v, _ = A.frame(np.array([[0.3, 0.5, 0.2]]), n[None, :])
    world = lambda d: d[:, 0:1] * u + d[:, 1:2] * v + d[:, 2:3] * n
    return np.broadcast_to(n, (k, 3)), world(_dirs(rng, k)), world(_dirs(rng, k)), rng.random((k, 3))


def test_degenerate_weights_are_the_sibling_statements(monkeypatch):
    rng = np.random.default_rng(5)
    cond, ani = C.conductor_entry(0.3, C.CU), C.aniso_entry(0.12, 0.45, AC.SKEW[1], C.AL, C.GGX)
    table = np.concatenate([cond, ani,                                          # heads 0, 1 (+ frame 2)
                            C.mixture((1.0, 0.0), (0, C.DIFFUSE)),               # 3: the plain conductor
                            C.mixture((0.0, 1.0), (0, C.DIFFUSE)),               # 4: the Lambertian
                            C.mixture((0.6, 0.4), (1, C.DIFFUSE), 1),            # 5: child 0 alone
                            C.mixture((0.6, 0.4), (1, C.DIFFUSE), 2),            # 6: child 1 alone
                            C.mixture((0.9, 0.3), (0, 1)),                       # 7: two metals, weights summing above 1
                            C.mixture((0.7, 0.3), (C.ABSENT, 1), 2)])            # 8: beside an absent child
    monkeypatch.setattr(I, "BSDFS", table)
    k = 400
    n, wi, wo, kd = _rows(rng, k, BACK)
    at = lambda h: M.phong_world_with_mixture(kd, np.full(k, h), n, wi, wo)
    f0, p0, k0 = INNER(kd, np.full(k, 0), n, wi, wo)
    f1, p1, k1 = INNER(kd, np.full(k, 1), n, wi, wo)
    co = (n * wo).sum(-1)
    lam_f, lam_p = kd / np.pi * co[:, None], co / np.pi
    assert k0.all() and k1.all() and (p0 > 0).sum() > 300 and (p1 > 0).sum() > 100
    f, p, kn = at(3)
    assert kn.all() and np.array_equal(f, f0) and np.array_equal(p, p0)
    f, p, kn = at(4)
    assert kn.all() and np.allclose(f, lam_f, rtol=1e-15) and np.allclose(p, lam_p, rtol=1e-15)
    w = np.float32([0.6, 0.4]).astype(np.float64)
    f, p, kn = at(5)
    assert kn.all() and np.allclose(f, w[0] * f1, rtol=1e-15) and np.allclose(p, w[0] / w.sum() * p1, rtol=1e-15)
    f, p, kn = at(6)
    assert kn.all() and np.allclose(f, w[1] * lam_f, rtol=1e-15) and np.allclose(p, w[1] / w.sum() * lam_p, rtol=1e-15)
    w = np.float32([0.9, 0.3]).astype(np.float64)
    f, p, kn = at(7)
    assert kn.all() and np.allclose(f, w[0] * f0 + w[1] * f1, rtol=1e-14) and np.allclose(p, (w[0] * p0 + w[1] * p1) / w.sum(), rtol=1e-14)
    f, p, kn = at(8)
    w = np.float32([0.7, 0.3]).astype(np.float64)
    assert kn.all() and np.allclose(f, w[1] * f1, rtol=1e-15) and np.allclose(p, w[1] * p1, rtol=1e-15)
    # light from behind: undefined, a failed shift; every other entry is handed on untouched
    fb, pb, kb = M.phong_world_with_mixture(kd, np.full(k, 7), n, -wi, wo)
    assert not kb.any() and not fb.any() and not pb.any()
    for h in (0, 1, 2, 9, -1):
        a, b = M.phong_world_with_mixture(kd, np.full(k, h), n, wi, wo), INNER(kd, np.full(k, h), n, wi, wo)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_an_undefined_child_leaves_the_row_undefined_and_a_zero_child_does_not(monkeypatch):
    """an anisotropic child whose tangent is parallel to the normal spans no frame: the whole row is undefined; a conductor child with
    D = 0 (a half vector far outside a lobe of alpha 0.001) contributes zero and the Lambertian child still counts"""
    table = np.concatenate([C.aniso_entry(0.12, 0.45, BACK), C.conductor_entry(0.001), C.mixture((0.5, 0.5), (0, C.DIFFUSE)),
                            C.mixture((0.5, 0.5), (2, C.DIFFUSE))])
    monkeypatch.setattr(I, "BSDFS", table)
    rng = np.random.default_rng(6)
    n, wi, wo, kd = _rows(rng, 50, BACK)
    f, p, kn = M.phong_world_with_mixture(kd, np.full(50, 3), n, wi, wo)
    assert not kn.any() and not f.any()
    f, p, kn = M.phong_world_with_mixture(kd, np.full(50, 4), n, wi, wo)
    co = (n * wo).sum(-1)
    assert kn.all() and np.allclose(p, 0.5 * co / np.pi, rtol=1e-15) and np.allclose(f, 0.5 * kd / np.pi * co[:, None], rtol=1e-15)


# ---- the host's sampler ------------------------------------------------------------------------------------------------------------
def _host_statement(scene, wall, n, wi, wo, component=-1):
    """(f, pdf, defined) of the scene's wall with the host's double-precision parameters; component: the child selected (-1: both)"""
    sc_name = scene.replace("_rot", "")
    table = _scene(scene).bsdfs()
    children, weights, first = _scene(scene).mixture(C.MATS[sc_name][wall])
    head = first + max(component, 0)
    assert table["distribution"][head] == component + 1
    k = len(wo)
    one = lambda x: np.broadcast_to(np.asarray(x, np.float64), (k, 3))
    return M.mixture_world(table, one(C.KD.get(wall, 0.0)), np.full(k, head), one(n), one(wi), wo, C.host_children(sc_name), weights=weights,
                           child_kinds=False)


_SCENES = {}


def _scene(name):
    from gvpm_amd.host import SynthScene
    if name not in _SCENES:
        _SCENES[name] = SynthScene(name, 8, 8)
    return _SCENES[name]


CASES = [("cbox_mixture", "floor", -1), ("cbox_mixture", "back", -1), ("cbox_mixture1", "floor", 0), ("cbox_mixture1", "floor", 1)]


@pytest.mark.parametrize("scene,wall,component", CASES)
def test_sampling_matches_the_statements_pdf_chi_square(scene, wall, component):
    """the host's bounce against the statement's pdf, 10 x 20 bins at significance 0.01.  Both components (cbox_mixture's floor, a
    Lambertian and a conductor; its back wall, two conductors, one anisotropic): the density is p_0 pdf_0 + p_1 pdf_1.  One component
    (cbox_mixture1's floor): the bounces that selected child c are distributed as pdf_c and arrive with probability p_c -- the others
    count as lost, and the statement's pdf of the component entry, pdf_c p_c, is the density over all bounces."""
    sc = _scene(scene)
    mat = C.MATS[scene][wall]
    n = UP if wall == "floor" else BACK
    rng = np.random.default_rng(17 + 3 * CASES.index((scene, wall, component)))
    u, v, _ = A.frame(np.array([[0.3, 0.5, 0.2]]), n[None, :])
    to_world = lambda d: d[..., 0:1] * u + d[..., 1:2] * v + d[..., 2:3] * n
    to_local = lambda d: np.stack([(d * u).sum(-1), (d * v).sum(-1), (d * n).sum(-1)], -1)

    def sample(wi_l, count):
        wi = to_world(wi_l)[0]
        res = [sc.sample_mixture(mat, n, wi, *rng.random(2)) for _ in range(count)]
        ok = [r for r in res if r is not None and r[3] == component]
        assert all(r[3] in ((-1,) if component == -1 else (0, 1)) for r in res if r is not None)
        return to_local(np.array([r[0] for r in ok])), len(res) - len(ok)

    def pdf_of(wi_l, dirs_l):
        return _host_statement(scene, wall, n, to_world(wi_l)[0], to_world(dirs_l), component)[1]

    if component == 1:
        _chi_square_fine(sample, pdf_of, rng, 4, 30000, 40, 80, 16)
    else:
        _chi_square(sample, pdf_of, rng, 6, 30000)


def _chi_square_fine(sample, pdf_of, rng, n_wi, n_samples, theta_bins, phi_bins, sub):
    """test_plastic_parents._chi_square's protocol with bins and quadrature four times finer each way (40 x 80 bins of 4.5 degrees, the
    pdf on a 16 x 16 grid in each): the conductor child of cbox_mixture1's floor has alpha 0.03, its lobe is a few degrees wide -- one
    or two of the 18-degree bins, which leaves the statistic no degree of freedom -- and at grazing incidence narrower than the coarse
    grid's 1.1 degrees (measured at cos_i = 0.15: that grid integrates the component's density to 0.219, this one to 0.29994, of
    p_1 = 0.3)"""
    from scipy import stats
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
        assert e.size >= 4, e.size
        chi2 = ((o - e) ** 2 / e).sum()
        pval = 1 - stats.chi2.cdf(chi2, df=e.size - 1)
        assert pval > alpha, (wi, chi2, pval)


@pytest.mark.parametrize("scene,wall", [("cbox_mixture", "floor"), ("cbox_mixture", "left"), ("cbox_mixture", "back"), ("cbox_mixture1", "floor"),
                                        ("cbox_mixture1", "back")])
def test_weight_times_pdf_is_the_statements_eval_to_1e9(scene, wall):
    """weight x pdf = eval and pdf = the statement's (pdfComponent in both), to 1e-9: the host is fp64 and the statement takes the
    host's own doubles.  cbox_mixture1's floor is met through one child at a time: both are seen, with the sampled lobe's type."""
    sc = _scene(scene)
    mat = C.MATS[scene][wall]
    n = {"floor": UP, "back": BACK, "left": np.array([1.0, 0.0, 0.0])}[wall]
    rng = np.random.default_rng(29)
    u, v, _ = A.frame(np.array([[0.3, 0.5, 0.2]]), n[None, :])
    wis = _dirs(rng, 700)
    wis = wis[:, 0:1] * u + wis[:, 1:2] * v + wis[:, 2:3] * n
    seen = {-1: 0, 0: 0, 1: 0}
    one_child = scene == "cbox_mixture1" and wall == "floor"
    for wi in wis:
        r = sc.sample_mixture(mat, n, wi, *rng.random(2))
        if r is None:
            continue
        wo, weight, pdf, comp, typ = r
        assert (comp in (0, 1)) == one_child
        f, p, d = _host_statement(scene, wall, n, wi, wo[None, :], comp)
        assert d[0] and abs(p[0] - pdf) <= 1e-9 * pdf, (comp, p, pdf)
        assert np.allclose(weight * pdf, f[0], rtol=1e-9, atol=1e-300), (comp, weight * pdf, f[0])
        if one_child:
            assert typ == (abi.GVPM_BSDF_DIFFUSE_REFLECTION if comp == 0 else 0x8)
        seen[comp] += 1
    if one_child:
        # p_0 = 0.7, p_1 = 0.3 of the bounces; the conductor at alpha 0.03 loses the directions it reflects below the floor
        assert seen[0] > 350 and seen[1] > 120 and 0.6 < seen[0] / (seen[0] + seen[1]) < 0.8, seen
    else:
        assert seen[-1] > 400, seen


def test_the_sampler_draws_no_number_of_its_own():
    """sampleReuse re-stretches the vertex's two numbers: the same (u1, u2) give the same bounce, and the walk's streams are those of
    every other material (the existing goldens are the check for the other scenes)"""
    sc = _scene("cbox_mixture")
    wi = np.array([0.3, 0.8, 0.1]) / np.linalg.norm([0.3, 0.8, 0.1])
    a, b = sc.sample_mixture(7, UP, wi, 0.31, 0.77), sc.sample_mixture(7, UP, wi, 0.31, 0.77)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2]
    with pytest.raises(ValueError):
        sc.sample_mixture(4, UP, wi, 0.5, 0.5)          # a child, not a mixture
    # u1 below p_0 = 0.6 samples the Lambertian child, above it the conductor (the sampled lobe's type says which)
    assert sc.sample_mixture(7, UP, wi, 0.59, 0.5)[4] == abi.GVPM_BSDF_DIFFUSE_REFLECTION
    assert sc.sample_mixture(7, UP, wi, 0.61, 0.5)[4] == 0x8


# ---- flattening -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", C.SCENES)
def test_the_scenes_tables_and_records(scene):
    """every GVPM_PARENT_SURFACE_BSDF record names a mixture head, with shift type 1 (a mixture vertex classifies as diffuse), the
    Lambertian child's reflectance in parent_scat (zero where there is none) and the area pdf with pdfComponent in parent_pdf"""
    c = cases.make_case(scene, 20, 16, 20000, 4.0)
    t = c.bsdfs
    heads, mix = abi.bsdf_heads(t), M.is_mixture(t)
    one = scene == "cbox_mixture1"
    assert list(t["kind"][heads]) == [2, 2, 8] + [10] * (3 if one else 4) and t.size == (7 if one else 8)
    assert np.allclose(t["exponent"][:3], [0.03 if one else 0.3, 0.2, 0.12]) and np.isclose(abi.frame_of(t, 2)[1], 0.45)
    back = t[-1]
    assert list(back["eta"][:2]) == [1.0, 2.0] and list(back["specular"][:2]) == [0.5, 0.5] and back["distribution"] == 0
    if one:
        assert list(t["distribution"][4:6]) == [1, 2] and (t["eta"][4:6, :2] == [-1.0, 0.0]).all()
        assert np.allclose(t["specular"][4:6, :2], [0.7, 0.3])
    else:
        assert not t["distribution"][4:7].any() and (t["eta"][4:7, :2] == [-1.0, 0.0]).all() and np.allclose(t["specular"][4:7, :2], [0.6, 0.4])
    for records in (c.ph, c.sc.shoot_beams(1, 3000)[0]):
        gl = (records.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
        idx = records.parent_g[gl].astype(np.int64)
        assert gl.sum() >= 200 and mix[idx].all() and set(np.unique(idx)) == set(np.flatnonzero(mix))
        assert (((records.flags[gl] >> 2) & 7) == 1).all()
        scat = records.parent_scat[gl]
        lam = (t["eta"][idx, :2] == -1.0).any(-1)
        assert not scat[~lam].any() and (scat[lam].max(-1) > 0).all()
        if not one:
            for h, wall in ((4, "floor"), (5, "left"), (6, "right")):
                assert np.allclose(scat[idx == h], C.KD[wall], rtol=1e-6)
    cases.use_bsdfs(cases.make_case("cbox", 8, 8, 10, 4.0))


def test_parent_pdf_carries_the_component_probability():
    """cbox_mixture1's floor records name one of its two component heads, and parent_pdf is the child's own area pdf times p_c: the
    statement of the component entry (pdf_c p_c towards the photon, times cos / l^2) reproduces it"""
    c = cases.make_case("cbox_mixture1", 20, 16, 20000, 4.0)
    ph, t = c.ph, c.bsdfs
    gl = (ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    for head, comp in ((4, 0), (5, 1)):
        r = np.flatnonzero(gl & (ph.parent_g == head))
        assert r.size > 50, (head, r.size)
        d = ph.pos[r].astype(np.float64) - ph.parent_pos[r]
        l2 = (d * d).sum(-1)
        wo = d / np.sqrt(l2)[:, None]
        n, wi = ph.parent_n[r].astype(np.float64), ph.parent_wi[r].astype(np.float64)
        _, pdf, ok = M.mixture_world(t, ph.parent_scat[r].astype(np.float64), np.full(r.size, head), n, wi, wo, C.host_children("cbox_mixture1"),
                                     weights=(0.7, 0.3), child_kinds=False)
        # (the photon is a medium vertex: no cosine at its end; fp32 records: 1e-4 at a lobe of alpha 0.03, whose pdf moves by 1 / alpha^2
        # per unit of the direction's rounding)
        assert ok.all() and np.allclose(pdf / l2, ph.parent_pdf[r], rtol=2e-3 if comp else 1e-5), (head, np.abs(pdf / l2 / ph.parent_pdf[r] - 1).max())
    cases.use_bsdfs(cases.make_case("cbox", 8, 8, 10, 4.0))


def test_the_existing_scenes_keep_their_streams():
    """the mixture draws at mixture vertices only: a Lambertian and a conductor scene shoot what they shot (pinned by the suite's
    goldens); here, that the new material did not change the table of a scene that has none"""
    assert cases.make_case("cbox_conductor", 8, 8, 100, 4.0).bsdfs.size == 2 and cases.make_case("cbox", 8, 8, 10, 4.0).bsdfs.size == 0
