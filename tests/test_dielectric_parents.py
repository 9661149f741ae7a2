"""Rough-dielectric surface parents (GVPM_BSDF_ROUGHDIELECTRIC; include/gvpm_hip.h), CPU side: the host's sampler against the
numpy statement of tests/indep_dielectric.py (chi-square against its pdf, weight x pdf against its eval), the statement against
itself in the other frame and against the rough conductor it becomes, the flattened records of the two scenes, and the packed
and linked round trips."""
import numpy as np
import pytest

import cases
import dielectric_cases as DC
import indep_dielectric as D
import indep_statements as I
from gvpm_amd import abi, hip
from gvpm_amd.host import SynthScene

GGX, BECKMANN = abi.GVPM_MICROFACET_GGX, abi.GVPM_MICROFACET_BECKMANN
SCENE_OF = {BECKMANN: "cbox_roughglass", GGX: "cbox_roughglass_ggx"}
N = np.array([0.0, 0.0, 1.0])


def test_abi():
    assert abi.GVPM_BSDF_ROUGHDIELECTRIC == 9 and abi.bsdf_tail_entries(9) == 0
    t = DC.surface_table(1.5, 0.25, DC.KS, DC.KT)
    assert list(t["kind"]) == [9, 9] and np.allclose(t["eta"][:, 0], (1.5, 1 / 1.5)) and not t["eta"][:, 1:].any()
    assert not t["specular_sampling_weight"].any() and not t["reserved"].any() and abi.bsdf_heads(t).all()


def _statement(ggx, wi, wo):
    """eval and pdf of the scenes' pane (front normal N) in fp64 parameters, the reference's frame"""
    k = len(wo)
    one = np.ones(k)
    return D.reference_rows(np.array(DC.KS), np.array(DC.KT), DC.ALPHA * one, DC.ETA * one, np.full(k, bool(ggx)), np.zeros(k, bool),
                            np.broadcast_to(N, (k, 3)), np.broadcast_to(wi, (k, 3)), wo, count=False)


# ---- (a) the sampler against the statement's pdf ---------------------------------------------------------------------------------
@pytest.mark.parametrize("z", [0.9, 0.6, 0.25])
@pytest.mark.parametrize("side", [1, -1])
@pytest.mark.parametrize("distribution", [BECKMANN, GGX])
def test_dielectric_sampling_matches_its_pdf_chi_square(distribution, side, z):
    """the harness of test_glossy_parents (src/tests/test_chisquare.cpp, test01_BSDF) over the WHOLE sphere: 10 x 20 (theta, phi)
    bins, bins with an expected frequency below 5 pooled, significance 0.01.  wi outside (side 1) and inside; cos 0.6 lies
    beyond the critical angle from inside (sin = 0.8 > 1 / 1.5): only tilted facets transmit there."""
    from scipy import stats
    sc = SynthScene(SCENE_OF[distribution], 8, 8)
    mat = DC.dielectric_material(sc)
    rng = np.random.default_rng(23)
    phi0 = 2 * np.pi * rng.random()
    wi = np.array([np.sqrt(1 - z * z) * np.cos(phi0), np.sqrt(1 - z * z) * np.sin(phi0), side * z])
    theta_bins, phi_bins, n_samples = 10, 20, 30000
    res = [sc.sample_dielectric(mat, N, wi, *rng.random(3)) for _ in range(n_samples)]
    lost = sum(r is None for r in res)
    wo = np.array([r[0] for r in res if r is not None])
    types = np.array([r[3] for r in res if r is not None])
    assert ((types == 0x8) == (wo[:, 2] * wi[2] > 0)).all() and set(types) <= {0x8, 0x10}
    if side == -1 and z == 0.6:
        assert (types == 0x8).sum() > 0.5 * len(types)      # (total internal reflection off most facets; GGX's tails transmit more)
    theta = np.arccos(np.clip(wo[:, 2], -1, 1))
    phi = np.arctan2(wo[:, 1], wo[:, 0]) % (2 * np.pi)
    obs, _, _ = np.histogram2d(theta, phi, bins=[theta_bins, phi_bins], range=[[0, np.pi], [0, 2 * np.pi]])
    sub = 16
    th = (np.arange(theta_bins * sub) + 0.5) * (np.pi / (theta_bins * sub))
    phs = (np.arange(phi_bins * sub) + 0.5) * (2 * np.pi / (phi_bins * sub))
    T, Pm = np.meshgrid(th, phs, indexing="ij")
    dirs = np.stack([np.sin(T) * np.cos(Pm), np.sin(T) * np.sin(Pm), np.cos(T)], -1).reshape(-1, 3)
    f, pdf, _ = _statement(distribution == GGX, wi, dirs)
    # RoughDielectric::pdf does not look at G: it is positive on directions no facet sends wi to (wi . H and wo . H of one sign
    # behind the generalised half vector; eval = 0 there, 2 % of the sphere's mass at cos 0.9 from inside) and on facets seen
    # from behind.  The sampler never lands there -- its samples with G = 0 carry no weight and are lost -- so the histogram is
    # held against the pdf where eval > 0, and the lost samples against the rest of the unit mass.
    dead = float((np.where((f > 0).any(1), 0.0, pdf) * (np.sin(T) * (np.pi / (theta_bins * sub)) * (2 * np.pi / (phi_bins * sub))).ravel()).sum())
    print(f"pdf mass on directions with eval = 0: {dead:.4f}, samples lost: {lost / n_samples:.4f}")
    pdf = np.where((f > 0).any(1), pdf, 0.0).reshape(theta_bins * sub, phi_bins * sub)
    cell = np.sin(T) * (np.pi / (theta_bins * sub)) * (2 * np.pi / (phi_bins * sub))
    exp_ = (pdf * cell).reshape(theta_bins, sub, phi_bins, sub).sum((1, 3)) * n_samples
    # the pdf integrates to 1 minus what the side checks lose
    assert abs(exp_.sum() - (n_samples - lost)) < 5 * np.sqrt(n_samples) + 0.01 * n_samples
    o, e = obs.ravel(), exp_.ravel()
    order = np.argsort(e)
    o, e = o[order], e[order]
    k = int(np.searchsorted(np.cumsum(e), 5.0)) + 1
    o = np.concatenate([[o[:k].sum()], o[k:]])
    e = np.concatenate([[e[:k].sum()], e[k:]])
    chi2 = ((o - e) ** 2 / e).sum()
    pval = 1 - stats.chi2.cdf(chi2, df=e.size - 1)
    assert pval > 0.01, (wi, chi2, pval)


# ---- (b) weight x pdf = eval: the second derivation of the transmission term -----------------------------------------------------
@pytest.mark.parametrize("distribution", [BECKMANN, GGX])
def test_the_hosts_weight_times_pdf_is_the_statements_eval(distribution):
    """RoughDielectric::sample's weight |D G wi.m / (pdf_m cos_i)| x reflectance | transmittance contains neither eta^2 nor
    (wi.H + eta wo.H)^2 nor dwh_dwo; the statement's eval and pdf do.  10^4 sampled directions in each of the four classes
    (reflected / transmitted x wi outside / inside), every channel to 1e-9 relative; the pdf too."""
    sc = SynthScene(SCENE_OF[distribution], 8, 8)
    mat = DC.dielectric_material(sc)
    rng = np.random.default_rng(41)
    got = {(t, s): [] for t in (0x8, 0x10) for s in (1, -1)}
    while min(len(v) for v in got.values()) < 10000:
        side = 1 if rng.random() < 0.3 else -1           # (transmission from inside is the rare class)
        z = 0.05 + 0.95 * rng.random() if side == 1 else 0.6 + 0.4 * rng.random()
        ph = 2 * np.pi * rng.random()
        wi = np.array([np.sqrt(1 - z * z) * np.cos(ph), np.sqrt(1 - z * z) * np.sin(ph), side * z])
        r = sc.sample_dielectric(mat, N, wi, *rng.random(3))
        if r is not None and len(got[(r[3], side)]) < 10000:
            got[(r[3], side)].append((wi, r[0], r[1], r[2]))
    for key, rows in got.items():
        wi, wo, weight, pdf = (np.array([r[j] for r in rows]) for j in range(4))
        f, p, defined = D.reference_rows(np.array(DC.KS), np.array(DC.KT), np.full(len(rows), DC.ALPHA), np.full(len(rows), DC.ETA),
                                         np.full(len(rows), distribution == GGX), np.zeros(len(rows), bool),
                                         np.broadcast_to(N, wi.shape), wi, wo, count=False)
        assert defined.all() and (f > 0).all(), key
        assert np.abs(p / pdf - 1).max() < 1e-9, (key, np.abs(p / pdf - 1).max())
        err = np.abs(weight * pdf[:, None] / f - 1).max()
        assert err < 1e-9, (key, err)


# ---- the statement in the device's frame, and (c) the limit -------------------------------------------------------------------------
@pytest.mark.parametrize("visible", [0, 1])
@pytest.mark.parametrize("distribution", [BECKMANN, GGX])
def test_the_statement_is_the_same_in_either_frame(distribution, visible):
    """the reference's text with its signed cosines gives one value whichever way the frame normal points, as long as m_eta
    turns with it: N, m_eta and -N, 1 / m_eta.  (The device evaluates in wi's frame, the statement in the record's.)"""
    rng = np.random.default_rng(7)
    k = 4000
    v = rng.normal(size=(3, k, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    n, wi, wo = v
    args = (np.array(DC.KS), np.array(DC.KT), np.full(k, 0.2), np.full(k, bool(distribution == GGX)), np.full(k, bool(visible)))
    f1, p1, d1 = D.reference_rows(args[0], args[1], args[2], np.full(k, 1.5), args[3], args[4], n, wi, wo, count=False)
    f2, p2, d2 = D.reference_rows(args[0], args[1], args[2], np.full(k, 1 / 1.5), args[3], args[4], -n, wi, wo, count=False)
    assert (d1 == d2).all() and (f1 > 0).any(1).sum() > 1000 and ((p1 > 0) & ~(f1 > 0).any(1)).sum() >= 0
    assert np.allclose(f1, f2, rtol=1e-10, atol=0) and np.allclose(p1, p2, rtol=1e-10, atol=0)
    # both classes were met from both sides
    cls = (np.sign((n * wi).sum(1)), np.sign((n * wi).sum(1) * (n * wo).sum(1)))
    assert all(((cls[0] == a) & (cls[1] == b) & (f1 > 0).any(1)).sum() > 50 for a in (1, -1) for b in (1, -1))


@pytest.mark.parametrize("distribution", [BECKMANN, GGX])
def test_reflection_from_outside_is_the_conductor_with_k_zero(distribution):
    """(c) the limit: with k = 0 the conductor's complex Fresnel term is the dielectric's, and reflection met from outside is
    indep_statements' rough conductor with the same scalar eta -- the eval to 1e-12; the visible-normal pdfs differ by F alone"""
    rng = np.random.default_rng(19)
    k = 3000
    v = rng.normal(size=(3, k, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    n, wi, wo = v
    wi = np.where(((n * wi).sum(1) < 0)[:, None], -wi, wi)
    wo = np.where(((n * wo).sum(1) < 0)[:, None], -wo, wo)
    cond = np.zeros(1, abi.BSDF_DTYPE)
    cond["kind"], cond["specular"], cond["exponent"] = abi.GVPM_BSDF_ROUGHCONDUCTOR, (0.9, 0.8, 1.0), 0.2
    cond["distribution"], cond["sample_visible"], cond["eta"], cond["k"] = distribution, 1, 1.5, 0.0
    _, diel = DC.conductor_limit(cond)
    I.set_bsdfs(cond)
    fc, pc, known = I.phong_world(np.zeros((1, 3)), np.zeros(k, np.int64), n, wi, wo)
    fd, pd, defined = D.dielectric_world(diel, np.zeros(k, np.int64), n, wi, wo, count=False)
    I.set_bsdfs(cond[:0])
    assert known.all() and defined.all() and (fc > 0).all(1).sum() > 2000
    assert np.allclose(fd, fc, rtol=1e-12, atol=0)
    h = wi + wo
    h /= np.linalg.norm(h, axis=1, keepdims=True)
    F, _ = D.fresnel_ext((wi * h).sum(1), np.full(k, 1.5))
    assert np.allclose(pd, pc * F, rtol=1e-12, atol=0)


# ---- (d) the flattened records of the two scenes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("beams", [False, True])
@pytest.mark.parametrize("scene", DC.SCENES)
def test_the_flattened_records(scene, beams):
    """the record's normal points to the side the photon left, the entry is the one of the side the light arrived on (the pane's
    front is its upper side: entry 0 = the light came from above), the component bits are the sampled lobe's, the shift is a
    diffuse reconnection, and all four classes occur"""
    if beams:
        from test_oracle_beams import make_beam_case
        c = make_beam_case(scene, 12, 10, 3000, 5.0)
        rec = c.beams
    else:
        c = cases.make_case(scene, 20, 16, 20000, 4.0)
        rec = c.ph
    t = c.bsdfs
    assert t.size == 2 and (t["kind"] == abi.GVPM_BSDF_ROUGHDIELECTRIC).all()
    assert np.array_equal(t[:1], abi.dielectric_entry(DC.KS, DC.KT, DC.ALPHA, DC.ETA))
    assert np.array_equal(t[1:], abi.dielectric_entry(DC.KS, DC.KT, DC.ALPHA, 1.0 / DC.ETA))
    gl = (rec.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    assert gl.sum() > (300 if beams else 3000) and ((rec.flags & 3) == abi.GVPM_PARENT_SURFACE).sum() > 100
    n = rec.parent_n[gl].astype(np.float64)
    assert ((n * (rec.pos[gl].astype(np.float64) - rec.parent_pos[gl])).sum(1) > 0).all()
    assert (((rec.flags[gl] >> 2) & 7) == 1).all()
    # one plane, its front normal up in the room's frame: the records' normals are +- one vector
    front = n[np.argmax(np.abs(n @ n[0]))]
    assert np.abs(np.abs(n @ front) - 1).max() < 1e-6
    tri_n = np.cross(c.tris[1][-3], c.tris[2][-3]).astype(np.float64)     # (the pane: the quad before the light's)
    front = front * np.sign(front @ tri_n)
    assert abs(front @ tri_n / np.linalg.norm(tri_n) - 1) < 1e-6
    cos_i = (rec.parent_wi[gl].astype(np.float64) * front).sum(1)
    entry = rec.parent_g[gl].astype(np.int64)
    assert set(np.unique(entry)) == {0, 1} and ((entry == 1) == (cos_i < 0)).all()
    cls = DC.classes(rec, t)
    counts = {k: int(m.sum()) for k, m in cls.items()}
    print(scene, "beams" if beams else "photons", "records per class (reflected, from outside):", counts)
    assert all(v >= (5 if beams else 50) for v in counts.values()), counts
    if not beams:    # (beam records carry no component bits: every flattener writes EDiffuseReflection there)
        for (reflected, _), m in cls.items():
            assert (rec.flags[m] >> 16 == (0x8 if reflected else 0x10)).all()
        # a photon right behind the bounce: flux = prefix (eval / pdf) rr (Tr / edgePdf), pdf = the stored area pdf x len^2
        idx = np.flatnonzero(gl)
        d = rec.pos[idx].astype(np.float64) - rec.parent_pos[idx]
        ln = np.linalg.norm(d, axis=1)
        far = ln > 0.05                                  # (directions from fp32 positions)
        idx, ln, wo = idx[far], ln[far], (d / ln[:, None])[far]
        f, pdf, defined = D.dielectric_world(t, rec.parent_g[idx].astype(np.int64), rec.parent_n[idx].astype(np.float64),
                                             rec.parent_wi[idx].astype(np.float64), wo, count=False)
        assert defined.all() and np.allclose(pdf, rec.parent_pdf[idx] * ln * ln, rtol=2e-3)
        tr = np.exp(-float(c.m.sigma_t[0]) * ln)
        want = rec.prefix_w[idx] * (f / pdf[:, None]) * rec.parent_rr[idx][:, None] * (tr / rec.edge_pdf[idx])[:, None]
        assert np.allclose(rec.flux[idx], want, rtol=2e-3)


def test_the_other_scenes_keep_their_streams():
    """the extra random number is drawn at rough-dielectric vertices only"""
    a = cases.make_case("cbox", 8, 8, 3000, 4.0)
    assert not ((a.ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF).any() and a.bsdfs.size == 0


# ---- (e) packed and linked round trips ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("linked", [False, True])
@pytest.mark.parametrize("scene", DC.SCENES)
def test_packed_records_keep_the_entry_the_flags_and_the_normals_side(scene, linked):
    c = cases.make_case(scene, 20, 16, 6000, 4.0)
    t = hip.MaterialTable()
    if linked:
        unp = hip.unpack_photons_linked(hip.pack_photons_linked(c.ph, t), t)
    else:
        unp = hip.unpack_photons(hip.pack_photons(c.ph, t), t)
    assert np.array_equal(unp.parent_g, c.ph.parent_g) and np.array_equal(unp.flags, c.ph.flags)
    gl = (unp.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    assert gl.sum() > 1000 and set(np.unique(unp.parent_g[gl])) == {0.0, 1.0}
    assert ((unp.parent_n[gl].astype(np.float64) * (unp.pos[gl].astype(np.float64) - unp.parent_pos[gl])).sum(1) > 0).all()
    assert (np.sign((unp.parent_n[gl] * unp.parent_wi[gl]).sum(1)) == np.sign((c.ph.parent_n[gl] * c.ph.parent_wi[gl]).sum(1))).all()
    assert all(np.array_equal(m, DC.classes(c.ph, c.bsdfs)[k]) for k, m in DC.classes(unp, c.bsdfs).items())


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------
def test_the_statement_reconnects_through_the_pane(monkeypatch):
    """the BRE-3D statement on the mirrored copy: with the wrapper installed the dielectric parents reconnect, in each of the
    four classes; without the table every one of their shifts fails"""
    c = cases.make_case("cbox_roughglass", 20, 16, 20000, 4.0)
    D.install(monkeypatch)
    D.reset_near()
    _, cnt = I.bre3d_full(D.mirrored_case(c))[:2]
    assert D.NEAR <= 2
    I.set_bsdfs(c.bsdfs[:0])
    _, none = I.bre3d_full(D.mirrored_case(c))[:2]
    I.set_bsdfs(c.bsdfs)
    through = cnt["diffuse_shifts"] - none["diffuse_shifts"]
    assert through == none["failed_shifts"] - cnt["failed_shifts"] and through > 300
    per_class = {}
    for k, m in DC.classes(c.ph, c.bsdfs).items():
        d = cases.Case()
        d.__dict__.update(c.__dict__)
        d.ph = DC.only_class(c.ph, m)
        per_class[k] = I.bre3d_full(D.mirrored_case(d))[1]["diffuse_shifts"] - none["diffuse_shifts"]
    print("reconnections through the pane:", through, "per class (reflected, from outside):", per_class)
    assert sum(per_class.values()) == through and min(per_class.values()) >= 50, per_class
