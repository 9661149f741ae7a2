"""Anisotropic Ward and rough-conductor surface parents (GVPM_BSDF_WARD_ANISO, GVPM_BSDF_ROUGHCONDUCTOR_ANISO; include/gvpm_hip.h),
CPU side: the table layout of the host scenes, the host's two samplers against the numpy statement of tests/indep_aniso.py
(chi-square; weight = eval / pdf), the statement's invariances, and the limit in which the frozen fp64 oracle already states what
the new kinds compute: alphaV == alphaU, whatever the tangent."""
import numpy as np
import pytest

import aniso_cases as AC
import cases
import indep_aniso as A
import indep_statements as I
import oracle_lib as O
from gvpm_amd import abi
from test_oracle_beams import make_beam_case
from test_oracle_vpm import make_vpm_case
from test_plastic_parents import _chi_square, _dirs, _same

SCENES = ["cbox_ward_aniso", "cbox_conductor_aniso"]
# the host walks with its materials' parameters in double, the table carries them as float32 (2^-24 relative; an alpha enters a
# Gaussian lobe as exp(-tan^2 / alpha^2): times 2 tan^2 / alpha^2, up to ~100 where the lobe is still sampled)
PARAM_RTOL = 1e-5


# ---- the helper and the table layout ---------------------------------------------------------------------------------------------
def test_bsdf_heads_covers_both_raw_entry_mechanisms():
    import plastic_cases as PC
    ward = abi.aniso_entry(abi.GVPM_BSDF_WARD_ANISO, 0.3, 0.1, 0.3, (1.0, 0.0, 0.0), weight=0.5)
    cond = abi.aniso_entry(abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO, 1.0, 0.1, 0.3, (0.0, 0.0, 1.0), eta=1.5, k=3.0)
    rough = PC.rough_entry("beckmann", 0.1, 0.3, 0.4)
    phong = np.zeros(1, abi.BSDF_DTYPE)
    phong["kind"] = abi.GVPM_BSDF_PHONG
    table = np.concatenate([ward, phong, rough, cond, phong])
    want = [0, 2, 3, 3 + PC.E, 3 + PC.E + AC.E]
    assert list(np.flatnonzero(abi.bsdf_heads(table))) == want
    assert abi.bsdf_heads(table[:0]).size == 0 and list(abi.bsdf_heads(ward[:1])) == [True]
    # a raw entry read as a head never shows a valid kind: 0 or a word beyond 2^23 in magnitude
    raw = table[~abi.bsdf_heads(table)]["kind"].astype(np.int64)
    assert ((raw == 0) | (np.abs(raw) >= 2 ** 23)).all()
    s, av = abi.frame_of(table, 0)
    assert list(s) == [1.0, 0.0, 0.0] and av == np.float32(0.3)
    assert (abi.GVPM_BSDF_WARD_ANISO, abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO, abi.GVPM_ANISO_ENTRIES) == (6, 8, 1)
    tails = {abi.GVPM_BSDF_ROUGHPLASTIC: 7, abi.GVPM_BSDF_WARD_ANISO: 1, abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO: 1, abi.GVPM_BSDF_PHONG: 0,
             abi.GVPM_BSDF_ROUGHCONDUCTOR: 0, abi.GVPM_BSDF_WARD: 0, abi.GVPM_BSDF_PLASTIC: 0}
    assert {k: abi.bsdf_tail_entries(k) for k in tails} == tails


@pytest.mark.parametrize("rot", ["", "_rot"])
@pytest.mark.parametrize("scene", SCENES)
def test_the_scenes_have_photons_behind_anisotropic_walls_and_a_table_for_them(scene, rot):
    c = cases.make_case(scene + rot, 40, 36, 30000, 2.5)
    heads = abi.bsdf_heads(c.bsdfs)
    assert c.bsdfs.size == 2 * AC.E and list(np.flatnonzero(heads)) == [0, AC.E]
    kind = abi.GVPM_BSDF_WARD_ANISO if scene == "cbox_ward_aniso" else abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO
    assert list(c.bsdfs["kind"][heads]) == [kind, kind]
    gl = (c.ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    idx = c.ph.parent_g[gl].astype(np.int64)
    assert gl.sum() >= 1000 and heads[idx].all() and set(np.unique(idx)) == {0, AC.E}   # parent_g always names a head
    assert (((c.ph.flags[gl] >> 2) & 7) == 1).all()                                     # diffuse reconnections
    raw = c.bsdfs.view(np.float32).reshape(-1, 16)
    normals = AC.wall_normals(c)                                                        # one plane per material
    axes = 0
    for k, h in enumerate((0, AC.E)):
        s, av = abi.frame_of(c.bsdfs, h)
        au = float(c.bsdfs["exponent"][h])
        assert abs(np.linalg.norm(s) - 1) < 1e-6 and (raw[h + 1, 4:] == 0).all()
        assert max(au, av) / min(au, av) > 3                                            # clearly different alphas
        assert abs(normals[k] @ s) < 0.9                                                # spans a frame with the wall's normal
        if not rot:
            axes += int(np.isclose(np.abs(s).max(), 1.0))
    assert rot or axes == 0                                                             # no tangent along a box axis
    if scene == "cbox_ward_aniso":
        assert list(c.bsdfs["sample_visible"][heads]) == [abi.GVPM_WARD_BALANCED, abi.GVPM_WARD_WARD]
        assert (c.bsdfs["distribution"][heads] == 0).all() and set(np.unique(c.ph.flags[gl] >> 16)) == {0x2, 0x8}
    else:
        assert list(c.bsdfs["distribution"][heads]) == [abi.GVPM_MICROFACET_BECKMANN, abi.GVPM_MICROFACET_GGX]
        assert (c.bsdfs["sample_visible"][heads] == 0).all() and set(np.unique(c.ph.flags[gl] >> 16)) == {0x8}
    # the `_rot` scene's tangents are the plain scene's, turned with everything else: same angle to the wall's normal
    if rot:
        p = cases.make_case(scene, 12, 10, 3000, 2.5)
        pn = AC.wall_normals(p)
        for k, h in enumerate((0, AC.E)):
            assert np.isclose(abi.frame_of(p.bsdfs, h)[0] @ pn[k], abi.frame_of(c.bsdfs, h)[0] @ normals[k], atol=1e-6)
            assert not np.allclose(abi.frame_of(p.bsdfs, h)[0], abi.frame_of(c.bsdfs, h)[0], atol=1e-3)
    cases.use_bsdfs(p if rot else c)


def test_the_device_generator_keeps_refusing_glossy_materials():
    """the anisotropic kinds are host-only like the other glossy ones: their material kinds lie beyond MAT_MIRROR, the last the
    device generator takes (checked on the source: gvpm_devgen_create needs a GPU)"""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gvpm_amd")
    core = open(os.path.join(root, "host", "synth_core.h")).read()
    kinds = dict((k, int(v)) for k, v in re.findall(r"(MAT_\w+) = (\d+)", core))
    assert kinds["MAT_WARD_ANISO"] > kinds["MAT_MIRROR"] and kinds["MAT_ROUGHCONDUCTOR_ANISO"] > kinds["MAT_MIRROR"]
    assert "kind > MAT_MIRROR) return bail(GVPM_ERR_UNSUPPORTED)" in open(os.path.join(root, "csrc", "synth_device.hip")).read()


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def _rows(rng, k, n):
    """k rows of (wi, wo) in the upper hemisphere of unit normal n"""
    u, v, _ = A.frame(np.broadcast_to(np.roll(n, 1) + 0.3, (1, 3)), n[None, :])
    loc = lambda d: d[:, 0:1] * u + d[:, 1:2] * v + d[:, 2:3] * n[None, :]
    return loc(_dirs(rng, k)), loc(_dirs(rng, k))


@pytest.mark.parametrize("which", ["ward", "conductor"])
def test_tangent_invariance_reciprocity_and_positivity(which):
    """the statement is invariant under s -> -s and under adding any multiple of n to s; Ward's f (without the cosine) and the
    conductor's f / F-free part are symmetric in (wi, wo); nothing is negative"""
    table, heads = AC.other_tables(which)
    rng = np.random.default_rng(5)
    k = 4000
    n = np.array([0.36, 0.48, 0.8])
    wi, wo = _rows(rng, k, n)
    kd = np.full((k, 3), 0.3 if which == "ward" else 0.0)
    nn = np.broadcast_to(n, (k, 3))
    for h in heads:
        idx = np.full(k, h)
        f, p, d = A.aniso_world(table, kd, idx, nn, wi, wo)
        assert d.all() and (f >= 0).all() and (p >= 0).all() and (p > 0).any() and np.isfinite(f).all() and np.isfinite(p).all()
        for change in (lambda s: -s, lambda s: s + 0.7 * n, lambda s: -2.5 * n + s):
            s64 = change(table.view(np.float32).reshape(-1, 16)[h + 1, 0:3].astype(np.float64))   # (float64: not re-rounded)
            f2, p2, d2 = A.aniso_world(table, kd, idx, nn, wi, wo, tangent=s64)
            assert d2.all() and np.allclose(f2, f, rtol=1e-12, atol=0) and np.allclose(p2, p, rtol=1e-12, atol=0)
        # reciprocity of the BRDF: f cos / cos_o is symmetric (Ward's original variant and Duer's, GGX / Beckmann conductors)
        fr, _, _ = A.aniso_world(table, kd, idx, nn, wo, wi)
        ci, co = (nn * wi).sum(-1), (nn * wo).sum(-1)
        assert np.allclose(f / co[:, None], fr / ci[:, None], rtol=1e-9, atol=1e-300)
    # a quarter turn is NOT an invariance: these alphas differ
    normal_turn = AC.turned(table, [n, n])
    f2, p2, _ = A.aniso_world(normal_turn, kd, np.full(k, heads[0]), nn, wi, wo)
    f, p, _ = A.aniso_world(table, kd, np.full(k, heads[0]), nn, wi, wo)
    assert np.abs(p2 - p).max() > 1e-3 * p.max()


def test_a_tangent_along_the_normal_spans_no_frame_and_raw_entries_are_unknown(monkeypatch):
    table, heads = AC.other_tables("ward")
    n = np.array([0.0, 0.6, 0.8])
    bad = table.copy()
    bad.view(np.float32).reshape(-1, 16)[1, 0:3] = -n
    rng = np.random.default_rng(6)
    wi, wo = _rows(rng, 32, n)
    kd, nn = np.full((32, 3), 0.3), np.broadcast_to(n, (32, 3))
    I.set_bsdfs(bad)
    A.install(monkeypatch)
    assert not I.phong_world(kd, np.zeros(32, np.int64), nn, wi, wo)[2].any()        # head 0: no frame
    f, p, known = I.phong_world(kd, np.full(32, AC.E), nn, wi, wo)                     # head 1 is fine
    assert known.all() and (p > 0).all()
    for raw in (1, AC.E + 1, -1, bad.size):                                           # frame entries, outside the table
        assert not I.phong_world(kd, np.full(32, raw), nn, wi, wo)[2].any()
    # the other kinds are handed on untouched
    c = cases.make_case("cbox_conductor", 12, 10, 500, 4.0)
    I.set_bsdfs(c.bsdfs)
    f_c, p_c, _ = I.phong_world(kd, np.zeros(32, np.int64), nn, wi, wo)
    I.set_bsdfs(np.concatenate([table, c.bsdfs]))
    f, p, known = I.phong_world(kd, np.full(32, 2 * AC.E), nn, wi, wo)
    assert known.all() and np.array_equal(f, f_c) and np.array_equal(p, p_c)
    cases.use_bsdfs(c)


# ---- the limit the fp64 oracle states: alphaV == alphaU, an arbitrary tangent ------------------------------------------------------
def _limit(c, records="ph"):
    """the case's isotropic table as equal-alpha anisotropic heads with skew tangents, its records re-labelled"""
    table, mapping = AC.equal_alpha_table(c.bsdfs)
    for k, h in enumerate(mapping):                      # not perpendicular to the normal, not along it
        d = abs(abi.frame_of(table, h)[0] @ AC.WALL_N[k])
        assert 0.3 < d < 0.9
    setattr(c, records, AC.relabelled(getattr(c, records), mapping))
    AC.use_table(c, table)
    return c


@pytest.mark.parametrize("scene", ["cbox_ward", "cbox_ward_duer", "cbox_conductor"])
def test_equal_alphas_are_the_isotropic_kind_bre3d(scene, monkeypatch):
    """cbox_ward (balanced, ward), cbox_ward_duer (the third variant) and cbox_conductor (Beckmann, GGX; pdf over all normals):
    the statement on the re-labelled records == the frozen oracle on the untouched case, 27 accumulators to 1e-9, counters equal"""
    c = cases.make_case(scene, 20, 16, 20000, 4.0)
    ref, rcnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    assert rcnt["diffuse_shifts"] > 300
    _limit(c)
    A.install(monkeypatch)
    acc, cnt = I.bre3d_full(c)
    _same(acc, cnt, ref, rcnt)
    # the frozen oracle does not know the new kinds: on the re-labelled records it fails those shifts
    O.set_bsdfs(c.bsdfs)
    _, cnt0, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    assert cnt0["failed_shifts"] > rcnt["failed_shifts"] + 100
    cases.use_bsdfs(cases.make_case(scene, 8, 8, 10, 4.0))


def test_equal_alphas_conductor_visible_normals_vpm(monkeypatch):
    """the other form of the pdf (sample_visible = 1: G1 of the projected roughness is in it), G-VPM"""
    c = make_vpm_case("cbox_conductor", 12, 10, 20000, 8.0, 6)
    vis = c.bsdfs.copy()
    vis["sample_visible"] = 1
    O.set_bsdfs(vis)
    ref, _, _, rcnt, _ = O.gather_vpm(c.p, c.m, c.tris, c.ph, c.rays, c.samples, 64, use_accel=True)
    assert rcnt["evaluations"] > 300
    c.bsdfs = vis
    _limit(c)
    A.install(monkeypatch)
    acc, cnt, _ = I.vpm_full(c)
    _same(acc, cnt, ref, rcnt)
    cases.use_bsdfs(cases.make_case("cbox_conductor", 8, 8, 10, 4.0))


def test_equal_alphas_ward_beams(monkeypatch):
    c = make_beam_case("cbox_ward", 12, 10, 1500, 4.0)
    ref, rcnt, _ = O.gather_beams(c.p, c.m, c.tris, c.beams, c.end_n, c.rays, c.r, 1, c.nb, 64)
    assert rcnt["diffuse_shifts"] > 50
    _limit(c, "beams")
    A.install(monkeypatch)
    acc, cnt = I.beams_full(c)
    _same(acc, cnt, ref, rcnt)
    cases.use_bsdfs(cases.make_case("cbox_ward", 8, 8, 10, 4.0))


# ---- the host's samplers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", SCENES)
def test_the_hosts_bounce_is_weight_times_pdf_equals_eval(scene):
    """flux = prefix * (f cos / pdf) * rr * (Tr / edgePdf) and pdf in solid angle = the stored area pdf * len^2 of the photons behind
    each anisotropic wall, against the numpy statement (the records are float32)"""
    c = cases.make_case(scene, 20, 16, 20000, 4.0)
    I.set_bsdfs(c.bsdfs)
    all_gl = np.flatnonzero((c.ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF)
    for h in np.flatnonzero(abi.bsdf_heads(c.bsdfs)):
        gl = all_gl[c.ph.parent_g[all_gl] == h][:400]
        assert gl.size >= 10, (h, gl.size)
        d = c.ph.pos[gl].astype(np.float64) - c.ph.parent_pos[gl]
        ln = np.linalg.norm(d, axis=1)
        wo = d / ln[:, None]
        f, pdf, known = A.phong_world_with_aniso(c.ph.parent_scat[gl].astype(np.float64), c.ph.parent_g[gl].astype(np.int64),
                                                 c.ph.parent_n[gl].astype(np.float64), c.ph.parent_wi[gl].astype(np.float64), wo)
        assert known.all() and (pdf > 0).all()
        assert np.allclose(pdf, c.ph.parent_pdf[gl] * ln * ln, rtol=2e-4), h
        tr = np.exp(-float(c.m.sigma_t[0]) * ln)
        want = c.ph.prefix_w[gl] * (f / pdf[:, None]) * c.ph.parent_rr[gl][:, None] * (tr / c.ph.edge_pdf[gl])[:, None]
        assert np.allclose(c.ph.flux[gl], want, rtol=4e-4), h


@pytest.mark.parametrize("wall", [0, 1])
@pytest.mark.parametrize("scene", SCENES)
def test_sampling_matches_the_statements_pdf_chi_square_and_weight_is_eval_over_pdf(scene, wall):
    """the host's bounce (Ward::sample's anisotropic phiH / thetaH; sampleAll's anisotropic branch) against the numpy pdf, 10 x 20
    bins at significance 0.01 as the other sampler tests; and the weight it returns IS eval / pdf (to 1e-5 against the float32
    table here; to 1e-9 with the host's own parameters in the next test)"""
    from gvpm_amd.host import SynthScene
    sc = SynthScene(scene, 8, 8)
    table = sc.bsdfs()
    mat = AC.aniso_materials(sc)[wall]
    head = wall * AC.E
    n = AC.WALL_N[wall]
    kd = np.array([[0.3, 0.3, 0.3], [0.2, 0.25, 0.4]])[wall] if scene == "cbox_ward_aniso" else np.zeros(3)
    rng = np.random.default_rng(51 + wall)
    # the local frame the histogram is taken in: any frame around n
    u, v, _ = A.frame(np.array([[0.3, 0.5, 0.2]]), n[None, :])
    to_world = lambda d: d[..., 0:1] * u + d[..., 1:2] * v + d[..., 2:3] * n
    to_local = lambda d: np.stack([(d * u).sum(-1), (d * v).sum(-1), (d * n).sum(-1)], -1)
    exact = {"cbox_ward_aniso": [(0.08, 0.35), (0.4, 0.1)], "cbox_conductor_aniso": [(0.12, 0.45), (0.35, 0.08)]}[scene][wall]
    assert np.allclose([float(table["exponent"][head]), abi.frame_of(table, head)[1]], exact, rtol=1e-6)

    def sample(wi_l, count):
        wi = to_world(wi_l)[0]
        res = [sc.sample_aniso(mat, n, wi, *rng.random(2)) for _ in range(count)]
        ok = [r for r in res if r is not None]
        for wo, weight, pdf in ok[:50]:
            f, p, d = A.aniso_world(table, kd[None, :], np.array([head]), n[None, :], wi[None, :], wo[None, :])
            assert d.all() and abs(p[0] - pdf) < PARAM_RTOL * pdf and np.allclose(f[0] / p[0], weight, rtol=PARAM_RTOL)
        return to_local(np.array([r[0] for r in ok])), len(res) - len(ok)

    def pdf_of(wi_l, dirs_l):
        dirs = to_world(dirs_l)
        wi = to_world(wi_l)[0]
        return A.aniso_world(table, np.broadcast_to(kd, dirs.shape), np.full(len(dirs), head), np.broadcast_to(n, dirs.shape),
                             np.broadcast_to(wi, dirs.shape), dirs)[1]

    _chi_square(sample, pdf_of, rng, 6, 30000)


# the host's materials as the scenes set them (synth.cpp), in double: (alphaU, alphaV), tangent, kd, ks, eta, k, variant | distribution
HOST = {
    "cbox_ward_aniso": [((0.08, 0.35), (1.0, 0.0, 0.6), (0.3, 0.3, 0.3), (0.5, 0.5, 0.45), 0, 0, abi.GVPM_WARD_BALANCED),
                        ((0.4, 0.1), (0.9, 0.35, 0.25), (0.2, 0.25, 0.4), (0.3, 0.3, 0.3), 0, 0, abi.GVPM_WARD_WARD)],
    "cbox_conductor_aniso": [((0.12, 0.45), (1.0, 0.0, 0.6), (0, 0, 0), (1, 1, 1), (0.2004, 0.9240, 1.1022), (3.9129, 2.4528, 2.1421),
                              abi.GVPM_MICROFACET_BECKMANN),
                             ((0.35, 0.08), (0.9, 0.35, 0.25), (0, 0, 0), (1, 1, 1), (1.6574, 0.8803, 0.5212), (9.2238, 6.2695, 4.8370),
                              abi.GVPM_MICROFACET_GGX)]}


@pytest.mark.parametrize("scene", SCENES)
def test_sampling_weight_is_eval_over_pdf_to_1e9(scene):
    """weight = eval / pdf (and the pdf itself) of the host's bounce against the statement to 1e-9: the statement is given the
    host's own double-precision parameters (HOST above, checked against the float32 table), so no rounding of a table is in
    the comparison"""
    from gvpm_amd.host import SynthScene
    sc = SynthScene(scene, 8, 8)
    table = sc.bsdfs()
    ward = scene == "cbox_ward_aniso"
    lum = lambda c: np.asarray(c, np.float64) @ np.array([0.212671, 0.715160, 0.072169])
    rng = np.random.default_rng(77)
    for wall, mat in enumerate(AC.aniso_materials(sc)):
        (au, av), tang, kd, ks, eta, kk, sel = HOST[scene][wall]
        head = wall * AC.E
        tang = np.asarray(tang) / np.linalg.norm(tang)
        assert np.allclose([float(table["exponent"][head]), abi.frame_of(table, head)[1]], (au, av), rtol=1e-6)
        assert np.allclose(abi.frame_of(table, head)[0], tang, atol=1e-6) and np.allclose(table["specular"][head], ks, rtol=1e-6)
        n = AC.WALL_N[wall]
        wi, _ = _rows(rng, 400, n)
        one = lambda x: np.broadcast_to(np.asarray(x, np.float64), (1, 3))
        checked = 0
        for q in range(400):
            r = sc.sample_aniso(mat, n, wi[q], *rng.random(2))
            if r is None:
                continue
            wo, weight, pdf = r
            f, p, d = A.aniso_rows(np.array([ward]), one(ks), au, av, one(tang), lum(ks) / (lum(kd) + lum(ks)) if ward else 0.0,
                                   np.array([sel]), np.array([(not ward) and sel == abi.GVPM_MICROFACET_GGX]), np.array([False]),
                                   one(eta), one(kk), one(kd), one(n), one(wi[q]), one(wo))
            assert d[0] and abs(p[0] - pdf) <= 1e-9 * pdf, (p, pdf)
            assert np.allclose(f[0] / p[0], weight, rtol=1e-9, atol=1e-300)
            checked += 1
        assert checked > 150
