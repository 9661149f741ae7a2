"""Two-component mixture parents on the device (GVPM_BSDF_MIXTURE; parent_bsdf.h mixtureEval over roughConductorEval): what
gvpm_upload_bsdfs accepts and refuses, pins against the frozen fp64 oracle at degenerate weights (relabelled tables over
cbox_conductor's records: the oracle knows the plain conductor and the Lambertian, not the kind), linearity of the device against
itself, component entries and corners against the numpy statement of tests/indep_mixture.py, the gathers of every technique that
reconnects on the three synthetic scenes, the exact pass, the linked upload and a moved and resized scene.

Counters: the statement counts the reconnections within rounding of an fp32 decision (the children's own: indep_mixture.near());
failed_shifts / diffuse_shifts may differ from the statement's by at most that count, and it must be <= 2 in every case (`agree` of
test_dielectric_parents_gpu.py asserts both)."""
import numpy as np
import pytest

import aniso_cases as AC
import indep_dielectric as D
import indep_mixture as M
import indep_statements as I
import mixture_cases as C
import oracle_lib as O
import similarity_cases as S
from gvpm_amd import abi, hip
from test_dielectric_parents_gpu import agree
from test_oracle_beams import TECHS
from test_parity_gpu import device_gather, l2, TOL
from test_plastic_parents_gpu import run_vpm, run_beams, TOL_BEAMS

pytestmark = pytest.mark.gpu
RECORDS = {"bre": "ph", "vpm": "ph", "beams": "beams"}
STATEMENT = {"bre": lambda c: I.bre3d_full(c)[:2], "vpm": lambda c: I.vpm_full(c)[:2], "beams": lambda c: I.beams_full(c)[:2]}
DEVICE = {"bre": lambda c: device_gather(c)[:2], "vpm": run_vpm, "beams": run_beams}
INV, UNS = abi.GVPM_ERR_INVALID_ARG, abi.GVPM_ERR_UNSUPPORTED
KD = (0.35, 0.5, 0.25)          # the fixed reflectance of the pins and of linearity


def statement(c, technique):
    """(film, counters, reconnections near an fp32 decision) of the wrapped numpy statement"""
    M.reset_near()
    ref, cnt = STATEMENT[technique](D.mirrored_case(c, RECORDS[technique]))
    return ref, cnt, M.near()


def through_mixtures(c, cnt, technique):
    """Reconnections through mixture heads: the records of parent type GVPM_PARENT_SURFACE_BSDF all name such heads here (asserted),
    so the statement run once more WITHOUT the table fails exactly their shifts"""
    records = getattr(c, RECORDS[technique])
    gl = (records.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    assert gl.any() and M.is_mixture(c.bsdfs)[records.parent_g[gl].astype(np.int64)].all()
    table = c.bsdfs
    I.set_bsdfs(table[:0])
    try:
        none = STATEMENT[technique](c)[1]
    finally:
        I.set_bsdfs(table)
    n = cnt["diffuse_shifts"] - none["diffuse_shifts"]
    assert n == none["failed_shifts"] - cnt["failed_shifts"]
    print("reconnections through mixture heads:", n)
    return n


def check(c, technique, monkeypatch, what="", floor=300):
    M.install(monkeypatch)
    ref, cnt, near = statement(c, technique)
    acc, st = DEVICE[technique](c)
    agree(acc, st, ref, cnt, near, tol=TOL_BEAMS if technique == "beams" else TOL, what=what)
    if floor:
        assert through_mixtures(c, cnt, technique) >= floor
    return acc, st, ref, cnt


# ---- the case builders (module level: the sizes were chosen with them on the CPU) ------------------------------------------------
def bre_case(scene, **kw):
    return C.make_case(scene, 20, 16, 20000, 4.0, **kw)


def vpm_case(scene):
    return C.make_vpm_case(scene, 12, 10, 8000, 8.0, 6)


def beam_case(scene, tech=abi.GVPM_BEAM_BEAM_3D_OPTIMIZED):
    return C.make_beam_case(scene, 12, 10, 800, 5.0, technique=tech)


# ---- (a) acceptance and refusal ---------------------------------------------------------------------------------------------------
def _context(c):
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    return ctx


def test_upload_accepts_the_scenes_tables_and_refuses_bad_ones_before_anything_is_copied(monkeypatch):
    """every table of the header's list, one defect each, with the stated code; a refusal leaves the previous table in force: after
    all of them the gather is the one of the good table"""
    c = bre_case("cbox_mixture")
    good = c.bsdfs
    ctx = _context(c)
    from gvpm_amd.host import SynthScene
    for scene in C.SCENES:
        ctx.upload_bsdfs(SynthScene(scene, 8, 8).bsdfs())          # (not through make_case: the statements' table is process state)
    for table in C.accepted_tables():
        ctx.upload_bsdfs(table)
    ctx.upload_bsdfs(good)
    refused = C.refused_tables()
    assert len(refused) >= 25
    for what, table, code in refused:
        with pytest.raises(hip.GvpmError) as e:
            ctx.upload_bsdfs(np.ascontiguousarray(table))
        assert e.value.code == (INV if code == "invalid" else UNS), (what, e.value)
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(c.rays)
    ctx.gather(1, c.nb)
    acc, st = ctx.download_accum(), ctx.stats()
    ctx.upload_bsdfs(good[:0])
    ctx.close()
    M.install(monkeypatch)
    ref, cnt, near = statement(c, "bre")
    agree(acc, st, ref, cnt, near, what="after refusals")


# ---- (b) pins against the frozen fp64 oracle ----------------------------------------------------------------------------------------
def _oracle(c):
    O.set_bsdfs(c.bsdfs)
    ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    return ref, cnt


def test_weights_one_zero_are_the_oracles_plain_conductor():
    """cbox_conductor's records (20 x 16 pixels, 20 000 photons, scale 4: 7 797 evaluations, 1 759 reconnections through the walls)
    under mixtures {that wall's conductor entry, Lambertian} at weights (1, 0), both components: the film and the counters of the
    oracle on the plain conductor table"""
    c = C.conductor_records()
    ref, cnt = _oracle(c)
    C.over_conductor(c, (1.0, 0.0))
    acc, st = DEVICE["bre"](c)
    agree(acc, st, ref, cnt, 0, what="weights (1, 0)")
    assert cnt["diffuse_shifts"] > 1500


def test_weights_zero_one_are_the_oracles_lambertian():
    """the same mixtures at weights (0, 1) with the records' parent_scat overwritten by a fixed reflectance: the oracle on the same
    records retyped GVPM_PARENT_SURFACE"""
    c = C.retyped_lambertian(C.conductor_records(), KD)
    ref, cnt = _oracle(c)
    c = C.set_parent_scat(C.conductor_records(), KD)
    C.over_conductor(c, (0.0, 1.0))
    acc, st = DEVICE["bre"](c)
    agree(acc, st, ref, cnt, 0, what="weights (0, 1)")
    assert cnt["diffuse_shifts"] > 1500


# ---- (c) linearity: the device against itself -------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(0.6, 0.4), (0.9, 0.8)])
def test_the_shifted_accumulators_are_linear_in_the_weights(weights):
    """use_mis = 0: the four `shifted` accumulators under weights (w_0, w_1) are w_0 x those of the plain conductor table plus w_1 x
    those of the retyped Lambertian records, to TOL of the mean luminance (a failed shift adds zero flux, so the differing success
    sets do not break this).  The accumulators also hold the shifts through every OTHER parent (the medium, the Lambertian walls, the
    emitter), once in each of the three runs: where the weights do not sum to 1 -- the second pair -- that share, measured with an
    empty table (the glossy shifts all fail), enters with 1 - w_0 - w_1."""
    c = C.conductor_records(use_mis=0)
    acc_c = DEVICE["bre"](c)[0].astype(np.float64)
    acc_o = DEVICE["bre"](C.with_table(C.conductor_records(use_mis=0), c.bsdfs[:0]))[0].astype(np.float64)
    acc_l = DEVICE["bre"](C.retyped_lambertian(C.conductor_records(use_mis=0), KD))[0].astype(np.float64)
    c = C.set_parent_scat(C.conductor_records(use_mis=0), KD)
    C.over_conductor(c, weights)
    acc_m, st = DEVICE["bre"](c)
    acc_m = acc_m.astype(np.float64)
    lum = acc_c[..., 0:3].mean()
    # (27 floats per pixel: mediumFlux, shiftedMediumFlux[4], weightedMediumFlux[4], each RGB -- include/gvpm_hip.h)
    want = weights[0] * acc_c + weights[1] * acc_l + (1.0 - weights[0] - weights[1]) * acc_o
    shifted = slice(3, 15)
    assert np.abs(acc_c[..., shifted] - acc_o[..., shifted]).max() > 0.01 * lum          # (the glossy share is there)
    err = np.sqrt(((acc_m[..., shifted] - want[..., shifted]) ** 2).mean()) / lum
    print("linearity", weights, err, st)
    assert st["diffuse_shifts"] > 1500 and lum > 0 and err < TOL, err


# ---- (d) component entries and corners, judged by the statement -----------------------------------------------------------------------
def _corner(which):
    c = C.conductor_records()
    if which == "component 1 over alpha 0.03":
        walls = np.concatenate([C.conductor_entry(0.03, C.CU), C.conductor_entry(0.03, C.AL, C.GGX)])
        C.over_conductor(c, (0.7, 0.3), component=1, wall_entries=walls)
    elif which == "component 2 beside an absent child":
        C.over_conductor(c, (0.3, 0.7), other=C.ABSENT, component=2, conductor_first=False)
    elif which == "children after the mixture":
        C.over_conductor(c, (0.6, 0.4), children_last=True)
    elif which == "anisotropic and Phong-distribution children":
        walls = np.concatenate([C.aniso_entry(0.12, 0.45, AC.SKEW[0], C.CU), C.conductor_entry(0.3, C.AL, C.PHONG)])
        C.over_conductor(c, (0.5, 0.5), wall_entries=walls)
    elif which == "weights summing above 1":
        C.over_conductor(c, (0.9, 0.8))
    return c


CORNERS = ["component 1 over alpha 0.03", "component 2 beside an absent child", "children after the mixture",
           "anisotropic and Phong-distribution children", "weights summing above 1"]


@pytest.mark.parametrize("which", CORNERS)
def test_corners_match_the_numpy_statement(which, monkeypatch):
    """cbox_conductor's records under relabelled tables (20 x 16 pixels, 20 000 photons, scale 4).  Measured on the CPU with the statement
    (evaluations / reconnections through mixture heads / near a decision): component 1 over alpha 0.03: 7 823 / 1 258 / 0 (the lobes of
    alpha 0.03 are met by 1 258 of the 1 744 reconnections; the others have pdf = 0 and fail, in the statement as on the device: that
    case is held to 150); component 2 beside an absent child: 7 823 / 1 741 / 0; children after the mixture, anisotropic and
    Phong-distribution children, weights summing above 1: 7 823 / 1 744 / 0 each."""
    c = _corner(which)
    check(c, "bre", monkeypatch, what=which, floor=150 if which == CORNERS[0] else 300)


def test_an_absent_child_is_the_same_entry_with_a_real_conductor_there():
    """a component-2 entry whose other child is -2 against the same entry with a real conductor in its place: the film to 1e-6 of the
    mean luminance (the sums are atomic), the counters exactly"""
    c = _corner("component 2 beside an absent child")
    acc_a, st_a = DEVICE["bre"](c)
    c = C.conductor_records()
    C.over_conductor(c, (0.3, 0.7), other=1, component=2, conductor_first=False)
    acc_r, st_r = DEVICE["bre"](c)
    lum = acc_r[..., 0:3].astype(np.float64).mean()
    err = l2(acc_a, acc_r.astype(np.float64), lum)
    print("absent against real", err, st_a, st_r)
    assert st_a == st_r and st_a["diffuse_shifts"] > 300 and lum > 0 and err < 1e-6, err


# ---- (e) the three scenes against the statement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(use_mis=0), dict(power_heuristic=1), dict(use_shift_null=0)])
@pytest.mark.parametrize("scene", C.SCENES)
def test_bre3d_matches_the_numpy_statement(scene, kw, monkeypatch):
    """20 x 16 pixels, 20 000 photons, scale 4.  Measured with these sizes on the CPU (default flags; evaluations / reconnections through
    mixture heads / near a decision): cbox_mixture 7 848 / 3 715 / 0, _rot 19 394 / 5 275 / 0, cbox_mixture1 7 802 / 1 427 / 0.  Four mixture
    walls carry twice the reconnections of the siblings' two glossy walls (1 759)."""
    check(bre_case(scene, **kw), "bre", monkeypatch, what=f"{scene} {kw}")


@pytest.mark.parametrize("scene", C.SCENES)
def test_vpm_matches_the_numpy_statement(scene, monkeypatch):
    """12 x 10 pixels, 8 000 photons, scale 8, 6 camera samples.  Measured: cbox_mixture 5 247 / 2 005 / 0, _rot 22 497 / 5 090 / 0,
    cbox_mixture1 5 161 / 641 / 0."""
    check(vpm_case(scene), "vpm", monkeypatch, what=f"vpm {scene}")


@pytest.mark.parametrize("tech", TECHS)
@pytest.mark.parametrize("scene", C.SCENES)
def test_beams_match_the_numpy_statement(scene, tech, monkeypatch):
    """12 x 10 pixels, 800 beams, scale 5; the floor is 100 reconnections through mixture heads.  Measured (3D and 1D kernel):
    cbox_mixture 775 / 300 / 0 and 777 / 297 / 0, _rot 1 086 / 291 / 0 and 1 119 / 288 / 0, cbox_mixture1 771 / 129 / 0 and 784 / 121 / 0 (its two
    mixture walls: the siblings' one reconnection in six)."""
    check(beam_case(scene, tech), "beams", monkeypatch, what=f"beams {tech} {scene}", floor=100)


# ---- (f) the exact pass, the linked upload, a moved and resized scene -----------------------------------------------------------------
def test_exact_all_bre(monkeypatch):
    """GVPM_EXACT_ALL=1: every shift through the fp64 pass (exact_shift.hip), which evaluates these parents through glossyParentEval"""
    monkeypatch.setenv("GVPM_EXACT_ALL", "1")
    check(bre_case("cbox_mixture_rot"), "bre", monkeypatch, what="exact", floor=0)


def test_linked_photons_end_to_end(monkeypatch):
    """the mixture's head index rides through the linked records"""
    c = bre_case("cbox_mixture1")
    t = hip.MaterialTable()
    pk = hip.pack_photons_linked(c.ph, t)
    unp = hip.unpack_photons_linked(pk, t)
    assert np.array_equal(unp.parent_g, c.ph.parent_g) and np.array_equal(unp.flags, c.ph.flags)
    ctx = _context(c)
    ctx.upload_bsdfs(c.bsdfs)
    ctx.upload_materials(t)
    ctx.upload_photons_linked(pk)
    ctx.upload_camera_beams(c.rays)
    ctx.gather(1, c.nb)
    acc, st = ctx.download_accum().astype(np.float64), ctx.stats()
    ctx.close()
    M.install(monkeypatch)
    c.ph = unp
    ref, cnt, near = statement(c, "bre")
    agree(acc, st, ref, cnt, near, what="linked")


def test_a_moved_and_resized_scene(monkeypatch):
    """the `large` transform of tests/similarity_cases.py (64 x, 360 units from the origin): the table is the scene's own"""
    check(S.named(bre_case("cbox_mixture"), "large"), "bre", monkeypatch, what="large", floor=0)


def test_the_device_generator_refuses_the_new_scenes():
    """glossy materials are the host generator's: gvpm_devgen_create answers GVPM_ERR_UNSUPPORTED, as for every glossy scene"""
    from gvpm_amd.host import SynthScene
    for scene in C.SCENES:
        with pytest.raises(hip.GvpmError) as e:
            hip.DeviceGenerator(SynthScene(scene, 16, 12))
        assert e.value.code == UNS, e.value
