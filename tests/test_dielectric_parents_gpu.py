"""Rough-dielectric surface parents on the device (GVPM_BSDF_ROUGHDIELECTRIC; parent_bsdf.h roughDielectricEval): reflection and
transmission, met from both sides.  The gathers of every technique that reconnects against the numpy statement of
tests/indep_dielectric.py (the frozen fp64 oracle does not know the kind: it fails these shifts), tables the scenes do not have,
the limit in which the oracle does state it (reflection from outside = the rough conductor with k = 0), the side of incidence,
the exact passes, the packed and linked uploads, what gvpm_upload_bsdfs refuses, and records of other kinds lit from behind.

Counters: the statement counts the reconnections within rounding of an fp32 decision this kind adds (indep_dielectric.NEAR: D cos_H
or D' cos_H against 1e-20, the edge of total internal reflection, |cos_i| ~ 0, |wi + eta wo|^2 ~ 1e-12); failed_shifts /
diffuse_shifts may differ from the statement's by at most that count, and it must be <= 2 in every case (a cap, asserted).

The statements run on the mirrored copy of the records (indep_dielectric.mirrored_case); the device gets the records as they
are."""
import numpy as np
import pytest

import cases
import dielectric_cases as DC
import indep_dielectric as D
import indep_statements as I
import oracle_lib as O
from gvpm_amd import abi, hip
from test_oracle_beams import make_beam_case, TECHS
from test_oracle_vpm import make_vpm_case
from test_parity_gpu import device_gather, l2, TOL
from test_plastic_parents_gpu import run_vpm, run_beams, oracle_diffuse_shifts, TOL_BEAMS

pytestmark = pytest.mark.gpu
RECORDS = {"bre": "ph", "vpm": "ph", "beams": "beams"}
STATEMENT = {"bre": lambda c: I.bre3d_full(c)[:2], "vpm": lambda c: I.vpm_full(c)[:2], "beams": lambda c: I.beams_full(c)[:2]}
DEVICE = {"bre": lambda c: device_gather(c)[:2], "vpm": run_vpm, "beams": run_beams}


def statement(c, technique):
    """(film, counters, reconnections near an fp32 decision) of the wrapped numpy statement on the mirrored records"""
    D.reset_near()
    ref, cnt = STATEMENT[technique](D.mirrored_case(c, RECORDS[technique]))
    return ref, cnt, D.NEAR


def agree(acc, st, ref, cnt, near=0, tol=TOL, what=""):
    lum = max(ref[..., 0:3].mean(), 1e-30)
    err = l2(acc, ref, lum)
    print(f"{what}: evaluations {st['evaluations']} / {cnt['evaluations']}, shifts "
          + ", ".join(f"{k} {st[k]} / {cnt[k]}" for k in ("null_shifts", "diffuse_shifts", "failed_shifts"))
          + f", near a decision {near}, L2 / lum {err:.3e}")
    assert near <= 2, near
    assert st["evaluations"] == cnt["evaluations"], (st, cnt)
    assert st["null_shifts"] == cnt["null_shifts"], (st, cnt)
    for k in ("diffuse_shifts", "failed_shifts"):
        assert abs(st[k] - cnt[k]) <= near, (k, st, cnt)
    assert err < tol, err
    return err


def through_dielectric(c, st, cnt, technique):
    """Reconnections through dielectric parents: the records of parent type GVPM_PARENT_SURFACE_BSDF all name such entries here
    (asserted), so the statement run once more WITHOUT the table fails exactly their shifts.  Beside it the feature itself: the
    device reconnects more shifts than the frozen oracle does on the same inputs."""
    records = getattr(c, RECORDS[technique])
    gl = (records.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    assert gl.any() and (c.bsdfs["kind"][records.parent_g[gl].astype(np.int64)] == D.KIND).all()
    table = c.bsdfs
    I.set_bsdfs(table[:0])
    try:
        none = STATEMENT[technique](c)[1]
    finally:
        I.set_bsdfs(table)
    n = cnt["diffuse_shifts"] - none["diffuse_shifts"]
    assert n == none["failed_shifts"] - cnt["failed_shifts"]
    assert st["diffuse_shifts"] > oracle_diffuse_shifts(c, technique)
    print("reconnections through dielectric parents:", n)
    return n


def check(c, technique, monkeypatch, tol=None, what="", count=True):
    D.install(monkeypatch)
    ref, cnt, near = statement(c, technique)
    acc, st = DEVICE[technique](c)
    agree(acc, st, ref, cnt, near, tol=tol or (TOL_BEAMS if technique == "beams" else TOL), what=what)
    if count:
        assert through_dielectric(c, st, cnt, technique) >= 300
    return acc, st, ref, cnt


# ---- the case builders (module level: the sizes were chosen with them on the CPU) ------------------------------------------------
def bre_case(scene, **kw):
    return cases.make_case(scene, 20, 16, 20000, 4.0, **kw)


def vpm_case(scene):
    return make_vpm_case(scene, 12, 10, 8000, 8.0, 6)


def beam_case(scene, tech=abi.GVPM_BEAM_BEAM_3D_OPTIMIZED):
    return make_beam_case(scene, 12, 10, 800, 5.0, technique=tech)


def with_table(c, table):
    DC.use_table(c, table)
    O.set_bsdfs(c.bsdfs)   # (the oracle ignores the kind: those shifts fail there)
    return c


# ---- the two scenes: device against the numpy statement ------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(use_mis=0), dict(power_heuristic=1), dict(use_shift_null=0)])
@pytest.mark.parametrize("scene", DC.SCENES)
def test_bre3d_matches_the_numpy_statement(scene, kw, monkeypatch):
    """20 x 16 pixels, 20 000 photons, scale 4 (the statement: seconds).  Measured with these sizes on the CPU (default flags;
    evaluations / reconnections through dielectric parents / near a decision; then the reconnections per class -- reflected met
    from outside, reflected from inside, transmitted from outside, transmitted from inside): cbox_roughglass 6 551 / 6 609 / 0,
    110 / 304 / 6 093 / 102; _rot 17 234 / 10 647 / 0, 314 / 719 / 9 335 / 279."""
    check(bre_case(scene, **kw), "bre", monkeypatch, what=f"{scene} {kw}")


@pytest.mark.parametrize("scene", DC.SCENES)
def test_vpm_matches_the_numpy_statement(scene, monkeypatch):
    """12 x 10 pixels, 8 000 photons, scale 8, 6 camera samples (at the 20 000 photons of the other kinds' tests the pane alone
    had 8 121 and 19 933 reconnections and the statement took half a minute).  Measured: cbox_roughglass 3 657 / 3 218 / 0, _rot
    18 919 / 7 799 / 0."""
    check(vpm_case(scene), "vpm", monkeypatch, what=f"vpm {scene}")


@pytest.mark.parametrize("tech", TECHS)
@pytest.mark.parametrize("scene", DC.SCENES)
def test_beams_match_the_numpy_statement(tech, scene, monkeypatch):
    """12 x 10 pixels, 800 beams, scale 5 (at 3 000 beams: 1 547 to 1 909 reconnections through the pane, and a minute and more of
    the statement's plain Python).  Measured (3D and 1D kernel): cbox_roughglass 376 / 424 / 0 and 381 / 430 / 0, _rot 657 / 422 / 0 and
    668 / 509 / 0."""
    check(beam_case(scene, tech), "beams", monkeypatch, what=f"beams {tech} {scene}")


# ---- relabelled tables: what the scenes do not have -------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.08, 0.5])
def test_relabelled_bre3d_matches_the_numpy_statement(alpha, monkeypatch):
    """what a reconnection evaluates is a function of the record and the table: the records of cbox_roughglass under GGX entries
    sampled with visible normals (the pdf's other form), index 1.33, other tints, alpha 0.08 and 0.5.  Measured (either alpha:
    with visible normals the pdf is zero only where D is): 6 551 / 7 262 / 0, per class 111 / 312 / 6 737 / 102."""
    c = with_table(bre_case("cbox_roughglass"), DC.other_table(alpha))
    assert (c.bsdfs["sample_visible"] == 1).all() and (c.bsdfs["distribution"] == abi.GVPM_MICROFACET_GGX).all()
    check(c, "bre", monkeypatch, what=f"relabelled GGX visible alpha {alpha}")


def test_relabelled_vpm_and_beams(monkeypatch):
    """Measured: G-VPM on cbox_roughglass_rot, alpha 0.08: 18 919 / 9 661 / 0; beams 3D on cbox_roughglass, alpha 0.5: 376 / 510 / 0"""
    check(with_table(vpm_case("cbox_roughglass_rot"), DC.other_table(0.08)), "vpm", monkeypatch, what="relabelled vpm")
    check(with_table(beam_case("cbox_roughglass"), DC.other_table(0.5)), "beams", monkeypatch, what="relabelled beams")


# ---- the limit: reflection from outside against the frozen fp64 oracle --------------------------------------------------------------
def _limit_case(make, records="ph"):
    """cbox_conductor's records: the oracle under a conductor table with k = 0 and eta (1.5, 1.5, 1.5), the device under the
    dielectric entries that equal it in reflection from outside.  Visible normals and use_mis = 0: the pdfs differ by the
    factor F, so only the weight-free film can agree -- and the counters, since F > 0."""
    o, d = make("cbox_conductor"), make("cbox_conductor")
    cond, diel = DC.conductor_limit(o.bsdfs)
    DC.use_table(o, cond)
    DC.use_table(d, diel)
    O.set_bsdfs(o.bsdfs)
    assert ((getattr(d, records).flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF).sum() > 300
    return d, o


def test_limit_bre_matches_fp64_oracle():
    d, o = _limit_case(lambda s: cases.make_case(s, 40, 36, 30000, 2.5, use_mis=0))
    ref, cnt, _ = O.gather_bre(o.p, o.m, o.tris, o.ph, o.rays, o.r, 1, o.nb, 64, use_accel=False)
    acc, st, _ = device_gather(d)
    agree(acc, st, ref, cnt, 0, what="limit bre")
    assert st["evaluations"] > 10000 and st["diffuse_shifts"] > 10000


def test_limit_vpm_matches_fp64_oracle():
    d, o = _limit_case(lambda s: make_vpm_case(s, 32, 28, 40000, 5.0, nb=10, use_mis=0))
    ref, _, _, cnt, _ = O.gather_vpm(o.p, o.m, o.tris, o.ph, o.rays, o.samples, 64, use_accel=False)
    acc, st = run_vpm(d)
    agree(acc, st, ref, cnt, 0, what="limit vpm")
    assert st["evaluations"] > 5000 and st["diffuse_shifts"] > 2000


def test_limit_beams3d_matches_fp64_oracle():
    d, o = _limit_case(lambda s: make_beam_case(s, 32, 28, 12000, 2.5, use_mis=0), records="beams")
    ref, cnt, _ = O.gather_beams(o.p, o.m, o.tris, o.beams, o.end_n, o.rays, o.r, 1, o.nb, 64)
    acc, st = run_beams(d)
    agree(acc, st, ref, cnt, 0, tol=TOL_BEAMS, what="limit beams")
    assert st["evaluations"] > 20000 and st["diffuse_shifts"] > 5000


# ---- the side of incidence matters ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", DC.SCENES)
def test_the_side_matters(scene, monkeypatch):
    """each surface's two entries exchanged (every record now evaluates the index of the wrong side): the statement's film moves
    by more than the parity bar (checked on the CPU: by 0.24 and 0.078 of the mean luminance) and the device's moves with it.
    3 000 photons: a photon transmitted from outside and evaluated with the inverse index sits on the edge of total internal
    reflection wherever wi . wo = -1 / eta -- cos^2(theta_T) = (wi . wo + 1 / eta)^2 / |H|^2 touches zero along a whole band of
    directions -- and at 20 000 photons 7 and 6 reconnections lay within the statement's 1e-6 of it; here 1 and 1."""
    c = cases.make_case(scene, 20, 16, 3000, 4.0)
    acc, st, ref, cnt = check(c, "bre", monkeypatch, what=f"{scene} as built", count=False)
    lum = ref[..., 0:3].mean()
    with_table(c, DC.swapped(c.bsdfs))
    acc_t, st_t, ref_t, cnt_t = check(c, "bre", monkeypatch, what=f"{scene} swapped", count=False)
    moved = l2(ref_t, ref, lum), l2(acc_t, acc.astype(np.float64), lum)
    print("film moved by", moved)
    assert moved[0] > TOL and moved[1] > TOL and abs(moved[0] - moved[1]) < 2 * TOL   # (each film within TOL of its statement)


# ---- the exact passes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", DC.SCENES)
def test_exact_all_bre(scene, monkeypatch):
    """GVPM_EXACT_ALL=1: every shift through the fp64 pass (exact_shift.hip), which evaluates this parent in fp32 as it does Ward
    and the conductor"""
    monkeypatch.setenv("GVPM_EXACT_ALL", "1")
    check(bre_case(scene), "bre", monkeypatch, what=f"exact {scene}", count=False)


@pytest.mark.parametrize("scene", DC.SCENES)
def test_beams_fp64_transcription(scene, monkeypatch):
    monkeypatch.setenv("GVPM_BEAMS_FP64", "1")
    check(beam_case(scene), "beams", monkeypatch, what=f"beams fp64 {scene}", count=False)


# ---- packed and linked uploads ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("linked", [False, True])
def test_packed_photons_end_to_end(linked, monkeypatch):
    """the entry index and the departure-side normal ride through the packed and the linked records (the normal octahedrally
    encoded: the statement runs on what the unpacker returns)"""
    c = bre_case("cbox_roughglass_rot")
    t = hip.MaterialTable()
    if linked:
        pk = hip.pack_photons_linked(c.ph, t)
        unp = hip.unpack_photons_linked(pk, t)
    else:
        pk = hip.pack_photons(c.ph, t)
        unp = hip.unpack_photons(pk, t)
    assert np.array_equal(unp.parent_g, c.ph.parent_g) and np.array_equal(unp.flags, c.ph.flags)
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ctx.upload_bsdfs(c.bsdfs)
    ctx.upload_materials(t)
    if linked:
        ctx.upload_photons_linked(pk)
    else:
        ctx.upload_photons_packed(pk)
    ctx.upload_camera_beams(c.rays)
    ctx.gather(1, c.nb)
    acc, st = ctx.download_accum().astype(np.float64), ctx.stats()
    ctx.close()
    D.install(monkeypatch)
    c.ph = unp
    ref, cnt, near = statement(c, "bre")
    agree(acc, st, ref, cnt, near, what=f"packed (linked {linked})")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(ctx, table, code):
    with pytest.raises(hip.GvpmError) as e:
        ctx.upload_bsdfs(np.ascontiguousarray(table))
    assert e.value.code == code, e.value


def test_malformed_entries_are_refused_and_leave_the_previous_table_in_force(monkeypatch):
    c = cases.make_case("cbox_roughglass", 20, 16, 6000, 4.0)
    good = c.bsdfs
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ctx.upload_bsdfs(good)
    INV, UNS = abi.GVPM_ERR_INVALID_ARG, abi.GVPM_ERR_UNSUPPORTED

    def bad(field, v, entry=1, lane=None):
        t = good.copy()
        if lane is None:
            t[field][entry] = v
        else:
            t[field][entry, lane] = v
        return t

    _refused(ctx, bad("exponent", 5e-5), INV)                              # alpha below 1e-4
    _refused(ctx, bad("exponent", np.nan), INV)
    for v in (np.nan, np.inf, -1.5, 0.0, 0.19, 5.01):                      # eta[0] not finite or outside [0.2, 5]
        _refused(ctx, bad("eta", v, lane=0), INV)
    for field in ("specular", "k"):                                        # a reflectance / transmittance channel outside [0, 1]
        for lane in (0, 1, 2):
            for v in (-0.01, 1.01, np.nan):
                _refused(ctx, bad(field, v, lane=lane), INV)
    for field, lane in (("eta", 1), ("eta", 2), ("specular_sampling_weight", None), ("reserved", 0), ("reserved", 1)):
        for v in (0.5, -0.0):                                              # a non-zero word where zero is asked
            _refused(ctx, bad(field, v, lane=lane), INV)
    for v in (2, -1):                                                      # the Phong distribution, nonsense
        _refused(ctx, bad("distribution", v), UNS)
        _refused(ctx, bad("distribution", v, entry=0), UNS)
    # legal: the ends of the ranges
    ctx.upload_bsdfs(bad("eta", 0.2, lane=0))
    ctx.upload_bsdfs(bad("eta", 5.0, lane=0))
    ctx.upload_bsdfs(bad("exponent", 1e-4))
    ctx.upload_bsdfs(good)
    _refused(ctx, bad("exponent", 0.0, entry=0), INV)
    # after all of that the good table is still the one the gather reads
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(c.rays)
    ctx.gather(1, c.nb)
    acc, st = ctx.download_accum(), ctx.stats()
    ctx.upload_bsdfs(good[:0])
    ctx.close()
    D.install(monkeypatch)
    ref, cnt, near = statement(c, "bre")
    agree(acc, st, ref, cnt, near, what="after refusals")


# ---- other kinds lit from behind -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("technique", ["bre", "beams"])
def test_a_record_of_another_kind_lit_from_behind_fails_as_before(technique):
    """every third glossy photon record (every second beam record) of cbox_conductor with its incident direction mirrored about
    the wall (cosWi < 0): the call sites no longer reject it before the table is read, the table's one-sided kinds do -- the
    frozen fp64 oracle's failed shift.  Beams: 3 000 of them, 130 turned (the 800 of the scenes' cases have 78 glossy records)."""
    c = bre_case("cbox_conductor") if technique == "bre" else make_beam_case("cbox_conductor", 12, 10, 3000, 5.0)
    rec, turned = DC.facing_away(getattr(c, RECORDS[technique]), 3 if technique == "bre" else 2)
    setattr(c, RECORDS[technique], rec)
    assert len(turned) > 100 and ((rec.parent_n[turned] * rec.parent_wi[turned]).sum(1) < 0).all()
    O.set_bsdfs(c.bsdfs)
    if technique == "bre":
        ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    else:
        ref, cnt, _ = O.gather_beams(c.p, c.m, c.tris, c.beams, c.end_n, c.rays, c.r, 1, c.nb, 64)
    acc, st = DEVICE[technique](c)
    agree(acc, st, ref, cnt, 0, tol=TOL_BEAMS if technique == "beams" else TOL, what=f"lit from behind {technique}")
