"""Plastic surface parents on the device (GVPM_BSDF_ROUGHPLASTIC, GVPM_BSDF_PLASTIC; parent_bsdf.h glossyParentEval): the
gathers of every technique that reconnects against the numpy statement of tests/indep_plastic.py (the frozen fp64 oracle
has no plastic: it fails these shifts), the two limits in which the oracle does state them, the exact passes, the packed and
linked uploads, and what gvpm_upload_bsdfs refuses."""
import numpy as np
import pytest

import cases
import indep_plastic as P
import indep_statements as I
import oracle_lib as O
import plastic_cases as PC
from gvpm_amd import abi, hip
from test_oracle_beams import make_beam_case, TECHS
from test_oracle_vpm import make_vpm_case
from test_parity_gpu import device_gather, l2, TOL

pytestmark = pytest.mark.gpu
SHIFTS = ("null_shifts", "diffuse_shifts", "failed_shifts")
TOL_BEAMS = 2e-4  # (the G-Beams bar)


def run_vpm(c):
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    cases.upload_bsdfs(ctx, c)
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(c.rays)
    ctx.upload_vpm_samples(c.samples)
    ctx.gather(1, c.nb)
    acc, st = ctx.download_accum(), ctx.stats()
    ctx.close()
    return acc, st


def run_beams(c):
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    cases.upload_bsdfs(ctx, c)
    assert abs(ctx.radius() - c.r) == 0.0
    ctx.upload_beams(c.beams, c.end_n)
    ctx.upload_camera_beams(c.rays)
    ctx.gather(1, c.nb)
    acc, st = ctx.download_accum(), ctx.stats()
    ctx.close()
    return acc, st


def agree(acc, st, ref, cnt, tol=TOL, what=""):
    lum = max(ref[..., 0:3].mean(), 1e-30)
    err = l2(acc, ref, lum)
    print(f"{what}: evaluations {st['evaluations']} / {cnt['evaluations']}, shifts "
          + ", ".join(f"{k} {st[k]} / {cnt[k]}" for k in SHIFTS) + f", L2 / lum {err:.3e}")
    assert st["evaluations"] == cnt["evaluations"], (st, cnt)
    for k in SHIFTS:
        assert st[k] == cnt[k], (k, st, cnt)
    assert err < tol, err
    return err


def oracle_diffuse_shifts(c, technique):
    """the frozen oracle on the same inputs: it does not know the plastic kinds and fails those shifts"""
    O.set_bsdfs(c.bsdfs)
    if technique == "bre":
        _, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
    elif technique == "vpm":
        _, _, _, cnt, _ = O.gather_vpm(c.p, c.m, c.tris, c.ph, c.rays, c.samples, 64, use_accel=True)
    else:
        _, cnt, _ = O.gather_beams(c.p, c.m, c.tris, c.beams, c.end_n, c.rays, c.r, 1, c.nb, 64)
    return cnt["diffuse_shifts"]


# ---- the three scenes: device against the numpy statement ----------------------------------------------------------------------
def through_plastic(c, st, cnt, technique):
    """Reconnections through plastic parents, counted from the photons' flags and the statement: the records of parent type
    GVPM_PARENT_SURFACE_BSDF all name plastic heads here (asserted), so the statement run once more WITHOUT the table fails
    exactly their shifts, and the difference of its diffuse shifts is the count.  (To be called with the wrapper installed.)
    Beside it the feature itself: the device reconnects more shifts than the frozen oracle does on the same inputs."""
    records = c.beams if technique == "beams" else c.ph
    gl = (records.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    heads = P.heads_of(c.bsdfs)
    idx = records.parent_g[gl].astype(np.int64)
    assert gl.any() and heads[idx].all() and np.isin(c.bsdfs["kind"][idx], (abi.GVPM_BSDF_ROUGHPLASTIC, abi.GVPM_BSDF_PLASTIC)).all()
    table = c.bsdfs
    I.set_bsdfs(table[:0])
    try:
        none = {"bre": lambda: I.bre3d_full(c)[1], "vpm": lambda: I.vpm_full(c)[1], "beams": lambda: I.beams_full(c)[1]}[technique]()
    finally:
        I.set_bsdfs(table)
    n = cnt["diffuse_shifts"] - none["diffuse_shifts"]
    assert n == none["failed_shifts"] - cnt["failed_shifts"]
    assert st["diffuse_shifts"] > oracle_diffuse_shifts(c, technique)
    print("reconnections through plastic parents:", n)
    return n


@pytest.mark.parametrize("kw", [dict(), dict(use_mis=0), dict(power_heuristic=1), dict(use_shift_null=0)])
@pytest.mark.parametrize("rot", ["", "_rot"])
@pytest.mark.parametrize("scene", ["cbox_roughplastic", "cbox_roughplastic1", "cbox_plastic"])
def test_bre3d_matches_the_numpy_statement(scene, rot, kw, monkeypatch):
    """20 x 16 pixels, 20 000 photons, scale 4: the statement runs 5 - 10 s here.  Measured with these sizes (default flags):
    cbox_roughplastic 7 728 evaluations, 1 558 reconnections through plastic parents; _rot 19 451 / 3 022; cbox_plastic 7 782 /
    1 595 (counts of the statement and the oracle; the device must reproduce them).  Shift counters are asserted EQUAL to the
    fp64 statement's: the only fp32 decision these kinds add is the conductor's `D == 0`."""
    c = PC.make_case(scene + rot, 20, 16, 20000, 4.0, **kw)
    P.install(monkeypatch)
    ref, cnt = I.bre3d_full(c)
    acc, st, _ = device_gather(c)
    agree(acc, st, ref, cnt, what=f"{scene}{rot} {kw}")
    assert through_plastic(c, st, cnt, "bre") > 300


@pytest.mark.parametrize("scene", ["cbox_roughplastic", "cbox_plastic_rot", "cbox_roughplastic1_rot"])
def test_vpm_matches_the_numpy_statement(scene, monkeypatch):
    """12 x 10 pixels, 20 000 photons, scale 8, 6 camera samples (statement: 9 s); cbox_roughplastic: 13 203 evaluations,
    1 937 reconnections through plastic parents"""
    c = PC.make_vpm_case(scene, 12, 10, 20000, 8.0, 6)
    P.install(monkeypatch)
    ref, cnt, _ = I.vpm_full(c)
    acc, st = run_vpm(c)
    agree(acc, st, ref, cnt, what=f"vpm {scene}")
    assert through_plastic(c, st, cnt, "vpm") > 300


@pytest.mark.parametrize("tech", TECHS)
@pytest.mark.parametrize("scene", ["cbox_roughplastic", "cbox_plastic_rot", "cbox_roughplastic1_rot"])
def test_beams_match_the_numpy_statement(tech, scene, monkeypatch):
    """12 x 10 pixels, 2 400 beams, scale 5 (statement: 12 s; at 1 500 beams cbox_roughplastic had 274 / 264 reconnections through
    plastic parents for the 3D / 1D kernel: under the 300 asked for)"""
    c = PC.make_beam_case(scene, 12, 10, 2400, 5.0, technique=tech)
    P.install(monkeypatch)
    ref, cnt = I.beams_full(c)
    acc, st = run_beams(c)
    agree(acc, st, ref, cnt, tol=TOL_BEAMS, what=f"beams {tech} {scene}")
    assert through_plastic(c, st, cnt, "beams") > 300


# ---- relabelled records: the table's other switches -----------------------------------------------------------------------------
# (what a reconnection evaluates is a function of the record and the table: the records of cbox_phong / cbox_phong1 -- two walls
# with a diffuse reflectance -- under plastic entries the host scenes do not have: visible-normal pdf, other weights)
@pytest.mark.parametrize("scene,which", [("cbox_phong", "rough"), ("cbox_phong1_rot", "rough1")])
def test_relabelled_bre3d_matches_the_numpy_statement(scene, which, monkeypatch):
    c = PC.relabelled_case(cases.make_case(scene, 20, 16, 20000, 4.0), which)
    assert (c.bsdfs["sample_visible"][P.heads_of(c.bsdfs)] != 0).any() or which == "rough1"
    P.install(monkeypatch)
    ref, cnt = I.bre3d_full(c)
    acc, st, _ = device_gather(c)
    agree(acc, st, ref, cnt, what=f"relabelled {scene} {which}")
    assert through_plastic(c, st, cnt, "bre") > 300


# ---- the limits, against the fp64 oracle at the sizes of the parity tests ------------------------------------------------------
def _limit_case(limit, make, records="ph"):
    """(case for the device, case for the oracle): limit 1 / 4 and 1 / 5 -- a plain cbox, its Lambertian parents re-labelled to
    a plastic entry with eta = 1, Fdr = 0, T = 1 (rough, smooth); limit 2 -- cbox_conductor with k = 0 against the glossy component
    alone with T = 0"""
    if limit == 2:
        o = make("cbox_conductor")
        cond, plastic, mapping = PC.limit2_tables(o.bsdfs)
        d = make("cbox_conductor")
        setattr(d, records, PC.relabelled(getattr(d, records), mapping))
        PC.use_table(d, plastic)
        O.set_bsdfs(cond)
        return d, o
    o = make("cbox")
    d = make("cbox")
    setattr(d, records, PC.relabelled(getattr(d, records), None, lambertian_to=0))
    PC.use_table(d, PC.limit1_table(limit))
    O.set_bsdfs(o.bsdfs)
    return d, o


LIMITS = [abi.GVPM_BSDF_ROUGHPLASTIC, abi.GVPM_BSDF_PLASTIC, 2]


@pytest.mark.parametrize("kw", [dict(), dict(vol_technique=abi.GVPM_VOL_BRE2D, use_shift_null=0), dict(use_mis=0), dict(power_heuristic=1)])
@pytest.mark.parametrize("limit", LIMITS)
def test_limits_bre_match_fp64_oracle(limit, kw):
    d, o = _limit_case(limit, lambda s: cases.make_case(s, 40, 36, 30000, 2.5, **kw))
    assert ((d.ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF).sum() > 1000
    ref, cnt, _ = O.gather_bre(o.p, o.m, o.tris, o.ph, o.rays, o.r, 1, o.nb, 64, use_accel=False)
    acc, st, _ = device_gather(d)
    agree(acc, st, ref, cnt, what=f"limit {limit} {kw}")
    assert st["evaluations"] > 10000 and st["diffuse_shifts"] > 10000


@pytest.mark.parametrize("limit", LIMITS)
def test_limits_vpm_match_fp64_oracle(limit):
    d, o = _limit_case(limit, lambda s: make_vpm_case(s, 32, 28, 40000, 5.0, nb=10))
    ref, _, _, cnt, _ = O.gather_vpm(o.p, o.m, o.tris, o.ph, o.rays, o.samples, 64, use_accel=False)
    acc, st = run_vpm(d)
    agree(acc, st, ref, cnt, what=f"vpm limit {limit}")
    assert st["evaluations"] > 5000 and st["diffuse_shifts"] > 2000


@pytest.mark.parametrize("limit", LIMITS)
def test_limits_beams3d_match_fp64_oracle(limit):
    d, o = _limit_case(limit, lambda s: make_beam_case(s, 32, 28, 12000, 2.5), records="beams")
    ref, cnt, _ = O.gather_beams(o.p, o.m, o.tris, o.beams, o.end_n, o.rays, o.r, 1, o.nb, 64)
    acc, st = run_beams(d)
    agree(acc, st, ref, cnt, tol=TOL_BEAMS, what=f"beams limit {limit}")
    assert st["evaluations"] > 20000 and st["diffuse_shifts"] > 5000


# ---- the exact passes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cbox_roughplastic", "cbox_plastic_rot"])
def test_exact_all_bre(scene, monkeypatch):
    """GVPM_EXACT_ALL=1: every shift through the fp64 pass (exact_shift.hip), which evaluates these parents in fp32 as it does
    Ward and the conductor"""
    c = PC.make_case(scene, 20, 16, 20000, 4.0)
    P.install(monkeypatch)
    ref, cnt = I.bre3d_full(c)
    monkeypatch.setenv("GVPM_EXACT_ALL", "1")
    acc, st, _ = device_gather(c)
    agree(acc, st, ref, cnt, what=f"exact {scene}")
    assert through_plastic(c, st, cnt, "bre") > 300


def test_beams_fp64_transcription(monkeypatch):
    c = PC.make_beam_case("cbox_roughplastic", 12, 10, 2400, 5.0)
    P.install(monkeypatch)
    ref, cnt = I.beams_full(c)
    monkeypatch.setenv("GVPM_BEAMS_FP64", "1")
    acc, st = run_beams(c)
    agree(acc, st, ref, cnt, tol=TOL_BEAMS, what="beams fp64")
    assert through_plastic(c, st, cnt, "beams") > 300


# ---- packed and linked uploads ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("linked", [False, True])
def test_packed_photons_carry_the_head_index(linked, monkeypatch):
    """the head index (0 and 8 here) rides through the material table like any parent_g"""
    c = PC.make_case("cbox_roughplastic", 20, 16, 20000, 4.0)
    t = hip.MaterialTable()
    if linked:
        pk = hip.pack_photons_linked(c.ph, t)
        unp = hip.unpack_photons_linked(pk, t)
    else:
        pk = hip.pack_photons(c.ph, t)
        unp = hip.unpack_photons(pk, t)
    assert np.array_equal(unp.parent_g, c.ph.parent_g) and np.array_equal(unp.flags, c.ph.flags)
    assert set(np.unique(unp.parent_g[(unp.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF])) == {0.0, float(PC.E)}
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
    P.install(monkeypatch)
    c.ph = unp
    ref, cnt = I.bre3d_full(c)
    agree(acc, st, ref, cnt, what=f"packed (linked {linked})")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(ctx, table, code):
    with pytest.raises(hip.GvpmError) as e:
        ctx.upload_bsdfs(np.ascontiguousarray(table))
    assert e.value.code == code, e.value


def test_malformed_tables_are_refused_and_leave_the_previous_one_in_force(monkeypatch):
    c = PC.make_case("cbox_roughplastic", 20, 16, 6000, 4.0)
    good = c.bsdfs
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ctx.upload_bsdfs(good)
    INV, UNS = abi.GVPM_ERR_INVALID_ARG, abi.GVPM_ERR_UNSUPPORTED
    _refused(ctx, good[:PC.E + 1], INV)                      # the second head without its slice
    _refused(ctx, good[:2 * PC.E - 1], INV)                  # ... with a part of it
    for v in (1.5, np.nan, -0.25, np.inf, 1e-40):            # (1e-40: subnormal)
        bad = good.copy()
        bad.view(np.float32).reshape(-1, 16)[PC.E + 3, 5] = v
        _refused(ctx, bad, INV)
    bad = good.copy()
    bad.view(np.float32).reshape(-1, 16)[7, 9] = 0.5         # behind the 100 values: zero words
    _refused(ctx, bad, INV)
    for field, col, v in (("eta", 0, 0.9), ("eta", 0, np.inf), ("eta", 1, 1.0), ("eta", 1, -0.1), ("k", 0, 3.0), ("k", 0, 0.5), ("k", 1, 2.0)):
        bad = good.copy()
        bad[field][0, col] = v
        _refused(ctx, bad, INV)
    for field, v in (("exponent", 5e-5), ("specular_sampling_weight", 1.5)):
        bad = good.copy()
        bad[field][0] = v
        _refused(ctx, bad, INV)
    bad = good.copy()
    bad["distribution"][0] = 2
    _refused(ctx, bad, UNS)
    bad = good.copy()
    bad["kind"][0] = 7
    _refused(ctx, bad, UNS)
    _refused(ctx, good[1:], UNS)                             # raw entries without their head: no kind
    smooth, _ = PC.plastic_tables("smooth")
    for comp in (0.0, 1.0):
        bad = smooth.copy()
        bad["k"][1, 0] = comp
        _refused(ctx, bad, INV)
    bad = smooth.copy()
    bad["eta"][0, 0] = 0.5
    _refused(ctx, bad, INV)
    # after all of that the good table is still the one the gather reads
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(c.rays)
    ctx.gather(1, c.nb)
    acc, st = ctx.download_accum(), ctx.stats()
    ctx.upload_bsdfs(smooth)
    ctx.upload_bsdfs(good[:0])
    ctx.close()
    P.install(monkeypatch)
    ref, cnt = I.bre3d_full(c)
    agree(acc, st, ref, cnt, what="after refusals")


def test_a_photon_that_names_a_raw_entry_fails_its_shift(monkeypatch):
    c = PC.make_case("cbox_roughplastic", 20, 16, 6000, 4.0)
    gl = (c.ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    c.ph.parent_g[gl] += np.where(c.ph.parent_g[gl] == 0, 3, 7).astype(np.float32)   # entries 3 and 15: inside the two slices
    P.install(monkeypatch)
    ref, cnt = I.bre3d_full(c)
    acc, st, _ = device_gather(c)
    agree(acc, st, ref, cnt, what="raw entries")
    assert st["diffuse_shifts"] == oracle_diffuse_shifts(c, "bre")


# ---- the component matters -----------------------------------------------------------------------------------------------------
def test_the_sampled_component_matters(monkeypatch):
    """cbox_roughplastic1's photons name the entry of the component their parent was sampled through; with those entries
    re-labelled to "both components" eval and pdf differ: the statement's film moves beyond the parity bar and the device's
    with it"""
    c = PC.make_case("cbox_roughplastic1", 20, 16, 20000, 4.0)
    P.install(monkeypatch)
    ref, cnt = I.bre3d_full(c)
    acc, st, _ = device_gather(c)
    agree(acc, st, ref, cnt, what="one component")
    lum = ref[..., 0:3].mean()
    both = c.bsdfs.copy()
    both["k"][np.flatnonzero(both["kind"] == abi.GVPM_BSDF_ROUGHPLASTIC), 0] = 0
    PC.use_table(c, both)
    ref_b, cnt_b = I.bre3d_full(c)
    acc_b, st_b, _ = device_gather(c)
    agree(acc_b, st_b, ref_b, cnt_b, what="both components")
    print("film moved by", l2(ref_b, ref, lum), l2(acc_b, acc.astype(np.float64), lum))
    assert l2(ref_b, ref, lum) > TOL and l2(acc_b, acc.astype(np.float64), lum) > TOL
