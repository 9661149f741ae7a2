"""Configuration flags CROSSED with every BSDF-parent kind, on the device (the CPU side: tests/test_flag_cross.py).  The flag
sweeps of the parity files run on Lambertian cbox and every parent kind was run under the default, use_mis = 0, power_heuristic = 1
and use_shift_null = 0 only; the filters of computeVolumeContribution (shift_device.h) read the record's parent-type, component
and depth bits, and a G-BRE handle under the default flags over a table runs the specialised evaluation kernel -- here they meet.

The kinds the fp64 oracle states (Phong, Phong one component at a time, rough conductor, Ward) are judged by it with the parity
helpers (test_parity_gpu.check, device_vpm, device_beams: counters exact, L2 < TOL = 1e-4, 2e-4 for G-Beams, the film included);
the kinds it does not state (rough and smooth plastic, anisotropic Ward and conductor, rough dielectric, a mixture, a
Phong-distribution conductor) by the numpy statement with each kind's own wrapper and `agree`, at the sizes of those files.

No case is vacuous: the judge's counters under the flags differ from its counters under the default flags on the same inputs
(printed side by side), more than 100 evaluations are left, and for the lighting modes the BSDF-parent records that pass the
statement's mask are counted from their flags: at least one under surf2media, none under media2media."""
import numpy as np
import pytest

import cases
import indep_aniso as A
import indep_dielectric as D
import indep_mixture as M
import indep_phong_dist as PD
import indep_plastic as P
import indep_statements as I
import oracle_lib as O
import plastic_cases as PC
import test_aniso_parents_gpu as TA
import test_dielectric_parents_gpu as TD
import test_mixture_parents_gpu as TM
import test_phong_dist_parents_gpu as TP
import test_plastic_parents_gpu as TPL
from gvpm_amd import abi
from test_flag_cross import FLAGS, FILTERS, SCENES, BRE_PHOTONS, VPM_PHOTONS, BEAMS, COUNTERS, flag_id, with_flags, not_vacuous, beams_with_sampled_components
from test_oracle_beams import make_beam_case
from test_oracle_vpm import make_vpm_case
from test_parity_beams_gpu import device_beams
from test_parity_gpu import check, device_gather, l2, TOL
from test_parity_vpm_gpu import device_vpm
from test_plastic_parents_gpu import run_vpm, run_beams, TOL_BEAMS

pytestmark = pytest.mark.gpu
S2M, M2M = abi.GVPM_SURF2MEDIA, abi.GVPM_MEDIA2MEDIA


def bsdf_parents_that_contribute(p, records):
    """BSDF-parent records that pass computeVolumeContribution, from their flags with the mask of the numpy statement
    (indep_statements.bre3d_full: parent type in bits 0-1, the parent's sampled component from bit 16)"""
    fl = records.flags
    ptype, comp = fl & 3, (fl >> 16) & 0xFFFF
    mode = p.lighting_interaction_mode
    contributes = np.ones(records.n, bool)
    if not ((mode & S2M) and (mode & M2M)):
        contributes &= np.where(ptype == abi.GVPM_PARENT_MEDIUM, bool(mode & M2M), bool(mode & S2M))
    if p.bsdf_interaction_mode != abi.GVPM_BSDF_ALL:
        contributes &= ~((comp > 0) & ((comp & p.bsdf_interaction_mode) == 0))
    return int((contributes & (ptype == abi.GVPM_PARENT_SURFACE_BSDF)).sum())


def the_lighting_mode_sorts_the_bsdf_parents(what, p, records):
    n = bsdf_parents_that_contribute(p, records)
    print(f"{what}: BSDF-parent records that contribute {n} of {int(((records.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF).sum())}")
    if p.lighting_interaction_mode == S2M:
        assert n >= 1, what
    if p.lighting_interaction_mode == M2M:
        assert n == 0, what


# ---- the kinds the oracle states -------------------------------------------------------------------------------------------
_default = {}


def oracle_default(key, make, gather):
    """the case under default flags and the oracle's counters on it, once per (technique, scene, size)"""
    if key not in _default:
        c = make()
        _default[key] = c, gather(c)
    c, cnt = _default[key]
    cases.use_bsdfs(c)
    return c, cnt


@pytest.mark.parametrize("kw", FLAGS, ids=flag_id)
@pytest.mark.parametrize("scene", SCENES)
def test_bre3d_flags_on_stated_kinds(scene, kw):
    """20 x 16 pixels, 20 000 photons, scale 4: under the default-like flag sets the specialised evaluation kernel with a BSDF
    table present, under the others the generic one"""
    nph = BRE_PHOTONS.get((scene, flag_id(kw)), 20000)
    c0, default = oracle_default(("bre", scene, nph), lambda: cases.make_case(scene, 20, 16, nph, 4.0),
                                 lambda c: O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)[1])
    c = with_flags(c0, kw)
    acc, ref, st = check(c)
    what = f"bre3d {scene} {flag_id(kw)}"
    print(f"{what}: L2 / lum {l2(acc, ref, max(ref[..., 0:3].mean(), 1e-30)):.3e}")
    not_vacuous(what, default, st)   # (check asserted the device's counters equal to the oracle's)
    the_lighting_mode_sorts_the_bsdf_parents(what, c.p, c.ph)


@pytest.mark.parametrize("kw", FILTERS, ids=flag_id)
@pytest.mark.parametrize("scene", SCENES)
def test_vpm_flags_on_stated_kinds(scene, kw):
    """12 x 10 pixels, 20 000 photons, scale 8, 6 camera samples"""
    nph = VPM_PHOTONS.get((scene, flag_id(kw)), 20000)
    c0, default = oracle_default(("vpm", scene, nph), lambda: make_vpm_case(scene, 12, 10, nph, 8.0, 6),
                                 lambda c: O.gather_vpm(c.p, c.m, c.tris, c.ph, c.rays, c.samples, 64, use_accel=False)[3])
    c = with_flags(c0, kw)
    acc, ref, st = device_vpm(c)
    what = f"vpm {scene} {flag_id(kw)}"
    print(f"{what}: L2 / lum {l2(acc, ref, max(ref[..., 0:3].mean(), 1e-30)):.3e}")
    not_vacuous(what, default, st)
    the_lighting_mode_sorts_the_bsdf_parents(what, c.p, c.ph)


@pytest.mark.parametrize("kw", FILTERS, ids=flag_id)
@pytest.mark.parametrize("scene", SCENES)
def test_beams3d_flags_on_stated_kinds(scene, kw):
    """12 x 10 pixels, 2 400 beams, scale 5 (glossy only: the beams of test_flag_cross.BEAMS, with the components it gives them)"""
    nbeams = BEAMS.get((scene, flag_id(kw)), 2400)
    c0, default = oracle_default(("beams", scene, nbeams), lambda: beams_with_sampled_components(make_beam_case(scene, 12, 10, nbeams, 5.0)),
                                 lambda c: O.gather_beams(c.p, c.m, c.tris, c.beams, c.end_n, c.rays, c.r, 1, c.nb, 64)[1])
    c = with_flags(c0, kw)
    acc, ref, st = device_beams(c)
    what = f"beams3d {scene} {flag_id(kw)}"
    print(f"{what}: L2 / lum {l2(acc, ref, max(ref[..., 0:3].mean(), 1e-30)):.3e}")
    not_vacuous(what, default, st)
    the_lighting_mode_sorts_the_bsdf_parents(what, c.p, c.beams)


# ---- the kinds the oracle does not state: the numpy statement with the kind's wrapper --------------------------------------
def _plastic_statement(c, technique):
    """(film, counters, 0): the plastic kinds add no fp32 decision the statement would have to count (test_plastic_parents_gpu)"""
    return {"bre": I.bre3d_full, "vpm": I.vpm_full, "beams": I.beams_full}[technique](c)[:2] + (0,)


def _plastic_agree(acc, st, ref, cnt, near, tol, what):
    return TPL.agree(acc, st, ref, cnt, tol=tol, what=what)


def _agree(module):
    return lambda acc, st, ref, cnt, near, tol, what: module.agree(acc, st, ref, cnt, near, tol=tol, what=what)


class Kind:
    def __init__(self, scene, install, statement, agree, bre, vpm, beams):
        self.scene, self.install, self.statement, self.agree = scene, install, statement, agree
        self.make = {"bre": bre, "vpm": vpm, "beams": beams}


def _plastic(scene):
    return Kind(scene, P.install, _plastic_statement, _plastic_agree, lambda s, nph=20000: PC.make_case(s, 20, 16, nph, 4.0),
                lambda s: PC.make_vpm_case(s, 12, 10, 20000, 8.0, 6), lambda s: PC.make_beam_case(s, 12, 10, 2400, 5.0))


# (one scene per kind, with the case builders -- and so the sizes -- of the kind's own file)
KINDS = {
    "rough plastic": _plastic("cbox_roughplastic"),
    "smooth plastic": _plastic("cbox_plastic"),
    "anisotropic Ward": Kind("cbox_ward_aniso", A.install, TA.statement, _agree(TA), TA.bre_case, TA.vpm_case, TA.beam_case),
    "anisotropic conductor": Kind("cbox_conductor_aniso", A.install, TA.statement, _agree(TA), TA.bre_case, TA.vpm_case, TA.beam_case),
    "rough dielectric": Kind("cbox_roughglass", D.install, TD.statement, _agree(TD), TD.bre_case, TD.vpm_case,
                             # (media to media leaves 78 evaluations of the 800 beams of the kind's own file: twice the beams)
                             lambda s: make_beam_case(s, 12, 10, 1600, 5.0)),
    "mixture": Kind("cbox_mixture", M.install, TM.statement, _agree(TD), TM.bre_case, TM.vpm_case, TM.beam_case),
    "Phong-distribution conductor": Kind("cbox_conductor_phong", PD.install, TP.statement, _agree(TD), TP.bre_case, TP.vpm_case, TP.beam_case),
}
# glossy only keeps the photons whose parent sampled its glossy lobe; behind the plastic walls 20 000 photons leave
# 34 (rough) and 35 (smooth) evaluations, 80 000 leave 121 and 123 (the statement's time goes with the evaluations)
PHOTONS = {("rough plastic", "bsdf_interaction_mode=0x8"): 80000, ("smooth plastic", "bsdf_interaction_mode=0x8"): 80000}
DEVICE = {"bre": lambda c: device_gather(c)[:2], "vpm": run_vpm, "beams": run_beams}
RECORDS = {"bre": "ph", "vpm": "ph", "beams": "beams"}
_stated_by_numpy = {}


def flagged_against_the_statement(kind, technique, kw, monkeypatch):
    k = KINDS[kind]
    k.install(monkeypatch)
    nph = PHOTONS.get((kind, flag_id(kw))) if technique == "bre" else None
    if (kind, technique, nph) not in _stated_by_numpy:
        c0 = k.make[technique](k.scene, nph) if nph else k.make[technique](k.scene)
        _stated_by_numpy[kind, technique, nph] = c0, k.statement(c0, technique)[1]
    c0, default = _stated_by_numpy[kind, technique, nph]
    O.set_bsdfs(c0.bsdfs)
    I.set_bsdfs(c0.bsdfs)
    c = with_flags(c0, kw)
    records = getattr(c, RECORDS[technique])
    assert ((records.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF).sum() > 30
    ref, cnt, near = k.statement(c, technique)
    acc, st = DEVICE[technique](c)
    what = f"{technique} {kind} ({k.scene}) {flag_id(kw)}"
    k.agree(acc, st, ref, cnt, near, TOL_BEAMS if technique == "beams" else TOL, what)
    not_vacuous(what, default, cnt)
    the_lighting_mode_sorts_the_bsdf_parents(what, c.p, records)


@pytest.mark.parametrize("kw", FILTERS + [dict(max_depth=3)], ids=flag_id)
@pytest.mark.parametrize("kind", list(KINDS))
def test_bre3d_flags_on_kinds_the_oracle_does_not_state(kind, kw, monkeypatch):
    """the three filters that read the record's parent-type, component and depth bits; 20 x 16 pixels, 20 000 photons, scale 4"""
    flagged_against_the_statement(kind, "bre", kw, monkeypatch)


@pytest.mark.parametrize("kind", list(KINDS))
def test_vpm_media2media_on_kinds_the_oracle_does_not_state(kind, monkeypatch):
    flagged_against_the_statement(kind, "vpm", dict(lighting_interaction_mode=M2M), monkeypatch)


@pytest.mark.parametrize("kind", list(KINDS))
def test_beams3d_media2media_on_kinds_the_oracle_does_not_state(kind, monkeypatch):
    flagged_against_the_statement(kind, "beams", dict(lighting_interaction_mode=M2M), monkeypatch)
