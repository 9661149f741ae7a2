"""Configuration flags CROSSED with BSDF parents, on the CPU: the oracle against the independent numpy statement
(tests/indep_statements.py) for the four glossy scenes the oracle states, under the flag sets that filter or re-route
photons by what their record says of the parent (parent type, sampled component, depth) or change which shift they take.
Every flag was swept on Lambertian cbox only and every BSDF-parent kind under four flag sets only; the crossing found
computeVolumeContribution letting GVPM_PARENT_SURFACE_BSDF photons through lightingInteractionMode = media2media
(shift_utilities.h:241-247 drops every isSurfaceInteraction() parent).

The bar is test_indep_statements.compare's: the four counters equal, each of the nine accumulator groups within 1e-9 of
the mean luminance.  No case is vacuous: the flagged run's counters differ from the default-flag run of the same inputs
(printed side by side) and it keeps more than 100 evaluations."""
import numpy as np
import pytest

import cases
import indep_statements as I
import oracle_lib as O
from gvpm_amd import abi
from test_indep_statements import compare, compare_beams
from test_oracle_beams import make_beam_case, TECHS
from test_oracle_vpm import make_vpm_case

SCENES = ["cbox_phong", "cbox_phong1", "cbox_conductor", "cbox_ward"]
FLAGS = [
    dict(lighting_interaction_mode=abi.GVPM_SURF2MEDIA),
    dict(lighting_interaction_mode=abi.GVPM_MEDIA2MEDIA),
    dict(bsdf_interaction_mode=0x8),
    dict(bsdf_interaction_mode=0x2),
    dict(max_depth=3),
    dict(path_set=0),
    dict(visibility_as_written=0),
    dict(debug_shift=abi.GVPM_SHIFT_NULL),
    dict(lighting_interaction_mode=abi.GVPM_MEDIA2MEDIA, use_mis=0),
    dict(bsdf_interaction_mode=0x8, use_shift_null=0),
]
# the three that read the record's parent-type and component bits: what G-VPM and G-Beams are crossed with
FILTERS = FLAGS[:3]
COUNTERS = ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts")


def flag_id(kw):
    return "-".join(f"{k}={v:#x}" if k.endswith("_mode") else f"{k}={v}" for k, v in kw.items())


def with_flags(c, kw):
    """the same inputs under other flags (the flags live in the parameter block only)"""
    f = cases.Case()
    f.__dict__.update(c.__dict__)
    f.p = c.p.copy()
    for k, v in kw.items():
        setattr(f.p, k, v)
    return f


def not_vacuous(what, default, flagged):
    """the flag set changed what was evaluated or how it was shifted, and left enough to compare"""
    d, f = [default[k] for k in COUNTERS], [flagged[k] for k in COUNTERS]
    print(f"{what}: default {dict(zip(COUNTERS, d))} flagged {dict(zip(COUNTERS, f))}")
    assert d != f, (what, d)
    assert flagged["evaluations"] > 100, (what, f)


# ---- G-BRE 3D ----------------------------------------------------------------------------------------------------------
# bsdfInteractionMode = glossy keeps the photons whose parent sampled its glossy lobe, a few per cent of a Phong or Ward map:
# the larger map where 20 000 photons leave 100 evaluations or fewer
BRE_PHOTONS = {}
_bre = {}


def bre_case(scene, nph):
    if (scene, nph) not in _bre:
        c = cases.make_case(scene, 20, 16, nph, 4.0)
        _, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, 1, c.nb, 64, use_accel=False)
        _bre[scene, nph] = c, cnt
    c, cnt = _bre[scene, nph]
    O.set_bsdfs(c.bsdfs)
    I.set_bsdfs(c.bsdfs)
    return c, cnt


@pytest.mark.parametrize("kw", FLAGS, ids=flag_id)
@pytest.mark.parametrize("scene", SCENES)
def test_bre3d_flags_on_bsdf_parents(scene, kw):
    c, default = bre_case(scene, BRE_PHOTONS.get((scene, flag_id(kw)), 20000))
    assert ((c.ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF).sum() > 500
    cnt = compare(with_flags(c, kw))
    not_vacuous(f"bre3d {scene} {flag_id(kw)}", default, cnt)


# ---- G-VPM -------------------------------------------------------------------------------------------------------------
VPM_PHOTONS = {}
_vpm = {}


def vpm_case(scene, nph):
    if (scene, nph) not in _vpm:
        c = make_vpm_case(scene, 12, 10, nph, 8.0, 6)
        cnt = O.gather_vpm(c.p, c.m, c.tris, c.ph, c.rays, c.samples, 64, use_accel=True)[3]
        _vpm[scene, nph] = c, cnt
    c, cnt = _vpm[scene, nph]
    O.set_bsdfs(c.bsdfs)
    I.set_bsdfs(c.bsdfs)
    return c, cnt


@pytest.mark.parametrize("kw", FILTERS, ids=flag_id)
@pytest.mark.parametrize("scene", ["cbox_phong", "cbox_conductor"])
def test_vpm_flags_on_bsdf_parents(scene, kw):
    c0, default = vpm_case(scene, VPM_PHOTONS.get((scene, flag_id(kw)), 20000))
    c = with_flags(c0, kw)
    ref, rsv, rnv, cnt, _ = O.gather_vpm(c.p, c.m, c.tris, c.ph, c.rays, c.samples, 64, use_accel=True)
    acc, icnt, mvol = I.vpm_full(c)
    for k in COUNTERS:
        assert icnt[k] == cnt[k], (k, icnt, cnt)
    lum = ref[..., 0:3].mean()
    for j in range(9):
        assert np.abs(acc[..., 3 * j:3 * j + 3] - ref[..., 3 * j:3 * j + 3]).max() / lum < 1e-9, j
    # the SPPM update counts every photon in the radius, filtered or not (gvpm.cpp:1191-1195)
    N = mvol * c.p.alpha
    with np.errstate(invalid="ignore", divide="ignore"):
        sv = np.where(mvol > 0, c.p.initial_scale_volume * np.cbrt((c.p.alpha * mvol) / mvol), c.p.initial_scale_volume)
    assert np.allclose(rnv, N, rtol=1e-12) and np.allclose(rsv, sv, rtol=1e-12)
    not_vacuous(f"vpm {scene} {flag_id(kw)}", default, cnt)


# ---- G-Beams -----------------------------------------------------------------------------------------------------------
def beams_with_sampled_components(c):
    """The synthetic host labels EVERY beam's parent component EDiffuseReflection (synth_core.h, the beam records), also the beams
    that leave a glossy wall, whose photons it labels with the lobe that was sampled: under bsdfInteractionMode = glossy no beam of
    any scene is left, however many are shot.  What the filter reads is the record's bits, so the BSDF-parent beams are re-labelled
    here with a component their table entry can have been sampled through: EGlossyReflection for a rough conductor and for a
    one-component Phong entry of the specular lobe, EDiffuseReflection for one of the diffuse lobe, and for the entries that hold
    both lobes (Phong, Ward) one of the two by a bit of the path id that is not the path set's parity bit."""
    fl = c.beams.flags
    gl = (fl & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    entry = c.bsdfs[c.beams.parent_g[gl].astype(np.int64)]
    two_lobes = np.isin(entry["kind"], (abi.GVPM_BSDF_PHONG, abi.GVPM_BSDF_WARD))
    one_of_phong = (entry["kind"] == abi.GVPM_BSDF_PHONG) & (entry["distribution"] != 0)
    diffuse = np.where(one_of_phong, entry["distribution"] == 2, two_lobes & (((c.beams.path_id[gl] >> 1) & 1) == 0))
    fl[gl] = (fl[gl] & np.uint32(0xFFFF)) | (np.where(diffuse, 0x2, 0x8).astype(np.uint32) << 16)
    return c


# (glossy only: the re-labelled glossy-lobe beams of two walls are a few per cent of the beams; measured with 2 400 beams 41 to
# 69 evaluations on cbox_phong, cbox_phong1 and cbox_ward and 129 / 133 on cbox_conductor; with 8 000 beams 144 to 196)
BEAMS = {(s, "bsdf_interaction_mode=0x8"): 8000 for s in ("cbox_phong", "cbox_phong1", "cbox_ward")}
_beams = {}


def beam_case(scene, tech, nbeams):
    if (scene, tech, nbeams) not in _beams:
        c = beams_with_sampled_components(make_beam_case(scene, 12, 10, nbeams, 5.0, technique=tech))
        _, cnt, _ = O.gather_beams(c.p, c.m, c.tris, c.beams, c.end_n, c.rays, c.r, 1, c.nb, 64)
        _beams[scene, tech, nbeams] = c, cnt
    c, cnt = _beams[scene, tech, nbeams]
    O.set_bsdfs(c.bsdfs)
    I.set_bsdfs(c.bsdfs)
    return c, cnt


@pytest.mark.parametrize("kw", FILTERS, ids=flag_id)
@pytest.mark.parametrize("tech", TECHS)
@pytest.mark.parametrize("scene", ["cbox_phong", "cbox_conductor"])
def test_beams_flags_on_bsdf_parents(scene, tech, kw):
    c, default = beam_case(scene, tech, BEAMS.get((scene, flag_id(kw)), 2400))
    assert ((c.beams.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF).sum() > 30
    cnt = compare_beams(with_flags(c, kw))
    not_vacuous(f"beams {tech} {scene} {flag_id(kw)}", default, cnt)
