"""The one table of inputs for the per-entry parity bars (tests/entry_parity.py), shared by the CPU admission / mutation tests
(test_entry_parity.py) and the device tests (test_entry_parity_gpu.py).

A case is ADMITTED when, with the oracle alone: it has at least 1 000 evaluations; the strict fp32 oracle's counters all equal the
fp64 oracle's (no shift flips: the tail bar T is a rounding figure, not a discrete event); max(rho_ref) <= 2e-4, hence T <= 1.6e-3;
and at most 1 % of the non-zero entries are tiny.  test_entry_parity.test_admission asserts it for every case below.

Sizes.  G-BRE: make_case(scene, 24, 20, 8000, 3.0).  G-Beams: make_beam_case(scene, 16, 12, 3000, 3.0).  G-VPM: 20 x 16, 6 000 photons,
scale 6, 4 camera samples, the inputs of iteration 2 (iteration 1's fail admission: the fp32 oracle takes another shift, max(rho_ref)
1.3e-2 at 20 000 photons).  G-Planes: cbox_in 16 x 12, 500 planes, the inputs of iteration 2 (2 000 planes of iteration 1: max(rho_ref)
4.3e-3).  Values that had to move from these for admission are written at the case.

BSDF-parent families.  The frozen oracle states Phong, the isotropic rough conductor and Ward; their scenes are used as they are.
It does not know the plastics, the anisotropic kinds, the rough dielectric or mixtures (it fails those shifts), so for these the
device runs the family's entries in the LIMIT in which they equal a kind the oracle states -- the tables of plastic_cases.py,
aniso_cases.py, dielectric_cases.py and mixture_cases.py, as the *_parents_gpu.py tests use them against the global bar -- over the
same records, re-labelled to name the family's heads.  The yardstick is then the oracle's fp32 noise on the kind the limit equals.
The Phong microfacet distribution has no such limit (the oracle reads a non-GGX conductor as Beckmann): there is no fp32 reference
for it and it has no case here.

A prepared case carries: c (the oracle's inputs), tech, dev_records / dev_table (what the device is given; the same objects unless
the case is a limit), r64 / cnt64, r32 / cnt32 (strict fp32), rfast (the -ffast-math fp32 build), lum, and for G-VPM the fp64
per-pixel state sv / nv."""
import numpy as np

import aniso_cases as AC
import cases
import dielectric_cases as DC
import medium_cases
import mixture_cases as MC
import oracle_lib as O
import plastic_cases as PC
from entry_parity import luminance
from gvpm_amd import abi
from test_oracle_beams import make_beam_case
from test_oracle_planes import make_plane_case
from test_oracle_vpm import make_vpm_case

COUNTERS = ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts")
RECORDS = {"bre": ("ph",), "vpm": ("ph",), "beams": ("beams", "end_n"), "planes": ("beams", "w1", "len1")}


def _bre(scene, **kw):
    return cases.make_case(scene, 24, 20, 8000, 3.0, **kw)


def _plain(c):
    c.oracle_table = c.bsdfs
    c.dev_table = c.bsdfs
    c.dev_records = None   # the oracle's own
    return c


def _limit(c, oracle_table, dev_table, dev_ph):
    c.oracle_table = np.ascontiguousarray(oracle_table, abi.BSDF_DTYPE)
    c.dev_table = np.ascontiguousarray(dev_table, abi.BSDF_DTYPE)
    c.dev_records = (dev_ph,)
    assert ((dev_ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF).sum() > 300
    return c


def _rough_plastic():
    """plastic_cases.limit2_tables: cbox_conductor with k = 0 against the rough plastic's glossy component alone (T = 0)"""
    c = _bre("cbox_conductor")
    cond, plastic, mapping = PC.limit2_tables(c.bsdfs)
    return _limit(c, cond, plastic, PC.relabelled(c.ph, mapping))


def _smooth_plastic():
    """plastic_cases.limit1_table: eta = 1, Fdr = 0 -- the smooth plastic IS the Lambertian wall it replaces"""
    c = _bre("cbox")
    return _limit(c, c.bsdfs, PC.limit1_table(abi.GVPM_BSDF_PLASTIC), PC.relabelled(c.ph, None, lambertian_to=0))


def _aniso(scene):
    """aniso_cases.equal_alpha_table: the scene's isotropic Ward / conductor entries as anisotropic heads with skew tangents"""
    c = _bre(scene)
    table, mapping = AC.equal_alpha_table(c.bsdfs)
    return _limit(c, c.bsdfs, table, PC.relabelled(c.ph, mapping))


def _dielectric():
    """dielectric_cases.conductor_limit: reflection from outside equals a k = 0 conductor; the pdfs differ by F, hence use_mis = 0"""
    c = _bre("cbox_conductor", use_mis=0)
    cond, diel = DC.conductor_limit(c.bsdfs)
    return _limit(c, cond, diel, c.ph)


def _mixture():
    """mixture_cases.over_conductor at weights (1, 0): {the wall's conductor, Lambertian} is the plain conductor"""
    c = _bre("cbox_conductor")
    own, ph = c.bsdfs.copy(), c.ph
    MC.over_conductor(c, (1.0, 0.0))          # (re-labels c.ph into a copy and replaces c.bsdfs)
    dev_ph, table = c.ph, c.bsdfs
    c.ph, c.bsdfs = ph, own
    return _limit(c, own, table, dev_ph)


def _medium(name, nph=8000, scale=3.0):
    return _plain(medium_cases.apply(cases.make_case("cbox", 24, 20, nph, scale), name))


def _beams(scene, tech):
    return _plain(make_beam_case(scene, 16, 12, 3000, 3.0, technique=tech))


def _vpm(scene):
    return _plain(make_vpm_case(scene, 20, 16, 6000, 6.0, nb=4, it=2))


def _planes():
    """500 planes light every one of the 16 x 12 x 27 entries, and assertion A (an entry the oracle leaves at exactly 0 is 0) would
    hold of anything: the camera beams of every pixel with (x + 3 y) % 7 == 0 are left out (28 pixels, one of them the corner
    (0, 0)): their 756 entries are exact zeros between lit neighbours."""
    c = _plain(make_plane_case("cbox_in", 16, 12, 500, it=2))
    px, py = cases.pixels_of(c.rays)
    c.rays = np.ascontiguousarray(c.rays[(px + 3 * py) % 7 != 0])
    return c


B3, B1 = abi.GVPM_BEAM_BEAM_3D_OPTIMIZED, abi.GVPM_BEAM_BEAM_1D
CASES = {
    # G-BRE 3D
    "bre cbox": ("bre", lambda: _plain(_bre("cbox"))),
    "bre cbox_hg": ("bre", lambda: _plain(_bre("cbox_hg"))),
    "bre cbox_rot": ("bre", lambda: _plain(_bre("cbox_rot"))),
    "bre phong": ("bre", lambda: _plain(_bre("cbox_phong"))),
    "bre conductor": ("bre", lambda: _plain(_bre("cbox_conductor"))),
    "bre ward": ("bre", lambda: _plain(_bre("cbox_ward"))),
    "bre rough plastic (limit)": ("bre", _rough_plastic),
    "bre smooth plastic (limit)": ("bre", _smooth_plastic),
    "bre ward aniso (limit)": ("bre", lambda: _aniso("cbox_ward")),
    "bre conductor aniso (limit)": ("bre", lambda: _aniso("cbox_conductor")),
    "bre rough dielectric (limit)": ("bre", _dielectric),
    "bre mixture (limit)": ("bre", _mixture),
    # G-BRE 2D
    "bre2d cbox": ("bre", lambda: _plain(_bre("cbox", vol_technique=abi.GVPM_VOL_BRE2D, use_shift_null=0))),
    # media
    "bre chroma": ("bre", lambda: _medium("chroma")),
    # thick (sigma_t = 32): at 8 000 photons and scale 3 an entry is the transmittance of ONE camera depth and 4 118 of the 8 649
    # non-zero entries lie below 1e-7 lum (iterations 1 - 3 alike); 30 000 photons at scale 8 put near terms into every entry: 63 of 12 030
    "bre thick": ("bre", lambda: _medium("thick", 30000, 8.0)),
    # G-Beams
    "beams3d cbox": ("beams", lambda: _beams("cbox", B3)),
    "beams3d phong": ("beams", lambda: _beams("cbox_phong", B3)),
    "beams1d cbox": ("beams", lambda: _beams("cbox", B1)),
    "beams1d phong": ("beams", lambda: _beams("cbox_phong", B1)),
    # G-VPM
    "vpm cbox": ("vpm", lambda: _vpm("cbox")),
    "vpm phong": ("vpm", lambda: _vpm("cbox_phong")),
    # G-Planes
    "planes cbox_in": ("planes", _planes),
}
NAMES = list(CASES)
MUTATED = ["bre cbox", "beams1d cbox", "vpm cbox", "planes cbox_in"]   # the cases the mutation tests run on


def records_of(c, tech):
    return tuple(getattr(c, k) for k in RECORDS[tech])


def without(records, i):
    """the records with entry i removed (photons / beams by subset, the side arrays by deletion)"""
    keep = np.delete(np.arange(records[0].n), i)
    return (records[0].subset(keep),) + tuple(np.ascontiguousarray(np.delete(a, i, axis=0)) for a in records[1:])


def oracle(c, tech, precision=64, fast=False, records=None):
    """(accum[H, W, 27] float64, counters, (scale_vol, n_vol) or None) of ONE gather at iteration c.it on the case's inputs"""
    rec = records_of(c, tech) if records is None else records
    O.set_bsdfs(c.oracle_table)
    if tech == "bre":
        acc, cnt, _ = O.gather_bre(c.p, c.m, c.tris, rec[0], c.rays, c.r, c.it, c.nb, precision, use_accel=False, fast=fast)
        return acc, cnt, None
    if tech == "beams":
        acc, cnt, _ = O.gather_beams(c.p, c.m, c.tris, rec[0], rec[1], c.rays, c.r, c.it, c.nb, precision, fast=fast)
        return acc, cnt, None
    if tech == "vpm":
        acc, sv, nv, cnt, _ = O.gather_vpm(c.p, c.m, c.tris, rec[0], c.rays, c.samples, precision, use_accel=False, fast=fast)
        return acc, cnt, (sv, nv)
    acc, cnt, _ = O.gather_planes(c.p, c.m, c.tris, rec[0], rec[1], rec[2], c.rays, c.it, c.nb, precision, fast=fast)
    return acc, cnt, None


class Prepared:
    pass


_CACHE = {}


def prepared(name):
    """the case with its three oracle runs, once per process"""
    if name not in _CACHE:
        tech, make = CASES[name]
        r = Prepared()
        r.name, r.tech, r.c = name, tech, make()
        r.r64, r.cnt64, state = oracle(r.c, tech, 64)
        r.sv, r.nv = state if state else (None, None)
        r.r32, r.cnt32, _ = oracle(r.c, tech, 32)
        r.rfast, r.cntfast, _ = oracle(r.c, tech, 32, fast=True)
        r.lum = luminance(r.r64)
        r.dev_records = records_of(r.c, tech) if r.c.dev_records is None else r.c.dev_records
        r.dev_table = r.c.dev_table
        for a in (r.r64, r.r32, r.rfast):
            a.setflags(write=False)
        _CACHE[name] = r
    return _CACHE[name]


def lost_evaluation(r):
    """m5: the fp64 oracle re-run with the first photon / beam / plane removed whose removal loses at least one evaluation"""
    rec = records_of(r.c, r.tech)
    for i in range(rec[0].n):
        acc, cnt, _ = oracle(r.c, r.tech, 64, records=without(rec, i))
        if cnt["evaluations"] < r.cnt64["evaluations"]:
            return acc, i, r.cnt64["evaluations"] - cnt["evaluations"]
    raise AssertionError("no record of the case has an evaluation")
