"""Builders for the tests of the Phong / Ashikhmin-Shirley microfacet distribution (GVPM_MICROFACET_PHONG): table entries of the four
kinds that carry it (plastic_cases.rough_entry cannot name the distribution), the slices of tests/golden/rtrans_slices_phong.npz,
the three synthetic scenes with their slices set, and relabelled tables over the records of existing scenes -- what a reconnection
evaluates is a function of the record and the table alone."""
import os

import numpy as np

import aniso_cases as AC
import cases
import oracle_lib
import plastic_cases as PC
from gvpm_amd import abi

PHONG, BECKMANN = abi.GVPM_MICROFACET_PHONG, abi.GVPM_MICROFACET_BECKMANN
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rtrans_slices_phong.npz")
SCENES = ["cbox_conductor_phong", "cbox_roughplastic_phong", "cbox_roughglass_phong"]
CU = ((0.2004, 0.9240, 1.1022), (3.9129, 2.4528, 2.1421))   # eta, k
AL = ((1.6574, 0.8803, 0.5212), (9.2238, 6.2695, 4.8370))


def rtrans(eta, alpha):
    """(slice[100], Fdr) of the fixture (data/microfacet/phong.dat reduced at eta and alpha)"""
    v = np.load(GOLDEN)[f"phong_eta{eta:g}_alpha{alpha:g}"]
    return v[:abi.GVPM_RTRANS_KNOTS].copy(), float(v[abi.GVPM_RTRANS_KNOTS])


# ---- entries ----------------------------------------------------------------------------------------------------------------------
def conductor_entry(alpha, metal=CU, specular=1.0, distribution=PHONG, sample_visible=0):
    b = np.zeros(1, abi.BSDF_DTYPE)
    b["kind"], b["specular"], b["exponent"] = abi.GVPM_BSDF_ROUGHCONDUCTOR, specular, alpha
    b["distribution"], b["sample_visible"], b["eta"], b["k"] = distribution, sample_visible, metal[0], metal[1]
    return b


def aniso_entry(alpha_u, alpha_v, tangent, metal=AL, specular=1.0, distribution=PHONG, sample_visible=0):
    return abi.aniso_entry(abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO, specular, alpha_u, alpha_v, tangent, distribution=distribution,
                           sample_visible=sample_visible, eta=metal[0], k=metal[1])


def rough_entry(alpha, specular, weight, component=0, eta=1.5, nonlinear=False, distribution=PHONG, sample_visible=0, slice_alpha=None):
    """head + the 7 raw entries of its slice: the fixture's at `slice_alpha` (alpha unless given)"""
    sl, fdr = rtrans(eta, alpha if slice_alpha is None else slice_alpha)
    head = abi.plastic_entry(abi.GVPM_BSDF_ROUGHPLASTIC, specular, eta, fdr, weight, component, alpha=alpha, distribution=distribution,
                             sample_visible=sample_visible, nonlinear=nonlinear)
    return np.concatenate([head, abi.rtrans_entries(sl)])


def glass_table(alpha, eta=1.5, ks=(1.0, 0.95, 0.9), kt=(0.9, 0.95, 1.0), distribution=PHONG, sample_visible=0):
    """the two entries of one rough-dielectric surface: met from outside (eta), met from inside (1 / eta)"""
    return np.concatenate([abi.dielectric_entry(ks, kt, alpha, eta, distribution, sample_visible),
                           abi.dielectric_entry(ks, kt, alpha, 1.0 / eta, distribution, sample_visible)])


# ---- relabelled tables over the records of existing scenes --------------------------------------------------------------------------
def with_table(c, table, mapping=None, records="ph"):
    if mapping is not None:
        setattr(c, records, PC.relabelled(getattr(c, records), mapping))
    PC.use_table(c, table)
    oracle_lib.set_bsdfs(c.bsdfs)   # (the oracle reads these entries as Beckmann's or not at all)
    return c


def conductor_table(alpha, distribution=PHONG):
    """cbox_conductor's two walls (entries 0 and 1) at one alpha under `distribution`"""
    return np.concatenate([conductor_entry(alpha, CU, distribution=distribution), conductor_entry(alpha, AL, (0.9, 0.9, 1.0), distribution)])


def aniso_table(alpha_u, alpha_v, distribution=PHONG):
    """cbox_conductor_aniso's two walls (heads 0 and AC.E) at the given alphas, skew tangents"""
    return np.concatenate([aniso_entry(alpha_u, alpha_v, AC.SKEW[0], CU, distribution=distribution),
                           aniso_entry(alpha_v, alpha_u, AC.SKEW[1], AL, (0.9, 0.9, 1.0), distribution)])


ANISO_TO_ISO = np.array([0, 0, 1])   # cbox_conductor_aniso's heads (0, 2) -> conductor_table's entries


def plastic_table(alpha, component=0, distribution=PHONG, slice_alpha=None):
    """cbox_roughplastic's two walls (heads 0 and PC.E) at one alpha, met through `component`"""
    return np.concatenate([rough_entry(alpha, (0.25, 0.3, 0.2), 0.35, component, distribution=distribution, slice_alpha=slice_alpha),
                           rough_entry(alpha, (0.2, 0.2, 0.3), 0.45, component, nonlinear=True, distribution=distribution,
                                       slice_alpha=slice_alpha)])


# ---- the synthetic scenes ----------------------------------------------------------------------------------------------------------
def scene(name, W, H):
    """SynthScene with the fixture's slices set where the scene has rough-plastic walls (nothing can be shot before)"""
    from gvpm_amd.host import SynthScene
    sc = SynthScene(name, W, H)
    for mat, dist, alpha, eta in sc.rtrans_materials():
        assert dist == "phong"
        sc.set_rtrans(mat, *rtrans(round(eta, 4), round(alpha, 4)))
    return sc


def make_case(name, W=24, H=20, nph=6000, scale=4.0, it=1, **overrides):
    """cases.make_case with the slices set before the first shot"""
    c = cases.Case()
    c.sc = scene(name, W, H)
    c.p = c.sc.params()
    c.p.initial_scale_volume = scale
    for k, v in overrides.items():
        setattr(c.p, k, v)
    c.m = c.sc.medium()
    c.tris = c.sc.triangles()
    c.ph, c.nb = c.sc.shoot_photons(it, nph)
    c.rays = c.sc.camera_beams(it)
    c.r = cases.radius_of(c.p)
    c.it = it
    cases.use_bsdfs(c)
    return c


def make_beam_case(name, W=16, H=12, nbeams=3000, scale=3.0, technique=abi.GVPM_BEAM_BEAM_3D_OPTIMIZED, it=1, **kw):
    if technique == abi.GVPM_BEAM_BEAM_1D:
        kw.setdefault("use_shift_null", 0)
    c = make_case(name, W, H, 10, scale, it=it, vol_technique=technique, **kw)
    c.beams, c.end_n, c.nb = c.sc.shoot_beams(it, nbeams)
    return c


def make_vpm_case(name, W=20, H=16, nph=20000, scale=6.0, nb=8, it=1, **kw):
    c = make_case(name, W, H, nph, scale, it=it, vol_technique=abi.GVPM_DISTANCE, nb_camera_samples=nb, **kw)
    c.rays, c.samples = c.sc.camera_beams_and_vpm_samples(it, nb)
    return c
