"""Builders for the tests of the plastic parents (GVPM_BSDF_ROUGHPLASTIC / GVPM_BSDF_PLASTIC): tables with their transmittance
slices from tests/golden/rtrans_slices.npz, the two limit tables the fp64 oracle can state, and cases whose photons are
re-labelled to name such entries."""
import copy
import os

import numpy as np

import cases
import indep_statements
import oracle_lib
from gvpm_amd import abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rtrans_slices.npz")
E = 1 + abi.bsdf_tail_entries(abi.GVPM_BSDF_ROUGHPLASTIC)  # table entries a rough-plastic surface takes


def rtrans(dist, eta, alpha):
    """(slice[100], Fdr) of the fixture"""
    v = np.load(GOLDEN)[f"{dist}_eta{eta:g}_alpha{alpha:g}"]
    return v[:abi.GVPM_RTRANS_KNOTS].copy(), float(v[abi.GVPM_RTRANS_KNOTS])


def rough_entry(dist, alpha, specular, weight, component=0, eta=1.5, sample_visible=0, nonlinear=False, slice_=None, fdr=None):
    """head + the 7 raw entries of its slice (the fixture's, unless given)"""
    if slice_ is None:
        slice_, fdr = rtrans(dist, eta, alpha)
    head = abi.plastic_entry(abi.GVPM_BSDF_ROUGHPLASTIC, specular, eta, fdr, weight, component, alpha=alpha,
                             distribution=abi.GVPM_MICROFACET_GGX if dist == "ggx" else abi.GVPM_MICROFACET_BECKMANN,
                             sample_visible=sample_visible, nonlinear=nonlinear)
    return np.concatenate([head, abi.rtrans_entries(slice_)])


def smooth_fdr_int(eta):
    """1 - the diffuse Fresnel transmittance from inside (fresnelDiffuseReflectance(1 / eta), what plastic.cpp's m_fdrInt holds):
    the cosine-weighted hemispherical mean of the reflectance seen from the denser side, by quadrature"""
    mu = (np.arange(200000) + 0.5) / 200000
    s2 = (1 - mu * mu) * eta * eta
    ct = np.sqrt(np.maximum(1 - s2, 0))
    rs, rp = (eta * mu - ct) / (eta * mu + ct), (mu - eta * ct) / (mu + eta * ct)
    return float((np.where(s2 >= 1, 1.0, 0.5 * (rs * rs + rp * rp)) * 2 * mu).mean())


def smooth_entry(specular, weight, eta=1.5, nonlinear=False, fdr=None):
    return abi.plastic_entry(abi.GVPM_BSDF_PLASTIC, specular, eta, smooth_fdr_int(eta) if fdr is None else fdr, weight, 2,
                             nonlinear=nonlinear)


def use_table(c, table):
    """the case's table for the device (c.bsdfs) and the numpy statements; the oracle keeps whatever it was given"""
    c.bsdfs = np.ascontiguousarray(table, abi.BSDF_DTYPE)
    indep_statements.set_bsdfs(c.bsdfs)


def relabelled(ph, mapping, lambertian_to=None):
    """a copy of photon / beam records whose glossy parents name mapping[old index]; lambertian_to: GVPM_PARENT_SURFACE parents
    become GVPM_PARENT_SURFACE_BSDF parents naming that entry"""
    out = copy.deepcopy(ph)
    pt = out.flags & 3
    gl = pt == abi.GVPM_PARENT_SURFACE_BSDF
    if mapping is not None:
        out.parent_g[gl] = np.asarray(mapping, np.float32)[out.parent_g[gl].astype(np.int64)]
    if lambertian_to is not None:
        lam = pt == abi.GVPM_PARENT_SURFACE
        out.flags[lam] |= np.uint32(abi.GVPM_PARENT_SURFACE_BSDF)
        out.parent_g[lam] = lambertian_to
    return out


def limit1_table(kind):
    """eta = 1, Fdr = 0, T = 1: either plastic IS the Lambertian surface (eval kd cos / pi, pdf cos / pi)"""
    if kind == abi.GVPM_BSDF_PLASTIC:
        return smooth_entry((0.7, 0.6, 0.5), 0.4, eta=1.0, fdr=0.0)
    return rough_entry("beckmann", 0.1, (0.7, 0.6, 0.5), 0.4, eta=1.0, slice_=np.ones(abi.GVPM_RTRANS_KNOTS, np.float32), fdr=0.0)


def limit2_tables(conductor, eta=1.5):
    """(the conductor table with eta = (eta, eta, eta), k = 0; the rough-plastic table that equals it: glossy component alone,
    T = 0 and w > 0, so pS = 1; the index mapping conductor entry -> plastic head)"""
    cond = conductor.copy()
    cond["eta"], cond["k"] = eta, 0.0
    parts = []
    for b in cond:
        parts.append(rough_entry("ggx" if b["distribution"] == abi.GVPM_MICROFACET_GGX else "beckmann", float(b["exponent"]),
                                 b["specular"], 0.5, component=1, eta=eta, sample_visible=int(b["sample_visible"]),
                                 slice_=np.zeros(abi.GVPM_RTRANS_KNOTS, np.float32), fdr=0.0))
    return cond, np.concatenate(parts), np.arange(cond.size) * E


def plastic_tables(which):
    """(table, heads) for two glossy walls: 'rough' (Beckmann 0.1 / GGX 0.3, both components), 'rough1' (alpha 0.03 / 0.04: an entry
    per component), 'smooth'"""
    ks = ((0.25, 0.3, 0.2), (0.2, 0.2, 0.3))
    if which == "rough":
        t = [rough_entry("beckmann", 0.1, ks[0], 0.35), rough_entry("ggx", 0.3, ks[1], 0.45, sample_visible=1, nonlinear=True)]
        return np.concatenate(t), [0, E]
    if which == "rough1":
        t = [rough_entry("beckmann", 0.03, ks[0], 0.35, component=1), rough_entry("beckmann", 0.03, ks[0], 0.35, component=2),
             rough_entry("ggx", 0.04, ks[1], 0.45, component=1), rough_entry("ggx", 0.04, ks[1], 0.45, component=2, nonlinear=True)]
        return np.concatenate(t), [0, E, 2 * E, 3 * E]
    t = [smooth_entry(ks[0], 0.35), smooth_entry(ks[1], 0.45, nonlinear=True)]
    return np.concatenate(t), [0, 1]


def relabelled_case(c, which, records="ph"):
    """A case of a scene with two glossy walls (cbox_phong*, cbox_conductor) whose table is replaced by plastic entries: the
    photons (records = "beams": the beams) that named wall k's entries now name the plastic entries of wall k.  What a
    reconnection evaluates depends on the record and the table alone, so this states the gather for plastic parents
    whatever BSDF the host sampled the path with."""
    table, heads = plastic_tables(which)
    per_wall = len(heads) // 2
    old = np.arange(c.bsdfs.size)
    wall = old * 2 // max(c.bsdfs.size, 1)            # the scene's entries: first half floor, second half back wall
    comp = old % per_wall if per_wall > 1 else 0 * old
    mapping = np.asarray(heads)[wall * per_wall + comp]
    setattr(c, records, relabelled(getattr(c, records), mapping))
    use_table(c, table)
    oracle_lib.set_bsdfs(c.bsdfs)                     # (the oracle ignores the kinds it does not know: those shifts fail there)
    return c


# ---- the synthetic scenes with plastic walls ----------------------------------------------------------------------------------
def scene(name, W, H):
    """SynthScene of a plastic scene with the fixture's slices set (rough kinds: nothing can be shot before)"""
    from gvpm_amd.host import SynthScene
    sc = SynthScene(name, W, H)
    for mat, dist, alpha, eta in sc.rtrans_materials():
        sl, fdr = rtrans(dist, round(eta, 4), round(alpha, 4))
        sc.set_rtrans(mat, sl, fdr)
    return sc


def plastic_materials(sc):
    """material indices of the scene's plastic walls, in table order (the host's sample_plastic refuses every other material)"""
    out = []
    for mat in range(64):
        try:
            sc.sample_plastic(mat, (0.0, 0.0, 1.0), (0.0, 0.0, 1.0), 0.5, 0.5)
            out.append(mat)
        except ValueError:
            pass
    return out


def make_case(name="cbox_roughplastic", W=24, H=20, nph=6000, scale=4.0, it=1, **overrides):
    """cases.make_case for the plastic scenes: the same fields, the slices set before the first shot"""
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
