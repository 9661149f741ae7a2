"""Builders for the tests of the two-component mixture (GVPM_BSDF_MIXTURE): entries, the tables of the three synthetic scenes stated
with the host's own double-precision parameters, relabelled tables over the records of cbox_conductor -- what a reconnection
evaluates is a function of the record and the table alone -- and the tables gvpm_upload_bsdfs refuses."""
import copy

import numpy as np

import aniso_cases as AC
import cases
import indep_aniso
import oracle_lib
import phong_dist_cases as PD_C
import plastic_cases as PC
from gvpm_amd import abi

SCENES = ["cbox_mixture", "cbox_mixture_rot", "cbox_mixture1"]
CU, AL = PD_C.CU, PD_C.AL
BECKMANN, GGX, PHONG = abi.GVPM_MICROFACET_BECKMANN, abi.GVPM_MICROFACET_GGX, abi.GVPM_MICROFACET_PHONG
DIFFUSE, ABSENT = abi.GVPM_MIXTURE_CHILD_DIFFUSE, abi.GVPM_MIXTURE_CHILD_ABSENT
TANGENT = np.array([0.9, 0.35, 0.25]) / np.linalg.norm([0.9, 0.35, 0.25])   # the brushed child's (synth.cpp)
# material indices of the scenes (synth.cpp): the children 4 (copper), 5 (aluminium), 6 (brushed copper), then the mixtures
MATS = {"cbox_mixture": {"floor": 7, "left": 8, "right": 9, "back": 10}, "cbox_mixture1": {"floor": 7, "back": 8}}
KD = {"floor": (0.5, 0.5, 0.5), "left": (0.63, 0.065, 0.05), "right": (0.14, 0.45, 0.091)}


# ---- entries ----------------------------------------------------------------------------------------------------------------------
def conductor_entry(alpha, metal=CU, distribution=BECKMANN, specular=1.0, sample_visible=0):
    return PD_C.conductor_entry(alpha, metal, specular, distribution, sample_visible)


def aniso_entry(alpha_u, alpha_v, tangent, metal=CU, distribution=BECKMANN, specular=1.0, sample_visible=0):
    return PD_C.aniso_entry(alpha_u, alpha_v, tangent, metal, specular, distribution, sample_visible)


mixture = abi.mixture_entry


# ---- the scenes' children with the host's double-precision parameters ----------------------------------------------------------------
def host_children(scene, tangent=TANGENT):
    """the statement of the scene's conductor children by TABLE index (0 copper, 1 aluminium, 2 brushed copper) with the doubles the
    host walks with (synth.cpp), for the 1e-9 comparisons: indep_aniso.aniso_rows takes its parameters as numbers"""
    alpha_cu = 0.03 if scene == "cbox_mixture1" else 0.3
    params = {0: (alpha_cu, alpha_cu, CU, False), 1: (0.2, 0.2, AL, True), 2: (0.12, 0.45, CU, False)}

    def children(kd, index, n, wi, wo):
        k = len(index)
        f, pdf, known = np.zeros((k, 3)), np.zeros(k), np.zeros(k, bool)
        for child, (au, av, metal, ggx) in params.items():
            r = np.flatnonzero(np.asarray(index) == child)
            if not r.size:
                continue
            one = lambda x: np.broadcast_to(np.asarray(x, np.float64), (r.size, 3))
            s = one(tangent) if child == 2 else np.eye(3)[np.argmin(np.abs(n[r]), axis=-1)]
            z, flag = np.zeros(r.size), np.zeros(r.size, bool)
            f[r], pdf[r], known[r] = indep_aniso.aniso_rows(flag, one(1.0), au + z, av + z, s, z, flag.astype(np.int32), flag | ggx, flag,
                                                            one(metal[0]), one(metal[1]), kd[r], n[r], wi[r], wo[r])
        return f, pdf, known

    return children


# ---- relabelled tables over cbox_conductor's records (entries 0: the floor's copper, 1: the back wall's aluminium) ----------------
def conductor_records(**kw):
    """20 x 16 pixels, 20 000 photons, scale 4: 7 797 evaluations and 1 759 reconnections through the two walls (the siblings' figures)"""
    return cases.make_case("cbox_conductor", 20, 16, 20000, 4.0, **kw)


def with_table(c, table, mapping=None, records="ph"):
    return PD_C.with_table(c, table, mapping, records)


def over_conductor(c, weights, other=DIFFUSE, component=0, conductor_first=True, children_last=False, wall_entries=None):
    """the case's table replaced by, per wall, a mixture of {that wall's conductor entry, `other`} (the other way round with
    conductor_first = False); children_last: the mixtures first in the table, the children behind them.  Returns the mixtures' heads."""
    walls = c.sc.bsdfs() if wall_entries is None else wall_entries
    heads = np.flatnonzero(abi.bsdf_heads(walls))
    nmix = heads.size
    base = nmix if children_last else 0
    off = 0 if children_last else walls.size
    mix = []
    for h in heads:
        kids = (base + h, other) if conductor_first else (other, base + h)
        mix.append(mixture(weights if conductor_first else weights[::-1], kids, component))
    table = np.concatenate(mix + [walls]) if children_last else np.concatenate([walls] + mix)
    own = c.sc.bsdfs()                               # the records name the scene's own heads, wall by wall
    mapping = np.zeros(own.size, np.int64)
    mapping[np.flatnonzero(abi.bsdf_heads(own))] = off + np.arange(nmix)
    with_table(c, table, mapping)
    return off + np.arange(nmix)


def retyped_lambertian(c, kd):
    """the glossy records retyped GVPM_PARENT_SURFACE with reflectance kd (what the oracle knows)"""
    ph = copy.deepcopy(c.ph)
    gl = (ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    ph.flags[gl] = (ph.flags[gl] & ~np.uint32(3)) | np.uint32(abi.GVPM_PARENT_SURFACE)
    ph.parent_scat[gl] = kd
    ph.parent_g[gl] = c.m.g
    c.ph = ph
    return c


def set_parent_scat(c, kd):
    ph = copy.deepcopy(c.ph)
    gl = (ph.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    ph.parent_scat[gl] = kd
    c.ph = ph
    return c


# ---- the synthetic scenes ----------------------------------------------------------------------------------------------------------
make_case = cases.make_case


def make_beam_case(name, W=12, H=10, nbeams=800, scale=5.0, technique=abi.GVPM_BEAM_BEAM_3D_OPTIMIZED, it=1, **kw):
    return PD_C.make_beam_case(name, W, H, nbeams, scale, technique, it, **kw)


def make_vpm_case(name, W=12, H=10, nph=8000, scale=8.0, nb=6, it=1, **kw):
    return PD_C.make_vpm_case(name, W, H, nph, scale, nb, it, **kw)


# ---- what gvpm_upload_bsdfs refuses ------------------------------------------------------------------------------------------------
def refused_tables():
    """[(what, table, "invalid" | "unsupported")]: each table of include/gvpm_hip.h's list, one defect each"""
    cond, ani = conductor_entry(0.3), aniso_entry(0.12, 0.45, AC.SKEW[0])
    phong = np.zeros(1, abi.BSDF_DTYPE)
    phong["kind"], phong["specular"], phong["exponent"], phong["specular_sampling_weight"] = abi.GVPM_BSDF_PHONG, 0.3, 40.0, 0.5
    good = lambda: np.concatenate([cond, ani, mixture((0.6, 0.4), (DIFFUSE, 0))])      # heads 0, 1 (+ frame 2), mixture 3
    out = []

    def bad(what, code, edit, table=None):
        t = good() if table is None else table
        edit(t)
        out.append((what, t, code))

    def field(name, value, col=None):
        def edit(t):
            if col is None:
                t[name][3] = value
            else:
                t[name][3, col] = value
        return edit

    bad("negative weight", "invalid", field("specular", -0.1, 0))
    bad("infinite weight", "invalid", field("specular", np.inf, 1))
    bad("nan weight", "invalid", field("specular", np.nan, 0))
    bad("weights sum to zero", "invalid", lambda t: t["specular"].__setitem__((3, slice(0, 2)), 0.0))
    bad("component 3", "invalid", field("distribution", 3))
    bad("component -1", "invalid", field("distribution", -1))
    bad("child -3", "invalid", field("eta", -3.0, 1))
    bad("child 0.5", "invalid", field("eta", 0.5, 1))
    bad("child past the table", "invalid", field("eta", 4.0, 1))
    bad("child nan", "invalid", field("eta", np.nan, 1))
    bad("child names a raw entry", "invalid", field("eta", 2.0, 1))
    bad("absent child selected", "invalid", lambda t: (field("eta", float(ABSENT), 1)(t), field("distribution", 2)(t)))
    bad("absent child with both components", "invalid", field("eta", float(ABSENT), 1))
    for name, col in (("specular", 2), ("exponent", None), ("specular_sampling_weight", None), ("eta", 2), ("k", 0), ("k", 2), ("reserved", 0),
                      ("reserved", 1)):
        bad(f"unused word {name}[{col}]", "invalid", field(name, 1.0, col))
    bad("unused word sample_visible", "invalid", field("sample_visible", 1))
    bad("unused word -0", "invalid", field("exponent", -0.0))
    bad("a Phong child", "unsupported", lambda t: None, np.concatenate([phong, ani, mixture((0.6, 0.4), (DIFFUSE, 0))]))
    bad("a mixture as a child", "unsupported", field("eta", 3.0, 1))
    bad("two Lambertian children", "unsupported", field("eta", float(DIFFUSE), 1))
    return out


def accepted_tables():
    """legal corners: an absent child beside the selected one, children behind the mixture, a shared child, zero weight"""
    cond, ani = conductor_entry(0.3), aniso_entry(0.12, 0.45, AC.SKEW[0])
    return [np.concatenate([cond, mixture((0.7, 0.3), (0, ABSENT), 1)]),
            np.concatenate([mixture((0.5, 0.5), (1, 2)), cond, ani]),
            np.concatenate([cond, mixture((0.5, 0.5), (0, 0)), mixture((1.0, 0.0), (0, DIFFUSE))]),
            np.concatenate([cond, mixture((0.9, 0.8), (DIFFUSE, 0), 2)])]
