"""Builders for the tests of the rough-dielectric parent (GVPM_BSDF_ROUGHDIELECTRIC): the scene's material index, tables the
scenes do not have, the conductor limit, records sorted into the four classes (reflected / transmitted x met from outside /
inside) and records of another kind turned to face away from the light."""
import copy

import numpy as np

import indep_dielectric as D
from gvpm_amd import abi
from plastic_cases import relabelled, use_table  # noqa: F401  (the same record surgery)

SCENES = ["cbox_roughglass", "cbox_roughglass_rot"]
# the scenes' pane: eta 1.5 seen from its front, Beckmann alpha 0.25, reflectance and transmittance tinted differently
ETA, ALPHA, KS, KT = 1.5, 0.25, (1.0, 0.95, 0.9), (0.9, 0.95, 1.0)


def dielectric_material(sc):
    """the material index of a scene's rough-glass pane (sample_dielectric refuses every other material)"""
    for mat in range(64):
        try:
            sc.sample_dielectric(mat, (0.0, 0.0, 1.0), (0.0, 0.0, 1.0), 0.5, 0.5, 0.5)
            return mat
        except ValueError:
            pass
    raise AssertionError("the scene has no rough dielectric")


def surface_table(eta, alpha, ks, kt, distribution=abi.GVPM_MICROFACET_BECKMANN, sample_visible=0):
    """the two entries of one surface: met from outside (eta), met from inside (1 / eta)"""
    return np.concatenate([abi.dielectric_entry(ks, kt, alpha, eta, distribution, sample_visible),
                           abi.dielectric_entry(ks, kt, alpha, 1.0 / eta, distribution, sample_visible)])


def other_table(alpha):
    """a table the scenes do not have: GGX sampled with visible normals, water's index, other tints"""
    return surface_table(1.33, alpha, (0.8, 0.9, 1.0), (1.0, 0.85, 0.7), abi.GVPM_MICROFACET_GGX, 1)


def swapped(table):
    """each surface's two entries exchanged: every record now names the entry of the WRONG side of incidence"""
    out = table.copy()
    out[0::2], out[1::2] = table[1::2], table[0::2]
    return out


def classes(records, table):
    """{(reflected?, met from outside?): mask} over the records that name rough-dielectric entries"""
    tr, diel = D.is_transmitted(records, table)
    outside = records.parent_g.astype(np.int64) % 2 == 0
    return {(r, o): diel & (tr != r) & (outside == o) for r in (True, False) for o in (True, False)}


def only_class(records, mask):
    """a copy of the records in which the dielectric parents outside `mask` name no entry (their shifts fail)"""
    out = copy.deepcopy(records)
    gl = (records.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    out.parent_g[gl & ~mask] = -1.0
    return out


def conductor_limit(conductor):
    """(the conductor table with eta = (1.5, 1.5, 1.5), k = 0 and visible normals; the dielectric table that equals it in
    reflection from outside, entry for entry)"""
    cond = conductor.copy()
    cond["eta"], cond["k"], cond["sample_visible"] = 1.5, 0.0, 1
    diel = np.concatenate([abi.dielectric_entry(b["specular"], (0.5, 0.5, 0.5), float(b["exponent"]), 1.5, int(b["distribution"]), 1)
                           for b in cond])
    return cond, diel


def facing_away(records, every=3):
    """a copy of the records in which every `every`-th glossy parent's incident direction is mirrored about its surface: the
    light now arrives from behind a one-sided surface"""
    out = copy.deepcopy(records)
    gl = np.flatnonzero((records.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF)[::every]
    n, wi = records.parent_n[gl].astype(np.float64), records.parent_wi[gl].astype(np.float64)
    out.parent_wi[gl] = (wi - 2.0 * n * (n * wi).sum(1)[:, None]).astype(np.float32)
    return out, gl
