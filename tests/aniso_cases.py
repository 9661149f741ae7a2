"""Builders for the tests of the anisotropic parents (GVPM_BSDF_WARD_ANISO / GVPM_BSDF_ROUGHCONDUCTOR_ANISO): tables the scenes do
not have, the equal-alpha tables that ARE the isotropic kinds the frozen fp64 oracle states, cases whose records are
re-labelled to name such heads, and tables with every tangent turned a quarter about its wall's normal."""
import numpy as np

import indep_statements
import oracle_lib
from gvpm_amd import abi
from plastic_cases import relabelled, use_table  # noqa: F401  (the same record surgery)

E = 1 + abi.bsdf_tail_entries(abi.GVPM_BSDF_WARD_ANISO)  # table entries an anisotropic surface takes
# the walls of the cbox scenes that carry glossy materials (floor, back wall) and a tangent for each that is neither in the
# wall nor along an axis: the device projects it
WALL_N = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
SKEW = np.array([[0.48, 0.6, -0.64], [-0.36, 0.8, 0.48]])   # unit vectors, 0.6 / 0.48 along the normals


def aniso_materials(sc):
    """material indices of a scene's anisotropic walls, in table order (sample_aniso refuses every other material)"""
    out = []
    for mat in range(64):
        try:
            sc.sample_aniso(mat, (0.0, 0.0, 1.0), (0.0, 0.0, 1.0), 0.5, 0.5)
            out.append(mat)
        except ValueError:
            pass
    return out


def equal_alpha_table(iso, tangents=SKEW):
    """(table, mapping): the isotropic Ward / rough-conductor entries of `iso` as anisotropic heads with alphaV == alphaU and
    the given tangents -- the same BSDFs, whatever the tangent; mapping: iso entry -> head"""
    parts = []
    for j, b in enumerate(iso):
        if b["kind"] == abi.GVPM_BSDF_WARD:
            parts.append(abi.aniso_entry(abi.GVPM_BSDF_WARD_ANISO, b["specular"], b["exponent"], b["exponent"], tangents[j % len(tangents)],
                                         weight=b["specular_sampling_weight"], variant=int(b["sample_visible"])))
        else:
            assert b["kind"] == abi.GVPM_BSDF_ROUGHCONDUCTOR
            parts.append(abi.aniso_entry(abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO, b["specular"], b["exponent"], b["exponent"],
                                         tangents[j % len(tangents)], distribution=int(b["distribution"]),
                                         sample_visible=int(b["sample_visible"]), eta=b["eta"], k=b["k"]))
    return np.concatenate(parts), np.arange(iso.size) * E


def other_tables(which):
    """tables for two walls that the scenes do not have: 'ward' -- the third variant (ward-duer) and the original one, alphas 0.06 x
    0.5 / 0.45 x 0.07; 'conductor' -- visible-normal sampling (the projected roughness is in the pdf), 0.07 x 0.5 Beckmann and
    0.4 x 0.09 GGX"""
    if which == "ward":
        t = [abi.aniso_entry(abi.GVPM_BSDF_WARD_ANISO, (0.5, 0.45, 0.4), 0.06, 0.5, SKEW[0], weight=0.55, variant=abi.GVPM_WARD_DUER),
             abi.aniso_entry(abi.GVPM_BSDF_WARD_ANISO, (0.3, 0.3, 0.35), 0.45, 0.07, SKEW[1], weight=0.4, variant=abi.GVPM_WARD_WARD)]
    else:
        t = [abi.aniso_entry(abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO, (1.0, 0.9, 0.8), 0.07, 0.5, SKEW[0], distribution=abi.GVPM_MICROFACET_BECKMANN,
                             sample_visible=1, eta=(0.2004, 0.9240, 1.1022), k=(3.9129, 2.4528, 2.1421)),
             abi.aniso_entry(abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO, (0.9, 0.9, 1.0), 0.4, 0.09, SKEW[1], distribution=abi.GVPM_MICROFACET_GGX,
                             sample_visible=1, eta=(1.6574, 0.8803, 0.5212), k=(9.2238, 6.2695, 4.8370))]
    return np.concatenate(t), [0, E]


def relabelled_case(c, table, heads, records="ph"):
    """A case of a scene with two glossy walls of one entry each (cbox_ward, cbox_conductor, cbox_phong) whose table is replaced:
    the records that named wall k's entry now name heads[k].  What a reconnection evaluates depends on the record and the
    table alone."""
    assert c.bsdfs.size == 2
    setattr(c, records, relabelled(getattr(c, records), np.asarray(heads)))
    use_table(c, table)
    oracle_lib.set_bsdfs(c.bsdfs)   # (the oracle ignores the kinds it does not know: those shifts fail there)
    return c


def turned(table, normals):
    """a copy of `table` whose heads' tangents are turned a quarter about normals[k] (head k's wall): s' = n x (s - n (n . s)),
    normalised"""
    out = table.copy()
    raw = out.view(np.float32).reshape(-1, 16)
    heads = np.flatnonzero(abi.bsdf_heads(table))
    for h, n in zip(heads, np.asarray(normals, np.float64)):
        s = raw[h + 1, 0:3].astype(np.float64)
        s = s - n * (n @ s)
        t = np.cross(n, s / np.linalg.norm(s))
        t = np.where(np.abs(t) < 1e-30, 0.0, t)
        raw[h + 1, 0:3] = t
    return out


def wall_normals(c, records="ph"):
    """the parent normal of the records that name each head of the case's table (one plane per head, asserted)"""
    rec = getattr(c, records)
    gl = (rec.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    out = []
    for h in np.flatnonzero(abi.bsdf_heads(c.bsdfs)):
        ns = rec.parent_n[gl][rec.parent_g[gl] == h].astype(np.float64)
        assert len(ns) and np.abs(ns - ns[0]).max() < 1e-6
        out.append(ns[0] / np.linalg.norm(ns[0]))
    return np.array(out)


def set_tables(table):
    indep_statements.set_bsdfs(table)
    oracle_lib.set_bsdfs(table)
