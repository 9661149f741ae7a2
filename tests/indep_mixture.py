"""Second statement of the two-component mixture (GVPM_BSDF_MIXTURE; include/gvpm_hip.h) in numpy, fp64, WORLD space, vectorised over rows
like indep_statements.phong_world: a wrapper with phong_world's signature that answers the rows naming a mixture head itself and hands
every other row -- and the mixture's own conductor children -- on to the statements of the sibling modules (indep_phong_dist over
indep_dielectric, indep_aniso, indep_plastic and indep_statements).  The frozen fp64 oracle does not know the kind.

Written from src/bsdfs/mixturebsdf.cpp:177-209,316-319: with the weights w_0, w_1 (after the constructor's rescale, :130-142) and
p_i = w_i / (w_0 + w_1) (the normalised m_pdf, :171-173)

  component -1 (entry `distribution` 0):      eval = w_0 eval_0 + w_1 eval_1,   pdf = p_0 pdf_0 + p_1 pdf_1
  component c  (entry `distribution` c + 1):  eval = w_c eval_c,                pdf * pdfComponent = pdf_c p_c

A child word is a table index (a rough-conductor head, isotropic or anisotropic, any distribution: the sibling statement of that head),
-1 the Lambertian (diffuse.cpp:110-127: eval = kd / pi cos_o, pdf = cos_o / pi, kd the record's reflectance) or -2, a child that is
not evaluable and contributes nothing.  A conductor child the siblings call undefined (an anisotropic head whose tangent spans no frame)
leaves the whole row undefined; one with D = 0 contributes zero and the other child still counts.  Light from behind (cos_i <= 0) is
undefined: a failed shift.

NEAR: the reconnections within rounding of an fp32 decision are the children's own (indep_phong_dist.NEAR, which the conductor
statements count into: D cos_H against 1e-20); the mixture adds no decision."""
import numpy as np

import indep_phong_dist
import indep_statements
from gvpm_amd import abi

KIND = abi.GVPM_BSDF_MIXTURE
DIFFUSE, ABSENT = abi.GVPM_MIXTURE_CHILD_DIFFUSE, abi.GVPM_MIXTURE_CHILD_ABSENT


def reset_near():
    indep_phong_dist.reset_near()


def near():
    return indep_phong_dist.NEAR


def _dot(a, b):
    return (a * b).sum(-1)


def is_mixture(table):
    """which entries of a table are mixture heads"""
    if not table.size:
        return np.zeros(0, bool)
    return abi.bsdf_heads(table) & (table["kind"] == KIND)


def weights(entry):
    """(w [2], p [2]) of one mixture entry, fp64"""
    w = np.asarray(entry["specular"], np.float64).reshape(-1)[:2]
    return w, w / w.sum()


def mixture_world(table, kd, index, n, wi, wo, children, weights=None, child_kinds=True):
    """(f cos [k, 3], pdf [k], defined [k]) of rows that name mixture heads of `table`; `children(kd, index, n, wi, wo)`: the statement
    of the table's other heads; weights: instead of the entries' own (the host's doubles); child_kinds = False: `children` answers for
    whatever the child words name"""
    index = np.asarray(index, np.int64)
    b = table[index]
    k = index.size
    w = b["specular"][:, :2].astype(np.float64) if weights is None else np.broadcast_to(np.asarray(weights, np.float64), (k, 2))
    p = w / w.sum(-1, keepdims=True)
    comp = b["distribution"].astype(np.int64)
    ci, co = _dot(n, wi), _dot(n, wo)
    up = (ci > 0) & (co > 0)
    f, pdf, defined = np.zeros((k, 3)), np.zeros(k), ci > 0
    for c in (0, 1):
        word = b["eta"][:, c].astype(np.float64)
        met = (comp == 0) | (comp == c + 1)
        lam = met & (word == DIFFUSE)
        fc = np.where((lam & up)[:, None], kd / np.pi * co[:, None], 0.0)
        pc = np.where(lam & up, co / np.pi, 0.0)
        cond = met & (word >= 0)
        if cond.any():
            r = np.flatnonzero(cond)
            fa, pa, known = children(kd[r], word[r].astype(np.int64), n[r], wi[r], wo[r])
            if child_kinds:
                kinds = table["kind"][word[r].astype(np.int64)]
                known = known & np.isin(kinds, (abi.GVPM_BSDF_ROUGHCONDUCTOR, abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO))
            fc[r], pc[r] = np.where((known & up[r])[:, None], fa, 0.0), np.where(known & up[r], pa, 0.0)
            defined[r] &= known
        f += w[:, c, None] * fc
        pdf += p[:, c] * pc
    return np.where(defined[:, None], f, 0.0), np.where(defined, pdf, 0.0), defined


def phong_world_with_mixture(kd, index, n, wi, wo, _inner=indep_phong_dist.phong_world_with_phong_dist):
    table = indep_statements.BSDFS
    index = np.asarray(index)
    f, pdf, known = _inner(kd, index, n, wi, wo)
    if not table.size:
        return f, pdf, known
    inside = (index >= 0) & (index < table.size)
    idx = np.where(inside, index, 0).astype(np.int64)
    mine = inside & is_mixture(table)[idx]
    if mine.any():
        r = np.flatnonzero(mine)
        bc = lambda a: np.broadcast_to(a, f.shape)[r]
        fa, pa, defined = mixture_world(table, bc(kd), idx[r], bc(n), bc(wi), bc(wo), _inner)
        f, pdf, known = f.copy(), pdf.copy(), known.copy()
        f[r], pdf[r], known[r] = fa, pa, defined
    return f, pdf, known


def install(monkeypatch):
    monkeypatch.setattr(indep_statements, "phong_world", phong_world_with_mixture)
