"""Second statement of the rough-dielectric parent (GVPM_BSDF_ROUGHDIELECTRIC; include/gvpm_hip.h) in numpy, fp64, WORLD space,
vectorised over rows like indep_statements.phong_world, written from the text of src/bsdfs/roughdielectric.cpp:270-422,
src/bsdfs/microfacet.h:191-232,404-407,462-522 and src/libcore/util.cpp:659-689 -- and a wrapper with phong_world's signature
that answers the rows naming such entries itself and hands every other row on.

reference_rows is the reference's eval / pdf AS WRITTEN: a frame normal N, the plugin's m_eta (the index on the side N points
away from over the index on the side it points to), SIGNED cosines cosTheta(wi) and cosTheta(wo), m_eta or m_invEta picked by
the sign of cosTheta(wi), the half vector flipped into N's hemisphere.  dielectric_world applies it to a record and its table
entry: N = the record's normal (the side the photon LEFT, include/gvpm_hip.h), and since the entry's eta[0] is the index
behind the surface over the index on wi's side, m_eta in that frame is eta[0] where N . wi > 0 and 1 / eta[0] where N . wi < 0.
(The device works in wi's frame instead; that the reference's text gives the same value in either frame is asserted by
tests/test_dielectric_parents.py.)

How the statements of indep_statements meet transmitted records -- the choice the module makes: indep_statements.py stays as
it is, and it tests cos_wi > 0 before it asks phong_world.  So the statements run on a COPY of the records (mirrored()) in
which parent_wi of the records with N . wi < 0 that name a dielectric entry is mirrored about the surface, wi - 2 N (N . wi),
in float64, and parent_g names entry + table size; the wrapper (phong_world_with_dielectric) reads that offset as "mirrored",
mirrors wi back and evaluates the entry.  Nothing else of the statements reads parent_wi of a surface parent.  Rows of any
other kind are handed on unchanged: such a record with N . wi < 0 is not mirrored and fails there as ever.

NEAR counts, over all rows answered since reset_near(), the reconnections within rounding of an fp32 decision this kind adds:
D cos_H or D' cos_H (the distribution at the scaled alpha) within a relative 1e-3 of 1e-20; cos^2(theta_T) within 1e-6 of 0
(the edge of total internal reflection); |N . wi| < 1e-6; |wi + eta wo|^2 within a factor 2 of 1e-12."""
import copy

import numpy as np

import indep_statements
from gvpm_amd import abi

KIND = abi.GVPM_BSDF_ROUGHDIELECTRIC
NEAR = 0


def reset_near():
    global NEAR
    NEAR = 0


def _dot(a, b):
    return (a * b).sum(-1)


def distribution(ggx, alpha, cos_h):
    """(D, D cos_H before the cut) -- MicrofacetDistribution::eval, isotropic: zero at or below the horizon and where
    D cos_H < 1e-20"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        c2 = cos_h * cos_h
        e = (1.0 - c2) / (alpha * alpha * c2)
        root = (1.0 + e) * c2
        d = np.where(ggx, 1.0 / (np.pi * alpha * alpha * root * root), np.exp(-e) / (np.pi * alpha * alpha * c2 * c2))
        raw = np.where(cos_h > 0, d * cos_h, 0.0)
        return np.where((cos_h > 0) & (raw >= 1e-20), d, 0.0), raw


def smith_g1(ggx, alpha, cos_v, v_dot_m):
    """MicrofacetDistribution::smithG1 by cosines: zero where dot(v, m) cosTheta(v) <= 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        tan = np.abs(np.sqrt(np.maximum(1.0 - cos_v * cos_v, 0.0)) / cos_v)
        a = 1.0 / (alpha * tan)
        beck = np.where(a >= 1.6, 1.0, (3.535 * a + 2.181 * a * a) / (1.0 + 2.276 * a + 2.577 * a * a))
        g = np.where(ggx, 2.0 / (1.0 + np.hypot(1.0, alpha * tan)), beck)
        g = np.where(tan == 0, 1.0, g)
        return np.where(v_dot_m * cos_v > 0, g, 0.0)


def fresnel_ext(cos_i, eta):
    """(F, cos^2(theta_T)) -- fresnelDielectricExt(cosThetaI, eta) for a cosine of either sign"""
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.where(cos_i > 0, 1.0 / eta, eta)
        ct2 = 1.0 - (1.0 - cos_i * cos_i) * scale * scale
        ci, ct = np.abs(cos_i), np.sqrt(np.maximum(ct2, 0.0))
        rs = (ci - eta * ct) / (ci + eta * ct)
        rp = (eta * ci - ct) / (eta * ci + ct)
        f = np.where(ct2 <= 0, 1.0, 0.5 * (rs * rs + rp * rp))
        return np.where(eta == 1.0, 0.0, f), ct2


def reference_rows(ks, kt, alpha, m_eta, ggx, visible, N, wi, wo, count=True):
    """RoughDielectric::eval (EImportance: factor = 1) and ::pdf with bRec.component = -1 in the frame of normal N:
    (eval [k, 3], pdf [k], defined [k]); undefined: no half vector (|wi + eta wo|^2 < 1e-12)"""
    global NEAR
    ci, co = _dot(N, wi), _dot(N, wo)
    reflect = ci * co > 0
    eta = np.where(ci > 0, m_eta, 1.0 / m_eta)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        h = np.where(reflect[..., None], wi + wo, wi + wo * eta[..., None])
        hh = _dot(h, h)
        defined = hh >= 1e-12
        h = h / np.sqrt(np.where(defined, hh, 1.0))[..., None]
        dwh = np.where(reflect, 1.0 / (4.0 * _dot(wo, h)), eta * eta * _dot(wo, h) / (_dot(wi, h) + eta * _dot(wo, h)) ** 2)
        h = h * np.sign(_dot(N, h))[..., None]
        cos_h, wih, woh = _dot(N, h), _dot(wi, h), _dot(wo, h)
        D, raw = distribution(ggx, alpha, cos_h)
        F, ct2 = fresnel_ext(wih, m_eta)
        G = smith_g1(ggx, alpha, ci, wih) * smith_g1(ggx, alpha, co, woh)
        sd = wih + eta * woh
        value = np.where(reflect, F * D * G / (4.0 * np.abs(ci)), np.abs((1.0 - F) * D * G * eta * eta * wih * woh / (ci * sd * sd)))
        f = np.where(reflect[..., None], ks, kt) * value[..., None]
        f = np.where(((D == 0) | (ci == 0))[..., None], 0.0, f)
        # pdf: the half vector's density under the sign-corrected wi, times F or 1 - F, times the Jacobian
        alpha_s = alpha * (1.2 - 0.2 * np.sqrt(np.abs(ci)))
        Ds, raw_s = distribution(ggx, alpha_s, cos_h)
        swi = np.sign(ci)
        prob = np.where(visible, np.where(ci == 0, 0.0, smith_g1(ggx, alpha, swi * ci, swi * wih) * np.abs(wih) * D / np.abs(ci)), Ds * cos_h)
        pdf = np.abs(prob * np.where(reflect, F, 1.0 - F) * dwh)
        pdf = np.where(np.isfinite(pdf), pdf, 0.0)
    if count:
        near = (np.abs(raw - 1e-20) <= 1e-23) | (~visible & (np.abs(raw_s - 1e-20) <= 1e-23)) | (np.abs(ct2) < 1e-6) | (np.abs(ci) < 1e-6) | \
               (~reflect & (hh > 0.5e-12) & (hh < 2e-12))
        NEAR += int(near.sum())
    return np.where(defined[..., None], f, 0.0), np.where(defined, pdf, 0.0), defined


def dielectric_world(table, index, n, wi, wo, count=True):
    """(eval [k, 3], pdf [k], defined [k]) of rows that name rough-dielectric entries of `table`: n the record's normal (the
    side the photon left: n . wo > 0 is the caller's test), wi the true incident direction, on either side"""
    b = table[index]
    f64 = lambda name: b[name].astype(np.float64)
    eta_entry = f64("eta")[..., 0]
    m_eta = np.where(_dot(n, wi) > 0, eta_entry, 1.0 / eta_entry)
    return reference_rows(f64("specular"), f64("k"), f64("exponent"), m_eta, b["distribution"] == abi.GVPM_MICROFACET_GGX,
                          b["sample_visible"] != 0, n, wi, wo, count)


def is_transmitted(records, table):
    """records that name a rough-dielectric entry of `table` and whose light arrived on the far side of their normal"""
    gl = (records.flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
    idx = np.where(gl, records.parent_g, 0).astype(np.int64)
    inside = gl & (idx >= 0) & (idx < table.size)
    diel = inside & (table["kind"][np.where(inside, idx, 0)] == KIND) if table.size else inside & False
    return diel & (_dot(records.parent_n.astype(np.float64), records.parent_wi.astype(np.float64)) < 0), diel


def mirrored(records, table):
    """the copy of photon / beam records the statements of indep_statements run on (module docstring)"""
    out = copy.deepcopy(records)
    tr, _ = is_transmitted(records, table)
    n, wi = records.parent_n.astype(np.float64), records.parent_wi.astype(np.float64)
    out.parent_wi = np.where(tr[:, None], wi - 2.0 * n * _dot(n, wi)[:, None], wi)
    out.parent_g = np.where(tr, records.parent_g.astype(np.float64) + table.size, records.parent_g.astype(np.float64))
    return out


def mirrored_case(c, records="ph"):
    out = copy.copy(c)
    setattr(out, records, mirrored(getattr(c, records), c.bsdfs))
    return out


def phong_world_with_dielectric(kd, index, n, wi, wo, _inner=indep_statements.phong_world):
    """indep_statements.phong_world for tables that also carry rough-dielectric entries: rows naming one (index + table size:
    the row's wi was mirrored about the surface by mirrored(), and is mirrored back here) are answered here, the rest is
    handed on"""
    table = indep_statements.BSDFS
    index = np.asarray(index)
    f, pdf, known = _inner(kd, index, n, wi, wo)
    if not table.size:
        return f, pdf, known
    flipped = (index >= table.size) & (index < 2 * table.size)
    idx = np.where(flipped, index - table.size, index)
    inside = (idx >= 0) & (idx < table.size)
    idx = np.where(inside, idx, 0).astype(np.int64)
    diel = inside & (table["kind"][idx] == KIND)
    if diel.any():
        r = np.nonzero(diel)[0]
        nn, ww = np.broadcast_to(n, f.shape)[r], np.broadcast_to(wi, f.shape)[r]
        ww = np.where(flipped[r][:, None], ww - 2.0 * nn * _dot(nn, ww)[:, None], ww)
        fa, pa, defined = dielectric_world(table, idx[r], nn, ww, np.broadcast_to(wo, f.shape)[r])
        up = _dot(nn, np.broadcast_to(wo, f.shape)[r]) > 0
        f, pdf, known = f.copy(), pdf.copy(), known.copy()
        f[r], pdf[r], known[r] = np.where(up[:, None], fa, 0.0), np.where(up, pa, 0.0), defined
    return f, pdf, known


def install(monkeypatch):
    monkeypatch.setattr(indep_statements, "phong_world", phong_world_with_dielectric)
