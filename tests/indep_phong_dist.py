"""Second statement of the Phong / Ashikhmin-Shirley microfacet distribution (GVPM_MICROFACET_PHONG; include/gvpm_hip.h) under the four
kinds that carry a `distribution` -- GVPM_BSDF_ROUGHCONDUCTOR, GVPM_BSDF_ROUGHCONDUCTOR_ANISO, GVPM_BSDF_ROUGHPLASTIC and
GVPM_BSDF_ROUGHDIELECTRIC -- in numpy, fp64, WORLD space, vectorised over rows like indep_statements.phong_world, and a wrapper with
phong_world's signature that answers the rows naming such heads itself and hands every other row on to the statements of the
sibling modules (indep_plastic, indep_aniso, indep_dielectric).  The frozen oracle cannot judge these entries: it reads any
non-GGX conductor as Beckmann.

Written from src/bsdfs/microfacet.h (eval :191-232, pdfAll, sampleAll :349-375, smithG1 :477-518, projectRoughness :541-551,
interpolatePhongExponent :553-565, computePhongExponent :700-704) and the plugins (roughconductor.cpp:257-319, roughplastic.cpp:
326-437, roughdielectric.cpp:270-422):

  e(alpha) = max(2 / alpha^2 - 2, 0);  eU = e(alphaU), eV = e(alphaV)
  D(m)     = sqrt((eU + 2)(eV + 2)) / (2 pi) cos(theta_m)^e,  0 at or below the horizon and where D cos(theta_m) < 1e-20
             e = eU where alphaU == alphaV or sin^2(theta_m) <= 2^-128, else (eU m.x^2 + eV m.y^2) / sin^2(theta_m)
  G1(v, m) = Beckmann's rational fit at a = 1 / (alpha(v) tan(theta_v)), alpha(v) the roughness projected on v's azimuth; 0 where
             (v . m) cos(theta_v) <= 0, 1 at perpendicular incidence
  pdf(m)   = D cos(theta_m)  (all normals: the reference forces sampleVisible off for this distribution, :140-144)

The rough dielectric samples the half vector at alpha (1.2 - 0.2 sqrt(|cos_i|)); scaleAlpha (:178-183) recomputes the exponent.

Transmitted records reach the statements mirrored, as indep_dielectric arranges it (mirrored_case there; index + table size).

NEAR counts, over all rows answered since reset_near(), the reconnections within rounding of an fp32 decision: D cos_H -- and for
the dielectric D' cos_H -- within a relative 1e-3 of 1e-20 (the band indep_dielectric uses), and the dielectric's own: cos^2(theta_T)
within 1e-6 of 0, |N . wi| < 1e-6, |wi + eta wo|^2 within a factor 2 of 1e-12."""
import numpy as np

import indep_aniso
import indep_dielectric
import indep_plastic
import indep_statements
from gvpm_amd import abi

PHONG = abi.GVPM_MICROFACET_PHONG
KINDS = (abi.GVPM_BSDF_ROUGHCONDUCTOR, abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO, abi.GVPM_BSDF_ROUGHPLASTIC, abi.GVPM_BSDF_ROUGHDIELECTRIC)
RCPOVERFLOW = 2.0 ** -128
NEAR = 0


def reset_near():
    global NEAR
    NEAR = 0
    indep_dielectric.reset_near()


def _dot(a, b):
    return (a * b).sum(-1)


def exponent(alpha):
    """computePhongExponent"""
    alpha = np.asarray(alpha, np.float64)
    return np.maximum(2.0 / (alpha * alpha) - 2.0, 0.0)


def interpolated_exponent(au, av, mx, my, mz):
    eu, ev = exponent(au), exponent(av)
    s2 = 1.0 - mz * mz
    with np.errstate(invalid="ignore", divide="ignore"):
        e = (eu * mx * mx + ev * my * my) / s2
    return np.where((np.asarray(au) == np.asarray(av)) | (s2 <= RCPOVERFLOW), eu, e)


def distribution(au, av, mx, my, mz):
    """(D, D cos before the cut) of the unit micro-normal (mx, my, mz) in the surface's frame"""
    eu, ev = exponent(au), exponent(av)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        d = np.sqrt((eu + 2.0) * (ev + 2.0)) / (2.0 * np.pi) * np.power(np.where(mz > 0, mz, 1.0), interpolated_exponent(au, av, mx, my, mz))
        raw = np.where(mz > 0, d * mz, 0.0)
    return np.where((mz > 0) & (raw >= 1e-20), d, 0.0), raw


def smith_g1(au, av, vx, vy, vz, v_dot_m):
    with np.errstate(invalid="ignore", divide="ignore"):
        s2 = 1.0 - vz * vz
        inv = 1.0 / s2
        alpha = np.where((np.asarray(au) == np.asarray(av)) | ~(inv > 0), au, np.sqrt(vx * vx * inv * au * au + vy * vy * inv * av * av))
        tan = np.abs(np.sqrt(np.maximum(s2, 0.0)) / vz)
        a = 1.0 / (alpha * tan)
        g = np.where(a >= 1.6, 1.0, (3.535 * a + 2.181 * a * a) / (1.0 + 2.276 * a + 2.577 * a * a))
        g = np.where(tan == 0, 1.0, g)
    return np.where(v_dot_m * vz > 0, g, 0.0)


def any_tangent(n):
    """a vector that spans a frame with each row of n (the isotropic kinds have no tangent: any frame serves)"""
    n = np.asarray(n, np.float64)
    axis = np.argmin(np.abs(n), axis=-1)
    return np.eye(3)[axis]


def _count_near(mask):
    global NEAR
    NEAR += int(np.asarray(mask).sum())


def _band(raw):
    return np.abs(raw - 1e-20) <= 1e-23


def fresnel_conductor(cos_i, eta, k):
    """unpolarised reflectance of the complex index eta + i k, per channel, in complex arithmetic"""
    nn = eta + 1j * k
    c = cos_i[..., None].astype(np.complex128)
    root = np.sqrt(nn * nn - (1.0 - c * c))
    rs = (c - root) / (c + root)
    rp = (nn * nn * c - root) / (nn * nn * c + root)
    return 0.5 * (np.abs(rs) ** 2 + np.abs(rp) ** 2)


def _reflection_terms(au, av, tangent, n, wi, wo, count):
    """what RoughConductor and RoughPlastic share: (D, G, cos_h, wi . h, wo . h, ci, co, up, spans)"""
    u, v, spans = indep_aniso.frame(tangent, n)
    ci, co = _dot(n, wi), _dot(n, wo)
    up = (ci > 0) & (co > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = wi + wo
        h = h / np.linalg.norm(h, axis=-1, keepdims=True)
    loc = lambda d: (_dot(d, u), _dot(d, v), _dot(d, n))
    hx, hy, hz = loc(h)
    wih, woh = _dot(wi, h), _dot(wo, h)
    D, raw = distribution(au, av, hx, hy, hz)
    if count:
        _count_near(up & spans & _band(raw))
    G = smith_g1(au, av, *loc(wi), wih) * smith_g1(au, av, *loc(wo), woh)
    return D, G, hz, wih, woh, ci, co, up, spans


def conductor_rows(ks, au, av, tangent, eta, k, n, wi, wo, count=True):
    """RoughConductor::eval (x cos is in it: F D G / (4 cos_i)) and ::pdf without visible normals: (f [k, 3], pdf [k], defined [k])"""
    D, G, ch, wih, woh, ci, co, up, spans = _reflection_terms(au, av, tangent, n, wi, wo, count)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = ks * fresnel_conductor(wih, eta, k) * (D * G / (4.0 * ci))[..., None]
        pdf = D * ch / (4.0 * np.abs(woh))
    ok = up & spans & (D > 0)
    return np.where(ok[..., None], f, 0.0), np.where(ok, pdf, 0.0), spans


def plastic_rows(ks, alpha, w, eta, fdr, comp, nonlinear, slices, kd, n, wi, wo, count=True):
    """RoughPlastic::eval and ::pdf x pdfComponent (comp 0: both components, 1: the glossy one alone, 2: the diffuse one alone):
    (f [k, 3], pdf [k], defined [k]); undefined: the probability of the glossy component is 0 / 0"""
    D, G, ch, wih, woh, ci, co, up, _ = _reflection_terms(alpha, alpha, any_tangent(n), n, wi, wo, count)
    cic, coc = np.where(up, ci, 1.0), np.where(up, co, 1.0)
    Ti, To = indep_plastic.transmittance(slices, cic), indep_plastic.transmittance(slices, coc)
    pS = indep_plastic.prob_specular(Ti, w)
    defined = np.isfinite(pS)
    pS = np.where(defined, pS, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        on = (comp != 2) & (D > 0)
        spec = np.where(on, indep_plastic.fresnel_dielectric(np.abs(wih), eta) * D * G / (4.0 * cic), 0.0)
        pdf_h = np.where(on, D * ch / (4.0 * woh), 0.0)
    d_on = np.where(comp == 1, 0.0, 1.0)
    kdp = np.where(nonlinear[..., None], kd / (1.0 - kd * fdr[..., None]), kd / (1.0 - fdr[..., None]))
    f = ks * spec[..., None] + kdp * (coc / np.pi * Ti * To / (eta * eta) * d_on)[..., None]
    pdf = pS * pdf_h + (1.0 - pS) * coc / np.pi * d_on
    return np.where(up[..., None], f, 0.0), np.where(up, pdf, 0.0), defined | ~up


def dielectric_rows(ks, kt, alpha, m_eta, N, wi, wo, count=True):
    """RoughDielectric::eval (EImportance) and ::pdf in the frame of normal N, m_eta = the index on the side N points away from over
    the index on the side it points to (indep_dielectric.reference_rows with this distribution): (f [k, 3], pdf [k], defined [k])"""
    ci, co = _dot(N, wi), _dot(N, wo)
    reflect = ci * co > 0
    eta = np.where(ci > 0, m_eta, 1.0 / m_eta)
    u, v, _ = indep_aniso.frame(any_tangent(N), N)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        h = np.where(reflect[..., None], wi + wo, wi + wo * eta[..., None])
        hh = _dot(h, h)
        defined = hh >= 1e-12
        h = h / np.sqrt(np.where(defined, hh, 1.0))[..., None]
        dwh = np.where(reflect, 1.0 / (4.0 * _dot(wo, h)), eta * eta * _dot(wo, h) / (_dot(wi, h) + eta * _dot(wo, h)) ** 2)
        h = h * np.sign(_dot(N, h))[..., None]
        loc = lambda d: (_dot(d, u), _dot(d, v), _dot(d, N))
        hx, hy, cos_h = loc(h)
        wih, woh = _dot(wi, h), _dot(wo, h)
        D, raw = distribution(alpha, alpha, hx, hy, cos_h)
        F, ct2 = indep_dielectric.fresnel_ext(wih, m_eta)
        G = smith_g1(alpha, alpha, *loc(wi), wih) * smith_g1(alpha, alpha, *loc(wo), woh)
        sd = wih + eta * woh
        value = np.where(reflect, F * D * G / (4.0 * np.abs(ci)), np.abs((1.0 - F) * D * G * eta * eta * wih * woh / (ci * sd * sd)))
        f = np.where(reflect[..., None], ks, kt) * value[..., None]
        f = np.where(((D == 0) | (ci == 0))[..., None], 0.0, f)
        alpha_s = alpha * (1.2 - 0.2 * np.sqrt(np.abs(ci)))
        Ds, raw_s = distribution(alpha_s, alpha_s, hx, hy, cos_h)
        pdf = np.abs(Ds * cos_h * np.where(reflect, F, 1.0 - F) * dwh)
        pdf = np.where(np.isfinite(pdf), pdf, 0.0)
    if count:
        _count_near(_band(raw) | _band(raw_s) | (np.abs(ct2) < 1e-6) | (np.abs(ci) < 1e-6) | (~reflect & (hh > 0.5e-12) & (hh < 2e-12)))
    return np.where(defined[..., None], f, 0.0), np.where(defined, pdf, 0.0), defined


def phong_dist_world(table, kd, index, n, wi, wo, count=True):
    """(f cos [k, 3], pdf [k], defined [k]) of rows that name heads of `table` whose distribution is the Phong one; n: the record's
    normal, wi the true incident direction (a dielectric's on either side)"""
    index = np.asarray(index, np.int64)
    b = table[index]
    raw = np.ascontiguousarray(table).view(np.float32).reshape(-1, 16)
    f64 = lambda name: b[name].astype(np.float64)
    kind = b["kind"]
    k = index.size
    f, pdf, defined = np.zeros((k, 3)), np.zeros(k), np.zeros(k, bool)
    alpha = f64("exponent")
    cond = np.isin(kind, (abi.GVPM_BSDF_ROUGHCONDUCTOR, abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO))
    if cond.any():
        r = np.flatnonzero(cond)
        aniso = kind[r] == abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO
        frame_row = raw[np.minimum(index[r] + 1, table.size - 1)].astype(np.float64)
        av = np.where(aniso, frame_row[:, 3], alpha[r])
        tangent = np.where(aniso[:, None], frame_row[:, 0:3], any_tangent(n[r]))
        f[r], pdf[r], defined[r] = conductor_rows(f64("specular")[r], alpha[r], av, tangent, f64("eta")[r], f64("k")[r], n[r], wi[r], wo[r], count)
    pl = kind == abi.GVPM_BSDF_ROUGHPLASTIC
    if pl.any():
        r = np.flatnonzero(pl)
        rows = (index[r, None] + 1) * 16 + np.arange(abi.GVPM_RTRANS_KNOTS)[None, :]
        f[r], pdf[r], defined[r] = plastic_rows(f64("specular")[r], alpha[r], f64("specular_sampling_weight")[r], f64("eta")[r, 0],
                                                f64("eta")[r, 1], b["k"][r, 0].astype(np.int64), b["k"][r, 1] != 0,
                                                raw.reshape(-1)[rows].astype(np.float64), kd[r], n[r], wi[r], wo[r], count)
    di = kind == abi.GVPM_BSDF_ROUGHDIELECTRIC
    if di.any():
        r = np.flatnonzero(di)
        eta_entry = f64("eta")[r, 0]
        m_eta = np.where(_dot(n[r], wi[r]) > 0, eta_entry, 1.0 / eta_entry)
        fa, pa, da = dielectric_rows(f64("specular")[r], f64("k")[r], alpha[r], m_eta, n[r], wi[r], wo[r], count)
        up = _dot(n[r], wo[r]) > 0
        f[r], pdf[r], defined[r] = np.where(up[:, None], fa, 0.0), np.where(up, pa, 0.0), da
    return f, pdf, defined


def _others(kd, index, n, wi, wo):
    """the statements of every other kind, composed: dielectric over anisotropic over plastic over indep_statements'"""
    plastics = indep_plastic.phong_world_with_plastics
    aniso = lambda *a: indep_aniso.phong_world_with_aniso(*a, _inner=plastics)
    return indep_dielectric.phong_world_with_dielectric(kd, index, n, wi, wo, _inner=aniso)


def is_phong_dist(table):
    """which entries of a table are heads of the four kinds under the Phong distribution"""
    if not table.size:
        return np.zeros(0, bool)
    return abi.bsdf_heads(table) & np.isin(table["kind"], KINDS) & (table["distribution"] == PHONG)


def phong_world_with_phong_dist(kd, index, n, wi, wo, _inner=_others):
    table = indep_statements.BSDFS
    index = np.asarray(index)
    f, pdf, known = _inner(kd, index, n, wi, wo)
    if not table.size:
        return f, pdf, known
    flipped = (index >= table.size) & (index < 2 * table.size)     # (a transmitted record, mirrored by indep_dielectric.mirrored)
    idx = np.where(flipped, index - table.size, index)
    inside = (idx >= 0) & (idx < table.size)
    idx = np.where(inside, idx, 0).astype(np.int64)
    mine = inside & is_phong_dist(table)[idx]
    mine &= ~flipped | (table["kind"][idx] == abi.GVPM_BSDF_ROUGHDIELECTRIC)
    if mine.any():
        r = np.flatnonzero(mine)
        bc = lambda a: np.broadcast_to(a, f.shape)[r]
        nn, ww = bc(n), bc(wi)
        ww = np.where(flipped[r][:, None], ww - 2.0 * nn * _dot(nn, ww)[:, None], ww)
        fa, pa, defined = phong_dist_world(table, bc(kd), idx[r], nn, ww, bc(wo))
        f, pdf, known = f.copy(), pdf.copy(), known.copy()
        f[r], pdf[r], known[r] = fa, pa, defined
    return f, pdf, known


def install(monkeypatch):
    monkeypatch.setattr(indep_statements, "phong_world", phong_world_with_phong_dist)
