"""Second statement of the two plastic parents (GVPM_BSDF_ROUGHPLASTIC, GVPM_BSDF_PLASTIC; include/gvpm_hip.h) in numpy, fp64,
WORLD space, vectorised over rows like indep_statements.phong_world -- and a wrapper with phong_world's signature that
answers the rows naming such entries itself and hands every other row on.  Installed over indep_statements.phong_world
(monkeypatch.setattr), the BRE-3D / G-VPM / G-Beams statements of that module state whole gathers for tables that carry
the new kinds.

Rough plastic (Walter et al. 2007 coating over a diffuse base, as src/bsdfs/roughplastic.cpp composes it):
  f cos = ks F(wi . h) D(h) G1(wi) G1(wo) / (4 n . wi)  +  kd' / pi (n . wo) T(n . wi) T(n . wo) / eta^2
  pdf   = pS pdf_h + (1 - pS) (n . wo) / pi,   pS = p w / (p w + (1 - p)(1 - w)),  p = 1 - T(n . wi)
with h the normalised half vector, F the unpolarised Fresnel reflectance of a dielectric (real arithmetic), D / G1 the
textbook Beckmann / GGX forms (Beckmann's G1: Walter's rational fit), pdf_h = D (n . h) / (4 wo . h) or D G1(wi) / (4 n . wi)
(visible normals), T the tabulated transmittance -- a Catmull-Rom spline through 100 values over cos^(1/4) -- clamped to
[0, 1], and kd' = kd / (1 - kd Fdr) or kd / (1 - Fdr).  An entry met through ONE component: that term of each.
Smooth plastic, diffuse component: T(c) = 1 - F(c); f cos = the diffuse term above, pdf = (1 - pS) (n . wo) / pi."""
import numpy as np

import indep_statements
from gvpm_amd import abi

KNOTS = abi.GVPM_RTRANS_KNOTS


def fresnel_dielectric(c, eta):
    """unpolarised reflectance of a dielectric of relative index eta >= 1 seen from outside under cosine c >= 0"""
    c = np.asarray(c, np.float64)
    g = np.sqrt(eta * eta - (1.0 - c * c))
    rs = (c - g) / (c + g)
    rp = (eta * eta * c - g) / (eta * eta * c + g)
    return 0.5 * (rs * rs + rp * rp)


def catmull_rom(values, x):
    """the spline through values[..., 0..m-1] at uniform knots j / (m - 1), evaluated at x in [0, 1]; knot derivatives are central
    differences, one-sided at the two ends; values: [rows, m] (one table per row) or [m]"""
    values = np.asarray(values, np.float64)
    if values.ndim == 1:
        values = np.broadcast_to(values, np.shape(x) + values.shape)
    m = values.shape[-1]
    t = np.asarray(x, np.float64) * (m - 1)
    k = np.minimum(np.floor(t).astype(np.int64), m - 2)
    take = lambda j: np.take_along_axis(values, np.clip(j, 0, m - 1)[..., None], -1)[..., 0]
    f0, f1 = take(k), take(k + 1)
    d0 = np.where(k > 0, 0.5 * (f1 - take(k - 1)), f1 - f0)
    d1 = np.where(k + 2 < m, 0.5 * (take(k + 2) - f0), f1 - f0)
    u = t - k
    h00, h01 = 2 * u ** 3 - 3 * u ** 2 + 1, -2 * u ** 3 + 3 * u ** 2
    h10, h11 = u ** 3 - 2 * u ** 2 + u, u ** 3 - u ** 2
    return h00 * f0 + h01 * f1 + h10 * d0 + h11 * d1


def transmittance(slices, c):
    return np.clip(catmull_rom(slices, np.sqrt(np.sqrt(np.clip(c, 0.0, 1.0)))), 0.0, 1.0)


def heads_of(table):
    """which entries of a table are heads (nameable by a photon): not the raw entries behind a rough-plastic head"""
    head = np.zeros(table.size, bool)
    i = 0
    while i < table.size:
        head[i] = True
        i += 1 + (abi.GVPM_RTRANS_ENTRIES if table["kind"][i] == abi.GVPM_BSDF_ROUGHPLASTIC else 0)
    return head


def prob_specular(T_i, w):
    p = 1.0 - T_i
    with np.errstate(invalid="ignore", divide="ignore"):
        return p * w / (p * w + (1.0 - p) * (1.0 - w))


def plastic_world(table, kd, index, n, wi, wo):
    """(f cos [k, 3], pdf x pdfComponent [k], defined [k]) of rows that name plastic heads of `table`; defined = False where pS is 0 / 0"""
    b = table[index]
    raw = np.ascontiguousarray(table).view(np.float32).reshape(-1, 16)
    rough = b["kind"] == abi.GVPM_BSDF_ROUGHPLASTIC
    ks, al, w = b["specular"].astype(np.float64), b["exponent"].astype(np.float64), b["specular_sampling_weight"].astype(np.float64)
    eta, fdr = b["eta"][..., 0].astype(np.float64), b["eta"][..., 1].astype(np.float64)
    comp, nonlinear = b["k"][..., 0].astype(np.int64), b["k"][..., 1] != 0
    ci, co = (n * wi).sum(-1), (n * wo).sum(-1)
    up = (ci > 0) & (co > 0)
    cic, coc = np.where(up, ci, 1.0), np.where(up, co, 1.0)
    # transmittances: the slice behind a rough head (entries index + 1 .. + 7, 100 floats), 1 - Fresnel for the smooth one
    Ti, To = 1.0 - fresnel_dielectric(cic, eta), 1.0 - fresnel_dielectric(coc, eta)
    if rough.any():
        r = np.nonzero(rough)[0]
        rows = (np.asarray(index)[r, None] + 1) * 16 + np.arange(KNOTS)[None, :]
        sl = raw.reshape(-1)[rows].astype(np.float64)
        Ti[r], To[r] = transmittance(sl, cic[r]), transmittance(sl, coc[r])
    pS = prob_specular(Ti, w)
    defined = np.isfinite(pS)
    pS = np.where(defined, pS, 0.0)
    # the coating
    spec, pdf_h = np.zeros(ci.shape), np.zeros(ci.shape)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        h = wi + wo
        h = h / np.linalg.norm(h, axis=-1, keepdims=True)
        ch, wih, woh = (n * h).sum(-1), (wi * h).sum(-1), (wo * h).sum(-1)
        ggx = b["distribution"] == abi.GVPM_MICROFACET_GGX
        c2 = ch * ch
        t2 = (1.0 - c2) / c2
        a2 = np.where(rough, al * al, 1.0)
        D = np.where(ggx, a2 / (np.pi * (c2 * (a2 - 1.0) + 1.0) ** 2), np.exp(-t2 / a2) / (np.pi * a2 * c2 * c2))
        D = np.where((ch > 0) & (D * ch >= 1e-20), D, 0.0)

        def g1(cv, vh):
            tan = np.sqrt(np.maximum(1.0 - cv * cv, 0.0)) / np.abs(cv)
            aa = 1.0 / (np.sqrt(a2) * tan)
            beck = np.where(aa >= 1.6, 1.0, (3.535 * aa + 2.181 * aa * aa) / (1.0 + 2.276 * aa + 2.577 * aa * aa))
            g = np.where(ggx, 2.0 / (1.0 + np.sqrt(1.0 + a2 * tan * tan)), beck)
            g = np.where(tan == 0, 1.0, g)
            return np.where(vh * cv > 0, g, 0.0)

        g1i, g1o = g1(cic, wih), g1(coc, woh)
        F = fresnel_dielectric(np.abs(wih), eta)
        on = rough & (D > 0) & (comp != 2)
        spec = np.where(on, F * D * g1i * g1o / (4.0 * cic), 0.0)
        pdf_h = np.where(on, np.where(b["sample_visible"] != 0, D * g1i / (4.0 * cic), D * ch / (4.0 * np.abs(woh))), 0.0)
    # the base
    d_on = np.where(comp == 1, 0.0, 1.0)
    kdp = np.where(nonlinear[..., None], kd / (1.0 - kd * fdr[..., None]), kd / (1.0 - fdr[..., None]))
    f = ks * spec[..., None] + kdp * (coc / np.pi * Ti * To / (eta * eta) * d_on)[..., None]
    pdf = pS * pdf_h + (1.0 - pS) * coc / np.pi * d_on
    return np.where(up[..., None], f, 0.0), np.where(up, pdf, 0.0), defined | ~up


def phong_world_with_plastics(kd, index, n, wi, wo, _inner=indep_statements.phong_world):
    """indep_statements.phong_world for tables that also carry the plastic kinds: rows naming a plastic head are answered
    here, rows naming a raw slice entry (or a plastic whose pS is undefined) are unknown, the rest is handed on"""
    table = indep_statements.BSDFS
    index = np.asarray(index)
    f, pdf, known = _inner(kd, index, n, wi, wo)
    if not table.size:
        return f, pdf, known
    inside = (index >= 0) & (index < table.size)
    idx = np.where(inside, index, 0).astype(np.int64)
    head = heads_of(table)[idx] & inside
    plastic = head & np.isin(table["kind"][idx], (abi.GVPM_BSDF_ROUGHPLASTIC, abi.GVPM_BSDF_PLASTIC))
    known = known & head
    if plastic.any():
        r = np.nonzero(plastic)[0]
        kd_r = np.broadcast_to(kd, f.shape)[r]
        fp, pp, defined = plastic_world(table, kd_r, idx[r], np.broadcast_to(n, f.shape)[r], np.broadcast_to(wi, f.shape)[r],
                                        np.broadcast_to(wo, f.shape)[r])
        f, pdf, known = f.copy(), pdf.copy(), known.copy()
        f[r], pdf[r], known[r] = fp, pp, defined
    return f, pdf, known


def install(monkeypatch):
    monkeypatch.setattr(indep_statements, "phong_world", phong_world_with_plastics)
