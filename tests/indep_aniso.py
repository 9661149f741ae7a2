"""Second statement of the two anisotropic parents (GVPM_BSDF_WARD_ANISO, GVPM_BSDF_ROUGHCONDUCTOR_ANISO; include/gvpm_hip.h) in
numpy, fp64, WORLD space, vectorised over rows like indep_statements.phong_world -- and a wrapper with phong_world's
signature that answers the rows naming such heads itself and hands every other row on.  Installed over
indep_statements.phong_world (monkeypatch.setattr), the BRE-3D / G-VPM / G-Beams statements of that module state whole
gathers for tables that carry the new kinds.

The surface's frame: u = the table's tangent with its part along the normal n removed, normalised; v = n x u.  For a direction d:
(d . u, d . v, d . n).  A tangent (anti)parallel to n (|s - n (n . s)|^2 < 1e-12) spans no frame: such a row is unknown.

Ward (Ward 1992, the anisotropic Gaussian lobe; Duer's and the energy-balanced variants as src/bsdfs/ward.cpp has them): with the
half vector h = wi + wo (any length),
  lobe  = exp(-((h . u / au)^2 + (h . v / av)^2) / (h . n)^2) / (4 pi au av)
  f cos = (ks spec + kd / pi) (n . wo),  spec = lobe / sqrt(ci co) | lobe / (ci co) | lobe 4 |h|^2 / (n . h)^4, dropped below 1e-10
  pdf   = w lobe / ((wi . hn) cos^3(theta_hn)) + (1 - w) (n . wo) / pi,  hn = h / |h|
Rough conductor (Walter et al. 2007 with the anisotropic Beckmann / GGX distributions, src/bsdfs/roughconductor.cpp + microfacet.h):
with the unit half vector m = (mx, my, mz) in the frame,
  D     = exp(-(mx^2 / au^2 + my^2 / av^2) / mz^2) / (pi au av mz^4)   |   1 / (pi au av (mx^2 / au^2 + my^2 / av^2 + mz^2)^2),
          zero where D mz < 1e-20
  G1(d) = the isotropic G1 at the roughness along d's azimuth, a(d)^2 = (dx^2 au^2 + dy^2 av^2) / (dx^2 + dy^2)
  f cos = F D G1(wi) G1(wo) / (4 n . wi),  pdf = D mz / (4 |wo . m|)  or  D G1(wi) / (4 n . wi)  (visible normals)
F: the unpolarised Fresnel reflectance of the complex index eta + i k, in complex arithmetic.

NEAR counts, over all rows answered since reset_near(), the conductor rows whose D mz lies within a relative 1e-3 of the 1e-20
threshold: the one decision these kinds add that fp32 may take the other way."""
import numpy as np

import indep_statements
from gvpm_amd import abi

ANISO = (abi.GVPM_BSDF_WARD_ANISO, abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO)
NEAR = 0


def reset_near():
    global NEAR
    NEAR = 0


def frame(tangent, n):
    """(u [k, 3], v [k, 3], spans [k])"""
    u = tangent - n * (n * tangent).sum(-1, keepdims=True)
    uu = (u * u).sum(-1)
    spans = uu >= 1e-12
    u = u / np.sqrt(np.where(spans, uu, 1.0))[..., None]
    return u, np.cross(n, u), spans


def aniso_rows(ward, ks, au, av, tangent, w, variant, ggx, visible, eta, k, kd, n, wi, wo):
    """the two BSDFs for rows of explicit float64 parameters (ward [k] bool: Ward rows, else conductor rows; ks, eta, k, kd
    [k, 3]; tangent, n, wi, wo [k, 3]): (f cos [k, 3], pdf [k], defined [k])"""
    global NEAR
    u, v, spans = frame(tangent, n)
    ci, co = (n * wi).sum(-1), (n * wo).sum(-1)
    up = (ci > 0) & (co > 0)
    loc = lambda d: ((d * u).sum(-1), (d * v).sum(-1), (d * n).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cic, coc = np.where(up, ci, 1.0), np.where(up, co, 1.0)
        h = wi + wo
        hh = (h * h).sum(-1)
        hx, hy, hz = loc(h)
        # Ward
        lobe = np.exp(-((hx / au) ** 2 + (hy / av) ** 2) / (hz * hz)) / (4.0 * np.pi * au * av)
        spec = np.where(variant == abi.GVPM_WARD_WARD, lobe / np.sqrt(cic * coc),
                        np.where(variant == abi.GVPM_WARD_DUER, lobe / (cic * coc), lobe * 4.0 * hh / hz ** 4))
        spec = np.where(spec > 1e-10, spec, 0.0)
        fw = (ks * spec[..., None] + kd / np.pi) * coc[..., None]
        lh = np.sqrt(hh)
        pw = w * lobe / (((wi * h).sum(-1) / lh) * (hz / lh) ** 3) + (1.0 - w) * coc / np.pi
        # rough conductor
        mx, my, mz = hx / lh, hy / lh, hz / lh
        wim, wom = (wi * h).sum(-1) / lh, (wo * h).sum(-1) / lh
        q = mx * mx / (au * au) + my * my / (av * av)
        D = np.where(ggx, 1.0 / (np.pi * au * av * (q + mz * mz) ** 2), np.exp(-q / (mz * mz)) / (np.pi * au * av * mz ** 4))
        NEAR += int((~ward & up & spans & (mz > 0) & (np.abs(D * mz - 1e-20) <= 1e-23)).sum())
        D = np.where((mz > 0) & (D * mz >= 1e-20), D, 0.0)

        def g1(d, cv, dm):
            dx, dy, _ = loc(d)
            s2 = dx * dx + dy * dy
            a = np.sqrt((dx * dx * au * au + dy * dy * av * av) / np.where(s2 > 0, s2, 1.0))
            tan = np.sqrt(np.maximum(1.0 - cv * cv, 0.0)) / np.abs(cv)
            aa = 1.0 / (a * tan)
            beck = np.where(aa >= 1.6, 1.0, (3.535 * aa + 2.181 * aa * aa) / (1.0 + 2.276 * aa + 2.577 * aa * aa))
            g = np.where(ggx, 2.0 / (1.0 + np.sqrt(1.0 + (a * tan) ** 2)), beck)
            g = np.where((tan == 0) | (s2 <= 0), 1.0, g)
            return np.where(dm * cv > 0, g, 0.0)

        g1i, g1o = g1(wi, cic, wim), g1(wo, coc, wom)
        nn = eta + 1j * k
        cth = wim[..., None].astype(np.complex128)
        root = np.sqrt(nn * nn - (1.0 - cth * cth))
        rs = (cth - root) / (cth + root)
        rp = (nn * nn * cth - root) / (nn * nn * cth + root)
        F = 0.5 * (np.abs(rs) ** 2 + np.abs(rp) ** 2)
        fc = np.where((D > 0)[..., None], ks * F * (D * g1i * g1o / (4.0 * cic))[..., None], 0.0)
        pc = np.where(D > 0, np.where(visible, D * g1i / (4.0 * cic), D * mz / (4.0 * np.abs(wom))), 0.0)
    f = np.where(ward[..., None], fw, fc)
    pdf = np.where(ward, pw, pc)
    ok = up & spans
    return np.where(ok[..., None], f, 0.0), np.where(ok, pdf, 0.0), spans


def aniso_world(table, kd, index, n, wi, wo, tangent=None):
    """(f cos [k, 3], pdf [k], defined [k]) of rows that name anisotropic heads of `table`; tangent: instead of the heads' own"""
    b = table[index]
    raw = np.ascontiguousarray(table).view(np.float32).reshape(-1, 16)[np.asarray(index) + 1].astype(np.float64)
    f64 = lambda name: b[name].astype(np.float64)
    return aniso_rows(b["kind"] == abi.GVPM_BSDF_WARD_ANISO, f64("specular"), f64("exponent"), raw[:, 3],
                      raw[:, 0:3] if tangent is None else np.broadcast_to(np.asarray(tangent, np.float64), raw[:, 0:3].shape),
                      f64("specular_sampling_weight"), b["sample_visible"], b["distribution"] == abi.GVPM_MICROFACET_GGX,
                      b["sample_visible"] != 0, f64("eta"), f64("k"), kd, n, wi, wo)


def phong_world_with_aniso(kd, index, n, wi, wo, _inner=indep_statements.phong_world):
    """indep_statements.phong_world for tables that also carry the anisotropic kinds: rows naming an anisotropic head are
    answered here, rows naming a raw entry (a frame entry, a slice entry) or a head whose tangent spans no frame are unknown,
    the rest is handed on"""
    table = indep_statements.BSDFS
    index = np.asarray(index)
    f, pdf, known = _inner(kd, index, n, wi, wo)
    if not table.size:
        return f, pdf, known
    inside = (index >= 0) & (index < table.size)
    idx = np.where(inside, index, 0).astype(np.int64)
    head = abi.bsdf_heads(table)[idx] & inside
    aniso = head & np.isin(table["kind"][idx], ANISO)
    known = known & head
    if aniso.any():
        r = np.nonzero(aniso)[0]
        fa, pa, defined = aniso_world(table, np.broadcast_to(kd, f.shape)[r], idx[r], np.broadcast_to(n, f.shape)[r],
                                      np.broadcast_to(wi, f.shape)[r], np.broadcast_to(wo, f.shape)[r])
        f, pdf, known = f.copy(), pdf.copy(), known.copy()
        f[r], pdf[r], known[r] = fa, pa, defined
    return f, pdf, known


def install(monkeypatch):
    monkeypatch.setattr(indep_statements, "phong_world", phong_world_with_aniso)
