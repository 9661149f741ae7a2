"""Generates tests/golden/rtrans_slices.npz: the 100-value rough-transmittance slices and the internal diffuse reflectance
Fdr of the rough-plastic surfaces the tests use, derived from the reference's precomputed tables
(/root/reference/data/microfacet/{beckmann,ggx}.dat).  Our own numpy reading of the file layout, of the two reductions
RoughPlastic::configure asks for (src/bsdfs/rtrans.h:294-390: fix eta, then fix alpha) and of the cubic spline they use
(src/libcore/spline.cpp: Catmull-Rom, one-sided differences at the ends), everything in fp32 as the reference's
SINGLE_PRECISION build has it.  Run in the build container (needs /root/reference).

File layout: "MTS_TRANSMITTANCE", three u64 sizes (eta 50, alpha 50, theta 100), four f32 ranges (eta min / max, alpha
min / max), then per (eta block, alpha) 100 transmittance values + 1 diffuse value; the first 50 eta rows hold eta > 1,
the next 50 the reciprocal index (leaving the denser medium).  All three axes are warped: x -> ((x - min) / (max - min))^(1/4)
(theta: cos^(1/4))."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DATA_DIR = "/root/reference/data/microfacet"
OUT = os.path.join(HERE, "rtrans_slices.npz")
# (distribution, eta, alpha) of the surfaces of the plastic tests
ENTRIES = (("beckmann", 1.5, 0.1), ("ggx", 1.5, 0.3), ("beckmann", 1.5, 0.03), ("ggx", 1.5, 0.04))
F = np.float32


def key(dist, eta, alpha):
    return f"{dist}_eta{eta:g}_alpha{alpha:g}"


def read_dat(path):
    with open(path, "rb") as f:
        raw = f.read()
    magic = b"MTS_TRANSMITTANCE"
    assert raw[:len(magic)] == magic, "not a transmittance file"
    o = len(magic)
    ne, na, nt = (int(x) for x in np.frombuffer(raw, "<u8", 3, o))
    o += 24
    eta_min, eta_max, alpha_min, alpha_max = np.frombuffer(raw, "<f4", 4, o)
    o += 16
    body = np.frombuffer(raw, "<f4", 2 * ne * na * (nt + 1), o).reshape(2 * ne, na, nt + 1)
    assert o + body.nbytes == len(raw)
    return dict(trans=body[..., :nt].copy(), diff=body[..., nt].copy(), ne=ne, na=na, nt=nt, eta_min=F(eta_min), eta_max=F(eta_max),
                alpha_min=F(alpha_min), alpha_max=F(alpha_max))


def knot_weights(x, size):
    """left knot - 1 and the four node weights of the spline at x in [0, 1] over `size` uniform knots (fp32)"""
    t = F(F(x) * F(size - 1))
    k = min(int(t), size - 2)
    t = F(t - F(k))
    t2 = F(t * t)
    t3 = F(t2 * t)
    w = [F(0), F(2 * t3 - 3 * t2 + 1), F(-2 * t3 + 3 * t2), F(0)]
    d0, d1 = F(t3 - 2 * t2 + t), F(t3 - t2)
    if k > 0:
        w[2] += F(0.5) * d0
        w[0] -= F(0.5) * d0
    else:
        w[2] += d0
        w[1] -= d0
    if k + 2 < size:
        w[3] += F(0.5) * d1
        w[1] -= F(0.5) * d1
    else:
        w[2] += d1
        w[1] -= d1
    return k, np.array(w, F)


def interp_axis0(values, x):
    """spline along axis 0 of `values` at x (the other axes ride along); nodes outside the array carry weight zero"""
    k, w = knot_weights(x, values.shape[0])
    out = np.zeros(values.shape[1:], F)
    for j in range(4):
        if w[j] != 0:
            out = (out + values[k - 1 + j] * w[j]).astype(F)
    return out


def spline_eval(values, x):
    """evalCubicInterp1D over [0, 1] (any float precision of `values`; the reference's end rules)"""
    values = np.asarray(values)
    size = values.shape[0]
    x = np.asarray(x, values.dtype)
    t = x * (size - 1)
    k = np.clip(t.astype(np.int64), 0, size - 2)
    f0, f1 = values[k], values[k + 1]
    d0 = np.where(k > 0, 0.5 * (f1 - values[np.maximum(k - 1, 0)]), f1 - f0)
    d1 = np.where(k + 2 < size, 0.5 * (values[np.minimum(k + 2, size - 1)] - f0), f1 - f0)
    t = t - k
    t2 = t * t
    t3 = t2 * t
    return (2 * t3 - 3 * t2 + 1) * f0 + (-2 * t3 + 3 * t2) * f1 + (t3 - 2 * t2 + t) * d0 + (t3 - t2) * d1


def warp(x, lo, hi):
    return F(np.power(F(F(x - lo) / F(hi - lo)), F(0.25)))


def reduce_slice(d, eta, alpha):
    """(slice[100] float32, Fdr float32) of a surface of relative index eta >= 1 and roughness alpha"""
    ne = d["ne"]
    eta = F(max(F(eta), d["eta_min"]))
    w_eta, w_alpha = warp(eta, d["eta_min"], d["eta_max"]), warp(F(alpha), d["alpha_min"], d["alpha_max"])
    # stage 1, setEta: the exterior table at eta, the interior one (second block) at 1 / eta -- same warped coordinate
    ext = interp_axis0(d["trans"][:ne], w_eta)            # [alpha, theta]
    int_diff = interp_axis0(d["diff"][ne:], w_eta)        # [alpha]
    # stage 2, setAlpha (the theta knots are the table's own: the spline returns them)
    sl = interp_axis0(ext, w_alpha)                       # [theta]
    fdr = F(1) - np.clip(interp_axis0(int_diff, w_alpha), F(0), F(1))
    return np.clip(sl, F(0), F(1)).astype(F), F(fdr)


def make():
    out = {}
    tables = {}
    for dist, eta, alpha in ENTRIES:
        if dist not in tables:
            tables[dist] = read_dat(os.path.join(DATA_DIR, dist + ".dat"))
        sl, fdr = reduce_slice(tables[dist], eta, alpha)
        out[key(dist, eta, alpha)] = np.concatenate([sl, [fdr]]).astype(F)
    return out


if __name__ == "__main__":
    np.savez(OUT, **make())
    for k, v in np.load(OUT).items():
        print(k, "T(0) %.4f T(1) %.4f Fdr %.4f" % (v[0], v[99], v[100]))
