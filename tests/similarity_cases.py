"""Similarity transforms of seeded cases: the one place that knows which input field is a position.

Every scene the generators make is a room of half-width 1 at the origin.  `transformed(c, s, t, scale_epsilon)` maps every
geometric input of a Case by p' = fp32(s * p + t) (formed in float64, rounded once) and leaves everything else alone, so the
device and the oracle can be compared on a room that is 256 wide and a thousand units from the origin, or 1/64 wide.  It is no
physically consistent change of units -- pdfs and fluxes keep their numbers -- and need not be one: device and oracle receive
the same arrays, and parity between them is what the tests assert.

Scales are powers of two (exact in fp32: the scaled inputs are the inputs' own bits with another exponent, so the evaluated
set cannot move under a pure scale).  Scenes with mirror camera paths (cbox_mirror*) are out of scope: their second edge
starts at the first edge's fp32 end point, and rounding after the transform breaks that link.  Plain SoA uploads only.
"""
import copy
import ctypes as C
import math

import numpy as np

import cases
from gvpm_amd import abi

# name -> (s, t, scale_epsilon)
TRANSFORMS = {
    "shifted": (1.0, (3.03, -1.38, 4.72), False),
    "small": (1.0 / 64, (0.0, 0.0, 0.0), True),
    "large": (64.0, (193.7, -88.3, 301.9), True),
    "centimetres": (256.0, (700.3, -300.7, 1100.9), False),   # Epsilon left at 1e-4: below the ulp of a coordinate
    "far": (1.0, (1000.3, -700.7, 2000.9), False),
}
LARGE_AT_ORIGIN = (64.0, (0.0, 0.0, 0.0), True)

POSITION, LENGTH, KEEP = "position", "length", "keep"

# photon / beam / plane records (abi.Photons): a beam or plane record's origin is parent_pos, its end point pos
PHOTON_FIELDS = {
    "pos": POSITION, "parent_pos": POSITION,
    "wi": KEEP, "parent_n": KEEP, "parent_wi": KEEP,                                   # directions and normals
    "flux": KEEP, "prefix_w": KEEP, "parent_scat": KEEP,                               # weights
    "parent_pdf": KEEP, "edge_pdf": KEEP, "parent_rr": KEEP, "parent_g": KEEP,         # pdfs, Jacobian terms, table index
}
# camera rays (abi.CAMERA_RAY_DTYPE); `eye` is the eye path's weight (include/gvpm_hip.h), not a position
RAY_FIELDS = {
    "o": POSITION, "len": LENGTH,
    "d": KEEP, "pdf": KEEP, "eye": KEEP, "jacobian": KEEP, "gop": KEEP, "info": KEEP, "rand": KEEP, "pixel": KEEP,
}
PARAM_LENGTHS = ("bsphere_radius",)
# Epsilon is a length (ray minima, the [Epsilon, len - Epsilon] clip of a camera beam).  ShadowEpsilon is NOT: both visibility
# segments use it as a fraction of the reconnection distance (lProj * ShadowEpsilon as written, lProj * (1 - ShadowEpsilon) as
# intended), so it stays whatever the scale -- scaling it by 64 moves two shadow tests of fogroom_rot (tests/test_similarity.py)
PARAM_EPSILONS = ("epsilon",)
PARAM_RATIOS = ("shadow_epsilon",)
MEDIUM_INVERSE_LENGTHS = ("sigma_a", "sigma_s", "sigma_t")


def _kind(table, field, what):
    if field not in table:
        raise KeyError(f"similarity_cases: {what} field '{field}' is not classified as position, length or untouched")
    return table[field]


def _pos(a, s, t):
    return np.ascontiguousarray((np.asarray(a, np.float64) * s + np.asarray(t, np.float64)).astype(np.float32))


def _len(a, s):
    return np.ascontiguousarray((np.asarray(a, np.float64) * s).astype(np.float32))


def transform_records(ph, s, t):
    """a copy of photon / beam / plane records (abi.Photons) under p' = s p + t"""
    kinds = {k: _kind(PHOTON_FIELDS, k, "photon") for k in abi.PHOTON_VEC3 + abi.PHOTON_F1}
    out = ph.subset(np.arange(ph.n))
    for k, kind in kinds.items():
        if kind == POSITION:
            setattr(out, k, _pos(getattr(ph, k), s, t))
        elif kind == LENGTH:
            setattr(out, k, _len(getattr(ph, k), s))
    return out


def transform_rays(rays, s, t):
    """a copy of camera-beam sets (abi.CAMERA_RAY_DTYPE, any shape) under p' = s p + t"""
    assert rays.dtype == abi.CAMERA_RAY_DTYPE
    out = rays.copy()
    for k in abi.CAMERA_RAY_DTYPE.names:
        kind = _kind(RAY_FIELDS, k, "camera ray")
        if kind == POSITION:
            out[k] = _pos(rays[k], s, t)
        elif kind == LENGTH:
            out[k] = _len(rays[k], s)
    return out


def transformed(c, s, t=(0.0, 0.0, 0.0), scale_epsilon=True):
    """A copy of Case `c` (cases.make_case, make_vpm_case, make_beam_case, make_plane_case) for its one iteration with
    every position mapped by p' = fp32(s p + t), every length by s, the medium's coefficients by 1 / s; Epsilon scales only
    when `scale_epsilon` is set (ShadowEpsilon is a ratio and never does)."""
    m, e = math.frexp(s)
    assert s > 0 and m == 0.5, f"scale {s} is not a power of two"
    assert "mirror" not in c.sc.name, "two-edge camera paths: the second edge's origin would no longer be the first's end point"
    q = copy.copy(c)
    # params: lengths
    q.p = c.p.copy()
    for k in PARAM_LENGTHS + (PARAM_EPSILONS if scale_epsilon else ()):
        setattr(q.p, k, float(np.float32(np.float64(getattr(c.p, k)) * s)))
    q.r = cases.radius_of(q.p)
    # medium: inverse lengths (a power-of-two s keeps sigma_a + sigma_s == sigma_t bit for bit)
    q.m = type(c.m)()
    C.memmove(C.byref(q.m), C.byref(c.m), C.sizeof(c.m))
    for k in MEDIUM_INVERSE_LENGTHS:
        for i in range(3):
            getattr(q.m, k)[i] = float(np.float32(np.float64(getattr(c.m, k)[i]) / s))
    # triangles: v0 a position, the edges lengths
    v0, e1, e2 = c.tris
    q.tris = (_pos(v0, s, t), _len(e1, s), _len(e2, s))
    q.ph = transform_records(c.ph, s, t)
    q.rays = transform_rays(c.rays, s, t)
    if hasattr(c, "beams"):                        # G-Beams / G-Planes: origin parent_pos, end point pos; end_n, w1 directions
        q.beams = transform_records(c.beams, s, t)
        q.end_n = c.end_n.copy()
    if hasattr(c, "len1"):                         # G-Planes: second edge = w1 (direction) * len1 (length)
        q.w1 = c.w1.copy()
        q.len1 = _len(c.len1, s)
    if hasattr(c, "samples"):                      # G-VPM: set index, random number, selection pdf
        q.samples = c.samples.copy()
    q.xf = (s, tuple(t), scale_epsilon)
    cases.use_bsdfs(q)                             # (the oracle's table is process state: make it this case's again)
    return q


def named(c, name):
    return transformed(c, *TRANSFORMS[name])
