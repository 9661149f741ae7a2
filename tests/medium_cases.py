"""The one table of trial media: MEDIA[name] = (sigma_s[3], sigma_t, g, medium_sampling_weight), and apply(c, name).

Every generated scene carries one medium family: sigma_s equal in R, G and B, albedo 0.5, g in {0, 0.7}, medium_sampling_weight
(msw) 1.  Under it a kernel that reads sigmaS[0] three times, drops a (1 - msw) term or flips the sign of g passes every test.
As in similarity_cases.py the medium a case is EVALUATED under need not be the one its photons were shot in: device and oracle
get the same arrays and the same gvpm_medium, and parity between them is what is asserted.

Why these values.  The reference's Float is float, so the oracle at precision=32 is the reference's own arithmetic and its
distance from the fp64 oracle the error a faithful fp32 implementation may have.  A medium of EXACT is admitted for a technique
only if, on the very case the GPU test runs (tests/test_medium_space_gpu.py TECHNIQUES), the fp32 oracle's counters equal the
fp64 oracle's, its output is finite, and its L2 (test_parity_gpu.l2: 27 accumulators / mean luminance) and its per-channel L2
(per_channel_l2) stay at least 4x under the bar the technique's driver asserts (G-BRE 1e-4, G-VPM 1e-4, G-Beams 2e-4).  G-Planes
is held to 1e-5 by device_planes with its geometry in fp64: the fp32 oracle is no yardstick for it (above that bar under every
medium).  Measured, fp32 oracle against fp64 oracle, pooled L2 (largest per-channel L2 in brackets where it differs), counters:

  medium  G-BRE             G-VPM             Beams 3D          Beams 1D          Planes      fp32 counters
  grey    4.9e-7            8.0e-7            5.5e-7            3.5e-6            2.7e-5      equal
  chroma  5.7e-7 (4.9e-7)   1.4e-6 (1.3e-6)   6.3e-7 (5.8e-7)   4.1e-6 (3.6e-6)   3.7e-5      equal
  msw     5.4e-7 (5.5e-7)   8.3e-7 (8.6e-7)   5.9e-7 (6.0e-7)   6.1e-6 (6.2e-6)   3.0e-5      equal
  back    5.0e-7            1.9e-7            7.3e-7 (7.6e-7)   4.1e-5 (4.2e-5)   1.1e-4      equal
  all     6.9e-7 (5.8e-7)   2.6e-7 (2.3e-7)   8.1e-7 (7.1e-7)   4.3e-5 (3.8e-5)   1.3e-4      equal
  thick   3.6e-6 (3.4e-6)   4.7e-7 (4.5e-7)   6.3e-6 (5.9e-6)   3.1e-5 (2.8e-5)   1.1e-5      equal
  opaque  6.5e-6            1.9e-7            non-finite        non-finite        non-finite  G-BRE 2 134 and G-VPM 5 947 reconnections
                                                                                              become failed; Beams: the evaluated
                                                                                              set differs (6 393 / 4 979 pairs)

`back` is g = -0.55, not -0.6: at -0.6 the fp32 oracle's 1-D beams stand at 5.7e-5, 3.5x under the 2e-4 bar (one near-parallel
pair carries 4.5e-3 of the mean luminance; -0.5: 3.1e-5, -0.4: 1.8e-5) -- the medium is softened, never the bar.  |g| >= 0.8 is out
for the same reason.  sigma_t = 32 (`thick`) is the largest at which the fp32 oracle still takes every decision as fp64 does; at 64
(`opaque`) a reconnection whose pdfSuccess = sigma_t exp(-sigma_t t) underflows is a failed shift in fp32 and a zero-flux
reconnection in fp64, hence the weaker counter rule of test_medium_space_gpu.test_opaque.

The cut-off is reached: of the pixels the grey medium lights, the `thick` fp64 reference has a flux of exactly 0 in 1 of 1 185
(G-BRE), 22 of 859 (G-VPM), 29 of 821 / 29 of 824 (Beams 3D / 1D); `opaque`: 48, 64, 69 / 68.  G-Planes: 0 of 896 pixels, but
single pairs are cut (edges longer than 46 / sigma_t), where the reference divides by the cut transmittance: see
oracle/gvpm_oracle_planes.hpp cutRatio and test_medium_space.py.
"""
import ctypes as C

import numpy as np

# name -> (sigma_s per channel, sigma_t (common to the channels), g, medium_sampling_weight)
MEDIA = {
    "chroma": ((0.9, 0.5, 0.1), 1.0, 0.0, 1.0),     # the channel order of sigma_s
    "msw": ((0.5, 0.5, 0.5), 1.0, 0.0, 0.5),        # the 1 - msw terms; pdfSuccess * msw in the reconnection's MIS
    "back": ((0.5, 0.5, 0.5), 1.0, -0.55, 1.0),     # the sign conventions of phaseEval / phaseD (-0.6: see the table above)
    "all": ((0.9, 0.5, 0.1), 1.0, -0.4, 0.3),       # the three together
    "thick": ((26.0, 16.0, 6.0), 32.0, 0.0, 1.0),   # the 1e-20 cut-off and the fp32 quotients near it; counters still exact
    "opaque": ((52.0, 32.0, 12.0), 64.0, 0.0, 1.0), # beyond fp32's exponent range: finiteness, relaxed counters
}
EXACT = ("chroma", "msw", "back", "all", "thick")   # the media under which fp32 takes every decision as fp64 does


def apply(c, name):
    """Case `c` evaluated under MEDIA[name] (in place; returns c).  c.m becomes a copy of its own, so a medium the scene
    object hands out again is not touched."""
    sigma_s, sigma_t, g, msw = MEDIA[name]
    m = type(c.m)()
    C.memmove(C.byref(m), C.byref(c.m), C.sizeof(c.m))
    for k in range(3):
        m.sigma_s[k] = sigma_s[k]
        m.sigma_a[k] = sigma_t - sigma_s[k]
        m.sigma_t[k] = sigma_t
    m.g = g
    m.medium_sampling_weight = msw
    c.m = m
    c.medium_name = name
    return c


def per_channel_l2(acc, ref):
    """test_parity_gpu.l2 on one channel's nine slots, normalised by that channel's own mean flux: (R, G, B)"""
    acc = np.asarray(acc, np.float64)
    out = []
    for ch in range(3):
        d = acc[..., ch::3] - ref[..., ch::3]
        out.append(float(np.sqrt((d ** 2).mean()) / max(ref[..., ch].mean(), 1e-300)))
    return out
