"""The device under the per-entry parity bars (tests/entry_parity.py): for every admitted input of tests/entry_cases.py one upload,
one gather, the counters equal to the fp64 oracle's, and then assertions A (zeros), B (bulk) and C (tail) of the downloaded
accumulators against the fp64 oracle in units of the strict fp32 oracle's own distance from it.  G-Beams also under the literal
fp64 transcription (GVPM_BEAMS_FP64=1), G-BRE also at 16 and 32 beams a wave: the same inputs, the same bars.

Below that, film_kernel (assemble.hip) entry by entry against the fp64 assembly of the device's OWN accumulators, with and without
reusePrimal and an emission image, through the host and the device entry points, with G-VPM's division by the emitted count, and on
the smallest images gvpm_create admits.

Run with -s for the figures NOTEBOOK.md records."""
import os

import numpy as np
import pytest

import cases
import entry_cases as E
import entry_parity as P
import oracle_lib as O
from gvpm_amd import abi, hip
from test_oracle_vpm import make_vpm_case

pytestmark = pytest.mark.gpu


def context(p, env=None):
    """hip.Context with `env` set around the constructor only, where the library reads it"""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return hip.Context(p, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v


def device(r, env=None):
    """(accum, stats, (scale_vol, n_vol) or None) of one gather at iteration c.it on what the case gives the device"""
    c, rec = r.c, r.dev_records
    ctx = context(c.p, env)
    try:
        ctx.upload_scene(*c.tris)
        ctx.upload_medium(c.m)
        if r.dev_table.size:
            ctx.upload_bsdfs(r.dev_table)
        if r.tech in ("bre", "vpm"):
            ctx.upload_photons(rec[0])
        elif r.tech == "beams":
            ctx.upload_beams(rec[0], rec[1])
        else:
            ctx.upload_planes(rec[0], rec[1], rec[2])
        ctx.upload_camera_beams(c.rays)
        if r.tech == "vpm":
            ctx.upload_vpm_samples(c.samples)
        if r.tech in ("bre", "beams"):
            assert abs(ctx.radius() - c.r) == 0.0
        ctx.gather(c.it, c.nb)
        acc, st = ctx.download_accum(), ctx.stats()
        state = ctx.download_vpm_state() if r.tech == "vpm" else None
    finally:
        ctx.close()
    return acc, st, state


def under_the_bars(name, env=None):
    r = E.prepared(name)
    what = name + ("" if not env else " " + " ".join(f"{k}={v}" for k, v in env.items()))
    acc, st, state = device(r, env)
    for k in E.COUNTERS:
        assert st[k] == r.cnt64[k], (what, k, st, r.cnt64)
    if state is not None:
        assert np.allclose(state[0], r.sv, rtol=1e-6) and np.allclose(state[1], r.nv, rtol=1e-6)
    rho = P.entry_stats(acc, r.r64, r.lum)
    zero, tiny, compared = P.masks(r.r64, r.lum)
    print(P.report(what, dict(ref=P.percentiles(P.entry_stats(r.r32, r.r64, r.lum)), dev=P.percentiles(rho),
                              T=P.tail_bar(P.entry_stats(r.r32, r.r64, r.lum)), compared=int(compared.sum()), tiny=int(tiny.sum()),
                              zero=int(zero.sum()))) + f"; old bar {P.l2(acc, r.r64, r.lum):.2e}")
    P.assert_entry_parity(acc, r.r64, r.r32, r.lum, what=what)


@pytest.mark.parametrize("name", E.NAMES)
def test_device_entries(name):
    under_the_bars(name)


@pytest.mark.parametrize("name", [n for n in E.NAMES if E.CASES[n][0] == "beams"])
def test_beams_fp64_transcription_entries(name):
    under_the_bars(name, {"GVPM_BEAMS_FP64": "1"})


@pytest.mark.parametrize("bpw", [16, 32])
@pytest.mark.parametrize("name", [n for n in E.NAMES if E.CASES[n][0] == "bre"])
def test_bre_beams_per_wave_entries(name, bpw):
    under_the_bars(name, {"GVPM_BEAMS_PER_WAVE": str(bpw)})


# ---- film_kernel ---------------------------------------------------------------------------------------------------------------------
L, R, T, B = abi.GVPM_LEFT, abi.GVPM_RIGHT, abi.GVPM_TOP, abi.GVPM_BOTTOM
U = 2.0 ** -24


def stencil(acc, it, reuse_primal, emission, inv_div=1.0, magnitudes=False):
    """throughput (gvpm.cpp:480-500), reusePrimal (:503-532) and computeGradient (:1205-1306) in fp64 numpy over accumulators
    [H, W, 27]; magnitudes: the same stencil over absolute values with every difference a sum -- S, the sum of the magnitudes of the
    terms that enter an entry times the divisor, which is what the rounding errors of an fp32 evaluation scale with."""
    H, W = acc.shape[:2]
    A = (np.abs(acc) if magnitudes else np.asarray(acc, np.float64)).astype(np.float64).reshape(H, W, 9, 3)
    s = 1.0 if magnitudes else -1.0
    sh, wt = (lambda i: A[:, :, 1 + i]), (lambda i: A[:, :, 5 + i])
    if reuse_primal:
        t = wt(B) + wt(T) + wt(R) + wt(L)
        t[:, :-1] += sh(L)[:, 1:]
        t[:, 1:] += sh(R)[:, :-1]
        t[:-1] += sh(B)[1:]
        t[1:] += sh(T)[:-1]
        thr = t / 4.0 * inv_div
    else:
        thr = A[:, :, 0] * inv_div
        if emission is not None:
            thr = thr + np.abs(np.asarray(emission, np.float64)) / it
    dx = sh(R) + s * wt(R)
    dx[:, :-1] += wt(L)[:, 1:] + s * sh(L)[:, 1:]
    dy = sh(T) + s * wt(T)
    dy[:-1] += wt(B)[1:] + s * sh(B)[1:]
    return thr, dx * inv_div, dy * inv_div


def film_within_bound(film, acc, it, reuse_primal, emission, total_emitted=0.0, what=""):
    """|dev - ref| <= 12 * 2^-24 * S per entry: at most 8 fp32 terms and 7 additions, the / 4 and invDiv products, one rounding in
    download_accum's scale (the reference assembles what download_accum returned; the kernel reads the unscaled sums).  Derived."""
    ref = O.assemble(acc, it, reuse_primal, emission, total_emitted=total_emitted)
    inv = 1.0 / total_emitted if total_emitted else 1.0
    mine = stencil(acc, it, reuse_primal, emission, inv)
    S = stencil(acc, it, reuse_primal, emission, inv, magnitudes=True)
    for k, plane in enumerate(("throughput", "dx", "dy")):
        assert np.allclose(mine[k], ref[k], rtol=1e-13, atol=1e-13 * S[k].max()), (what, plane, "the numpy stencil is not the oracle's")
        err, bound = np.abs(film[k].astype(np.float64) - ref[k]), 12 * U * S[k]
        bad = np.argwhere(err > bound)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{what} {plane}: largest |dev - ref| / (12 u S) = {worst:.3f}")
        assert bad.size == 0, (what, plane, len(bad), [(tuple(int(v) for v in b), float(film[k][tuple(b)]), float(ref[k][tuple(b)]),
                                                         float(bound[tuple(b)])) for b in bad[:4]])
    return S


def gathered(c, iters):
    """a handle after `iters` G-BRE gathers of the case's scene (it = 1 .. iters, new photons and beams each), and its accumulators"""
    ctx = hip.Context(c.p, device=0)
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    for it in range(1, iters + 1):
        ph, nb = (c.ph, c.nb) if it == 1 else c.sc.shoot_photons(it, c.ph.n)
        ctx.upload_photons(ph)
        ctx.upload_camera_beams(c.rays if it == 1 else c.sc.camera_beams(it))
        ctx.gather(it, nb)
    return ctx, ctx.download_accum().astype(np.float64)


def emission_for(acc, seed=11):
    """a positive H x W x 3 float32 image of about the mean luminance"""
    H, W = acc.shape[:2]
    lum = max(float(acc[..., 0:3].mean()), 1e-6)
    return (np.random.default_rng(seed).uniform(0.5, 1.5, (H, W, 3)) * lum).astype(np.float32)


@pytest.fixture(scope="module")
def three_gathers():
    ctx, acc = gathered(cases.make_case("cbox", 24, 20, 8000, 3.0), 3)
    yield ctx, acc
    ctx.close()


def test_film_entries(three_gathers):
    ctx, acc = three_gathers
    assert (acc[..., 3:15] != 0).any() and (acc[..., 15:27] != 0).any()
    em = emission_for(acc)
    films = {}
    for reuse in (False, True):
        for e in (None, em):
            what = f"reuse_primal={reuse} emission={'yes' if e is not None else 'no'}"
            films[reuse, e is not None] = f = ctx.download_film(3, reuse, e)
            film_within_bound(f, acc, 3, reuse, e, what=what)
    # the emission term alone: emission / it where the primal is the medium flux, nothing where reusePrimal overwrites it
    # (gvpm.cpp:503-532)
    S = stencil(acc, 3, False, em, magnitudes=True)[0]
    diff = films[False, True][0].astype(np.float64) - films[False, False][0].astype(np.float64)
    assert (np.abs(diff - em.astype(np.float64) / 3) <= 12 * U * S).all()
    assert (diff > 0).all()
    for k in range(3):
        assert np.array_equal(films[True, True][k], films[True, False][k])
        if k:
            assert np.array_equal(films[False, True][k], films[False, False][k])   # (dx and dy never see it)


def test_film_entries_through_device_pointers(three_gathers):
    """gvpm_download_film_dev with the emission image in device memory (the tensor pattern of
    test_parity_gpu.test_partial_films_of_interleaved_shards_sum_to_the_frames_film)"""
    import torch
    ctx, acc = three_gathers
    H, W = acc.shape[:2]
    n = H * W * 3
    em = emission_for(acc, seed=12)
    emt = torch.from_numpy(em.reshape(-1)).cuda()
    for reuse in (False, True):
        for e in (None, emt):
            t = torch.zeros(3 * n, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()  # the fill and the copy run on torch's stream, the film kernel on the context's
            ctx.download_film_dev(3, t.data_ptr(), reuse_primal=reuse, emission_dev_ptr=None if e is None else e.data_ptr())
            ctx.synchronize()
            out = t.cpu().numpy()
            film = tuple(out[k * n:(k + 1) * n].reshape(H, W, 3) for k in range(3))
            film_within_bound(film, acc, 3, reuse, None if e is None else em, what=f"dev pointers reuse_primal={reuse} emission={e is not None}")
            host = ctx.download_film(3, reuse, None if e is None else em)
            for a, b in zip(film, host):
                assert np.array_equal(a, b)   # (the same kernel on the same inputs)


def test_film_entries_vpm_divides_by_the_emitted_count():
    c = make_vpm_case("cbox", 20, 16, 6000, 6.0, nb=4)
    ctx = hip.Context(c.p, device=0)
    try:
        ctx.upload_scene(*c.tris)
        ctx.upload_medium(c.m)
        emitted = 0
        for it in (1, 2):
            ph, nb = (c.ph, c.nb) if it == 1 else c.sc.shoot_photons(it, c.ph.n)
            rays, smp = (c.rays, c.samples) if it == 1 else c.sc.camera_beams_and_vpm_samples(it, c.p.nb_camera_samples)
            ctx.upload_photons(ph)
            ctx.upload_camera_beams(rays)
            ctx.upload_vpm_samples(smp)
            ctx.gather(it, nb)
            emitted += nb
        acc = ctx.download_accum().astype(np.float64)
        assert acc.any()
        em = (emission_for(acc, seed=13) / emitted).astype(np.float32)   # (about the film's own size: sums / emitted)
        for reuse in (False, True):
            for e in (None, em):
                film_within_bound(ctx.download_film(2, reuse, e), acc, 2, reuse, e, total_emitted=float(emitted),
                                  what=f"vpm reuse_primal={reuse} emission={e is not None}")
    finally:
        ctx.close()


@pytest.mark.parametrize("W,H", [(1, 1), (1, 7), (9, 1)])
def test_film_entries_on_the_smallest_images(W, H):
    """The border arms of the stencil: a single pixel has no neighbour at all, a column none to the left or right, a row none
    above or below.  30 000 photons at scale 12: at the usual 8 000 / 3 the one beam set of the 1 x 7 image meets no photon."""
    ctx, acc = gathered(cases.make_case("cbox", W, H, 30000, 12.0), 2)
    try:
        assert acc.shape == (H, W, 27) and acc.any()
        em = emission_for(acc, seed=14)
        for reuse in (False, True):
            for e in (None, em):
                film_within_bound(ctx.download_film(2, reuse, e), acc, 2, reuse, e, what=f"{W} x {H} reuse_primal={reuse} emission={e is not None}")
    finally:
        ctx.close()
