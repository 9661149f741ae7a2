"""The G-BRE evaluation as its own translation unit (gvpm_amd/csrc/gather_bre_eval.hip), built without the SLP vectoriser: every
form launchEvaluate can start must still compute what the fp64 oracle computes, with the same counters -- scalar and packed
fp32 may contract differently at the last bit, and the pair decision's bands (decidePair, decidePairFine) must hold for both.

Shapes: a 32 x 32 frame, 20 000 photons, three iterations on one handle under the shrinking radius -- the smallest at which
every branch below still gets pairs (the oracle's counters are asserted to be in the hundreds at least: `branches_have_pairs`).
Scenes: cbox (Lambertian walls), cbox_conductor (glossy walls), and cbox_conductor's records relabelled to mixtures {the
wall's conductor, Lambertian} at weights (1, 0), which the oracle states as the plain conductor and which runs
evaluate_bre_mix_kernel (tests/test_eval_specialised_gpu.py).
Forms: 16 / 32 / 64 beams a wave; near lists, the occluder BVH (visibility_as_written = 0) and a forced near-list overflow
(896 occluders and a ShadowEpsilon of 0.2: more list entries than the extension array holds, tests/test_parity_gpu.py -- here the
oracle tests the same 896 triangles, so the counters are held exactly); the specialised and the generic configuration
(GVPM_EVAL_GENERIC=1); the host-shift form.

Bar: evaluations, null_shifts, diffuse_shifts and failed_shifts == the fp64 oracle's; L2 of the 27 accumulators over the mean
reference luminance < 1e-3 ("Parity bar").

The rim case: 4096 photons of cbox moved onto the rim of a beam's kernel (|perpendicular offset| = r (1 + x), x from 0 to
+-1e-3) or to the beam's end and beyond it (projection maxt + r x, x from -1e-3 to 1.5), so that the decision's bands, the
own-box branch and the hand-over to the exact pass all occur.  Counters exact, and the pairs handed to the exact pass for
their HIT (GVPM_TRACE_EXACT's `pair` cause) not more than the parent commit handed over on the same inputs
(tests/golden/eval_scalar_rim_parent.json, read once from the library of the commit before this file: 786 pairs).  A change of
the decision may narrow the bands, never widen them: deciding every pair by decidePairFine alone (NOTEBOOK.md round 22,
measured and dropped) handed over 785."""
import json
import os
import re

import numpy as np
import pytest

import cases
import mixture_cases as MC
import oracle_lib as O
import plastic_cases as PC
from gvpm_amd import abi, hip
from test_parity_gpu import l2

pytestmark = pytest.mark.gpu
W = H = 32
NPH = 20000
ITERS = (1, 2, 3)
SCALE = 3.0
BAR = 1e-3
COUNTERS = ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_scalar_rim_parent.json")
_inputs, _refs = {}, {}


class Run:
    pass


def inputs(scene, **kw):
    """The case and the photons / beams / radii of the three iterations, once per (scene, parameters)."""
    key = (scene, tuple(sorted(kw.items())))
    if key not in _inputs:
        r = Run()
        r.c = cases.make_case(scene, W, H, NPH, SCALE, **kw)
        r.steps, r.radii, scale = [], [], r.c.p.initial_scale_volume
        for it in ITERS:
            ph, nb = r.c.sc.shoot_photons(it, NPH)
            r.steps.append((ph, nb, r.c.sc.camera_beams(it)))
            r.radii.append(cases.radius_of(r.c.p, np.float32(scale)))
            scale = np.float32(O.scale_volume_apa(float(scale), it, float(r.c.p.alpha), r.c.p.vol_technique))
        r.key = key
        _inputs[key] = r
    return _inputs[key]


def reference(r, tris=None, what=""):
    """The fp64 oracle's fold over the run's iterations and its summed counters, once per (run, occluders)."""
    key = (r.key, what)
    if key not in _refs:
        O.set_bsdfs(r.c.bsdfs)
        ref, total = None, dict.fromkeys(COUNTERS, 0)
        for it, (ph, nb, rays), radius in zip(ITERS, r.steps, r.radii):
            ref, cnt, _ = O.gather_bre(r.c.p, r.c.m, r.c.tris if tris is None else tris, ph, rays, radius, it, nb, 64,
                                       use_accel=False, accum=ref)
            for k in COUNTERS:
                total[k] += cnt[k]
        _refs[key] = (ref, total)
    return _refs[key]


def device(r, monkeypatch, env=None, p=None, tris=None, table=None, mapping=None, host_shifts=False):
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = hip.Context(r.c.p if p is None else p, device=0)
    for k in env:
        monkeypatch.delenv(k)
    try:
        ctx.upload_scene(*(r.c.tris if tris is None else tris))
        ctx.upload_medium(r.c.m)
        table = r.c.bsdfs if table is None else table
        if table is not None and table.size:
            ctx.upload_bsdfs(table)
        if host_shifts:
            ctx.enable_host_shifts(1 << 16)
        for it, (ph, nb, rays), radius in zip(ITERS, r.steps, r.radii):
            assert ctx.radius() == radius
            ctx.upload_photons(ph if mapping is None else PC.relabelled(ph, mapping))
            ctx.upload_camera_beams(rays)
            ctx.gather(it, nb)
        if host_shifts:
            ctx.download_shift_requests(1 << 16)   # (none is answered: failed shifts, as with use_manifold off)
        return ctx.download_accum(), ctx.stats()
    finally:
        ctx.close()


def branches_have_pairs(cnt):
    """the sizes are the smallest at which the base term, the null shifts, the reconnections and the failed ones all occur"""
    assert cnt["evaluations"] > 10000 and cnt["null_shifts"] > 1000 and cnt["diffuse_shifts"] > 1000 and cnt["failed_shifts"] > 100, cnt


def meets_the_bar(acc, st, ref, cnt, what):
    lum = max(ref[..., 0:3].mean(), 1e-30)
    err = l2(acc, ref, lum)
    print(what, "device", {k: st[k] for k in COUNTERS}, "oracle", cnt, "L2 accum / lum", err)
    for k in COUNTERS:
        assert st[k] == cnt[k], (what, k, st, cnt)
    assert err < BAR, (what, err)


def mixture_table():
    """per wall a mixture {that wall's conductor entry, Lambertian} at weights (1, 0) behind the scene's own entries, and the map
    from the records' entries to the mixture heads (tests/test_eval_specialised_gpu.py)"""
    throwaway = cases.make_case("cbox_conductor", 8, 8, 100, 4.0)
    heads = MC.over_conductor(throwaway, (1.0, 0.0))
    table = throwaway.bsdfs
    assert (table["kind"][heads] == abi.GVPM_BSDF_MIXTURE).all()
    own = throwaway.sc.bsdfs()
    mapping = np.zeros(own.size, np.int64)
    mapping[np.flatnonzero(abi.bsdf_heads(own))] = heads
    return table, mapping


GENERIC = {"GVPM_EVAL_GENERIC": "1"}
FORMS = {
    # name: (scene, case parameters, environment of gvpm_create)
    "cbox-B16": ("cbox", {}, {}),
    "cbox-B16-generic": ("cbox", {}, GENERIC),
    "cbox-B32": ("cbox", {}, {"GVPM_BEAMS_PER_WAVE": "32"}),
    "cbox-B64": ("cbox", {}, {"GVPM_BEAMS_PER_WAVE": "64"}),
    "cbox-bvh-B16": ("cbox", dict(visibility_as_written=0), {}),
    "cbox-bvh-B16-generic": ("cbox", dict(visibility_as_written=0), GENERIC),
    "cbox-bvh-B32": ("cbox", dict(visibility_as_written=0), {"GVPM_BEAMS_PER_WAVE": "32"}),
    "cbox-bvh-B64": ("cbox", dict(visibility_as_written=0), {"GVPM_BEAMS_PER_WAVE": "64"}),
    "glossy-B16": ("cbox_conductor", {}, {}),
    "glossy-B16-generic": ("cbox_conductor", {}, GENERIC),
    "glossy-bvh-B16": ("cbox_conductor", dict(visibility_as_written=0), {}),
    "glossy-B64": ("cbox_conductor", {}, {"GVPM_BEAMS_PER_WAVE": "64"}),
    "mixture-B16": ("mixture", {}, {}),
    "mixture-B16-generic": ("mixture", {}, GENERIC),
    "mixture-B32": ("mixture", {}, {"GVPM_BEAMS_PER_WAVE": "32"}),
    "mixture-B64": ("mixture", {}, {"GVPM_BEAMS_PER_WAVE": "64"}),
    "mixture-bvh-B16": ("mixture", dict(visibility_as_written=0), {}),
    "mixture-bvh-B16-generic": ("mixture", dict(visibility_as_written=0), GENERIC),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_of_the_evaluation_matches_the_oracle(form, monkeypatch):
    scene, kw, env = FORMS[form]
    mix = scene == "mixture"
    r = inputs("cbox_conductor" if mix else scene, **kw)
    ref, cnt = reference(r)
    branches_have_pairs(cnt)
    table, mapping = mixture_table() if mix else (None, None)
    if mix:
        gl = (r.steps[0][0].flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
        assert gl.sum() > 500   # (reconnections through the mixture heads)
    acc, st = device(r, monkeypatch, env=env, table=table, mapping=mapping)
    meets_the_bar(acc, st, ref, cnt, form)


@pytest.mark.parametrize("env", [{}, GENERIC], ids=["as-selected", "generic"])
def test_forced_near_list_overflow_runs_the_bvh_form(env, monkeypatch, capfd):
    r = inputs("cbox", shadow_epsilon=0.2)
    fine = cases.tessellate(r.c.tris, 3)
    assert fine[0].shape[0] > 254
    ref, cnt = reference(r, tris=fine, what="896 occluders")
    branches_have_pairs(cnt)
    acc, st = device(r, monkeypatch, env=dict(env, GVPM_TRACE_VIS="1"), tris=fine)
    err = capfd.readouterr().err
    over = [int(m) for m in re.findall(r"(\d+) lists overflowed", err)]
    assert over and max(over) > 0 and "fullvis 1" in err, err[-2000:]   # (the step went through the BVH kernels with the flag on)
    meets_the_bar(acc, st, ref, cnt, "forced near-list overflow")


@pytest.mark.parametrize("kw,env", [(dict(), {}), (dict(visibility_as_written=0), {}), (dict(), {"GVPM_BEAMS_PER_WAVE": "32"}),
                                    (dict(), {"GVPM_BEAMS_PER_WAVE": "64"})], ids=["B16", "bvh-B16", "B32", "B64"])
def test_host_shift_form(kw, env, monkeypatch):
    """gvpm_enable_host_shifts with use_manifold on and no request answered: the oracle's statement with use_manifold off"""
    r = inputs("cbox", **kw)
    ref, cnt = reference(r)
    p = r.c.p.copy()
    p.use_manifold = 1
    acc, st = device(r, monkeypatch, env=env, p=p, host_shifts=True)
    meets_the_bar(acc, st, ref, cnt, f"host shifts {kw} {env}")


# ---- the rim of the kernel and the beam's end -----------------------------------------------------------------------------------
RIM_X = (0.0, 1e-7, -1e-7, 5e-7, -5e-7, 1.5e-6, -1.5e-6, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3)
END_X = (-1e-3, -1e-6, 0.0, 1e-6, 1e-3, 0.3, 0.9, 1.5)


def rim_case():
    """cbox with 4096 of its photons moved: half of them onto the rim of a beam's kernel, half to the beam's end and beyond it
    (within the radius of the axis); each takes the checkerboard parity of its beam's pixel, so that the pair is a candidate."""
    c = cases.make_case("cbox", W, H, NPH, SCALE)
    rng = np.random.default_rng(22)
    K, half = 4096, 2048
    base = c.rays[:, 0]
    r, eps = np.float64(c.r), np.float64(c.p.epsilon)
    k = rng.choice(c.ph.n, K, replace=False)
    long_enough = np.flatnonzero((base["len"] > 6 * r) & ((base["info"] & 1) == 1))
    assert long_enough.size > base.shape[0] // 2
    s = rng.choice(long_enough, K)
    o, d, ln = base["o"][s].astype(np.float64), base["d"][s].astype(np.float64), base["len"][s].astype(np.float64)
    a = rng.normal(size=(K, 3))
    a -= (a * d).sum(1)[:, None] * d
    a /= np.linalg.norm(a, axis=1)[:, None]
    t = rng.uniform(eps + r, ln - eps - r)
    dist = r * (1.0 + rng.choice(RIM_X, K))
    t[half:] = (ln - eps)[half:] + r * rng.choice(END_X, K - half)
    dist[half:] = r * rng.uniform(0.0, 1.0, K - half)
    c.ph.pos[k] = (o + d * t[:, None] + a * dist[:, None]).astype(np.float32)
    px, py = cases.pixels_of(c.rays)
    c.ph.path_id[k] = (c.ph.path_id[k] & ~np.uint32(1)) | ((px[s] + py[s]) & 1).astype(np.uint32)
    return c


def rim_device(c, monkeypatch, capfd, env=None):
    """-> accumulators, counters, pairs handed to the exact pass for their hit"""
    env = dict(env or {}, GVPM_TRACE_EXACT="1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = hip.Context(c.p, device=0)
    for k in env:
        monkeypatch.delenv(k)
    try:
        ctx.upload_scene(*c.tris)
        ctx.upload_medium(c.m)
        ctx.upload_photons(c.ph)
        ctx.upload_camera_beams(c.rays)
        ctx.gather(c.it, c.nb)
        acc, st = ctx.download_accum(), ctx.stats()
        capfd.readouterr()
        evaluated, lost = ctx.exact_shifts()
        m = re.search(r"\[exact\] evaluated (\d+) lost (\d+) .*by cause: pair (\d+)", capfd.readouterr().err)
        assert m and lost == 0, (evaluated, lost)
        return acc, st, int(m.group(3))
    finally:
        ctx.close()


@pytest.mark.parametrize("env", [{}, GENERIC], ids=["as-selected", "generic"])
def test_rim_pairs_are_decided_as_the_oracle_decides_them_and_fewer_are_deferred(env, monkeypatch, capfd):
    c = rim_case()
    O.set_bsdfs(c.bsdfs)
    ref, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, c.it, c.nb, 64, use_accel=False)
    acc, st, pairs = rim_device(c, monkeypatch, capfd, env)
    parent = json.load(open(GOLD))
    print("pairs handed to the exact pass for their hit:", pairs, "parent:", parent["deferred_pairs"])
    meets_the_bar(acc, st, ref, {k: cnt[k] for k in COUNTERS}, "rim")
    assert cnt["evaluations"] == parent["oracle_evaluations"]   # (the fixture was read on these inputs)
    assert 1 <= pairs <= parent["deferred_pairs"], (pairs, parent)
