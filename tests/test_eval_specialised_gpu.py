"""The specialised G-BRE evaluation (gather_bre.hip launchEvaluate; shift_device.h EvalCfgHeadline): a handle whose configuration is
the synthetic hosts' default -- 3D kernel, null shifts, MIS with the balance heuristic, the checkerboard path set, no debug filter --
runs an evaluation kernel with the other side of every test on those flags compiled out; GVPM_EVAL_GENERIC=1 keeps the kernel that
reads them from its arguments.  Both must compute what the fp64 oracle computes, with the same counters; every configuration the
launcher must send to the generic kernel still passes against the oracle.

Shapes: a 48 x 48 frame, 20 000 photons, three iterations under the shrinking radius.  The four specialised instantiations:
cbox (near lists, plain table), cbox_rot with visibility_as_written = 0 (the occluder BVH), and cbox_conductor's records through
mixtures {the wall's conductor, Lambertian} at weights (1, 0) -- a table with mixture heads, which the frozen oracle states as the
plain conductor (tests/test_mixture_parents_gpu.py) -- with visibility_as_written on and off.

Bar (tests/test_parity_gpu.py): evaluation count == the oracle's, L2 of the accumulators and of the film over the mean reference
luminance < 1e-3."""
import numpy as np
import pytest

import cases
import mixture_cases as MC
import oracle_lib as O
import plastic_cases as PC
from gvpm_amd import abi, hip
from test_parity_gpu import l2

pytestmark = pytest.mark.gpu
W = H = 48
NPH = 20000
ITERS = (1, 2, 3)
BAR = 1e-3
COUNTERS = ("evaluations", "candidates", "null_shifts", "diffuse_shifts", "failed_shifts")
_built = {}


class Run:
    pass


def build(scene, accel=False, oracle_kw=None, **kw):
    """The inputs of the three iterations and the oracle's fold over them, once per (scene, parameters)."""
    key = (scene, accel, tuple(sorted((oracle_kw or {}).items())), tuple(sorted(kw.items())))
    if key in _built:
        return _built[key]
    mix = scene == "mixture"
    c = cases.make_case("cbox_conductor" if mix else scene, W, H, NPH, 1.6 if scene.endswith("_rot") else 2.5, **kw)
    r = Run()
    r.c, r.p = c, c.p
    r.table, mapping = c.bsdfs, None
    plain = c.bsdfs
    if mix:
        # per wall a mixture {that wall's conductor entry, Lambertian} at weights (1, 0) behind the scene's own entries
        throwaway = cases.make_case("cbox_conductor", 8, 8, 100, 4.0)
        heads = MC.over_conductor(throwaway, (1.0, 0.0))
        r.table = throwaway.bsdfs
        assert (r.table["kind"][heads] == abi.GVPM_BSDF_MIXTURE).all()
        own = c.sc.bsdfs()
        mapping = np.zeros(own.size, np.int64)
        mapping[np.flatnonzero(abi.bsdf_heads(own))] = heads
    po = c.p.copy()
    for k, v in (oracle_kw or {}).items():
        setattr(po, k, v)
    O.set_bsdfs(plain)   # (the oracle reads the plain conductor table and the records that name it)
    r.steps, r.radii, ref, ev, scale = [], [], None, 0, c.p.initial_scale_volume
    for it in ITERS:
        ph, nb = c.sc.shoot_photons(it, NPH)
        rays = c.sc.camera_beams(it)
        radius = cases.radius_of(c.p, np.float32(scale))
        ref, cnt, _ = O.gather_bre(po, c.m, c.tris, ph, rays, radius, it, nb, 64, use_accel=accel, accum=ref)
        ev += cnt["evaluations"]
        r.steps.append((PC.relabelled(ph, mapping) if mix else ph, nb, rays))
        r.radii.append(radius)
        scale = np.float32(O.scale_volume_apa(float(scale), it, float(c.p.alpha), c.p.vol_technique))
    if mix:
        gl = (r.steps[0][0].flags & 3) == abi.GVPM_PARENT_SURFACE_BSDF
        assert gl.sum() > 500 and np.isin(r.steps[0][0].parent_g[gl].astype(np.int64), heads).all()
    r.ref, r.evaluations = ref, ev
    r.film = O.assemble(ref, ITERS[-1], True)
    _built[key] = r
    return r


def device(r, monkeypatch, env=None, host_shifts=False):
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = hip.Context(r.p, device=0)
    for k in env:
        monkeypatch.delenv(k)
    ctx.upload_scene(*r.c.tris)
    ctx.upload_medium(r.c.m)
    if r.table is not None and r.table.size:
        ctx.upload_bsdfs(r.table)
    if host_shifts:
        ctx.enable_host_shifts(1 << 16)
    for it, (ph, nb, rays), radius in zip(ITERS, r.steps, r.radii):
        assert ctx.radius() == radius
        ctx.upload_photons(ph)
        ctx.upload_camera_beams(rays)
        ctx.gather(it, nb)
    if host_shifts:
        ctx.download_shift_requests(1 << 16)   # (none is answered: failed shifts, as with use_manifold off)
    acc, st = ctx.download_accum(), ctx.stats()
    film = ctx.download_film(ITERS[-1], True)
    ctx.close()
    return acc, st, film


def meets_the_bar(r, acc, st, film, what):
    lum = max(r.ref[..., 0:3].mean(), 1e-30)
    errs = [l2(acc, r.ref, lum)] + [l2(a, b, lum) for a, b in zip(film, r.film)]
    print(what, "evaluations", st["evaluations"], "oracle", r.evaluations, "L2 accum / throughput / dx / dy", errs, st)
    assert st["evaluations"] == r.evaluations > 10000, (what, st, r.evaluations)
    assert max(errs) < BAR, (what, errs)


@pytest.mark.parametrize("scene,kw", [("cbox", dict()), ("cbox_rot", dict(visibility_as_written=0)), ("mixture", dict()),
                                      ("mixture", dict(visibility_as_written=0))],
                         ids=["cbox", "cbox_rot-bvh", "mixture", "mixture-bvh"])
def test_specialised_and_generic_kernels_agree_and_match_the_oracle(scene, kw, monkeypatch):
    r = build(scene, **kw)
    acc_s, st_s, film_s = device(r, monkeypatch)
    acc_g, st_g, film_g = device(r, monkeypatch, env={"GVPM_EVAL_GENERIC": "1"})
    for k in COUNTERS:
        assert st_s[k] == st_g[k], (k, st_s, st_g)
    assert st_s["diffuse_shifts"] > 1000 and st_s["null_shifts"] > 1000   # (both phases ran)
    meets_the_bar(r, acc_s, st_s, film_s, f"{scene} {kw} as selected")
    meets_the_bar(r, acc_g, st_g, film_g, f"{scene} {kw} GVPM_EVAL_GENERIC=1")


FALLBACK = {
    "bre2d": dict(kw=dict(vol_technique=abi.GVPM_VOL_BRE2D, use_shift_null=0)),
    "use_shift_null=0": dict(kw=dict(use_shift_null=0)),
    "debug_shift=null": dict(kw=dict(debug_shift=abi.GVPM_SHIFT_NULL)),
    "GVPM_EXACT_ALL": dict(env={"GVPM_EXACT_ALL": "1"}),
    "host shifts": dict(kw=dict(use_manifold=1), oracle_kw=dict(use_manifold=0), host_shifts=True),
    "B=32": dict(env={"GVPM_BEAMS_PER_WAVE": "32"}),
}


@pytest.mark.parametrize("which", list(FALLBACK))
def test_configurations_of_the_generic_kernel_still_match_the_oracle(which, monkeypatch):
    f = FALLBACK[which]
    r = build("cbox", oracle_kw=f.get("oracle_kw"), **f.get("kw", {}))
    acc, st, film = device(r, monkeypatch, env=f.get("env"), host_shifts=f.get("host_shifts", False))
    meets_the_bar(r, acc, st, film, which)
