"""The device side of tests/test_scatter_near_gpu.py, as a process of its own: GVPM_NEAR_SCALAR is read once, in gvpm_create, so
each setting gets a fresh child that has not opened the GPU before (python tests/scatter_near_worker.py --out FILE.npz, the
setting in the environment).  Also the inputs both sides share: the seeded synthetic scenes, two iterations on one handle.

Writes, per case, the 27 accumulators after the last iteration and the summed counters."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases  # noqa: E402
import oracle_lib as O  # noqa: E402
from gvpm_amd import abi, hip  # noqa: E402

W = H = 32
NPH = 20000
ITERS = (1, 2)
SCALE = 3.0
# all of 64 or fewer occluders: the linear scan of near_lists.h (asserted where the inputs are made)
# case: (scene, parameters).  ShadowEpsilon 0.2 makes the as-written shadow segment a fifth of the reconnection distance and
# dmax a quarter of the room: lists of real occluders, most of them longer than the inline slots (the extension lists' second
# visit), and reconnections that a block occludes.
BRE_CASES = {"cbox": ("cbox", {}), "cbox_rot": ("cbox_rot", {}), "laser": ("laser", {}),
             "cbox_rot-se0.2": ("cbox_rot", dict(shadow_epsilon=0.2))}
VPM_SCENE, VPM_SCALE, VPM_SAMPLES = "cbox_rot", 5.0, 8
COUNTERS = ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts")


class Run:
    pass


def bre_inputs(case):
    """the case and, per iteration, (photons, emitted paths, camera beams) and the radius G-BRE shrinks to"""
    scene, kw = BRE_CASES[case]
    r = Run()
    r.c = cases.make_case(scene, W, H, NPH, SCALE, **kw)
    assert r.c.tris[0].shape[0] <= 64, scene
    r.steps, r.radii, scale = [], [], r.c.p.initial_scale_volume
    for it in ITERS:
        ph, nb = r.c.sc.shoot_photons(it, NPH)
        r.steps.append((ph, nb, r.c.sc.camera_beams(it)))
        r.radii.append(cases.radius_of(r.c.p, np.float32(scale)))
        scale = np.float32(O.scale_volume_apa(float(scale), it, float(r.c.p.alpha), r.c.p.vol_technique))
    return r


def vpm_inputs():
    """G-VPM on the same frame: its build goes through reorder_kernel (grid_build.hip)"""
    r = Run()
    r.c = cases.make_case(VPM_SCENE, W, H, NPH, VPM_SCALE, vol_technique=abi.GVPM_DISTANCE, nb_camera_samples=VPM_SAMPLES)
    assert r.c.tris[0].shape[0] <= 64
    r.steps = []
    for it in ITERS:
        ph, nb = r.c.sc.shoot_photons(it, NPH)
        rays, samples = r.c.sc.camera_beams_and_vpm_samples(it, VPM_SAMPLES)
        r.steps.append((ph, nb, rays, samples))
    return r


def device_bre(r):
    ctx = hip.Context(r.c.p, device=0)
    try:
        ctx.upload_scene(*r.c.tris)
        ctx.upload_medium(r.c.m)
        cases.upload_bsdfs(ctx, r.c)
        for it, (ph, nb, rays), radius in zip(ITERS, r.steps, r.radii):
            assert ctx.radius() == radius
            ctx.upload_photons(ph)
            ctx.upload_camera_beams(rays)
            ctx.gather(it, nb)
        return ctx.download_accum(), ctx.stats()
    finally:
        ctx.close()


def device_vpm(r):
    ctx = hip.Context(r.c.p, device=0)
    try:
        ctx.upload_scene(*r.c.tris)
        ctx.upload_medium(r.c.m)
        cases.upload_bsdfs(ctx, r.c)
        for it, (ph, nb, rays, samples) in zip(ITERS, r.steps):
            ctx.upload_photons(ph)
            ctx.upload_camera_beams(rays)
            ctx.upload_vpm_samples(samples)
            ctx.gather(it, nb)
        return ctx.download_accum(), ctx.stats()
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    out, stats = {}, {}
    for case in BRE_CASES:
        acc, st = device_bre(bre_inputs(case))
        out["acc_" + case] = acc
        stats[case] = {k: int(st[k]) for k in COUNTERS}
    acc, st = device_vpm(vpm_inputs())
    out["acc_vpm"] = acc
    stats["vpm"] = {k: int(st[k]) for k in COUNTERS}
    np.savez(a.out, stats=json.dumps(stats), **out)


if __name__ == "__main__":
    main()
