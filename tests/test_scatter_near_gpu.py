"""The photon scatter's near-occluder lists for small scenes (near_lists.h): the linear scan over <= 64 occluders reads its
table through the scalar cache; GVPM_NEAR_SCALAR=0 keeps the scan with per-lane vector loads.  Same visit order, same fp32
expressions => the same lists => the same shadow-ray outcomes: both settings must give the fp64 oracle's counters, and each
other's.

Shapes: a 32 x 32 frame, 20 000 photons, two iterations on one handle (tests/scatter_near_worker.py).  Scenes: cbox (every
surface parent sits on an axis-aligned wall: ownWall's in-front branch), cbox_rot (the tilted Cornell blocks: parents with
real occluders within dmax, and tilted walls, whose parents lie behind their plane by rounding as often as in front), laser
(the coplanar aperture quads).  One G-VPM case, whose build goes through reorder_kernel instead of the build chain's tail.

Inputs, checked on the CPU with the oracle (NOTEBOOK.md round 24): every scene has reconnections (diffuse_shifts > 0 is
asserted below).  In cbox_rot as configured NO reconnection is occluded by a block, at this size or with the camera window
moved over a larger frame: the as-written shadow segment is ShadowEpsilon = 1e-3 of the reconnection distance, and the oracle
counts the same failed shifts with the blocks among the occluders as without.  The case stays (tilted walls, the blocks'
triangles in every scan), and a fourth one is added: cbox_rot with ShadowEpsilon 0.2 -- segments a fifth of the distance,
dmax a quarter of the room: lists of real occluders, most of them longer than the inline slots (the extension lists and their
second visit), and a few reconnections that a block does occlude (asserted below against the oracle without the blocks).

Each setting runs in a fresh child process: the switch is read once, in gvpm_create.

Bar: evaluations, null_shifts, diffuse_shifts and failed_shifts == the fp64 oracle's, in both settings; L2 of the 27
accumulators over the mean reference luminance < 1e-3 ("Parity bar")."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import scatter_near_worker as SW
from test_parity_gpu import l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-3
SETTINGS = {"scalar": None, "vector": "0"}   # GVPM_NEAR_SCALAR of the child (None: unset, the default)


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """{setting: (accumulators by case, counters by case)}: one child per setting, every case in it"""
    got = {}
    for name, flag in SETTINGS.items():
        path = str(tmp_path_factory.mktemp("scatter_near") / (name + ".npz"))
        env = {k: v for k, v in os.environ.items() if k != "GVPM_NEAR_SCALAR"}
        if flag is not None:
            env["GVPM_NEAR_SCALAR"] = flag
        out = subprocess.run([sys.executable, SW.__file__, "--out", path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:] + out.stdout[-1000:]
        z = np.load(path)
        got[name] = (z, json.loads(str(z["stats"])))
    return got


_refs = {}


def bre_reference(scene, tris=None):
    """the fp64 oracle's fold over the two iterations and its summed counters, once per (scene, occluders)"""
    key = (scene, tris is None)
    if key not in _refs:
        r = SW.bre_inputs(scene)
        O.set_bsdfs(r.c.bsdfs)
        ref, total = None, dict.fromkeys(SW.COUNTERS, 0)
        for it, (ph, nb, rays), radius in zip(SW.ITERS, r.steps, r.radii):
            ref, cnt, _ = O.gather_bre(r.c.p, r.c.m, r.c.tris if tris is None else tris(r.c.tris), ph, rays, radius, it, nb, 64,
                                       use_accel=False, accum=ref)
            for k in SW.COUNTERS:
                total[k] += cnt[k]
        _refs[key] = (ref, total)
    return _refs[key]


def held(device, case, ref, cnt):
    lum = max(ref[..., 0:3].mean(), 1e-30)
    for name in SETTINGS:
        z, stats = device[name]
        err = l2(z["acc_" + case], ref, lum)
        print(case, name, "device", stats[case], "oracle", cnt, "L2 accum / lum", err)
    for name in SETTINGS:
        z, stats = device[name]
        for k in SW.COUNTERS:
            assert stats[case][k] == cnt[k], (case, name, k, stats[case], cnt)
        assert l2(z["acc_" + case], ref, lum) < BAR, (case, name)
    assert device["scalar"][1][case] == device["vector"][1][case]


@pytest.mark.parametrize("scene", list(SW.BRE_CASES))
def test_both_scans_give_the_oracles_counters(scene, device):
    ref, cnt = bre_reference(scene)
    assert cnt["diffuse_shifts"] > 0 and cnt["evaluations"] > 1000, cnt   # (reconnections: the lists are read)
    held(device, scene, ref, cnt)


def test_the_blocks_of_cbox_rot_occlude_reconnections_at_shadow_epsilon_02():
    """the input of the cbox_rot-se0.2 case: without the two blocks among the occluders (synth.cpp makeScene: the room's twelve
    triangles, the blocks' twenty-four, the light's two) the oracle's shadow rays fail less often -- some reconnections are
    occluded by a block.  (At the scene's own ShadowEpsilon none is: the two counts are printed.)"""
    ncbox, nrot = SW.bre_inputs("cbox").c.tris[0].shape[0], SW.bre_inputs("cbox_rot").c.tris[0].shape[0]
    assert (ncbox, nrot) == (14, 38)
    keep = np.r_[0:ncbox - 2, nrot - 2:nrot]
    for case in ("cbox_rot", "cbox_rot-se0.2"):
        _, with_blocks = bre_reference(case)
        _, without = bre_reference(case, tris=lambda t: tuple(np.ascontiguousarray(x[keep]) for x in t))
        print(case, "failed shifts: with the blocks", with_blocks["failed_shifts"], "room only", without["failed_shifts"])
    assert with_blocks["failed_shifts"] > without["failed_shifts"]


def test_vpm_build_through_reorder_kernel(device):
    r = SW.vpm_inputs()
    O.set_bsdfs(r.c.bsdfs)
    ref = sv = nv = None
    total = dict.fromkeys(SW.COUNTERS, 0)
    for ph, nb, rays, samples in r.steps:
        ref, sv, nv, cnt, _ = O.gather_vpm(r.c.p, r.c.m, r.c.tris, ph, rays, samples, 64, use_accel=False, accum=ref, scale_vol=sv, n_vol=nv)
        for k in SW.COUNTERS:
            total[k] += cnt[k]
    assert total["diffuse_shifts"] > 0 and total["evaluations"] > 1000, total
    held(device, "vpm", ref, total)
