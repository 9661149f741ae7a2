"""G-BRE traversal, its two instantiations (gather_bre.hip traverse_bre_kernel<B, OWN_WALK>): the one that reads the
planner's slab boxes (the default) and the one that computes every box from its own beams (GVPM_PLAN_BOXES=0, or a grid
dimension of 1024 or more).  The boxes only select the staged photons -- the hit test, hence the evaluated set, is the
same -- so the counters must be equal, to each other and to the oracle's, and the sums may differ by their order only."""
import os

import numpy as np
import pytest

import cases
import oracle_lib as O
from gvpm_amd import hip

pytestmark = pytest.mark.gpu
COUNTERS = ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts")


def run(c, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = hip.Context(c.p, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    ctx.upload_scene(*c.tris)
    ctx.upload_medium(c.m)
    ctx.upload_photons(c.ph)
    ctx.upload_camera_beams(c.rays)
    ctx.gather(c.it, c.nb)
    acc = ctx.download_accum().astype(np.float64)
    st = ctx.stats()
    ctx.close()
    return acc, st


def assert_same(a0, s0, a1, s1):
    for k in COUNTERS:
        assert s1[k] == s0[k], (k, s0, s1)
    lum = max(a0[..., 0:3].mean(), 1e-30)
    assert np.abs(a1 - a0).max() <= 2e-4 * max(np.abs(a0).max(), lum)


@pytest.mark.parametrize("scene", ["cbox", "cbox_hg", "laser"])
@pytest.mark.parametrize("bpw", ["16", "32", "64"])
def test_own_walk_and_plan_boxes_give_the_same_pairs(scene, bpw):
    c = cases.make_case(scene, 48, 40, 30000, 3.0)
    env = {"GVPM_BEAMS_PER_WAVE": bpw}
    a1, s1 = run(c, dict(env, GVPM_PLAN_BOXES="1"))
    a0, s0 = run(c, dict(env, GVPM_PLAN_BOXES="0"))
    assert s1["evaluations"] > 10000
    assert_same(a0, s0, a1, s1)


@pytest.mark.parametrize("plan_boxes", ["0", "1"])
def test_both_paths_match_the_oracle_with_coalesced_staging_and_no_prefilter(plan_boxes):
    # every staging window through the dense-box branch (GVPM_COALESCE_AT=1), every staged photon tested (no cylinder)
    c = cases.make_case("cbox_hg", 40, 32, 20000, 3.0)
    base, sb = run(c, {"GVPM_PLAN_BOXES": plan_boxes})
    acc, st = run(c, {"GVPM_PLAN_BOXES": plan_boxes, "GVPM_COALESCE_AT": "1", "GVPM_TRAV_PREFILTER": "0"})
    assert_same(base, sb, acc, st)
    _, cnt, _ = O.gather_bre(c.p, c.m, c.tris, c.ph, c.rays, c.r, c.it, c.nb, 64)
    for k in COUNTERS:
        assert st[k] == cnt[k], (k, st, cnt)
