"""Scripted sessions on the device (tests/session_cases.py): ONE long-lived handle against the fp64 oracle, step by step.

Every test is one session.  Observed mode reads and compares after every step, so a failure names the step where the handle went
wrong; blind mode reads nothing before the end, so the deferred exact shifts, the flush pacing and the pipelines run as they do
in production, and must end where the observed run ended (counters equal, sums to the device-against-device bar) and where the
oracle's fold ends.  Bars: session_cases.BAR / EXACT_BAR / DEVICE_BAR -- the existing drivers' own."""
import time

import numpy as np
import pytest

import oracle_lib as O
import session_cases as S
from gvpm_amd import hip

pytestmark = pytest.mark.gpu
SESSIONS = S.all_sessions()


def report(s, res, folded, dev, err, bvo, t0):
    """one line per session for the notebook (pytest -s)"""
    evals = sum(f.cnt["evaluations"] for f in folded) if folded is not None else dev.stats["evaluations"]
    print(f"\nSESSION {s.name}: steps {len(res)} evaluations {evals} exact shifts taken {dev.exact[0]} lost {dev.exact[1]} "
          f"final L2 {err:.2e} blind-vs-observed L2 {'-' if bvo is None else format(bvo, '.2e')} wall {time.time() - t0:.2f} s")


def both_modes(name):
    """the session observed (every step against the oracle's fold), then blind; both ends against the oracle and each other"""
    t0 = time.time()
    s = SESSIONS[name]
    res, folded = S.prepared(s)
    observed = S.run_device(s, res, "observed", folded)
    S.check_final(s, res, folded, observed)
    blind = S.run_device(s, res, "blind")
    err = S.check_final(s, res, folded, blind)
    bvo = S.check_blind_against_observed(s, blind, observed)
    report(s, res, folded, blind, err, bvo, t0)
    return s, res, folded, observed, blind


@pytest.mark.parametrize("tech", list(S.TECH))
def test_collapse(tech):
    """counts N -> 1 -> 0 -> 1.5 N -> 64 -> N, beam sets all -> 37 -> none -> all, a central box then everywhere then a corner box,
    one gather again without uploading: what the rotating build sets, the cached bounds and the staging rings carry"""
    both_modes(f"collapse-{tech}")


@pytest.mark.parametrize("tech", ["bre3d", "vpm", "beams3d"])
def test_swap(tech):
    """scene 14 <-> 782 occluders, medium grey <-> all <-> thick, the global scale above every earlier radius under the large
    scene (the near grid's reach) and far below, gvpm_reset in the middle"""
    both_modes(f"swap-{tech}")


@pytest.mark.parametrize("tech", ["bre3d", "vpm"])
def test_tables(tech):
    """BSDF tables on one handle: changed, refused (run_device asserts the refusal; the gathers behind it are the oracle's under
    the previous table), with GVPM_BSDF_MIXTURE heads and without again -- bsdfMixtures flips both ways"""
    s, res, folded, observed, blind = both_modes(f"tables-{tech}")
    assert sum(r.refused_table is not None for r in res) == 2
    mixed = [bool((r.table["kind"] == S.abi.GVPM_BSDF_MIXTURE).any()) for r in res]
    assert sum(a != b for a, b in zip(mixed, mixed[1:])) >= 4


def test_formats():
    """the seven upload paths twice round on one handle against the oracle on the unpacked arrays, and against a plain-SoA
    session of the same arrays"""
    t0 = time.time()
    s = SESSIONS["formats-bre3d"]
    res, folded = S.prepared(s)
    assert [r.path for r in res] == list(S.PATHS) * 2 and len({r.rec.n for r in res}) > 10
    got = S.run_device(s, res, "observed", folded)
    err = S.check_final(s, res, folded, got)
    soa = S.run_device(s, res, "blind", force_path="soa")
    S.check_final(s, res, folded, soa)
    bvo = S.check_blind_against_observed(s, soa, got)
    report(s, res, folded, got, err, bvo, t0)


@pytest.mark.parametrize("tech", ["bre3d", "vpm", "beams3d"])
def test_exact_all(tech):
    """GVPM_EXACT_ALL=1 with GVPM_EXACT_EVERY=3: every shift of every step waits in the handle's list across gathers while the
    radius, `it`, the counts, the medium and the scene change between two flushes (session_cases.exact_all says where the
    driver's joins fall; test_sessions.py asserts that the paced flush and the uploads find entries waiting)"""
    s, res, folded, observed, blind = both_modes(f"exact_all-{tech}")
    total = S.expected_totals(res, folded)
    shifts = total["null_shifts"] + total["diffuse_shifts"] + total["failed_shifts"]
    assert max(f.cnt["evaluations"] for f in folded) < 15000      # three gathers' entries stay far below the list's quarter
    for dev in (observed, blind):
        taken, lost = dev.exact
        assert lost == 0 and taken >= shifts > 20000, (dev.exact, shifts)


def test_exact_all_glossy():
    """the same on cbox_conductor at the exact pass's glossy bar: the BSDF table changes, and is once refused, with one or two
    gathers' entries waiting (test_sessions.py asserts that they wait): the pass must run under the old table first"""
    s, res, folded, observed, blind = both_modes("exact_all-glossy")
    total = S.expected_totals(res, folded)
    shifts = total["null_shifts"] + total["diffuse_shifts"] + total["failed_shifts"]
    for dev in (observed, blind):
        assert dev.exact[1] == 0 and dev.exact[0] >= shifts > 20000, (dev.exact, shifts)


def test_exact_adaptive_pacing():
    """GVPM_EXACT_ALL=1, GVPM_EXACT_EVERY unset, blind: the paced flush behind the eighth gather and the one at the interval the
    driver then sets, each with 200 000 entries waiting (test_sessions.py); nothing lost, every shift taken, the exact bar"""
    t0 = time.time()
    s = SESSIONS["exact_adaptive-bre3d"]
    res, folded = S.prepared(s)
    blind = S.run_device(s, res, "blind")
    err = S.check_final(s, res, folded, blind)
    total = S.expected_totals(res, folded)
    shifts = total["null_shifts"] + total["diffuse_shifts"] + total["failed_shifts"]
    assert blind.exact[1] == 0 and blind.exact[0] >= shifts > 400000, (blind.exact, shifts)
    report(s, res, folded, blind, err, None, t0)


def test_exact_default_pacing():
    """GVPM_EXACT_EVERY unset, the kernels' own bands: 20 blind steps, the first nine successive, so the paced flush behind the
    eighth gather runs (on the few shifts the bands defer); nothing may be lost"""
    t0 = time.time()
    s = SESSIONS["exact_default-bre3d"]
    res, folded = S.prepared(s)
    blind = S.run_device(s, res, "blind")
    err = S.check_final(s, res, folded, blind)
    assert blind.exact[1] == 0
    report(s, res, folded, blind, err, None, t0)


def test_bundle_auto():
    """GVPM_BUNDLE_AUTO=1: the cell kind of every build as the rule of context.h predicts it (hysteresis, a moved origin), the
    counters exact at every step"""
    t0 = time.time()
    s = SESSIONS["bundle_auto-bre3d"]
    res, folded = S.prepared(s)
    dev = S.run_device(s, res, "observed", folded)
    err = S.check_final(s, res, folded, dev)
    assert dev.kinds == S.bundle_kinds(s, res), (dev.kinds, S.bundle_kinds(s, res))
    report(s, res, folded, dev, err, None, t0)


def test_marathon_bre3d():
    """288 blind steps at alpha = 1 cycling through three inputs: across the 256-entry event ring, the adaptive flush pacing and 96
    rotations of the build sets.  The oracle runs three times: the counters are 96 x the sum, the mean (A + B + C) / 3"""
    t0 = time.time()
    s = S.marathon("bre3d")
    res = S.materialise_cycle(s)
    parts = [S.oracle_step(s, r, 64, it=1) for r in res[:3]]
    dev = S.run_device(s, res, "blind")
    for k in S.COUNTERS:
        assert dev.stats[k] == 96 * sum(c[k] for _, c, _, _ in parts), (k, dev.stats)
    mean = sum(a for a, _, _, _ in parts) / 3
    err = S.l2(dev.acc, mean, mean[..., 0:3].mean())
    assert err < S.TOL, err
    assert dev.refused == 0 and dev.exact[1] == 0
    report(s, res, None, dev, err, None, t0)


def test_marathon_vpm():
    """48 blind G-VPM steps cycling through three inputs against the oracle's fold of all 48 (the per-pixel state is a real fold)"""
    t0 = time.time()
    s = S.marathon("vpm")
    res = S.materialise_cycle(s)
    folded = S.fold(s, res, 64)
    dev = S.run_device(s, res, "blind")
    err = S.check_final(s, res, folded, dev)
    assert dev.exact[1] == 0
    report(s, res, folded, dev, err, None, t0)


def test_poisson_interleaved():
    """poisson_solve between the gathers of one session: two sizes A, B, A, the three presets, with and without a throughput image
    (alpha forced to 0), once with cg_tolerance > 0 (the host-checked path).  Every solve equals the same solve on a fresh handle
    bit for bit (the solver is deterministic by design), and the gathers behind each solve are the oracle's (observed mode).
    The oracle's solver cannot be told to stop early, so the cg_tolerance solve is compared with the fresh handle only."""
    t0 = time.time()
    s = SESSIONS["collapse-bre3d"]
    res, folded = S.prepared(s)
    rng = np.random.default_rng(3)

    def images(W, H):
        dx, dy = (rng.standard_normal((H, W, 3)).astype(np.float32) * 0.1 for _ in range(2))
        return dx, dy, rng.random((H, W, 3)).astype(np.float32)

    A, B = images(33, 20), images(64, 48)
    tolerant = hip.poisson_preset("L2D")
    # (the presets check every 100 iterations of at most 50, i.e. never after the start: a check every 5, and a tolerance on
    # r.z -- absolute, summed over the channels, some thousands at the start for these images -- that CG crosses on its way)
    tolerant.alpha, tolerant.cg_iter_check, tolerant.cg_tolerance = 0.2, 5, 10.0
    plan = {0: (A, "L1D", True, None), 1: (B, "L2D", True, None), 2: (A, "L2Q", True, None), 4: (A, "L1D", False, None),
            5: (B, "L2D", True, tolerant), 7: (A, "L1D", True, None), 8: (B, "L2Q", False, None)}
    solved = {}

    def solve(ctx, k):
        (dx, dy, tp), preset, with_tp, params = plan[k]
        return ctx.poisson_solve(dx, dy, tp if with_tp else None, None, preset, 0.2, params=params)

    def hook(ctx, r):
        if r.k in plan:
            solved[r.k] = solve(ctx, r.k)

    dev = S.run_device(s, res, "observed", folded, hook=hook)
    err = S.check_final(s, res, folded, dev)
    assert sorted(solved) == sorted(plan)
    for k in plan:
        fresh = hip.Context(res[0].p, device=0)
        try:
            want = solve(fresh, k)
            if plan[k][3] is not None:
                # the tolerance must have ended the solve early: the same solve without it runs on and ends elsewhere
                (dx, dy, tp), preset, _, _ = plan[k]
                every = hip.poisson_preset(preset)
                every.alpha, every.cg_iter_check, every.cg_tolerance = 0.2, 5, 1e-30     # the same loop, never satisfied
                full = fresh.poisson_solve(dx, dy, tp, None, params=every)
                assert np.isfinite(full).all()
                assert not np.array_equal(want, full)
        finally:
            fresh.close()
        assert np.isfinite(want).all() and np.array_equal(solved[k], want), (k, plan[k][1])
    # the untouched presets against the oracle, at test_random_images_and_edge_sizes' bars
    for k, tol in ((0, 2e-3), (1, 2e-5), (2, 1e-4)):
        (dx, dy, tp), preset, _, _ = plan[k]
        ref = O.poisson_solve(dx, dy, tp, None, preset, 0.2)
        assert float(np.abs(solved[k] - ref).max() / np.abs(ref).max()) < tol, (k, preset)
    assert np.array_equal(solved[0], solved[7])
    report(s, res, folded, dev, err, None, t0)
