"""The scripted sessions of tests/session_cases.py on the CPU: admission of every session by the fp32 oracle, and a proof that
the observed-mode comparator reports stale state at the step where it happens.

Admission (the manner of medium_cases.py).  The reference's Float is float, so the oracle at precision=32 is the reference's own
arithmetic.  A session is admitted only if at EVERY step the fp32 oracle's four counters equal the fp64 oracle's, its folded
output is finite, and its L2 against the fp64 oracle's fold (27 accumulators / mean luminance, the largest over the session's
steps) stays at least 4x under the bar its technique's driver asserts.  G-Planes is judged by counters and finiteness only
(medium_cases.py: the fp32 oracle is no yardstick for it).  Every session holds at least 12 gathers, at least three steps with
more than 1 000 evaluations and at least one with none.  Measured (largest step L2 / L2 of the last step, fp32 against fp64):

  session               steps  evaluations  largest   last      session               steps  evaluations  largest   last
  collapse-bre3d        12     18 114       9.2e-7    6.2e-7    tables-bre3d          12     45 016       2.6e-7    1.5e-7
  collapse-bre2d        12     14 998       2.6e-7    1.5e-7    tables-vpm            12     50 979       5.6e-7    3.4e-7
  collapse-vpm          12     22 505       5.1e-7    1.8e-7    formats-bre3d         14     37 379       3.3e-7    1.9e-7
  collapse-beams3d      12     46 587       9.8e-7    6.3e-7    exact_all-bre3d       16     39 207       6.0e-7    3.7e-7
  collapse-beams1d      12     29 919       1.3e-5    7.8e-7    exact_all-vpm         16     24 291       3.1e-7    3.0e-7
  collapse-planes       12     290 126      (1.7e-5)  (1.3e-5)  exact_all-beams3d     16     75 854       5.5e-7    3.2e-7
  swap-bre3d            13     79 867       2.7e-6    2.1e-7    exact_all-glossy      13     69 816       2.6e-7    1.2e-7
  swap-vpm              13     34 583       4.9e-7    2.0e-7    exact_default-bre3d   20     61 236       4.3e-7    1.8e-7
  swap-beams3d          13     110 439      3.0e-6    3.8e-7    exact_adaptive-bre3d  20     125 935      2.8e-7    1.3e-7
  bundle_auto-bre3d     12     19 803       1.2e-6    2.8e-7

Counters equal and output finite everywhere.  Three sessions were softened (another draw of their inputs; see collapse(),
tables() and exact_all()): never a bar.
"""
import numpy as np
import pytest

import session_cases as S

SESSIONS = S.all_sessions()


def admit(s, res, f64, f32):
    assert len(res) >= 12
    evals = [f.cnt["evaluations"] for f in f64]
    assert sum(e > 1000 for e in evals) >= 3, evals
    assert sum(e == 0 for e in evals) >= 1, evals
    worst = 0.0
    for r, a, b in zip(res, f64, f32):
        for k in S.COUNTERS:
            assert a.cnt[k] == b.cnt[k], (S.describe(s, r), k, a.cnt, b.cnt)
        assert np.isfinite(b.acc).all(), S.describe(s, r)
        worst = max(worst, S.l2(b.acc, a.acc, a.lum))
    print(f"ADMIT {s.name}: steps {len(res)} evaluations {sum(evals)} largest step L2 {worst:.2e} "
          f"last {S.l2(f32[-1].acc, f64[-1].acc, f64[-1].lum):.2e}")
    if s.tech != "planes":
        assert worst * 4 <= S.BAR[s.tech], (s.name, worst)


@pytest.mark.parametrize("name", sorted(SESSIONS))
def test_session_is_admitted_by_the_fp32_oracle(name):
    s = SESSIONS[name]
    res, f64 = S.prepared(s)
    admit(s, res, f64, S.fold(s, res, 32))


def test_marathon_inputs_are_admitted():
    """the three inputs of the G-BRE marathon one by one (its 288 steps repeat them at one radius), G-VPM's 48 steps as a fold"""
    s = S.marathon("bre3d")
    res = S.materialise_cycle(s)
    assert len(res) == 288 and len({r.rec.n for r in res[:3]}) == 3
    evals = []
    for r in res[:3]:
        a, c64, _, _ = S.oracle_step(s, r, 64, it=1)
        b, c32, _, _ = S.oracle_step(s, r, 32, it=1)
        assert all(c64[k] == c32[k] for k in S.COUNTERS) and np.isfinite(b).all(), (c64, c32)
        evals.append(c64["evaluations"])
        if c64["evaluations"]:
            assert S.l2(b, a, a[..., 0:3].mean()) * 4 <= S.BAR["bre3d"]
    assert sum(e > 1000 for e in evals) == 2 and evals[2] == 0, evals
    assert len({r.radius for r in res}) == 1       # alpha = 1: the radius never moves
    s = S.marathon("vpm")
    res = S.materialise_cycle(s)
    assert len(res) == 48
    admit(s, res, S.fold(s, res, 64), S.fold(s, res, 32))


# ---- the comparator bites -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def collapse():
    s = SESSIONS["collapse-bre3d"]
    res, f64 = S.prepared(s)
    return s, res, f64, S.perfect_observations(s, res, f64)


def test_comparator_passes_the_oracle_itself(collapse):
    s, res, f64, obs = collapse
    assert S.first_failure(s, res, f64, obs) is None
    # the statement the tampered folds are written in IS the oracle's fold when nothing is tampered with
    again = S.fold(s, res, 64, tamper=("python", "every"))
    for a, b in zip(f64, again):
        assert a.cnt == b.cnt and np.allclose(a.acc, b.acc, rtol=1e-13, atol=0)


@pytest.mark.parametrize("kind,k", [("radius", 4), ("twice", 7), ("dropped", 1), ("rescale", 9)])
def test_comparator_reports_stale_state_at_its_step(collapse, kind, k):
    """An oracle fold that is wrong at step k the way stale state would make the device wrong -- the previous step's radius, the
    step's contribution added twice, dropped, the running sum not rescaled where `it` jumps (9 -> 11) -- against observations that
    are right: the comparator must name step k and no other, i.e. pass every step before it and stop there (the steps behind a
    wrong one inherit its error through the fold, so the first miss is the one a report names)."""
    s, res, f64, obs = collapse
    if kind == "rescale":
        assert res[k].it - 1 != res[k - 1].it
    if kind == "radius":
        assert res[k].radius != res[k - 1].radius
    wrong = S.fold(s, res, 64, tamper=(kind, k))
    got = S.first_failure(s, res, wrong, obs)
    assert got is not None and got[0] == k, (kind, k, got)
    assert "step %d " % k in S.describe(s, res[got[0]])


def test_bundle_rule_on_the_bundle_session():
    """the sequence of cell kinds the rule of context.h predicts for the bundle_auto session meets every branch of it"""
    s = SESSIONS["bundle_auto-bre3d"]
    res, _ = S.prepared(s)
    kinds = S.bundle_kinds(s, res)
    assert kinds == [1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 0]
    cover = [r.rays.shape[0] / (s.W * s.H) for r in res]
    assert any(0.4 < c <= 0.5 and k == 0 for c, k in zip(cover, kinds))     # half, arriving from the whole frame: stays 3D
    assert any(0.4 < c <= 0.5 and k == 1 for c, k in zip(cover, kinds))     # half, arriving from a share: stays bundle


# ---- the exact sessions reach what they are for --------------------------------------------------------------------------------------
def passes(name):
    s = SESSIONS[name]
    res, f64 = S.prepared(s)
    return S.exact_passes(s, res, f64)


@pytest.mark.parametrize("tech", ["bre3d", "vpm"])
def test_exact_all_meets_the_paced_flush_and_the_uploads_with_entries_waiting(tech):
    """exact_passes() mirrors the driver's join points.  Under GVPM_EXACT_EVERY=3 the paced flush must fire behind three gathers
    with 30 000 entries or more waiting, and the medium and scene uploads must find one or two gathers' entries in the list, for
    G-BRE and for G-VPM; G-BRE's `it` skip is a join of its own."""
    got = passes(f"exact_all-{tech}")
    paced = [p for p in got if p[1] == "paced"]
    assert paced and paced[0][2:] >= (3, 30000), got
    uploads = [p for p in got if p[1] == "upload"]
    assert {p[2] for p in uploads} == {1, 2} and all(p[3] > 3000 for p in uploads), got
    assert all((p[0] + 1) % 3 for p in uploads)                     # steps counted from 1: no multiple of three
    assert any(p[1] == "it" for p in got) == (tech == "bre3d")


def test_exact_all_glossy_changes_the_table_with_entries_waiting():
    got = passes("exact_all-glossy")
    uploads = [p for p in got if p[1] == "upload"]
    assert len(uploads) == 4 and {p[2] for p in uploads} == {1, 2} and all(p[3] > 20000 for p in uploads), got
    s = SESSIONS["exact_all-glossy"]
    refused = [r.k for r in S.prepared(s)[0] if r.refused_table is not None]
    assert refused and all(any(p[0] == k and p[1] == "upload" for p in got) for k in refused)
    assert sum(p[1] == "paced" for p in got) >= 2


def test_exact_adaptive_fires_at_the_default_interval_and_at_the_one_it_sets():
    """8 gathers, then the interval the first pass sets (9 to 12 gathers), both inside the session; what either pass finds stays
    under a quarter of the 2^20-entry list, so the list is never regrown (a regrowth would allocate 2 GB on a shared card)"""
    got = passes("exact_adaptive-bre3d")
    assert [p[1] for p in got] == ["paced", "paced"] and got[0][2] == 8 and 9 <= got[1][2] <= 12, got
    assert all(100000 < p[3] < (1 << 20) // 4 for p in got), got
    s = SESSIONS["exact_adaptive-bre3d"]
    assert max(f.cnt["evaluations"] for f in S.prepared(s)[1]) < 15000


def test_exact_default_runs_eight_successive_gathers():
    s = SESSIONS["exact_default-bre3d"]
    its = [r.it for r in S.prepared(s)[0]]
    assert its[:9] == list(range(1, 10)) and len(its) == 20 and its[9] == 11
