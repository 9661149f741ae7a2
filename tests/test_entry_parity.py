"""The per-entry parity bars (tests/entry_parity.py) on the CPU, with the oracle alone: every input of tests/entry_cases.py is
ADMITTED, both fp32 builds of the oracle PASS the three assertions at their full margins, and five mutations of the strict fp32
result are REJECTED, each by the assertion meant for it -- while the old global bar (L2 / luminance < 1e-4) accepts the first three.
That is the record of the gap the new bars close."""
import numpy as np
import pytest

import entry_cases as E
import entry_parity as P
from gvpm_amd import abi


@pytest.mark.parametrize("name", E.NAMES)
def test_admission(name):
    r = E.prepared(name)
    zero, tiny, compared = P.masks(r.r64, r.lum)
    rho = P.entry_stats(r.r32, r.r64, r.lum)
    print(P.report(name, dict(ref=P.percentiles(rho), dev=P.percentiles(P.entry_stats(r.rfast, r.r64, r.lum)), T=P.tail_bar(rho),
                              compared=int(compared.sum()), tiny=int(tiny.sum()), zero=int(zero.sum()))) + "  (device column: the fast build)")
    assert r.cnt64["evaluations"] >= 1000, r.cnt64
    assert r.cnt32 == r.cnt64, (r.cnt32, r.cnt64)
    assert rho.max() <= 2e-4, rho.max()
    assert P.tail_bar(rho) <= 1.6e-3
    assert tiny.sum() <= 0.01 * (~zero).sum(), (int(tiny.sum()), int((~zero).sum()))
    assert compared.sum() >= 1000


@pytest.mark.parametrize("name", E.NAMES)
def test_both_fp32_oracles_are_accepted(name):
    r = E.prepared(name)
    P.assert_entry_parity(r.r32, r.r64, r.r32, r.lum, what=f"{name}, strict fp32")
    s = P.assert_entry_parity(r.rfast, r.r64, r.r32, r.lum, what=f"{name}, fast-math fp32")
    print(P.report(name + " (fast-math build as the device)", s))


def rejected_by(letter, dev, r, **only):
    """the assertion `letter` alone (the other two switched off) rejects `dev`; returns its message"""
    flags = dict(zeros=False, bulk=False, tail=False)
    flags.update(only)
    with pytest.raises(AssertionError) as e:
        P.assert_entry_parity(dev, r.r64, r.r32, r.lum, **flags)
    assert f" {letter} (" in str(e.value), str(e.value)
    return str(e.value)


def accepted_by_the_others(dev, r, **off):
    flags = dict(zeros=True, bulk=True, tail=True)
    flags.update(off)
    P.assert_entry_parity(dev, r.r64, r.r32, r.lum, **flags)


def T_of(r):
    return P.tail_bar(P.entry_stats(r.r32, r.r64, r.lum))


@pytest.mark.parametrize("name", E.MUTATED)
def test_m1_one_entry_off_by_2T(name):
    r = E.prepared(name)
    T = T_of(r)
    compared = np.argwhere(P.masks(r.r64, r.lum)[2])
    rho = P.entry_stats(r.r32, r.r64, r.lum)
    idx = tuple(compared[int(np.argsort(rho)[rho.size // 2])])    # an entry of median fp32 error
    dev = r.r32.copy()
    dev[idx] *= 1 + 2 * T
    msg = rejected_by("C", dev, r, tail=True)
    assert f"(y {idx[0]}, x {idx[1]}, slot {idx[2] // 3}, channel {idx[2] % 3})" in msg, msg
    accepted_by_the_others(dev, r, tail=False)      # (A and B do not see it: one entry moves no percentile)
    assert P.l2(dev, r.r64, r.lum) < P.OLD_BAR, P.l2(dev, r.r64, r.lum)


# m2 and the old bar.  The row is 1 / H of the image and the old number grows with 2 T sqrt(row's share of the squares): under 1e-4
# on G-BRE's 24 x 20 (T 4.4e-4: the old number is 1.4e-5) and G-VPM's 20 x 16 (T 3.5e-5: 2.0e-6).  On the 16 x 12 images of G-Beams 1D
# (T 1.5e-3: 2.5e-4, above that driver's own 2e-4 too) and G-Planes (T 6.0e-4: 1.1e-4) a row-wide 2 T is within the old bar's sight,
# so the gap is asserted where it exists and the figure printed where it does not.
M2_UNDER_THE_OLD_BAR = ("bre cbox", "vpm cbox")


@pytest.mark.parametrize("name", E.MUTATED)
def test_m2_one_slot_of_the_last_row_off_by_2T(name):
    r = E.prepared(name)
    T = T_of(r)
    k = 3 * (1 + abi.GVPM_TOP)
    row = r.r64[-1, :, k:k + 3]
    assert (row >= P.TINY * r.lum).sum() >= 3, "the last row's shifted[TOP] must hold compared entries"
    dev = r.r32.copy()
    dev[-1, :, k:k + 3] *= 1 + 2 * T
    msg = rejected_by("C", dev, r, tail=True)
    assert f"(y {r.r64.shape[0] - 1}, " in msg and f"slot {1 + abi.GVPM_TOP}, " in msg, msg
    print(f"{name}: T {T:.2e}, old bar {P.l2(dev, r.r64, r.lum):.3e}")
    if name in M2_UNDER_THE_OLD_BAR:
        assert P.l2(dev, r.r64, r.lum) < P.OLD_BAR, P.l2(dev, r.r64, r.lum)


@pytest.mark.parametrize("name", E.MUTATED)
def test_m3_every_entry_biased_by_4e_6(name):
    r = E.prepared(name)
    dev = r.r32 * (1 + 4e-6)
    rejected_by("B", dev, r, bulk=True)
    accepted_by_the_others(dev, r, bulk=False)      # (no zero is touched and 4e-6 is far below T)
    assert P.l2(dev, r.r64, r.lum) < P.OLD_BAR, P.l2(dev, r.r64, r.lum)


@pytest.mark.parametrize("name", E.MUTATED)
def test_m4_a_stray_write_into_a_zero(name):
    r = E.prepared(name)
    zeros = np.argwhere(r.r64 == 0)
    assert len(zeros), "the case must have entries the oracle leaves at exactly 0"
    idx = tuple(zeros[len(zeros) // 2])
    dev = r.r32.copy()
    dev[idx] = 1e-6 * r.lum
    msg = rejected_by("A", dev, r, zeros=True)
    assert f"(y {idx[0]}, x {idx[1]}, slot {idx[2] // 3}, channel {idx[2] % 3})" in msg, msg
    accepted_by_the_others(dev, r, zeros=False)
    assert P.l2(dev, r.r64, r.lum) < P.OLD_BAR


@pytest.mark.parametrize("name", E.MUTATED)
def test_m5_a_lost_evaluation(name):
    r = E.prepared(name)
    dev, i, lost = E.lost_evaluation(r)
    print(f"{name}: record {i} removed, {lost} evaluations lost, old bar {P.l2(dev, r.r64, r.lum):.3e}")
    with pytest.raises(AssertionError) as e:
        P.assert_entry_parity(dev, r.r64, r.r32, r.lum, bulk=False)
    assert " C (" in str(e.value) or " A (" in str(e.value), str(e.value)


def test_messages_name_the_entry_and_the_three_values():
    r = E.prepared("bre cbox")
    dev = r.r32.copy()
    y, x, k = (int(v) for v in np.argwhere(P.masks(r.r64, r.lum)[2])[17])
    dev[y, x, k] *= 1.5
    with pytest.raises(AssertionError) as e:
        P.assert_entry_parity(dev, r.r64, r.r32, r.lum)
    for part in (f"(y {y}, x {x}, slot {k // 3}, channel {k % 3})", f"dev {float(dev[y, x, k])!r}", f"r64 {float(r.r64[y, x, k])!r}",
                 f"r32 {float(r.r32[y, x, k])!r}"):
        assert part in str(e.value), (part, str(e.value))


def test_tiny_entries():
    """0 < r64 < 1e-7 lum: not compared; the device may hold [0, 2e-7 lum] there, and more than 1 % of them is refused as an input"""
    r = E.prepared("bre cbox")
    r64 = r.r64.copy()
    idx = tuple(np.argwhere(r64 == 0)[3])
    r64[idx] = 5e-8 * r.lum
    dev = r.r32.copy()
    dev[idx] = 1.9e-7 * r.lum
    P.assert_entry_parity(dev, r64, r.r32, r.lum)
    for bad in (2.1e-7 * r.lum, -1e-12 * r.lum):
        dev[idx] = bad
        with pytest.raises(AssertionError, match=r"A \(tiny\)"):
            P.assert_entry_parity(dev, r64, r.r32, r.lum)
    many = r.r64.copy()
    many[many > 0] = np.where(np.arange((many > 0).sum()) % 50 == 0, 5e-8 * r.lum, many[many > 0])   # 2 % of the non-zero entries
    with pytest.raises(AssertionError, match=r"A \(inputs\)"):
        P.assert_entry_parity(many, many, many, r.lum)
