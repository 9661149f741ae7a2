"""The host codecs of the side inputs (include/gvpm_hip.h, "packed photon beams, photon planes and G-VPM samples"): the
octahedral code of the beams' end normals, the run packer of the G-VPM samples, and the linked packer on beam records.
Plain host code: no GPU."""
import numpy as np
import pytest

import cases
from gvpm_amd import abi, hip
from test_oracle_vpm import make_vpm_case

AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)


# ---- end normals ---------------------------------------------------------------------------------------------------------
def test_normal_codec_zero_axes_accuracy_and_idempotence():
    assert hip.pack_normals_oct(np.zeros((1, 3), np.float32))[0] == abi.GVPM_OCT_ZERO == 0x80008000
    assert np.array_equal(hip.unpack_normals_oct(np.array([abi.GVPM_OCT_ZERO], np.uint32)), np.zeros((1, 3), np.float32))
    # axis-aligned normals are exact (the walls of every test scene)
    assert np.array_equal(hip.unpack_normals_oct(hip.pack_normals_oct(AXES)), AXES)
    v = np.random.default_rng(11).normal(size=(10000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    codes = hip.pack_normals_oct(v.astype(np.float32))
    back = hip.unpack_normals_oct(codes).astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(back, axis=1) - 1.0) < 1e-6)
    # the angle through the cross product: arccos of a dot product near 1 has no resolution at 1e-5 rad
    angle = np.arctan2(np.linalg.norm(np.cross(back, v), axis=1), np.sum(back * v, axis=1))
    print("largest angle", angle.max())
    assert angle.max() <= 4.8e-5   # the header's bound for parent_n, the same code
    # a code is a fixed point
    assert np.array_equal(hip.pack_normals_oct(back.astype(np.float32)), codes)
    assert np.array_equal(hip.pack_normals_oct(hip.unpack_normals_oct(hip.pack_normals_oct(AXES))), hip.pack_normals_oct(AXES))
    assert hip.pack_normals_oct(np.zeros((0, 3), np.float32)).size == 0


# ---- G-VPM samples as runs -----------------------------------------------------------------------------------------------
def roundtrip(samples):
    runs, rands = hip.pack_vpm_samples(samples)
    assert rands.size == samples.size and int(runs["count"].sum()) == samples.size
    back = hip.unpack_vpm_samples(runs, rands)
    assert back.tobytes() == np.ascontiguousarray(samples).tobytes()
    return runs


@pytest.mark.parametrize("scene", ["cbox", "cbox_mirror"])
def test_run_packer_round_trips_the_samples_of_a_frame(scene):
    c = make_vpm_case(scene, 24, 20, 100, 5.0, nb=8)
    assert c.samples.size > 1000
    runs = roundtrip(c.samples)
    # maximal runs: neighbours differ in set or in the bits of pdf_sel
    same = (runs["set"][1:] == runs["set"][:-1]) & (runs["pdf_sel"][1:].view(np.uint32) == runs["pdf_sel"][:-1].view(np.uint32))
    assert not same.any()
    assert np.array_equal(runs["first"], np.concatenate([[0], np.cumsum(runs["count"])[:-1]]).astype(np.uint32))
    if scene == "cbox":
        # one medium edge a pixel: a run a pixel, 4 + 16 / nb bytes a sample
        assert runs.size * 8 == c.samples.size
    else:
        # two sets behind the mirror's pixels, chosen with probability below 1
        assert np.any(c.samples["pdf_sel"] != 1.0) and runs.size * 8 > c.samples.size


@pytest.mark.parametrize("nb", [1, 8, 64, 70])
def test_run_packer_round_trips_every_run_length(nb):
    c = make_vpm_case("cbox", 8, 6, 100, 5.0, nb=nb)
    runs = roundtrip(c.samples)
    assert runs["count"].max() == nb
    for n in (0, 1):
        assert roundtrip(c.samples[:n]).size == n


def test_run_packer_keeps_the_bits_and_refuses_reserved():
    s = np.zeros(6, abi.VPM_SAMPLE_DTYPE)
    s["set"] = [3, 3, 3, 3, 4, 4]
    s["pdf_sel"] = [0.0, -0.0, np.nan, np.nan, 0.5, 0.5]   # (-0 and 0 are two runs; the two NaNs share their bits: one)
    s["rand"] = np.linspace(0.1, 0.9, 6)
    assert roundtrip(s).size == 4
    s["reserved"][2] = 1
    with pytest.raises(hip.GvpmError):
        hip.pack_vpm_samples(s)


def malformed_run_lists(n=20):
    """[(what, runs, n)]: every rule of gvpm_unpack_vpm_samples broken once, from a good list of three runs over n samples"""
    good = np.zeros(3, abi.VPM_RUN_DTYPE)
    good["set"], good["pdf_sel"] = [0, 1, 2], 1.0
    good["first"], good["count"] = [0, 8, 12], [8, 4, n - 12]
    out = []

    def bad(what, edit, total=n):
        r = good.copy()
        edit(r)
        out.append((what, r, total))

    bad("first run not at sample 0", lambda r: r["first"].__setitem__(0, 1))
    bad("a gap between two runs", lambda r: r["first"].__setitem__(1, 9))
    bad("two runs overlap", lambda r: r["first"].__setitem__(2, 11))
    bad("an empty run", lambda r: r["count"].__setitem__(1, 0))
    bad("counts short of n", lambda r: None, total=n + 1)
    bad("counts beyond n", lambda r: None, total=n - 1)
    out.append(("runs for no samples", good.copy(), 0))
    out.append(("samples without runs", good[:0].copy(), n))
    return good, out


def test_unpack_refuses_every_malformed_run_list():
    good, bads = malformed_run_lists()
    rands = np.linspace(0.0, 0.9, 40).astype(np.float32)
    assert hip.unpack_vpm_samples(good, rands[:20]).size == 20
    for what, runs, n in bads:
        with pytest.raises(hip.GvpmError):
            hip.unpack_vpm_samples(runs, rands[:n])
            pytest.fail(what)


# ---- the linked packer on beam records -----------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cbox", "laser"])
def test_linked_packer_carries_beam_records(scene):
    c = cases.make_case(scene, 16, 12, 10, 3.0)
    beams, end_n, _ = c.sc.shoot_beams(1, 12000)
    assert beams.n > 1000
    t = hip.MaterialTable()
    blob = hip.pack_photons_linked(beams, t)
    hd = hip.linked_header(blob)
    print(scene, "beams", beams.n, "bytes a beam", blob.size / beams.n, "chain / emit / full",
          hd["n_chain"] / beams.n, hd["n_emit"] / beams.n, hd["n_full"] / beams.n)
    assert hd["n"] == beams.n and blob.size <= 76 * beams.n + 65536
    got = hip.unpack_photons_linked(blob, t)
    # everything the records carry in fp32 (or as an index of a table of fp32 entries), whatever kind the packer chose
    for k in ("pos", "parent_pos", "flux", "prefix_w", "parent_pdf", "edge_pdf", "parent_rr", "parent_scat", "parent_g", "flags"):
        assert np.ascontiguousarray(getattr(got, k)).tobytes() == np.ascontiguousarray(getattr(beams, k)).tobytes(), k
    # what the gathers read of path_id (beams_build.hip: the checkerboard parity)
    assert np.array_equal(got.path_id, beams.path_id & 1)
    # wi is derived: normalize(parent_pos - pos) -- which is what a beam's wi IS, to the rounding of the producer's fp32
    d = beams.parent_pos.astype(np.float64) - beams.pos.astype(np.float64)
    ln = np.linalg.norm(d, axis=1)
    ok = ln > 0
    assert np.allclose(got.wi[ok], (d[ok] / ln[ok, None]).astype(np.float32), rtol=0, atol=1e-7)
    # the end normals of these scenes: walls (axis-aligned: exact) and medium vertices (zero)
    assert np.array_equal(hip.unpack_normals_oct(hip.pack_normals_oct(end_n)), end_n)
