"""The device generators over glossy scenes, CPU side (gvpm_devgen_create_ex, include/gvpm_hip.h): what the host library hands over as
a scene's materials against the scene's own BSDF table, and every refusal of the entry point -- all of them are decided on the host
before the device is touched, so a machine without a GPU reaches each one and gets GVPM_ERR_NO_DEVICE for a well-formed scene."""
import ctypes as C

import numpy as np
import pytest

import devgen_glossy_cases as DG
from gvpm_amd import abi, hip
from gvpm_amd.host import SynthScene

ALL = DG.SCENES + DG.MIXTURES + DG.ROTATED


def no_gpu():
    h = C.c_void_p()
    sc = SynthScene("cbox", 8, 8)
    d = sc.devgen_scene()
    rc = hip.lib().gvpm_devgen_create(C.byref(d), 0, C.byref(h))
    if rc == 0:
        hip.lib().gvpm_devgen_destroy(h)
    return rc == abi.GVPM_ERR_NO_DEVICE


def test_material_record_has_the_c_layout(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gvpm_hip.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(gvpm_devgen_material), offsetof(gvpm_devgen_material, rtrans),'
                   'offsetof(gvpm_devgen_material, bsdf), offsetof(gvpm_devgen_material, child),'
                   'offsetof(gvpm_devgen_material, reserved));return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    M = abi.DevgenMaterial
    assert got == [C.sizeof(M), M.rtrans.offset, M.bsdf.offset, M.child.offset, M.reserved.offset]


@pytest.mark.parametrize("name", ALL)
def test_materials_agree_with_the_table(name):
    sc = DG.scene(name, 8, 8)
    kinds, mats, table = DG.mat_kinds(sc), sc.devgen_materials(), sc.bsdfs()
    assert len(kinds) == len(mats) and max(kinds) > DG.MAT_MIRROR
    heads = set(int(i) for i in np.flatnonzero(abi.bsdf_heads(table)))
    seen, slots = set(), 0
    for i, (kind, m) in enumerate(zip(kinds, mats)):
        assert list(m.reserved) == [0, 0, 0]
        n = DG.bsdf_entries(kind, m.exponent)
        if n == 0:
            assert m.bsdf == -1 and kind <= DG.MAT_MIRROR
            continue
        stride = 1 + abi.bsdf_tail_entries(DG.BSDF_KIND[kind])
        for c in range(n):
            at = m.bsdf + c * stride
            assert at in heads and at not in seen, (name, i, at)
            assert int(table[at]["kind"]) == DG.BSDF_KIND[kind], (name, i, at)
            seen.add(at)
        slots += n * stride
        assert (m.rtrans is not None) == (kind == DG.MAT_ROUGHPLASTIC)
        if kind == DG.MAT_ROUGHPLASTIC:
            sl = np.array((C.c_float * abi.GVPM_RTRANS_KNOTS).from_address(m.rtrans))
            assert np.array_equal(sl, abi.rtrans_of(table, m.bsdf))
        if kind == DG.MAT_MIXTURE:
            children, weights, first = sc.mixture(i)
            assert list(m.child) == list(children) and list(m.mix_w) == list(weights) and first == m.bsdf
    # every head of the table belongs to exactly one material
    assert seen == heads and slots == table.size


@pytest.mark.parametrize("name", DG.SCENES + DG.MIXTURES + ["cbox_roughglass_rot"])
@pytest.mark.parametrize("beams", [0, 1])
def test_streaming_flattening_is_the_array_flattening_on_glossy_scenes(name, beams):
    """What the device walk stores (StreamPath, host/synth_core.h: the path flattened while it is walked) against flattenPath /
    flattenBeams over the whole path, bit for bit, host build: a plastic vertex is classified by the component it was sampled
    through, which the streaming form knows one vertex later than the closed set's kinds."""
    from gvpm_amd.host import lib
    sc = DG.scene(name, 32, 24)
    n = C.c_uint64(0)
    differ = lib().gvpm_synth_stream_check(sc._h, 2, 20000, beams, C.byref(n))
    assert differ == 0 and n.value > 5000


def test_min_depth_setter():
    """minDepth = 2: no photon and no beam is reconnected from the emitter; the scene struct and the parameters carry the value; the
    streaming flattening still is the array flattening; values outside [0, maxDepth) are refused"""
    from gvpm_amd.host import lib
    sc = DG.scene("cbox_conductor", 16, 12)
    ph0, _ = sc.shoot_photons(1, 3000)
    assert ((ph0.flags & 3) == abi.GVPM_PARENT_EMITTER).sum() > 100
    sc.set_min_depth(2)
    assert sc.devgen_scene().min_depth == 2 and sc.params().min_depth == 2
    ph, _ = sc.shoot_photons(1, 3000)
    bm, _, _ = sc.shoot_beams(1, 3000)
    for rec in (ph, bm):
        assert rec.n > 1000 and ((rec.flags & 3) != abi.GVPM_PARENT_EMITTER).all()
        assert (((rec.flags >> 8) & 0xFF) >= 2).all()
    for beams in (0, 1):
        n = C.c_uint64(0)
        assert lib().gvpm_synth_stream_check(sc._h, 2, 20000, beams, C.byref(n)) == 0 and n.value > 3000
    for bad in (-1, sc.devgen_scene().max_depth, 1000):
        with pytest.raises(ValueError):
            sc.set_min_depth(bad)
    sc.set_min_depth(0)
    again, _ = sc.shoot_photons(1, 3000)
    assert np.array_equal(again.flags, ph0.flags) and np.array_equal(again.pos, ph0.pos)


def test_a_rough_plastic_without_its_slice_fails_as_the_shoot_calls_do():
    sc = SynthScene("cbox_roughplastic", 8, 8)
    with pytest.raises(RuntimeError, match="transmittance slice"):
        sc.shoot_photons(1, 10)
    with pytest.raises(RuntimeError, match="transmittance slice"):
        sc.devgen_materials()


@pytest.mark.parametrize("name", ALL + ["cbox", "cbox_mirror"])
def test_a_well_formed_scene_reaches_the_device(name):
    rc, msg = DG.create_ex(DG.scene(name, 8, 8))
    assert rc == (abi.GVPM_ERR_NO_DEVICE if no_gpu() else 0), (rc, msg)


def test_the_plain_entry_point_still_refuses_glossy_kinds():
    sc = SynthScene("cbox_phong", 8, 8)
    d, h = sc.devgen_scene(), C.c_void_p()
    assert hip.lib().gvpm_devgen_create(C.byref(d), 0, C.byref(h)) == abi.GVPM_ERR_UNSUPPORTED
    assert b"gvpm_devgen_create_ex" in hip.lib().gvpm_devgen_last_error()
    with pytest.raises(hip.GvpmError) as e:
        hip.DeviceGenerator(sc)
    assert e.value.code == abi.GVPM_ERR_UNSUPPORTED


def first_of(sc, *kinds):
    return next(i for i, k in enumerate(DG.mat_kinds(sc)) if k in kinds)


def refusals():
    """[(what, scene, damage(sc, scene struct, materials, keep-alive list), status, a word of its text)]: one defect each"""
    R = []

    def add(what, scene, status, word):
        def deco(f):
            R.append((what, scene, f, status, word))
            return f
        return deco
    inv, uns = abi.GVPM_ERR_INVALID_ARG, abi.GVPM_ERR_UNSUPPORTED

    @add("unknown kind", "cbox_phong", inv, "kind")
    def _(sc, d, m, keep):
        kinds = (C.c_int32 * d.n_mats)(*DG.mat_kinds(sc))
        kinds[first_of(sc, DG.MAT_PHONG)] = 12
        keep.append(kinds)
        d.mat_kind = C.addressof(kinds)

    @add("negative kind", "cbox_phong", inv, "kind")
    def _(sc, d, m, keep):
        kinds = (C.c_int32 * d.n_mats)(*DG.mat_kinds(sc))
        kinds[0] = -1
        keep.append(kinds)
        d.mat_kind = C.addressof(kinds)

    for w in range(3):
        @add(f"reserved word {w}", "cbox_ward", inv, "reserved")
        def _(sc, d, m, keep, w=w):
            m[0].reserved[w] = 1

    @add("rough plastic without a slice", "cbox_roughplastic", inv, "slice is missing")
    def _(sc, d, m, keep):
        m[first_of(sc, DG.MAT_ROUGHPLASTIC)].rtrans = None

    for what, v in (("above one", 1.5), ("negative", -0.25), ("NaN", float("nan")), ("infinite", float("inf"))):
        @add(f"slice value {what}", "cbox_roughplastic_phong", inv, "slice values")
        def _(sc, d, m, keep, v=v):
            i = first_of(sc, DG.MAT_ROUGHPLASTIC)
            sl = (C.c_float * abi.GVPM_RTRANS_KNOTS).from_address(m[i].rtrans)
            bad = (C.c_float * abi.GVPM_RTRANS_KNOTS)(*sl)
            bad[abi.GVPM_RTRANS_KNOTS - 1] = v
            keep.append(bad)
            m[i].rtrans = C.addressof(bad)

    for scene, kind in (("cbox_ward_aniso", DG.MAT_WARD_ANISO), ("cbox_conductor_aniso", DG.MAT_ROUGHCONDUCTOR_ANISO)):
        @add("tangent not a unit vector", scene, inv, "unit vector")
        def _(sc, d, m, keep, kind=kind):
            t = m[first_of(sc, kind)].tangent
            for c in range(3):
                t[c] *= 1.01

        @add("zero tangent", scene, inv, "unit vector")
        def _(sc, d, m, keep, kind=kind):
            t = m[first_of(sc, kind)].tangent
            t[0] = t[1] = t[2] = 0.0

        @add("alphaU below 1e-4", scene, inv, "alphaU, alphaV")
        def _(sc, d, m, keep, kind=kind):
            m[first_of(sc, kind)].exponent = 5e-5

        @add("alphaV below 1e-4", scene, inv, "alphaU, alphaV")
        def _(sc, d, m, keep, kind=kind):
            m[first_of(sc, kind)].alpha_v = 0.0

    for c, v in ((0, -1), (1, 1000)):
        @add(f"mixture child {c} out of range", "cbox_mixture", inv, "child")
        def _(sc, d, m, keep, c=c, v=v):
            m[first_of(sc, DG.MAT_MIXTURE)].child[c] = v

    for what, w in (("sum to zero", (0.0, 0.0)), ("negative", (-0.5, 1.0)), ("NaN", (float("nan"), 0.5)), ("infinite", (0.5, float("inf")))):
        @add(f"mixture weights {what}", "cbox_mixture", inv, "weights")
        def _(sc, d, m, keep, w=w):
            i = first_of(sc, DG.MAT_MIXTURE)
            m[i].mix_w[0], m[i].mix_w[1] = w

    @add("bsdf below -1", "cbox_phong", inv, "bsdf")
    def _(sc, d, m, keep):
        m[first_of(sc, DG.MAT_PHONG)].bsdf = -2

    for scene, kind in (("cbox_conductor", DG.MAT_ROUGHCONDUCTOR), ("cbox_conductor_aniso", DG.MAT_ROUGHCONDUCTOR_ANISO),
                        ("cbox_roughplastic", DG.MAT_ROUGHPLASTIC), ("cbox_roughglass", DG.MAT_ROUGHDIELECTRIC)):
        for v in (2, 4, -1):
            @add(f"distribution {v}", scene, uns, "Beckmann, GGX or Phong")
            def _(sc, d, m, keep, kind=kind, v=v):
                m[first_of(sc, kind)].distribution = v

    @add("Ward variant 3", "cbox_ward", uns, "variant")
    def _(sc, d, m, keep):
        m[first_of(sc, DG.MAT_WARD)].distribution = 3

    @add("a mixture as a mixture's child", "cbox_mixture", uns, "Lambertian or a rough conductor")
    def _(sc, d, m, keep):
        i = first_of(sc, DG.MAT_MIXTURE)
        m[i].child[0] = i

    @add("a mirror-like child kind", "cbox_mixture1", uns, "Lambertian or a rough conductor")
    def _(sc, d, m, keep):
        # (the scene's index-matched boundary: a material that is neither Lambertian nor a conductor)
        m[first_of(sc, DG.MAT_MIXTURE)].child[1] = first_of(sc, DG.MAT_NULL)
    return R


REFUSALS = refusals()


@pytest.mark.parametrize("what,scene,damage,status,word", REFUSALS, ids=[f"{r[1]}-{r[0]}".replace(" ", "_") for r in REFUSALS])
def test_refusals(what, scene, damage, status, word):
    sc = DG.scene(scene, 8, 8)
    d, mats, keep = sc.devgen_scene(), sc.devgen_materials(), []
    damage(sc, d, mats, keep)
    rc, msg = DG.create_ex(sc, mats, d)
    assert rc == status, (what, rc, msg)
    assert word in msg, (what, msg)


def test_refusal_texts_are_distinct_and_argument_checks():
    texts = {}
    for what, scene, damage, status, word in REFUSALS:
        sc = DG.scene(scene, 8, 8)
        d, mats, keep = sc.devgen_scene(), sc.devgen_materials(), []
        damage(sc, d, mats, keep)
        texts.setdefault(DG.create_ex(sc, mats, d)[1], set()).add(word)
    # a text per rule: no text serves two different rules
    assert all(len(w) == 1 for w in texts.values()), texts
    assert len(texts) >= 13
    sc = DG.scene("cbox_phong", 8, 8)
    d, mats, h = sc.devgen_scene(), sc.devgen_materials(), C.c_void_p()
    L = hip.lib()
    assert L.gvpm_devgen_create_ex(C.byref(d), mats, len(mats) - 1, 0, C.byref(h)) == abi.GVPM_ERR_INVALID_ARG
    assert L.gvpm_devgen_create_ex(C.byref(d), None, len(mats), 0, C.byref(h)) == abi.GVPM_ERR_INVALID_ARG
    assert L.gvpm_devgen_create_ex(None, mats, len(mats), 0, C.byref(h)) == abi.GVPM_ERR_INVALID_ARG
    assert L.gvpm_devgen_create_ex(C.byref(d), mats, len(mats), 0, None) == abi.GVPM_ERR_INVALID_ARG
