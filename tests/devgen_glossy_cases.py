"""Builders for the tests of the device generators over glossy scenes (gvpm_devgen_create_ex): the project's glossy scenes with
their transmittance slices set from tests/golden/ (through the existing helpers), the material kinds of host/synth_core.h, and
ctypes copies of a scene's materials that a test may damage."""
import ctypes as C
import math

import numpy as np

import phong_dist_cases as PD
import plastic_cases as PC
from gvpm_amd import abi, hip

(MAT_LAMBERT, MAT_NULL, MAT_MIRROR, MAT_PHONG, MAT_ROUGHCONDUCTOR, MAT_WARD, MAT_ROUGHPLASTIC, MAT_PLASTIC, MAT_WARD_ANISO,
 MAT_ROUGHCONDUCTOR_ANISO, MAT_ROUGHDIELECTRIC, MAT_MIXTURE) = range(12)
BSDF_KIND = {MAT_PHONG: abi.GVPM_BSDF_PHONG, MAT_ROUGHCONDUCTOR: abi.GVPM_BSDF_ROUGHCONDUCTOR, MAT_WARD: abi.GVPM_BSDF_WARD,
             MAT_ROUGHPLASTIC: abi.GVPM_BSDF_ROUGHPLASTIC, MAT_PLASTIC: abi.GVPM_BSDF_PLASTIC, MAT_WARD_ANISO: abi.GVPM_BSDF_WARD_ANISO,
             MAT_ROUGHCONDUCTOR_ANISO: abi.GVPM_BSDF_ROUGHCONDUCTOR_ANISO, MAT_ROUGHDIELECTRIC: abi.GVPM_BSDF_ROUGHDIELECTRIC,
             MAT_MIXTURE: abi.GVPM_BSDF_MIXTURE}

# the sixteen glossy scenes, by family
FAMILIES = dict(phong=["cbox_phong", "cbox_phong1", "cbox_phong_hg"],
                ward=["cbox_ward", "cbox_ward_duer", "cbox_ward_aniso"],
                conductor=["cbox_conductor", "cbox_conductor_phong", "cbox_conductor_aniso"],
                plastic=["cbox_roughplastic", "cbox_roughplastic1", "cbox_roughplastic_phong", "cbox_plastic"],
                glass=["cbox_roughglass", "cbox_roughglass_ggx", "cbox_roughglass_phong"])
SCENES = [s for f in FAMILIES.values() for s in f]
MIXTURES = ["cbox_mixture", "cbox_mixture1"]
# the scene in general position: one per family, and a mixture
ROTATED = ["cbox_phong_rot", "cbox_ward_aniso_rot", "cbox_conductor_rot", "cbox_roughplastic_rot", "cbox_roughglass_rot", "cbox_mixture_rot"]


def scene(name, W, H):
    """SynthScene with the fixtures' slices set where the scene has rough-plastic walls"""
    from gvpm_amd.host import SynthScene
    sc = SynthScene(name, W, H)
    for mat, dist, alpha, eta in sc.rtrans_materials():
        sl, fdr = PD.rtrans(round(eta, 4), round(alpha, 4)) if dist == "phong" else PC.rtrans(dist, round(eta, 4), round(alpha, 4))
        sc.set_rtrans(mat, sl, fdr)
    return sc


def mat_kinds(sc):
    d = sc.devgen_scene()
    return [int(k) for k in (C.c_int32 * d.n_mats).from_address(d.mat_kind)]


def bsdf_entries(kind, exponent):
    """bsdfEntries (host/synth_core.h): the heads a material of `kind` has in the table"""
    if kind in (MAT_ROUGHPLASTIC, MAT_MIXTURE):
        return 2 if exponent < 0.05 else 1
    if kind == MAT_ROUGHDIELECTRIC:
        return 2
    if kind == MAT_PHONG:
        return 2 if math.sqrt(2.0 / (2.0 + exponent)) < 0.05 else 1
    return 1 if kind in BSDF_KIND else 0


def create_ex(sc, mats=None, scene_struct=None):
    """gvpm_devgen_create_ex on device 0 -> (status, last-error text); a generator that came to life is destroyed"""
    d = sc.devgen_scene() if scene_struct is None else scene_struct
    mats = sc.devgen_materials() if mats is None else mats
    h = C.c_void_p()
    rc = hip.lib().gvpm_devgen_create_ex(C.byref(d), mats, len(mats), 0, C.byref(h))
    msg = hip.lib().gvpm_devgen_last_error().decode()
    if rc == 0:
        hip.lib().gvpm_devgen_destroy(h)
    return rc, msg


def min_depth_without_emitter(rays):
    """The smallest gvpm_params.min_depth that removes the photons reconnected from the emitter: the G-BRE gather keeps a photon for
    a camera beam where depth + edge >= min_depth (shift_volume_photon.cpp:670-673); such a photon has depth 1 (the path's second
    edge), every other one depth >= 2, and the scenes' camera beams all sit on one edge of their paths."""
    edges = set(((rays["info"][:, 0] >> 8) & 0xFF).tolist())
    assert len(edges) == 1, edges
    return 2 + edges.pop()


def taken(rec, p, edge=None):
    """which of the photon or beam records `rec` the gather under params `p` takes: photonContributes' parent-type rule for
    lighting_interaction_mode (csrc/shift_device.h) and, where `edge` is given (G-BRE: the camera beams' edge), the depth window
    depth + edge >= min_depth"""
    pt = rec.flags & 3
    depth = ((rec.flags >> 8) & 0xFF).astype(np.int64)
    mode = p.lighting_interaction_mode
    keep = np.ones(rec.n, bool)
    if not (mode & abi.GVPM_SURF2MEDIA and mode & abi.GVPM_MEDIA2MEDIA):
        medium = pt == abi.GVPM_PARENT_MEDIUM
        keep &= np.where(medium, bool(mode & abi.GVPM_MEDIA2MEDIA), bool(mode & abi.GVPM_SURF2MEDIA))
    if edge is not None and p.min_depth != 0:
        keep &= depth + edge >= p.min_depth
    return keep


def table_parent_share(rec, p, edge=None):
    """(share, kept): of the records the gather takes (taken), the share whose parent is a table entry, and how many are taken"""
    keep = taken(rec, p, edge)
    pt = rec.flags & 3
    return (float((pt[keep] == abi.GVPM_PARENT_SURFACE_BSDF).mean()) if keep.any() else 0.0), int(keep.sum())
