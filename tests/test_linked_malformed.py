"""Malformed blobs of linked photon records (include/gvpm_hip.h "linked photon records"): what a blob means is DEFINED by
gvpm_unpack_photons_linked (pack_host.hip), and the device decoder (decode_device.hip) must reject exactly the blobs it rejects.  Here: the host
definition refuses hand-edited blobs -- a kind code of 3, per-64-photon group bases that are not the running counts, kinds
that disagree with the header's counts, a header whose layout only fits uint32 fields by wrapping, a truncated blob -- and a
sweep of single-bit flips over the kinds and groups words either raises or decodes as the independent numpy decoder does.
The same edits go to the device in test_decode_parity_gpu.py.  Plain host code: no GPU."""
import ctypes as C

import numpy as np
import pytest

import cases
from gvpm_amd import abi, hip
from test_packed_upload import linked_decode_numpy

N_MAX = 1 << 25  # the packer's limit (gvpm_pack_photons_linked)


def align16(x):
    return (x + 15) // 16 * 16


def layout(n, n_emitters, n_full, n_emit, n_chain):
    """the offsets {kinds, groups, emitters, full, emit, chain} and size of a blob, unbounded (Python ints)"""
    o = [64]
    o.append(align16(o[-1] + (n + 15) // 16 * 4))
    o.append(align16(o[-1] + (n + 63) // 64 * 8))
    o.append(align16(o[-1] + 32 * n_emitters))
    o.append(align16(o[-1] + 76 * n_full))
    o.append(align16(o[-1] + 48 * n_emit))
    o.append(align16(o[-1] + 40 * n_chain))
    return o


def blob_views(blob):
    """(header, kinds words, groups (ngroups, 2), kind of every photon) -- the words are views INTO blob"""
    hd = hip.linked_header(blob)
    n = hd["n"]
    kinds = blob[hd["off_kinds"]:hd["off_kinds"] + 4 * ((n + 15) // 16)].view(np.uint32)
    groups = blob[hd["off_groups"]:hd["off_groups"] + 8 * ((n + 63) // 64)].view(np.uint32).reshape(-1, 2)
    i = np.arange(n)
    kind = (kinds[i // 16] >> (2 * (i % 16)).astype(np.uint32)) & 3
    return hd, kinds, groups, kind


def set_kind(blob, i, k):
    _, kinds, _, _ = blob_views(blob)
    sh = 2 * (i % 16)
    kinds[i // 16] = (kinds[i // 16] & np.uint32(~(3 << sh) & 0xFFFFFFFF)) | np.uint32(k << sh)


def linked_case(n=1189):
    """a blob of n photons of real light paths (n: neither a multiple of 16 nor of 64) and its material table"""
    c = cases.make_case("cbox", 16, 12, 3000, 3.0)
    ph = c.ph.subset(np.arange(n))
    t = hip.MaterialTable()
    blob = hip.pack_photons_linked(ph, t).copy()
    return blob, t


def wrapped_header_blob():
    """A header of n = 2^26 photons (2^26 - nf chain records, nf full ones, one emitter) whose fields hold the layout's
    offsets mod 2^32 -- what a uint32 layout computes -- with nf chosen so that the wrapped size is a few hundred bytes:
    a layout check that wraps the same way accepts it, and a decoder then reads 2^26 photons out of that many bytes."""
    n = 1 << 26
    nf0 = (2 ** 32 - layout(n, 1, 0, 0, n)[-1]) // 36
    for nf in range(nf0, nf0 + 64):
        o = layout(n, 1, nf, 0, n - nf)
        if 256 <= o[-1] % 2 ** 32 <= 4096:
            break
    else:
        raise AssertionError("no wrapped layout in range")
    w = [o_ % 2 ** 32 for o_ in o]
    assert w[-1] < o[1]  # the blob ends before its kinds would
    hd = np.zeros(1, abi.LINKED_HEADER_DTYPE)
    for k, v in zip(("magic", "n", "n_full", "n_emit", "n_chain", "n_emitters"), (abi.GVPM_LINKED_MAGIC, n, nf, 0, n - nf, 1)):
        hd[k] = v
    for k, v in zip(("off_kinds", "off_groups", "off_emitters", "off_full", "off_emit", "off_chain", "bytes"), w):
        hd[k] = v
    blob = np.zeros(w[-1], np.uint8)
    blob[:64] = hd.view(np.uint8)
    return blob


def group_for_pm1(hd, groups, kind):
    """a group g (not the last) where a base off by +-1 still indexes inside the blob even for a decoder that trusts the
    bases: records of both kinds before it and behind the next group, chain records before it and behind it"""
    ng = groups.shape[0]
    chains_before = np.concatenate([[0], np.cumsum(kind == 2)])[np.arange(ng) * 64]
    for g in range(ng // 2, ng - 1):
        nx = groups[g + 1]
        if (groups[g] >= 1).all() and nx[0] < hd["n_full"] and nx[1] < hd["n_emit"] and chains_before[g] >= 1 and \
                chains_before[g + 1] < hd["n_chain"]:
            return g
    raise AssertionError("no group fit for the +-1 edits")


def malformed_blobs(blob):
    """{name: (blob, kind of defect)}: 'header' defects fail at upload, 'body' ones in the decode.  Every body edit keeps
    the record indices a decoder that trusts the bases would compute inside the blob's bytes (see the comments)."""
    hd, kinds, groups, kind = blob_views(blob)
    n, ng = hd["n"], groups.shape[0]
    out = {}
    # a kind 3 on what was a chain record: such a decoder reads an earlier chain record (its index collides with the next one's)
    b = blob.copy()
    i3 = int(np.nonzero(kind == 2)[0][len(np.nonzero(kind == 2)[0]) // 2])
    set_kind(b, i3, 3)
    out["kind3"] = (b, "body")
    # each group base off by one (see group_for_pm1)
    g = group_for_pm1(hd, groups, kind)
    for name, col, d in (("full_base+1", 0, 1), ("full_base-1", 0, -1), ("emit_base+1", 1, 1), ("emit_base-1", 1, -1)):
        b = blob.copy()
        gw = blob_views(b)[2]
        gw[g, col] = np.uint32(int(gw[g, col]) + d)
        out[name] = (b, "body")
    # a full base past the count, in the last group: its full records would be read from the emit records behind them, its
    # chain base stays >= 0
    b = blob.copy()
    gl = ng - 1
    assert 64 * gl - (hd["n_full"] + 5) - int(groups[gl, 1]) >= 0 and 48 * hd["n_emit"] > 76 * 70
    blob_views(b)[2][gl, 0] = hd["n_full"] + 5
    out["full_base_past_count"] = (b, "body")
    # the kinds hold one chain record fewer (one full record more) than the header's n_chain: the last chain photon of the
    # last group becomes full -- the full records behind it shift by one, the last onto the first emit record
    b = blob.copy()
    last_chain = int(np.nonzero(kind == 2)[0][-1])
    assert last_chain >= 64 * gl
    set_kind(b, last_chain, 0)
    out["n_chain_vs_kinds"] = (b, "body")
    out["n_2^26_wrapped"] = (wrapped_header_blob(), "header")
    out["truncated"] = (blob[:-16].copy(), "header")
    return out


def host_unpack(blob, table):
    """gvpm_unpack_photons_linked on the blob; GvpmError when it refuses.  A header beyond the packer's limit gets a
    one-photon destination (the definition must refuse it before writing a photon)."""
    n = hip.linked_header(blob)["n"] if blob.size >= 64 else 0
    if n <= N_MAX:
        return hip.unpack_photons_linked(blob, table)
    ph = abi.Photons(1)
    soa = ph.soa()
    soa.n = n
    rc = hip.lib().gvpm_unpack_photons_linked(blob.ctypes.data, blob.size, table.table.ctypes.data, table.n, C.byref(soa))
    if rc != 0:
        raise hip.GvpmError(rc, "gvpm_unpack_photons_linked failed")
    return ph


def test_the_edits_are_what_they_say():
    blob, t = linked_case()
    hd, kinds, groups, kind = blob_views(blob)
    assert hd["n"] % 16 and hd["n"] % 64 and hd["n_full"] and hd["n_emit"] and hd["n_chain"]
    host_unpack(blob, t)  # the unedited blob decodes
    bad = malformed_blobs(blob)
    assert len(bad) == 9
    _, _, _, k3 = blob_views(bad["kind3"][0])
    assert (k3 == 3).sum() == 1 and (kind == 2).sum() == (k3 == 2).sum() + 1
    _, _, _, kc = blob_views(bad["n_chain_vs_kinds"][0])
    assert (kc == 2).sum() == hd["n_chain"] - 1 and (kc == 0).sum() == hd["n_full"] + 1
    w = hip.linked_header(bad["n_2^26_wrapped"][0])
    assert w["n"] == 1 << 26 and w["bytes"] == bad["n_2^26_wrapped"][0].size < w["off_groups"]
    assert w["n_full"] + w["n_emit"] + w["n_chain"] == w["n"]


@pytest.mark.parametrize("name", ["kind3", "full_base+1", "full_base-1", "emit_base+1", "emit_base-1", "full_base_past_count",
                                  "n_chain_vs_kinds", "n_2^26_wrapped", "truncated"])
def test_host_definition_refuses_malformed_blobs(name):
    blob, t = linked_case()
    b, _ = malformed_blobs(blob)[name]
    with pytest.raises(hip.GvpmError):
        host_unpack(b, t)


def test_single_bit_flips_of_kinds_and_groups():
    """every flip either makes the host refuse the blob -- exactly when the independent numpy decoder finds its kinds or
    bases inconsistent -- or leaves a blob that decodes bit for bit as the numpy decoder says (padding bits of the last
    kinds word)"""
    blob, t = linked_case()
    hd, kinds, groups, kind = blob_views(blob)
    n = hd["n"]
    kbits, gbits = 32 * kinds.size, 64 * groups.shape[0]
    rng = np.random.default_rng(20261015)
    flips = set(rng.choice(kbits + gbits, 400, replace=False).tolist())
    flips |= set(range(2 * n, kbits))  # every padding bit of the last kinds word
    accepted = 0
    for f in sorted(flips):
        b = blob.copy()
        _, kw, gw, _ = blob_views(b)
        if f < kbits:
            kw[f // 32] ^= np.uint32(1 << (f % 32))
        else:
            f -= kbits
            gw.reshape(-1)[f // 32] ^= np.uint32(1 << (f % 32))
        try:
            want, _ = linked_decode_numpy(b, t)
        except (AssertionError, IndexError):
            want = None
        try:
            got = hip.unpack_photons_linked(b, t)
        except hip.GvpmError:
            got = None
        assert (got is None) == (want is None), f"bit {f}: host {'refused' if got is None else 'accepted'}"
        if got is not None:
            accepted += 1
            for k in abi.PHOTON_VEC3 + abi.PHOTON_F1 + abi.PHOTON_U1:
                assert np.array_equal(getattr(got, k).view(np.uint32), getattr(want, k).view(np.uint32)), (f, k)
    assert accepted == kbits - 2 * n  # only the padding bits leave a valid blob
