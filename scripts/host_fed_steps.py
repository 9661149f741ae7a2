#!/usr/bin/env python3
"""ms per step of C1 (G-VPM), C3 (G-Beams 3D) and C5 (G-Planes) FED FROM HOST MEMORY, the way a Mitsuba host feeds them:

  plain     today's synchronous calls from pageable memory (gvpm_upload_photons / _beams / _planes / _camera_beams /
            _vpm_samples, then gvpm_gather);
  prefetch  the SoA arrays from pinned memory, step N + 1 handed over (gvpm_prefetch_*) before gather N;
  packed    the same loop with the packed forms: linked beam records + octahedral end normals (C3), linked records + fp32
            second edges (C5), run-packed samples (C1); camera-beam sets as packed records;
  device    inputs already in device memory (what bench.py's line for the workload times): the floor the others approach.

Every (workload, mode) runs in a fresh child process under its own `timeout`; the parent prints one JSON line per run and a
table.  Also reported: bytes a step over PCIe, and the bytes per beam and the chain / emit / full shares of the linked packer
on the workload's beam records.  `--modes plain` runs on a library without the prefetch entry points too.

  python scripts/host_fed_steps.py [--workloads c1,c3,c5] [--modes plain,prefetch,packed,device] [--steps K] [--warmup W]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# BASELINE.json's configs at their stated sizes (bench.py: WORKLOADS); steps per timed run
WORKLOADS = {
    "c1": dict(scene="cbox", frame=256, records=100000, technique="vpm", samples=40, scale=2.0, steps=24),
    "c3": dict(scene="laser", frame=512, records=2000000, technique="beams3d", scale=1.0, steps=8),
    "c5": dict(scene="laser_in", frame=256, records=50000, technique="planes0d", scale=1.0, steps=12),
}
MODES = ("plain", "prefetch", "packed", "device")
DISTINCT = 3   # input sets cycled through (a prefetched set must not be the one in flight or the current one)


def child(args):
    from gvpm_amd import abi, hip
    from gvpm_amd.host import SynthScene
    wl = WORKLOADS[args.one]
    mode, tech = args.mode, wl["technique"]
    if mode == "device":
        # (the device-resident inputs live in torch tensors, as in bench.py: torch opens the device before the library does)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("the device mode needs a GPU")
        torch.cuda.set_device(0)
    W = H = args.frame or wl["frame"]
    nrec = args.records or wl["records"]
    sc = SynthScene(wl["scene"], W, H)
    p = sc.params()
    p.initial_scale_volume = wl["scale"]
    if tech == "vpm":
        p.vol_technique, p.nb_camera_samples = abi.GVPM_DISTANCE, wl["samples"]
    elif tech == "beams3d":
        p.vol_technique = abi.GVPM_BEAM_BEAM_3D_OPTIMIZED
    else:
        p.vol_technique, p.use_shift_null, p.min_depth = abi.GVPM_VOL_PLANE0D, 0, 2
    ctx = hip.Context(p, device=0)
    ctx.upload_scene(*sc.triangles())
    ctx.upload_medium(sc.medium())
    table = hip.MaterialTable()
    sets, keep = [], []
    for i in range(DISTINCT):
        it, s = i + 1, {}
        if tech == "vpm":
            s["ph"], s["nb"] = sc.shoot_photons(it, nrec)
            s["rays"], s["smp"] = sc.camera_beams_and_vpm_samples(it, wl["samples"])
        elif tech == "beams3d":
            s["ph"], s["en"], s["nb"] = sc.shoot_beams(it, nrec)
            s["rays"] = sc.camera_beams(it)
        else:
            s["ph"], _, s["w1"], s["l1"], s["nb"] = sc.shoot_planes(it, nrec)
            s["rays"] = sc.camera_beams(it)
        sets.append(s)
    soa_bytes = lambda s: s["ph"].n * 120 + s["rays"].nbytes + (s["smp"].nbytes if tech == "vpm" else
                                                               s["ph"].n * (12 if tech == "beams3d" else 16))
    info = {"records": int(np.mean([s["ph"].n for s in sets])), "sets": int(np.mean([s["rays"].shape[0] for s in sets]))}
    if tech != "vpm" and mode in ("packed", "plain"):
        # the linked packer on beam records: bytes a beam and the shares of the three kinds
        blob = hip.pack_photons_linked(sets[0]["ph"], hip.MaterialTable())
        hd, n = hip.linked_header(blob), max(sets[0]["ph"].n, 1)
        info["linked"] = {"bytes_per_beam": blob.size / n, "chain": hd["n_chain"] / n, "emit": hd["n_emit"] / n, "full": hd["n_full"] / n}
    if mode == "plain":
        info["bytes_per_step"] = int(np.mean([soa_bytes(s) for s in sets]))

        def feed(s, prefetch):
            assert not prefetch
            if tech == "vpm":
                ctx.upload_photons(s["ph"])
            elif tech == "beams3d":
                ctx.upload_beams(s["ph"], s["en"])
            else:
                ctx.upload_planes(s["ph"], s["w1"], s["l1"])
            ctx.upload_camera_beams(s["rays"])
            if tech == "vpm":
                ctx.upload_vpm_samples(s["smp"])
    elif mode == "device":
        import torch
        info["bytes_per_step"] = 0

        def dev(a):
            t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).cuda()
            keep.append(t)
            return t.data_ptr()
        for s in sets:
            soa = abi.PhotonSoA()
            for k in abi.PHOTON_VEC3 + abi.PHOTON_F1 + abi.PHOTON_U1:
                setattr(soa, k, dev(getattr(s["ph"], k)))
            soa.n = s["ph"].n
            s["soa"], s["drays"] = soa, dev(s["rays"].view(np.uint8).reshape(-1))
            for k in ("en", "w1", "l1"):
                if k in s:
                    s["d" + k] = dev(np.ascontiguousarray(s[k], np.float32))
            if tech == "vpm":
                s["dsmp"] = dev(s["smp"].view(np.uint8).reshape(-1))
        torch.cuda.synchronize()

        def feed(s, prefetch):
            assert not prefetch
            if tech == "vpm":
                ctx.upload_photons_dev(s["soa"])
            elif tech == "beams3d":
                ctx.upload_beams_dev(s["soa"], s["den"])
            else:
                ctx.upload_planes_dev(s["soa"], s["dw1"], s["dl1"])
            ctx.upload_camera_beams_dev(s["drays"], s["rays"].shape[0])
            if tech == "vpm":
                ctx.upload_vpm_samples_dev(s["dsmp"], s["smp"].size)
    else:
        packed = mode == "packed"
        if packed and tech != "vpm":
            for s in sets:   # (every set's materials first: the table is complete before the first upload)
                hip.pack_photons_linked(s["ph"], table)
            ctx.upload_materials(table)
        nbytes = []
        for s in sets:
            if tech == "vpm":
                s["pin_ph"] = hip.PinnedPhotons(s["ph"].n).fill(s["ph"])
                s["pin_smp"] = hip.PinnedSamples(s["smp"])
                side = s["pin_smp"].packed_nbytes if packed else s["pin_smp"].nbytes
                photons = s["ph"].n * 120
            else:
                s["pin"] = hip.PinnedBeams(s["ph"], end_n=s.get("en"), w1=s.get("w1"), len1=s.get("l1"), table=table if packed else None)
                side, photons = 0, (s["pin"].packed_nbytes if packed else s["pin"].nbytes)
            if packed:
                s["pin_rays"] = hip.PinnedArray(hip.pack_camera_beams(s["rays"]))
            else:
                s["pin_rays"] = hip.PinnedRays(s["rays"])
            nbytes.append(photons + side + (s["pin_rays"].nbytes if packed else s["rays"].nbytes))
        info["bytes_per_step"] = int(np.mean(nbytes))
        L, h = hip.lib(), ctx._h

        def feed(s, prefetch):
            if tech == "vpm":
                # (the G-VPM photon map is a plain photon upload: pinned SoA in both modes)
                ctx.prefetch(photons=s["pin_ph"]) if prefetch else ctx.upload_pinned(photons=s["pin_ph"])
                ctx.upload_pinned_vpm_samples(s["pin_smp"], prefetch=prefetch, packed=packed)
            else:
                ctx.upload_pinned_beams(s["pin"], prefetch=prefetch, packed=packed)
            n = s["rays"].shape[0]
            if packed:
                f = L.gvpm_prefetch_camera_beams_packed if prefetch else L.gvpm_upload_camera_beams_packed
                ctx._check(f(h, s["pin_rays"].ptr, n))
            else:
                ctx.prefetch(rays=s["pin_rays"]) if prefetch else ctx.upload_pinned(rays=s["pin_rays"])

    pipelined = mode in ("prefetch", "packed")

    def run(first_it, count):
        if pipelined:
            feed(sets[(first_it - 1) % DISTINCT], False)
        for it in range(first_it, first_it + count):
            s = sets[(it - 1) % DISTINCT]
            if pipelined:
                if it + 1 < first_it + count:
                    feed(sets[it % DISTINCT], True)
            else:
                feed(s, False)
            ctx.gather(it, s["nb"])
        ctx.synchronize()

    run(1, args.warmup)
    ctx.reset()
    ctx.synchronize()
    t0 = time.perf_counter()
    run(1, args.steps)
    elapsed = time.perf_counter() - t0
    st = ctx.stats()
    ctx.close()
    info.update(workload=args.one, mode=mode, ms_per_step=1e3 * elapsed / args.steps, steps=args.steps, warmup=args.warmup,
                evaluations=st["evaluations"], frame=W)
    print("HOST_FED " + json.dumps(info), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="c1,c3,c5")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--steps", type=int, default=0, help="timed steps (0: the workload's)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frame", type=int, default=0, help="frame side (0: the workload's stated size)")
    ap.add_argument("--records", type=int, default=0, help="map records (0: the workload's stated size)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds a single (workload, mode) run may take")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    ap.add_argument("--mode", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        args.steps = args.steps or WORKLOADS[args.one]["steps"]
        return child(args)
    rows = []
    for w in args.workloads.split(","):
        for mode in args.modes.split(","):
            assert w in WORKLOADS and mode in MODES, (w, mode)
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", w, "--mode", mode,
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--frame", str(args.frame), "--records", str(args.records)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = [x for x in r.stdout.splitlines() if x.startswith("HOST_FED ")]
            if r.returncode != 0 or not line:
                # nothing more on this GPU after a run that faulted, aborted or ran into its limit
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                raise SystemExit(f"{w} {mode}: exit {r.returncode}")
            rows.append(json.loads(line[0][9:]))
            print(json.dumps(rows[-1]), flush=True)
    print("\n| workload | mode | ms / step | MB / step | evaluations |\n|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['workload']} | {r['mode']} | {r['ms_per_step']:.3f} | {r['bytes_per_step'] / 1e6:.2f} | {r['evaluations']} |")
    for r in rows:
        if "linked" in r and r["mode"] in ("packed", "plain"):
            k = r["linked"]
            print(f"{r['workload']}: linked beam records {k['bytes_per_beam']:.1f} B a beam "
                  f"(chain {k['chain']:.1%}, emit {k['emit']:.1%}, full {k['full']:.1%})")


if __name__ == "__main__":
    main()
