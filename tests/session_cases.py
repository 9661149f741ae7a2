"""Scripted sessions: a seeded list of steps on ONE handle, driven on the device and folded through the fp64 oracle.

The parity suites check one gather on a fresh handle; what a handle carries from one gather to the next (DESIGN section 5,
last paragraph: the rotating build sets, the cached bounds, the near grid's reach, the staging rings, G-VPM's clean buffers and scale
bound, the running sum, the deferred exact shifts) is checked here.  A Step names what changes before its gather; materialise()
turns a Session into the arrays of every step (what the device is fed and what the oracle is fed are the SAME arrays: for the
lossy upload formats the host unpackers' output, which defines what a blob means); fold() runs the oracle over them
(accum=ref, scale_vol / n_vol for G-VPM) and mirrors the radius schedule; run_device() drives the handle in one of two modes:

  observed  after every step stats(), download_accum(), download_film() (and download_vpm_state()) are read and compared:
            counter increments == the oracle's step counters, sums and film within the technique's driver bar; a failure
            names its step (first_failure).
  blind     nothing is read before the last step, so the deferred shifts, the flush pacing and the pipelines run undisturbed.

Bars are the drivers' own: G-BRE / G-VPM 1e-4 (test_parity_gpu.TOL), G-Beams 2e-4, G-Planes 1e-5, device against device 1e-6,
exact-pass sessions 2e-6 (glossy tables 2e-5, beams 5e-5).  A session that cannot meet its bar is softened, never the bar
(the rule of medium_cases.py); tests/test_sessions.py admits every session by the fp32 oracle.

Admission, fp32 oracle against fp64 oracle on this file's sessions (CPU): see the table in tests/test_sessions.py's docstring.
"""
import copy
import os
from dataclasses import dataclass, field

import numpy as np

import cases
import medium_cases
import oracle_lib as O
from gvpm_amd import abi, hip
from gvpm_amd.host import SynthScene
from test_parity_gpu import TOL


DEVICE_BAR = 1e-6            # device against device: test_optimistic_step_..., test_vpm_kernel_paths_agree
COUNTERS = ("evaluations", "null_shifts", "diffuse_shifts", "failed_shifts")
TECH = {
    "bre3d": abi.GVPM_VOL_BRE3D, "bre2d": abi.GVPM_VOL_BRE2D, "vpm": abi.GVPM_DISTANCE,
    "beams3d": abi.GVPM_BEAM_BEAM_3D_OPTIMIZED, "beams1d": abi.GVPM_BEAM_BEAM_1D, "planes": abi.GVPM_VOL_PLANE0D,
}
BAR = {"bre3d": TOL, "bre2d": TOL, "vpm": TOL, "beams3d": 2e-4, "beams1d": 2e-4, "planes": 1e-5}
EXACT_BAR = {"bre3d": 2e-6, "vpm": 2e-6, "beams3d": 5e-5, "glossy": 2e-5}   # test_exact_pass_gpu.py
PATHS = ("soa", "pinned", "prefetch", "packed", "linked", "compact", "dev")


def l2(a, ref, lum):
    return float(np.sqrt(((np.asarray(a, np.float64) - ref) ** 2).mean()) / max(lum, 1e-30))


@dataclass
class Step:
    it: int
    n: object = None          # records uploaded (photons, beams or planes), 0 and 1 included; None: the previous step's stay
    rays: object = "all"      # "all" | "37" (a random 37) | "none" | a fraction of the frame's rows, from the top | "keep"
    moved: bool = False       # the frame's rays leave another origin
    box: str = None           # "centre" | "corner": only the records whose end lies in that box
    scene: str = None         # upload this scene's occluders (and shoot from it from here on)
    medium: str = None        # "grey" (the scene's own) or a name of medium_cases.MEDIA
    table: str = None         # a key of Session.tables
    scale: float = None       # set_global_scale before the gather
    reset: bool = False       # gvpm_reset before anything else of the step
    path: str = "soa"         # one of PATHS (photon techniques)
    again: bool = False       # gather again without uploading anything


@dataclass
class Session:
    name: str
    tech: str
    scene: str
    W: int
    H: int
    N: int                    # the nominal record count (what "N" means in the steps' comments)
    scale: float
    steps: list
    params: dict = field(default_factory=dict)
    nb: int = 6               # G-VPM: camera samples per pixel
    tables: dict = field(default_factory=dict)   # name -> (table, refused: bool, the table the oracle evaluates it as)
    env: dict = field(default_factory=dict)      # set only around hip.Context(...)
    bar: float = None
    seed: int = 11
    first_gen: int = 1        # the generators' iteration number of the first step (softening: another draw of every input)

    def __post_init__(self):
        if self.bar is None:
            self.bar = BAR[self.tech]


class Resolved:
    """one step's arrays: what is uploaded (when `upload_*` says so) and what the oracle is fed"""


# ---- materialise ------------------------------------------------------------------------------------------------------------------
def _scene_case(s, scene):
    kw = dict(s.params)
    kw["vol_technique"] = TECH[s.tech]
    if s.tech == "vpm":
        kw["nb_camera_samples"] = s.nb
    if s.tech in ("beams1d", "bre2d", "planes"):
        kw.setdefault("use_shift_null", 0)
    if s.tech == "planes":
        kw.setdefault("min_depth", 2)
    return cases.make_case(scene, s.W, s.H, 10, s.scale, **kw)


def _box(pos, which):
    q = np.quantile(pos, [0.25, 0.6, 0.75], axis=0) if pos.shape[0] else np.zeros((3, 3))
    if which == "centre":
        return np.nonzero(((pos > q[0]) & (pos < q[2])).all(1))[0]
    return np.nonzero((pos > q[1]).all(1))[0]


def _select_rays(rays, how, H, rng):
    if how == "all":
        return np.arange(rays.shape[0])
    if how == "none":
        return np.zeros(0, np.int64)
    if how == "37":
        return np.sort(rng.permutation(rays.shape[0])[:37])
    return np.nonzero(cases.pixels_of(rays)[1] < int(H * float(how)))[0]


def materialise(s):
    """Session -> [Resolved]: every step's inputs and the mirrored radius, from the session's seed alone"""
    rng = np.random.default_rng(s.seed)
    scenes = {s.scene: _scene_case(s, s.scene)}
    cur = scenes[s.scene]
    p = cur.p
    tech = TECH[s.tech]
    mtable = hip.MaterialTable()
    out, prev = [], None
    medium, medium_name = cur.sc.medium(), "grey"
    table = otable = cur.sc.bsdfs()
    scale = np.float32(p.initial_scale_volume)
    for k, st in enumerate(s.steps):
        g = k + s.first_gen                          # the generators' iteration number: every step its own inputs
        r = Resolved()
        r.step, r.k, r.it, r.reset, r.path, r.moved = st, k, st.it, st.reset, st.path, st.moved
        r.upload_scene = r.upload_medium = r.upload_table = False
        r.refused_table = None
        if st.reset:
            scale = np.float32(p.initial_scale_volume)
        if st.scene is not None:
            if st.scene not in scenes:
                scenes[st.scene] = _scene_case(s, st.scene)
            cur = scenes[st.scene]
            r.upload_scene = True
        if st.medium is not None:
            holder = cases.Case()
            holder.m = cur.sc.medium()
            medium = holder.m if st.medium == "grey" else medium_cases.apply(holder, st.medium).m
            medium_name = st.medium
            r.upload_medium = True
        if st.table is not None:
            t, refused, as_oracle = s.tables[st.table]
            if refused:
                r.refused_table = t
            else:
                table, otable = t, as_oracle
                r.upload_table = True
        r.tris, r.m, r.medium_name, r.table, r.otable = cur.tris, medium, medium_name, table, otable
        r.scene = cur.sc.name
        r.set_scale = st.scale
        if st.scale is not None:
            scale = np.float32(st.scale)
        again = st.again or (st.n is None and st.rays == "keep")
        r.upload_records = (not again) and st.n is not None
        r.upload_rays = (not again) and st.rays != "keep"
        # records
        if r.upload_records:
            n = int(st.n)
            cap = max(n, 64)
            if s.tech in ("bre3d", "bre2d", "vpm"):
                rec, nb = cur.sc.shoot_photons(g, cap)
                extra = {}
            elif s.tech in ("beams3d", "beams1d"):
                rec, end_n, nb = cur.sc.shoot_beams(g, cap)
                extra = {"end_n": end_n}
            else:
                rec, end_n, w1, len1, nb = cur.sc.shoot_planes(g, cap)
                extra = {"w1": w1, "len1": len1}
            idx = np.arange(rec.n) if st.box is None else _box(rec.pos, st.box)
            idx = idx[:n]
            rec = rec.subset(idx)
            extra = {a: np.ascontiguousarray(v[idx]) for a, v in extra.items()}
            r.blob = r.pk = None
            if st.path == "packed":
                r.pk = hip.pack_photons(rec, mtable)
                rec = hip.unpack_photons(r.pk, mtable)
            elif st.path == "linked" and rec.n:
                r.blob = hip.pack_photons_linked(rec, mtable).copy()
                rec = hip.unpack_photons_linked(r.blob, mtable)
            r.rec, r.extra, r.nb = rec, extra, max(int(nb), 1)
        else:
            r.rec, r.extra, r.nb, r.blob, r.pk = prev.rec, prev.extra, prev.nb, None, None
        # camera beams (and G-VPM's samples, which name their set by index)
        if r.upload_rays:
            if s.tech == "vpm":
                rays, smp = cur.sc.camera_beams_and_vpm_samples(g, s.nb)
            else:
                rays, smp = cur.sc.camera_beams(g), None
            sel = _select_rays(rays, st.rays, s.H, rng)
            if smp is not None:
                new = np.full(rays.shape[0], -1, np.int64)
                new[sel] = np.arange(sel.size)
                smp = smp[new[smp["set"]] >= 0].copy()
                smp["set"] = new[smp["set"]]
            rays = np.ascontiguousarray(rays[sel])
            if st.moved:
                rays["o"] += np.float32(0.01)
            r.rp = r.comp = r.full = None
            if st.path == "packed":
                r.rp = hip.pack_camera_beams(rays)
                rays = hip.unpack_camera_beams(r.rp)
            elif st.path == "compact":
                sensor = cur.sc.sensor()
                r.comp, r.full, _ = hip.pack_camera_beams_compact(sensor, rays, cur.sc.jitter(g, rays))
                r.comp, r.full, r.sensor = r.comp.copy(), r.full.copy(), sensor
                rays = np.concatenate([hip.unpack_camera_beams_compact(sensor, r.comp), hip.unpack_camera_beams(r.full)])
            r.rays, r.samples = rays, smp
        else:
            r.rays, r.samples, r.rp, r.comp, r.full = prev.rays, prev.samples, None, None, None
        r.radius = cases.radius_of(p, scale)
        if s.tech != "vpm":                          # (G-VPM's radii are its per-pixel scales: the global one never moves)
            scale = np.float32(O.scale_volume_apa(float(scale), st.it, float(p.alpha), tech))
        out.append(r)
        prev = r
    for r in out:
        r.p, r.mtable = p, mtable
    return out


# ---- the oracle's fold -------------------------------------------------------------------------------------------------------------
class Folded:
    """the oracle's state after one step: the folded accumulators, this step's counters, G-VPM's state, the film"""


def oracle_step(s, r, precision, accum=None, sv=None, nv=None, radius=None, it=None):
    """one step through the oracle -> (accum, counters, scale_vol, n_vol)"""
    O.set_bsdfs(r.otable)
    radius = r.radius if radius is None else radius
    it = r.it if it is None else it
    if s.tech in ("bre3d", "bre2d"):
        a, cnt, _ = O.gather_bre(r.p, r.m, r.tris, r.rec, r.rays, radius, it, r.nb, precision, use_accel=False, accum=accum)
        return a, cnt, None, None
    if s.tech == "vpm":
        a, sv, nv, cnt, _ = O.gather_vpm(r.p, r.m, r.tris, r.rec, r.rays, r.samples, precision, use_accel=False, accum=accum,
                                         scale_vol=sv, n_vol=nv)
        return a, cnt, sv, nv
    if s.tech in ("beams3d", "beams1d"):
        a, cnt, _ = O.gather_beams(r.p, r.m, r.tris, r.rec, r.extra["end_n"], r.rays, radius, it, r.nb, precision, accum=accum)
        return a, cnt, None, None
    a, cnt, _ = O.gather_planes(r.p, r.m, r.tris, r.rec, r.extra["w1"], r.extra["len1"], r.rays, it, r.nb, precision, accum=accum)
    return a, cnt, None, None


def fold(s, res, precision=64, tamper=None):
    """the oracle over the session -> [Folded].  tamper = (kind, k): an oracle fold that is wrong at step k the way stale state
    would make the device wrong (APA techniques; test_sessions.py): "radius" the previous step's radius, "twice" the step's
    contribution added twice, "dropped" not at all, "rescale" the running sum not rescaled although `it` jumped; ("python",
    "every"): nothing wrong, every step folded by the statement the tampered steps use (its own check)."""
    out = []
    ref = sv = nv = None
    emitted, last_it = 0, 0
    for r in res:
        if r.reset:
            ref = sv = nv = None
            emitted, last_it = 0, 0
        kind = tamper[0] if tamper is not None and tamper[1] in (r.k, "every") else None
        if kind is None:
            ref, cnt, sv, nv = oracle_step(s, r, precision, ref, sv, nv)
        else:
            assert s.tech != "vpm"
            radius = res[r.k - 1].radius if kind == "radius" else r.radius
            assert kind in ("radius", "twice", "dropped", "rescale", "python"), kind
            v, cnt, _, _ = oracle_step(s, r, precision, None, radius=radius, it=1)   # it = 1: the step's own estimate
            old = np.zeros_like(v) if ref is None else ref
            w = {"twice": 2.0, "dropped": 0.0}.get(kind, 1.0)
            cnt = {c: int(w * n) for c, n in cnt.items()}
            weight = last_it if kind == "rescale" else r.it - 1                      # (mean * (it - 1) + v) / it
            ref = (old * weight + w * v) / r.it
        emitted += r.nb
        last_it = r.it
        f = Folded()
        f.acc, f.cnt, f.it, f.emitted = ref.copy(), cnt, r.it, emitted
        f.sv, f.nv = (None, None) if sv is None else (sv.copy(), nv.copy())
        f.lum = float(ref[..., 0:3].mean())
        f.film = O.assemble(ref, r.it, True, total_emitted=emitted if s.tech == "vpm" else 0.0)
        out.append(f)
    return out


# ---- the comparator (no device in it) -----------------------------------------------------------------------------------------------
class Observation:
    """what observed mode reads after a step: stats (since the last reset), accum, film, G-VPM's state"""

    def __init__(self, stats, acc, film, sv=None, nv=None):
        self.stats, self.acc, self.film, self.sv, self.nv = stats, acc, film, sv, nv


def perfect_observations(s, res, folded):
    """the observations of a device that IS the fp64 oracle (rounded to what the ABI returns): the comparator's own test"""
    out, total = [], {k: 0 for k in COUNTERS}
    for r, f in zip(res, folded):
        if r.reset:
            total = {k: 0 for k in COUNTERS}
        for k in COUNTERS:
            total[k] += f.cnt[k]
        out.append(Observation(dict(total), f.acc.astype(np.float32), tuple(a.astype(np.float32) for a in f.film),
                               None if f.sv is None else f.sv.astype(np.float32), None if f.nv is None else f.nv.astype(np.float32)))
    return out


def step_failures(s, r, f, obs, prev_stats, bar):
    """the ways observation `obs` of step r.k misses the oracle's fold `f`: [] or [text].  bar: for the sums (an exact-pass
    session's is tighter than its technique's); the film, fp32 differences of the sums, is held to the technique's driver bar"""
    bad = []
    film_bar = max(bar, BAR[s.tech])
    for k in COUNTERS:
        inc = obs.stats[k] - (0 if r.reset else prev_stats[k])
        if inc != f.cnt[k]:
            bad.append(f"{k}: the step added {inc}, the oracle {f.cnt[k]}")
    e = l2(obs.acc, f.acc, f.lum)
    if not e < bar:
        bad.append(f"accumulators: L2 {e:.3g} >= {bar:g}")
    flum = f.lum / f.emitted if s.tech == "vpm" else f.lum
    for name, a, b in zip(("throughput", "dx", "dy"), obs.film, f.film):
        e = l2(a, b, flum)
        if not e < film_bar:
            bad.append(f"film {name}: L2 {e:.3g} >= {film_bar:g}")
    if f.sv is not None and obs.sv is not None:
        if not (np.allclose(obs.sv, f.sv, rtol=1e-6) and np.allclose(obs.nv, f.nv, rtol=1e-6)):   # device_vpm's own bar
            bad.append("G-VPM per-pixel state (scale_vol / n_vol) differs")
    return bad


def first_failure(s, res, folded, observations, bar=None):
    """None, or (step index, [what failed]) of the FIRST step whose observation misses the fold: the step a report names"""
    bar = s.bar if bar is None else bar
    prev = {k: 0 for k in COUNTERS}
    for r, f, obs in zip(res, folded, observations):
        bad = step_failures(s, r, f, obs, prev, bar)
        if bad:
            return r.k, bad
        prev = obs.stats
    return None


def describe(s, r):
    st = r.step
    return (f"session {s.name} step {r.k} (it={r.it}, n={r.rec.n}, sets={r.rays.shape[0]}, scene={r.scene}, medium={r.medium_name}, "
            f"path={r.path}, radius={r.radius:.6g}{', reset' if r.reset else ''}{', again' if st.again else ''})")


# ---- the device half ----------------------------------------------------------------------------------------------------------------
class _Env:
    """environment variables set only around hip.Context(...), as the existing tests do"""

    def __init__(self, env):
        self.env = {k: str(v) for k, v in env.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _torch_photons(rec):
    import torch
    keep, soa = [], abi.PhotonSoA()
    for k in abi.PHOTON_VEC3 + abi.PHOTON_F1 + abi.PHOTON_U1:
        a = np.ascontiguousarray(getattr(rec, k))
        t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        keep.append(t)
        setattr(soa, k, t.data_ptr())
    soa.n = rec.n
    return soa, keep


class DeviceResult:
    pass


def run_device(s, res, mode, folded=None, force_path=None, hook=None):
    """Drive one handle through the session.  mode "observed": read and compare after every step (`folded` required; the first
    miss raises, naming its step); "blind": read at the end only.  force_path: every step through that upload path (the plain-SoA
    twin of a formats session).  hook(ctx, r): called after each gather (e.g. a Poisson solve in between).
    -> DeviceResult: stats, acc, film, sv, nv, exact (taken, lost), refused, kinds (grid_info()[0] per step, observed only)"""
    assert mode in ("observed", "blind")
    p = res[0].p
    with _Env(s.env):
        ctx = hip.Context(p, device=0)
    keep, pinned = [], {}
    out = DeviceResult()
    out.kinds, out.observations = [], []
    prev_stats = {k: 0 for k in COUNTERS}
    photon_tech = s.tech in ("bre3d", "bre2d", "vpm")

    def path_of(r):
        return r.path if force_path is None or r.path == "soa" else force_path

    def pin(r):
        if r.k not in pinned:
            pinned[r.k] = (hip.PinnedPhotons(r.rec.n).fill(r.rec), hip.PinnedRays(r.rays))
        return pinned[r.k]

    try:
        first = res[0]
        ctx.upload_scene(*first.tris)
        ctx.upload_medium(first.m)
        if first.table.size:
            ctx.upload_bsdfs(first.table)
        for r in res:
            if r.reset:
                ctx.reset()
            if r.upload_scene:
                ctx.upload_scene(*r.tris)
            if r.upload_medium:
                ctx.upload_medium(r.m)
            if r.upload_table:
                ctx.upload_bsdfs(r.table)
            if r.refused_table is not None:
                try:
                    ctx.upload_bsdfs(r.refused_table)
                except hip.GvpmError as e:
                    assert e.code in (abi.GVPM_ERR_INVALID_ARG, abi.GVPM_ERR_UNSUPPORTED), e
                else:
                    raise AssertionError(describe(s, r) + ": the table was not refused")
            if r.set_scale is not None:
                ctx.set_global_scale(r.set_scale)
            path = path_of(r)
            prefetched = path == "prefetch" and r.k > 0 and r.upload_records and r.upload_rays
            if photon_tech and not prefetched:
                if path in ("packed", "linked") and r.upload_records:
                    ctx.upload_materials(r.mtable)
                if r.upload_records:
                    if path == "packed":
                        ctx.upload_photons_packed(r.pk)
                    elif path == "linked" and r.blob is not None:
                        ctx.upload_photons_linked(r.blob)
                    elif path in ("pinned", "prefetch"):
                        ctx.upload_pinned(photons=pin(r)[0])
                    elif path == "dev":
                        import torch
                        soa, k = _torch_photons(r.rec)
                        keep.append(k)
                        torch.cuda.synchronize()      # (the copies run on torch's stream, the gather on the handle's)
                        ctx.upload_photons_dev(soa)
                    else:
                        ctx.upload_photons(r.rec)
                if r.upload_rays:
                    if path == "packed":
                        ctx.upload_camera_beams_packed(r.rp)
                    elif path == "compact":
                        ctx.upload_sensor(r.sensor)
                        ctx.upload_camera_beams_compact(r.comp, r.full)
                    elif path in ("pinned", "prefetch"):
                        ctx.upload_pinned(rays=pin(r)[1])
                    elif path == "dev":
                        import torch
                        t = torch.from_numpy(r.rays.view(np.uint8).reshape(-1).copy()).cuda()
                        keep.append(t)
                        torch.cuda.synchronize()
                        ctx.upload_camera_beams_dev(t.data_ptr(), r.rays.shape[0])
                    else:
                        ctx.upload_camera_beams(r.rays)
            elif not photon_tech:
                if r.upload_records:
                    if s.tech == "planes":
                        ctx.upload_planes(r.rec, r.extra["w1"], r.extra["len1"])
                    else:
                        ctx.upload_beams(r.rec, r.extra["end_n"])
                if r.upload_rays:
                    ctx.upload_camera_beams(r.rays)
            if s.tech == "vpm" and r.upload_rays:
                ctx.upload_vpm_samples(r.samples)
            # the copy of the NEXT step's inputs is started before this step's gather (gvpm_prefetch_*)
            nxt = res[r.k + 1] if r.k + 1 < len(res) else None
            if nxt is not None and photon_tech and path_of(nxt) == "prefetch" and nxt.upload_records and nxt.upload_rays:
                pp, pr = pin(nxt)
                ctx.prefetch(pp, pr)
            got = ctx.radius()
            assert got == r.radius, describe(s, r) + f": ctx.radius() {got!r}, the mirrored schedule {r.radius!r}"
            ctx.gather(r.it, r.nb)
            if hook is not None:
                hook(ctx, r)
            if mode == "observed":
                st = ctx.stats()
                sv, nv = ctx.download_vpm_state() if s.tech == "vpm" else (None, None)
                obs = Observation(st, ctx.download_accum(), ctx.download_film(r.it, True), sv, nv)
                out.kinds.append(ctx.grid_info()[0])
                out.observations.append(obs)
                if folded is not None:
                    bad = step_failures(s, r, folded[r.k], obs, prev_stats, s.bar)
                    assert not bad, describe(s, r) + ": " + "; ".join(bad)
                prev_stats = st
        last = res[-1]
        out.stats = ctx.stats()
        out.acc = ctx.download_accum().astype(np.float64)
        out.film = ctx.download_film(last.it, True)
        out.sv, out.nv = ctx.download_vpm_state() if s.tech == "vpm" else (None, None)
        out.exact = ctx.exact_shifts()
        out.refused = ctx.refused_steps()
    finally:
        ctx.close()
        for pp, pr in pinned.values():
            pp.close()
            pr.close()
    return out


def expected_totals(res, folded):
    """the counters a handle shows at the end: the oracle's step counters since the last reset"""
    total = {k: 0 for k in COUNTERS}
    for r, f in zip(res, folded):
        if r.reset:
            total = {k: 0 for k in COUNTERS}
        for k in COUNTERS:
            total[k] += f.cnt[k]
    return total


def check_final(s, res, folded, dev, bar=None):
    """the end of a run (either mode) against the oracle's fold: counters exact, sums and film within the bar"""
    bar = s.bar if bar is None else bar
    f, total = folded[-1], expected_totals(res, folded)
    for k in COUNTERS:
        assert dev.stats[k] == total[k], (s.name, k, dev.stats, total)
    e = l2(dev.acc, f.acc, f.lum)
    assert e < bar, (s.name, "accumulators", e, bar)
    flum = f.lum / f.emitted if s.tech == "vpm" else f.lum
    for a, b in zip(dev.film, f.film):
        assert l2(a, b, flum) < max(bar, BAR[s.tech]), (s.name, "film", l2(a, b, flum))
    if f.sv is not None:
        assert np.allclose(dev.sv, f.sv, rtol=1e-6) and np.allclose(dev.nv, f.nv, rtol=1e-6), (s.name, "G-VPM state")
    return e


def check_blind_against_observed(s, blind, observed):
    """blind and observed runs of one session: counters equal, sums to the device-against-device bar"""
    for k in COUNTERS:
        assert blind.stats[k] == observed.stats[k], (s.name, k, blind.stats, observed.stats)
    e = l2(blind.acc, observed.acc, float(observed.acc[..., 0:3].mean()))
    assert e < DEVICE_BAR, (s.name, "blind against observed", e)
    return e


# ---- the sessions -------------------------------------------------------------------------------------------------------------------
SIZES = {   # tech -> (scene, W, H, N, scale)
    "bre3d": ("cbox", 32, 24, 8000, 3.0), "bre2d": ("cbox", 32, 24, 8000, 3.0), "vpm": ("cbox", 24, 20, 8000, 5.0),
    "beams3d": ("cbox", 24, 20, 4000, 3.0), "beams1d": ("cbox", 24, 20, 4000, 3.0), "planes": ("cbox_in", 24, 20, 2000, 1.0),
}


def collapse(tech):
    """N -> 1 -> 0 -> 1.5 N (regrowth) -> 64 -> N; beam sets all -> 37 -> none -> all; records in a small central box, then
    everywhere, then everywhere -> a small box in a corner; one gather again without uploading in the middle"""
    scene, W, H, N, scale = SIZES[tech]
    steps = [
        Step(1, N * 2, box="centre"),         # (the box keeps about an eighth: shoot more so that the step still evaluates)
        Step(2, N),
        Step(3, 1, rays="37"),
        Step(4, 0, rays="none"),
        Step(5, N * 3 // 2),
        Step(6, again=True),
        Step(7, 64),
        Step(8, N),
        Step(9, N * 2, box="corner"),
        Step(11, N // 2, rays=0.5),           # `it` skips 10
        Step(12, 1),
        Step(13, N),
    ]
    # (G-BRE 2D from another draw: with the first, one pair of step 5 sits on the rim of its disc -- the fp32 oracle evaluates
    # 3 319 pairs where the fp64 oracle evaluates 3 320, 3.4e-3 of the mean luminance; the session is softened, not the bar)
    return Session(f"collapse-{tech}", tech, scene, W, H, N, scale, steps, first_gen=21 if tech == "bre2d" else 1)


def swap(tech):
    """cbox (14 occluders) <-> fogroom (782: across the near grid's 64-occluder threshold both ways), medium grey <-> all <->
    thick, set_global_scale above every earlier radius under the 782-triangle scene (the near grid's reach) then far below,
    reset in the middle and on from it = 1"""
    scene, W, H, N, scale = SIZES[tech]
    steps = [
        Step(1, N),
        Step(2, N, scene="fogroom"),
        Step(3, N, medium="all"),
        Step(4, N, scale=scale * 1.5),
        Step(5, N),
        Step(6, N, scale=scale * 0.3, medium="thick"),
        Step(7, N, scene="cbox"),
        Step(1, N, reset=True, medium="grey"),
        Step(2, 0, scene="fogroom"),
        Step(3, N, medium="all"),
        Step(4, N, scale=scale * 2.0),
        Step(6, N, scene="cbox", medium="thick"),
        Step(7, N // 2, medium="grey"),
    ]
    return Session(f"swap-{tech}", tech, scene, W, H, N, scale, steps)


def _conductor_tables():
    """cbox_conductor's records name heads 0 and 1.  The fp64 oracle is frozen before GVPM_BSDF_MIXTURE (it knows the conductor and
    the Lambertian, not the kind), so the mixture tables are the ones it can still judge: per wall {that wall's conductor, Lambertian}
    at weights (1, 0) -- the pin of test_mixture_parents_gpu.test_weights_one_zero_are_the_oracles_plain_conductor -- which the
    device evaluates through its mixture kernels (bsdfMixtures) and the oracle as the plain conductor table behind them."""
    import mixture_cases as MC
    sc = SynthScene("cbox_conductor", 8, 8)
    walls = sc.bsdfs()
    assert walls.size == 2 and abi.bsdf_heads(walls).all()
    changed = walls.copy()
    changed["exponent"][0] = 0.2                      # the copper floor's alpha: one parameter
    # mixtures at the heads the records name, their children (the walls' conductors) behind them
    heads = [MC.mixture((1.0, 0.0), (2, MC.DIFFUSE)), MC.mixture((1.0, 0.0), (3, MC.DIFFUSE))]
    mixed, mixed_changed = np.concatenate(heads + [walls]), np.concatenate(heads + [changed])
    bad1 = mixed.copy()
    bad1["specular"][0, 0] = -0.1                     # a negative weight
    bad2 = mixed.copy()
    bad2["eta"][1, 0] = 9.0                           # a child past the table
    return {"walls": (walls, False, walls), "changed": (changed, False, changed), "mixed": (mixed, False, walls),
            "mixed_changed": (mixed_changed, False, changed), "bad1": (bad1, True, None), "bad2": (bad2, True, None)}


def tables(tech):
    """a glossy scene's table, one parameter changed, a refused table (the previous one stays in force), a table with
    GVPM_BSDF_MIXTURE heads, one without again: bsdfMixtures flips both ways on one handle"""
    W, H, N, scale = (24, 20, 12000, 4.0) if tech == "bre3d" else (20, 16, 12000, 6.0)
    steps = [
        Step(1, N, table="walls"),
        Step(2, N, table="changed"),
        Step(3, N, table="bad1"),
        Step(4, N, table="mixed"),
        Step(5, N, table="walls"),
        Step(6, 0),
        Step(7, N // 2, table="mixed_changed"),
        Step(8, again=True),
        Step(9, N, table="changed"),
        Step(10, N, table="bad2"),
        Step(11, N, table="mixed"),
        Step(12, N, table="walls"),
    ]
    # (G-VPM from another draw: with the first, the fp32 oracle takes one shift of step 1 as a reconnection where the fp64 oracle
    # takes the null shift, 2.5e-4 of the mean luminance)
    return Session(f"tables-{tech}", tech, "cbox_conductor", W, H, N, scale, steps, tables=_conductor_tables(),
                   first_gen=31 if tech == "vpm" else 1)


def formats():
    """the seven upload paths twice round, sizes differing: a staging slot last filled by one format is next filled by another
    (seven paths over three slots: the second round meets every slot one further on)"""
    steps, k = [], 0
    for rnd in range(2):
        for path in PATHS:
            k += 1
            steps.append(Step(k, 4000 + 700 * ((k * 5) % 14), path=path))
    steps[10].rays = "none"                           # (a packed step without a beam set)
    return Session("formats-bre3d", "bre3d", "cbox", 32, 24, 8000, 3.0, steps)


def exact_all(tech):
    """GVPM_EXACT_ALL=1, GVPM_EXACT_EVERY=3: every shift of every step waits in the handle's list across gathers.  Scripted
    against the driver's join points (exact_passes below states them): steps 1-3 are three successive `it` with nothing swapped
    and the count and the radius changing, so the paced flush behind step 3 finds three gathers' entries; the medium and the
    scene change at steps 5, 7, 13 and 16 (counted from 1, no multiple of three) where one or two gathers' entries wait -- for
    G-BRE and for G-VPM alike up to step 10; `it` skips 11 at step 11, which for G-BRE is a join of its own (the running sum is
    rescaled) and for G-VPM none, so that the scene change of step 13 meets G-BRE with entries waiting and G-VPM just flushed."""
    scene, W, H, N, scale = SIZES[tech]
    N = N * 3 // 4
    steps = [
        Step(1, N),
        Step(2, N // 2, scale=scale * 1.2),
        Step(3, N),                                   # the paced flush: three gathers' entries
        Step(4, N // 3),
        Step(5, N, medium="all"),                     # one gather's entries wait
        Step(6, 64, scale=scale * 0.8),
        Step(7, N, scene="fogroom"),                  # two gathers' entries wait
        Step(8, 0),
        Step(9, N // 2),                              # paced
        Step(10, N),
        Step(12, N // 4, scale=scale * 1.1),          # `it` skips 11
        Step(13, N),
        Step(14, N, scene="cbox"),
        Step(15, N),
        Step(16, N // 2),
        Step(17, N, medium="grey"),
    ]
    # (G-BRE from another draw: in the first, one term of the last step moves the fp32 oracle 2.0e-5 of the mean luminance from
    # the fp64 oracle -- ten times the exact sessions' bar, which allows for fp32 accumulation noise only; the others: 6e-7)
    return Session(f"exact_all-{tech}", tech, scene, W, H, N, scale, steps, env={"GVPM_EXACT_ALL": 1, "GVPM_EXACT_EVERY": 3},
                   bar=EXACT_BAR[tech], first_gen=61 if tech == "bre3d" else 1)


def exact_all_glossy():
    """the same on a glossy scene (cbox_conductor, G-BRE 3D) at the exact pass's glossy bar: the BSDF table changes, and is once
    refused, with one or two gathers' entries waiting -- gvpm_upload_bsdfs must run the pass under the OLD table first"""
    N, scale = 12000, 4.0
    steps = [
        Step(1, N, table="walls"),
        Step(2, N // 2),
        Step(3, N, scale=scale * 1.1),                # paced
        Step(4, N),
        Step(5, N, table="changed"),                  # one gather's entries wait
        Step(6, 0),
        Step(7, N, table="bad1"),                     # refused, two gathers' entries wait (the join comes before the checks)
        Step(8, N // 3),
        Step(9, N, table="walls"),                    # two gathers' entries wait
        Step(10, N),
        Step(11, N // 2),                             # paced
        Step(13, N),                                  # `it` skips 12 behind the flush
        Step(14, N, table="changed"),
    ]
    return Session("exact_all-glossy", "bre3d", "cbox_conductor", 24, 20, N, scale, steps, tables=_conductor_tables(),
                   env={"GVPM_EXACT_ALL": 1, "GVPM_EXACT_EVERY": 3}, bar=EXACT_BAR["glossy"])


def exact_default():
    """GVPM_EXACT_EVERY unset, the fast kernels' own bands: 20 blind steps; nine successive `it` first, so that the paced flush
    behind the eighth gather runs (on the one shift in 1e5 the bands defer; the interval it then sets is 256)"""
    steps = [Step(k + 1 + (k >= 9) + (k >= 15), 4000 + 1000 * (k % 5)) for k in range(20)]
    steps[6].n, steps[6].rays = 0, "37"
    steps[11].scale = 3.5
    return Session("exact_default-bre3d", "bre3d", "cbox", 32, 24, 8000, 3.0, steps)


def exact_adaptive():
    """GVPM_EXACT_ALL=1 with GVPM_EXACT_EVERY unset: the adaptive pacing of exactAfterGather with a full list.  20 successive `it`
    at alpha = 1, about 6 000 evaluations a gather: the first paced flush comes behind the eighth gather (the default interval)
    and finds under a quarter of the 2^20-entry list, so the list is not regrown; from what it found the driver sets an interval
    of 9 to 12 gathers and flushes again within the session (exact_passes; test_sessions.py asserts both)."""
    steps = [Step(k + 1, 11000 + 500 * (k % 3), scale=3.0 * (1.0 + 0.01 * (k % 4))) for k in range(20)]
    steps[12].n, steps[12].rays = 0, "37"
    return Session("exact_adaptive-bre3d", "bre3d", "cbox", 32, 24, 12000, 3.0, steps, params=dict(alpha=1.0),
                   env={"GVPM_EXACT_ALL": 1}, bar=EXACT_BAR["bre3d"])


def exact_passes(s, res, folded):
    """The exact passes of a BLIND run under GVPM_EXACT_ALL as the driver's join points start them -> [(step, cause, gathers
    waiting, entries waiting)].  gvpm_join_exact runs a pass whenever gathers wait (exSince > 0) and something reads or rescales
    the sums: gvpm_upload_scene / _medium / _bsdfs (gvpm_api.hip; a refused table too: the join comes first), G-BRE's
    foldRunningSum when `it` is not the successor (drivers_bre.hip), and exactAfterGather behind every exFlushEvery-th gather
    ("paced"; GVPM_EXACT_EVERY, else 8 and then (capacity / 4) / (entries a gather of the last pass + 1), at most 256)."""
    fixed = "GVPM_EXACT_EVERY" in s.env
    every, cap = int(s.env.get("GVPM_EXACT_EVERY", 8)), 1 << 20
    since = entries = last_it = 0
    out = []
    for r, f in zip(res, folded):
        if r.reset:
            since = entries = last_it = 0
        cause = None
        if r.upload_scene or r.upload_medium or r.upload_table or r.refused_table is not None:
            cause = "upload"
        elif s.tech in ("bre3d", "bre2d") and last_it and r.it - 1 != last_it:
            cause = "it"
        if cause and since:
            out.append((r.k, cause, since, entries))
            since = entries = 0
        last_it = r.it
        since += 1
        entries += f.cnt["null_shifts"] + f.cnt["diffuse_shifts"] + f.cnt["failed_shifts"]
        if since >= every:
            out.append((r.k, "paced", since, entries))
            if not fixed:
                every = max(1, min(256, (cap // 4) // (entries // since + 1)))
            since = entries = 0
    return out


def bundle_auto():
    """GVPM_BUNDLE_AUTO=1: coverage alternates between the whole frame and at most half of it, steps from a moved origin"""
    N = 12000
    steps = [
        Step(1, N, rays=0.35),                        # a rank's share: bundle cells, the frame fitted
        Step(2, N, rays=0.35, moved=True),            # not the bundle the cells were keyed for: this step on the 3D grid
        Step(3, N, rays=0.35, moved=True),            # the frame fitted anew
        Step(4, N, rays="all"),                       # the whole frame: the 3D grid
        Step(5, N, rays=0.5, moved=True),             # half: inside the hysteresis band, stays 3D
        Step(6, N, rays=0.35, moved=True),            # bundle cells again, the frame still step 3's
        Step(7, N, rays=0.5, moved=True),             # half: stays bundle, but rows beyond the fitted frame: 3D for this step
        Step(8, N, rays=0.5, moved=True),             # the frame fitted anew: half the frame on bundle cells
        Step(9, N, rays=0.25, moved=True),            # inside the frame
        Step(10, N, rays="all"),
        Step(11, N // 2, rays=0.35),                  # the first origin again: not the frame's
        Step(12, 0, rays="all"),
    ]
    return Session("bundle_auto-bre3d", "bre3d", "cbox", 40, 32, N, 3.0, steps, env={"GVPM_BUNDLE_AUTO": 1})


def bundle_kinds(s, res):
    """grid_info()[0] per step as the rule of context.h / drivers_build.hip (buildGrid, fitBundle) and drivers_bre.hip predicts it:
    bundle cells when the beam sets cover at most 0.4 of the frame's pixels, left again only above 0.6; the frame (common origin,
    (u, v) range plus two pixels) is fitted at the first such build and kept; a step with a ray outside it is redone on the 3D
    grid and the frame fitted anew at the next bundle build.  (Not mirrored, because the session stays away from both: the
    two-pixel margin -- a step covers no row or at least five beyond its frame -- and the fourth such step, after which the
    handle gives up.)"""
    npix, on, kinds, frame = s.W * s.H, False, [], None      # frame: (the origin is the moved one, rows covered)
    for r in res:
        nsets = r.rays.shape[0]
        rows = int(cases.pixels_of(r.rays)[1].max()) + 1 if nsets else 0
        on = nsets > 0 and (nsets * 10 <= npix * 6 if on else nsets * 10 <= npix * 4)
        kind = 0
        if on and r.rec.n > 0:
            if frame is None:
                frame = (r.moved, rows)
            if frame[0] == r.moved and rows <= frame[1]:
                kind = 1
            else:
                frame = None
        kinds.append(kind)
    return kinds


def marathon(tech):
    """three inputs A, B, C of different sizes, cycled: G-BRE 288 steps at alpha = 1 (the radius never moves, so the mean is
    the oracle's (A + B + C) / 3), G-VPM 48 steps whose per-pixel state makes the expectation a real fold"""
    if tech == "bre3d":
        # (the largest input first: the first arrival of a larger one is refused by the build's guard and queued again BY DESIGN
        # -- DESIGN section 5, test_optimistic_step_refused_by_the_build_is_queued_again -- and refused_steps() == 0 is asserted
        # of a handle whose buffers have seen their largest input)
        n, sizes = 288, ((12000, "all"), (8000, "all"), (0, "37"))
        kw = dict(params=dict(alpha=1.0))
        scene, W, H, scale = "cbox", 32, 24, 3.0
    else:
        n, sizes = 48, ((8000, "all"), (12000, "all"), (0, "37"))
        kw = {}
        scene, W, H, scale = "cbox", 24, 20, 5.0
    steps = [Step(k + 1, sizes[k % 3][0], rays=sizes[k % 3][1]) for k in range(n)]
    return Session(f"marathon-{tech}", tech, scene, W, H, 8000, scale, steps, **kw)


def materialise_cycle(s, period=3):
    """materialise() for a session that cycles through `period` inputs: the first period's arrays, repeated (it and the
    mirrored radius are each step's own)"""
    head = copy.copy(s)
    head.steps = s.steps[:period]
    base = materialise(head)
    tech, p = TECH[s.tech], base[0].p
    scale = np.float32(p.initial_scale_volume)
    out = []
    for k, st in enumerate(s.steps):
        r = copy.copy(base[k % period])
        r.step, r.k, r.it = st, k, st.it
        r.upload_records = r.upload_rays = True
        r.radius = cases.radius_of(p, scale)
        if s.tech != "vpm":
            scale = np.float32(O.scale_volume_apa(float(scale), st.it, float(p.alpha), tech))
        out.append(r)
    return out


def all_sessions():
    """every session of tests/test_sessions_gpu.py, by name (the marathons: see marathon())"""
    out = [collapse(t) for t in TECH]
    out += [swap(t) for t in ("bre3d", "vpm", "beams3d")]
    out += [tables(t) for t in ("bre3d", "vpm")]
    out += [formats()]
    out += [exact_all(t) for t in ("bre3d", "vpm", "beams3d")]
    out += [exact_all_glossy(), exact_default(), exact_adaptive(), bundle_auto()]
    return {s.name: s for s in out}


_CACHE = {}


def prepared(s, precision=64):
    """(materialised steps, the oracle's fold) of a session, computed once per process"""
    key = (s.name, precision)
    if key not in _CACHE:
        res = _CACHE[(s.name, "res")] if (s.name, "res") in _CACHE else materialise(s)
        _CACHE[(s.name, "res")] = res
        _CACHE[key] = (res, fold(s, res, precision))
    return _CACHE[key]
