"""What the ray-tracer section of hip_kernels.HipKernels passes to the library, recorded without a GPU, for
test_raytracer_binding_pinned.py. Recorder is a HipKernels on the CPU whose _c keeps (entry, arguments) and launches nothing; a
case is one call of a public method on the inputs of raytracer_aer_scenes.general (4 x 3 x 4 cells, 2 g-points in 2 bands, 3
background layers), and its transcript is

  - per recorded call "entry_with_suffix nargs digest": the blake2b digest of the canonical form of every argument, in order;
  - "-> digest" of the returned value: its keys and each value's type, shape and dtype (a returned int also its value);
  - or "ValueError: the message" where the call was refused.

The canonical form of an argument: None; a Python or numpy scalar by type and value (1 and True differ); a tensor that is one of the
case's inputs by its label in the case's table (a swapped tau and ssa shows); a tensor that an earlier recorded call of the case got
as an argument by that call and position; any other tensor by dtype and shape if HipKernels.empty made it, by dtype, shape and
content otherwise (zeros, and what is filled by value); a numpy array by dtype, shape and content, whoever made it; a ctypes array
of pointers by the labels of the tensors it points to.

tests/golden/raytracer_binding_calls.json holds the transcripts, in golden_form, as recorded before the section was restated on one
gathered scene: `python tests/raytracer_binding_pinned.py FILE` writes them."""
import ctypes
import hashlib
import itertools
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

from rte_rrtmgp_cpp_amd.hip_kernels import HipKernels
from rte_rrtmgp_cpp_amd.phase_tables import PhaseTable
import raytracer_aer_scenes as SA
import raytracer_bw_ref as B
import raytracer_dev as D

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "raytracer_binding_calls.json")
DT = {"f64": np.float64, "f32": np.float32}
SCALARS = (bool, int, float, str, np.generic)


def _digest(parts):
    return hashlib.blake2b("\n".join(parts).encode(), digest_size=8).hexdigest()


class Recorder(HipKernels):
    def __init__(self, dtype):
        self.np_dtype = np.dtype(dtype)
        self.sfx = "_f64" if self.np_dtype == np.float64 else "_f32"
        self.tdtype = torch.float64 if self.np_dtype == np.float64 else torch.float32
        self.device = torch.device("cpu")
        self.stream = None
        self.reset({})

    def reset(self, labels):
        """labels: name -> tensor, the inputs of the next case"""
        self.names = {id(t): name for name, t in labels.items()}
        self.pointers = {t.data_ptr(): name for name, t in labels.items()}
        self.keep = list(labels.values())          # (alive, so that no id is used twice)
        self.empties, self.calls, self.forms = [], [], []

    def empty(self, shape, dtype=None):
        t = super().empty(shape, dtype)
        self.empties.append(t)
        return t

    def canon(self, v):
        if v is None:
            return "None"
        if isinstance(v, SCALARS):
            return f"{type(v).__name__} {v!r}"
        if isinstance(v, torch.Tensor):
            if id(v) in self.names:
                return "input " + self.names[id(v)]
            what = f"{v.dtype} {tuple(v.shape)}"
            if any(v is e for e in self.empties):
                return "empty " + what
            return f"made {what} {hashlib.blake2b(v.contiguous().numpy().tobytes(), digest_size=8).hexdigest()}"
        if isinstance(v, np.ndarray):
            return f"host {v.dtype} {v.shape} {hashlib.blake2b(np.ascontiguousarray(v).tobytes(), digest_size=8).hexdigest()}"
        if isinstance(v, ctypes.Array):
            return "pointers " + " ".join(self.pointers.get(p, "unknown") if p else "NULL" for p in v)
        raise TypeError(f"raytracer_binding_pinned: no canonical form for {type(v)}")

    def _c(self, name, *args):
        forms = [self.canon(a) for a in args]
        k = len(self.calls)
        for j, a in enumerate(args):          # what this call wrote may be an argument of the next
            if isinstance(a, torch.Tensor) and id(a) not in self.names:
                self.names[id(a)] = f"call {k} argument {j}"
                self.keep.append(a)
        self.calls.append(f"{name}{self.sfx} {len(args)} {_digest(forms)}")
        self.forms.append((name + self.sfx, forms))
        return 0

    def returned(self, r):
        def one(v):
            if isinstance(v, torch.Tensor):
                return f"tensor {v.dtype} {tuple(v.shape)}"
            return f"{type(v).__name__} {v!r}"
        if isinstance(r, dict):
            return [f"{k}: {one(v)}" for k, v in r.items()]
        if isinstance(r, tuple):
            return ["tuple"] + [one(v) for v in r]
        return [one(r)]


# ---- the inputs of a case

CAMERA = B.Sensor(0, 3, 2, 0.9, (100., 150., 90.), (0.6, 0., 0.2), (0., 0.6, 0.1), (0.3, 0.2, 0.9))
NPIX = 6
BG_KINDS = {"none": (False, False, False), "plain": (True, True, False), "aer": (True, True, True), "bare": (True, False, False),
            "aeronly": (True, False, True)}          # (a background, its cloud, its own aerosol)


def inputs(be, spec):
    """(a: what the methods below are called with, labels). spec: cloud, phase, lims (bools), bg (BG_KINDS), aer (none, null,
    triple), counts, profile (bools: supplied), max_events."""
    sc, bg = SA.general(be.np_dtype.type)
    d, dbg = D.dev(be, sc, bg)
    labels = dict(tau=d["tau"], ssa=d["ssa"], sfc_albedo=d["alb"], band_lims=d["lims"])
    triples = dict(cld=d["cloud"], aer=d["aer"], bg_cld=dbg.cloud, bg_aer=dbg.aerosol)
    for name, t in triples.items():
        labels.update({f"{name}_{k}": c for k, c in zip(("tau", "ssa", "g"), t)})
    labels.update(bg_tau=dbg.tau, bg_ssa=dbg.ssa)
    table = PhaseTable(mu=be.asarray(np.linspace(-1., 1., 5)), phase=be.asarray(np.full((2, 3, 5), 1.0)), cdf=be.asarray(np.full((2, 3, 5), 0.5)),
                       re0=2.5, dre=1.0, cld_re=be.asarray(np.full((sc.nz, sc.ncol), 3.0)))
    labels.update(ph_mu=table.mu, ph_phase=table.phase, ph_cdf=table.cdf, ph_cld_re=table.cld_re)
    has_bg, bg_cloud, bg_aer = BG_KINDS[spec["bg"]]
    background = None
    if has_bg:
        background = SimpleNamespace(dz=dbg.dz, tau=dbg.tau, ssa=dbg.ssa, cloud=dbg.cloud if bg_cloud else None,
                                     aerosol=dbg.aerosol if bg_aer else None)
    aerosol = {"none": None, "null": D.NO_TRIPLE, "triple": d["aer"]}[spec["aer"]]
    seven = aerosol is not None or bg_aer
    kn = tuple(sc.kn_grid)
    a = SimpleNamespace(
        sc=sc, tau=d["tau"], ssa=d["ssa"], nx=sc.nx, ny=sc.ny, dx=sc.dx, dy=sc.dy, dz=sc.dz, alb=d["alb"], mu0=sc.mu0, azimuth=sc.azimuth,
        inc_dir=sc.inc_dir, inc_dif=sc.inc_dif, kn_grid=sc.kn_grid, seed=-7, first=5, n=40, igpt=1, top_at_1=sc.top_at_1,
        independent_column=False, cloud=d["cloud"] if spec["cloud"] else None, lims=d["lims"] if spec["lims"] else None,
        phase=table if spec["phase"] else None, background=background, aerosol=aerosol, max_events=spec["max_events"], camera=CAMERA,
        k_null=be.asarray(np.ones(kn[::-1])), k_null_all=be.asarray(np.ones((2,) + kn[::-1])),
        end=np.array([0, 24, 60]), weight0=[0.5, 1.5], dif_frac=[0.25, 0.0], per_gpt=[3, 2], per_pixel=4,
        M=np.array([[1.0, 0.5], [0.0, 2.0], [0.25, 0.25]]), scale=1.5, bg_profile=None, bg_profile_all=None, counts_fw=None, counts_fw_bg=None,
        counts_bw=None, counts_cam=None, band_counts=torch.zeros((2, NPIX), dtype=torch.int64))
    labels.update(k_null=a.k_null, k_null_all=a.k_null_all, band_counts=a.band_counts)
    if spec["profile"]:
        a.bg_profile = be.asarray(np.ones((7 if seven else 5, 4)))
        a.bg_profile_all = be.asarray(np.ones((2, 7, 4)))
        labels.update(bg_profile=a.bg_profile, bg_profile_all=a.bg_profile_all)
    if spec["counts"]:
        a.counts_fw, a.counts_fw_bg = be.rt_zero_counts(sc.nz, sc.ncol), be.rt_zero_counts_bg(sc.nz, sc.ncol, 3 if has_bg else 0)
        a.counts_bw, a.counts_cam = be.rt_bw_zero_counts(NPIX), be.camera_zero_counts(2, NPIX)
        for name in ("counts_fw", "counts_fw_bg", "counts_bw", "counts_cam"):
            labels.update({f"{name}.{k}": t for k, t in getattr(a, name).items()})
    return a, labels


# ---- the public methods of the section, by family: name -> the call

def _grid(a):
    return (a.nx, a.ny, a.dx, a.dy, a.dz, a.alb, a.mu0, a.azimuth)


def _kw(a, *names):
    """the keyword arguments of a method: the medium and what `names` adds"""
    kw = dict(top_at_1=a.top_at_1, cloud=a.cloud, max_events=a.max_events, phase=a.phase)
    kw.update({"band_lims": a.lims} if "band_lims" in names else {})
    kw.update({"independent_column": a.independent_column} if "ic" in names else {})
    kw.update({"background": a.background, "aerosol": a.aerosol} if "medium" in names else {})
    return kw


PLAIN = {          # (cloud, phase, band_lims; no background, no aerosol)
    "rt_trace_counts": lambda be, a: be.rt_trace_counts(a.tau, a.ssa, a.igpt, *_grid(a), 340.0, 12.5, a.kn_grid, a.k_null, a.seed, a.first, a.n,
                                                        counts=a.counts_fw, **_kw(a, "band_lims", "ic")),
    "raytracer_sw": lambda be, a: be.raytracer_sw(a.tau, a.ssa, *_grid(a), a.inc_dir, a.inc_dif, a.kn_grid, a.per_pixel, a.seed,
                                                  **_kw(a, "band_lims", "ic")),
    "rt_bw_trace_counts": lambda be, a: be.rt_bw_trace_counts(a.tau, a.ssa, a.igpt, *_grid(a), a.kn_grid, a.k_null, a.camera, a.seed, a.first,
                                                              a.n, counts=a.counts_bw, **_kw(a, "band_lims")),
    "raytracer_bw": lambda be, a: be.raytracer_bw(a.tau, a.ssa, *_grid(a), a.inc_dir, a.kn_grid, a.camera, a.per_pixel, a.seed,
                                                  **_kw(a, "band_lims")),
}
MEDIUM = {         # (and background, aerosol)
    "rt_trace_counts_bg": lambda be, a: be.rt_trace_counts_bg(a.tau, a.ssa, a.igpt, *_grid(a), 340.0, 12.5, a.kn_grid, a.k_null, a.seed, a.first,
                                                              a.n, counts=a.counts_fw_bg, bg_profile=a.bg_profile,
                                                              **_kw(a, "band_lims", "ic", "medium")),
    "raytracer_sw_bg": lambda be, a: be.raytracer_sw_bg(a.tau, a.ssa, *_grid(a), a.inc_dir, a.inc_dif, a.kn_grid, a.per_pixel, a.seed,
                                                        **_kw(a, "band_lims", "ic", "medium")),
    "rt_trace_counts_spectral": lambda be, a: be.rt_trace_counts_spectral(a.tau, a.ssa, *_grid(a), a.end, a.weight0, a.dif_frac, a.kn_grid,
                                                                          a.k_null_all, a.seed, a.first, a.n, counts=a.counts_fw_bg,
                                                                          bg_profile=a.bg_profile_all, **_kw(a, "band_lims", "ic", "medium")),
    "raytracer_sw_spectral": lambda be, a: be.raytracer_sw_spectral(a.tau, a.ssa, *_grid(a), a.inc_dir, a.inc_dif, a.kn_grid, a.per_gpt, a.seed,
                                                                    **_kw(a, "band_lims", "ic", "medium")),
    "rt_bw_trace_counts_bg": lambda be, a: be.rt_bw_trace_counts_bg(a.tau, a.ssa, a.igpt, *_grid(a), a.kn_grid, a.k_null, a.camera, a.seed,
                                                                    a.first, a.n, counts=a.counts_bw, bg_profile=a.bg_profile,
                                                                    **_kw(a, "band_lims", "medium")),
    "raytracer_bw_bg": lambda be, a: be.raytracer_bw_bg(a.tau, a.ssa, *_grid(a), a.inc_dir, a.kn_grid, a.camera, a.per_pixel, a.seed,
                                                        **_kw(a, "band_lims", "medium")),
    "camera_trace_counts_spectral": lambda be, a: be.camera_trace_counts_spectral(a.tau, a.ssa, *_grid(a), a.end, a.weight0, a.kn_grid,
                                                                                  a.k_null_all, a.camera, a.seed, a.first, a.n, a.lims,
                                                                                  counts=a.counts_cam, bg_profile=a.bg_profile_all,
                                                                                  **_kw(a, "medium")),
    "camera_render_spectral": lambda be, a: be.camera_render_spectral(a.tau, a.ssa, *_grid(a), a.inc_dir, a.kn_grid, a.camera, a.per_gpt, a.seed,
                                                                      a.lims, a.M, **_kw(a, "medium")),
}
SETUP = {          # (cloud, band_lims and one triple)
    "rt_k_null": lambda be, a: be.rt_k_null(a.tau, a.igpt, a.nx, a.ny, a.dz, a.kn_grid, a.top_at_1, cloud=a.cloud, band_lims=a.lims,
                                            aerosol=a.aerosol),
    "rt_k_null_all": lambda be, a: be.rt_k_null_all(a.tau, a.nx, a.ny, a.dz, a.kn_grid, a.top_at_1, cloud=a.cloud, band_lims=a.lims,
                                                    aerosol=a.aerosol),
    "rt_bg_profile": lambda be, a: be.rt_bg_profile(a.background, a.igpt, a.lims, aerosol=a.aerosol),
    "rt_bg_profile_all": lambda be, a: be.rt_bg_profile_all(a.background, a.lims),
}
OTHER = {          # (no medium)
    "rt_phase_tables": lambda be, a: be.rt_phase_tables(a.phase.mu, a.phase.phase),
    "rt_phase_sample": lambda be, a: be.rt_phase_sample(a.phase, 1, a.k_null, a.k_null),
    "rt_phase_eval": lambda be, a: be.rt_phase_eval(a.phase, 0, a.k_null, a.k_null),
    "rt_zero_counts": lambda be, a: be.rt_zero_counts(4, 12),
    "rt_zero_counts_bg": lambda be, a: be.rt_zero_counts_bg(4, 12, 3),
    "rt_zero_counts_bg_nbg0": lambda be, a: be.rt_zero_counts_bg(4, 12, 0),
    "rt_bw_zero_counts": lambda be, a: be.rt_bw_zero_counts(NPIX),
    "camera_zero_counts": lambda be, a: be.camera_zero_counts(2, NPIX),
    "rt_counts_to_flux": lambda be, a: be.rt_counts_to_flux(a.band_counts, a.scale, a.k_null),
    "camera_channels": lambda be, a: be.camera_channels(a.band_counts, a.M, a.scale),
    "camera_channels_tensor_out": lambda be, a: be.camera_channels(a.band_counts, a.ph_M, a.scale, out=a.k_null),
}
METHODS = {**PLAIN, **MEDIUM, **SETUP, **OTHER}
SINGLE = ("rt_trace_counts", "rt_bw_trace_counts", "rt_trace_counts_bg", "rt_trace_counts_spectral", "rt_bw_trace_counts_bg",
          "camera_trace_counts_spectral")          # (the single-launch entries: counts=, and bg_profile= with a medium)
BARE = dict(cloud=False, phase=False, lims=True, bg="none", aer="none", counts=False, profile=False, max_events=None)
FULL = dict(cloud=True, phase=True, lims=True, bg="aer", aer="triple", counts=False, profile=False, max_events=None)


# ---- the defects of an input: name -> (the methods it is tried on, what it does to a)

def _set(**kw):
    return lambda be, a: a.__dict__.update(kw)


def _bg(**kw):
    return lambda be, a: a.background.__dict__.update({k: v(a.background) for k, v in kw.items()})


def _phase(**kw):
    def change(be, a):
        a.phase = a.phase.with_radius(a.phase.cld_re)          # (a copy: the table's fields are this case's to change)
        a.phase.__dict__.update({k: v(a.phase) for k, v in kw.items()})
    return change


TRACERS = tuple(PLAIN) + tuple(MEDIUM)
LOOPS = ("raytracer_sw", "raytracer_bw", "raytracer_sw_bg", "raytracer_bw_bg", "raytracer_sw_spectral", "camera_render_spectral")
WITH_BG = tuple(MEDIUM) + ("rt_bg_profile", "rt_bg_profile_all")
LISTS = ("rt_trace_counts_spectral", "camera_trace_counts_spectral")
DEFECTS = {
    "ncol": (TRACERS + ("rt_k_null", "rt_k_null_all"), _set(nx=5)),
    "no_lims": (TRACERS + tuple(SETUP), _set(lims=None)),
    "phase_no_radius": (TRACERS, _phase(cld_re=lambda p: None)),
    "phase_nbnd": (TRACERS, _phase(phase=lambda p: p.phase[:1], cdf=lambda p: p.cdf[:1])),
    "phase_cdf_shape": (TRACERS, _phase(cdf=lambda p: p.cdf[:, :2])),
    "phase_mu_shape": (TRACERS, _phase(mu=lambda p: p.mu[:4])),
    "phase_radius_shape": (TRACERS, _phase(cld_re=lambda p: p.cld_re[:3])),
    "bg_tau_shape": (WITH_BG, _bg(tau=lambda b: b.tau[:, :2])),
    "bg_ssa_shape": (WITH_BG, _bg(ssa=lambda b: b.ssa[:1])),
    "inc_dir_size": (LOOPS, _set(inc_dir=[1.0, 2.0, 3.0])),
    "inc_dif_size": (("raytracer_sw", "raytracer_sw_bg", "raytracer_sw_spectral"), _set(inc_dif=[1.0])),
    "per_gpt_size": (("raytracer_sw_spectral", "camera_render_spectral"), _set(per_gpt=[3, 2, 1])),
    "weight0_size": (LISTS, _set(weight0=[1.0])),
    "dif_frac_size": (("rt_trace_counts_spectral",), _set(dif_frac=[0.1, 0.2, 0.3])),
    "list_size": (LISTS, _set(end=np.array([0, 60]))),
    "list_start": (LISTS, _set(end=np.array([1, 24, 60]))),
    "list_descends": (LISTS, _set(end=np.array([0, 70, 60]))),
    "list_range": (LISTS, _set(first=30, n=31)),
    "chan_weights_1d": (("camera_channels", "camera_render_spectral"), _set(M=np.array([1.0, 0.5]))),
    "chan_weights_nbnd": (("camera_channels", "camera_render_spectral"), _set(M=np.ones((2, 3)))),
}
TWO_DEFECTS = [("ncol", "no_lims"), ("phase_no_radius", "bg_tau_shape"), ("inc_dir_size", "no_lims"), ("list_descends", "list_range"),
               ("list_size", "ncol"), ("list_start", "phase_nbnd"), ("chan_weights_nbnd", "per_gpt_size"), ("chan_weights_1d", "inc_dir_size"),
               ("no_lims", "phase_cdf_shape"), ("bg_ssa_shape", "inc_dir_size"), ("weight0_size", "list_descends"),
               ("per_gpt_size", "inc_dif_size"), ("bg_tau_shape", "no_lims")]


def cases():
    """name -> (method, spec, defects), without the precision"""
    out = {}

    def add(method, defects=(), **spec):
        name = " ".join([method] + [f"{k}={v}" for k, v in spec.items() if v != BARE[k]] + [f"defect={x}" for x in defects])
        spec = dict(BARE, **spec)
        assert name not in out, name
        out[name] = (method, spec, tuple(defects))

    some = lambda cloud, phase, lims: lims or not phase          # (band_lims None: the smaller cross, without a table)
    for cloud, phase, lims in filter(lambda c: some(*c), itertools.product((False, True), repeat=3)):
        for method in PLAIN:
            add(method, cloud=cloud, phase=phase, lims=lims)
        for method, bg, aer in itertools.product(MEDIUM, ("none", "plain", "aer") if lims else BG_KINDS, ("none", "null", "triple")):
            add(method, cloud=cloud, phase=phase, lims=lims, bg=bg, aer=aer)
    for cloud, lims, aer in itertools.product((False, True), (False, True), ("none", "null", "triple")):
        add("rt_k_null", cloud=cloud, lims=lims, aer=aer)
        add("rt_k_null_all", cloud=cloud, lims=lims, aer=aer)
    for lims, aer, bg in itertools.product((False, True), ("none", "null", "triple"), ("plain", "bare")):
        add("rt_bg_profile", lims=lims, bg=bg, aer=aer)
    for lims, bg in itertools.product((False, True), ("plain", "aer", "bare", "aeronly")):
        add("rt_bg_profile_all", lims=lims, bg=bg)
    # counts=, bg_profile= and max_events=
    for method in PLAIN:
        add(method, cloud=True, max_events=99)
    for method, bg, aer in itertools.product(MEDIUM, ("none", "plain", "aer"), ("none", "triple")):
        add(method, cloud=True, bg=bg, aer=aer, max_events=99)
    for method in SINGLE:
        mediums = [("none", "none")] if method in PLAIN else itertools.product(("none", "plain", "aer"), ("none", "triple"))
        for (bg, aer), counts, profile, max_events in itertools.product(mediums, (False, True), (False, True), (None, 7)):
            if (counts or profile) and not (profile and method in PLAIN):
                add(method, cloud=True, bg=bg, aer=aer, counts=counts, profile=profile, max_events=max_events)
    for method in OTHER:
        add(method, phase=True)
    # the refusals: one defect on the full medium, then two at once
    for defect, (methods, _) in DEFECTS.items():
        for method in methods:
            if defect != "no_lims":          # (band_lims None is crossed above)
                add(method, (defect,), **FULL)
    for pair in TWO_DEFECTS:
        for method in set(DEFECTS[pair[0]][0]) & set(DEFECTS[pair[1]][0]):
            add(method, pair, **FULL)
    return out


def run(be, method, spec, defects):
    """the transcript of one case"""
    a, labels = inputs(be, spec)
    a.ph_M = be.asarray(a.M)
    labels["ph_M"] = a.ph_M
    for x in defects:
        DEFECTS[x][1](be, a)
    if method == "rt_bg_profile" and spec["aer"] == "triple":          # (its aerosol= is the background's triple)
        a.aerosol = tuple(labels[f"bg_aer_{k}"] for k in ("tau", "ssa", "g"))
    be.reset(labels)
    try:
        r = METHODS[method](be, a)
    except ValueError as e:
        return be.calls + [f"ValueError: {e}"]
    return be.calls + ["-> " + _digest(be.returned(r))]


def transcripts():
    out = {}
    for dt in DT:
        be = Recorder(DT[dt])
        for name, case in sorted(cases().items()):
            out[f"{dt} {name}"] = run(be, *case)
    return out


def golden_form(transcripts):
    """The transcripts by method, as the golden file holds them: the number of cases and a digest of their names; in clear, how
    often each entry was called with how many arguments and how often each refusal was given; `each`, 16 bits of every case's
    transcript in the order of the names, which say where a difference lies; `digest`, 64 bits of all of them, which hold it."""
    out = {}
    for name in sorted(transcripts):
        t = transcripts[name]
        g = out.setdefault(name.split(" ")[1], dict(cases=0, names=[], digest=[], calls={}, refusals={}, each=[]))
        g["cases"] += 1
        g["names"].append(name)
        g["digest"] += [name] + t
        g["each"].append(_digest(t)[:4])
        for line in t:
            if line.startswith("ValueError"):
                g["refusals"][line] = g["refusals"].get(line, 0) + 1
            elif not line.startswith("->"):
                entry = line.rsplit(" ", 1)[0]
                g["calls"][entry] = g["calls"].get(entry, 0) + 1
    for g in out.values():
        g.update(names=_digest(g["names"]), digest=_digest(g["digest"]), each=" ".join(g["each"]), calls=dict(sorted(g["calls"].items())),
                 refusals=dict(sorted(g["refusals"].items())))
    return out


def write(form, path):
    def group(g):
        head = ", ".join(f"{json.dumps(k)}: {json.dumps(g[k])}" for k in ("cases", "names", "digest", "calls"))
        refusals = ",\n".join(f"   {json.dumps(k)}: {v}" for k, v in g["refusals"].items())
        return "{" + head + ',\n  "refusals": {' + ("\n" + refusals if refusals else "") + '},\n  "each": ' + json.dumps(g["each"]) + "}"
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(m)}: {group(g)}" for m, g in form.items()) + "\n}\n")


if __name__ == "__main__":
    write(golden_form(transcripts()), sys.argv[1])
