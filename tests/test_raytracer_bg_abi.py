"""CPU tests of the background-atmosphere entries (rrx_rt_bg_profile and the four rrx_*_bg entries of the ray tracers, DESIGN
4.17): declared in both precisions and exported; the _bg entries' argument lists are those of the _phase entries with the new
outputs behind the existing ones and nbg, dz_bg and the background in front of the stream; every refusal answers without a GPU
and names the argument."""
import numpy as np
import pytest

import abi

BASES = {"rrx_rt_trace_counts_bg": "rrx_rt_trace_counts_phase", "rrx_raytracer_sw_bg": "rrx_raytracer_sw_phase",
         "rrx_rt_bw_trace_counts_bg": "rrx_rt_bw_trace_counts_phase", "rrx_raytracer_bw_bg": "rrx_raytracer_bw_phase"}
ALL = list(BASES) + ["rrx_rt_bg_profile"]
TABLE = ("mu", "phase", "cdf", "cld_re")
BG_TRIPLE = ("bg_cld_tau", "bg_cld_ssa", "bg_cld_g")
SCENE = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, igpt=1, top_at_1=0, independent_column=0, dx=100., dy=100., dz=50., mu0=0.5, azimuth=0.3,
             knx=1, kny=2, knz=1, sensor_type=0, npx=3, npy=2, fov=1.0, seed=7, ray0=0, nrays=12, rays_per_pixel=2, photon0=0, nphotons=8,
             photons_per_pixel=2, max_events=100, nmu=5, nre=3, re0=4.0, dre=3.0, nbg=3)
SENSOR = (50., 60., 20., 0.5, 0., 0., 0., 0.5, 0., 0., 0., -1.)
LAST_EXTENT = {"rrx_rt_trace_counts_bg": "nphotons", "rrx_raytracer_sw_bg": "photons_per_pixel", "rrx_rt_bw_trace_counts_bg": "nrays",
               "rrx_raytracer_bw_bg": "rays_per_pixel", "rrx_rt_bg_profile": "ngpt"}


def _call(lib, entry, sfx, null=(), **over):
    """The entry on memory that the device never touches (the checks come before any HIP call). Returns the status."""
    F = np.float64 if sfx == "_f64" else np.float32
    scene = dict(SCENE, sensor=np.array(SENSOR, dtype=F), dz_bg=np.array([300., 1200., 4000., 1.], dtype=F))
    if entry.startswith("rrx_raytracer"):
        scene.update(inc_dir=np.array([1., 2.], dtype=F), inc_dif=np.array([0., 0.], dtype=F))
    scene = {k: v for k, v in scene.items() if k in abi.names(entry)}
    over = {k: (np.asarray(v, dtype=F) if k == "dz_bg" else v) for k, v in over.items()}
    return abi.call(lib, entry, sfx, null=null, **{**scene, **over})[0]


def test_header_declares_the_entries_and_they_extend_the_phase_entries():
    for name in ALL:
        assert abi.declares(name), name
    for sfx, F in zip(abi.SFXS, ("double", "float")):
        table = (("int", "nmu"), ("int", "nre"), (F, "re0"), (F, "dre"), (f"const {F}*", "mu"), (f"const {F}*", "phase"),
                 (f"const {F}*", "cdf"), (f"const {F}*", "cld_re"))
        medium = tuple((f"const {F}*", n) for n in ("bg_tau", "bg_ssa") + BG_TRIPLE)
        tails = {"rrx_rt_trace_counts_bg": (("const " + F + "*", "bg_profile"),), "rrx_rt_bw_trace_counts_bg": (("const " + F + "*", "bg_profile"),),
                 "rrx_raytracer_sw_bg": medium, "rrx_raytracer_bw_bg": medium}
        new_counts = tuple(("unsigned long long*", n) for n in ("toa_up", "tod_dn_dir", "tod_dn_dif", "bg_abs_dir", "bg_abs_dif"))
        new_fluxes = tuple((F + "*", n) for n in ("toa_up", "tod_dn_dir", "tod_dn_dif", "bg_abs_dir", "bg_abs_dif"))
        outs = {"rrx_rt_trace_counts_bg": new_counts, "rrx_raytracer_sw_bg": new_fluxes, "rrx_rt_bw_trace_counts_bg": (), "rrx_raytracer_bw_bg": ()}
        for entry, base in BASES.items():
            head = abi.params(base, sfx)[:-len(table) - 1]
            want = head + outs[entry] + table + (("int", "nbg"), (f"const {F}*", "dz_bg")) + tails[entry] + (("void*", "stream"),)
            assert abi.params(entry, sfx) == want, entry
        assert abi.params("rrx_rt_bg_profile", sfx) == (("int", "nbg"), ("int", "ngpt"), ("int", "nbnd"), ("int", "igpt"), (f"const {F}*", "dz_bg"),
                                                        (f"const {F}*", "bg_tau"), (f"const {F}*", "bg_ssa"), ("const int*", "band_lims_gpt")) \
            + tuple((f"const {F}*", n) for n in BG_TRIPLE) + ((F + "*", "bg_profile"), ("void*", "stream"))


def test_library_exports_the_entries():
    lib = abi.lib()
    for name in ALL:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ALL)
def test_the_entries_refuse_a_bad_background_without_a_gpu(entry, sfx):
    lib = abi.lib()
    cases = [({"nbg": -1}, "nbg is negative"), ({"nbg": 257}, "nbg must be <= 256"), ({"null": ("dz_bg",)}, "dz_bg is NULL"),
             ({"dz_bg": [300., 0., 4000., 1.]}, "dz_bg must be > 0"), ({"dz_bg": [300., 1200., -5., 1.]}, "dz_bg must be > 0"),
             ({"dz_bg": [float("nan"), 1200., 4000., 1.]}, "dz_bg must be > 0"), ({"dz_bg": [300., float("inf"), 4000., 1.]}, "dz_bg must be > 0")]
    if entry in ("rrx_rt_trace_counts_bg", "rrx_rt_bw_trace_counts_bg"):
        cases += [({"null": ("bg_profile",)}, "bg_profile is NULL")]
    else:
        cases += [({"null": ("bg_tau",)}, "bg_tau is NULL"), ({"null": ("bg_ssa",)}, "bg_ssa is NULL"),
                  ({"null": ("bg_cld_ssa",)}, "bg_cld_tau, bg_cld_ssa, bg_cld_g must be all NULL or all given"),
                  ({"null": ("bg_cld_tau", "bg_cld_g")}, "all NULL or all given")]
    if entry == "rrx_rt_bg_profile":
        cases += [({"null": ("bg_profile",)}, "bg_profile is NULL"), ({"igpt": 2}, "igpt is outside"),
                  ({"null": ("band_lims_gpt",)}, "band_lims_gpt is NULL")]
    elif entry in ("rrx_rt_trace_counts_bg", "rrx_raytracer_sw_bg"):
        cases += [({"null": (n,)}, n + " is NULL") for n in ("toa_up", "tod_dn_dir", "tod_dn_dif", "bg_abs_dir", "bg_abs_dif")]
    if entry != "rrx_rt_bg_profile":
        # what the _phase entries refuse is still refused
        cases += [({"mu0": 0.}, "mu0"), ({"knx": 3}, "knx"), ({"null": ("cld_ssa",)}, "cld_tau, cld_ssa, cld_g"), ({"null": ("tau",)}, "tau is NULL"),
                  ({"max_events": 0}, "max_events"), ({"nmu": 1}, "nmu must be >= 2"), ({"null": ("cdf",)}, "all NULL or all given")]
    for over, word in cases:
        assert _call(lib, entry, sfx, **over) != 0, over
        msg = abi.last_error(lib)
        assert msg.startswith(entry + sfx) and word in msg, (over, msg)


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ALL)
def test_zero_extents_and_the_largest_background_pass_the_checks(entry, sfx):
    lib = abi.lib()
    none = {LAST_EXTENT[entry]: 0}
    assert _call(lib, entry, sfx, **none) == 0
    assert _call(lib, entry, sfx, nbg=256, **none) == 0
    assert _call(lib, entry, sfx, **{LAST_EXTENT[entry]: -1}) != 0
    assert LAST_EXTENT[entry] + " is negative" in abi.last_error(lib)
    if entry == "rrx_rt_bg_profile":
        assert _call(lib, entry, sfx, nbg=0, null=abi.pointers(entry)) == 0
    else:
        # nbg = 0: neither dz_bg nor the background arrays nor the new outputs are read, with or without a table
        unread = ("dz_bg", "bg_profile", "bg_tau", "bg_ssa", "toa_up", "tod_dn_dir", "tod_dn_dif", "bg_abs_dir", "bg_abs_dif") + BG_TRIPLE
        assert _call(lib, entry, sfx, nbg=0, null=unread, **none) == 0
        assert _call(lib, entry, sfx, nbg=0, null=unread + TABLE, nmu=0, nre=0, dre=0., **none) == 0
        assert _call(lib, entry, sfx, nbg=0, null=unread, mu0=1.5) != 0 and "mu0" in abi.last_error(lib)
