"""CPU tests of the aerosol entries of the ray tracers (rrx_rt_k_null_aer, rrx_rt_bg_profile_aer and the four rrx_*_aer entries,
DESIGN 4.18): declared in both precisions and exported; each argument list is that of its _bg (or plain) counterpart with the
aerosol arguments in front of the stream; every refusal answers without a GPU and names the argument. rrx_raytracer_sw_aer takes
each triple as one host array of three device pointers (it would otherwise be the longest entry of the header): the tests below
name its pointers like the other entries' and _call packs them."""
import ctypes

import numpy as np
import pytest

import abi

BASES = {"rrx_rt_k_null_aer": "rrx_rt_k_null", "rrx_rt_bg_profile_aer": "rrx_rt_bg_profile", "rrx_rt_trace_counts_aer": "rrx_rt_trace_counts_bg",
         "rrx_raytracer_sw_aer": "rrx_raytracer_sw_bg", "rrx_rt_bw_trace_counts_aer": "rrx_rt_bw_trace_counts_bg",
         "rrx_raytracer_bw_aer": "rrx_raytracer_bw_bg"}
GRID = ("aer_tau", "aer_ssa", "aer_g")
ALOFT = ("bg_aer_tau", "bg_aer_ssa", "bg_aer_g")
ADDED = {"rrx_rt_k_null_aer": GRID[:1], "rrx_rt_bg_profile_aer": ALOFT, "rrx_rt_trace_counts_aer": GRID, "rrx_raytracer_sw_aer": GRID + ALOFT,
         "rrx_rt_bw_trace_counts_aer": GRID, "rrx_raytracer_bw_aer": GRID + ALOFT}
PACKED = {"rrx_raytracer_sw_aer": {"aer": GRID, "bg_aer": ALOFT}}          # argument -> the three pointers it holds
LOOPS = ("rrx_raytracer_sw_aer", "rrx_raytracer_bw_aer")
SCENE = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, igpt=1, top_at_1=0, independent_column=0, dx=100., dy=100., dz=50., mu0=0.5, azimuth=0.3,
             knx=1, kny=2, knz=1, sensor_type=0, npx=3, npy=2, fov=1.0, seed=7, ray0=0, nrays=12, rays_per_pixel=2, photon0=0, nphotons=8,
             photons_per_pixel=2, max_events=100, nmu=5, nre=3, re0=4.0, dre=3.0, nbg=3)
SENSOR = (50., 60., 20., 0.5, 0., 0., 0., 0.5, 0., 0., 0., -1.)
LAST_EXTENT = {"rrx_rt_k_null_aer": "ngpt", "rrx_rt_bg_profile_aer": "ngpt", "rrx_rt_trace_counts_aer": "nphotons",
               "rrx_raytracer_sw_aer": "photons_per_pixel", "rrx_rt_bw_trace_counts_aer": "nrays", "rrx_raytracer_bw_aer": "rays_per_pixel"}


def _has(entry, name):
    """whether the entry takes the pointer, as an argument of its own or inside a packed one"""
    return name in abi.names(entry) or any(name in names for names in PACKED.get(entry, {}).values())


def _call(lib, entry, sfx, null=(), **over):
    """The entry on memory that the device never touches (the checks come before any HIP call). Returns the status."""
    F = np.float64 if sfx == "_f64" else np.float32
    scene = dict(SCENE, sensor=np.array(SENSOR, dtype=F), dz_bg=np.array([300., 1200., 4000., 1.], dtype=F))
    if entry.startswith("rrx_raytracer"):
        scene.update(inc_dir=np.array([1., 2.], dtype=F), inc_dif=np.array([0., 0.], dtype=F))
    scene = {k: v for k, v in scene.items() if k in abi.names(entry)}
    keep = []          # (the buffers that the packed pointers point to live until the call returns)
    for arg, names in PACKED.get(entry, {}).items():
        keep += [None if n in null else np.zeros(4, dtype=F) for n in names]
        scene[arg] = (ctypes.c_void_p * 3)(*[None if b is None else b.ctypes.data for b in keep[-3:]])
    null = tuple(n for n in null if n in abi.names(entry) or not _has(entry, n))
    return abi.call(lib, entry, sfx, null=null, **{**scene, **over})[0]


def test_header_declares_the_entries_and_they_extend_their_counterparts():
    for entry, base in BASES.items():
        assert abi.declares(entry), entry
        for sfx, F in zip(abi.SFXS, ("double", "float")):
            added = tuple((f"const {F}* const*", n) for n in PACKED[entry]) if entry in PACKED else tuple((f"const {F}*", n) for n in ADDED[entry])
            want = abi.params(base, sfx)[:-1] + added + (("void*", "stream"),)
            assert abi.params(entry, sfx) == want, entry
    # the longest entry of the header stays the one it was
    assert max(len(abi.params(e, "_f64")) for e in BASES) < len(abi.params("rrx_gas_optics_lw_fractions_allsky", "_f64"))


def test_library_exports_the_entries():
    lib = abi.lib()
    for name in BASES:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", list(BASES))
def test_the_entries_refuse_a_bad_aerosol_without_a_gpu(entry, sfx):
    lib = abi.lib()
    cases = []
    if entry == "rrx_rt_k_null_aer":
        cases += [({"null": ("band_lims_gpt", "cld_tau")}, "band_lims_gpt is NULL"), ({"nbnd": 0, "null": ("cld_tau",)}, "nbnd must be >= 1"),
                  ({"knx": 3}, "knx"), ({"null": ("tau",)}, "tau is NULL"), ({"igpt": 2}, "igpt is outside")]
    if GRID[1] in ADDED[entry]:
        cld = ("cld_tau", "cld_ssa", "cld_g")
        cases += [({"null": ("aer_ssa",)}, "aer_tau, aer_ssa, aer_g must be all NULL or all given"),
                  ({"null": ("aer_tau", "aer_g")}, "aer_tau, aer_ssa, aer_g must be all NULL or all given"),
                  ({"null": ("aer_tau",)}, "all NULL or all given"),
                  ({"null": cld + ("band_lims_gpt",) + (ALOFT + ("bg_cld_tau", "bg_cld_ssa", "bg_cld_g") if entry in LOOPS else ())}, "band_lims_gpt is NULL"),
                  ({"nbnd": 0, "null": cld + (("bg_cld_tau", "bg_cld_ssa", "bg_cld_g") if entry in LOOPS else ())}, "nbnd must be >= 1 with an aerosol triple")]
    if ALOFT[1] in ADDED[entry]:
        cld = ("cld_tau", "cld_ssa", "cld_g", "bg_cld_tau", "bg_cld_ssa", "bg_cld_g")
        # (a phase table needs the cloud triple: the loops look at it before the background)
        no_table = (("mu", "phase", "cdf", "cld_re"), dict(nmu=0, nre=0, dre=0.)) if entry in LOOPS else ((), {})
        cases += [({"null": ("bg_aer_g",)}, "bg_aer_tau, bg_aer_ssa, bg_aer_g must be all NULL or all given"),
                  ({"null": ("bg_aer_tau", "bg_aer_ssa")}, "bg_aer_tau, bg_aer_ssa, bg_aer_g must be all NULL or all given"),
                  ({"null": tuple(n for n in cld + GRID + ("band_lims_gpt",) if _has(entry, n)) + no_table[0], **no_table[1]},
                   "band_lims_gpt is NULL"),
                  ({"nbnd": 0, "null": tuple(n for n in cld + GRID if _has(entry, n)) + no_table[0], **no_table[1]},
                   "nbnd must be >= 1 with an aerosol triple")]
    if entry not in ("rrx_rt_k_null_aer",):
        # what the _bg entries refuse is still refused
        cases += [({"nbg": -1}, "nbg is negative"), ({"nbg": 257}, "nbg must be <= 256"), ({"null": ("dz_bg",)}, "dz_bg is NULL"),
                  ({"dz_bg": np.array([300., 0., 4000., 1.], dtype=np.float64 if sfx == "_f64" else np.float32)}, "dz_bg must be > 0")]
    if entry in ("rrx_rt_trace_counts_aer", "rrx_rt_bw_trace_counts_aer"):
        cases += [({"null": ("bg_profile",)}, "bg_profile is NULL")]
    if entry in LOOPS:
        cases += [({"null": ("bg_tau",)}, "bg_tau is NULL"), ({"null": ("bg_cld_ssa",)}, "bg_cld_tau, bg_cld_ssa, bg_cld_g must be all NULL or all given")]
    if entry not in ("rrx_rt_k_null_aer", "rrx_rt_bg_profile_aer"):
        cases += [({"mu0": 0.}, "mu0"), ({"knx": 3}, "knx"), ({"null": ("cld_ssa",)}, "cld_tau, cld_ssa, cld_g"), ({"null": ("tau",)}, "tau is NULL"),
                  ({"max_events": 0}, "max_events"), ({"nmu": 1}, "nmu must be >= 2"), ({"null": ("cdf",)}, "all NULL or all given")]
    assert cases
    for over, word in cases:
        assert _call(lib, entry, sfx, **over) != 0, over
        msg = abi.last_error(lib)
        assert msg.startswith(entry + sfx) and word in msg, (over, msg)


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", list(BASES))
def test_zero_extents_pass_the_checks_and_without_layers_the_background_aerosol_is_not_read(entry, sfx):
    lib = abi.lib()
    none = {LAST_EXTENT[entry]: 0}
    assert _call(lib, entry, sfx, **none) == 0
    assert _call(lib, entry, sfx, null=ADDED[entry], **none) == 0
    if entry in PACKED:
        assert _call(lib, entry, sfx, null=tuple(PACKED[entry]), **none) == 0          # (NULL arrays)
    assert _call(lib, entry, sfx, **{LAST_EXTENT[entry]: -1}) != 0
    assert LAST_EXTENT[entry] + " is negative" in abi.last_error(lib)
    if entry == "rrx_rt_bg_profile_aer":
        assert _call(lib, entry, sfx, nbg=0, null=abi.pointers(entry)) == 0
    if entry in LOOPS:
        # nbg = 0: a partly-NULL background aerosol triple is not looked at; the refusal that follows is mu0's
        assert _call(lib, entry, sfx, nbg=0, null=("bg_aer_ssa",), mu0=1.5) != 0 and "mu0" in abi.last_error(lib)
        unread = ("dz_bg", "bg_tau", "bg_ssa", "toa_up", "tod_dn_dir", "tod_dn_dif", "bg_abs_dir", "bg_abs_dif", "bg_cld_tau", "bg_cld_ssa", "bg_cld_g")
        assert _call(lib, entry, sfx, nbg=0, null=tuple(n for n in unread + ALOFT if _has(entry, n)), **none) == 0
        # with layers it is
        assert _call(lib, entry, sfx, null=("bg_aer_ssa",), mu0=0.5) != 0 and "bg_aer_tau, bg_aer_ssa, bg_aer_g" in abi.last_error(lib)
