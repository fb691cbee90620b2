"""CPU tests of the entries of the forward tracer with all g-points in one launch (rrx_rt_k_null_all, rrx_rt_bg_profile_all,
rrx_rt_trace_counts_spectral, rrx_raytracer_sw_spectral): declared in both precisions and exported; each argument list
is that of its _aer counterpart with the changes the header names; every refusal answers without a GPU and names the argument.
(photon_end is a device array for rrx_rt_trace_counts_spectral, which cannot look into it: a list that does not ascend is refused by
the binding, hip_kernels.rt_trace_counts_spectral, and by rrx_raytracer_sw_spectral, which forms the list itself from m_g >= 0.)"""
import ctypes

import numpy as np
import pytest

import abi

BASES = {"rrx_rt_k_null_all": "rrx_rt_k_null_aer", "rrx_rt_bg_profile_all": "rrx_rt_bg_profile_aer",
         "rrx_rt_trace_counts_spectral": "rrx_rt_trace_counts_aer", "rrx_raytracer_sw_spectral": "rrx_raytracer_sw_aer"}
SCENE = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, top_at_1=0, independent_column=0, dx=100., dy=100., dz=50., mu0=0.5, azimuth=0.3,
             knx=1, kny=2, knz=1, seed=7, photon0=0, nphotons=8, max_events=100, nmu=5, nre=3, re0=4.0, dre=3.0, nbg=3)
LAST_EXTENT = {"rrx_rt_k_null_all": "ngpt", "rrx_rt_bg_profile_all": "ngpt", "rrx_rt_trace_counts_spectral": "nphotons",
               "rrx_raytracer_sw_spectral": "nz"}
LOOP = "rrx_raytracer_sw_spectral"


def _call(lib, entry, sfx, null=(), **over):
    """The entry on memory that the device never touches (the checks come before any HIP call). Returns the status."""
    F = np.float64 if sfx == "_f64" else np.float32
    scene = dict(SCENE, dz_bg=np.array([300., 1200., 4000., 1.], dtype=F))
    if entry == LOOP:
        scene.update(inc_dir=np.array([1., 2.], dtype=F), inc_dif=np.array([0., 0.], dtype=F),
                     photons_per_pixel_gpt=np.array([2, 3], dtype=np.int64))
    scene = {k: v for k, v in scene.items() if k in abi.names(entry)}
    return abi.call(lib, entry, sfx, null=null, **{**scene, **over})[0]


def test_header_declares_the_entries_as_their_counterparts_with_the_named_changes():
    for entry, base in BASES.items():
        assert abi.declares(entry), entry
        for sfx, F in zip(abi.SFXS, ("double", "float")):
            want = list(abi.params(base, sfx))
            if entry in ("rrx_rt_k_null_all", "rrx_rt_bg_profile_all"):
                want.remove(("int", "igpt"))
            elif entry == "rrx_rt_trace_counts_spectral":
                want.remove(("int", "igpt"))
                at = want.index((F, "inc_dir"))
                want[at:at+2] = [("const long long*", "photon_end"), (f"const {F}*", "weight0"), (f"const {F}*", "dif_frac")]
            else:
                want[want.index(("long long", "photons_per_pixel"))] = ("const long long*", "photons_per_pixel_gpt")
            assert list(abi.params(entry, sfx)) == want, entry
    assert len(abi.params("rrx_rt_trace_counts_spectral", "_f64")) == 57 == len(abi.params("rrx_raytracer_sw_spectral", "_f64"))
    assert max(len(abi.params(e, "_f64")) for e in BASES) < 58 == len(abi.params("rrx_gas_optics_lw_fractions_allsky", "_f64"))


def test_library_exports_the_entries():
    lib = abi.lib()
    for name in BASES:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", list(BASES))
def test_the_entries_refuse_without_a_gpu(entry, sfx):
    lib = abi.lib()
    F = np.float64 if sfx == "_f64" else np.float32
    cases = [({"ngpt": 1025}, "ngpt must be <= 1024")]
    if entry == "rrx_rt_k_null_all":
        cases += [({"null": ("band_lims_gpt", "cld_tau")}, "band_lims_gpt is NULL"), ({"nbnd": 0, "null": ("cld_tau",)}, "nbnd must be >= 1"),
                  ({"knx": 3}, "knx"), ({"null": ("tau",)}, "tau is NULL"), ({"null": ("k_null",)}, "k_null is NULL"), ({"dz": 0.}, "dz must be > 0")]
    if entry == "rrx_rt_bg_profile_all":
        cases += [({"null": ("bg_aer_g",)}, "bg_aer_tau, bg_aer_ssa, bg_aer_g must be all NULL or all given"),
                  ({"null": ("bg_cld_ssa",)}, "bg_cld_tau, bg_cld_ssa, bg_cld_g must be all NULL or all given"),
                  ({"null": ("bg_tau",)}, "bg_tau is NULL"), ({"null": ("bg_profile",)}, "bg_profile is NULL")]
    if entry != "rrx_rt_k_null_all":
        cases += [({"nbg": -1}, "nbg is negative"), ({"nbg": 257}, "nbg must be <= 256"), ({"null": ("dz_bg",)}, "dz_bg is NULL"),
                  ({"dz_bg": np.array([300., 0., 4000., 1.], dtype=F)}, "dz_bg must be > 0")]
    if entry in ("rrx_rt_trace_counts_spectral", LOOP):
        cases += [({"mu0": 0.}, "mu0"), ({"knx": 3}, "knx"), ({"null": ("cld_ssa",)}, "cld_tau, cld_ssa, cld_g"), ({"null": ("tau",)}, "tau is NULL"),
                  ({"max_events": 0}, "max_events"), ({"nmu": 1}, "nmu must be >= 2"), ({"null": ("cdf",)}, "all NULL or all given")]
    if entry == "rrx_rt_trace_counts_spectral":
        cases += [({"null": ("aer_ssa",)}, "aer_tau, aer_ssa, aer_g must be all NULL or all given"),
                  ({"null": ("photon_end",)}, "photon_end is NULL"), ({"null": ("weight0",)}, "weight0 is NULL"),
                  ({"null": ("dif_frac",)}, "dif_frac is NULL"), ({"null": ("bg_profile",)}, "bg_profile is NULL"),
                  ({"photon0": -1}, "photon0 is negative"), ({"null": ("toa_up",)}, "toa_up is NULL")]
    if entry == LOOP:
        m = lambda *v: np.array(v, dtype=np.int64)
        cases += [({"photons_per_pixel_gpt": m(2, -1)}, "photons_per_pixel_gpt is negative at g-point 1"),
                  ({"photons_per_pixel_gpt": m(2, 3), "inc_dir": np.array([1., 0.], dtype=F)}, "g-point 1, which has no incident flux"),
                  ({"inc_dir": np.array([1., -2.], dtype=F)}, "inc_dir, inc_dif must be >= 0"),
                  ({"null": ("photons_per_pixel_gpt",)}, "photons_per_pixel_gpt is NULL"),
                  ({"null": ("bg_tau",)}, "bg_tau is NULL"), ({"null": ("tod_dn_dif",)}, "tod_dn_dif is NULL")]
    for over, word in cases:
        assert _call(lib, entry, sfx, **over) != 0, over
        msg = abi.last_error(lib)
        assert msg.startswith(entry + sfx) and word in msg, (over, msg)


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", list(BASES))
def test_zero_extents_return_zero(entry, sfx):
    lib = abi.lib()
    assert _call(lib, entry, sfx, **{LAST_EXTENT[entry]: 0}) == 0
    assert _call(lib, entry, sfx, **{LAST_EXTENT[entry]: -1}) != 0
    assert LAST_EXTENT[entry] + " is negative" in abi.last_error(lib)
    if entry == "rrx_rt_bg_profile_all":
        assert _call(lib, entry, sfx, nbg=0, null=abi.pointers(entry)) == 0
    if entry == LOOP:
        # a packed triple of NULLs and a NULL array are both no aerosol; nbg = 0 reads nothing of the background
        assert _call(lib, entry, sfx, nz=0, aer=(ctypes.c_void_p * 3)(), null=("bg_aer",)) == 0
        assert _call(lib, entry, sfx, nbg=0, null=("bg_aer", "dz_bg", "bg_tau", "bg_ssa", "toa_up", "bg_abs_dir"), mu0=1.5) != 0
        assert "mu0" in abi.last_error(lib)
