"""CPU tests of the entries of the backward tracer with the rays of all g-points in one launch (rrx_camera_trace_counts_spectral,
rrx_camera_channels, rrx_camera_render_spectral): declared in both precisions and exported; the argument lists of the
two tracer entries are those of their _aer counterparts with the changes the header names; every refusal answers without a GPU and
names the entry and the argument; the signatures bind through _ffi. (ray_end is a device array for rrx_camera_trace_counts_spectral,
which cannot look into it: a list that does not ascend is refused by the binding, hip_kernels.camera_trace_counts_spectral, and by
rrx_camera_render_spectral, which forms the list itself from m_g >= 0.)"""
import numpy as np
import pytest

import abi

TRACE, CHANNELS, RENDER = "rrx_camera_trace_counts_spectral", "rrx_camera_channels", "rrx_camera_render_spectral"
ENTRIES = (TRACE, CHANNELS, RENDER)
SCENE = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, top_at_1=0, dx=100., dy=100., dz=50., mu0=0.5, azimuth=0.3, knx=1, kny=2, knz=1, seed=7,
             ray0=0, nrays=8, max_events=100, nmu=5, nre=3, re0=4.0, dre=3.0, nbg=3, sensor_type=2, npx=2, npy=2, fov=0., nchan=2, npix=4,
             scale=1.0)
LAST_EXTENT = {TRACE: "nrays", CHANNELS: "npix", RENDER: "npy"}


def _call(lib, entry, sfx, null=(), **over):
    """The entry on memory that the device never touches (the checks come before any HIP call). Returns the status."""
    F = np.float64 if sfx == "_f64" else np.float32
    scene = dict(SCENE, dz_bg=np.array([300., 1200., 4000., 1.], dtype=F),
                 sensor=np.array([0., 0., 0., 1., 0., 0., 0., 1., 0., 0., 0., -1.], dtype=F))
    if entry == RENDER:
        scene.update(inc_dir=np.array([1., 2.], dtype=F), rays_per_pixel_gpt=np.array([2, 3], dtype=np.int64))
    scene = {k: v for k, v in scene.items() if k in abi.names(entry)}
    return abi.call(lib, entry, sfx, null=null, **{**scene, **over})[0]


def test_header_declares_the_entries_as_their_counterparts_with_the_named_changes():
    for entry in ENTRIES:
        assert abi.declares(entry), entry
    for sfx, F in zip(abi.SFXS, ("double", "float")):
        want = list(abi.params("rrx_rt_bw_trace_counts_aer", sfx))
        want.remove(("int", "igpt"))
        at = want.index(("int", "knx"))
        want[at:at] = [("const long long*", "ray_end"), (f"const {F}*", "weight0")]
        assert list(abi.params(TRACE, sfx)) == want
        want = list(abi.params("rrx_raytracer_bw_aer", sfx))
        want[want.index(("long long", "rays_per_pixel"))] = ("const long long*", "rays_per_pixel_gpt")
        at = want.index((f"{F}*", "radiance"))
        want[at:at] = [("int", "nchan"), (f"const {F}*", "chan_weights")]
        assert list(abi.params(RENDER, sfx)) == want
        assert abi.names(CHANNELS, sfx) == ["npix", "nbnd", "nchan", "counts", "chan_weights", "scale", "out", "stream"]
    assert max(len(abi.params(e, "_f64")) for e in ENTRIES) < 58
    # the set of rrx_rt_ / rrx_raytracer_ symbols is closed: the new entries carry another prefix
    assert not [s for s in abi.declared_symbols() if "spectral" in s and "bw" in s]


def test_library_exports_the_entries_and_they_bind():
    lib = abi.lib()
    for name in ENTRIES:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx
            assert len(lib.converters(name + sfx)) == len(abi.params(name, sfx))


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_entries_refuse_without_a_gpu(entry, sfx):
    lib = abi.lib()
    F = np.float64 if sfx == "_f64" else np.float32
    if entry == CHANNELS:
        cases = [({"nchan": 0}, "nchan must be >= 1"), ({"nbnd": 0}, "nbnd must be >= 1"), ({"null": ("chan_weights",)}, "chan_weights is NULL"),
                 ({"null": ("counts",)}, "counts is NULL"), ({"null": ("out",)}, "out is NULL"), ({"npix": 2**31}, "npix exceeds")]
    else:
        cases = [({"ngpt": 1025}, "ngpt must be <= 1024"), ({"null": ("band_lims_gpt",)}, "band_lims_gpt is NULL"),
                 ({"nbnd": 0}, "nbnd must be >= 1"), ({"mu0": 0.}, "mu0"), ({"knx": 3}, "knx"), ({"null": ("cld_ssa",)}, "cld_tau, cld_ssa, cld_g"),
                 ({"null": ("tau",)}, "tau is NULL"), ({"max_events": 0}, "max_events"), ({"nmu": 1}, "nmu must be >= 2"),
                 ({"null": ("cdf",)}, "all NULL or all given"), ({"nbg": -1}, "nbg is negative"), ({"nbg": 257}, "nbg must be <= 256"),
                 ({"null": ("dz_bg",)}, "dz_bg is NULL"), ({"dz_bg": np.array([300., 0., 4000., 1.], dtype=F)}, "dz_bg must be > 0"),
                 ({"null": ("aer_ssa",)}, "aer_tau, aer_ssa, aer_g must be all NULL or all given"), ({"sensor_type": 4}, "sensor_type"),
                 ({"null": ("sensor",)}, "sensor is NULL"), ({"null": ("n_clamped",)}, "n_clamped is NULL")]
    if entry == TRACE:
        cases += [({"null": ("ray_end",)}, "ray_end is NULL"), ({"null": ("weight0",)}, "weight0 is NULL"), ({"null": ("k_null",)}, "k_null is NULL"),
                  ({"null": ("bg_profile",)}, "bg_profile is NULL"), ({"ray0": -1}, "ray0 is negative"), ({"null": ("counts",)}, "counts is NULL")]
    if entry == RENDER:
        m = lambda *v: np.array(v, dtype=np.int64)
        cases += [({"rays_per_pixel_gpt": m(2, -1)}, "rays_per_pixel_gpt is negative at g-point 1"),
                  ({"inc_dir": np.array([1., 0.], dtype=F)}, "g-point 1, which has no incident flux"),
                  ({"inc_dir": np.array([1., -2.], dtype=F)}, "inc_dir must be >= 0"),
                  ({"null": ("rays_per_pixel_gpt",)}, "rays_per_pixel_gpt is NULL"), ({"null": ("inc_dir",)}, "inc_dir is NULL"),
                  ({"nchan": 0}, "nchan must be >= 1"), ({"nchan": -1}, "nchan must be >= 1"), ({"null": ("chan_weights",)}, "chan_weights is NULL"),
                  ({"null": ("radiance",)}, "radiance is NULL"), ({"null": ("bg_tau",)}, "bg_tau is NULL"),
                  ({"null": ("bg_aer_g",)}, "bg_aer_tau, bg_aer_ssa, bg_aer_g must be all NULL or all given")]
    for over, word in cases:
        assert _call(lib, entry, sfx, **over) != 0, over
        msg = abi.last_error(lib)
        assert msg.startswith(entry + sfx) and word in msg, (over, msg)


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_extents_return_zero(entry, sfx):
    lib = abi.lib()
    assert _call(lib, entry, sfx, **{LAST_EXTENT[entry]: 0}) == 0
    assert _call(lib, entry, sfx, **{LAST_EXTENT[entry]: -1}) != 0
    assert LAST_EXTENT[entry] + " is negative" in abi.last_error(lib)
    if entry != CHANNELS:
        assert _call(lib, entry, sfx, nz=0, null=abi.pointers(entry)) == 0
