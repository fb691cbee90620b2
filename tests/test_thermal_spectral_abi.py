"""CPU tests of the entries of the thermal tracer with the rays of all g-points in one launch (rrx_thermal_trace_counts_spectral,
rrx_thermal_render_spectral): declared in both precisions and exported; the argument lists are those of
rrx_thermal_trace_counts and rrx_thermal_render with the changes the header names; every refusal answers without a GPU, with a
non-zero status and a message that names the entry and the argument; an extent of 0 returns 0. (ray_end is a device array for
rrx_thermal_trace_counts_spectral, which cannot look into it: a list that does not ascend is refused by the binding,
hip_kernels.thermal_trace_counts_spectral, and cannot arise in rrx_thermal_render_spectral, which forms the list itself from
m_g >= 0.)"""
import numpy as np
import pytest

import abi

TRACE, RENDER = "rrx_thermal_trace_counts_spectral", "rrx_thermal_render_spectral"
ENTRIES = (TRACE, RENDER)
SCENE = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, top_at_1=0, dx=100., dy=100., dz=50., knx=1, kny=2, knz=1, sensor_type=0, npx=3, npy=2,
             fov=1.0, seed=7, ray0=0, nrays=12, max_events=100, nchan=2)
SENSOR = (50., 60., 20., 0.5, 0., 0., 0., 0.5, 0., 0., 0., -1.)
LAST_EXTENT = {TRACE: "nrays", RENDER: "npy"}


def _call(lib, entry, sfx, null=(), **over):
    """The entry on memory that the device never touches (the checks come before any HIP call). Returns the status."""
    F = np.float64 if sfx == "_f64" else np.float32
    scene = dict(SCENE, sensor=np.array(SENSOR, dtype=F))
    if entry == RENDER:
        scene.update(top_radiance=np.array([0.5, 0.25], dtype=F), rays_per_pixel_gpt=np.array([2, 3], dtype=np.int64))
    scene = {k: v for k, v in {**scene, **over}.items() if k in abi.names(entry)}
    return abi.call(lib, entry, sfx, null=tuple(n for n in null if n in abi.names(entry)), **scene)[0]


def test_header_declares_the_entries_as_their_counterparts_with_the_named_changes():
    for entry in ENTRIES:
        assert abi.declares(entry), entry
    for sfx, F in zip(abi.SFXS, ("double", "float")):
        want = list(abi.params("rrx_thermal_trace_counts", sfx))
        want.remove(("int", "igpt"))
        at = want.index((F, "top_radiance"))
        want[at:at + 1] = [(f"const {F}*", "top_radiance"), ("const long long*", "ray_end"), (f"const {F}*", "weight0")]
        assert list(abi.params(TRACE, sfx)) == want
        want = list(abi.params("rrx_thermal_render", sfx))
        want[want.index(("long long", "rays_per_pixel"))] = ("const long long*", "rays_per_pixel_gpt")
        at = want.index(("RrxBool", "by_band"))
        want[at:at + 1] = [("int", "nchan"), (f"const {F}*", "chan_weights")]
        assert list(abi.params(RENDER, sfx)) == want
    assert max(len(abi.params(e, "_f64")) for e in ENTRIES) < 58
    # the closed set of rrx_rt_ / rrx_raytracer_ symbols does not grow: nothing thermal lies outside its own prefix
    assert not [s for s in abi.declared_symbols() if "thermal" in s and not s.startswith("rrx_thermal_")]
    text = abi.header_macro()
    for word in ("DESIGN.md 4.24", "rrx_camera_channels", "U = F(n_act) / F(P)"):
        assert word in text, word
    limits = text[text.index("rrx_thermal_render: the loop"):text.index("---- The thermal tracer with the rays of all g-points")]
    assert "LIMITS" in limits and "one g-point per launch" not in " ".join(limits.replace("\\", " ").split())


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
    sensor = lambda at: np.array([at.get(i, v) for i, v in enumerate(SENSOR)], dtype=F)
    cases = [
        # what the two entries of the per-g-point form refuse: the grid, the cloud triple, the sensor, the tracer's own arrays
        ({"nx": -1}, "nx is negative"), ({"nbnd": -1}, "nbnd is negative"), ({"dz": 0.}, "dx, dy, dz must be > 0"), ({"knx": 3}, "knx"),
        ({"knz": 0}, "knx, kny, knz must be >= 1"), ({"max_events": 0}, "max_events"),
        ({"null": ("cld_ssa",)}, "cld_tau, cld_ssa, cld_g must be all NULL or all given"),
        ({"sensor_type": 4}, "sensor_type"), ({"npx": -1}, "npx is negative"), ({"null": ("sensor",)}, "sensor is NULL"),
        ({"sensor": sensor({1: np.nan})}, "not finite"), ({"sensor": sensor({2: -1.})}, "below the surface"),
        ({"sensor": sensor({11: 0.})}, "e_d is zero"), ({"sensor_type": 1, "fov": 7.0}, "fov"),
        ({"sensor_type": 2, "sensor": sensor({11: 1.})}, "orthographic"), ({"sensor_type": 3, "sensor": sensor({11: 0.})}, "flux sensor"),
        ({"null": ("tau",)}, "tau is NULL"), ({"null": ("lay_src",)}, "lay_src is NULL"), ({"null": ("sfc_src",)}, "sfc_src is NULL"),
        ({"null": ("sfc_emis",)}, "sfc_emis is NULL"), ({"null": ("n_capped",)}, "n_capped is NULL"), ({"null": ("n_clamped",)}, "n_clamped is NULL"),
        # the spectral form's own
        ({"ngpt": 1025}, "ngpt must be <= 1024"), ({"nbnd": 0}, "nbnd must be >= 1"), ({"null": ("band_lims_gpt",)}, "band_lims_gpt is NULL"),
        ({"null": ("band_lims_gpt", "cld_tau", "cld_ssa", "cld_g")}, "band_lims_gpt is NULL"),
    ]
    if entry == TRACE:
        cases += [({"null": ("counts",)}, "counts is NULL"), ({"null": ("k_null",)}, "k_null is NULL"), ({"ray0": -1}, "ray0 is negative"),
                  ({"null": ("ray_end",)}, "ray_end is NULL"), ({"null": ("weight0",)}, "weight0 is NULL")]
    else:
        m = lambda *v: np.array(v, dtype=np.int64)
        cases += [({"null": ("radiance",)}, "radiance is NULL"), ({"top_radiance": np.array([0.5, -1.], dtype=F)}, "top_radiance"),
                  ({"top_radiance": np.array([np.inf, 1.], dtype=F)}, "top_radiance"), ({"top_radiance": np.array([np.nan, 1.], dtype=F)}, "top_radiance"),
                  ({"rays_per_pixel_gpt": m(2, -1)}, "rays_per_pixel_gpt is negative at g-point 1"),
                  ({"rays_per_pixel_gpt": m(2**62, 2**62)}, "the ray list exceeds 2^63 - 1"),
                  ({"null": ("rays_per_pixel_gpt",)}, "rays_per_pixel_gpt is NULL"), ({"nchan": 0}, "nchan must be >= 1"),
                  ({"nchan": -1}, "nchan must be >= 1"), ({"null": ("chan_weights",)}, "chan_weights is NULL")]
    for over, word in cases:
        assert _call(lib, entry, sfx, **over) != 0, over
        msg = abi.last_error(lib)
        assert msg.startswith(entry + sfx) and word in msg, (over, msg)


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_extents_return_0_and_what_may_be_null_is_not_refused(entry, sfx):
    lib = abi.lib()
    for extent in ("nx", "ny", "nz", "ngpt", "npx", "npy", LAST_EXTENT[entry]):
        assert _call(lib, entry, sfx, **{extent: 0}) == 0, extent
        # nothing is looked at behind an extent of 0
        assert _call(lib, entry, sfx, null=tuple(abi.pointers(entry)), **{extent: 0}) == 0, extent
    assert _call(lib, entry, sfx, **{LAST_EXTENT[entry]: -1}) != 0
    assert LAST_EXTENT[entry] + " is negative" in abi.last_error(lib)
    # a NULL ssa (the gas does not scatter), no cloud and a NULL top_radiance pass every check: the refusal that follows is the last
    # check's
    assert _call(lib, entry, sfx, null=("ssa", "cld_tau", "cld_ssa", "cld_g", "top_radiance"), sensor_type=4) != 0
    assert "sensor_type" in abi.last_error(lib)
