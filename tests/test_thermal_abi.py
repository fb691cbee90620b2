"""CPU tests of the thermal ray tracer's entries (rrx_thermal_trace_counts, rrx_thermal_render): declared in both precisions
and exported; the argument list is that of the backward entries with the sources in place of the sun; every refusal answers without
a GPU, with a non-zero status and a message that names the entry and the argument; an extent of 0 returns 0."""
import numpy as np
import pytest

import abi

TRACE, RENDER = "rrx_thermal_trace_counts", "rrx_thermal_render"
ENTRIES = (TRACE, RENDER)
SCENE = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, igpt=1, top_at_1=0, dx=100., dy=100., dz=50., top_radiance=0.5, knx=1, kny=2, knz=1,
             sensor_type=0, npx=3, npy=2, fov=1.0, seed=7, ray0=0, nrays=12, rays_per_pixel=2, max_events=100, by_band=0)
SENSOR = (50., 60., 20., 0.5, 0., 0., 0., 0.5, 0., 0., 0., -1.)
LAST_EXTENT = {TRACE: "nrays", RENDER: "rays_per_pixel"}


def _call(lib, entry, sfx, null=(), **over):
    """The entry on memory that the device never touches (the checks come before any HIP call). Returns the status."""
    F = np.float64 if sfx == "_f64" else np.float32
    scene = dict(SCENE, sensor=np.array(SENSOR, dtype=F))
    if entry == RENDER:
        scene["top_radiance"] = np.array([0.5, 0.25], dtype=F)
    scene = {k: v for k, v in {**scene, **over}.items() if k in abi.names(entry)}
    return abi.call(lib, entry, sfx, null=tuple(n for n in null if n in abi.names(entry)), **scene)[0]


def test_header_declares_the_entries_beside_the_backward_ones():
    for entry in ENTRIES:
        assert abi.declares(entry), entry
    for sfx, F in zip(abi.SFXS, ("double", "float")):
        bw = list(abi.params("rrx_rt_bw_trace_counts", sfx))
        sun = bw.index((F, "mu0"))
        assert bw[sun - 1] == (f"const {F}*", "sfc_albedo") and bw[sun + 1] == (F, "azimuth")
        want = bw[:sun - 1] + [(f"const {F}*", "sfc_emis"), (f"const {F}*", "lay_src"), (f"const {F}*", "sfc_src"), (F, "top_radiance")] + bw[sun + 2:]
        assert list(abi.params(TRACE, sfx)) == want
        names = abi.names(RENDER, sfx)
        assert names[-1] == "stream" and names[-5:-1] == ["by_band", "radiance", "n_capped", "n_clamped"]
        assert dict((n, t) for t, n in abi.params(RENDER, sfx))["top_radiance"] == f"const {F}*"
        assert not {"mu0", "azimuth", "sfc_albedo", "igpt", "k_null"} & set(names)
    # the closed set of rrx_rt_ / rrx_raytracer_ symbols does not grow
    assert not [s for s in abi.declared_symbols() if "thermal" in s and not s.startswith("rrx_thermal_")]
    text = abi.header_macro()
    for word in ("0xC0000000", "W m-2 sr-1", "LIMITS", "top_radiance"):
        assert word in text, word


def test_library_exports_the_entries():
    lib = abi.lib()
    for name in ENTRIES:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_entries_refuse_without_a_gpu(entry, sfx):
    lib = abi.lib()
    F = np.float64 if sfx == "_f64" else np.float32
    sensor = lambda at: np.array([at.get(i, v) for i, v in enumerate(SENSOR)], dtype=F)
    cld = ("cld_tau", "cld_ssa", "cld_g")
    cases = [
        # the grid and the cloud triple, as the backward entries refuse them
        ({"nx": -1}, "nx is negative"), ({"nbnd": -1}, "nbnd is negative"), ({"dz": 0.}, "dx, dy, dz must be > 0"), ({"knx": 3}, "knx"),
        ({"knz": 0}, "knx, kny, knz must be >= 1"), ({"max_events": 0}, "max_events"),
        ({"null": ("cld_ssa",)}, "cld_tau, cld_ssa, cld_g must be all NULL or all given"), ({"null": ("band_lims_gpt",)}, "band_lims_gpt is NULL"),
        ({"nbnd": 0}, "nbnd must be >= 1 with a cloud triple"),
        # the sensor
        ({"sensor_type": 4}, "sensor_type"), ({"npx": -1}, "npx is negative"), ({"null": ("sensor",)}, "sensor is NULL"),
        ({"sensor": sensor({1: np.nan})}, "not finite"), ({"sensor": sensor({2: -1.})}, "below the surface"),
        ({"sensor": sensor({11: 0.})}, "e_d is zero"), ({"sensor_type": 1, "fov": 7.0}, "fov"),
        ({"sensor_type": 2, "sensor": sensor({11: 1.})}, "orthographic"), ({"sensor_type": 3, "sensor": sensor({11: 0.})}, "flux sensor"),
        # what the tracer needs of its own
        ({"null": ("tau",)}, "tau is NULL"), ({"null": ("lay_src",)}, "lay_src is NULL"), ({"null": ("sfc_src",)}, "sfc_src is NULL"),
        ({"null": ("sfc_emis",)}, "sfc_emis is NULL"), ({"null": ("n_capped",)}, "n_capped is NULL"), ({"null": ("n_clamped",)}, "n_clamped is NULL"),
    ]
    if entry == TRACE:
        cases += [({"null": ("counts",)}, "counts is NULL"), ({"null": ("k_null",)}, "k_null is NULL"), ({"igpt": 2}, "igpt is outside"),
                  ({"ray0": -1}, "ray0 is negative"), ({"top_radiance": -1.}, "top_radiance"), ({"top_radiance": float("inf")}, "top_radiance"),
                  ({"top_radiance": float("nan")}, "top_radiance")]
    else:
        cases += [({"null": ("radiance",)}, "radiance is NULL"), ({"top_radiance": np.array([0.5, -1.], dtype=F)}, "top_radiance"),
                  ({"top_radiance": np.array([np.inf, 1.], dtype=F)}, "top_radiance"),
                  ({"by_band": 1, "null": cld + ("band_lims_gpt",)}, "band_lims_gpt is NULL"), ({"by_band": 1, "nbnd": 0, "null": cld}, "nbnd must be >= 1")]
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
    # a NULL ssa (the gas does not scatter), no cloud, and the loop's NULL top_radiance pass every check: the refusal that follows is
    # the last check's
    may_be_null = ("ssa", "band_lims_gpt", "cld_tau", "cld_ssa", "cld_g") + (("top_radiance",) if entry == RENDER else ())
    assert _call(lib, entry, sfx, null=may_be_null, sensor_type=4) != 0
    assert "sensor_type" in abi.last_error(lib)
