"""CPU tests of the entries of the thermal tracer's cell sensors (rrx_heating3d_counts, rrx_heating3d_counts_spectral,
rrx_heating3d_render): declared in both precisions and exported; the argument lists are those of the thermal
trace entries without the sensor, with signed counts; every refusal answers without a GPU, with a non-zero status and a message
that names the entry and the argument; an extent of 0 returns 0."""
import numpy as np
import pytest

import abi

COUNTS, SPECTRAL, RENDER = "rrx_heating3d_counts", "rrx_heating3d_counts_spectral", "rrx_heating3d_render"
ENTRIES = (COUNTS, SPECTRAL, RENDER)
SCENE = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, igpt=1, top_at_1=0, dx=100., dy=100., dz=50., top_radiance=0.5, knx=1, kny=2, knz=1,
             seed=7, ray0=0, nrays=16, max_events=100)
SENSOR = ("sensor_type", "npx", "npy", "fov", "sensor")
LAST_EXTENT = {COUNTS: "nrays", SPECTRAL: "nrays", RENDER: "ngpt"}


def _call(lib, entry, sfx, null=(), **over):
    """The entry on memory that the device never touches (the checks come before any HIP call). Returns the status."""
    F = np.float64 if sfx == "_f64" else np.float32
    scene = dict(SCENE)
    if entry != COUNTS:
        scene["top_radiance"] = np.array([0.5, 0.25], dtype=F)
    if entry == RENDER:
        scene["rays_per_cell_gpt"] = np.array([2, 3], dtype=np.int64)
    scene = {k: v for k, v in {**scene, **over}.items() if k in abi.names(entry)}
    return abi.call(lib, entry, sfx, null=tuple(n for n in null if n in abi.names(entry)), **scene)[0]


def test_header_declares_the_entries_as_the_thermal_ones_without_the_sensor():
    for entry in ENTRIES:
        assert abi.declares(entry), entry
    for sfx, F in zip(abi.SFXS, ("double", "float")):
        for entry, twin in ((COUNTS, "rrx_thermal_trace_counts"), (SPECTRAL, "rrx_thermal_trace_counts_spectral")):
            want = [p for p in abi.params(twin, sfx) if p[1] not in SENSOR]
            want[want.index(("unsigned long long*", "counts"))] = ("long long*", "counts")
            assert list(abi.params(entry, sfx)) == want, entry
        want = [p for p in abi.params("rrx_thermal_render_spectral", sfx) if p[1] not in SENSOR + ("nchan", "chan_weights")]
        want[want.index(("const long long*", "rays_per_pixel_gpt"))] = ("const long long*", "rays_per_cell_gpt")
        want[want.index((f"{F}*", "radiance"))] = (f"{F}*", "flux_conv")
        assert list(abi.params(RENDER, sfx)) == want
    # nothing thermal lies outside its own prefix
    assert not [s for s in abi.declared_symbols() if "thermal" in s and not s.startswith("rrx_thermal_")]
    assert sorted(s[:-4] for s in abi.declared_symbols() if s.startswith("rrx_heating3d_") and s.endswith("_f64")) == sorted(ENTRIES)
    text = abi.header_macro()
    new = text[text.index("---- 3-D longwave heating from cell sensors"):]
    for word in ("DESIGN.md 4.25", "0x40000000", "SIGNED 64-bit", "W m-2", "U = F(n_act) / F(P)", "LIMITS", "integer atomic"):
        assert word in new, word
    # the section stands below the two thermal sections
    assert text.index("---- 3-D longwave heating from cell sensors") > text.index("rrx_thermal_render_spectral##SFX")


def test_library_exports_the_entries_and_they_bind():
    lib = abi.lib()
    for name in ENTRIES:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx
            assert len(lib.converters(name + sfx)) == len(abi.params(name, sfx))
    counts = lib.converters(COUNTS + "_f64")[abi.names(COUNTS).index("counts")]
    assert counts(np.zeros(4, dtype=np.int64))
    with pytest.raises(TypeError):
        counts(np.zeros(4, dtype=np.float64))


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_entries_refuse_without_a_gpu(entry, sfx):
    lib = abi.lib()
    F = np.float64 if sfx == "_f64" else np.float32
    cases = [
        # what the thermal entries refuse of grid, cloud triple and sources
        ({"nx": -1}, "nx is negative"), ({"nbnd": -1}, "nbnd is negative"), ({"dz": 0.}, "dx, dy, dz must be > 0"), ({"knx": 3}, "knx"),
        ({"knz": 0}, "knx, kny, knz must be >= 1"), ({"max_events": 0}, "max_events"),
        ({"null": ("cld_ssa",)}, "cld_tau, cld_ssa, cld_g must be all NULL or all given"),
        ({"null": ("band_lims_gpt",)}, "band_lims_gpt is NULL"), ({"nbnd": 0}, "nbnd must be >= 1 with a cloud triple"),
        ({"null": ("tau",)}, "tau is NULL"), ({"null": ("lay_src",)}, "lay_src is NULL"), ({"null": ("sfc_src",)}, "sfc_src is NULL"),
        ({"null": ("sfc_emis",)}, "sfc_emis is NULL"), ({"null": ("n_capped",)}, "n_capped is NULL"), ({"null": ("n_clamped",)}, "n_clamped is NULL"),
    ]
    if entry == COUNTS:
        cases += [({"igpt": 2}, "igpt is outside"), ({"igpt": -1}, "igpt is outside"), ({"top_radiance": -1.}, "top_radiance"),
                  ({"top_radiance": float("inf")}, "top_radiance"), ({"top_radiance": float("nan")}, "top_radiance")]
    else:
        # the spectral forms' own
        cases += [({"ngpt": 1025}, "ngpt must be <= 1024"),
                  ({"null": ("band_lims_gpt", "cld_tau", "cld_ssa", "cld_g")}, "band_lims_gpt is NULL")]
    if entry != RENDER:
        cases += [({"null": ("counts",)}, "counts is NULL"), ({"null": ("k_null",)}, "k_null is NULL"), ({"ray0": -1}, "ray0 is negative")]
    if entry == SPECTRAL:
        cases += [({"null": ("ray_end",)}, "ray_end is NULL"), ({"null": ("weight0",)}, "weight0 is NULL")]
    if entry == RENDER:
        m = lambda *v: np.array(v, dtype=np.int64)
        cases += [({"null": ("flux_conv",)}, "flux_conv is NULL"), ({"top_radiance": np.array([0.5, -1.], dtype=F)}, "top_radiance"),
                  ({"top_radiance": np.array([np.inf, 1.], dtype=F)}, "top_radiance"), ({"top_radiance": np.array([np.nan, 1.], dtype=F)}, "top_radiance"),
                  ({"rays_per_cell_gpt": m(2, -1)}, "rays_per_cell_gpt is negative at g-point 1"), ({"rays_per_cell_gpt": m(2**62, 2**62)}, "the ray list exceeds 2^63 - 1"),
                  ({"null": ("rays_per_cell_gpt",)}, "rays_per_cell_gpt is NULL")]
    for over, word in cases:
        assert _call(lib, entry, sfx, **over) != 0, over
        msg = abi.last_error(lib)
        assert msg.startswith(entry + sfx) and word in msg, (over, msg)


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_extents_return_0_and_what_may_be_null_is_not_refused(entry, sfx):
    lib = abi.lib()
    for extent in {"nx", "ny", "nz", "ngpt", LAST_EXTENT[entry]}:
        assert _call(lib, entry, sfx, **{extent: 0}) == 0, extent
        # nothing is looked at behind an extent of 0
        assert _call(lib, entry, sfx, null=tuple(abi.pointers(entry)), **{extent: 0}) == 0, extent
    assert _call(lib, entry, sfx, **{LAST_EXTENT[entry]: -1}) != 0
    assert LAST_EXTENT[entry] + " is negative" in abi.last_error(lib)
    # a NULL ssa (the gas does not scatter), no cloud and a NULL top_radiance of the forms that take an array pass every check: the
    # refusal that follows is the last check's
    may_be_null = ("ssa", "cld_tau", "cld_ssa", "cld_g") + (("band_lims_gpt",) if entry == COUNTS else ("top_radiance",))
    assert _call(lib, entry, sfx, null=may_be_null, knx=3) != 0
    assert "knx does not divide nx" in abi.last_error(lib)
