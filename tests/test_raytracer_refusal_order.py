"""The ORDER in which the ray tracers' entries refuse their arguments (CPU). For every entry that checks arguments, in both
precisions, ORDER(entry) is the list of single faults in the order in which the code reports them: the three k_null*, the three
bg_profile*, the five forward trace entries, the five forward loops, the four backward trace entries and the four backward loops, the
camera's three spectral entries and the four thermal entries. For
every pair i < j of faults that do not concern the same argument the test applies both and asserts that fault i's message comes back,
prefixed with the entry's name. The order is part of the entries' behaviour: a zero extent returns 0 before any later fault is looked
at, nbg out of range is refused before that, and with nbg = 0 nothing of the background is looked at.

Every call here carries a fault or a zero extent, so that none reaches a HIP call: the pointers are host buffers. That is why the
loops, whose background checks are their last, show "a partly NULL bg_aer triple is not looked at with nbg = 0" beside the fault that
is checked last before it (the message is that fault's, where nbg = 3 alone gives the triple's); rrx_rt_bg_profile_aer / _all show it
outright: nbg = 0 returns 0."""
import ctypes
import itertools

import numpy as np
import pytest

import abi

K_NULL = ("rrx_rt_k_null", "rrx_rt_k_null_aer", "rrx_rt_k_null_all")
BG_PROFILE = ("rrx_rt_bg_profile", "rrx_rt_bg_profile_aer", "rrx_rt_bg_profile_all")
FW_TRACE = ("rrx_rt_trace_counts", "rrx_rt_trace_counts_phase", "rrx_rt_trace_counts_bg", "rrx_rt_trace_counts_aer", "rrx_rt_trace_counts_spectral")
FW_LOOP = ("rrx_raytracer_sw", "rrx_raytracer_sw_phase", "rrx_raytracer_sw_bg", "rrx_raytracer_sw_aer", "rrx_raytracer_sw_spectral")
BW_TRACE = ("rrx_rt_bw_trace_counts", "rrx_rt_bw_trace_counts_phase", "rrx_rt_bw_trace_counts_bg", "rrx_rt_bw_trace_counts_aer")
BW_LOOP = ("rrx_raytracer_bw", "rrx_raytracer_bw_phase", "rrx_raytracer_bw_bg", "rrx_raytracer_bw_aer")
CAMERA = ("rrx_camera_trace_counts_spectral", "rrx_camera_render_spectral")
CHANNELS = ("rrx_camera_channels",)
THERMAL = ("rrx_thermal_trace_counts", "rrx_thermal_render", "rrx_thermal_trace_counts_spectral", "rrx_thermal_render_spectral")
RENDER = ("rrx_camera_render_spectral", "rrx_thermal_render", "rrx_thermal_render_spectral")          # the loops among them
ENTRIES = K_NULL + BG_PROFILE + FW_TRACE + FW_LOOP + BW_TRACE + BW_LOOP + CAMERA + CHANNELS + THERMAL
# the forward loops from _aer on take each aerosol triple as a host array of three pointers
PACKED = {"aer": ("aer_tau", "aer_ssa", "aer_g"), "bg_aer": ("bg_aer_tau", "bg_aer_ssa", "bg_aer_g")}
SCENE = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, igpt=1, top_at_1=0, independent_column=0, dx=100., dy=100., dz=50., mu0=0.5, azimuth=0.3,
             inc_dir=1., inc_dif=0., knx=1, kny=2, knz=1, sensor_type=0, npx=3, npy=2, fov=1.0, seed=7, ray0=0, nrays=12, rays_per_pixel=2,
             photon0=0, nphotons=8, photons_per_pixel=2, max_events=100, nmu=5, nre=3, re0=4.0, dre=3.0, nbg=3, npix=6, nchan=2, scale=1., by_band=0)
SENSOR = (50., 60., 20., 0.5, 0., 0., 0., 0.5, 0., 0., 0., -1.)
NAN = float("nan")


def _has(entry, name):
    return name in abi.names(entry) or any(arg in abi.names(entry) and name in PACKED[arg] for arg in PACKED)


def _array(name, F):
    """the host arrays that an entry reads, by the name of a fault's value"""
    sensor = lambda **put: np.array([put.get(n, v) for n, v in zip(("x", "y", "z", "wx", "wy", "wz", "hx", "hy", "hz", "ex", "ey", "ez"), SENSOR)], dtype=F)
    return {"dz_bg": np.array([300., 1200., 4000., 1.], dtype=F), "dz_bg_zero": np.array([300., 0., 4000., 1.], dtype=F),
            "sensor": np.array(SENSOR, dtype=F), "inc_dir": np.array([1., 2.], dtype=F), "inc_dir_negative": np.array([1., -2.], dtype=F),
            "inc_dif": np.array([0., 0.], dtype=F), "m": np.array([2, 3], dtype=np.int64), "m_negative": np.array([2, -1], dtype=np.int64),
            # (the faults of the per-g-point checks sit at g-point 1, so that their order is that of the checks of one g-point)
            "inc_dir_zero": np.array([1., 0.], dtype=F), "m_huge": np.array([2, 2**62], dtype=np.int64),
            "top": np.array([0.5, 0.25], dtype=F), "top_negative": np.array([0.5, -1.], dtype=F), "top_nan": np.array([0.5, NAN], dtype=F),
            "sensor_nan": sensor(x=NAN), "sensor_e_d_zero": sensor(ez=0.), "sensor_below": sensor(z=-1.), "sensor_e_d_long": sensor(ez=-2.),
            "sensor_e_d_level": sensor(ex=1., ez=0.)}[name]


def _call(lib, entry, sfx, faults):
    """entry + sfx on a valid scene with the faults applied: overrides by name, "null": the pointers that are NULL, a value that is a
    string: _array's. Returns (status, message)."""
    F = np.float64 if sfx == "_f64" else np.float32
    loop = entry.startswith("rrx_raytracer") or entry in RENDER
    scene = dict(SCENE, dz_bg=_array("dz_bg", F), sensor=_array("sensor", F))
    if loop:
        scene.update(inc_dir=_array("inc_dir", F), inc_dif=_array("inc_dif", F), photons_per_pixel_gpt=_array("m", F),
                     rays_per_pixel_gpt=_array("m", F), top_radiance=_array("top", F))
    null = set()
    for fault in faults:
        null |= set(fault.get("null", ()))
        scene.update({k: (_array(v, F) if isinstance(v, str) else v) for k, v in fault.items() if k != "null"})
    scene = {k: v for k, v in scene.items() if k in abi.names(entry)}
    keep = []          # (the buffers that the packed pointers point to live until the call returns)
    for arg, three in PACKED.items():
        if arg in abi.names(entry):
            keep += [None if n in null else np.zeros(4, dtype=F) for n in three]
            scene[arg] = (ctypes.c_void_p * 3)(*[None if b is None else b.ctypes.data for b in keep[-3:]])
    return abi.call(lib, entry, sfx, null=tuple(n for n in null if n in abi.names(entry)), **scene)


def _arguments(fault):
    return set(fault.get("null", ())) | (set(fault) - {"null"})


def ORDER(entry):
    """[(fault, the word of its message)] in the order in which entry reports them, read from check_entry, check_sensor, walk_bound and
    ray_list of csrc/rrx_rt_host.h, the entries' own checks in csrc/rrx_raytracer.hip, csrc/rrx_raytracer_bw.hip and
    csrc/rrx_raytracer_thermal.hip, and the checks of csrc/rrx_rt_common.h, csrc/rrx_rt_phase.h"""
    has = lambda name: _has(entry, name)
    null = lambda name: {"null": (name,)}
    all_gpt = entry.endswith("_all") or entry.endswith("_spectral")
    order = []
    add = lambda fault, word, when=True: order.append((fault, word)) if when and all(has(a) for a in _arguments(fault)) else None
    if entry in K_NULL:
        add({"nx": -1}, "nx is negative"); add({"ngpt": -1}, "ngpt is negative"); add({"nbnd": -1}, "nbnd is negative")
        add({"ngpt": 1025}, "ngpt must be <= 1024", all_gpt)
        add(null("tau"), "tau is NULL"); add(null("k_null"), "k_null is NULL"); add(null("band_lims_gpt"), "band_lims_gpt is NULL")
        add({"nbnd": 0}, "nbnd must be >= 1 with an aerosol triple", has("aer_tau"))
        add({"igpt": 9}, "igpt is outside"); add({"dz": 0.}, "dz must be > 0")
        add({"knx": 3}, "knx does not divide nx"); add({"knz": 3}, "knz does not divide nz")
        return order
    if entry in BG_PROFILE:
        add({"nbg": -1}, "nbg is negative"); add({"nbg": 257}, "nbg must be <= 256")
        add({"ngpt": -1}, "ngpt is negative"); add({"nbnd": -1}, "nbnd is negative")
        add({"igpt": 9}, "igpt is outside"); add({"ngpt": 1025}, "ngpt must be <= 1024", all_gpt)
        add(null("dz_bg"), "dz_bg is NULL"); add(null("bg_tau"), "bg_tau is NULL"); add(null("bg_ssa"), "bg_ssa is NULL")
        add(null("bg_cld_ssa"), "bg_cld_tau, bg_cld_ssa, bg_cld_g must be all NULL or all given")
        add(null("band_lims_gpt"), "band_lims_gpt is NULL"); add({"nbnd": 0}, "nbnd must be >= 1 with a background cloud triple")
        add(null("bg_aer_g"), "bg_aer_tau, bg_aer_ssa, bg_aer_g must be all NULL or all given")
        add(null("bg_profile"), "bg_profile is NULL"); add({"dz_bg": "dz_bg_zero"}, "dz_bg must be > 0")
        return order
    if entry in CHANNELS:
        add({"npix": -1}, "npix is negative")
        for n in (0, -1):
            add({"nbnd": n}, "nbnd must be >= 1: the counts are kept by band")
        for n in (0, -1):
            add({"nchan": n}, "nchan must be >= 1")
        add({"npix": 2**31}, "npix exceeds 2^31 - 1"); add({"npix": 2**31 - 1, "nchan": 257}, "nchan npix exceeds 2^39")
        add(null("counts"), "counts is NULL"); add(null("chan_weights"), "chan_weights is NULL"); add(null("out"), "out is NULL")
        return order
    # the trace entries and the loops of the three tracers
    loop, backward, thermal = entry in FW_LOOP + BW_LOOP + RENDER, entry in BW_TRACE + BW_LOOP + CAMERA + THERMAL, entry in THERMAL
    by_band = entry in CAMERA + THERMAL and all_gpt          # the entries whose counts are kept by band, whatever the clouds
    add({"nbg": -1}, "nbg is negative"); add({"nbg": 257}, "nbg must be <= 256")
    add({"nx": -1}, "nx is negative"); add({"ngpt": -1}, "ngpt is negative", not loop or entry in RENDER)
    add({"npy": -1}, "npy is negative")
    for work in ("nphotons", "photons_per_pixel", "nrays", "rays_per_pixel"):
        add({work: -1}, work + " is negative")
    add({"nbnd": -1}, "nbnd is negative")
    add({"ngpt": 1025}, "ngpt must be <= 1024", all_gpt)
    add({"by_band": 1, "null": ("band_lims_gpt",)}, "band_lims_gpt is NULL"); add({"by_band": 1, "nbnd": 0}, "nbnd must be >= 1: the radiances are kept by band")
    add({"nbnd": 0}, "nbnd must be >= 1: the counts are kept by band", by_band); add({"nchan": 0}, "nchan must be >= 1")
    add({"photon0": -1}, "photon0 is negative"); add({"ray0": -1}, "ray0 is negative")
    # the thermal entries' own names come first; their ssa may be NULL
    for name in (("tau", "sfc_emis", "lay_src", "sfc_src") if thermal else ("tau", "ssa", "sfc_albedo")) + ("photon_end", "dif_frac") \
              + (("band_lims_gpt", "ray_end", "weight0") if by_band else ()) \
              + (("inc_dir", "inc_dif", "photons_per_pixel_gpt", "rays_per_pixel_gpt", "chan_weights") if loop else ()) \
              + ("k_null", "sensor", "sfc_dn_dir", "abs_dif", "counts", "radiance", "n_capped", "n_clamped"):
        add(null(name), name + " is NULL", name != "k_null" or not loop)
    add(null("cld_ssa"), "cld_tau, cld_ssa, cld_g must be all NULL or all given")
    # (where by_band is an argument the fault names it: with by_band = 1 the table is asked for earlier, above)
    add(dict(null("band_lims_gpt"), **({"by_band": 0} if has("by_band") else {})), "band_lims_gpt is NULL", not by_band); add({"nbnd": 0}, "nbnd must be >= 1 with a cloud triple", not by_band)
    add(null("aer_ssa"), "aer_tau, aer_ssa, aer_g must be all NULL or all given")
    add(null("cdf"), "mu, phase, cdf, cld_re must be all NULL or all given"); add({"nmu": 1}, "nmu must be >= 2")
    add({"igpt": 9}, "igpt is outside")
    add({"dx": 0.}, "dx, dy, dz must be > 0"); add({"mu0": 0.}, "mu0 must be in (0, 1]")
    too_many_pixels = ({"npx": 65536, "npy": 65536}, "npx npy exceeds 2^31 - 1")          # (the spectral loops need npix for their ray list)
    add(*too_many_pixels, by_band and loop)
    if loop:
        for value in ("top_negative", "top_nan"):
            add({"top_radiance": value}, "top_radiance must be finite and >= 0")
        add({"inc_dir": "inc_dir_negative"}, "inc_dir must be >= 0" if backward else "inc_dir, inc_dif must be >= 0")
        add({"photons_per_pixel_gpt": "m_negative"}, "photons_per_pixel_gpt is negative at g-point 1")
        add({"rays_per_pixel_gpt": "m_negative"}, "rays_per_pixel_gpt is negative at g-point 1")
        add({"inc_dir": "inc_dir_zero"}, "rays_per_pixel_gpt is > 0 at g-point 1, which has no incident flux", has("rays_per_pixel_gpt"))
        add({"rays_per_pixel_gpt": "m_huge"}, "the ray list exceeds 2^63 - 1")
    else:
        add({"inc_dir": -1.}, "inc_dir, inc_dif must be >= 0 with a positive sum")
        for value in (-1., NAN):
            add({"top_radiance": value}, "top_radiance must be finite and >= 0", entry == "rrx_thermal_trace_counts")
    add({"max_events": 0}, "max_events must be >= 1")
    add({"knx": 3}, "knx does not divide nx"); add({"knz": 3}, "knz does not divide nz")
    add(*too_many_pixels, not (by_band and loop)); add({"sensor_type": 7}, "sensor_type must be")
    add({"sensor": "sensor_nan"}, "sensor holds a number that is not finite"); add({"sensor": "sensor_e_d_zero"}, "sensor e_d is zero")
    add({"sensor": "sensor_below"}, "sensor position lies below the surface")
    add({"sensor_type": 1, "fov": 0.}, "fov must be in (0, 2 pi] for a fisheye sensor")
    add({"sensor_type": 2, "sensor": "sensor_e_d_long"}, "sensor e_d must be a unit vector with e_d.z < 0 for an orthographic sensor")
    add({"sensor_type": 3, "sensor": "sensor_e_d_level"}, "sensor e_d.z must be > 0")
    add({"mu0": 1.e-12}, "mu0 is too small for this domain", backward)
    if loop:
        add(null("bg_aer_g"), "bg_aer_tau, bg_aer_ssa, bg_aer_g must be all NULL or all given")
        add(null("dz_bg"), "dz_bg is NULL"); add(null("bg_ssa"), "bg_ssa is NULL")
        add(null("bg_cld_g"), "bg_cld_tau, bg_cld_ssa, bg_cld_g must be all NULL or all given")
    else:
        add(null("dz_bg"), "dz_bg is NULL"); add(null("bg_profile"), "bg_profile is NULL")
    add(null("toa_up"), "toa_up is NULL"); add(null("bg_abs_dif"), "bg_abs_dif is NULL")
    add({"dz_bg": "dz_bg_zero"}, "dz_bg must be > 0")
    return order


def test_every_entry_that_checks_arguments_is_listed():
    checked = {n[:-4] for n in abi.declared_symbols() if n.endswith("_f64") and n.startswith(("rrx_rt_", "rrx_raytracer_", "rrx_camera_", "rrx_thermal_"))}
    unlisted = checked - set(ENTRIES) - {"rrx_rt_counts_to_flux", "rrx_rt_phase_tables", "rrx_rt_phase_sample", "rrx_rt_phase_eval"}
    assert not unlisted, unlisted
    assert all(abi.declares(e) for e in ENTRIES) and len(ENTRIES) == 31
    assert all(len(ORDER(e)) >= 10 for e in ENTRIES), {e: len(ORDER(e)) for e in ENTRIES}


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_of_two_faults_the_one_that_is_checked_first_is_reported(entry, sfx):
    lib = abi.lib()
    order = ORDER(entry)
    for fault, word in order:          # (each fault alone gives its message)
        status, msg = _call(lib, entry, sfx, [fault])
        assert status != 0 and msg.startswith(entry + sfx + ": ") and word in msg, (fault, msg)
    pairs = list(itertools.combinations(order, 2))
    tried = 0
    for (first, word), (second, _) in pairs:
        if _arguments(first) & _arguments(second):
            continue
        tried += 1
        status, msg = _call(lib, entry, sfx, [second, first])
        assert status != 0 and msg.startswith(entry + sfx + ": ") and word in msg, (first, second, msg)
    assert 4*tried >= 3*len(pairs), (tried, len(pairs))


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_zero_extent_returns_zero_before_any_later_fault_and_nbg_is_refused_before_it(entry, sfx):
    lib = abi.lib()
    order = ORDER(entry)
    extent = "ngpt" if entry in BG_PROFILE else "npix" if entry in CHANNELS else "nz"
    later = [f for f, w in order if "negative" not in w and "nbg" not in f and extent not in f]
    assert len(later) >= 6
    for fault in later:
        assert _call(lib, entry, sfx, [fault, {extent: 0}])[0] == 0, fault
    if _has(entry, "nbg"):
        for nbg, word in ((-1, "nbg is negative"), (257, "nbg must be <= 256")):
            status, msg = _call(lib, entry, sfx, [{extent: 0, "nbg": nbg}])
            assert status != 0 and msg.startswith(entry + sfx + ": ") and word in msg, msg


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", [e for e in ENTRIES if _has(e, "bg_aer_g")])
def test_without_layers_a_partly_null_background_aerosol_triple_is_not_looked_at(entry, sfx):
    lib = abi.lib()
    partly, word = {"null": ("bg_aer_g",)}, "bg_aer_tau, bg_aer_ssa, bg_aer_g"
    status, msg = _call(lib, entry, sfx, [partly])
    assert status != 0 and word in msg, msg
    if entry in BG_PROFILE:
        assert _call(lib, entry, sfx, [partly, {"nbg": 0}])[0] == 0
        return
    # the loops: the last fault that is checked before the background's; with nbg = 0 nothing follows it
    last = {"sensor_type": 7} if entry in BW_LOOP + CAMERA else {"knz": 3}
    for nbg in (0, 3):
        status, msg = _call(lib, entry, sfx, [partly, last, {"nbg": nbg}])
        assert status != 0 and word not in msg and ("sensor_type" in msg or "knz" in msg), msg
    # and the whole background may be NULL then
    nothing = {"null": ("bg_aer_g", "bg_aer_tau", "dz_bg", "bg_tau", "bg_ssa", "toa_up", "bg_abs_dir")}
    status, msg = _call(lib, entry, sfx, [nothing, last, {"nbg": 0}])
    assert status != 0 and ("sensor_type" in msg or "knz" in msg), msg
