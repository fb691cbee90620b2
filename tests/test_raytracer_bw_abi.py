"""CPU tests of the backward ray tracer entries (rrx_rt_bw_trace_counts, rrx_raytracer_bw): declared in both precisions with the
stream last and exported, their argument checks answer without a GPU and name the argument, and the host libraries export
Raytracer_bw_gpu::trace_rays_bw and rrx_cxx_trace_rays_bw."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrx_hip.h")
LIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librrx_hip.so")
HOSTLIBS = [os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", n) for n in ("librte_rrtmgp_hip.so", "librte_rrtmgp_hip_sp.so")]
ENTRIES = ("rrx_rt_bw_trace_counts", "rrx_raytracer_bw")
NULL = ctypes.c_void_p(0)


def _lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    lib.rrx_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_the_entries_in_both_precisions_with_the_stream_last():
    text = open(HEADER).read()
    macro = text[text.index("#define RRX_DECLARE"):text.index("RRX_DECLARE(double")]
    for name in ENTRIES:
        m = re.search(r"\bint " + name + r"##SFX\s*\(([^;]*)\);", macro)
        assert m, name
        args = m.group(1).replace("\\", "")
        assert re.search(r"void\*\s*stream\s*$", args.strip()), name
        for piece in ("int sensor_type", "int npx", "int npy", "F fov", "const F* sensor", "unsigned long long seed", "int max_events",
                      "unsigned long long* n_capped", "unsigned long long* n_clamped"):
            assert piece in args, (name, piece)
    m = re.search(r"\bint rrx_rt_bw_trace_counts##SFX\s*\(([^;]*)\);", macro).group(1)
    for piece in ("const F* k_null", "long long ray0", "long long nrays", "unsigned long long* counts"):
        assert piece in m, piece


def test_library_exports_the_entries():
    lib = _lib()
    for name in ENTRIES:
        for sfx in ("_f64", "_f32"):
            assert hasattr(lib, name + sfx), name + sfx


def _args(entry, sfx, **over):
    """The argument list of an entry on host memory that is never touched: the checks come before any HIP call."""
    F = ctypes.c_double if sfx == "_f64" else ctypes.c_float
    buf = lambda: ctypes.cast((F * 64)(), ctypes.c_void_p)
    cnt = lambda: ctypes.cast((ctypes.c_ulonglong * 64)(), ctypes.c_void_p)
    a = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, igpt=1, top_at_1=ctypes.c_byte(0), tau=buf(), ssa=buf(),
             band_lims=ctypes.cast((ctypes.c_int * 2)(1, 2), ctypes.c_void_p), cld_tau=buf(), cld_ssa=buf(), cld_g=buf(),
             dx=F(100.), dy=F(100.), dz=F(50.), sfc_albedo=buf(), mu0=F(0.5), azimuth=F(0.3),
             inc_dir=ctypes.cast((F * 2)(1., 2.), ctypes.c_void_p), knx=1, kny=2, knz=1, k_null=buf(),
             sensor_type=0, npx=3, npy=2, fov=F(1.0), sensor_numbers=(50., 60., 20., 0.5, 0., 0., 0., 0.5, 0., 0., 0., -1.),
             seed=ctypes.c_ulonglong(7), ray0=0, nrays=12, rays_per_pixel=2, max_events=100,
             counts=cnt(), radiance=buf(), n_capped=cnt(), n_clamped=cnt())
    a.update(over)
    if "sensor" not in a:
        a["sensor"] = ctypes.cast((F * 12)(*a["sensor_numbers"]), ctypes.c_void_p)
    L = ctypes.c_longlong
    scene = [a["tau"], a["ssa"], a["band_lims"], a["cld_tau"], a["cld_ssa"], a["cld_g"], a["dx"], a["dy"], a["dz"], a["sfc_albedo"],
             a["mu0"], a["azimuth"]]
    sensor = [a["sensor_type"], a["npx"], a["npy"], a["fov"], a["sensor"]]
    if entry == "rrx_rt_bw_trace_counts":
        return [a["nx"], a["ny"], a["nz"], a["ngpt"], a["nbnd"], a["igpt"], a["top_at_1"]] + scene + \
               [a["knx"], a["kny"], a["knz"], a["k_null"]] + sensor + [a["seed"], L(a["ray0"]), L(a["nrays"]), a["max_events"],
                                                                      a["counts"], a["n_capped"], a["n_clamped"], NULL]
    return [a["nx"], a["ny"], a["nz"], a["ngpt"], a["nbnd"], a["top_at_1"]] + scene + [a["inc_dir"], a["knx"], a["kny"], a["knz"]] + sensor + \
           [L(a["rays_per_pixel"]), a["seed"], a["max_events"], a["radiance"], a["n_capped"], a["n_clamped"], NULL]


def _call(lib, entry, sfx, **over):
    fn = getattr(lib, entry + sfx)
    fn.restype = ctypes.c_int
    return fn(*_args(entry, sfx, **over))


NEEDED = {"rrx_rt_bw_trace_counts": ("tau", "ssa", "sfc_albedo", "k_null", "sensor", "counts", "n_capped", "n_clamped"),
          "rrx_raytracer_bw": ("tau", "ssa", "sfc_albedo", "inc_dir", "sensor", "radiance", "n_capped", "n_clamped")}
EXTENTS = {"rrx_rt_bw_trace_counts": ("nx", "ny", "nz", "ngpt", "npx", "npy", "nrays"),
           "rrx_raytracer_bw": ("nx", "ny", "nz", "ngpt", "npx", "npy", "rays_per_pixel")}


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_null_that_is_needed_is_refused_without_a_gpu(entry, sfx):
    lib = _lib()
    for name in NEEDED[entry]:
        assert _call(lib, entry, sfx, **{name: NULL}) != 0, name
        msg = lib.rrx_last_error().decode()
        assert entry + sfx in msg and name + " is NULL" in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_extents_return_zero_without_a_launch_and_negative_ones_are_refused(entry, sfx):
    lib = _lib()
    for d in EXTENTS[entry]:
        assert _call(lib, entry, sfx, **{d: 0}) == 0, d
        assert _call(lib, entry, sfx, **{d: 0, "tau": NULL, "counts": NULL, "radiance": NULL}) == 0, d
        assert _call(lib, entry, sfx, **{d: -1}) != 0, d
        msg = lib.rrx_last_error().decode()
        assert entry + sfx in msg and d + " is negative" in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_scene_and_sensor_checks_name_the_argument(entry, sfx):
    lib = _lib()
    F = ctypes.c_double if sfx == "_f64" else ctypes.c_float
    look = (50., 60., 20., 0.5, 0., 0., 0., 0.5, 0.)
    for over, word in (({"mu0": F(0.)}, "mu0"), ({"mu0": F(-0.2)}, "mu0"), ({"dz": F(0.)}, "dz"), ({"knx": 3}, "knx"), ({"knz": 0}, "knz"),
                       ({"cld_ssa": NULL}, "cld_tau, cld_ssa, cld_g"), ({"band_lims": NULL}, "band_lims_gpt"), ({"max_events": 0}, "max_events"),
                       ({"sensor_type": 4}, "sensor_type"), ({"sensor_type": -1}, "sensor_type"),
                       ({"sensor_numbers": look + (0., 0., 0.)}, "e_d"),
                       ({"sensor_numbers": (50., 60., -1.) + look[3:] + (0., 0., -1.)}, "position"),
                       ({"sensor_numbers": look + (0., float("nan"), -1.)}, "not finite"),
                       ({"sensor_type": 1, "fov": F(0.)}, "fov"), ({"sensor_type": 1, "fov": F(7.)}, "fov"),
                       ({"sensor_type": 2, "sensor_numbers": look + (0., 0., 1.)}, "e_d"),
                       ({"sensor_type": 2, "sensor_numbers": look + (0., 0., -2.)}, "e_d"),
                       ({"sensor_type": 3, "sensor_numbers": look + (1., 0., 0.)}, "e_d.z")):
        assert _call(lib, entry, sfx, **over) != 0, over
        msg = lib.rrx_last_error().decode()
        assert entry + sfx in msg and word in msg, msg
    # a clear sky: the whole triple NULL is accepted as far as the argument checks go (no rays: no launch)
    assert _call(lib, entry, sfx, cld_tau=NULL, cld_ssa=NULL, cld_g=NULL, band_lims=NULL, nrays=0, rays_per_pixel=0) == 0
    if entry == "rrx_rt_bw_trace_counts":
        assert _call(lib, entry, sfx, igpt=2) != 0 and "igpt" in lib.rrx_last_error().decode()
        assert _call(lib, entry, sfx, ray0=-1) != 0 and "ray0" in lib.rrx_last_error().decode()
    else:
        assert _call(lib, entry, sfx, inc_dir=ctypes.cast((F * 2)(1., -2.), ctypes.c_void_p)) != 0 and "inc_dir" in lib.rrx_last_error().decode()


def test_host_libraries_export_the_backward_raytracer_class():
    text = open(os.path.join(ROOT, "include", "Raytracer_bw.h")).read()
    assert "class Raytracer_bw_gpu" in text and "trace_rays_bw(" in text
    assert "rrx_cxx_trace_rays_bw(" in open(os.path.join(ROOT, "include_test", "rrx_cxx_driver.h")).read()
    for hostlib in HOSTLIBS:
        if not os.path.exists(hostlib):
            pytest.fail(f"{hostlib} not built: run __graft_entry__.build()")
        syms = subprocess.run(["nm", "-DC", "--defined-only", hostlib], capture_output=True, text=True).stdout
        assert "Raytracer_bw_gpu::trace_rays_bw(" in syms and "rrx_cxx_trace_rays_bw" in syms, hostlib
