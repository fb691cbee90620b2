"""CPU tests of the ray tracer entries (rrx_rt_k_null, rrx_rt_trace_counts, rrx_rt_counts_to_flux, rrx_raytracer_sw): declared in
both precisions with the stream last and exported, their argument checks answer without a GPU, and the host library exports
Raytracer_gpu::trace_rays."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrx_hip.h")
LIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librrx_hip.so")
HOSTLIBS = [os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", n) for n in ("librte_rrtmgp_hip.so", "librte_rrtmgp_hip_sp.so")]
ENTRIES = ("rrx_rt_k_null", "rrx_rt_trace_counts", "rrx_rt_counts_to_flux", "rrx_raytracer_sw")
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
        assert re.search(r"void\*\s*stream\s*$", m.group(1).replace("\\", "").strip()), name
    m = re.search(r"\bint rrx_rt_trace_counts##SFX\s*\(([^;]*)\);", macro).group(1)
    for piece in ("unsigned long long seed", "long long photon0", "long long nphotons", "int max_events", "unsigned long long* n_capped"):
        assert piece in m, piece
    assert "RRX_DECLARE(double, _f64)" in text and "RRX_DECLARE(float, _f32)" in text


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
    a = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, igpt=1, top_at_1=ctypes.c_byte(0), ic=ctypes.c_byte(0), tau=buf(), ssa=buf(),
             band_lims=ctypes.cast((ctypes.c_int * 2)(1, 2), ctypes.c_void_p), cld_tau=buf(), cld_ssa=buf(), cld_g=buf(),
             dx=F(100.), dy=F(100.), dz=F(50.), sfc_albedo=buf(), mu0=F(0.5), azimuth=F(0.3), inc_dir=F(1.), inc_dif=F(0.),
             inc_dir_arr=ctypes.cast((F * 2)(1., 2.), ctypes.c_void_p), inc_dif_arr=ctypes.cast((F * 2)(0., 0.), ctypes.c_void_p),
             knx=1, kny=2, knz=1, k_null=buf(), seed=ctypes.c_ulonglong(7), photon0=ctypes.c_longlong(0), nphotons=ctypes.c_longlong(8),
             photons_per_pixel=ctypes.c_longlong(2), max_events=100, n=ctypes.c_longlong(8), counts=cnt(), scale=F(1.), out=buf(),
             sfc_dn_dir=None, sfc_dn_dif=None, sfc_up=None, tod_up=None, abs_dir=None, abs_dif=None, n_capped=cnt())
    outs = ("sfc_dn_dir", "sfc_dn_dif", "sfc_up", "tod_up", "abs_dir", "abs_dif")
    for k in outs:
        a[k] = buf() if entry == "rrx_raytracer_sw" else cnt()
    a.update(over)
    for k in ("nphotons", "photons_per_pixel", "n", "photon0"):
        if isinstance(a[k], int):
            a[k] = ctypes.c_longlong(a[k])
    if entry == "rrx_rt_counts_to_flux":
        return [a["n"], a["counts"], a["scale"], a["out"], NULL]
    head = [a["nx"], a["ny"], a["nz"], a["ngpt"], a["nbnd"]]
    if entry == "rrx_rt_k_null":
        return head + [a["igpt"], a["top_at_1"], a["tau"], a["band_lims"], a["cld_tau"], a["dz"], a["knx"], a["kny"], a["knz"], a["k_null"], NULL]
    scene = [a["tau"], a["ssa"], a["band_lims"], a["cld_tau"], a["cld_ssa"], a["cld_g"], a["dx"], a["dy"], a["dz"], a["sfc_albedo"],
             a["mu0"], a["azimuth"]]
    tail = [a[k] for k in outs] + [a["n_capped"], NULL]
    if entry == "rrx_rt_trace_counts":
        return head + [a["igpt"], a["top_at_1"], a["ic"]] + scene + [a["inc_dir"], a["inc_dif"], a["knx"], a["kny"], a["knz"], a["k_null"],
                                                                     a["seed"], a["photon0"], a["nphotons"], a["max_events"]] + tail
    return head + [a["top_at_1"], a["ic"]] + scene + [a["inc_dir_arr"], a["inc_dif_arr"], a["knx"], a["kny"], a["knz"],
                                                      a["photons_per_pixel"], a["seed"], a["max_events"]] + tail


def _call(lib, entry, sfx, **over):
    fn = getattr(lib, entry + sfx)
    fn.restype = ctypes.c_int
    return fn(*_args(entry, sfx, **over))


OUTS = ("sfc_dn_dir", "sfc_dn_dif", "sfc_up", "tod_up", "abs_dir", "abs_dif", "n_capped")
NEEDED = {"rrx_rt_k_null": ("tau", "k_null"),
          "rrx_rt_trace_counts": ("tau", "ssa", "sfc_albedo", "k_null") + OUTS,
          "rrx_rt_counts_to_flux": ("counts", "out"),
          "rrx_raytracer_sw": ("tau", "ssa", "sfc_albedo", "inc_dir_arr", "inc_dif_arr") + OUTS}
EXTENTS = {"rrx_rt_k_null": ("nx", "ny", "nz", "ngpt"),
           "rrx_rt_trace_counts": ("nx", "ny", "nz", "ngpt", "nphotons"),
           "rrx_rt_counts_to_flux": ("n",),
           "rrx_raytracer_sw": ("nx", "ny", "nz", "ngpt", "photons_per_pixel")}


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_null_that_is_needed_is_refused_without_a_gpu(entry, sfx):
    lib = _lib()
    for name in NEEDED[entry]:
        assert _call(lib, entry, sfx, **{name: NULL}) != 0, name
        msg = lib.rrx_last_error().decode()
        assert entry + sfx in msg and name.replace("_arr", "") + " is NULL" in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_extents_return_zero_without_a_launch_and_negative_ones_are_refused(entry, sfx):
    lib = _lib()
    for d in EXTENTS[entry]:
        assert _call(lib, entry, sfx, **{d: 0}) == 0, d
        assert _call(lib, entry, sfx, **{d: 0, "tau": NULL, "counts": NULL, "sfc_up": NULL}) == 0, d
        assert _call(lib, entry, sfx, **{d: -1}) != 0, d
        msg = lib.rrx_last_error().decode()
        assert entry + sfx in msg and d + " is negative" in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("entry", ["rrx_rt_trace_counts", "rrx_raytracer_sw"])
def test_scene_checks_name_the_argument(entry, sfx):
    lib = _lib()
    F = ctypes.c_double if sfx == "_f64" else ctypes.c_float
    for over, word in (({"mu0": F(0.)}, "mu0"), ({"mu0": F(-0.2)}, "mu0"), ({"dz": F(0.)}, "dz"), ({"knx": 3}, "knx"), ({"knz": 0}, "knz"),
                       ({"cld_ssa": NULL}, "cld_tau, cld_ssa, cld_g"), ({"band_lims": NULL}, "band_lims_gpt"), ({"max_events": 0}, "max_events")):
        assert _call(lib, entry, sfx, **over) != 0, over
        msg = lib.rrx_last_error().decode()
        assert entry + sfx in msg and word in msg, msg
    # a clear sky: the whole triple NULL is accepted as far as the argument checks go (nphotons = 0: no launch)
    assert _call(lib, entry, sfx, cld_tau=NULL, cld_ssa=NULL, cld_g=NULL, band_lims=NULL, nphotons=0, photons_per_pixel=0) == 0
    if entry == "rrx_rt_trace_counts":
        assert _call(lib, entry, sfx, igpt=2) != 0 and "igpt" in lib.rrx_last_error().decode()
        assert _call(lib, entry, sfx, inc_dir=F(0.)) != 0 and "inc_dir" in lib.rrx_last_error().decode()


def test_host_libraries_export_the_raytracer_class():
    text = open(os.path.join(ROOT, "include", "Raytracer.h")).read()
    assert "class Raytracer_gpu" in text and "trace_rays(" in text
    for hostlib in HOSTLIBS:
        if not os.path.exists(hostlib):
            pytest.fail(f"{hostlib} not built: run __graft_entry__.build()")
        syms = subprocess.run(["nm", "-DC", "--defined-only", hostlib], capture_output=True, text=True).stdout
        assert "Raytracer_gpu::trace_rays(" in syms, hostlib
