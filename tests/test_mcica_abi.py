"""CPU tests of the McICA cloud-sampling entries (rrx_mcica_increment_1scalar, rrx_mcica_increment_2stream, rrx_mcica_cloud_mask):
declared in both precisions and exported, their argument checks answer without a GPU, and the host layer exports
set_cloud_sampling and the driver knows the options."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrx_hip.h")
LIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librrx_hip.so")
HOSTLIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")
ENTRIES = ("rrx_mcica_increment_1scalar", "rrx_mcica_increment_2stream", "rrx_mcica_cloud_mask")
NULL = ctypes.c_void_p(0)


def _lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    lib.rrx_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_the_mcica_entries_in_both_precisions():
    text = open(HEADER).read()
    macro = text[text.index("#define RRX_DECLARE"):text.index("RRX_DECLARE(double")]
    for name in ENTRIES:
        m = re.search(r"\bint " + name + r"##SFX\s*\(([^;]*)\);", macro)
        assert m, name
        assert re.search(r"void\*\s*stream\s*$", m.group(1).replace("\\", "").strip()), name          # the stream goes last
        assert "unsigned long long seed" in m.group(1) and "unsigned char* mask_out" in m.group(1), name
    assert "RRX_DECLARE(double, _f64)" in text and "RRX_DECLARE(float, _f32)" in text
    assert re.search(r"\bint rrx_mcica_column_ids\s*\(", text)


def test_library_exports_the_mcica_entries():
    lib = _lib()
    for name in ENTRIES:
        for sfx in ("_f64", "_f32"):
            assert hasattr(lib, name + sfx), name + sfx
    assert hasattr(lib, "rrx_mcica_column_ids")


def _args(entry, sfx, **over):
    """The argument list of an entry on host memory that is never touched: the checks come before any HIP call."""
    F = ctypes.c_double if sfx == "_f64" else ctypes.c_float
    buf = lambda: ctypes.cast((F * 64)(), ctypes.c_void_p)
    a = dict(ncol=2, nlay=3, ngpt=4, nbnd=2, band_lims=ctypes.cast((ctypes.c_int * 4)(1, 2, 3, 4), ctypes.c_void_p), cloud_frac=buf(), alpha=NULL,
             seed=ctypes.c_ulonglong(7), domain=0, col_id=NULL, col_id0=0, tau=buf(), ssa=buf(), g=buf(), cld_tau=buf(), cld_ssa=buf(),
             cld_g=buf(), mask=ctypes.cast((ctypes.c_ubyte * 64)(), ctypes.c_void_p))
    a.update(over)
    head = [a["ncol"], a["nlay"], a["ngpt"]]
    mid = [a["cloud_frac"], a["alpha"], a["seed"], a["domain"], a["col_id"], a["col_id0"]]
    if entry == "rrx_mcica_cloud_mask":
        return head + mid + [a["mask"], NULL]
    head += [a["nbnd"], a["band_lims"]]
    if entry == "rrx_mcica_increment_1scalar":
        return head + mid + [a["tau"], a["cld_tau"], a["mask"], NULL]
    return head + mid + [a["tau"], a["ssa"], a["g"], a["cld_tau"], a["cld_ssa"], a["cld_g"], a["mask"], NULL]


def _call(lib, entry, sfx, **over):
    fn = getattr(lib, entry + sfx)
    fn.restype = ctypes.c_int
    return fn(*_args(entry, sfx, **over))


NEEDED = {"rrx_mcica_increment_1scalar": ("cloud_frac", "band_lims", "tau", "cld_tau"),
          "rrx_mcica_increment_2stream": ("cloud_frac", "band_lims", "tau", "ssa", "g", "cld_tau", "cld_ssa", "cld_g"),
          "rrx_mcica_cloud_mask": ("cloud_frac", "mask")}


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_null_that_is_needed_is_refused_without_a_gpu(entry, sfx):
    lib = _lib()
    for name in NEEDED[entry]:
        assert _call(lib, entry, sfx, **{name: NULL}) == 1, name
        msg = lib.rrx_last_error().decode()
        assert entry + sfx in msg and "NULL" in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_extents_return_zero_without_a_launch_and_negative_ones_are_refused(entry, sfx):
    """An extent of 0 returns 0 although the machine may have no device (no launch is made), whatever the pointers are."""
    lib = _lib()
    dims = ("ncol", "nlay", "ngpt") + (("nbnd",) if entry != "rrx_mcica_cloud_mask" else ())
    for d in dims:
        assert _call(lib, entry, sfx, **{d: 0}) == 0, d
        assert _call(lib, entry, sfx, **{d: 0, "cloud_frac": NULL, "tau": NULL, "mask": NULL}) == 0, d
        assert _call(lib, entry, sfx, **{d: -1}) != 0, d
        assert entry + sfx in lib.rrx_last_error().decode()


def test_column_ids_checks_its_arguments_without_a_gpu():
    lib = _lib()
    lib.rrx_mcica_column_ids.restype = ctypes.c_int
    buf = ctypes.cast((ctypes.c_int * 4)(), ctypes.c_void_p)
    assert lib.rrx_mcica_column_ids(0, NULL, 0, NULL, NULL) == 0
    assert lib.rrx_mcica_column_ids(-1, buf, 0, buf, NULL) != 0
    assert lib.rrx_mcica_column_ids(4, NULL, 0, buf, NULL) != 0
    assert "rrx_mcica_column_ids" in lib.rrx_last_error().decode()


def test_host_library_exports_set_cloud_sampling_and_the_driver_knows_the_options():
    text = open(os.path.join(ROOT, "include_test", "Radiation_solver.h")).read()
    assert text.count("void set_cloud_sampling(const Array_gpu<Float,2>* cloud_frac, const int overlap, const Array_gpu<Float,2>* overlap_param,") == 2
    if not os.path.exists(HOSTLIB):
        pytest.fail(f"{HOSTLIB} not built: run __graft_entry__.build()")
    ctypes.CDLL(LIB)                      # (its dependency, by rpath; loaded here so the check does not depend on the loader path)
    host = ctypes.CDLL(HOSTLIB)
    assert hasattr(host, "rrx_cxx_cloud_sampling")
    syms = subprocess.run(["nm", "-DC", "--defined-only", HOSTLIB], capture_output=True, text=True).stdout
    assert "Radiation_solver_longwave::set_cloud_sampling(" in syms and "Radiation_solver_shortwave::set_cloud_sampling(" in syms
    drv = open(os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "host", "src_test", "test_rte_rrtmgp_gpu.cpp")).read()
    for opt in ('"cloud-fraction"', '"--cloud-overlap"', '"--mcica-seed"'):
        assert opt in drv, opt
