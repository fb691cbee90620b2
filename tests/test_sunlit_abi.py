"""CPU tests of the sunlit-only SW entries (rrx_sunlit_columns, rrx_scatter_cols_fill): declared in both precisions and exported,
their argument checks answer without a GPU, and the host layer exports the set_sunlit_columns switch and the driver knows the flag."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrx_hip.h")
LIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librrx_hip.so")
HOSTLIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")
ENTRIES = ("rrx_sunlit_columns", "rrx_scatter_cols_fill")


def _lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    lib.rrx_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_the_sunlit_entries_in_both_precisions():
    text = open(HEADER).read()
    macro = text[text.index("#define RRX_DECLARE"):text.index("RRX_DECLARE(double")]
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"##SFX\s*\(", macro), name
    assert "RRX_DECLARE(double, _f64)" in text and "RRX_DECLARE(float, _f32)" in text


def test_library_exports_the_sunlit_entries():
    lib = _lib()
    for name in ENTRIES:
        for sfx in ("_f64", "_f32"):
            assert hasattr(lib, name + sfx), name + sfx


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["negative_ncol", "null_mu0", "null_perm", "null_count", "pad_to0"])
def test_sunlit_columns_rejects_bad_arguments_without_a_gpu(sfx, case):
    """Arguments are checked before any HIP call: a status and a message, on a machine without a GPU too (the pointers are
    host memory and are never touched)."""
    lib = _lib()
    mu0 = (ctypes.c_double * 4)() if sfx == "_f64" else (ctypes.c_float * 4)()
    perm, count = (ctypes.c_int * 4)(), (ctypes.c_int * 1)()
    args = dict(ncol=4, mu0=ctypes.cast(mu0, ctypes.c_void_p), pad_to=1, perm=ctypes.cast(perm, ctypes.c_void_p),
                count=ctypes.cast(count, ctypes.c_void_p))
    bad = {"negative_ncol": ("ncol", -1), "null_mu0": ("mu0", ctypes.c_void_p(0)), "null_perm": ("perm", ctypes.c_void_p(0)),
           "null_count": ("count", ctypes.c_void_p(0)), "pad_to0": ("pad_to", 0)}[case]
    args[bad[0]] = bad[1]
    fn = getattr(lib, "rrx_sunlit_columns" + sfx)
    fn.restype = ctypes.c_int
    rc = fn(args["ncol"], args["mu0"], ctypes.c_void_p(0), args["pad_to"], args["perm"], args["count"], ctypes.c_void_p(0))
    assert rc != 0
    msg = lib.rrx_last_error().decode()
    assert "rrx_sunlit_columns" + sfx in msg, msg
    assert {"negative_ncol": "ncol", "null_mu0": "mu0", "null_perm": "perm", "null_count": "count", "pad_to0": "pad_to"}[case] in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["negative_n", "n_above_src", "null_perm", "null_out"])
def test_scatter_cols_fill_rejects_bad_arguments_without_a_gpu(sfx, case):
    lib = _lib()
    buf = (ctypes.c_double * 16)()
    perm = (ctypes.c_int * 4)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    # n, nrest, perm, ncol_src, in, ncol_dst, out
    a = [2, ctypes.c_ulonglong(2), p(perm), 4, p(buf), 4, p(buf)]
    if case == "negative_n":
        a[0] = -1
    elif case == "n_above_src":
        a[0] = 5
    elif case == "null_perm":
        a[2] = ctypes.c_void_p(0)
    else:
        a[6] = ctypes.c_void_p(0)
    fn = getattr(lib, "rrx_scatter_cols_fill" + sfx)
    fn.restype = ctypes.c_int
    assert fn(*a, ctypes.c_void_p(0)) != 0
    msg = lib.rrx_last_error().decode()
    assert "rrx_scatter_cols_fill" + sfx in msg, msg


def test_host_library_exports_set_sunlit_columns_and_the_driver_knows_the_flag():
    text = open(os.path.join(ROOT, "include_test", "Radiation_solver.h")).read()
    assert text.count("void set_sunlit_columns(const bool b)") == 1          # shortwave only
    if not os.path.exists(HOSTLIB):
        pytest.fail(f"{HOSTLIB} not built: run __graft_entry__.build()")
    ctypes.CDLL(LIB)                      # (its dependency, by rpath; loaded here so the check does not depend on the loader path)
    host = ctypes.CDLL(HOSTLIB)
    assert hasattr(host, "rrx_cxx_sunlit_columns")
    syms = subprocess.run(["nm", "-DC", "--defined-only", HOSTLIB], capture_output=True, text=True).stdout
    assert "Radiation_solver_shortwave::set_sunlit_columns(bool)" in syms
    drv = open(os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "host", "src_test", "test_rte_rrtmgp_gpu.cpp")).read()
    assert '"sunlit-columns"' in drv
    assert "--sunlit-columns" in open(os.path.join(ROOT, "tools", "acceptance.py")).read()
