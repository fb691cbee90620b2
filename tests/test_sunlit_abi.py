"""CPU tests of the sunlit-only SW entries (rrx_sunlit_columns, rrx_scatter_cols_fill): declared in both precisions and exported,
their argument checks answer without a GPU, and the host layer exports the set_sunlit_columns switch and the driver knows the flag."""
import ctypes
import os
import re
import subprocess

import pytest

import abi

ROOT = abi.ROOT
HOSTLIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")
ENTRIES = ("rrx_sunlit_columns", "rrx_scatter_cols_fill")


def test_header_declares_the_sunlit_entries_in_both_precisions():
    text = abi.header_text()
    for name in ENTRIES:
        assert abi.declares(name), name
    assert "RRX_DECLARE(double, _f64)" in text and "RRX_DECLARE(float, _f32)" in text


def test_library_exports_the_sunlit_entries():
    lib = abi.lib()
    for name in ENTRIES:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["negative_ncol", "null_mu0", "null_perm", "null_count", "pad_to0"])
def test_sunlit_columns_rejects_bad_arguments_without_a_gpu(sfx, case):
    """Arguments are checked before any HIP call: a status and a message, on a machine without a GPU too (the pointers are
    host memory and are never touched)."""
    lib = abi.lib()
    bad = {"negative_ncol": dict(ncol=-1), "null_mu0": dict(null=("order", "mu0")), "null_perm": dict(null=("order", "perm")),
           "null_count": dict(null=("order", "count")), "pad_to0": dict(pad_to=0)}[case]
    rc, msg = abi.call(lib, "rrx_sunlit_columns", sfx, **{**dict(null=("order",), ncol=4, pad_to=1), **bad})        # (no order: 0 .. ncol-1)
    assert rc != 0
    assert "rrx_sunlit_columns" + sfx in msg, msg
    assert {"negative_ncol": "ncol", "null_mu0": "mu0", "null_perm": "perm", "null_count": "count", "pad_to0": "pad_to"}[case] in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["negative_n", "n_above_src", "null_perm", "null_out"])
def test_scatter_cols_fill_rejects_bad_arguments_without_a_gpu(sfx, case):
    lib = abi.lib()
    bad = {"negative_n": dict(n=-1), "n_above_src": dict(n=5), "null_perm": dict(null=("perm",)), "null_out": dict(null=("out",))}[case]
    rc, msg = abi.call(lib, "rrx_scatter_cols_fill", sfx, **{**dict(n=2, nrest=2, ncol_src=4, ncol_dst=4), **bad})
    assert rc != 0
    assert "rrx_scatter_cols_fill" + sfx in msg, msg


def test_host_library_exports_set_sunlit_columns_and_the_driver_knows_the_flag():
    text = open(os.path.join(ROOT, "include_test", "Radiation_solver.h")).read()
    assert text.count("void set_sunlit_columns(const bool b)") == 1          # shortwave only
    if not os.path.exists(HOSTLIB):
        pytest.fail(f"{HOSTLIB} not built: run __graft_entry__.build()")
    abi.lib()                             # (its dependency, by rpath; loaded here so the check does not depend on the loader path)
    host = ctypes.CDLL(HOSTLIB)
    assert hasattr(host, "rrx_cxx_sunlit_columns")
    syms = subprocess.run(["nm", "-DC", "--defined-only", HOSTLIB], capture_output=True, text=True).stdout
    assert "Radiation_solver_shortwave::set_sunlit_columns(bool)" in syms
    drv = open(os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "host", "src_test", "test_rte_rrtmgp_gpu.cpp")).read()
    assert '"sunlit-columns"' in drv
    assert "--sunlit-columns" in open(os.path.join(ROOT, "tools", "acceptance.py")).read()
