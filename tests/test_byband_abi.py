"""CPU tests of the by-band solver entries (rrx_lw_solver_noscat_fractions_byband, rrx_sw_solver_2stream_byband): declared in both
precisions and exported, their argument checks answer without a GPU, and the host layer declares and links the by-band switch."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrx_hip.h")
LIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librrx_hip.so")
HOSTLIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")
ENTRIES = ("rrx_lw_solver_noscat_fractions_byband", "rrx_sw_solver_2stream_byband")


def _lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    lib.rrx_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_the_byband_entries_in_both_precisions():
    text = open(HEADER).read()
    macro = text[text.index("#define RRX_DECLARE"):text.index("RRX_DECLARE(double")]
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"##SFX\s*\(", macro), name
    assert "RRX_DECLARE(double, _f64)" in text and "RRX_DECLARE(float, _f32)" in text


def test_library_exports_the_byband_entries():
    lib = _lib()
    for name in ENTRIES:
        for sfx in ("_f64", "_f32"):
            assert hasattr(lib, name + sfx), name + sfx


def _null_args(n):
    return [ctypes.c_void_p(0)] * n


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["nbnd0", "null_band_lims", "ngpt0"])
def test_lw_byband_rejects_bad_arguments_without_a_gpu(sfx, case):
    """Arguments are checked before any HIP call: a status and a message, on a machine without a GPU too."""
    lib = _lib()
    ncol, nlay, ngpt, nbnd = 4, 3, 8, 2
    lims = (ctypes.c_int * 4)(1, 4, 5, 8)
    band_lims = ctypes.cast(lims, ctypes.c_void_p)
    if case == "nbnd0":
        nbnd = 0
    elif case == "null_band_lims":
        band_lims = ctypes.c_void_p(0)
    else:
        ngpt = 0
    fn = getattr(lib, "rrx_lw_solver_noscat_fractions_byband" + sfx)
    fn.restype = ctypes.c_int
    # ncol, nlay, ngpt, nbnd, top_at_1, secants, weights, tau, pfrac, blay, blev, gpoint_bands, band_lims_gpt, sfc_emis, sfc_src,
    # inc_flux, bnd_flux_up, bnd_flux_dn, bnd_flux_net, flux_up, flux_dn, stream
    rc = fn(ncol, nlay, ngpt, nbnd, ctypes.c_byte(1), *_null_args(6), band_lims, *_null_args(8), ctypes.c_void_p(0))
    assert rc != 0
    msg = lib.rrx_last_error().decode()
    assert "rrx_lw_solver_noscat_fractions_byband" in msg
    assert {"nbnd0": "nbnd", "null_band_lims": "band_lims", "ngpt0": "ngpt"}[case] in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["nbnd0", "null_band_lims"])
def test_sw_byband_rejects_bad_arguments_without_a_gpu(sfx, case):
    lib = _lib()
    ncol, nlay, ngpt, nbnd = 4, 3, 8, 2
    lims = (ctypes.c_int * 4)(1, 4, 5, 8)
    band_lims = ctypes.c_void_p(0) if case == "null_band_lims" else ctypes.cast(lims, ctypes.c_void_p)
    if case == "nbnd0":
        nbnd = 0
    fn = getattr(lib, "rrx_sw_solver_2stream_byband" + sfx)
    fn.restype = ctypes.c_int
    # ncol, nlay, ngpt, nbnd, top_at_1, tau, ssa, g, mu0, sfc_alb_dir, sfc_alb_dif, inc_flux_dir, has_dif_bc, inc_flux_dif,
    # band_lims_gpt, bnd_flux_up, bnd_flux_dn, bnd_flux_dir, bnd_flux_net, flux_up, flux_dn, flux_dir, stream
    rc = fn(ncol, nlay, ngpt, nbnd, ctypes.c_byte(1), *_null_args(7), ctypes.c_byte(0), ctypes.c_void_p(0), band_lims,
            *_null_args(7), ctypes.c_void_p(0))
    assert rc != 0
    msg = lib.rrx_last_error().decode()
    assert "rrx_sw_solver_2stream_byband" in msg
    assert ("nbnd" if case == "nbnd0" else "band_lims") in msg, msg


def test_radiation_solver_declares_the_byband_switch_and_the_host_library_links():
    text = open(os.path.join(ROOT, "include_test", "Radiation_solver.h")).read()
    assert text.count("void set_byband_solvers(const bool b)") == 2          # longwave and shortwave
    for h in ("Rte_lw.h", "Rte_sw.h"):
        assert re.search(r"void rte_[ls]w_byband\(", open(os.path.join(ROOT, "include", h)).read()), h
    if not os.path.exists(HOSTLIB):
        pytest.fail(f"{HOSTLIB} not built: run __graft_entry__.build()")
    ctypes.CDLL(LIB)                      # (its dependency, by rpath; loaded here so the check does not depend on the loader path)
    host = ctypes.CDLL(HOSTLIB)
    assert hasattr(host, "rrx_host_main")
    syms = subprocess.run(["nm", "-DC", "--defined-only", HOSTLIB], capture_output=True, text=True).stdout
    assert "Rte_lw_gpu::rte_lw_byband" in syms and "Rte_sw_gpu::rte_sw_byband" in syms
    # the driver knows the option
    drv = open(os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "host", "src_test", "test_rte_rrtmgp_gpu.cpp")).read()
    assert '"byband-solvers"' in drv
