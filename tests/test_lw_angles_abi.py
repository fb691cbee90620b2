"""CPU tests of the several-angle LW entry (rrx_lw_solver_noscat_fractions_angles): declared in both precisions and exported, and its
argument checks answer with the entry's name and the offending argument without a GPU; the host layer declares and exports the
setter and offers the option."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrx_hip.h")
LIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librrx_hip.so")
HOSTLIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")
DRIVER = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "test_rte_rrtmgp_gpu")
ENTRY = "rrx_lw_solver_noscat_fractions_angles"


def _lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    lib.rrx_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_the_entry_in_both_precisions():
    text = open(HEADER).read()
    macro = text[text.index("#define RRX_DECLARE"):text.index("RRX_DECLARE(double")]
    assert re.search(r"\b" + ENTRY + r"##SFX\s*\(", macro)


def test_library_exports_the_entry():
    lib = _lib()
    for sfx in ("_f64", "_f32"):
        assert hasattr(lib, ENTRY + sfx), ENTRY + sfx


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["nmus0", "nmus5", "ncol0", "nlay0", "null_flux_up", "null_flux_dn", "only_sfc_src_jac",
                                  "only_flux_up_jac"])
def test_entry_rejects_bad_arguments_without_a_gpu(sfx, case):
    """Arguments are checked before any HIP call (host buffers stand in for device pointers: nothing dereferences them)."""
    lib = _lib()
    keep = (ctypes.c_double * 4)()
    p, null = ctypes.cast(keep, ctypes.c_void_p), ctypes.c_void_p(0)
    ncol, nlay, ngpt, nmus = 4, 3, 8, 3
    up, dn, sjac, jac = p, p, null, null
    want = {"nmus0": "nmus", "nmus5": "nmus", "ncol0": "ncol", "nlay0": "nlay", "null_flux_up": "flux_up_loc",
            "null_flux_dn": "flux_dn_loc", "only_sfc_src_jac": "flux_up_jac", "only_flux_up_jac": "sfc_src_jac"}[case]
    if case == "nmus0":
        nmus = 0
    elif case == "nmus5":
        nmus = 5
    elif case == "ncol0":
        ncol = 0
    elif case == "nlay0":
        nlay = 0
    elif case == "null_flux_up":
        up = null
    elif case == "null_flux_dn":
        dn = null
    elif case == "only_sfc_src_jac":
        sjac = p
    else:
        jac = p
    fn = getattr(lib, ENTRY + sfx)
    fn.restype = ctypes.c_int
    # ncol, nlay, ngpt, top_at_1, nmus, secants, weights, tau, pfrac, blay, blev, gpoint_bands, sfc_emis, sfc_src, inc_flux,
    # flux_up_loc, flux_dn_loc, sfc_src_jac, flux_up_jac, stream
    rc = fn(ncol, nlay, ngpt, ctypes.c_byte(1), nmus, *([p] * 9), null, up, dn, sjac, jac, null)
    assert rc != 0
    msg = lib.rrx_last_error().decode()
    assert ENTRY in msg and want in msg, msg


def test_solver_header_declares_set_gauss_angles():
    text = open(os.path.join(ROOT, "include_test", "Radiation_solver.h")).read()
    assert re.search(r"void\s+set_gauss_angles\s*\(\s*(const\s+)?int\b", text)
    assert re.search(r"\brrx_cxx_lw_gauss_angles\s*\(", open(os.path.join(ROOT, "include_test", "rrx_cxx_driver.h")).read())


def test_host_library_exports_the_setter_and_keeps_two_rte_lw_overloads():
    if not os.path.exists(HOSTLIB):
        pytest.fail(f"{HOSTLIB} not built: run __graft_entry__.build()")
    syms = subprocess.run(["nm", "-DC", "--defined-only", HOSTLIB], capture_output=True, text=True).stdout
    assert re.search(r"\brrx_cxx_lw_gauss_angles\b", syms)
    overloads = [l for l in syms.splitlines() if "Rte_lw_gpu::rte_lw(" in l]
    assert len(overloads) == 2, overloads


def test_driver_help_lists_lw_gauss_angles():
    if not os.path.exists(DRIVER):
        pytest.fail(f"{DRIVER} not built: run __graft_entry__.build()")
    r = subprocess.run([DRIVER, "--help"], capture_output=True, text=True, timeout=60)
    assert "--lw-gauss-angles" in r.stdout + r.stderr
