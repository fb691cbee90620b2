"""CPU tests of the surface-temperature Jacobian entries (rrx_lw_solver_noscat_fractions_jac, rrx_lw_flux_up_adjust): declared in both
precisions and exported, their argument checks answer without a GPU, and the host layer declares, exports and offers the switch."""
import os
import re
import subprocess

import pytest

import abi

ROOT = abi.ROOT
HOSTLIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")
DRIVER = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "test_rte_rrtmgp_gpu")
ENTRIES = ("rrx_lw_solver_noscat_fractions_jac", "rrx_lw_flux_up_adjust")


def test_header_declares_the_jacobian_entries_in_both_precisions():
    for name in ENTRIES:
        assert abi.declares(name), name


def test_library_exports_the_jacobian_entries():
    lib = abi.lib()
    for name in ENTRIES:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["null_sfc_src_jac", "null_flux_up_jac", "ncol0", "nlay0", "null_broadband"])
def test_lw_jac_rejects_bad_arguments_without_a_gpu(sfx, case):
    """Arguments are checked before any HIP call: a status and a message, on a machine without a GPU too."""
    lib = abi.lib()
    null, extents = ["inc_flux"], {}                 # no flux from above; every other pointer is given
    if case in ("ncol0", "nlay0"):
        extents[case[:-1]] = 0
    else:
        null.append({"null_sfc_src_jac": "sfc_src_jac", "null_flux_up_jac": "flux_up_jac", "null_broadband": "flux_up_loc"}[case])
    rc, msg = abi.call(lib, "rrx_lw_solver_noscat_fractions_jac", sfx, null=null, top_at_1=1, **extents)
    assert rc != 0
    assert "rrx_lw_solver_noscat_fractions_jac" in msg
    want = {"null_sfc_src_jac": "sfc_src_jac", "null_flux_up_jac": "flux_up_jac", "ncol0": "empty", "nlay0": "empty",
            "null_broadband": "broadband"}[case]
    assert want in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["null_jac", "null_t_old", "null_t_new", "null_flux_up", "nlev0"])
def test_flux_up_adjust_rejects_bad_arguments_without_a_gpu(sfx, case):
    lib = abi.lib()
    null = ["flux_net"]                              # (optional)
    if case != "nlev0":
        null.append({"null_jac": "flux_up_jac", "null_t_old": "t_sfc_old", "null_t_new": "t_sfc_new", "null_flux_up": "flux_up"}[case])
    rc, msg = abi.call(lib, "rrx_lw_flux_up_adjust", sfx, null=null, ncol=4, nlev=0 if case == "nlev0" else 5)
    assert rc != 0
    assert "rrx_lw_flux_up_adjust" in msg
    want = {"null_jac": "flux_up_jac", "null_t_old": "surface temperatures", "null_t_new": "surface temperatures",
            "null_flux_up": "flux_up", "nlev0": "empty"}[case]
    assert want in msg, msg


def test_radiation_solver_declares_the_jacobian_switch_and_the_host_library_exports_the_overload():
    text = open(os.path.join(ROOT, "include_test", "Radiation_solver.h")).read()
    assert "void set_jacobian(const bool b)" in text and "get_lw_flux_up_jac()" in text
    assert text.count("Array_gpu<Float,3>& flux_up_jac") == 0                       # (the solver's own argument list is the reference's)
    assert re.search(r"Array_gpu<Float,3>& flux_up_jac,\s*const int n_gauss_angles\);", open(os.path.join(ROOT, "include", "Rte_lw.h")).read())
    if not os.path.exists(HOSTLIB):
        pytest.fail(f"{HOSTLIB} not built: run __graft_entry__.build()")
    syms = subprocess.run(["nm", "-DC", "--defined-only", HOSTLIB], capture_output=True, text=True).stdout
    overloads = [l for l in syms.splitlines() if "Rte_lw_gpu::rte_lw(" in l]
    assert len(overloads) == 2, overloads
    assert any(l.count("Array_gpu<double, 3>&") == 3 for l in overloads), overloads
    assert "Radiation_solver_longwave::solve_gpu(" in syms
    for name in ("rrx_cxx_lw_jacobian", "rrx_cxx_lw_flux_up_jac"):
        assert re.search(r"\b" + name + r"\b", syms), name


def test_driver_help_lists_lw_jacobian():
    if not os.path.exists(DRIVER):
        pytest.fail(f"{DRIVER} not built: run __graft_entry__.build()")
    r = subprocess.run([DRIVER, "--help"], capture_output=True, text=True, timeout=60)
    assert "--lw-jacobian" in r.stdout + r.stderr
