"""CPU tests of the several-angle LW entry (rrx_lw_solver_noscat_fractions_angles): declared in both precisions and exported, and its
argument checks answer with the entry's name and the offending argument without a GPU; the host layer declares and exports the
setter and offers the option."""
import os
import re
import subprocess

import pytest

import abi

ROOT = abi.ROOT
HOSTLIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")
DRIVER = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "test_rte_rrtmgp_gpu")
ENTRY = "rrx_lw_solver_noscat_fractions_angles"


def test_header_declares_the_entry_in_both_precisions():
    assert abi.declares(ENTRY)


def test_library_exports_the_entry():
    lib = abi.lib()
    for sfx in abi.SFXS:
        assert lib.has(ENTRY + sfx), ENTRY + sfx


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["nmus0", "nmus5", "ncol0", "nlay0", "null_flux_up", "null_flux_dn", "only_sfc_src_jac",
                                  "only_flux_up_jac"])
def test_entry_rejects_bad_arguments_without_a_gpu(sfx, case):
    """Arguments are checked before any HIP call (host buffers stand in for device pointers: nothing dereferences them)."""
    lib = abi.lib()
    want = {"nmus0": "nmus", "nmus5": "nmus", "ncol0": "ncol", "nlay0": "nlay", "null_flux_up": "flux_up_loc",
            "null_flux_dn": "flux_dn_loc", "only_sfc_src_jac": "flux_up_jac", "only_flux_up_jac": "sfc_src_jac"}[case]
    null = ["inc_flux", "sfc_src_jac", "flux_up_jac"]              # three angles, fluxes only, no flux from above
    scalars = dict(top_at_1=1, nmus=3)
    if case.startswith("nmus"):
        scalars["nmus"] = int(case[4:])
    elif case.endswith("0"):
        scalars[case[:-1]] = 0
    elif case.startswith("null_"):
        null.append(case[5:] + "_loc")
    else:
        null.remove(case[5:])
    rc, msg = abi.call(lib, ENTRY, sfx, null=null, **scalars)
    assert rc != 0
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
