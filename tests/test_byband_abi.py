"""CPU tests of the by-band solver entries (rrx_lw_solver_noscat_fractions_byband, rrx_sw_solver_2stream_byband): declared in both
precisions and exported, their argument checks answer without a GPU, and the host layer declares and links the by-band switch."""
import ctypes
import os
import re
import subprocess

import pytest

import abi

ROOT = abi.ROOT
HOSTLIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")
ENTRIES = ("rrx_lw_solver_noscat_fractions_byband", "rrx_sw_solver_2stream_byband")


def test_header_declares_the_byband_entries_in_both_precisions():
    text = abi.header_text()
    for name in ENTRIES:
        assert abi.declares(name), name
    assert "RRX_DECLARE(double, _f64)" in text and "RRX_DECLARE(float, _f32)" in text


def test_library_exports_the_byband_entries():
    lib = abi.lib()
    for name in ENTRIES:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx


def _call(lib, entry, sfx, case):
    """every pointer NULL but band_lims_gpt: the checks of the band arguments come first"""
    null = abi.pointers(entry) if case == "null_band_lims" else [n for n in abi.pointers(entry) if n != "band_lims_gpt"]
    extents = {"nbnd0": {"nbnd": 0}, "ngpt0": {"ngpt": 0}}.get(case, {})
    return abi.call(lib, entry, sfx, null=null, top_at_1=1, **extents)


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["nbnd0", "null_band_lims", "ngpt0"])
def test_lw_byband_rejects_bad_arguments_without_a_gpu(sfx, case):
    """Arguments are checked before any HIP call: a status and a message, on a machine without a GPU too."""
    lib = abi.lib()
    rc, msg = _call(lib, "rrx_lw_solver_noscat_fractions_byband", sfx, case)
    assert rc != 0
    assert "rrx_lw_solver_noscat_fractions_byband" in msg
    assert {"nbnd0": "nbnd", "null_band_lims": "band_lims", "ngpt0": "ngpt"}[case] in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["nbnd0", "null_band_lims"])
def test_sw_byband_rejects_bad_arguments_without_a_gpu(sfx, case):
    lib = abi.lib()
    rc, msg = _call(lib, "rrx_sw_solver_2stream_byband", sfx, case)
    assert rc != 0
    assert "rrx_sw_solver_2stream_byband" in msg
    assert ("nbnd" if case == "nbnd0" else "band_lims") in msg, msg


def test_radiation_solver_declares_the_byband_switch_and_the_host_library_links():
    text = open(os.path.join(ROOT, "include_test", "Radiation_solver.h")).read()
    assert text.count("void set_byband_solvers(const bool b)") == 2          # longwave and shortwave
    for h in ("Rte_lw.h", "Rte_sw.h"):
        assert re.search(r"void rte_[ls]w_byband\(", open(os.path.join(ROOT, "include", h)).read()), h
    if not os.path.exists(HOSTLIB):
        pytest.fail(f"{HOSTLIB} not built: run __graft_entry__.build()")
    abi.lib()                             # (its dependency, by rpath; loaded here so the check does not depend on the loader path)
    host = ctypes.CDLL(HOSTLIB)
    assert hasattr(host, "rrx_host_main")
    syms = subprocess.run(["nm", "-DC", "--defined-only", HOSTLIB], capture_output=True, text=True).stdout
    assert "Rte_lw_gpu::rte_lw_byband" in syms and "Rte_sw_gpu::rte_sw_byband" in syms
    # the driver knows the option
    drv = open(os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "host", "src_test", "test_rte_rrtmgp_gpu.cpp")).read()
    assert '"byband-solvers"' in drv
