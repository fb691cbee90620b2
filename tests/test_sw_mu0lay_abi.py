"""CPU tests of the mu0-by-layer entries (rrx_sw_solver_2stream_mu0lay, rrx_sw_solver_2stream_byband_mu0lay,
rrx_zenith_angle_spherical_correction): declared in both precisions, exported by the built library, and the correction's argument
checks answer without a GPU. The two 1-D solver entries keep their declarations."""
import ctypes
import os
import re

import pytest

import abi

ROOT = abi.ROOT
ENTRIES = ("rrx_sw_solver_2stream_mu0lay", "rrx_sw_solver_2stream_byband_mu0lay", "rrx_zenith_angle_spherical_correction")


def test_header_declares_the_entries_in_both_precisions():
    text = abi.header_text()
    for name in ENTRIES:
        assert abi.declares(name), name
        assert abi.params(name)[-1] == ("void*", "stream"), name          # the stream goes last
    assert "RRX_DECLARE(double, _f64)" in text and "RRX_DECLARE(float, _f32)" in text
    for sfx, F in zip(abi.SFXS, ("double", "float")):
        # the by-layer solvers take the 1-D entries' arguments with mu0_lay in the place of mu0
        for one, lay in (("rrx_sw_solver_2stream", ENTRIES[0]), ("rrx_sw_solver_2stream_byband", ENTRIES[1])):
            assert abi.params(lay, sfx) == tuple((t, "mu0_lay" if n == "mu0" else n) for t, n in abi.params(one, sfx))
            assert (f"const {F}*", "mu0") in abi.params(one, sfx)
        assert abi.params(ENTRIES[2], sfx) == (("int", "ncol"), ("int", "nlay"), (f"const {F}*", "ref_alt"), (f"const {F}*", "ref_mu"),
                                               (f"const {F}*", "alt"), (F, "planet_radius"), (f"{F}*", "mu0_lay"), ("void*", "stream"))


def test_library_exports_the_six_names():
    lib = abi.lib()
    for name in ENTRIES:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
def test_correction_checks_its_arguments_without_a_gpu(sfx):
    lib = abi.lib()
    entry = "rrx_zenith_angle_spherical_correction"
    call = lambda null=(), **kw: abi.call(lib, entry, sfx, null=("ref_alt",) + tuple(null), **{**dict(planet_radius=6.37123e6), **kw})
    for dims in (dict(ncol=0, nlay=3), dict(ncol=4, nlay=0)):        # nothing to do: no launch, whatever the pointers are
        assert call(**dims)[0] == 0
        assert call(null=abi.pointers(entry), **dims)[0] == 0
    for bad in (dict(ncol=-1), dict(nlay=-3), dict(null=("ref_mu",)), dict(null=("alt",)), dict(null=("mu0_lay",)), dict(planet_radius=0.)):
        rc, msg = call(**{**dict(ncol=4, nlay=3), **bad})
        assert rc != 0
        assert entry + sfx in msg


def test_host_layer_has_the_overloads_and_the_setter():
    import subprocess
    hostlib = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")
    if not os.path.exists(hostlib):
        pytest.fail(f"{hostlib} not built: run __graft_entry__.build()")
    abi.lib()                             # (its dependency, by rpath; loaded here so the check does not depend on the loader path)
    assert hasattr(ctypes.CDLL(hostlib), "rrx_cxx_spherical_mu0")
    syms = subprocess.run(["nm", "-DC", "--defined-only", hostlib], capture_output=True, text=True).stdout
    assert "Radiation_solver_shortwave::set_spherical_mu0(" in syms
    for fn in ("Rte_sw_gpu::rte_sw(", "Rte_sw_gpu::rte_sw_byband("):       # mu0 (ncol) and mu0 (ncol, nlay)
        sigs = [l for l in syms.splitlines() if fn in l]
        assert any("Array_gpu<double, 1> const&, Array_gpu<double, 2> const&" in l for l in sigs), fn
        assert any("bool, Array_gpu<double, 2> const&, Array_gpu<double, 2> const&" in l or
                   "char, Array_gpu<double, 2> const&, Array_gpu<double, 2> const&" in l for l in sigs), (fn, sigs)
    # the CPU boundary library calls the by-layer entry (its behaviour: tests/test_gpu_sw_mu0lay.py)
    boundary = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librrtmgp_kernels_hip.so")],
                              capture_output=True, text=True).stdout
    assert "rrx_sw_solver_2stream_mu0lay_f64" in boundary
