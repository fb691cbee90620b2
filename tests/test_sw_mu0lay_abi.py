"""CPU tests of the mu0-by-layer entries (rrx_sw_solver_2stream_mu0lay, rrx_sw_solver_2stream_byband_mu0lay,
rrx_zenith_angle_spherical_correction): declared in both precisions, exported by the built library, and the correction's argument
checks answer without a GPU. The two 1-D solver entries keep their declarations."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrx_hip.h")
LIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librrx_hip.so")
ENTRIES = ("rrx_sw_solver_2stream_mu0lay", "rrx_sw_solver_2stream_byband_mu0lay", "rrx_zenith_angle_spherical_correction")
NULL = ctypes.c_void_p(0)


def _lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    lib.rrx_last_error.restype = ctypes.c_char_p
    return lib


def _decl(macro, name):
    m = re.search(r"\bint " + name + r"##SFX\s*\(([^;]*)\);", macro)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1).replace("\\", "")).strip()


def test_header_declares_the_entries_in_both_precisions():
    text = open(HEADER).read()
    macro = text[text.index("#define RRX_DECLARE"):text.index("RRX_DECLARE(double")]
    for name in ENTRIES:
        assert re.search(r"void\* stream$", _decl(macro, name)), name          # the stream goes last
    assert "RRX_DECLARE(double, _f64)" in text and "RRX_DECLARE(float, _f32)" in text
    # the by-layer solvers take the 1-D entries' arguments with mu0_lay in the place of mu0
    for one, lay in (("rrx_sw_solver_2stream", ENTRIES[0]), ("rrx_sw_solver_2stream_byband", ENTRIES[1])):
        assert _decl(macro, lay) == _decl(macro, one).replace("const F* mu0,", "const F* mu0_lay,")
    assert _decl(macro, ENTRIES[2]) == ("int ncol, int nlay, const F* ref_alt, const F* ref_mu, const F* alt, F planet_radius, "
                                        "F* mu0_lay, void* stream")


def test_library_exports_the_six_names():
    lib = _lib()
    for name in ENTRIES:
        for sfx in ("_f64", "_f32"):
            assert hasattr(lib, name + sfx), name + sfx


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
def test_correction_checks_its_arguments_without_a_gpu(sfx):
    lib = _lib()
    F = ctypes.c_double if sfx == "_f64" else ctypes.c_float
    fn = getattr(lib, "rrx_zenith_angle_spherical_correction" + sfx)
    fn.restype = ctypes.c_int
    buf = lambda: ctypes.cast((F * 64)(), ctypes.c_void_p)
    R = F(6.37123e6)
    for dims in ((0, 3), (4, 0)):                                   # nothing to do: no launch, whatever the pointers are
        assert fn(*dims, NULL, buf(), buf(), R, buf(), NULL) == 0
        assert fn(*dims, NULL, NULL, NULL, R, NULL, NULL) == 0
    for args in ((-1, 3, NULL, buf(), buf(), R, buf()), (4, -3, NULL, buf(), buf(), R, buf()), (4, 3, NULL, NULL, buf(), R, buf()),
                 (4, 3, NULL, buf(), NULL, R, buf()), (4, 3, NULL, buf(), buf(), R, NULL), (4, 3, NULL, buf(), buf(), F(0.), buf())):
        assert fn(*args, NULL) != 0
        assert "rrx_zenith_angle_spherical_correction" + sfx in lib.rrx_last_error().decode()


def test_host_layer_has_the_overloads_and_the_setter():
    import subprocess
    hostlib = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")
    if not os.path.exists(hostlib):
        pytest.fail(f"{hostlib} not built: run __graft_entry__.build()")
    ctypes.CDLL(LIB)                      # (its dependency, by rpath; loaded here so the check does not depend on the loader path)
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
