"""CPU tests of the rescaled LW entries (rrx_lw_solver_noscat_rescaled, rrx_lw_solver_noscat_fractions_rescaled): declared in both
precisions with their semantics, exported, bound in hip_kernels.py, pipeline.ResidentSolver and the C++ classes and driver with
default off, and their argument checks answer with the entry's name and the offending argument without a GPU. The CPU boundary no
longer refuses do_rescaling."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrx_hip.h")
LIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librrx_hip.so")
GENERAL, FUSED = "rrx_lw_solver_noscat_rescaled", "rrx_lw_solver_noscat_fractions_rescaled"
GENERAL_ARGS = ["secants", "weights", "tau", "ssa", "g", "lay_source", "lev_source", "sfc_emis", "sfc_src", "inc_flux", "flux_up", "flux_dn"]
FUSED_ARGS = ["secants", "weights", "tau", "pfrac", "blay", "blev", "gpoint_bands", "band_lims_gpt", "cld_tau", "cld_ssa", "cld_g",
              "sfc_emis", "sfc_src", "inc_flux", "flux_up", "flux_dn"]


def _lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    lib.rrx_last_error.restype = ctypes.c_char_p
    return lib


@pytest.mark.parametrize("entry", [GENERAL, FUSED])
def test_header_declares_the_entries_with_their_semantics(entry):
    text = open(HEADER).read()
    macro = text[text.index("#define RRX_DECLARE"):text.index("RRX_DECLARE(double")]
    assert re.search(r"\b" + entry + r"##SFX\s*\(", macro)
    for word in ("wb = ssa (1 - g)/2", "st = 1 - ssa + wb", "Cn = 0.4 wb / max(st, 3 tiny)", "tl = tau D st", "An = 1 - tr tr",
                 "Cn (An dn[i]   - tr sdn - sup)", "Cn (An up[i+1] - tr sup - sdn)", "J[i] = tr J[i+1]"):
        assert word in macro, word


@pytest.mark.parametrize("entry", [GENERAL, FUSED])
def test_library_exports_the_entries(entry):
    lib = _lib()
    for sfx in ("_f64", "_f32"):
        assert hasattr(lib, entry + sfx), entry + sfx


def _call_general(lib, sfx, ncol=4, nlay=3, ngpt=8, nmus=1, null=(), broadband=False):
    keep = (ctypes.c_double * 4)()
    p, z = ctypes.cast(keep, ctypes.c_void_p), ctypes.c_void_p(0)
    a = {n: (z if n in null else p) for n in GENERAL_ARGS}
    loc = {n: (z if (n in null or not broadband) else p) for n in ("flux_up_loc", "flux_dn_loc")}
    fn = getattr(lib, GENERAL + sfx); fn.restype = ctypes.c_int
    return fn(ncol, nlay, ngpt, ctypes.c_byte(1), nmus, *[a[n] for n in GENERAL_ARGS], ctypes.c_byte(1 if broadband else 0),
              loc["flux_up_loc"], loc["flux_dn_loc"], ctypes.c_byte(0), z, z, z)


def _call_fused(lib, sfx, ncol=4, nlay=3, ngpt=8, nbnd=2, null=()):
    keep = (ctypes.c_double * 4)()
    p, z = ctypes.cast(keep, ctypes.c_void_p), ctypes.c_void_p(0)
    fn = getattr(lib, FUSED + sfx); fn.restype = ctypes.c_int
    return fn(ncol, nlay, ngpt, nbnd, ctypes.c_byte(1), *[(z if n in null else p) for n in FUSED_ARGS], z)


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("arg", [a for a in GENERAL_ARGS if a != "inc_flux"])
def test_general_entry_names_a_null_pointer(sfx, arg):
    """Arguments are checked before any HIP call (host buffers stand in for device pointers: nothing dereferences them)."""
    lib = _lib()
    assert _call_general(lib, sfx, null=(arg,)) != 0
    msg = lib.rrx_last_error().decode()
    assert msg.startswith(GENERAL + ":") and re.search(r"\b" + arg + r"\b", msg), msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
def test_general_entry_broadband_needs_its_outputs_only(sfx):
    lib = _lib()
    assert _call_general(lib, sfx, null=("flux_up_loc",), broadband=True) != 0
    msg = lib.rrx_last_error().decode()
    assert msg.startswith(GENERAL + ":") and "flux_up_loc" in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("nmus", [0, 5])
def test_general_entry_refuses_other_angle_counts(sfx, nmus):
    lib = _lib()
    assert _call_general(lib, sfx, nmus=nmus) != 0
    msg = lib.rrx_last_error().decode()
    assert msg.startswith(GENERAL + ":") and "n_quad_angs" in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("arg", [a for a in FUSED_ARGS if a != "inc_flux" and not a.startswith("cld_")])
def test_fused_entry_names_a_null_pointer(sfx, arg):
    lib = _lib()
    assert _call_fused(lib, sfx, null=(arg,)) != 0
    msg = lib.rrx_last_error().decode()
    assert msg.startswith(FUSED + ":") and re.search(r"\b" + arg + r"\b", msg), msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("null,named", [(("cld_tau",), "cld_tau"), (("cld_ssa",), "cld_ssa"), (("cld_g",), "cld_g"),
                                        (("cld_tau", "cld_g"), "cld_tau"), (("cld_ssa", "cld_g"), "cld_ssa")])
def test_fused_entry_refuses_a_partly_null_cloud_triple(sfx, null, named):
    lib = _lib()
    assert _call_fused(lib, sfx, null=null) != 0
    msg = lib.rrx_last_error().decode()
    assert msg.startswith(FUSED + ":") and named in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("extent", ["ncol", "nlay", "ngpt", "nbnd"])
def test_negative_extents_are_refused_and_zero_extents_do_nothing(sfx, extent):
    lib = _lib()
    everything = tuple(set(GENERAL_ARGS) | set(FUSED_ARGS))
    assert _call_fused(lib, sfx, **{extent: -1}) != 0
    msg = lib.rrx_last_error().decode()
    assert msg.startswith(FUSED + ":") and extent in msg, msg
    assert _call_fused(lib, sfx, **{extent: 0}, null=everything) == 0          # nothing is read, written or launched
    if extent != "nbnd":
        assert _call_general(lib, sfx, **{extent: -1}) != 0
        msg = lib.rrx_last_error().decode()
        assert msg.startswith(GENERAL + ":") and extent in msg, msg
        assert _call_general(lib, sfx, **{extent: 0}, null=everything) == 0


def test_python_bindings_carry_the_new_names_and_default_off():
    from rte_rrtmgp_cpp_amd import hip_kernels, pipeline, cxx_driver
    for name in ("lw_solver_noscat_rescaled", "lw_solver_noscat_fractions_rescaled"):
        assert callable(getattr(hip_kernels.HipKernels, name))
    assert inspect.signature(pipeline.ResidentSolver.__init__).parameters["lw_rescaling"].default is False
    assert inspect.signature(cxx_driver.CxxDriver.__init__).parameters["lw_rescaling"].default is False


def test_device_source_is_a_file_of_its_own():
    csrc = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "csrc")
    text = open(os.path.join(csrc, "rrx_solver_lw1r.hip")).read()
    assert "lw_rescaled_bb_kernel" in text and "lw_rescaled_serial_kernel" in text
    assert "rrx_solver_lw1r.hip" in open(os.path.join(csrc, "Makefile")).read()
    for other in ("rrx_solver_lw.hip", "rrx_solver_lw2s.hip", "rrx_solver_sw.hip"):
        assert "lw_rescaled" not in open(os.path.join(csrc, other)).read()


def test_host_classes_and_driver_carry_the_new_names_default_off():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    assert "void rte_lw_rescaled(" in read("include", "Rte_lw.h")
    solver = read("include_test", "Radiation_solver.h")
    assert "void set_lw_rescaling(const bool" in solver and "lw_rescaling = false" in solver
    assert "rrx_cxx_lw_rescaling" in read("include_test", "rrx_cxx_driver.h")
    assert "rrx_cxx_lw_rescaling" in read("rte-rrtmgp-cpp_amd", "host", "src_test", "cxx_driver_api.cpp")
    assert re.search(r'"lw-rescaling"\s*,\s*\{\s*false', read("rte-rrtmgp-cpp_amd", "host", "src_test", "test_rte_rrtmgp_gpu.cpp"))
    assert "Rte_lw_gpu::rte_lw_rescaled" in read("rte-rrtmgp-cpp_amd", "host", "src", "Rte.cpp")


def test_cpu_boundary_serves_do_rescaling():
    text = open(os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "host", "src", "rrtmgp_kernels_hip.cpp")).read()
    body = text[text.index("void rte_lw_solver_noscat("):text.index("void rte_sw_solver_2stream(")]
    assert "rrx_lw_solver_noscat_rescaled" in body and "is not served" not in body
    assert "do_rescaling must be false" not in open(os.path.join(ROOT, "include", "rrtmgp_kernels.h")).read()
