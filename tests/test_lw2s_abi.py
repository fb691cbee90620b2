"""CPU tests of the LW two-stream entries with scattering (rrx_lw_solver_2stream, rrx_lw_solver_2stream_fractions): declared in both
precisions with their semantics, exported, bound in hip_kernels.py and pipeline.ResidentSolver, and their argument checks answer with
the entry's name and the offending argument without a GPU. Rte_lw_gpu::rte_lw keeps its two overloads."""
import inspect
import os
import re
import subprocess

import pytest

import abi

ROOT = abi.ROOT
HOSTLIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")
GENERAL, FUSED = "rrx_lw_solver_2stream", "rrx_lw_solver_2stream_fractions"
# pointers that may be NULL, so no null-pointer check names them: the top boundary, the cloud triple (all or none), and the general
# entry's broadband outputs, which these calls give with broadband only
OPTIONAL_GENERAL = ("inc_flux", "flux_up_loc", "flux_dn_loc")
OPTIONAL_FUSED = ("inc_flux", "cld_tau", "cld_ssa", "cld_g")


@pytest.mark.parametrize("entry", [GENERAL, FUSED])
def test_header_declares_the_entries_with_their_semantics(entry):
    macro = abi.header_macro()
    assert abi.declares(entry)
    for word in ("gamma1", "gamma2", "Rdif", "Tdif", "1.66", "1e-8", "1e-12", "sfc_emis", "inc_flux", "rrx_inc_2stream_by_2stream_bybnd"):
        assert word in macro, word


@pytest.mark.parametrize("entry", [GENERAL, FUSED])
def test_library_exports_the_entries(entry):
    lib = abi.lib()
    for sfx in abi.SFXS:
        assert lib.has(entry + sfx), entry + sfx


def _call_general(lib, sfx, null=(), broadband=False, **extents):
    off = () if broadband else ("flux_up_loc", "flux_dn_loc")
    return abi.call(lib, GENERAL, sfx, null=tuple(null) + off, top_at_1=1, do_broadband=int(broadband), **extents)


def _call_fused(lib, sfx, null=(), **extents):
    return abi.call(lib, FUSED, sfx, null=null, top_at_1=1, **extents)


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("arg", [a for a in abi.pointers(GENERAL) if a not in OPTIONAL_GENERAL])
def test_general_entry_names_a_null_pointer(sfx, arg):
    """Arguments are checked before any HIP call (host buffers stand in for device pointers: nothing dereferences them)."""
    lib = abi.lib()
    rc, msg = _call_general(lib, sfx, null=(arg,))
    assert rc != 0
    assert msg.startswith(GENERAL + ":") and re.search(r"\b" + arg + r"\b", msg), msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
def test_general_entry_broadband_needs_its_outputs_only(sfx):
    lib = abi.lib()
    rc, msg = _call_general(lib, sfx, null=("flux_up_loc",), broadband=True)
    assert rc != 0
    assert msg.startswith(GENERAL + ":") and "flux_up_loc" in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("arg", [a for a in abi.pointers(FUSED) if a not in OPTIONAL_FUSED])
def test_fused_entry_names_a_null_pointer(sfx, arg):
    lib = abi.lib()
    rc, msg = _call_fused(lib, sfx, null=(arg,))
    assert rc != 0
    assert msg.startswith(FUSED + ":") and re.search(r"\b" + arg + r"\b", msg), msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("null,named", [(("cld_tau",), "cld_tau"), (("cld_ssa",), "cld_ssa"), (("cld_g",), "cld_g"),
                                        (("cld_tau", "cld_g"), "cld_tau"), (("cld_ssa", "cld_g"), "cld_ssa")])
def test_fused_entry_refuses_a_partly_null_cloud_triple(sfx, null, named):
    lib = abi.lib()
    rc, msg = _call_fused(lib, sfx, null=null)
    assert rc != 0
    assert msg.startswith(FUSED + ":") and named in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("extent", ["ncol", "nlay", "ngpt", "nbnd"])
def test_negative_extents_are_refused_and_zero_extents_do_nothing(sfx, extent):
    lib = abi.lib()
    everything = ("tau", "ssa", "g", "lev_source", "pfrac", "blev", "sfc_emis", "sfc_src", "flux_up", "flux_dn")
    rc, msg = _call_fused(lib, sfx, **{extent: -1})
    assert rc != 0
    assert msg.startswith(FUSED + ":") and extent in msg, msg
    assert _call_fused(lib, sfx, **{extent: 0}, null=everything)[0] == 0          # nothing is read, written or launched
    if extent != "nbnd":
        rc, msg = _call_general(lib, sfx, **{extent: -1})
        assert rc != 0
        assert msg.startswith(GENERAL + ":") and extent in msg, msg
        assert _call_general(lib, sfx, **{extent: 0}, null=everything)[0] == 0


def test_python_bindings_carry_the_new_names():
    from rte_rrtmgp_cpp_amd import hip_kernels, pipeline
    for name in ("lw_solver_2stream", "lw_solver_2stream_fractions"):
        assert callable(getattr(hip_kernels.HipKernels, name))
    sig = inspect.signature(pipeline.ResidentSolver.__init__)
    assert sig.parameters["lw_scattering"].default is False


def test_device_source_is_a_file_of_its_own():
    csrc = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "csrc")
    text = open(os.path.join(csrc, "rrx_solver_lw2s.hip")).read()
    assert "lw_2stream_bb_kernel" in text and "lw_2stream_serial_kernel" in text
    assert "rrx_solver_lw2s.hip" in open(os.path.join(csrc, "Makefile")).read()
    for other in ("rrx_solver_lw.hip", "rrx_solver_sw.hip"):
        assert "lw_2stream" not in open(os.path.join(csrc, other)).read()


def test_rte_lw_keeps_two_overloads():
    if not os.path.exists(HOSTLIB):
        pytest.fail(f"{HOSTLIB} not built: run __graft_entry__.build()")
    syms = subprocess.run(["nm", "-DC", "--defined-only", HOSTLIB], capture_output=True, text=True).stdout
    overloads = [l for l in syms.splitlines() if "Rte_lw_gpu::rte_lw(" in l]
    assert len(overloads) == 2, overloads


def test_host_classes_carry_the_new_names():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    rte = read("include", "Rte_lw.h")
    assert "void rte_lw_2stream(" in rte
    assert len(re.findall(r"\bvoid rte_lw\(", rte)) == 2                       # rte_lw keeps its two overloads
    assert "void set_lw_scattering(const bool" in read("include_test", "Radiation_solver.h")
    assert "rrx_cxx_lw_scattering" in read("include_test", "rrx_cxx_driver.h")
    assert "rrx_cxx_lw_scattering" in read("rte-rrtmgp-cpp_amd", "host", "src_test", "cxx_driver_api.cpp")
    assert '"lw-scattering"' in read("rte-rrtmgp-cpp_amd", "host", "src_test", "test_rte_rrtmgp_gpu.cpp")
    assert "lw_scattering=False" in read("rte-rrtmgp-cpp_amd", "cxx_driver.py")
    assert "Rte_lw_gpu::rte_lw_2stream" in read("rte-rrtmgp-cpp_amd", "host", "src", "Rte.cpp")
