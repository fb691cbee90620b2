"""CPU tests of the rescaled LW entries (rrx_lw_solver_noscat_rescaled, rrx_lw_solver_noscat_fractions_rescaled): declared in both
precisions with their semantics, exported, bound in hip_kernels.py, pipeline.ResidentSolver and the C++ classes and driver with
default off, and their argument checks answer with the entry's name and the offending argument without a GPU. The CPU boundary no
longer refuses do_rescaling."""
import inspect
import os
import re

import pytest

import abi

ROOT = abi.ROOT
GENERAL, FUSED = "rrx_lw_solver_noscat_rescaled", "rrx_lw_solver_noscat_fractions_rescaled"
# pointers that may be NULL, so no null-pointer check names them: the top boundary, the cloud triple (all or none), and the general
# entry's outputs of the modes these calls leave off
OPTIONAL_GENERAL = ("inc_flux", "flux_up_loc", "flux_dn_loc", "sfc_src_jac", "flux_up_jac")
OPTIONAL_FUSED = ("inc_flux", "cld_tau", "cld_ssa", "cld_g")


@pytest.mark.parametrize("entry", [GENERAL, FUSED])
def test_header_declares_the_entries_with_their_semantics(entry):
    macro = abi.header_macro()
    assert abi.declares(entry)
    for word in ("wb = ssa (1 - g)/2", "st = 1 - ssa + wb", "Cn = 0.4 wb / max(st, 3 tiny)", "tl = tau D st", "An = 1 - tr tr",
                 "Cn (An dn[i]   - tr sdn - sup)", "Cn (An up[i+1] - tr sup - sdn)", "J[i] = tr J[i+1]"):
        assert word in macro, word


@pytest.mark.parametrize("entry", [GENERAL, FUSED])
def test_library_exports_the_entries(entry):
    lib = abi.lib()
    for sfx in abi.SFXS:
        assert lib.has(entry + sfx), entry + sfx


def _call_general(lib, sfx, null=(), broadband=False, nmus=1, **extents):
    """no Jacobian; the broadband outputs are given with broadband only"""
    off = ("sfc_src_jac", "flux_up_jac") + (() if broadband else ("flux_up_loc", "flux_dn_loc"))
    return abi.call(lib, GENERAL, sfx, null=tuple(null) + off, top_at_1=1, nmus=nmus, do_broadband=int(broadband), do_jacobians=0,
                    **extents)


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
@pytest.mark.parametrize("nmus", [0, 5])
def test_general_entry_refuses_other_angle_counts(sfx, nmus):
    lib = abi.lib()
    rc, msg = _call_general(lib, sfx, nmus=nmus)
    assert rc != 0
    assert msg.startswith(GENERAL + ":") and "n_quad_angs" in msg, msg


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
    everything = tuple(set(abi.pointers(GENERAL)) | set(abi.pointers(FUSED)))
    rc, msg = _call_fused(lib, sfx, **{extent: -1})
    assert rc != 0
    assert msg.startswith(FUSED + ":") and extent in msg, msg
    assert _call_fused(lib, sfx, **{extent: 0}, null=everything)[0] == 0          # nothing is read, written or launched
    if extent != "nbnd":
        rc, msg = _call_general(lib, sfx, **{extent: -1})
        assert rc != 0
        assert msg.startswith(GENERAL + ":") and extent in msg, msg
        assert _call_general(lib, sfx, **{extent: 0}, null=everything)[0] == 0


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
