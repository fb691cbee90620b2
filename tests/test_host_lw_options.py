"""CPU test of the LW options of the C++ class API: lw_solve_plan() of Radiation_solver.cpp, through rrx_host_selftest_lw_plan, against the
rules as Radiation_solver_longwave::solve_gpu stated them before they became one table -- its chain of `if (a && b) throw`, transcribed
here as predicates, and its formulas for the effective flags. Every combination of the boolean inputs with 1 and 3 quadrature angles.
The list below is checked against that chain by eye; it is not derived from the C++ table."""
import ctypes
import itertools
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = ("broadband_solvers", "byband_solvers", "jacobian", "optimal_angles", "lw_scattering", "lw_rescaling", "mcica", "switch_fluxes",
        "switch_output_bnd_fluxes", "switch_cloud_optics", "n_bnd_lt_n_gpt")
FORMS = ("per_gpoint", "fractions", "angles", "optimal", "byband", "two_stream", "rescaled")


# the effective flags, as solve_gpu computed them
def broadband(f): return f["broadband_solvers"] and not f["switch_output_bnd_fluxes"]
def byband(f): return f["byband_solvers"] and f["switch_output_bnd_fluxes"] and f["switch_fluxes"] and f["n_bnd_lt_n_gpt"]
def jac(f): return f["jacobian"] and f["switch_fluxes"]
def resc(f): return f["lw_rescaling"] and f["switch_fluxes"]
def scat(f): return (f["lw_scattering"] or f["lw_rescaling"]) and f["switch_fluxes"]


# its refusals, in its order: (predicate, the two setters its message names)
REFUSALS = [
    (lambda f: jac(f) and f["byband_solvers"], ("set_jacobian", "set_byband_solvers")),
    (lambda f: byband(f) and f["n_gauss_angles"] > 1, ("set_gauss_angles", "set_byband_solvers")),
    (lambda f: f["optimal_angles"] and f["n_gauss_angles"] > 1, ("set_optimal_angles", "set_gauss_angles")),
    (lambda f: f["optimal_angles"] and f["byband_solvers"], ("set_optimal_angles", "set_byband_solvers")),
    (lambda f: f["lw_scattering"] and f["n_gauss_angles"] > 1, ("set_lw_scattering", "set_gauss_angles")),
    (lambda f: f["lw_scattering"] and f["optimal_angles"], ("set_lw_scattering", "set_optimal_angles")),
    (lambda f: f["lw_scattering"] and f["jacobian"], ("set_lw_scattering", "set_jacobian")),
    (lambda f: f["lw_scattering"] and f["byband_solvers"], ("set_lw_scattering", "set_byband_solvers")),
    (lambda f: f["lw_scattering"] and f["switch_fluxes"] and not broadband(f), ("set_lw_scattering", "set_broadband_solvers")),
    (lambda f: f["lw_rescaling"] and f["lw_scattering"], ("set_lw_rescaling", "set_lw_scattering")),
    (lambda f: f["lw_rescaling"] and f["n_gauss_angles"] > 1, ("set_lw_rescaling", "set_gauss_angles")),
    (lambda f: f["lw_rescaling"] and f["optimal_angles"], ("set_lw_rescaling", "set_optimal_angles")),
    (lambda f: f["lw_rescaling"] and f["jacobian"], ("set_lw_rescaling", "set_jacobian")),
    (lambda f: f["lw_rescaling"] and f["byband_solvers"], ("set_lw_rescaling", "set_byband_solvers")),
    (lambda f: f["lw_rescaling"] and f["switch_fluxes"] and not broadband(f), ("set_lw_rescaling", "set_broadband_solvers")),
    (lambda f: f["mcica"] and f["lw_scattering"], ("set_cloud_sampling", "set_lw_scattering")),
    (lambda f: f["mcica"] and f["lw_rescaling"], ("set_cloud_sampling", "set_lw_rescaling")),
]


def form(f):
    """the solver a block went to: the by-band branch, then solve_block's chain; the plain rte_lw by what the workspace holds"""
    if byband(f): return "byband"
    if resc(f): return "rescaled"
    if scat(f): return "two_stream"
    if f["optimal_angles"]: return "optimal"
    if not broadband(f): return "per_gpoint"
    return "angles" if f["n_gauss_angles"] > 1 else "fractions"


def test_lw_plan_refuses_and_plans_as_the_if_chain_did():
    lib = ctypes.CDLL(os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so"))
    lib.rrx_host_selftest_lw_plan.argtypes = [ctypes.c_uint, ctypes.c_char_p, ctypes.c_int]
    lib.rrx_host_selftest_lw_plan.restype = ctypes.c_int
    assert len(REFUSALS) == 17
    msg = ctypes.create_string_buffer(512)
    n_refused = 0
    for n_ang in (1, 3):
        for values in itertools.product((False, True), repeat=len(BITS)):
            f = dict(zip(BITS, values), n_gauss_angles=n_ang)
            packed = sum(int(v) << i for i, v in enumerate(values)) | n_ang << len(BITS)
            got = lib.rrx_host_selftest_lw_plan(packed, msg, len(msg))
            holding = [setters for pred, setters in REFUSALS if pred(f)]
            if holding:
                n_refused += 1
                text = msg.value.decode()
                assert got == -1, (f, got)
                assert text.startswith("Radiation_solver_longwave:"), text
                assert any(all(f"({s})" in text for s in setters) for setters in holding), (f, text)
            else:
                want = int(broadband(f)) | int(byband(f)) << 1 | int(jac(f)) << 2 | int(scat(f)) << 3 | FORMS.index(form(f)) << 4
                assert got == want, (f, got, want)
    assert 0 < n_refused < 2 * 2**len(BITS)
