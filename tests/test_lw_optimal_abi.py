"""CPU tests of the optimal-angle LW entries (rrx_lw_optimal_secants, rrx_lw_solver_noscat_fractions_optimal): declared in both
precisions and exported, argument checks that answer with the entry's name without a GPU, the forwarders and Python bindings, the
synthetic k-distribution's optimal_angle_fit (every other table bit for bit what it was before the fit existed) and its round trip
through the coefficient file."""
import hashlib
import inspect
import os
import re

import numpy as np
import pytest

import abi

from rte_rrtmgp_cpp_amd import synthetic, synthetic_files, rrxio

ROOT = abi.ROOT
PRODUCER = "rrx_lw_optimal_secants"
SOLVER = "rrx_lw_solver_noscat_fractions_optimal"
SMALL = dict(ngpt=32, nbnd=4, npres=20, nflav=4, nminor_lower=9, nminor_upper=5)

# sha256 over every field of synthetic.make_kdist(...) but the extras that hold the fit (kdist_digest below), computed on the commit before the
# fit was added
PARENT_DIGESTS = {
    ("lw", "default"): "6dbe31077b499a831306385bc6b7a9ce6de856fa9feba6af4f1975b308361c1e",
    ("lw", "small"): "a18dcbeabe9f76fd2af1d84d087e05c1bf92d0efc0de2afe6911fdf5007ce5c1",
    ("sw", "default"): "973cbf1871a13feb4eb5c365a8fd02087da8e73b2a46250f26beda574e6aa46c",
    ("sw", "small"): "b40393fa02793456794a58409d6591e1a5eab199ef73924623813f040fc2e195",
}


def kdist_digest(kd):
    h = hashlib.sha256()
    for k in sorted(kd.__dict__):
        if k == "extras":                                   # (where the fit lives; the parent had no such field)
            continue
        v = kd.__dict__[k]
        h.update(k.encode())
        if isinstance(v, np.ndarray):
            h.update(str(v.dtype).encode()); h.update(str(v.shape).encode()); h.update(np.ascontiguousarray(v).tobytes())
        else:
            h.update(repr(v).encode())
    return h.hexdigest()


@pytest.mark.parametrize("entry", [PRODUCER, SOLVER])
def test_header_declares_the_entries_in_both_precisions(entry):
    assert abi.declares(entry)
    assert "RRX_DECLARE(float" in abi.header_text()


@pytest.mark.parametrize("entry", [PRODUCER, SOLVER])
def test_library_exports_the_entries(entry):
    lib = abi.lib()
    for sfx in abi.SFXS:
        assert lib.has(entry + sfx), entry + sfx


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["ncol0", "nlay0", "ngpt0", "nbnd0", "null_fit", "null_tau", "null_secants"])
def test_producer_rejects_bad_arguments_without_a_gpu(sfx, case):
    """Arguments are checked before any HIP call (host buffers stand in for device pointers: nothing dereferences them)."""
    lib = abi.lib()
    want = {"ncol0": "ncol", "nlay0": "nlay", "ngpt0": "ngpt", "nbnd0": "nbnd", "null_fit": "optimal_angle_fit", "null_tau": "tau",
            "null_secants": "secants"}[case]
    if case.endswith("0"):
        rc, msg = abi.call(lib, PRODUCER, sfx, **{case[:-1]: 0})
    else:
        rc, msg = abi.call(lib, PRODUCER, sfx, null=(want,))
    assert rc == 1
    assert PRODUCER in msg and want in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("case", ["ncol0", "nlay0", "ngpt0", "nbnd0", "null_fit", "null_weights", "null_flux_up", "null_flux_dn",
                                  "only_sfc_src_jac", "only_flux_up_jac"])
def test_solver_rejects_bad_arguments_without_a_gpu(sfx, case):
    lib = abi.lib()
    want = {"ncol0": "ncol", "nlay0": "nlay", "ngpt0": "ngpt", "nbnd0": "nbnd", "null_fit": "optimal_angle_fit",
            "null_weights": "weights", "null_flux_up": "flux_up_loc", "null_flux_dn": "flux_dn_loc", "only_sfc_src_jac": "flux_up_jac",
            "only_flux_up_jac": "sfc_src_jac"}[case]
    null = ["inc_flux", "sfc_src_jac", "flux_up_jac", "secants_out"]          # fluxes only, no flux from above
    extents = {}
    if case.endswith("0"):
        extents[case[:-1]] = 0
    elif case.startswith("only_"):
        null.remove(case[5:])
    else:
        null.append(want)
    rc, msg = abi.call(lib, SOLVER, sfx, null=null, top_at_1=1, **extents)
    assert rc == 1
    assert SOLVER in msg and want in msg, msg


def test_forwarders_and_python_bindings_exist():
    text = open(os.path.join(ROOT, "include", "rte_solver_kernels_cuda.h")).read()
    for name in ("lw_optimal_secants", "lw_solver_noscat_fractions_optimal"):
        assert re.search(r"inline void " + name + r"\s*\(", text), name
        assert re.search(r"RRX_CALL\(rrx_" + name + r"\b", text), name
    src = open(os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "hip_kernels.py")).read()
    assert re.search(r"def lw_optimal_secants\(self", src) and re.search(r"def lw_solver_noscat_fractions_optimal\(self", src)
    from rte_rrtmgp_cpp_amd import pipeline
    params = inspect.signature(pipeline.ResidentSolver.__init__).parameters
    assert "optimal_angles" in params and "keep_secants" in params


@pytest.mark.parametrize("which", ["default", "small"])
def test_synthetic_fit_and_unchanged_tables(which):
    kw = {} if which == "default" else SMALL
    kd = synthetic.make_kdist("lw", **kw)
    fit = kd.optimal_angle_fit
    assert fit.shape == (2, kd.nbnd) and fit.dtype == np.float64
    assert (np.abs(fit[0]) <= 0.3).all() and (fit[1] >= 1.5).all() and (fit[1] <= 1.8).all()
    for trans in (0.0, 1.0):                                  # exp(-S) spans (0, 1]
        D = fit[0]*trans + fit[1]
        assert (D >= 1.2).all() and (D <= 2.1).all()
    assert np.array_equal(fit, synthetic.make_kdist("lw", **kw).optimal_angle_fit)          # seeded
    assert synthetic.make_kdist("sw", **kw).optimal_angle_fit is None
    for kind in ("lw", "sw"):
        assert kdist_digest(synthetic.make_kdist(kind, **kw)) == PARENT_DIGESTS[(kind, which)], kind
    assert np.array_equal(kd.astype(np.float32).optimal_angle_fit, fit.astype(np.float32))


def test_coefficient_file_round_trips_the_fit(tmp_path):
    kl, ks = synthetic.make_kdist("lw", **SMALL), synthetic.make_kdist("sw", **SMALL)
    atm = synthetic.make_atmosphere(5, 12, nbnd_lw=4, nbnd_sw=4)
    d = str(tmp_path / "with")
    synthetic_files.write_case(d, atm, kl, ks)
    dims, v = rrxio.read(os.path.join(d, "coefficients_lw.nc"))
    arr, names = v["optimal_angle_fit"]
    assert names == ["fit_coeffs", "bnd"] and dims["fit_coeffs"] == 2
    assert np.array_equal(arr, kl.optimal_angle_fit)
    _, vs = rrxio.read(os.path.join(d, "coefficients_sw.nc"))
    assert "optimal_angle_fit" not in vs
    # a k-distribution without the fit writes and reads as before
    bare = synthetic.KDist(**{**kl.__dict__, "extras": {}})
    d2 = str(tmp_path / "without")
    synthetic_files.write_case(d2, atm, bare, ks)
    dims2, v2 = rrxio.read(os.path.join(d2, "coefficients_lw.nc"))
    assert "optimal_angle_fit" not in v2 and "fit_coeffs" not in dims2
    assert set(v2) == set(v) - {"optimal_angle_fit"}
    for k in v2:
        assert np.array_equal(v2[k][0], v[k][0]), k


HOSTLIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")
DRIVER = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "test_rte_rrtmgp_gpu")


def test_host_headers_declare_the_optimal_angle_interface():
    inc = lambda *p: open(os.path.join(ROOT, *p)).read()
    gas = inc("include", "Gas_optics_rrtmgp.h")
    assert re.search(r"void\s+compute_optimal_angles\s*\(\s*const\s+Optical_props_arry_gpu&", gas)
    assert re.search(r"bool\s+has_optimal_angle_fit\s*\(", gas)
    rte = inc("include", "Rte_lw.h")
    assert re.search(r"void\s+rte_lw_optimal\s*\(", rte) and re.search(r"void\s+rte_lw_Ds\s*\(", rte)
    assert re.search(r"void\s+set_optimal_angles\s*\(\s*(const\s+)?bool\b", inc("include_test", "Radiation_solver.h"))
    assert re.search(r"\brrx_cxx_lw_optimal_angles\s*\(", inc("include_test", "rrx_cxx_driver.h"))
    from rte_rrtmgp_cpp_amd import cxx_driver
    assert "optimal_angles" in inspect.signature(cxx_driver.CxxDriver.__init__).parameters


def test_host_library_exports_the_optimal_angle_interface():
    import subprocess
    if not os.path.exists(HOSTLIB):
        pytest.fail(f"{HOSTLIB} not built: run __graft_entry__.build()")
    syms = subprocess.run(["nm", "-DC", "--defined-only", HOSTLIB], capture_output=True, text=True).stdout
    for name in (r"\brrx_cxx_lw_optimal_angles\b", r"Rte_lw_gpu::rte_lw_optimal\(", r"Rte_lw_gpu::rte_lw_Ds\(",
                 r"Gas_optics_rrtmgp_gpu::compute_optimal_angles\(", r"Radiation_solver_longwave::set_optimal_angles\("):
        assert re.search(name, syms), name


def test_driver_help_lists_lw_optimal_angles():
    import subprocess
    if not os.path.exists(DRIVER):
        pytest.fail(f"{DRIVER} not built: run __graft_entry__.build()")
    r = subprocess.run([DRIVER, "--help"], capture_output=True, text=True, timeout=60)
    assert "--lw-optimal-angles" in r.stdout + r.stderr
