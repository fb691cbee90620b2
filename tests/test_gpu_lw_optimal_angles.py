"""GPU tests of the optimal-angle LW secants (rrx_lw_optimal_secants, rrx_lw_solver_noscat_fractions_optimal): the secants of both
device forms against numpy, the fused entry against the two-step route (producer, then the _angles entry with one angle) over the
tilings and the route outside them, against the CPU oracle, closed forms (tau = 0, opaque columns, a fit that reproduces the fixed
angle), argument errors, and pipeline.ResidentSolver(optimal_angles=True). Inputs, column sets and bounds are those of
tests/test_gpu_lw_angles.py."""
import numpy as np
import pytest

import cases
from rte_rrtmgp_cpp_amd import synthetic, pipeline
from test_gpu_lw_angles import (inputs, Lw, check, backend, _chain, COLUMN_SETS, COLUMN_IDS, F64_FLUX_TOL, F64_FLOOR, F32_FLUX_TOL,
                                F32_FLOOR)

pytestmark = pytest.mark.gpu
NGPT, NBND = 32, 4
LAYERS = [60, 140, 200, 300, 600]      # every tiling of the one-kernel form; 600: the route outside them


def make_fit(seed=77):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.3, 0.3, NBND), rng.uniform(1.5, 1.8, NBND)])


def numpy_secants(I, fit, npdt):
    """D (ngpt, ncol) in float64 from the inputs as the device sees them (tau and fit rounded to the working precision)"""
    S = I["tau"].astype(np.float64).sum(axis=1)
    f = fit.astype(npdt).astype(np.float64)
    b = I["gb"] - 1
    return f[0][b][:, None] * np.exp(-S) + f[1][b][:, None]


def secant_error(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want)))


class Opt(Lw):
    """one input set on the device with one angle and an optimal-angle fit (2, nbnd)"""
    def __init__(self, be, I, top_at_1, with_inc, fit):
        super().__init__(be, I, top_at_1, with_inc, 1)
        self.fit = be.asarray(np.ascontiguousarray(fit.T))          # the C ABI's layout: (2, nbnd), first index fastest
        self.kd.optimal_angle_fit = be.asarray(fit)

    def producer(self):
        return self.be.lw_optimal_secants(self.kd, self.tau, fit=self.fit)

    def fused(self, jacobian, secants=True):
        r = self.be.lw_solver_noscat_fractions_optimal(self.top, self.kd, self.w, self.tau, self.fr, self.emis, fit=self.fit,
                                                       inc_flux=self.inc, jacobian=jacobian, keep_secants=secants)
        return {k: self.be.to_numpy(v) for k, v in r.items()}

    def with_secants(self, sec, jacobian):
        """the _angles entry with one angle and the (ngpt, ncol) secants given"""
        r = self.be.lw_solver_noscat_fractions_angles(self.top, self.kd, sec[None].contiguous(), self.w, self.tau, self.fr, self.emis,
                                                      inc_flux=self.inc, jacobian=jacobian)
        return {k: self.be.to_numpy(v) for k, v in r.items()}


@pytest.mark.parametrize("dt,ncol", COLUMN_SETS, ids=COLUMN_IDS)
@pytest.mark.parametrize("nlay", LAYERS)
@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
@pytest.mark.parametrize("with_inc", [False, True], ids=["noinc", "inc"])
def test_secants_and_fluxes_match_two_step_route(dt, ncol, nlay, top_at_1, with_inc, hip_f64, hip_f32):
    """(1) secants_out and rrx_lw_optimal_secants against numpy (float64 sums, np.exp) within (nlay + 8) eps: with |fit1| <= 0.3,
    D >= 1 and S exp(-S) <= 0.37 a reordered sum of nlay terms and an exp within 2 ulp stay well inside it. (2) the fused entry
    against producer + _angles entry with one angle at the bounds of tests/test_gpu_lw_angles.py; without the Jacobian pair the
    fluxes are the same bits."""
    be, npdt = backend(dt, hip_f64, hip_f32)
    I = inputs(ncol, nlay, NGPT, NBND, seed=nlay + 2*top_at_1 + with_inc + 31, dtype=npdt)
    fit = make_fit()
    lw = Opt(be, I, top_at_1, with_inc, fit)
    want_sec = numpy_secants(I, fit, npdt)
    bound = (nlay + 8) * np.finfo(npdt).eps
    sec = lw.producer()
    got = lw.fused(True)
    e_prod, e_fused = secant_error(be.to_numpy(sec), want_sec), secant_error(got.pop("secants"), want_sec)
    print(f"{dt} ncol={ncol} nlay={nlay}: secants producer {e_prod:.3e} fused {e_fused:.3e} bound {bound:.3e}")
    assert e_prod <= bound and e_fused <= bound
    check(got, lw.with_secants(sec, True), dt, f"{dt} ncol={ncol} nlay={nlay} optimal")
    plain = lw.fused(False, secants=False)
    assert set(plain) == {"flux_up", "flux_dn"}
    for k in plain:
        assert np.array_equal(plain[k], got[k]), k


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
def test_optimal_angles_match_cpu_oracle(dt, top_at_1, hip_f64, hip_f32, oracle_f64, oracle_f32):
    """36 columns x 140 layers: the numpy secants (1, ngpt, ncol) given to the oracle's lw_solver_noscat with the same weight, g-point
    sums in float64; the bounds of test_angles_match_cpu_oracle (1e-9 fp64; 3e-5 fp32 against the fp32 oracle)."""
    (be, npdt), orc = backend(dt, hip_f64, hip_f32), (oracle_f64 if dt == "f64" else oracle_f32)
    I = inputs(36, 140, NGPT, NBND, seed=13 + top_at_1, dtype=npdt)
    fit = make_fit(78)
    lw = Opt(be, I, top_at_1, True, fit)
    got = lw.fused(True, secants=False)
    lay, lev = (be.to_numpy(a) for a in lw.sources())
    sec = np.ascontiguousarray(numpy_secants(I, fit, npdt)[None].astype(npdt))
    o = orc.lw_solver_noscat(bool(top_at_1), orc.asarray(sec), orc.asarray(lw.w_np), I["tau"], lay, lev, I["emis"], I["ssrc"],
                             inc_flux=I["inc"], do_jacobians=True, sfc_src_jac=I["sjac"])
    tol, floor = (1e-9, 1e-6) if dt == "f64" else (3e-5, 1e-2)
    for k in ("flux_up", "flux_dn", "flux_up_jac"):
        want = orc.to_numpy(o[k]).astype(np.float64).sum(axis=0)
        e = cases.rel_err(got[k], want, floor=floor)
        print(f"{dt} optimal angles {k}: {e:.3e}")
        assert e <= tol, (k, e)


@pytest.fixture
def unsplit(hip_f64):
    hip_f64.set_broadband_gsplit(1)
    yield
    hip_f64.set_broadband_gsplit(0)


@pytest.mark.parametrize("dt,ncol", COLUMN_SETS, ids=COLUMN_IDS)
@pytest.mark.parametrize("nlay", LAYERS)
def test_transparent_columns(dt, ncol, nlay, hip_f64, hip_f32, unsplit):
    """tau = 0: D = fit1 + fit2 as the device rounds that sum, in both device forms; the fluxes are those of the _angles entry given
    that constant, bit for bit (one g-point range in both)."""
    be, npdt = backend(dt, hip_f64, hip_f32)
    I = inputs(ncol, nlay, NGPT, NBND, seed=nlay + 3, dtype=npdt)
    I["tau"] = np.zeros_like(I["tau"])
    fit = make_fit()
    lw = Opt(be, I, False, True, fit)
    f = fit.astype(npdt)
    want = np.ascontiguousarray(np.broadcast_to((f[0] + f[1])[I["gb"] - 1][:, None], (NGPT, ncol)))
    assert want.dtype == npdt
    got = lw.fused(True)
    assert np.array_equal(got.pop("secants"), want)
    assert np.array_equal(be.to_numpy(lw.producer()), want)
    ref = lw.with_secants(be.asarray(want), True)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("dt,ncol", COLUMN_SETS, ids=COLUMN_IDS)
@pytest.mark.parametrize("nlay", LAYERS)
def test_opaque_columns(dt, ncol, nlay, hip_f64, hip_f32):
    """tau = 50 in every layer: exp(-S) underflows to zero and D = fit2 exactly, in both device forms"""
    be, npdt = backend(dt, hip_f64, hip_f32)
    I = inputs(ncol, nlay, NGPT, NBND, seed=nlay + 4, dtype=npdt)
    I["tau"] = np.full_like(I["tau"], 50.0)
    fit = make_fit()
    lw = Opt(be, I, True, False, fit)
    want = np.ascontiguousarray(np.broadcast_to(fit.astype(npdt)[1][I["gb"] - 1][:, None], (NGPT, ncol)))
    assert np.array_equal(lw.fused(False)["secants"], want)
    assert np.array_equal(be.to_numpy(lw.producer()), want)


@pytest.mark.parametrize("dt,ncol", COLUMN_SETS, ids=COLUMN_IDS)
@pytest.mark.parametrize("nlay", LAYERS)
def test_constant_fit_is_the_fixed_angle(dt, ncol, nlay, hip_f64, hip_f32, unsplit):
    """fit1 = 0 and fit2 = the Gauss secant of the one-angle solve: the fluxes of rrx_lw_solver_noscat_fractions bit for bit (one
    g-point range in both): the optimal-angle form changes only where D comes from."""
    be, npdt = backend(dt, hip_f64, hip_f32)
    I = inputs(ncol, nlay, NGPT, NBND, seed=nlay + 5, dtype=npdt)
    fit = np.stack([np.zeros(NBND), np.full(NBND, float(np.asarray(pipeline.GAUSS_DS).ravel()[0]))])
    lw = Opt(be, I, False, True, fit)
    got = lw.fused(False)
    assert np.array_equal(got["secants"], be.to_numpy(lw.sec)[0])
    old = be.lw_solver_noscat_fractions(lw.top, lw.kd, lw.sec, lw.w, lw.tau, lw.fr, lw.emis, inc_flux=lw.inc)
    for k in ("flux_up", "flux_dn"):
        assert np.array_equal(got[k], be.to_numpy(old[k])), k


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("case", ["two_weights", "nbnd0", "only_sfc_src_jac", "only_flux_up_jac", "null_fit", "null_flux_up", "null_flux_dn",
                                  "producer_null_secants", "producer_null_fit"])
def test_errors_leave_the_outputs_alone(dt, case, hip_f64, hip_f32):
    from rte_rrtmgp_cpp_amd._ffi import BoolArg
    be, npdt = backend(dt, hip_f64, hip_f32)
    ncol, nlay = 6, 60
    lw = Opt(be, inputs(ncol, nlay, NGPT, NBND, seed=1, dtype=npdt), False, True, make_fit())
    up, dn, jac = (be.empty((nlay+1, ncol)).fill_(-7.0) for _ in range(3))
    sec = be.empty((NGPT, ncol)).fill_(-7.0)
    a = dict(nbnd=NBND, w=lw.w, fit=lw.fit, up=up, dn=dn, sjac=None, jac=None)
    if case == "two_weights":
        with pytest.raises(ValueError):
            be.lw_solver_noscat_fractions_optimal(lw.top, lw.kd, be.asarray(np.array([0.5, 0.5])), lw.tau, lw.fr, lw.emis, fit=lw.fit,
                                                  flux_up=up, flux_dn=dn, secants_out=sec)
    elif case.startswith("producer"):
        with pytest.raises(RuntimeError, match="rrx_lw_optimal_secants"):
            be._c("lw_optimal_secants", ncol, nlay, NGPT, NBND, lw.kd.gpoint_bands, None if case == "producer_null_fit" else lw.fit,
                  lw.tau, None if case == "producer_null_secants" else sec)
    else:
        if case == "nbnd0": a["nbnd"] = 0
        elif case == "only_sfc_src_jac": a["sjac"] = lw.fr["sfc_src_jac"]
        elif case == "only_flux_up_jac": a["jac"] = jac
        elif case == "null_fit": a["fit"] = None
        elif case == "null_flux_up": a["up"] = None
        else: a["dn"] = None
        with pytest.raises(RuntimeError, match="rrx_lw_solver_noscat_fractions_optimal"):
            be._c("lw_solver_noscat_fractions_optimal", ncol, nlay, NGPT, a["nbnd"], BoolArg(lw.top), a["w"], lw.tau, lw.fr["pfrac"],
                  lw.fr["blay"], lw.fr["blev"], lw.kd.gpoint_bands, a["fit"], lw.emis, lw.fr["sfc_src"], lw.inc, a["up"], a["dn"],
                  a["sjac"], a["jac"], sec)
    for t in (up, dn, jac, sec):
        assert bool((t == -7.0).all())


KW = dict(ngpt=32, nbnd=4, npres=20, nflav=4, nminor_lower=9, nminor_upper=5)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("jacobian", [False, True], ids=["fluxes", "jacobian"])
def test_resident_solver_with_optimal_angles(dt, jacobian, hip_f64, hip_f32, monkeypatch):
    """ResidentSolver(optimal_angles=True), 64 columns x 140 layers: LW fluxes and Jacobian are those of the two-step route on the
    step's own tau, SW outputs those of the plain solver bit for bit, LW fluxes differ from the plain solver's; the same with
    sunlit=True; the three refused combinations."""
    be, npdt = backend(dt, hip_f64, hip_f32)
    monkeypatch.setenv("RRX_PAD_COLUMNS", "0")
    kl0 = synthetic.make_kdist("lw", **KW)
    kl, ks = be.upload_kdist(kl0), be.upload_kdist(synthetic.make_kdist("sw", **KW))
    atm = pipeline.upload_atmosphere(be, synthetic.make_atmosphere(64, 140, nbnd_lw=4, nbnd_sw=4, seed=3).astype(npdt))
    sv1 = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", jacobian=jacobian)
    svo = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", jacobian=jacobian, optimal_angles=True,
                                  keep_secants=True)
    F1, Fo = be.to_numpy(sv1.step()).copy(), be.to_numpy(svo.step()).copy()
    assert np.array_equal(Fo[3:], F1[3:])                               # the SW outputs
    assert not np.array_equal(Fo[:2], F1[:2])
    buf = svo.lw
    sec = be.lw_optimal_secants(kl, buf["tau"])
    r = be.lw_solver_noscat_fractions_angles(atm.top_at_1, kl, sec[None].contiguous(), svo.weights, buf["tau"], buf, svo.sfc_emis_gpt,
                                             jacobian=jacobian)
    want = {k: be.to_numpy(v) for k, v in r.items()}
    got = dict(flux_up=Fo[0], flux_dn=Fo[1])
    if jacobian:
        got["flux_up_jac"] = be.to_numpy(svo.lw_flux_up_jac)
    check(got, want, dt, f"{dt} ResidentSolver optimal angles")
    kept, sec_np = be.to_numpy(svo.lw_secants).astype(np.float64), be.to_numpy(sec).astype(np.float64)
    assert np.max(np.abs(kept - sec_np) / sec_np) <= 2 * (140 + 8) * np.finfo(npdt).eps      # (each within (nlay + 8) eps of the exact value)
    fit = kl0.optimal_angle_fit
    assert kept.min() >= (fit[1] - np.abs(fit[0])).min() - 1e-6 and kept.max() <= (fit[1] + np.abs(fit[0])).max() + 1e-6
    svs = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", jacobian=jacobian, optimal_angles=True, sunlit=True)
    sv1s = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", jacobian=jacobian, sunlit=True)
    Fs, F1s = be.to_numpy(svs.step()).copy(), be.to_numpy(sv1s.step()).copy()
    assert np.array_equal(Fs[:3], Fo[:3]) and np.array_equal(Fs[3:], F1s[3:])
    with pytest.raises(ValueError):
        pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, optimal_angles=True, n_gauss_angles=2)
    with pytest.raises(ValueError):
        pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, optimal_angles=True, byband=True)
    bare = be.upload_kdist(synthetic.KDist(**{**kl0.__dict__, "extras": {}}))
    with pytest.raises(ValueError):
        pipeline.ResidentSolver(be, bare, ks, atm, do_broadband=True, optimal_angles=True)


def test_resident_solver_optimal_angles_sorted_and_padded(hip_f64, monkeypatch):
    """ResidentSolver(optimal_angles=True) on 16 385 columns (padded to 16 400) with a surface-pressure spread that switches sorting
    on, against an unsorted, unpadded run at 1e-11; the SW outputs are those of the plain solver bit for bit."""
    be = hip_f64
    atm0, kl0, ks0, _ = _chain(be, 16385, 30, seed=5, spread=True)
    kl, ks = be.upload_kdist(kl0), be.upload_kdist(ks0)
    atm = pipeline.upload_atmosphere(be, atm0)
    monkeypatch.setenv("RRX_PAD_COLUMNS", "0")
    plain = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", jacobian=True, optimal_angles=True)
    assert plain.perm is None
    ref = be.to_numpy(plain.step()).copy()
    ref_jac = be.to_numpy(plain.lw_flux_up_jac).copy()
    monkeypatch.setenv("RRX_PAD_COLUMNS", "1")
    solver = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="auto", jacobian=True, optimal_angles=True)
    assert solver.npad == 15 and solver.sort_columns
    F = be.to_numpy(solver.step()).copy()
    assert F.shape == (7, 31, 16385)
    for i in range(3):
        assert cases.rel_err(F[i], ref[i]) <= 1e-11, i
    assert cases.rel_err(be.to_numpy(solver.lw_flux_up_jac), ref_jac) <= 1e-11
    F1 = be.to_numpy(pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="auto", jacobian=True).step())
    assert np.array_equal(F[3:], F1[3:])
    assert not np.array_equal(F[:2], F1[:2])


@pytest.mark.parametrize("clouds", [False, True], ids=["clear", "allsky"])
def test_cxx_solver_optimal_angles_matches_pipeline(clouds, hip_f64):
    """Radiation_solver_longwave::set_optimal_angles(true) with a column block of 1 000 on 2 500 columns x 30 layers with a pressure
    spread, against ResidentSolver(optimal_angles=True) at 1e-11 (the same kernel); optimal angles are not the fixed angle; more than
    one angle with them is refused at the solve."""
    from rte_rrtmgp_cpp_amd import cxx_driver
    be = hip_f64
    atm0, kl0, ks0, luts0 = _chain(be, 2500, 30, seed=31, clouds=clouds, spread=True)
    luts = None if luts0 is None else tuple(be.upload_lut(l) for l in luts0)
    sv = pipeline.ResidentSolver(be, be.upload_kdist(kl0), be.upload_kdist(ks0), pipeline.upload_atmosphere(be, atm0), do_broadband=True,
                                 cloud_luts=luts, jacobian=True, optimal_angles=True)
    ref = be.to_numpy(sv.step()).copy()
    ref_jac = be.to_numpy(sv.lw_flux_up_jac).copy()
    drv = cxx_driver.CxxDriver(be, kl0, ks0, pipeline.upload_atmosphere(be, atm0), luts0, column_block=1000, jacobian=True,
                               optimal_angles=True)
    try:
        got = be.to_numpy(drv.step()).copy()
        got_jac = be.to_numpy(drv.lw_flux_up_jac).copy()
    finally:
        drv.close()
    one = pipeline.ResidentSolver(be, be.upload_kdist(kl0), be.upload_kdist(ks0), pipeline.upload_atmosphere(be, atm0), do_broadband=True,
                                  cloud_luts=luts)
    assert not np.array_equal(ref[:2], be.to_numpy(one.step())[:2])
    e = max(cases.rel_err(got[i], ref[i]) for i in range(7))
    ej = cases.rel_err(got_jac, ref_jac)
    print(f"CxxDriver optimal angles clouds={clouds}: flux {e:.3e} jac {ej:.3e}")
    assert e <= 1e-11 and ej <= 1e-11
    drv = cxx_driver.CxxDriver(be, kl0, ks0, pipeline.upload_atmosphere(be, atm0), luts0, column_block=1000, optimal_angles=True,
                               n_gauss_angles=2)
    try:
        with pytest.raises(RuntimeError):
            drv.step()
    finally:
        drv.close()
    bare = synthetic.KDist(**{**kl0.__dict__, "extras": {}})
    with pytest.raises(RuntimeError):
        cxx_driver.CxxDriver(be, bare, ks0, pipeline.upload_atmosphere(be, atm0), luts0, optimal_angles=True)


def test_driver_lw_optimal_angles(tmp_path, hip_f64):
    """--lw-optimal-angles with RRX_COL_BLOCK=7 (6 blocks + a residual of 3) on 45 columns x 60 layers against one block and against
    ResidentSolver(optimal_angles=True) at 1e-11; with --lw-gauss-angles 2, with the by-band solvers and on a coefficient file without
    the fit the driver ends with a non-zero status."""
    import os
    from rte_rrtmgp_cpp_amd import synthetic_files, rrxio
    from test_gpu_lw_angles import run_driver, KW as DKW
    d = str(tmp_path / "case")
    kl, ks = synthetic.make_kdist("lw", **DKW), synthetic.make_kdist("sw", **DKW)
    atm = synthetic.make_atmosphere(45, 60, nbnd_lw=DKW["nbnd"], nbnd_sw=DKW["nbnd"], clouds=True, seed=5)
    lut_l, lut_s = synthetic.make_cloud_lut(DKW["nbnd"], "lw"), synthetic.make_cloud_lut(DKW["nbnd"], "sw")
    synthetic_files.write_case(d, atm, kl, ks, lut_l, lut_s)
    outs = []
    for env in ({"RRX_COL_BLOCK": "7"}, None):
        assert run_driver(d, "--cloud-optics", "--lw-optimal-angles", env=env) == 0
        _, v = rrxio.read(os.path.join(d, "rte_rrtmgp_output.nc"))
        outs.append({k: v[k][0].copy() for k in ("lw_flux_up", "lw_flux_dn")})
    for k in outs[0]:
        assert outs[0][k].shape[0] == 61
        assert cases.rel_err(outs[0][k], outs[1][k]) <= 1e-11, k
    be = hip_f64
    luts = (be.upload_lut(lut_l), be.upload_lut(lut_s))
    F = {}
    for opt in (False, True):
        sv = pipeline.ResidentSolver(be, be.upload_kdist(kl), be.upload_kdist(ks), pipeline.upload_atmosphere(be, atm), do_broadband=True,
                                     cloud_luts=luts, optimal_angles=opt)
        F[opt] = be.to_numpy(sv.step()).copy()
    assert not np.array_equal(F[False][0], F[True][0])
    for i, k in enumerate(("lw_flux_up", "lw_flux_dn")):
        assert cases.rel_err(outs[1][k].reshape(F[True][i].shape), F[True][i]) <= 1e-11, k
    assert run_driver(d, "--cloud-optics", "--lw-optimal-angles", "--lw-gauss-angles", "2") != 0
    assert run_driver(d, "--cloud-optics", "--lw-optimal-angles", "--output-bnd-fluxes", "--byband-solvers") != 0
    d2 = str(tmp_path / "nofit")
    synthetic_files.write_case(d2, atm, synthetic.KDist(**{**kl.__dict__, "extras": {}}), ks, lut_l, lut_s)
    assert run_driver(d2, "--cloud-optics") == 0
    assert run_driver(d2, "--cloud-optics", "--lw-optimal-angles") != 0
