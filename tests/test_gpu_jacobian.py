"""GPU tests of the surface-temperature Jacobian of the LW upward flux (rrx_lw_solver_noscat_fractions_jac, rrx_lw_flux_up_adjust):
against the general kernel's per-g-point Jacobian + rrx_sum_broadband on the same inputs over the tilings (and the route outside them),
against the CPU oracle, fluxes bit for bit those of rrx_lw_solver_noscat_fractions, a finite difference through the whole LW chain,
and through pipeline.ResidentSolver(jacobian=True), the C++ solver (set_jacobian) and the driver (--lw-jacobian)."""
import os
import types

import numpy as np
import pytest

import cases
from host_driver import run_driver
from rte_rrtmgp_cpp_amd import synthetic, synthetic_files, rrxio, pipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def inputs(ncol, nlay, ngpt, nbnd, seed, dtype):
    rng = np.random.default_rng(seed)
    gb = np.repeat(np.arange(1, nbnd + 1, dtype=np.int32), ngpt // nbnd)
    shp = (ngpt, nlay, ncol)
    d = dict(gb=gb, tau=10.0**rng.uniform(-4, 1.0, shp), pfrac=rng.uniform(0.05, 1.0, shp),
             blay=rng.uniform(5., 40., (nbnd, nlay, ncol)), blev=rng.uniform(5., 40., (nbnd, nlay+1, ncol)),
             emis=rng.uniform(0.8, 1.0, (ngpt, ncol)), ssrc=rng.uniform(5., 40., (ngpt, ncol)),
             sjac=rng.uniform(0.1, 0.6, (ngpt, ncol)), inc=rng.uniform(0., 5., (ngpt, ncol)))
    return {k: (np.ascontiguousarray(v.astype(dtype)) if v.dtype.kind == "f" else v) for k, v in d.items()}


class Lw:
    def __init__(self, be, I, top_at_1, with_inc):
        self.be, self.top = be, bool(top_at_1)
        up = be.asarray
        ngpt, nlay, ncol = I["tau"].shape
        self.sec = be.lw_secants_array(ncol, ngpt, 1, 4, up(pipeline.GAUSS_DS))
        self.w = up(np.array([1.0]))
        self.tau, self.emis = up(I["tau"]), up(I["emis"])
        self.inc = up(I["inc"]) if with_inc else None
        self.gb = up(I["gb"])
        self.fr = dict(pfrac=up(I["pfrac"]), blay=up(I["blay"]), blev=up(I["blev"]), sfc_src=up(I["ssrc"]), sfc_src_jac=up(I["sjac"]))
        self.kd = types.SimpleNamespace(gpoint_bands=self.gb)

    def jac(self):
        r = self.be.lw_solver_noscat_fractions_jac(self.top, self.kd, self.sec, self.w, self.tau, self.fr, self.emis, inc_flux=self.inc)
        return {k: self.be.to_numpy(v) for k, v in r.items()}

    def plain(self):
        r = self.be.lw_solver_noscat_fractions(self.top, self.kd, self.sec, self.w, self.tau, self.fr, self.emis, inc_flux=self.inc)
        return {k: self.be.to_numpy(v) for k, v in r.items()}

    def sources(self):
        return self.be.planck_sources_from_fractions(self.kd, self.fr)

    def general(self):
        """the general kernel's per-g-point Jacobian, summed with rrx_sum_broadband"""
        lay, lev = self.sources()
        r = self.be.lw_solver_noscat(self.top, self.sec, self.w, self.tau, lay, lev, self.emis, self.fr["sfc_src"], inc_flux=self.inc,
                                     do_jacobians=True, sfc_src_jac=self.fr["sfc_src_jac"])
        return self.be.to_numpy(self.be.sum_broadband(r["flux_up_jac"]))


# 60 / 140 / 200 / 300 layers: every tiling of the one-kernel form; 600: the route outside them
@pytest.mark.parametrize("dt,ncol", [("f64", 45), ("f32", 46), ("f32", 45), ("f64", 6), ("f32", 6)],
                         ids=["f64", "f32even", "f32odd", "f64few", "f32few"])
@pytest.mark.parametrize("nlay", [60, 140, 200, 300, 600])
@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
@pytest.mark.parametrize("with_inc", [False, True], ids=["noinc", "inc"])
def test_jacobian_matches_general_kernel_and_fluxes_are_bit_identical(dt, ncol, nlay, top_at_1, with_inc, hip_f64, hip_f32):
    be = hip_f64 if dt == "f64" else hip_f32
    I = inputs(ncol, nlay, 32, 4, seed=nlay + 2*top_at_1 + with_inc, dtype=np.float64 if dt == "f64" else np.float32)
    lw = Lw(be, I, top_at_1, with_inc)
    got = lw.jac()
    want = lw.general()
    assert np.isfinite(got["flux_up_jac"]).all() and got["flux_up_jac"].min() >= 0      # (fp32: underflows to 0 near the top)
    tol, floor = (1e-12, 1e-6) if dt == "f64" else (1e-5, 1e-2)
    assert cases.rel_err(got["flux_up_jac"], want, floor=floor) <= tol
    plain = lw.plain()
    for k in ("flux_up", "flux_dn"):
        assert np.array_equal(got[k], plain[k]), k


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
def test_jacobian_matches_cpu_oracle(dt, top_at_1, hip_f64, hip_f32, oracle_f64, oracle_f32):
    """Against the oracle's per-g-point Jacobian summed over the g-points, at the bounds of the LW parity tests (1e-9 fp64; fp32
    against the fp32 oracle, 3e-5)."""
    be, orc = (hip_f64, oracle_f64) if dt == "f64" else (hip_f32, oracle_f32)
    I = inputs(36, 140, 32, 4, seed=11 + top_at_1, dtype=np.float64 if dt == "f64" else np.float32)
    lw = Lw(be, I, top_at_1, True)
    got = lw.jac()
    lay, lev = (be.to_numpy(a) for a in lw.sources())
    sec = orc.lw_secants_array(36, 32, 1, 4, orc.asarray(pipeline.GAUSS_DS))
    o = orc.lw_solver_noscat(bool(top_at_1), sec, orc.asarray(np.array([1.0])), I["tau"], lay, lev, I["emis"], I["ssrc"],
                             inc_flux=I["inc"], do_jacobians=True, sfc_src_jac=I["sjac"])
    want = orc.to_numpy(o["flux_up_jac"]).astype(np.float64).sum(axis=0)
    tol, floor = (1e-9, 1e-6) if dt == "f64" else (3e-5, 1e-2)
    assert cases.rel_err(got["flux_up_jac"], want, floor=floor) <= tol


def _chain(be, ncol, nlay, seed, clouds=False, spread=False):
    kw = dict(ngpt=32, nbnd=4, npres=20, nflav=4, nminor_lower=9, nminor_upper=5)
    kl0, ks0 = synthetic.make_kdist("lw", **kw), synthetic.make_kdist("sw", **kw)
    atm0 = synthetic.make_atmosphere(ncol, nlay, nbnd_lw=4, nbnd_sw=4, clouds=clouds, seed=seed)
    if spread:
        f = np.random.default_rng(seed + 1).uniform(0.65, 1.35, ncol)
        atm0.p_lay = np.ascontiguousarray(atm0.p_lay * f); atm0.p_lev = np.ascontiguousarray(atm0.p_lev * f)
    luts0 = (synthetic.make_cloud_lut(4, "lw"), synthetic.make_cloud_lut(4, "sw")) if clouds else None
    return atm0, kl0, ks0, luts0


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_finite_difference_through_the_lw_chain(dt, hip_f64, hip_f32, monkeypatch):
    """Gas optics, Planck fractions and the solver at t_sfc and t_sfc + 1 K, nothing else changed: only sfc_src depends on t_sfc, so
    the change of flux_up is the Jacobian to rounding."""
    be = hip_f64 if dt == "f64" else hip_f32
    monkeypatch.setenv("RRX_PAD_COLUMNS", "0")
    atm0, kl0, ks0, _ = _chain(be, 64, 140, seed=3)
    atm = pipeline.upload_atmosphere(be, atm0.astype(be.np_dtype))
    sv = pipeline.ResidentSolver(be, be.upload_kdist(kl0), be.upload_kdist(ks0), atm, do_broadband=True, sort_columns="0", jacobian=True)
    F0 = be.to_numpy(sv.step()).copy()
    J = be.to_numpy(sv.lw_flux_up_jac).copy()
    atm.t_sfc.add_(1.0)
    F1 = be.to_numpy(sv.step()).copy()
    tol = 1e-9 if dt == "f64" else 5e-3
    assert np.max(np.abs((F1[0].astype(np.float64) - F0[0]) - J)) <= tol
    assert np.array_equal(F1[1], F0[1])                              # flux_dn does not depend on t_sfc


@pytest.mark.parametrize("with_net", [True, False], ids=["net", "nonet"])
def test_flux_up_adjust_matches_numpy(with_net, hip_f64):
    be = hip_f64
    rng = np.random.default_rng(4)
    nlev, ncol = 41, 37
    jac, up, net = (rng.uniform(0.1, 1.0, (nlev, ncol)), rng.uniform(200., 400., (nlev, ncol)), rng.uniform(-100., 0., (nlev, ncol)))
    t0, t1 = rng.uniform(270., 300., ncol), rng.uniform(270., 300., ncol)
    up_d, net_d = be.asarray(up), be.asarray(net)
    be.lw_flux_up_adjust(be.asarray(jac), be.asarray(t0), be.asarray(t1), up_d, net_d if with_net else None)
    d = jac * (t1 - t0)[None, :]
    # (to rounding: the device may form up + jac*dt with one fused multiply-add)
    assert cases.rel_err(be.to_numpy(up_d), up + d) <= 1e-15
    if with_net:
        assert cases.rel_err(be.to_numpy(net_d), net - d) <= 1e-15
    else:
        assert np.array_equal(be.to_numpy(net_d), net)


def test_resident_solver_jacobian_sorted_and_padded(hip_f64, monkeypatch):
    """ResidentSolver(jacobian=True) on 16 385 columns (padded to 16 400) with a surface-pressure spread that switches sorting on: the
    Jacobian in the caller's column order against an unsorted, unpadded run; the seven fluxes bit for bit those of jacobian=False."""
    be = hip_f64
    atm0, kl0, ks0, _ = _chain(be, 16385, 30, seed=5, spread=True)
    kl, ks = be.upload_kdist(kl0), be.upload_kdist(ks0)
    atm = pipeline.upload_atmosphere(be, atm0)
    monkeypatch.setenv("RRX_PAD_COLUMNS", "0")
    plain = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", jacobian=True)
    assert plain.perm is None
    plain.step()
    ref = be.to_numpy(plain.lw_flux_up_jac).copy()
    monkeypatch.setenv("RRX_PAD_COLUMNS", "1")
    solver = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="auto", jacobian=True)
    assert solver.npad == 15 and solver.sort_columns
    F = be.to_numpy(solver.step()).copy()
    got = be.to_numpy(solver.lw_flux_up_jac)
    assert got.shape == (31, 16385)
    assert cases.rel_err(got, ref) <= 1e-11
    F_nojac = be.to_numpy(pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="auto").step())
    assert np.array_equal(F, F_nojac)
    with pytest.raises(ValueError):
        pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, byband=True, jacobian=True)
    with pytest.raises(ValueError):
        pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=False, jacobian=True)


@pytest.mark.parametrize("clouds", [False, True], ids=["clear", "allsky"])
@pytest.mark.parametrize("broadband", [True, False], ids=["broadband", "gpt"])
def test_cxx_solver_jacobian_matches_pipeline(clouds, broadband, hip_f64, monkeypatch):
    """Radiation_solver_longwave::set_jacobian with a column block of 1 000 on 2 500 columns with a pressure spread (sorted and padded on
    the device), broadband and per-g-point solvers, against ResidentSolver(jacobian=True)."""
    from rte_rrtmgp_cpp_amd import cxx_driver
    be = hip_f64
    atm0, kl0, ks0, luts0 = _chain(be, 2500, 30, seed=31, clouds=clouds, spread=True)
    sv = pipeline.ResidentSolver(be, be.upload_kdist(kl0), be.upload_kdist(ks0), pipeline.upload_atmosphere(be, atm0), do_broadband=True,
                                 cloud_luts=None if luts0 is None else tuple(be.upload_lut(l) for l in luts0), jacobian=True)
    sv.step()
    ref = be.to_numpy(sv.lw_flux_up_jac).copy()
    drv = cxx_driver.CxxDriver(be, kl0, ks0, pipeline.upload_atmosphere(be, atm0), luts0, column_block=1000, broadband=broadband,
                               jacobian=True)
    try:
        drv.step()
        got = be.to_numpy(drv.lw_flux_up_jac).copy()
    finally:
        drv.close()
    assert cases.rel_err(got, ref) <= 1e-11


KW = dict(ngpt=48, nbnd=3, npres=12, nflav=4, nminor_lower=7, nminor_upper=4)


def test_driver_lw_jacobian(tmp_path, hip_f64):
    """--lw-jacobian with RRX_COL_BLOCK=7 (6 blocks + a residual of 3) against one block and against ResidentSolver(jacobian=True);
    with --byband-solvers the driver fails."""
    d = str(tmp_path)
    kl, ks = synthetic.make_kdist("lw", **KW), synthetic.make_kdist("sw", **KW)
    atm = synthetic.make_atmosphere(45, 60, nbnd_lw=KW["nbnd"], nbnd_sw=KW["nbnd"], clouds=True, seed=5)
    synthetic_files.write_case(d, atm, kl, ks, synthetic.make_cloud_lut(KW["nbnd"], "lw"), synthetic.make_cloud_lut(KW["nbnd"], "sw"))
    outs = []
    for env in ({"RRX_COL_BLOCK": "7"}, None):
        assert run_driver(d, "--cloud-optics", "--lw-jacobian", env=env) == 0
        _, v = rrxio.read(os.path.join(d, "rte_rrtmgp_output.nc"))
        outs.append(v["lw_flux_up_jac"][0].copy())
    assert outs[0].shape[0] == 61
    assert cases.rel_err(outs[0], outs[1]) <= 1e-11
    assert run_driver(d, "--cloud-optics", "--lw-jacobian", "--no-broadband-solvers", env={"RRX_COL_BLOCK": "7"}) == 0
    _, v = rrxio.read(os.path.join(d, "rte_rrtmgp_output.nc"))
    assert cases.rel_err(v["lw_flux_up_jac"][0], outs[1]) <= 1e-11
    be = hip_f64
    sv = pipeline.ResidentSolver(be, be.upload_kdist(kl), be.upload_kdist(ks), pipeline.upload_atmosphere(be, atm), do_broadband=True,
                                 cloud_luts=(be.upload_lut(synthetic.make_cloud_lut(KW["nbnd"], "lw")),
                                             be.upload_lut(synthetic.make_cloud_lut(KW["nbnd"], "sw"))), jacobian=True)
    sv.step()
    ref = be.to_numpy(sv.lw_flux_up_jac)
    assert cases.rel_err(outs[1].reshape(ref.shape), ref) <= 1e-11
    assert run_driver(d, "--cloud-optics", "--lw-jacobian", "--output-bnd-fluxes", "--byband-solvers") != 0
