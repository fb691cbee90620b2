"""GPU tests of the fused broadband LW solver with 2-4 quadrature angles (rrx_lw_solver_noscat_fractions_angles): against the general
route on the same inputs (Planck sources from fractions -> general kernel with nmus angles per g-point -> rrx_sum_broadband) over the
tilings and the route outside them, with a per-column secants array, one angle bit for bit the one-angle entries, against the CPU
oracle, an isothermal column set whose upward flux is known in closed form, and through the layers: pipeline.ResidentSolver
(n_gauss_angles=3), the C++ solver (set_gauss_angles) and the driver (--lw-gauss-angles)."""
import os
import types

import numpy as np
import pytest

import cases
from host_driver import run_driver
from test_gpu_jacobian import _chain
from rte_rrtmgp_cpp_amd import synthetic, synthetic_files, rrxio, pipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def inputs(ncol, nlay, ngpt, nbnd, seed, dtype):
    """the input builder of tests/test_gpu_jacobian.py"""
    rng = np.random.default_rng(seed)
    gb = np.repeat(np.arange(1, nbnd + 1, dtype=np.int32), ngpt // nbnd)
    shp = (ngpt, nlay, ncol)
    d = dict(gb=gb, tau=10.0**rng.uniform(-4, 1.0, shp), pfrac=rng.uniform(0.05, 1.0, shp),
             blay=rng.uniform(5., 40., (nbnd, nlay, ncol)), blev=rng.uniform(5., 40., (nbnd, nlay+1, ncol)),
             emis=rng.uniform(0.8, 1.0, (ngpt, ncol)), ssrc=rng.uniform(5., 40., (ngpt, ncol)),
             sjac=rng.uniform(0.1, 0.6, (ngpt, ncol)), inc=rng.uniform(0., 5., (ngpt, ncol)))
    return {k: (np.ascontiguousarray(v.astype(dtype)) if v.dtype.kind == "f" else v) for k, v in d.items()}

# fp64: the bound tests/test_gpu_parity.py holds the fused LW form to against the per-g-point sum, and the one-angle Jacobian's bound.
F64_FLUX_TOL, F64_JAC_TOL, F64_FLOOR = 1e-10, 1e-12, 1e-6
# fp32 (twice the largest error observed against the general route over the grid of
# test_angles_match_general_route and test_per_column_secants): observed 5.78e-7 on the fluxes, 4.81e-7 on the Jacobian.
F32_FLUX_TOL, F32_JAC_TOL, F32_FLOOR = 2*5.78e-7, 2*4.81e-7, 1e-2

COLUMN_SETS = [("f64", 45), ("f32", 46), ("f32", 45), ("f64", 6), ("f32", 6)]
COLUMN_IDS = ["f64", "f32even", "f32odd", "f64few", "f32few"]


class Lw:
    """one input set on the device, with nmus angles; secants broadcast from the Gauss table or given per column"""
    def __init__(self, be, I, top_at_1, with_inc, nmus, secants=None, weights=None):
        self.be, self.top = be, bool(top_at_1)
        up = be.asarray
        ngpt, nlay, ncol = I["tau"].shape
        self.sec = be.lw_secants_array(ncol, ngpt, nmus, 4, up(pipeline.GAUSS_DS)) if secants is None else up(secants)
        self.w_np = np.ascontiguousarray(pipeline.GAUSS_WTS[nmus-1, :nmus]) if weights is None else weights
        self.w = up(self.w_np)
        self.tau, self.emis = up(I["tau"]), up(I["emis"])
        self.inc = up(I["inc"]) if with_inc else None
        self.fr = dict(pfrac=up(I["pfrac"]), blay=up(I["blay"]), blev=up(I["blev"]), sfc_src=up(I["ssrc"]), sfc_src_jac=up(I["sjac"]))
        self.kd = types.SimpleNamespace(gpoint_bands=up(I["gb"]))

    def angles(self, jacobian):
        r = self.be.lw_solver_noscat_fractions_angles(self.top, self.kd, self.sec, self.w, self.tau, self.fr, self.emis,
                                                      inc_flux=self.inc, jacobian=jacobian)
        return {k: self.be.to_numpy(v) for k, v in r.items()}

    def sources(self):
        return self.be.planck_sources_from_fractions(self.kd, self.fr)

    def general(self):
        """per-g-point fluxes and Jacobian of the general kernel (all angles), summed with rrx_sum_broadband"""
        lay, lev = self.sources()
        r = self.be.lw_solver_noscat(self.top, self.sec, self.w, self.tau, lay, lev, self.emis, self.fr["sfc_src"], inc_flux=self.inc,
                                     do_jacobians=True, sfc_src_jac=self.fr["sfc_src_jac"])
        return {k: self.be.to_numpy(self.be.sum_broadband(v)) for k, v in r.items()}


def errors(got, want, dt):
    floor = F64_FLOOR if dt == "f64" else F32_FLOOR
    e = {k: cases.rel_err(got[k], want[k], floor=floor) for k in got}
    return max(e["flux_up"], e["flux_dn"]), e.get("flux_up_jac", 0.0)


def check(got, want, dt, what):
    for k in got:
        assert np.isfinite(got[k]).all(), (what, k)
    ef, ej = errors(got, want, dt)
    print(f"{what}: flux {ef:.3e} jac {ej:.3e}")
    assert ef <= (F64_FLUX_TOL if dt == "f64" else F32_FLUX_TOL), (what, ef)
    assert ej <= (F64_JAC_TOL if dt == "f64" else F32_JAC_TOL), (what, ej)


def backend(dt, hip_f64, hip_f32):
    return (hip_f64, np.float64) if dt == "f64" else (hip_f32, np.float32)


# 60 / 140 / 200 / 300 layers: every tiling of the one-kernel form; 600: the route outside them (general kernel with nmus angles)
@pytest.mark.parametrize("dt,ncol", COLUMN_SETS, ids=COLUMN_IDS)
@pytest.mark.parametrize("nlay", [60, 140, 200, 300, 600])
@pytest.mark.parametrize("nmus", [2, 3, 4])
@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
@pytest.mark.parametrize("with_inc", [False, True], ids=["noinc", "inc"])
def test_angles_match_general_route(dt, ncol, nlay, nmus, top_at_1, with_inc, hip_f64, hip_f32):
    be, npdt = backend(dt, hip_f64, hip_f32)
    lw = Lw(be, inputs(ncol, nlay, 32, 4, seed=nlay + 2*top_at_1 + with_inc + 7*nmus, dtype=npdt), top_at_1, with_inc, nmus)
    want = lw.general()
    got = lw.angles(True)
    check(got, want, dt, f"{dt} ncol={ncol} nlay={nlay} nmus={nmus}")
    plain = lw.angles(False)                       # without the Jacobian pair: the same fluxes, bit for bit
    assert set(plain) == {"flux_up", "flux_dn"}
    for k in plain:
        assert np.array_equal(plain[k], got[k]), k


@pytest.mark.parametrize("dt,ncol", COLUMN_SETS, ids=COLUMN_IDS)
def test_per_column_secants(dt, ncol, hip_f64, hip_f32):
    """a secants array that differs per column, g-point and angle (as optimal-angle secants would)"""
    be, npdt = backend(dt, hip_f64, hip_f32)
    I = inputs(ncol, 140, 32, 4, seed=5, dtype=npdt)
    sec = np.random.default_rng(6).uniform(1.0, 2.5, (3, 32, ncol)).astype(npdt)
    lw = Lw(be, I, False, True, 3, secants=sec)
    check(lw.angles(True), lw.general(), dt, f"{dt} ncol={ncol} per-column secants")


@pytest.mark.parametrize("dt,ncol", COLUMN_SETS, ids=COLUMN_IDS)
@pytest.mark.parametrize("nlay", [60, 140, 200, 300, 600])
@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
def test_one_angle_is_the_one_angle_entry(dt, ncol, nlay, top_at_1, hip_f64, hip_f32):
    be, npdt = backend(dt, hip_f64, hip_f32)
    lw = Lw(be, inputs(ncol, nlay, 32, 4, seed=nlay + top_at_1, dtype=npdt), top_at_1, True, 1)
    N = be.to_numpy
    old = be.lw_solver_noscat_fractions(lw.top, lw.kd, lw.sec, lw.w, lw.tau, lw.fr, lw.emis, inc_flux=lw.inc)
    new = lw.angles(False)
    for k in ("flux_up", "flux_dn"):
        assert np.array_equal(new[k], N(old[k])), k
    old = be.lw_solver_noscat_fractions_jac(lw.top, lw.kd, lw.sec, lw.w, lw.tau, lw.fr, lw.emis, inc_flux=lw.inc)
    new = lw.angles(True)
    for k in ("flux_up", "flux_dn", "flux_up_jac"):
        assert np.array_equal(new[k], N(old[k])), k


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("nmus", [2, 4])
@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
def test_angles_match_cpu_oracle(dt, nmus, top_at_1, hip_f64, hip_f32, oracle_f64, oracle_f32):
    """Against the oracle's per-g-point fluxes and Jacobian for the same angles, summed over the g-points in float64, at the bounds of
    test_jacobian_matches_cpu_oracle (1e-9 fp64; fp32 against the fp32 oracle, 3e-5)."""
    (be, npdt), orc = backend(dt, hip_f64, hip_f32), (oracle_f64 if dt == "f64" else oracle_f32)
    I = inputs(36, 140, 32, 4, seed=11 + top_at_1 + nmus, dtype=npdt)
    lw = Lw(be, I, top_at_1, True, nmus)
    got = lw.angles(True)
    lay, lev = (be.to_numpy(a) for a in lw.sources())
    sec = orc.lw_secants_array(36, 32, nmus, 4, orc.asarray(pipeline.GAUSS_DS))
    o = orc.lw_solver_noscat(bool(top_at_1), sec, orc.asarray(lw.w_np), I["tau"], lay, lev, I["emis"], I["ssrc"],
                             inc_flux=I["inc"], do_jacobians=True, sfc_src_jac=I["sjac"])
    tol, floor = (1e-9, 1e-6) if dt == "f64" else (3e-5, 1e-2)
    for k in ("flux_up", "flux_dn", "flux_up_jac"):
        want = orc.to_numpy(o[k]).astype(np.float64).sum(axis=0)
        e = cases.rel_err(got[k], want, floor=floor)
        print(f"{dt} nmus={nmus} {k}: {e:.3e}")
        assert e <= tol, (k, e)


@pytest.mark.parametrize("dt,ncol", COLUMN_SETS, ids=COLUMN_IDS)
@pytest.mark.parametrize("nmus", [1, 2, 3, 4])
def test_isothermal_quadrature(dt, ncol, nmus, hip_f64, hip_f32):
    """One Planck value B per column at every layer, level and band, fractions constant with height, a black surface at sfc_src =
    pfrac*B and no incident flux: every angle carries the radiance pfrac*B upward unchanged, so flux_up is
    pi * (sum of the weights) * sum_g pfrac_g * B at every level, whatever the optical depths."""
    be, npdt = backend(dt, hip_f64, hip_f32)
    ngpt, nbnd, nlay = 32, 4, 140
    I = inputs(ncol, nlay, ngpt, nbnd, seed=21 + nmus, dtype=npdt)
    rng = np.random.default_rng(22)
    B = rng.uniform(5., 40., ncol).astype(npdt)
    pf = rng.uniform(0.05, 1.0, (ngpt, 1, ncol)).astype(npdt)
    I["pfrac"] = np.ascontiguousarray(np.broadcast_to(pf, (ngpt, nlay, ncol)))
    I["blay"] = np.ascontiguousarray(np.broadcast_to(B, (nbnd, nlay, ncol)))
    I["blev"] = np.ascontiguousarray(np.broadcast_to(B, (nbnd, nlay+1, ncol)))
    I["ssrc"] = np.ascontiguousarray(pf[:, 0, :] * B[None, :])
    I["emis"] = np.ones((ngpt, ncol), dtype=npdt)
    lw = Lw(be, I, False, False, nmus)
    got = lw.angles(False)["flux_up"]
    w = lw.w_np.astype(npdt).astype(np.float64)                       # the very weights passed in
    want = np.pi * w.sum() * (I["ssrc"].astype(np.float64)).sum(axis=0)
    e = cases.rel_err(got, np.broadcast_to(want, got.shape), floor=F64_FLOOR if dt == "f64" else F32_FLOOR)
    print(f"{dt} ncol={ncol} nmus={nmus} isothermal: {e:.3e}")
    assert e <= (F64_FLUX_TOL if dt == "f64" else F32_FLUX_TOL), e


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("jacobian", [False, True], ids=["fluxes", "jacobian"])
def test_resident_solver_with_three_angles(dt, jacobian, hip_f64, hip_f32, monkeypatch):
    """ResidentSolver(n_gauss_angles=3): its LW fluxes are those of the general route on the step's own gas optics, its SW outputs
    those of the one-angle solver bit for bit; by-band outputs with several angles are refused."""
    from rte_rrtmgp_cpp_amd import synthetic
    be, npdt = backend(dt, hip_f64, hip_f32)
    monkeypatch.setenv("RRX_PAD_COLUMNS", "0")
    kw = dict(ngpt=32, nbnd=4, npres=20, nflav=4, nminor_lower=9, nminor_upper=5)
    kl, ks = be.upload_kdist(synthetic.make_kdist("lw", **kw)), be.upload_kdist(synthetic.make_kdist("sw", **kw))
    atm = pipeline.upload_atmosphere(be, synthetic.make_atmosphere(64, 140, nbnd_lw=4, nbnd_sw=4, seed=3).astype(npdt))
    sv1 = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", jacobian=jacobian)
    sv3 = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", jacobian=jacobian, n_gauss_angles=3)
    F1, F3 = be.to_numpy(sv1.step()).copy(), be.to_numpy(sv3.step()).copy()
    assert np.array_equal(F3[3:], F1[3:])                               # the SW outputs
    assert not np.array_equal(F3[:2], F1[:2])
    buf = sv3.lw
    lay, lev = be.planck_sources_from_fractions(kl, buf)
    r = be.lw_solver_noscat(atm.top_at_1, sv3.secants, sv3.weights, buf["tau"], lay, lev, sv3.sfc_emis_gpt, buf["sfc_src"],
                            do_jacobians=jacobian, sfc_src_jac=buf["sfc_src_jac"] if jacobian else None)
    want = {k: be.to_numpy(be.sum_broadband(v)) for k, v in r.items()}
    got = dict(flux_up=F3[0], flux_dn=F3[1])
    if jacobian:
        got["flux_up_jac"] = be.to_numpy(sv3.lw_flux_up_jac)
    check(got, want, dt, f"{dt} ResidentSolver 3 angles")
    with pytest.raises(ValueError):
        pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, byband=True, n_gauss_angles=3)


def test_resident_solver_three_angles_sorted_and_padded(hip_f64, monkeypatch):
    """ResidentSolver(n_gauss_angles=3) on 16 385 columns (padded to 16 400) with a surface-pressure spread that switches sorting on,
    against an unsorted, unpadded run; the SW outputs are those of one angle bit for bit; by-band outputs are refused."""
    be = hip_f64
    atm0, kl0, ks0, _ = _chain(be, 16385, 30, seed=5, spread=True)
    kl, ks = be.upload_kdist(kl0), be.upload_kdist(ks0)
    atm = pipeline.upload_atmosphere(be, atm0)
    monkeypatch.setenv("RRX_PAD_COLUMNS", "0")
    plain = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", jacobian=True, n_gauss_angles=3)
    assert plain.perm is None
    ref = be.to_numpy(plain.step()).copy()
    ref_jac = be.to_numpy(plain.lw_flux_up_jac).copy()
    monkeypatch.setenv("RRX_PAD_COLUMNS", "1")
    solver = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="auto", jacobian=True, n_gauss_angles=3)
    assert solver.npad == 15 and solver.sort_columns
    F = be.to_numpy(solver.step()).copy()
    assert F.shape == (7, 31, 16385)
    for i in range(3):
        assert cases.rel_err(F[i], ref[i]) <= 1e-11, i
    assert cases.rel_err(be.to_numpy(solver.lw_flux_up_jac), ref_jac) <= 1e-11
    F1 = be.to_numpy(pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="auto", jacobian=True).step())
    assert np.array_equal(F[3:], F1[3:])
    assert not np.array_equal(F[:2], F1[:2])
    with pytest.raises(ValueError):
        pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, byband=True, n_gauss_angles=3)
    with pytest.raises(ValueError):
        pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, n_gauss_angles=5)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_finite_difference_with_three_angles(dt, hip_f64, hip_f32, monkeypatch):
    """As test_finite_difference_through_the_lw_chain (same bounds): t_sfc and t_sfc + 1 K through gas optics, fractions and the
    three-angle solver; only sfc_src depends on t_sfc, so the change of flux_up is the Jacobian to rounding."""
    be, npdt = backend(dt, hip_f64, hip_f32)
    monkeypatch.setenv("RRX_PAD_COLUMNS", "0")
    atm0, kl0, ks0, _ = _chain(be, 64, 140, seed=3)
    atm = pipeline.upload_atmosphere(be, atm0.astype(be.np_dtype))
    sv = pipeline.ResidentSolver(be, be.upload_kdist(kl0), be.upload_kdist(ks0), atm, do_broadband=True, sort_columns="0", jacobian=True,
                                 n_gauss_angles=3)
    F0 = be.to_numpy(sv.step()).copy()
    J = be.to_numpy(sv.lw_flux_up_jac).copy()
    atm.t_sfc.add_(1.0)
    F1 = be.to_numpy(sv.step()).copy()
    tol = 1e-9 if dt == "f64" else 5e-3
    e = np.max(np.abs((F1[0].astype(np.float64) - F0[0]) - J))
    print(f"{dt} finite difference, three angles: {e:.3e}")
    assert e <= tol
    assert np.array_equal(F1[1], F0[1])                              # flux_dn does not depend on t_sfc


@pytest.mark.parametrize("clouds", [False, True], ids=["clear", "allsky"])
@pytest.mark.parametrize("broadband", [True, False], ids=["broadband", "gpt"])
def test_cxx_solver_three_angles_matches_pipeline(clouds, broadband, hip_f64):
    """Radiation_solver_longwave::set_gauss_angles(3) with a column block of 1 000 on 2 500 columns with a pressure spread, against
    ResidentSolver(n_gauss_angles=3): 1e-11 on the broadband solvers (the same kernel), the general-route bound on the per-g-point ones."""
    from rte_rrtmgp_cpp_amd import cxx_driver
    be = hip_f64
    atm0, kl0, ks0, luts0 = _chain(be, 2500, 30, seed=31, clouds=clouds, spread=True)
    sv = pipeline.ResidentSolver(be, be.upload_kdist(kl0), be.upload_kdist(ks0), pipeline.upload_atmosphere(be, atm0), do_broadband=True,
                                 cloud_luts=None if luts0 is None else tuple(be.upload_lut(l) for l in luts0), jacobian=True,
                                 n_gauss_angles=3)
    ref = be.to_numpy(sv.step()).copy()
    ref_jac = be.to_numpy(sv.lw_flux_up_jac).copy()
    drv = cxx_driver.CxxDriver(be, kl0, ks0, pipeline.upload_atmosphere(be, atm0), luts0, column_block=1000, broadband=broadband,
                               jacobian=True, n_gauss_angles=3)
    try:
        got = be.to_numpy(drv.step()).copy()
        got_jac = be.to_numpy(drv.lw_flux_up_jac).copy()
    finally:
        drv.close()
    one = pipeline.ResidentSolver(be, be.upload_kdist(kl0), be.upload_kdist(ks0), pipeline.upload_atmosphere(be, atm0), do_broadband=True,
                                  cloud_luts=None if luts0 is None else tuple(be.upload_lut(l) for l in luts0))
    assert not np.array_equal(ref[:2], be.to_numpy(one.step())[:2])          # (three angles are not one)
    e = max(cases.rel_err(got[i], ref[i]) for i in range(3))
    ej = cases.rel_err(got_jac, ref_jac)
    print(f"CxxDriver three angles clouds={clouds} broadband={broadband}: flux {e:.3e} jac {ej:.3e}")
    assert e <= (1e-11 if broadband else F64_FLUX_TOL)
    assert ej <= (1e-11 if broadband else F64_JAC_TOL)


KW = dict(ngpt=48, nbnd=3, npres=12, nflav=4, nminor_lower=7, nminor_upper=4)


def test_driver_lw_gauss_angles(tmp_path, hip_f64):
    """--lw-gauss-angles 3 with RRX_COL_BLOCK=7 (6 blocks + a residual of 3) against one block and against
    ResidentSolver(n_gauss_angles=3); 5 angles, and 3 angles with the by-band solvers, end with a non-zero status."""
    d = str(tmp_path)
    kl, ks = synthetic.make_kdist("lw", **KW), synthetic.make_kdist("sw", **KW)
    atm = synthetic.make_atmosphere(45, 60, nbnd_lw=KW["nbnd"], nbnd_sw=KW["nbnd"], clouds=True, seed=5)
    synthetic_files.write_case(d, atm, kl, ks, synthetic.make_cloud_lut(KW["nbnd"], "lw"), synthetic.make_cloud_lut(KW["nbnd"], "sw"))
    outs = []
    for env in ({"RRX_COL_BLOCK": "7"}, None):
        assert run_driver(d, "--cloud-optics", "--lw-gauss-angles", "3", env=env) == 0
        _, v = rrxio.read(os.path.join(d, "rte_rrtmgp_output.nc"))
        outs.append({k: v[k][0].copy() for k in ("lw_flux_up", "lw_flux_dn")})
    for k in outs[0]:
        assert outs[0][k].shape[0] == 61
        assert cases.rel_err(outs[0][k], outs[1][k]) <= 1e-11, k
    be = hip_f64
    luts = (be.upload_lut(synthetic.make_cloud_lut(KW["nbnd"], "lw")), be.upload_lut(synthetic.make_cloud_lut(KW["nbnd"], "sw")))
    F = {}
    for n in (1, 3):
        sv = pipeline.ResidentSolver(be, be.upload_kdist(kl), be.upload_kdist(ks), pipeline.upload_atmosphere(be, atm), do_broadband=True,
                                     cloud_luts=luts, n_gauss_angles=n)
        F[n] = be.to_numpy(sv.step()).copy()
    assert not np.array_equal(F[1][0], F[3][0])
    for i, k in enumerate(("lw_flux_up", "lw_flux_dn")):
        assert cases.rel_err(outs[1][k].reshape(F[3][i].shape), F[3][i]) <= 1e-11, k
    assert run_driver(d, "--cloud-optics", "--lw-gauss-angles=3") == 0
    assert run_driver(d, "--cloud-optics", "--lw-gauss-angles", "5") != 0
    assert run_driver(d, "--cloud-optics", "--lw-gauss-angles", "3", "--output-bnd-fluxes", "--byband-solvers") != 0
