"""GPU tests of the rescaled LW no-scattering solver: the general entry (rrx_lw_solver_noscat_rescaled) against the numpy
reference (tests/lw1r_ref.py), the fused Planck-lite entry (rrx_lw_solver_noscat_fractions_rescaled) against the materialised route
on the device and against numpy over its tilings and the route outside them, null clouds against zero clouds and against the
no-scattering solver, the isothermal closure, pipeline.ResidentSolver(lw_rescaling=True), the C++ classes, the driver and the CPU
boundary's do_rescaling.

Tolerances. fp64 against numpy: 1e-10, the project's LW bound (tests/test_gpu_parity.py). Routes of the same arithmetic (fused against
materialised, column blocks against one block, sorted against unsorted): 1e-11. fp32: twice the largest error observed over this file's
grids against the float32 numpy reference (DESIGN 8's rule). The largest error observed on an MI355X stands beside each constant.
Floors of the relative error as in the neighbouring tests: 1e-6 (fp64), 1e-2 (fp32)."""
import types

import numpy as np
import pytest

import cases
import lw1r_ref
from test_gpu_lw_2stream import SIZES, backend, floor, inputs, _chain
from rte_rrtmgp_cpp_amd import synthetic, pipeline

pytestmark = pytest.mark.gpu

# Largest errors observed over the grids of this file on an MI355X (every test prints its own):
#   fp64  general per g-point vs numpy 6.59e-12, general broadband 2.91e-14, fused vs numpy 6.03e-14, CPU boundary 1.06e-12 -> the 1e-10 holds
#         fused vs materialised 9.86e-14, sorted and padded 1.61e-14, C++ classes in blocks 6.69e-15                          -> the 1e-11 holds
#   fp32  broadband: general 1.76e-6, fused vs numpy 2.44e-6 -> 4.9e-6; fused vs materialised 6.18e-7 -> 1.3e-6
#         per g-point 1.88e-4 -> 3.8e-4. Single g-points need more than their sums. Against a longdouble truth per profile
#         (tests/lw1r_truth.py; tests/test_gpu_lw1r_truth.py on an MI355X) the float32 reference is at most 4.7e2 eps = 5.6e-5 of a
#         profile's own flux (seam, just above and below the switch) and the kernels at most 1.8e2 eps = 2.1e-5, each 0.3 ... 1 x the
#         reference's figure in every regime: both carry the same cancellation, so this tolerance is neither's alone -- it is their two
#         roundings of one ill-conditioned factor, in a norm over the array's largest value. How the reference comes by its share:
#         on the same inputs the float32 numpy reference differs from the float64 one by 6.2e-5 ... 2.4e-4 per g-point and by
#         0.9 ... 1.4e-6 broadband. It is the thick branch of the source factor, (1 - tr)/tl - tr, just above tau_thres = eps^(1/4) =
#         0.019: tr carries up to eps, divided by tl and set against fact = tl/2 that is 2 eps/tl^2 <= 6.9e-4 of the layer's source
#         (tests/test_lw1r_ref.py shows it in isolation); nearly transparent g-points consist of such layers, in the sums they vanish
F64_TOL = 1e-10
SAME_TOL = 1e-11
F32_TOL = 4.9e-6
F32_GPT_TOL = 3.8e-4
F32_SAME_TOL = 1.3e-6


def tol(dt):
    return F64_TOL if dt == "f64" else F32_TOL


def same_tol(dt):
    return SAME_TOL if dt == "f64" else F32_SAME_TOL


def with_angles(I, nmus, seed, dtype):
    """secants (nmus, ngpt, ncol) in [1.2, 2.2] and weights in [0.2, 0.6] beside the neighbour's inputs; a Jacobian source"""
    rng = np.random.default_rng(1000 + seed)
    ngpt, _, ncol = I["tau"].shape
    I["sec"] = np.ascontiguousarray(rng.uniform(1.2, 2.2, (nmus, ngpt, ncol)).astype(dtype))
    I["wts"] = rng.uniform(0.2, 0.6, nmus).astype(dtype)
    I["sjac"] = np.ascontiguousarray(rng.uniform(0.1, 0.5, (ngpt, ncol)).astype(dtype))
    return I


class Case:
    """One input set on the device with the routes of this file"""
    def __init__(self, be, I, top_at_1):
        self.be, self.I, self.top = be, I, bool(top_at_1)
        up = be.asarray
        self.tau, self.emis, self.sec, self.wts, self.sjac = up(I["tau"]), up(I["emis"]), up(I["sec"]), up(I["wts"]), up(I["sjac"])
        self.fr = dict(pfrac=up(I["pfrac"]), blay=up(I["blay"]), blev=up(I["blev"]), sfc_src=up(I["ssrc"]))
        self.kd = types.SimpleNamespace(band_lims_gpt=up(I["lims"]), gpoint_bands=up(I["gb"]))
        self.inc = None if I["inc"] is None else up(I["inc"])
        self.cld = (up(I["ct"]), up(I["cw"]), up(I["cg"])) if "ct" in I else None
        self.cld_np = (I["ct"], I["cw"], I["cg"]) if "ct" in I else None

    def fused(self, cloud="own"):
        r = self.be.lw_solver_noscat_fractions_rescaled(self.top, self.kd, self.sec, self.wts, self.tau, self.fr, self.emis,
                                                        cloud=self.cld if cloud == "own" else cloud, inc_flux=self.inc)
        return {k: self.be.to_numpy(v) for k, v in r.items()}

    def materialised(self, do_broadband=True, jac=False):
        """rrx_inc_2stream_by_2stream_bybnd, rrx_planck_sources_from_fractions, the general entry"""
        be = self.be
        tau, ssa, g = self.tau.clone(), be.zeros(tuple(self.tau.shape)), be.zeros(tuple(self.tau.shape))
        if self.cld is not None:
            be.inc_2stream_by_2stream_bybnd(tau, ssa, g, *self.cld, self.kd.band_lims_gpt)
        lay, lev = be.planck_sources_from_fractions(self.kd, self.fr)
        r = be.lw_solver_noscat_rescaled(self.top, self.sec, self.wts, tau, ssa, g, lay, lev, self.emis, self.fr["sfc_src"], inc_flux=self.inc,
                                         do_broadband=do_broadband, do_jacobians=jac, sfc_src_jac=self.sjac if jac else None)
        return {k: be.to_numpy(v) for k, v in r.items()}

    def numpy_gpt(self, jac=False):
        I = self.I
        tau, ssa, g = lw1r_ref.combine(I["tau"], self.cld_np, I["gb"])
        return lw1r_ref.solve(I["sec"], I["wts"], tau, ssa, g, lw1r_ref.layer_sources(I["pfrac"], I["blay"], I["gb"]),
                              lw1r_ref.level_sources(I["pfrac"], I["blev"], I["gb"]), I["emis"], I["ssrc"], I["inc"], self.top,
                              sfc_src_jac=I["sjac"] if jac else None)


def report(label, dt, got, want, keys=("flux_up", "flux_dn")):
    worst = 0.0
    for k, w in zip(keys, want):
        worst = max(worst, cases.rel_err(got[k], w, floor=floor(dt)))
    print(f"LW1R {label}: {worst:.3e}")
    return worst


# (ncol, nlay, top_at_1, nmus, jacobian, inc)
GENERAL = [(45, 5, True, 1, False, True), (46, 5, False, 3, True, False), (45, 60, False, 1, True, True), (46, 60, True, 3, False, True),
           (45, 60, True, 3, True, False), (46, 60, False, 1, False, False)]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ncol,nlay,top_at_1,nmus,jac,inc", GENERAL,
                         ids=[f"{c}x{l}-top{int(t)}-mu{m}-{'jac' if j else 'nojac'}-{'inc' if i else 'noinc'}" for c, l, t, m, j, i in GENERAL])
def test_general_entry_against_numpy(dt, ncol, nlay, top_at_1, nmus, jac, inc, hip_f64, hip_f32):
    """Per g-point and broadband, 1 and 3 angles, with and without the Jacobian and the incident flux, both orientations"""
    be, npdt = backend(dt, hip_f64, hip_f32)
    c = Case(be, with_angles(inputs(ncol, nlay, seed=3*nlay + ncol + nmus, dtype=npdt, inc=inc), nmus, nlay + ncol, npdt), top_at_1)
    want = c.numpy_gpt(jac)
    keys = ("flux_up", "flux_dn") + (("flux_up_jac",) if jac else ())
    tag = f"{dt} {ncol}x{nlay} top{int(top_at_1)} mu{nmus}"
    e_gpt = report(f"{tag} general per g-point vs numpy", dt, c.materialised(do_broadband=False, jac=jac), want, keys)
    # do_broadband: the fluxes are g-point sums, the Jacobian stays per g-point (rrx_lw_solver_noscat's convention)
    want_bb = (lw1r_ref.broadband(want[0]), lw1r_ref.broadband(want[1])) + tuple(want[2:])
    e_bb = report(f"{tag} general broadband vs numpy", dt, c.materialised(do_broadband=True, jac=jac), want_bb, keys)
    assert e_gpt <= (F64_TOL if dt == "f64" else F32_GPT_TOL), e_gpt
    assert e_bb <= tol(dt), e_bb


# (ncol, nlay, top_at_1, clouds, inc): the smallest nlay that reaches each tiling, the same in both precisions --
#   fp64 two waves of 8 x 8 lanes (16 level-lanes), fp32 four waves of 16 x 4 lanes (16 level-lanes): K = 2 (5 layers), 4 (32), 6 (64), 9 (96);
#   fp64 four waves of 8 x 8 lanes, fp32 eight waves of 16 x 4 lanes (32 level-lanes): K = 5 (144), 7 (160), 9 (224);
#   eight waves of 8 x 8 lanes (64 level-lanes): K = 5 (288), 7 (320), 9 (448); 600 layers: outside the tilings (materialised inside).
# The last layer count of a tiling too (143, 287, 575); odd and even column counts, few columns.
FUSED = [(45, 5, True, True, True), (46, 32, False, True, False), (45, 64, True, True, True), (46, 96, False, True, True),
         (45, 143, True, True, False), (45, 144, False, True, True), (6, 160, True, True, True), (46, 224, False, False, True),
         (45, 287, True, True, True), (6, 288, False, True, False), (6, 320, True, True, True), (6, 448, False, True, True),
         (6, 575, True, True, False), (6, 600, False, True, True)]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ncol,nlay,top_at_1,clouds,inc", FUSED,
                         ids=[f"{c}x{l}-top{int(t)}-{'cld' if cl else 'nocld'}-{'inc' if i else 'noinc'}" for c, l, t, cl, i in FUSED])
def test_fused_entry_against_the_materialised_route_and_numpy(dt, ncol, nlay, top_at_1, clouds, inc, hip_f64, hip_f32):
    be, npdt = backend(dt, hip_f64, hip_f32)
    c = Case(be, with_angles(inputs(ncol, nlay, seed=nlay + ncol + top_at_1, dtype=npdt, clouds=clouds, inc=inc), 1, nlay, npdt), top_at_1)
    up, dn = c.numpy_gpt()
    want_bb = (lw1r_ref.broadband(up), lw1r_ref.broadband(dn))
    tag = f"{dt} {ncol}x{nlay} top{int(top_at_1)}"
    dev = c.materialised()
    got = c.fused()
    e_dev = report(f"{tag} fused vs materialised", dt, got, (dev["flux_up"], dev["flux_dn"]))
    e_np = report(f"{tag} fused vs numpy", dt, got, want_bb)
    assert e_dev <= same_tol(dt), e_dev
    assert e_np <= tol(dt), e_np


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("nlay", [140, 600])
def test_null_clouds_are_zero_clouds_bit_for_bit(dt, nlay, hip_f64, hip_f32):
    be, npdt = backend(dt, hip_f64, hip_f32)
    c = Case(be, with_angles(inputs(45, nlay, seed=11, dtype=npdt, clouds=False), 1, 11, npdt), True)
    z = tuple(be.zeros((len(SIZES), nlay, 45)) for _ in range(3))
    a, b = c.fused(cloud=None), c.fused(cloud=z)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("ncol,nlay,top_at_1", [(45, 60, True), (46, 140, False), (6, 300, True), (6, 600, False)])
def test_null_clouds_are_the_no_scattering_solve(ncol, nlay, top_at_1, hip_f64):
    """ssa = 0: st = 1 and Cn = 0, pass 3 reproduces pass 1 -- rrx_lw_solver_noscat_fractions at 1e-13 in fp64"""
    be = hip_f64
    c = Case(be, with_angles(inputs(ncol, nlay, seed=17 + nlay, dtype=np.float64, clouds=False), 1, nlay, np.float64), top_at_1)
    got = c.fused(cloud=None)
    want = be.lw_solver_noscat_fractions(c.top, c.kd, c.sec, c.wts, c.tau, c.fr, c.emis, inc_flux=c.inc)
    e = report(f"f64 {ncol}x{nlay} null clouds vs noscat_fractions", "f64", got, (be.to_numpy(want["flux_up"]), be.to_numpy(want["flux_dn"])))
    assert e <= 1e-13, e


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("nlay,top_at_1", [(60, False), (200, True), (600, True)])
def test_isothermal_closure_through_the_fused_entry(dt, nlay, top_at_1, hip_f64, hip_f32):
    """Every source B per g-point and inc_flux = pi B: every flux is pi * weight * the sum of B, for any tau, ssa, g and emissivity"""
    be, npdt = backend(dt, hip_f64, hip_f32)
    I = with_angles(inputs(45, nlay, seed=7 + nlay, dtype=npdt), 1, nlay, npdt)
    b = np.random.default_rng(nlay).uniform(5., 40., I["tau"].shape[0]).astype(npdt)
    I["pfrac"] = np.ascontiguousarray(np.broadcast_to(b[:, None, None], I["pfrac"].shape))       # the source rides on pfrac, B = 1
    I["blev"] = np.ones_like(I["blev"]); I["blay"] = np.ones_like(I["blay"])
    I["ssrc"] = np.ascontiguousarray(np.broadcast_to(b[:, None], I["ssrc"].shape))
    I["inc"] = (npdt(np.pi) * I["ssrc"]).astype(npdt)
    I["emis"] = np.random.default_rng(1).uniform(0.3, 1.0, I["emis"].shape).astype(npdt)
    got = Case(be, I, top_at_1).fused()
    want = np.full(got["flux_up"].shape, np.pi * float(I["wts"][0]) * b.astype(np.float64).sum())
    e = report(f"{dt} nlay={nlay} isothermal closure", dt, got, (want, want))
    assert e <= tol(dt), e


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_resident_solver_with_lw_rescaling(dt, hip_f64, hip_f32, monkeypatch):
    """ResidentSolver(lw_rescaling=True): its LW fluxes are the fused entry's on the step's own buffers, its SW outputs are the plain
    solver's bit for bit, its LW differs from the no-scattering all-sky result and from the two-stream one; without cloud LUTs it is
    the ssa = 0 solve"""
    be, npdt = backend(dt, hip_f64, hip_f32)
    monkeypatch.setenv("RRX_PAD_COLUMNS", "0")
    atm0, kl0, ks0, luts0 = _chain(64, 140, seed=3)
    kl, ks = be.upload_kdist(kl0), be.upload_kdist(ks0)
    atm = pipeline.upload_atmosphere(be, atm0.astype(npdt))
    luts = tuple(be.upload_lut(l) for l in luts0)
    for overlap in (False, True):
        kw = dict(do_broadband=True, sort_columns="0", cloud_luts=luts, overlap=overlap)
        plain = pipeline.ResidentSolver(be, kl, ks, atm, **kw)
        resc = pipeline.ResidentSolver(be, kl, ks, atm, lw_rescaling=True, **kw)
        F0, F1 = be.to_numpy(plain.step()).copy(), be.to_numpy(resc.step()).copy()
        assert np.array_equal(F1[3:], F0[3:])                            # the SW outputs
        assert cases.rel_err(F1[0], F0[0], floor=floor(dt)) > 1e-4        # clouds scatter: the LW fluxes are others
        cld = be.cloud_optics_2str(luts[0], atm.lwp, atm.iwp, atm.rel, atm.dei)
        want = be.lw_solver_noscat_fractions_rescaled(atm.top_at_1, kl, resc.secants, resc.weights, resc.lw["tau"], resc.lw,
                                                      resc.sfc_emis_gpt, cloud=cld)
        assert np.array_equal(F1[0], be.to_numpy(want["flux_up"])) and np.array_equal(F1[1], be.to_numpy(want["flux_dn"]))
        assert np.array_equal(F1[2], F1[1] - F1[0])
    scat = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", cloud_luts=luts, lw_scattering=True)
    assert cases.rel_err(F1[0], be.to_numpy(scat.step())[0], floor=floor(dt)) > 1e-5
    clear = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", lw_rescaling=True)
    Fc = be.to_numpy(clear.step()).copy()
    want = be.lw_solver_noscat_fractions_rescaled(atm.top_at_1, kl, clear.secants, clear.weights, clear.lw["tau"], clear.lw,
                                                  clear.sfc_emis_gpt, cloud=None)
    assert np.array_equal(Fc[0], be.to_numpy(want["flux_up"])) and np.array_equal(Fc[1], be.to_numpy(want["flux_dn"]))
    sun = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", cloud_luts=luts, sunlit=True, lw_rescaling=True)
    assert np.array_equal(be.to_numpy(sun.step())[:3], F1[:3])


def test_resident_solver_lw_rescaling_sorted_and_padded(hip_f64, monkeypatch):
    """16 385 columns (padded to 16 400) with a surface-pressure spread that switches sorting on, against an unsorted, unpadded run.
    Observed on an MI355X (up, dn, net): 1.3e-15, 1.6e-14, 9.4e-15 against 1e-11."""
    be = hip_f64
    atm0, kl0, ks0, luts0 = _chain(16385, 30, seed=5, spread=True)
    kl, ks = be.upload_kdist(kl0), be.upload_kdist(ks0)
    atm = pipeline.upload_atmosphere(be, atm0)
    luts = tuple(be.upload_lut(l) for l in luts0)
    monkeypatch.setenv("RRX_PAD_COLUMNS", "0")
    plain = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", cloud_luts=luts, lw_rescaling=True)
    assert plain.perm is None
    ref = be.to_numpy(plain.step()).copy()
    monkeypatch.setenv("RRX_PAD_COLUMNS", "1")
    solver = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="auto", cloud_luts=luts, lw_rescaling=True)
    assert solver.npad == 15 and solver.sort_columns
    F = be.to_numpy(solver.step()).copy()
    assert F.shape == (7, 31, 16385)
    errs = [cases.rel_err(F[i], ref[i]) for i in range(3)]
    print("LW1R sorted and padded vs unsorted (up, dn, net):", " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) <= SAME_TOL, errs


def test_resident_solver_refuses_the_pairs_it_cannot_serve(hip_f64):
    be = hip_f64
    atm0, kl0, ks0, _ = _chain(32, 30, seed=1, clouds=False)
    kl0.extras["optimal_angle_fit"] = np.ones((2, 4)) if "optimal_angle_fit" not in kl0.extras else kl0.extras["optimal_angle_fit"]
    kl, ks = be.upload_kdist(kl0), be.upload_kdist(ks0)
    atm = pipeline.upload_atmosphere(be, atm0)
    for kw, word in ((dict(lw_scattering=True), "lw_scattering"), (dict(byband=True), "byband"), (dict(jacobian=True), "jacobian"),
                     (dict(n_gauss_angles=2), "n_gauss_angles"), (dict(optimal_angles=True), "optimal_angles")):
        with pytest.raises(ValueError, match="lw_rescaling.*" + word):
            pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, lw_rescaling=True, **kw)
    with pytest.raises(ValueError, match="lw_rescaling"):
        pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=False, lw_rescaling=True)


def test_cxx_solver_lw_rescaling_matches_pipeline(hip_f64):
    """Radiation_solver_longwave::set_lw_rescaling(true) with a column block of 1 000 on 2 500 columns x 30 layers with a pressure
    spread, against ResidentSolver(lw_rescaling=True) at 1e-11 (the same kernels); without cloud optics it is the ssa = 0 solve; every
    refused pair fails at the solve. Observed on an MI355X: 6.7e-15 at most."""
    from rte_rrtmgp_cpp_amd import cxx_driver
    be = hip_f64
    for clouds in (True, False):
        atm0, kl0, ks0, luts0 = _chain(2500, 30, seed=31, clouds=clouds, spread=True)
        luts = None if luts0 is None else tuple(be.upload_lut(l) for l in luts0)
        sv = pipeline.ResidentSolver(be, be.upload_kdist(kl0), be.upload_kdist(ks0), pipeline.upload_atmosphere(be, atm0), do_broadband=True,
                                     cloud_luts=luts, lw_rescaling=True)
        ref = be.to_numpy(sv.step()).copy()
        drv = cxx_driver.CxxDriver(be, kl0, ks0, pipeline.upload_atmosphere(be, atm0), luts0, column_block=1000, lw_rescaling=True)
        try:
            got = be.to_numpy(drv.step()).copy()
        finally:
            drv.close()
        errs = [cases.rel_err(got[i], ref[i]) for i in range(7)]
        print(f"LW1R CxxDriver clouds={clouds} vs ResidentSolver:", " ".join(f"{e:.3e}" for e in errs))
        assert max(errs) <= SAME_TOL, errs
        if clouds:
            one = pipeline.ResidentSolver(be, be.upload_kdist(kl0), be.upload_kdist(ks0), pipeline.upload_atmosphere(be, atm0),
                                          do_broadband=True, cloud_luts=luts)
            assert cases.rel_err(ref[0], be.to_numpy(one.step())[0]) > 1e-4
    for kw in (dict(lw_scattering=True), dict(n_gauss_angles=2), dict(optimal_angles=True), dict(jacobian=True), dict(broadband=False)):
        drv = cxx_driver.CxxDriver(be, kl0, ks0, pipeline.upload_atmosphere(be, atm0), luts0, column_block=1000, lw_rescaling=True, **kw)
        try:
            with pytest.raises(RuntimeError, match="set_lw_rescaling"):
                drv.step()
        finally:
            drv.close()


def test_driver_lw_rescaling(tmp_path, hip_f64):
    """--lw-rescaling with RRX_COL_BLOCK=7 (6 blocks + a residual of 3) on 45 columns x 60 layers against one block and against
    ResidentSolver(lw_rescaling=True) at 1e-11; every refused pair ends the driver with a non-zero status."""
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
        assert run_driver(d, "--cloud-optics", "--lw-rescaling", env=env) == 0
        _, v = rrxio.read(os.path.join(d, "rte_rrtmgp_output.nc"))
        outs.append({k: v[k][0].copy() for k in ("lw_flux_up", "lw_flux_dn")})
    for k in outs[0]:
        assert outs[0][k].shape[0] == 61
        assert cases.rel_err(outs[0][k], outs[1][k]) <= SAME_TOL, k
    be = hip_f64
    luts = (be.upload_lut(lut_l), be.upload_lut(lut_s))
    F = {}
    for resc in (False, True):
        sv = pipeline.ResidentSolver(be, be.upload_kdist(kl), be.upload_kdist(ks), pipeline.upload_atmosphere(be, atm), do_broadband=True,
                                     cloud_luts=luts, lw_rescaling=resc)
        F[resc] = be.to_numpy(sv.step()).copy()
    assert not np.array_equal(F[False][0], F[True][0])
    for i, k in enumerate(("lw_flux_up", "lw_flux_dn")):
        assert cases.rel_err(outs[1][k].reshape(F[True][i].shape), F[True][i]) <= SAME_TOL, k
    assert run_driver(d, "--cloud-optics", "--lw-rescaling", "--lw-scattering") != 0
    assert run_driver(d, "--cloud-optics", "--lw-rescaling", "--lw-gauss-angles", "2") != 0
    assert run_driver(d, "--cloud-optics", "--lw-rescaling", "--lw-optimal-angles") != 0
    assert run_driver(d, "--cloud-optics", "--lw-rescaling", "--lw-jacobian") != 0
    assert run_driver(d, "--cloud-optics", "--lw-rescaling", "--output-bnd-fluxes", "--byband-solvers") != 0
    assert run_driver(d, "--cloud-optics", "--lw-rescaling", "--output-bnd-fluxes") != 0


@pytest.mark.parametrize("top_at_1,nmus,broadband,jac", [(True, 1, False, False), (False, 3, False, True), (True, 2, True, True),
                                                         (False, 1, True, False)])
def test_cpu_boundary_serves_do_rescaling(top_at_1, nmus, broadband, jac):
    """rte_lw_solver_noscat of the CPU boundary library with do_rescaling set (host arrays in and out), against numpy: n_quad_angs,
    do_broadband and do_jacobians with it; in broadband mode the Jacobian comes back summed over the g-points, like the fluxes"""
    import cpu_boundary
    from rte_rrtmgp_cpp_amd._ffi import BoolArg
    b = cpu_boundary.HipCpuBoundary(np.float64)
    ncol, nlay = 20, 30
    I = with_angles(inputs(ncol, nlay, seed=12 + nmus, dtype=np.float64), nmus, nmus, np.float64)
    ngpt = I["tau"].shape[0]
    tau, ssa, g = lw1r_ref.combine(I["tau"], (I["ct"], I["cw"], I["cg"]), I["gb"])
    tau, ssa, g = (np.ascontiguousarray(a) for a in (tau, ssa, g))
    lay = lw1r_ref.layer_sources(I["pfrac"], I["blay"], I["gb"]); lev = lw1r_ref.level_sources(I["pfrac"], I["blev"], I["gb"])
    want = lw1r_ref.solve(I["sec"], I["wts"], tau, ssa, g, lay, lev, I["emis"], I["ssrc"], I["inc"], top_at_1, sfc_src_jac=I["sjac"])
    if broadband:
        want = tuple(lw1r_ref.broadband(a) for a in want)
    shape = (nlay+1, ncol) if broadband else (ngpt, nlay+1, ncol)
    up = np.zeros(shape); dn = np.zeros(shape); out_jac = np.zeros(shape) if jac else np.zeros(1); dummy = np.zeros(1)
    gpt = (dummy, dummy) if broadband else (up, dn)
    b.lib.call("rte_lw_solver_noscat", ncol, nlay, ngpt, BoolArg(top_at_1), nmus, I["sec"], I["wts"], tau, lay, lev, I["emis"], I["ssrc"],
               I["inc"], *gpt, BoolArg(broadband), up, dn, BoolArg(jac), I["sjac"], out_jac, BoolArg(True), ssa, g)
    got = dict(flux_up=up, flux_dn=dn, flux_up_jac=out_jac)
    keys = ("flux_up", "flux_dn") + (("flux_up_jac",) if jac else ())
    e = report(f"CPU boundary top{int(top_at_1)} mu{nmus} bb{int(broadband)} jac{int(jac)} vs numpy", "f64", got, want, keys)
    assert e <= F64_TOL, e
