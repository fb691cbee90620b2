"""GPU tests of the LW two-stream solver with scattering: the general entry (rrx_lw_solver_2stream) against the numpy reference
(tests/lw2s_ref.py), the fused Planck-lite entry (rrx_lw_solver_2stream_fractions) against the materialised route on the device and
against numpy over its tilings and the route outside them, the isothermal closure, null clouds against zero clouds, and
pipeline.ResidentSolver(lw_scattering=True).

Tolerances. fp64: 1e-10, what tests/test_gpu_parity.py holds the fused LW form to; the largest error observed over this
grid is written beside each constant. fp32: twice the largest error observed over this grid against the float32 numpy reference
(DESIGN 8's rule). Floors of the relative error as in the neighbouring tests: 1e-6 (fp64), 1e-2 (fp32)."""
import types

import numpy as np
import pytest

import cases
import lw2s_ref
from test_gpu_byband import band_layout
from rte_rrtmgp_cpp_amd import synthetic, pipeline

pytestmark = pytest.mark.gpu

SIZES = [5, 11, 16]                      # 32 g-points in three uneven bands
F64_FLOOR, F32_FLOOR = 1e-6, 1e-2
# Largest errors observed over the grids of this file on an MI355X (every test prints its own):
#   fp64  fused vs materialised 8.4e-16, fused vs numpy 3.3e-13, general broadband vs numpy 3.3e-13    -> the 1e-10 holds
#         general per g-point vs numpy 1.09e-8: single g-points whose flux is 1e-6 of the largest carry the absolute error of the thin
#         layers' source terms AS THE REFERENCE EVALUATES THEM (Z = (lev_bot - lev_top)/(tau (gamma1 + gamma2)) reaches 1e5 at
#         tau = 1e-4 and Z (1 + Rdif - Tdif) cancels to rounding). The kernels evaluate the same terms regrouped, without that
#         cancellation -> twice the 1.02e-8 first observed; not widened since
#   fp32  broadband: general 1.83e-4, fused vs materialised 5.1e-7, fused vs numpy 1.83e-4 -> 3.7e-4; per g-point 4.51e-2 -> 9.1e-2
#   Whose error the two per-g-point figures are, measured against a longdouble truth per profile (tests/lw2s_truth.py,
#   tests/test_lw2s_truth.py on a CPU, tests/test_gpu_lw2s_truth.py on an MI355X; eps of the dtype, worst over its regimes and shapes): on
#   thin g-points (tau 1e-8 ... 1e-4) this reference is 2e6 ... 8e10 eps from truth in fp64 and 3e6 ... 5e10 eps in fp32, i.e. up to 2e-5
#   and of order one of the g-point's own flux; the general kernel is at 1e2 ... 2e2 eps where a flux is lit and at 6e3 ... 3e4 eps where
#   flux_dn is layer emission alone, within 1.5 x of the regrouped formula in numpy. So all but 6e-12 (fp64) and 3e-3 (fp32; dark thin
#   flux_dn only) of a thin profile's flux in these two tolerances is the as-written reference's share, the rest the regrouped formula's, which the kernel
#   reproduces; in the norm of this file they say nothing about a thin g-point, and tests/test_gpu_lw2s_truth.py is what holds those.
F64_TOL = 1e-10
F64_GPT_TOL = 2.1e-8
F32_TOL = 3.7e-4
F32_GPT_TOL = 9.1e-2


def backend(dt, hip_f64, hip_f32):
    return (hip_f64, np.float64) if dt == "f64" else (hip_f32, np.float32)


def tol(dt):
    return F64_TOL if dt == "f64" else F32_TOL


def floor(dt):
    return F64_FLOOR if dt == "f64" else F32_FLOOR


def inputs(ncol, nlay, seed, dtype, clouds=True, inc=True):
    """The builder of tests/test_gpu_byband.py with band clouds: tau in 10^[-4, 1.5] plus a few cells at 0 and 1e-9, cloud tau zero in
    most cells, ssa_c in [0, 0.999999], g_c in [-0.3, 0.9]"""
    rng = np.random.default_rng(seed)
    lims, gb = band_layout(SIZES)
    ngpt, nbnd = len(gb), len(SIZES)
    shp, bshp = (ngpt, nlay, ncol), (nbnd, nlay, ncol)
    tau = 10.0**rng.uniform(-4, 1.5, shp)
    tau[rng.uniform(size=shp) < 0.01] = 0.0
    tau[rng.uniform(size=shp) < 0.01] = 1e-9
    d = dict(lims=lims, gb=gb, tau=tau, pfrac=rng.uniform(0.05, 1.0, shp), blay=rng.uniform(5., 40., bshp),
             blev=rng.uniform(5., 40., (nbnd, nlay+1, ncol)), emis=rng.uniform(0.8, 1.0, (ngpt, ncol)), ssrc=rng.uniform(5., 40., (ngpt, ncol)),
             inc=rng.uniform(0., 5., (ngpt, ncol)) if inc else None)
    if clouds:
        d.update(ct=np.where(rng.uniform(size=bshp) < 0.8, 0.0, 10.0**rng.uniform(-2, 1.5, bshp)),
                 cw=rng.uniform(0., 0.999999, bshp), cg=rng.uniform(-0.3, 0.9, bshp))
    return {k: (np.ascontiguousarray(v.astype(dtype)) if (v is not None and v.dtype.kind == "f") else v) for k, v in d.items()}


class Case:
    """One input set on the device with the routes of this file"""
    def __init__(self, be, I, top_at_1):
        self.be, self.I, self.top = be, I, bool(top_at_1)
        up = be.asarray
        self.tau, self.emis = up(I["tau"]), up(I["emis"])
        self.fr = dict(pfrac=up(I["pfrac"]), blay=up(I["blay"]), blev=up(I["blev"]), sfc_src=up(I["ssrc"]))
        self.kd = types.SimpleNamespace(band_lims_gpt=up(I["lims"]), gpoint_bands=up(I["gb"]))
        self.inc = None if I["inc"] is None else up(I["inc"])
        self.cld = (up(I["ct"]), up(I["cw"]), up(I["cg"])) if "ct" in I else None
        self.cld_np = (I["ct"], I["cw"], I["cg"]) if "ct" in I else None

    def fused(self, cloud="own"):
        r = self.be.lw_solver_2stream_fractions(self.top, self.kd, self.tau, self.fr, self.emis, cloud=self.cld if cloud == "own" else cloud,
                                                inc_flux=self.inc)
        return {k: self.be.to_numpy(v) for k, v in r.items()}

    def materialised(self, do_broadband=True):
        """route (b): rrx_inc_2stream_by_2stream_bybnd, rrx_planck_sources_from_fractions, the general entry"""
        be = self.be
        tau, ssa, g = self.tau.clone(), be.zeros(tuple(self.tau.shape)), be.zeros(tuple(self.tau.shape))
        if self.cld is not None:
            be.inc_2stream_by_2stream_bybnd(tau, ssa, g, *self.cld, self.kd.band_lims_gpt)
        _, lev = be.planck_sources_from_fractions(self.kd, self.fr)
        r = be.lw_solver_2stream(self.top, tau, ssa, g, lev, self.emis, self.fr["sfc_src"], inc_flux=self.inc, do_broadband=do_broadband)
        return {k: be.to_numpy(v) for k, v in r.items()}

    def numpy_gpt(self):
        I = self.I
        tau, ssa, g = lw2s_ref.combine(I["tau"], self.cld_np, I["gb"])
        return lw2s_ref.solve(tau, ssa, g, lw2s_ref.level_sources(I["pfrac"], I["blev"], I["gb"]), I["emis"], I["ssrc"], I["inc"], self.top)


def report(label, dt, got, want):
    worst = 0.0
    for k, w in zip(("flux_up", "flux_dn"), want):
        e = cases.rel_err(got[k], w, floor=floor(dt))
        worst = max(worst, e)
    print(f"LW2S {label}: {worst:.3e}")
    return worst


# (ncol, nlay, top_at_1, clouds, inc): the smallest shapes that reach every tiling -- fp64 K = 4 / 9 / 12 of two waves (60, 140, 180
# layers; K = 6 at 80), four waves (200) and eight (K = 5 at 300, 7 at 400, 9 at 500); fp32 one and two groups per workgroup (60 / 140, 180), 8 x 8 lanes (200, 300); odd and
# even column counts, few columns; 600 layers: outside the tilings
GRID = [(45, 60, False, True, True), (45, 60, True, True, False), (45, 80, False, True, True), (45, 140, False, True, False),
        (46, 140, True, True, True), (45, 180, True, False, True), (45, 200, False, True, True), (6, 200, True, True, False),
        (45, 300, True, True, True), (6, 400, True, True, True), (6, 500, False, True, False), (6, 600, False, True, True)]
IDS = [f"{c}x{l}-top{int(t)}-{'cld' if cl else 'nocld'}-{'inc' if i else 'noinc'}" for c, l, t, cl, i in GRID]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ncol,nlay,top_at_1,clouds,inc", GRID, ids=IDS)
def test_entries_against_numpy_and_each_other(dt, ncol, nlay, top_at_1, clouds, inc, hip_f64, hip_f32):
    """General entry against numpy per g-point and broadband; fused entry against the materialised device route and against numpy"""
    be, npdt = backend(dt, hip_f64, hip_f32)
    c = Case(be, inputs(ncol, nlay, seed=nlay + ncol + top_at_1, dtype=npdt, clouds=clouds, inc=inc), top_at_1)
    up, dn = c.numpy_gpt()
    tag = f"{dt} {ncol}x{nlay} top{int(top_at_1)}"
    e_gpt = report(f"{tag} general per g-point vs numpy", dt, c.materialised(do_broadband=False), (up, dn))
    want_bb = (lw2s_ref.broadband(up), lw2s_ref.broadband(dn))
    dev = c.materialised()
    e_bb = report(f"{tag} general broadband vs numpy", dt, dev, want_bb)
    got = c.fused()
    e_dev = report(f"{tag} fused vs materialised", dt, got, (dev["flux_up"], dev["flux_dn"]))
    e_np = report(f"{tag} fused vs numpy", dt, got, want_bb)
    assert e_gpt <= (F64_GPT_TOL if dt == "f64" else F32_GPT_TOL), e_gpt
    assert max(e_bb, e_dev, e_np) <= tol(dt), (e_bb, e_dev, e_np)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("nlay,top_at_1", [(60, False), (200, True), (600, True)])
def test_isothermal_closure_through_the_fused_entry(dt, nlay, top_at_1, hip_f64, hip_f32):
    """B_lev, sfc_src and inc_flux/pi equal per g-point: flux_up = flux_dn = pi * sum of the sources at every level, for any tau, ssa,
    g and emissivity"""
    be, npdt = backend(dt, hip_f64, hip_f32)
    I = inputs(45, nlay, seed=7 + nlay, dtype=npdt)
    b = np.random.default_rng(nlay).uniform(5., 40., I["tau"].shape[0]).astype(npdt)
    I["pfrac"] = np.ascontiguousarray(np.broadcast_to(b[:, None, None], I["pfrac"].shape))       # the source rides on pfrac, B_lev = 1
    I["blev"] = np.ones_like(I["blev"])
    I["ssrc"] = np.ascontiguousarray(np.broadcast_to(b[:, None], I["ssrc"].shape))
    I["inc"] = (npdt(np.pi) * I["ssrc"]).astype(npdt)
    I["emis"] = np.random.default_rng(1).uniform(0.3, 1.0, I["emis"].shape).astype(npdt)
    got = Case(be, I, top_at_1).fused()
    want = np.full(got["flux_up"].shape, np.pi * b.astype(np.float64).sum())
    e = report(f"{dt} nlay={nlay} isothermal closure", dt, got, (want, want))
    # a layer at or below the thin-layer switch (0 < tau <= 1e-8) transmits exp(-D tau) and emits nothing: by the stated semantics the
    # closure loses up to D tau of the flux per such layer (observed: 4.0e-10 in fp64 with the builder's cells at 1e-9, all of it this)
    tt = lw2s_ref.combine(I["tau"], (I["ct"], I["cw"], I["cg"]), I["gb"])[0].astype(np.float64)
    thin = 1.66 * np.where(tt <= 1e-8, tt, 0.0).sum(axis=1).max()
    assert e <= tol(dt) + thin, (e, thin)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("nlay", [140, 600])
def test_null_clouds_are_zero_clouds_bit_for_bit(dt, nlay, hip_f64, hip_f32):
    be, npdt = backend(dt, hip_f64, hip_f32)
    c = Case(be, inputs(45, nlay, seed=11, dtype=npdt, clouds=False), True)
    z = tuple(be.zeros((len(SIZES), nlay, 45)) for _ in range(3))
    a, b = c.fused(cloud=None), c.fused(cloud=z)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _chain(ncol, nlay, seed, clouds=True, spread=False):
    kw = dict(ngpt=32, nbnd=4, npres=20, nflav=4, nminor_lower=9, nminor_upper=5)
    kl0, ks0 = synthetic.make_kdist("lw", **kw), synthetic.make_kdist("sw", **kw)
    atm0 = synthetic.make_atmosphere(ncol, nlay, nbnd_lw=4, nbnd_sw=4, clouds=clouds, seed=seed)
    if spread:
        f = np.random.default_rng(seed + 1).uniform(0.65, 1.35, ncol)
        atm0.p_lay = np.ascontiguousarray(atm0.p_lay * f); atm0.p_lev = np.ascontiguousarray(atm0.p_lev * f)
    luts0 = (synthetic.make_cloud_lut(4, "lw"), synthetic.make_cloud_lut(4, "sw")) if clouds else None
    return atm0, kl0, ks0, luts0


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_resident_solver_with_lw_scattering(dt, hip_f64, hip_f32, monkeypatch):
    """ResidentSolver(lw_scattering=True): its LW fluxes are the fused entry's on the step's own buffers, its SW outputs are the plain
    solver's bit for bit, its LW differs from the no-scattering all-sky result; without cloud LUTs it is the ssa = 0 solve"""
    be, npdt = backend(dt, hip_f64, hip_f32)
    monkeypatch.setenv("RRX_PAD_COLUMNS", "0")
    atm0, kl0, ks0, luts0 = _chain(64, 140, seed=3)
    kl, ks = be.upload_kdist(kl0), be.upload_kdist(ks0)
    atm = pipeline.upload_atmosphere(be, atm0.astype(npdt))
    luts = tuple(be.upload_lut(l) for l in luts0)
    for overlap in (False, True):
        kw = dict(do_broadband=True, sort_columns="0", cloud_luts=luts, overlap=overlap)
        plain = pipeline.ResidentSolver(be, kl, ks, atm, **kw)
        scat = pipeline.ResidentSolver(be, kl, ks, atm, lw_scattering=True, **kw)
        F0, F1 = be.to_numpy(plain.step()).copy(), be.to_numpy(scat.step()).copy()
        assert np.array_equal(F1[3:], F0[3:])                            # the SW outputs
        assert cases.rel_err(F1[0], F0[0], floor=floor(dt)) > 1e-4        # clouds scatter: the LW fluxes are others
        cld = be.cloud_optics_2str(luts[0], atm.lwp, atm.iwp, atm.rel, atm.dei)
        want = be.lw_solver_2stream_fractions(atm.top_at_1, kl, scat.lw["tau"], scat.lw, scat.sfc_emis_gpt, cloud=cld)
        assert np.array_equal(F1[0], be.to_numpy(want["flux_up"])) and np.array_equal(F1[1], be.to_numpy(want["flux_dn"]))
        assert np.array_equal(F1[2], F1[1] - F1[0])
    clear = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", lw_scattering=True)
    Fc = be.to_numpy(clear.step()).copy()
    want = be.lw_solver_2stream_fractions(atm.top_at_1, kl, clear.lw["tau"], clear.lw, clear.sfc_emis_gpt, cloud=None)
    assert np.array_equal(Fc[0], be.to_numpy(want["flux_up"])) and np.array_equal(Fc[1], be.to_numpy(want["flux_dn"]))
    sun = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", cloud_luts=luts, sunlit=True, lw_scattering=True)
    assert np.array_equal(be.to_numpy(sun.step())[:3], F1[:3])


def test_resident_solver_lw_scattering_sorted_and_padded(hip_f64, monkeypatch):
    """16 385 columns (padded to 16 400) with a surface-pressure spread that switches sorting on, against an unsorted, unpadded run.

    Sorting moves columns between the windowed and the gather gas-optics kernels, whose tau differ in the last bit. Observed on an
    MI355X: flux_up 4.9e-16, flux_dn 4.8e-16, flux_net 1.8e-15 against 1e-11. (With the layer sources evaluated as the formulas are
    written, Z (1 + Rdif - Tdif) at Z up to 1e5 times the level sources amplified those last bits to 2.3e-11 on flux_dn.)"""
    be = hip_f64
    atm0, kl0, ks0, luts0 = _chain(16385, 30, seed=5, spread=True)
    kl, ks = be.upload_kdist(kl0), be.upload_kdist(ks0)
    atm = pipeline.upload_atmosphere(be, atm0)
    luts = tuple(be.upload_lut(l) for l in luts0)
    monkeypatch.setenv("RRX_PAD_COLUMNS", "0")
    plain = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", cloud_luts=luts, lw_scattering=True)
    assert plain.perm is None
    ref = be.to_numpy(plain.step()).copy()
    monkeypatch.setenv("RRX_PAD_COLUMNS", "1")
    solver = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="auto", cloud_luts=luts, lw_scattering=True)
    assert solver.npad == 15 and solver.sort_columns
    F = be.to_numpy(solver.step()).copy()
    assert F.shape == (7, 31, 16385)
    errs = [cases.rel_err(F[i], ref[i]) for i in range(3)]
    print("LW2S sorted and padded vs unsorted (up, dn, net):", " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) <= 1e-11, errs


def test_resident_solver_refuses_the_pairs_it_cannot_serve(hip_f64, monkeypatch):
    be = hip_f64
    atm0, kl0, ks0, _ = _chain(32, 30, seed=1, clouds=False)
    kl0.extras["optimal_angle_fit"] = np.ones((2, 4)) if "optimal_angle_fit" not in kl0.extras else kl0.extras["optimal_angle_fit"]
    kl, ks = be.upload_kdist(kl0), be.upload_kdist(ks0)
    atm = pipeline.upload_atmosphere(be, atm0)
    for kw, word in ((dict(byband=True), "byband"), (dict(jacobian=True), "jacobian"), (dict(n_gauss_angles=2), "n_gauss_angles"),
                     (dict(optimal_angles=True), "optimal_angles")):
        with pytest.raises(ValueError, match="lw_scattering.*" + word):
            pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, lw_scattering=True, **kw)
    with pytest.raises(ValueError, match="lw_scattering"):
        pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=False, lw_scattering=True)


def test_cxx_solver_lw_scattering_matches_pipeline(hip_f64):
    """Radiation_solver_longwave::set_lw_scattering(true) with a column block of 1 000 on 2 500 columns x 30 layers with a pressure
    spread, against ResidentSolver(lw_scattering=True) at 1e-11 (the same kernels); without cloud optics it is the ssa = 0 solve; every
    refused pair fails at the solve."""
    from rte_rrtmgp_cpp_amd import cxx_driver
    be = hip_f64
    for clouds in (True, False):
        atm0, kl0, ks0, luts0 = _chain(2500, 30, seed=31, clouds=clouds, spread=True)
        luts = None if luts0 is None else tuple(be.upload_lut(l) for l in luts0)
        sv = pipeline.ResidentSolver(be, be.upload_kdist(kl0), be.upload_kdist(ks0), pipeline.upload_atmosphere(be, atm0), do_broadband=True,
                                     cloud_luts=luts, lw_scattering=True)
        ref = be.to_numpy(sv.step()).copy()
        drv = cxx_driver.CxxDriver(be, kl0, ks0, pipeline.upload_atmosphere(be, atm0), luts0, column_block=1000, lw_scattering=True)
        try:
            got = be.to_numpy(drv.step()).copy()
        finally:
            drv.close()
        errs = [cases.rel_err(got[i], ref[i]) for i in range(7)]
        print(f"LW2S CxxDriver clouds={clouds} vs ResidentSolver:", " ".join(f"{e:.3e}" for e in errs))
        assert max(errs) <= 1e-11, errs
        if clouds:
            one = pipeline.ResidentSolver(be, be.upload_kdist(kl0), be.upload_kdist(ks0), pipeline.upload_atmosphere(be, atm0),
                                          do_broadband=True, cloud_luts=luts)
            assert cases.rel_err(ref[0], be.to_numpy(one.step())[0]) > 1e-4
    for kw in (dict(n_gauss_angles=2), dict(optimal_angles=True), dict(jacobian=True), dict(broadband=False)):
        drv = cxx_driver.CxxDriver(be, kl0, ks0, pipeline.upload_atmosphere(be, atm0), luts0, column_block=1000, lw_scattering=True, **kw)
        try:
            with pytest.raises(RuntimeError, match="set_lw_scattering"):
                drv.step()
        finally:
            drv.close()


def test_driver_lw_scattering(tmp_path, hip_f64):
    """--lw-scattering with RRX_COL_BLOCK=7 (6 blocks + a residual of 3) on 45 columns x 60 layers against one block and against
    ResidentSolver(lw_scattering=True) at 1e-11; every refused pair ends the driver with a non-zero status."""
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
        assert run_driver(d, "--cloud-optics", "--lw-scattering", env=env) == 0
        _, v = rrxio.read(os.path.join(d, "rte_rrtmgp_output.nc"))
        outs.append({k: v[k][0].copy() for k in ("lw_flux_up", "lw_flux_dn")})
    for k in outs[0]:
        assert outs[0][k].shape[0] == 61
        assert cases.rel_err(outs[0][k], outs[1][k]) <= 1e-11, k
    be = hip_f64
    luts = (be.upload_lut(lut_l), be.upload_lut(lut_s))
    F = {}
    for scat in (False, True):
        sv = pipeline.ResidentSolver(be, be.upload_kdist(kl), be.upload_kdist(ks), pipeline.upload_atmosphere(be, atm), do_broadband=True,
                                     cloud_luts=luts, lw_scattering=scat)
        F[scat] = be.to_numpy(sv.step()).copy()
    assert not np.array_equal(F[False][0], F[True][0])
    for i, k in enumerate(("lw_flux_up", "lw_flux_dn")):
        assert cases.rel_err(outs[1][k].reshape(F[True][i].shape), F[True][i]) <= 1e-11, k
    assert run_driver(d, "--cloud-optics", "--lw-scattering", "--lw-gauss-angles", "2") != 0
    assert run_driver(d, "--cloud-optics", "--lw-scattering", "--lw-optimal-angles") != 0
    assert run_driver(d, "--cloud-optics", "--lw-scattering", "--lw-jacobian") != 0
    assert run_driver(d, "--cloud-optics", "--lw-scattering", "--output-bnd-fluxes", "--byband-solvers") != 0
    assert run_driver(d, "--cloud-optics", "--lw-scattering", "--output-bnd-fluxes") != 0
