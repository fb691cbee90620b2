"""GPU tests of the by-band form of the fused broadband solvers (rrx_lw_solver_noscat_fractions_byband, rrx_sw_solver_2stream_byband):
against the per-g-point solvers + band sums on the same inputs, against the CPU oracle, on uneven / degenerate bands, over the tilings
(and the route outside them), through the C++ driver (--byband-solvers) and through pipeline.ResidentSolver(byband=True)."""
import os
import types

import numpy as np
import pytest

import cases
from host_driver import run_driver
from rte_rrtmgp_cpp_amd import synthetic, synthetic_files, rrxio, pipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def band_layout(sizes):
    """(nbnd, 2) 1-based inclusive g-point limits and the (ngpt,) 1-based band of each g-point; a size of 0 is an empty band."""
    lims, gb, g = [], [], 1
    for ib, n in enumerate(sizes):
        lims.append((g, g + n - 1)); gb += [ib + 1]*n; g += n
    return np.array(lims, dtype=np.int32), np.array(gb, dtype=np.int32)


def inputs(ncol, nlay, sizes, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    lims, gb = band_layout(sizes)
    ngpt, nbnd = len(gb), len(sizes)
    shp = (ngpt, nlay, ncol)
    d = dict(lims=lims, gb=gb, tau=10.0**rng.uniform(-4, 1.5, shp), pfrac=rng.uniform(0.05, 1.0, shp),
             blay=rng.uniform(5., 40., (nbnd, nlay, ncol)), blev=rng.uniform(5., 40., (nbnd, nlay+1, ncol)),
             emis=rng.uniform(0.8, 1.0, (ngpt, ncol)), ssrc=rng.uniform(5., 40., (ngpt, ncol)),
             ssa=rng.uniform(0., 1., shp), g=rng.uniform(-0.3, 0.9, shp), mu0=rng.uniform(0.05, 1.0, ncol),
             adir=rng.uniform(0., 0.6, (ngpt, ncol)), adif=rng.uniform(0., 0.6, (ngpt, ncol)), inc=rng.uniform(0., 5., (ngpt, ncol)))
    return {k: (np.ascontiguousarray(v.astype(dtype)) if v.dtype.kind == "f" else v) for k, v in d.items()}


def band_sums(gpt, lims):
    """numpy band sums of per-g-point fluxes (ngpt, nlev, ncol), g-points in order; an empty band is zero"""
    out = np.zeros((lims.shape[0],) + gpt.shape[1:], dtype=gpt.dtype)
    for ib, (lo, hi) in enumerate(lims):
        for ig in range(lo - 1, hi):
            out[ib] += gpt[ig]
    return out


class Lw:
    """LW by-band solve and its references on one backend-neutral input set"""
    def __init__(self, be, I, top_at_1):
        self.be, self.I, self.top = be, I, bool(top_at_1)
        up = be.asarray
        ngpt, nlay, ncol = I["tau"].shape
        self.sec = be.lw_secants_array(ncol, ngpt, 1, 4, up(pipeline.GAUSS_DS))
        self.w = up(np.array([1.0]))
        self.tau, self.emis = up(I["tau"]), up(I["emis"])
        self.fr = dict(pfrac=up(I["pfrac"]), blay=up(I["blay"]), blev=up(I["blev"]), sfc_src=up(I["ssrc"]))
        self.lims, self.gb = up(I["lims"]), up(I["gb"])
        self.kd = types.SimpleNamespace(band_lims_gpt=self.lims, gpoint_bands=self.gb)

    def byband(self):
        r = self.be.lw_solver_noscat_fractions_byband(self.top, self.kd, self.sec, self.w, self.tau, self.fr, self.emis)
        return {k: self.be.to_numpy(v) for k, v in r.items()}

    def sources(self):
        be = self.be
        ngpt, nlay, ncol = self.tau.shape
        lay, lev = be.empty((ngpt, nlay, ncol)), be.empty((ngpt, nlay+1, ncol))
        be._c("planck_sources_from_fractions", ncol, nlay, ngpt, self.gb, self.fr["pfrac"], self.fr["blay"], self.fr["blev"], lay, lev)
        return lay, lev

    def per_gpoint(self):
        lay, lev = self.sources()
        r = self.be.lw_solver_noscat(self.top, self.sec, self.w, self.tau, lay, lev, self.emis, self.fr["sfc_src"])
        return r, lay, lev

    def broadband(self):
        r = self.be.lw_solver_noscat_fractions(self.top, self.kd, self.sec, self.w, self.tau, self.fr, self.emis)
        return {k: self.be.to_numpy(v) for k, v in r.items()}


class Sw:
    def __init__(self, be, I, top_at_1, with_g):
        self.be, self.I, self.top = be, I, bool(top_at_1)
        up = be.asarray
        self.tau, self.ssa, self.mu0 = up(I["tau"]), up(I["ssa"]), up(I["mu0"])
        self.g = up(I["g"]) if with_g else None
        self.g_arr = self.g if with_g else up(np.zeros_like(I["g"]))
        self.adir, self.adif, self.inc = up(I["adir"]), up(I["adif"]), up(I["inc"])
        self.lims = up(I["lims"])

    def byband(self):
        r = self.be.sw_solver_2stream_byband(self.top, self.tau, self.ssa, self.g, self.mu0, self.adir, self.adif, self.inc, self.lims)
        return {k: self.be.to_numpy(v) for k, v in r.items()}

    def per_gpoint(self):
        return self.be.sw_solver_2stream(self.top, self.tau, self.ssa, self.g_arr, self.mu0, self.adir, self.adif, self.inc)

    def broadband(self):
        r = self.be.sw_solver_2stream(self.top, self.tau, self.ssa, self.g, self.mu0, self.adir, self.adif, self.inc, do_broadband=True)
        return {k: self.be.to_numpy(v) for k, v in r.items()}


SIZES_16 = [16]*8                        # 128 g-points in 8 bands of 16


@pytest.mark.parametrize("nlay", [60, 140])
@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
@pytest.mark.parametrize("sky", ["clear", "allsky"])
def test_byband_matches_per_gpoint_solve_and_band_sums(nlay, top_at_1, sky, hip_f64):
    """Fused by-band form against the per-g-point solvers + rrx_sum_byband on the same inputs (clear sky: SW without g array)."""
    be = hip_f64
    I = inputs(45, nlay, SIZES_16, seed=nlay + 2*top_at_1)
    lw = Lw(be, I, top_at_1)
    got = lw.byband()
    ref, _, _ = lw.per_gpoint()
    for k in ("up", "dn"):
        want = be.to_numpy(be.sum_byband(ref["flux_" + k], lw.lims))
        assert cases.rel_err(got["bnd_flux_" + k], want) <= 1e-11, "lw " + k
    sw = Sw(be, I, top_at_1, with_g=(sky == "allsky"))
    got = sw.byband()
    ref = sw.per_gpoint()
    for k in ("up", "dn", "dir"):
        want = be.to_numpy(be.sum_byband(ref["flux_" + k], sw.lims))
        assert cases.rel_err(got["bnd_flux_" + k], want) <= 1e-11, "sw " + k


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
def test_byband_matches_cpu_oracle(dt, top_at_1, hip_f64, hip_f32, oracle_f64, oracle_f32):
    """Against the oracle's per-g-point solvers + sum_byband: 1e-9 LW / 1e-7 SW in fp64; fp32 against the fp32 oracle at twice the
    error observed for the fp32 solvers (tests/test_gpu_parity.py)."""
    be, orc = (hip_f64, oracle_f64) if dt == "f64" else (hip_f32, oracle_f32)
    I = inputs(36, 60, [4, 12, 16], seed=11 + top_at_1, dtype=np.float64 if dt == "f64" else np.float32)
    lw = Lw(be, I, top_at_1)
    got = lw.byband()
    lay, lev = (be.to_numpy(a) for a in lw.sources())                # (bit-identical to the reference's Planck source expressions)
    sec = orc.lw_secants_array(I["tau"].shape[2], I["tau"].shape[0], 1, 4, orc.asarray(pipeline.GAUSS_DS))
    o = orc.lw_solver_noscat(bool(top_at_1), sec, orc.asarray(np.array([1.0])), I["tau"], lay, lev, I["emis"], I["ssrc"])
    # (fp32: the fp32 solver bounds of tests/test_gpu_parity.py, LW 3e-5; SW twice the 1.3e-4 observed on an MI355X)
    tol_lw, tol_sw, floor = (1e-9, 1e-7, 1e-6) if dt == "f64" else (3e-5, 2.5e-4, 1e-2)
    for k in ("up", "dn"):
        want = orc.to_numpy(orc.sum_byband(o["flux_" + k], I["lims"]))
        assert cases.rel_err(got["bnd_flux_" + k], want, floor=floor) <= tol_lw, "lw " + k
    sw = Sw(be, I, top_at_1, with_g=True)
    got = sw.byband()
    o = orc.sw_solver_2stream(bool(top_at_1), I["tau"], I["ssa"], I["g"], I["mu0"], I["adir"], I["adif"], I["inc"])
    for k in ("up", "dn", "dir"):
        want = orc.to_numpy(orc.sum_byband(o["flux_" + k], I["lims"]))
        assert cases.rel_err(got["bnd_flux_" + k], want, floor=floor) <= tol_sw, "sw " + k


@pytest.mark.parametrize("sky", ["clear", "allsky"])
def test_band_net_and_broadband_outputs(sky, hip_f64):
    """Band net = dn - up of the returned band sums, bit for bit; the broadband outputs and the band sums added over the bands match
    the broadband mode of the existing entries within 1e-13."""
    be = hip_f64
    I = inputs(70, 140, [3, 16, 8, 1, 40, 12], seed=3)
    lw = Lw(be, I, False)
    got, bb = lw.byband(), lw.broadband()
    assert np.array_equal(got["bnd_flux_net"], got["bnd_flux_dn"] - got["bnd_flux_up"])
    for k in ("up", "dn"):
        assert cases.rel_err(got["flux_" + k], bb["flux_" + k]) <= 1e-13, "lw " + k
        assert cases.rel_err(got["bnd_flux_" + k].sum(axis=0), bb["flux_" + k]) <= 1e-13, "lw " + k
    sw = Sw(be, I, True, with_g=(sky == "allsky"))
    got, bb = sw.byband(), sw.broadband()
    assert np.array_equal(got["bnd_flux_net"], got["bnd_flux_dn"] - got["bnd_flux_up"])
    for k in ("up", "dn", "dir"):
        assert cases.rel_err(got["flux_" + k], bb["flux_" + k]) <= 1e-13, "sw " + k
        assert cases.rel_err(got["bnd_flux_" + k].sum(axis=0), bb["flux_" + k]) <= 1e-13, "sw " + k


@pytest.mark.parametrize("sizes", [[1, 3, 8, 16, 40], [1]*24, [48], [8, 0, 16, 8], [0, 16, 16, 0]],
                         ids=["uneven", "one-per-gpoint", "one-band", "empty-inside", "empty-at-ends"])
def test_uneven_and_degenerate_bands(sizes, hip_f64):
    """Bands of 1 ... 40 g-points, one band per g-point, one band over all g-points (= broadband mode) and empty bands (zeros; at the
    ends the band's first g-point lies outside the g-point range), LW with gpoint_bands / blay / blev built to match.
    LW at 1e-10: a band of one g-point is that g-point's flux, where the fused kernel and the per-g-point kernel differ in the last
    bits of exp(-tau) (the fp64 fused form reads an LDS table); near tau = eps^(1/4) the source term (1 - T)/tau - T amplifies that
    to 2.4e-11 of the small fluxes below the top (MI355X). Bands of 16 g-points stay within 1e-11 (the test above)."""
    be = hip_f64
    I = inputs(45, 60, sizes, seed=len(sizes))
    lw, sw = Lw(be, I, True), Sw(be, I, False, with_g=True)
    got_l, got_s = lw.byband(), sw.byband()
    ref_l, _, _ = lw.per_gpoint()
    ref_s = sw.per_gpoint()
    for k in ("up", "dn"):
        assert cases.rel_err(got_l["bnd_flux_" + k], band_sums(be.to_numpy(ref_l["flux_" + k]), I["lims"])) <= 1e-10, "lw " + k
    for k in ("up", "dn", "dir"):
        assert cases.rel_err(got_s["bnd_flux_" + k], band_sums(be.to_numpy(ref_s["flux_" + k]), I["lims"])) <= 1e-11, "sw " + k
    for ib, n in enumerate(sizes):
        if n == 0:
            for k in ("up", "dn", "net"):
                assert not got_l["bnd_flux_" + k][ib].any() and not got_s["bnd_flux_" + k][ib].any(), (ib, k)
    if len(sizes) == 1:
        bl, bs = lw.broadband(), sw.broadband()
        for k in ("up", "dn"):
            assert cases.rel_err(got_l["bnd_flux_" + k][0], bl["flux_" + k]) <= 1e-13
        for k in ("up", "dn", "dir"):
            assert cases.rel_err(got_s["bnd_flux_" + k][0], bs["flux_" + k]) <= 1e-13


@pytest.mark.parametrize("dt,ncol,nlay", [("f64", 21, 287), ("f64", 21, 288), ("f64", 13, 575), ("f64", 9, 600),
                                           ("f32", 21, 140), ("f32", 22, 140), ("f32", 22, 288), ("f32", 9, 600),
                                           ("f64", 16384, 140)],
                         ids=["287", "288", "575", "600-fallback", "f32-odd", "f32-even", "f32-288", "f32-600-fallback", "full-chip"])
def test_geometries(dt, ncol, nlay, hip_f64, hip_f32):
    """The tilings the broadband launchers serve (W = 8 forms up to 575 layers, fp32 one- and two-column lanes, a few workgroups
    and a full chip) and the route outside them (600 layers: per-g-point fluxes in the workspace + band sums). fp64 at 1e-10: over
    16 384 columns with bands of two g-points the rare ill-conditioned cells show the per-g-point difference of the fused and the
    per-g-point kernels (observed on an MI355X: LW 6.7e-11, see test_uneven_and_degenerate_bands; SW 1.7e-11, near-resonant cells,
    tests/cases.py Checker); fp32 at twice what was observed (LW 5.8e-6, SW 1.0e-4)."""
    be = hip_f64 if dt == "f64" else hip_f32
    sizes = [8, 24] if ncol < 1000 else [2, 6, 8, 16]
    I = inputs(ncol, nlay, sizes, seed=ncol + nlay, dtype=np.float64 if dt == "f64" else np.float32)
    tol_lw, tol_sw, floor = (1e-10, 1e-10, 1e-6) if dt == "f64" else (1.2e-5, 2e-4, 1e-2)
    lw = Lw(be, I, nlay % 2 == 0)
    got = lw.byband()
    ref, lay, lev = lw.per_gpoint()
    del lay, lev
    for k in ("up", "dn"):
        want = be.to_numpy(be.sum_byband(ref["flux_" + k], lw.lims))
        assert cases.rel_err(got["bnd_flux_" + k], want, floor=floor) <= tol_lw, "lw " + k
    del ref
    sw = Sw(be, I, nlay % 2 == 1, with_g=(ncol % 2 == 1))
    got = sw.byband()
    ref = sw.per_gpoint()
    for k in ("up", "dn", "dir"):
        want = be.to_numpy(be.sum_byband(ref["flux_" + k], sw.lims))
        assert cases.rel_err(got["bnd_flux_" + k], want, floor=floor) <= tol_sw, "sw " + k


# ---- C++ driver ---------------------------------------------------------------------------------------------------------------
KW = dict(ngpt=48, nbnd=3, npres=12, nflav=4, nminor_lower=7, nminor_upper=4)


def read_output(d):
    _, v = rrxio.read(os.path.join(d, "rte_rrtmgp_output.nc"))
    return {k: a[0].copy() for k, a in v.items()}


def test_driver_byband_solvers(tmp_path):
    """--cloud-optics --output-bnd-fluxes --byband-solvers with RRX_COL_BLOCK=7 (6 blocks + a residual of 3): band and broadband
    fluxes against a --no-broadband-solvers --output-bnd-fluxes run."""
    d = str(tmp_path)
    kl, ks = synthetic.make_kdist("lw", **KW), synthetic.make_kdist("sw", **KW)
    atm = synthetic.make_atmosphere(45, 60, nbnd_lw=KW["nbnd"], nbnd_sw=KW["nbnd"], clouds=True, seed=5)
    synthetic_files.write_case(d, atm, kl, ks, synthetic.make_cloud_lut(KW["nbnd"], "lw"), synthetic.make_cloud_lut(KW["nbnd"], "sw"))
    env = {"RRX_COL_BLOCK": "7"}
    assert run_driver(d, "--cloud-optics", "--output-bnd-fluxes", "--no-broadband-solvers", env=env) == 0
    ref = read_output(d)
    for whole in (False, True):
        assert run_driver(d, "--cloud-optics", "--output-bnd-fluxes", "--byband-solvers", env=None if whole else env) == 0
        got = read_output(d)
        keys = [k for k in ref if "flux" in k]
        assert {"lw_bnd_flux_up", "sw_bnd_flux_dn_dir", "sw_bnd_flux_net", "lw_flux_net"} <= set(keys)
        for k in keys:
            assert got[k].shape == ref[k].shape, k
            assert cases.rel_err(got[k], ref[k]) <= 1e-11, (k, whole)


# ---- ResidentSolver ------------------------------------------------------------------------------------------------------------
def test_resident_solver_byband_sorted_and_padded(hip_f64, monkeypatch):
    """ResidentSolver(byband=True) on 1 000 columns (padded to 1 008) with a surface-pressure spread that switches sorting on: its
    band fluxes, in the caller's column order, against an unsorted, unpadded run; the broadband arrays against the broadband step."""
    be = hip_f64
    ncol, nlay = 1000, 40
    kw = dict(ngpt=64, nbnd=4, npres=20, nflav=4, nminor_lower=9, nminor_upper=5)
    kl, ks = be.upload_kdist(synthetic.make_kdist("lw", **kw)), be.upload_kdist(synthetic.make_kdist("sw", **kw))
    atm0 = synthetic.make_atmosphere(ncol, nlay, nbnd_lw=4, nbnd_sw=4, seed=5)
    f = np.random.default_rng(8).uniform(0.65, 1.35, ncol)
    atm0.p_lay = np.ascontiguousarray(atm0.p_lay * f); atm0.p_lev = np.ascontiguousarray(atm0.p_lev * f)
    atm = pipeline.upload_atmosphere(be, atm0)
    monkeypatch.setenv("RRX_PAD_COLUMNS", "0")
    plain = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0", byband=True)
    assert plain.perm is None
    F_ref = be.to_numpy(plain.step()).copy()
    ref = {k: be.to_numpy(v).copy() for k, v in plain.bnd_fluxes.items()}
    monkeypatch.setenv("RRX_PAD_COLUMNS", "1")
    solver = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="auto", byband=True)
    assert solver.npad == 8 and solver.sort_columns
    F = be.to_numpy(solver.step())
    got = {k: be.to_numpy(v) for k, v in solver.bnd_fluxes.items()}
    assert set(got) == {"lw_up", "lw_dn", "lw_net", "sw_up", "sw_dn", "sw_dir", "sw_net"}
    for k in got:
        assert got[k].shape == (4, nlay+1, ncol), k
        assert cases.rel_err(got[k], ref[k]) <= 1e-11, k
    assert cases.rel_err(F, F_ref) <= 1e-11
    # the seven broadband arrays: as the broadband step's
    bb = be.to_numpy(pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="0").step())
    assert cases.rel_err(F_ref, bb) <= 1e-13
    assert np.array_equal(got["lw_net"], got["lw_dn"] - got["lw_up"])
    with pytest.raises(ValueError):
        pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=False, byband=True)
