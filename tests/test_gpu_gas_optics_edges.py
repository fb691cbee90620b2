"""The HIP gas optics where its inputs had no variety: irregular k-distributions (unequal bands, minor-contributor intervals inside
a band, of one g-point, over two bands, overlapping, over the whole spectrum), every reason for which the windowed kernel hands a
workgroup back to the gather kernel, and atmospheres that leave the tables, sit on their nodes or lose their key species
(tests/gas_cases.py). Every entry point is compared with the NumPy reference tests/gas_optics_ref.py and with the CPU oracle.

Tolerances (cases.rel_err, floor 1e-6 in fp64, 1e-2 in fp32), from the rounding floor of the reference arithmetic that
tests/test_gas_optics_ref.py measures on the CPU and gas_cases.E_ORACLE / E_ORACLE32 record -- never from what the HIP code returns:

    family      e_oracle: optics   sfc_src_jac   fminor/fmajor  |  e_oracle32: optics   sfc_src_jac
    regular           8.6e-16       1.7e-14        9.0e-10      |        4.3e-07         8.5e-06
    irregular         8.6e-16       2.7e-14        9.0e-10      |        3.5e-07         1.5e-05
    edges             1.2e-15       2.7e-14        6.2e-10      |        5.2e-07         1.5e-05

(e_oracle = fp64 oracle against the long-double reference; e_oracle32 = fp32 oracle against the fp64 reference on the same float32
inputs -- which keep 1e-4 of a spacing clear of eta = 1, where single precision is discontinuous; "optics" = tau, ssa, sources,
Planck outputs, col_mix; the largest over LW and SW at 193 columns x 30 layers.) fp64 against the reference:
max(1e-12, 8 e_oracle) -- 1e-12, the windowed kernel's own bound, for everything but the interpolation weights; gather and
reference-shaped kernels against the oracle: bit-equal among themselves where the suite asserts that, 1e-12 against the oracle;
fluxes 1e-9 (LW) and 1e-7 (SW); fp32: 4 e_oracle32."""
import os
import re

import numpy as np
import pytest
import torch

import cases
import gas_cases as gc
import gas_optics_ref as ref
from rte_rrtmgp_cpp_amd import synthetic, pipeline
from test_gas_window_tables import GCH, NCW, NXW, check_tables, read_tables, restate

pytestmark = pytest.mark.gpu

CENSUS = re.compile(r"\[gas window ([^\]]+)\] (\d+) of (\d+) workgroups handed back: temperature (\d+), pressure (\d+), regimes (\d+), "
                    r"chunk form (\d+), eta (\d+)")
REASONS = ("temperature", "pressure", "regimes", "chunk form", "eta")


def windowed(capfd, fn):
    """Run fn with the census of its windowed launches: (result, [dict(what, handed, total, temperature, ...)])."""
    capfd.readouterr()
    os.environ["RRX_GW_STATS"] = "1"
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        os.environ.pop("RRX_GW_STATS", None)
    err = capfd.readouterr().err
    lines = [dict(what=m[0], handed=int(m[1]), total=int(m[2]), **{r: int(x) for r, x in zip(REASONS, m[3:])}) for m in CENSUS.findall(err)]
    for c in lines:
        assert c["handed"] == sum(c[r] for r in REASONS) and c["handed"] <= c["total"], c
    return out, lines


def grid_of(ncol, nlay):
    """(geometry, workgroups) of a windowed launch: 256 columns x 1 layer from 192 columns on, else 64 columns x 4 layers."""
    return (1, -(-ncol // 256) * nlay) if ncol >= 192 else (0, -(-ncol // 64) * -(-nlay // 4))


def parts_of(nblk, ngpt):
    nz, nchunk = 1, (ngpt + GCH - 1) // GCH
    while nblk * nz < 768 and nz < 4 and 2 * nz <= nchunk:
        nz *= 2
    return nz


def check_windowed_tables(be, kd0, nlist, with_bands, with_lims):
    buf, L = read_tables(be)
    assert (L["ngpt"], L["ncmax"]) == (kd0.ngpt, (kd0.ngpt + GCH - 1) // GCH + kd0.nbnd)
    want = restate(kd0, L["ncmax"], nlist, with_bands=with_bands, with_lims=with_lims)
    check_tables(buf, L, want, nlist)
    return want


class Hip:
    """The HIP entry points of one case on one set of device arrays."""

    def __init__(self, be, kd0, atm, col_dry, col_gas):
        self.be, self.kd0, self.N = be, kd0, be.to_numpy
        self.kd = be.upload_kdist(kd0.astype(be.np_dtype))
        up = be.asarray
        self.play, self.tlay, self.tlev, self.tsfc = up(atm.p_lay), up(atm.t_lay), up(atm.t_lev), up(atm.t_sfc)
        self.col_dry, self.col_gas = up(col_dry), up(col_gas)
        self.sfc_lay = atm.nlay if atm.top_at_1 else 1
        self.shape = (kd0.ngpt, atm.nlay, atm.ncol)

    def lw_direct(self, by_band=None):
        return self.N(self.be.gas_optics_lw_direct(self.kd, self.play, self.tlay, self.col_gas, self.be.empty(self.shape), by_band=by_band))

    def sw_direct(self, by_band=None):
        t, w, g = (self.be.empty(self.shape) for _ in range(3))
        self.be.gas_optics_sw_direct(self.kd, self.play, self.tlay, self.col_gas, self.col_dry, t, w, g, by_band=by_band)
        return dict(tau=self.N(t), ssa=self.N(w), g=self.N(g))

    def planck_direct(self):
        return {k: self.N(v) for k, v in self.be.planck_source_direct(self.kd, self.play, self.tlay, self.tlev, self.tsfc, self.sfc_lay, self.col_gas).items()}

    def planck_fractions(self):
        fr = self.be.planck_fractions(self.kd, self.play, self.tlay, self.tlev, self.tsfc, self.sfc_lay, self.col_gas)
        lay, lev = self.be.planck_sources_from_fractions(self.kd, fr)
        return dict({k: self.N(v) for k, v in fr.items()}, lay_src=self.N(lay), lev_src=self.N(lev))

    def lw_fractions(self, by_band=None):
        tau = self.be.empty(self.shape)
        fr = self.be.gas_optics_lw_fractions(self.kd, self.play, self.tlay, self.tlev, self.tsfc, self.sfc_lay, self.col_gas, tau, by_band=by_band)
        lay, lev = self.be.planck_sources_from_fractions(self.kd, fr)
        return dict({k: self.N(v) for k, v in fr.items()}, tau=self.N(tau), lay_src=self.N(lay), lev_src=self.N(lev))


def close(family, key, got, want, f32=False, what=""):
    e = cases.rel_err(got, np.asarray(want, dtype=np.float64), floor=1e-2 if f32 else 1e-6)
    tol = gc.tol32(family, key) if f32 else gc.tol64(family, key)
    print(f"{what} {key}: {e:.2e} (bound {tol:.1e})")
    assert e <= tol, f"{what} {key}: {e:.3e} > {tol:.1e}"


def gather_only(be, fn):
    be.lib.call("rrx_set_gas_window", 0)
    try:
        return fn()
    finally:
        be.lib.call("rrx_set_gas_window", 1)


LW_KEYS = ("pfrac", "blay", "blev", "sfc_src", "sfc_src_jac", "lay_src", "lev_src")


def check_every_entry(be, orc, capfd, family, kd0, atm, col_dry, col_gas, fluxes=True):
    """Every gas-optics entry of one kind on one case, against the reference R and the oracle O; returns the census lines."""
    kind = kd0.kind
    R = gc.reference_outputs(kd0, atm, col_dry, col_gas)
    O = gc.shaped_route(orc, kd0, atm, col_dry, col_gas)
    S = gc.shaped_route(be, kd0, atm, col_dry, col_gas)
    H = Hip(be, kd0, atm, col_dry, col_gas)
    N = be.to_numpy
    # ---- the reference-shaped route: integer state equal to the oracle's and the reference's, the rest 1e-12 from the oracle
    for k in gc.INT_KEYS:
        assert np.array_equal(np.asarray(S["it_" + k]).astype(np.int64), np.asarray(O["it_" + k]).astype(np.int64)), k
        assert np.array_equal(np.asarray(S["it_" + k]).astype(np.int64), np.asarray(R["it_" + k]).astype(np.int64)), k
    for k in tuple("it_" + s for s in gc.STATE_KEYS) + gc.float_keys(kind):
        e = cases.rel_err(S[k], O[k])
        assert e <= 1e-12, f"reference-shaped {k}: {e:.3e} from the oracle"
        close(family, k, S[k], R[k], what="reference-shaped")
    it = be.interpolation(H.kd, H.play, H.tlay, H.col_gas)
    if kind == "lw":
        t_set = N(be.compute_tau_absorption_set(H.kd, it, H.play, H.tlay, H.col_gas, be.empty(H.shape)))
        assert np.array_equal(t_set, S["tau"]), "store form != add form on a zeroed tau"
        # ---- gather kernels of the direct forms: the bits of the interpolation route
        assert np.array_equal(gather_only(be, H.lw_direct), t_set)
        pd = H.planck_direct()
        for k in ("lay_src", "lev_src", "sfc_src", "sfc_src_jac"):
            assert np.array_equal(pd[k], S[k]), k
        pf = H.planck_fractions()
        for k in ("lay_src", "lev_src", "sfc_src", "sfc_src_jac"):
            assert np.array_equal(pf[k], pd[k]), k
        for k in ("pfrac", "blay", "blev"):
            close(family, k, pf[k], R[k], what="planck_fractions")
        # ---- windowed forms
        tau_w, c1 = windowed(capfd, H.lw_direct)
        check_windowed_tables(be, kd0, NXW, with_bands=False, with_lims=False)
        close(family, "tau", tau_w, R["tau"], what="lw_direct")
        fr, c2 = windowed(capfd, H.lw_fractions)
        want = check_windowed_tables(be, kd0, NXW, with_bands=True, with_lims=False)
        assert np.array_equal(fr["tau"], tau_w), "fractions form != plain windowed form"
        for k in ("blay", "blev"):
            assert np.array_equal(fr[k], pf[k]), k
        for k in LW_KEYS:
            close(family, k, fr[k], R[k], what="lw_fractions")
        # ---- all-sky forms: by-band optical depth on the unequal bands
        rng = np.random.default_rng(23)
        ct = np.where(rng.random((kd0.nbnd,) + H.shape[1:]) < 0.5, 0.0, 10.0 ** rng.uniform(-3, 1, (kd0.nbnd,) + H.shape[1:]))
        Rc = ref.add_by_band_1scalar(kd0, R["tau"], ct)
        tau_c, c3 = windowed(capfd, lambda: H.lw_direct(by_band=be.asarray(ct)))
        check_windowed_tables(be, kd0, NXW, with_bands=False, with_lims=True)
        close(family, "tau", tau_c, Rc, what="lw_direct_allsky")
        frc, c4 = windowed(capfd, lambda: H.lw_fractions(by_band=be.asarray(ct)))
        check_windowed_tables(be, kd0, NXW, with_bands=True, with_lims=True)
        close(family, "tau", frc["tau"], Rc, what="lw_fractions_allsky")
        for k in LW_KEYS:
            close(family, k, frc[k], R[k], what="lw_fractions_allsky")
        if fluxes:
            sec = pipeline.GAUSS_DS; w1 = np.array([1.0]); emis = np.full((kd0.ngpt, atm.ncol), 0.98)
            fo = orc.lw_solver_noscat(atm.top_at_1, orc.lw_secants_array(atm.ncol, kd0.ngpt, 1, 4, sec), w1, R["tau"], R["lay_src"], R["lev_src"], emis,
                                      R["sfc_src"], do_broadband=True)
            up = be.asarray
            fh = be.lw_solver_noscat(atm.top_at_1, be.lw_secants_array(atm.ncol, kd0.ngpt, 1, 4, up(sec)), up(w1), up(fr["tau"]), up(fr["lay_src"]),
                                     up(fr["lev_src"]), up(emis), up(fr["sfc_src"]), do_broadband=True)
            for k in ("flux_up", "flux_dn"):
                e = cases.rel_err(N(fh[k]), fo[k])
                assert e <= 1e-9, f"lw {k}: {e:.3e}"
        return want, c1 + c2 + c3 + c4
    # ---- shortwave
    t2, w2, g2 = (be.empty(H.shape) for _ in range(3))
    be.gas_optics_sw_fused(H.kd, it, H.play, H.tlay, H.col_gas, H.col_dry, t2, w2, g2)
    fused = dict(tau=N(t2), ssa=N(w2), g=N(g2))
    for k in ("tau", "ssa"):
        e = cases.rel_err(fused[k], O[k])
        assert e <= 1e-12, f"gas_optics_sw_fused {k}: {e:.3e} from the oracle"
        close(family, k, fused[k], R[k], what="sw_fused")
    assert not fused["g"].any()
    gat = gather_only(be, H.sw_direct)
    for k in ("tau", "ssa", "g"):
        assert np.array_equal(gat[k], fused[k]), k
    sw, c1 = windowed(capfd, H.sw_direct)
    want = check_windowed_tables(be, kd0, NCW, with_bands=False, with_lims=False)
    for k in ("tau", "ssa"):
        close(family, k, sw[k], R[k], what="sw_direct")
    assert not sw["g"].any()
    rng = np.random.default_rng(29)
    bshape = (kd0.nbnd,) + H.shape[1:]
    ct = np.where(rng.random(bshape) < 0.5, 0.0, 10.0 ** rng.uniform(-3, 1, bshape)); cw = rng.uniform(0, 1, bshape); cg = rng.uniform(0, 0.9, bshape)
    Rc = dict(zip(("tau", "ssa", "g"), ref.add_by_band_2stream(kd0, R["tau"], R["ssa"], R["g"], ct, cw, cg)))
    swc, c2 = windowed(capfd, lambda: H.sw_direct(by_band=tuple(be.asarray(x) for x in (ct, cw, cg))))
    check_windowed_tables(be, kd0, NCW, with_bands=False, with_lims=True)
    for k in ("tau", "ssa", "g"):
        close(family, k, swc[k], Rc[k], what="sw_direct_allsky")
    if fluxes:
        rng = np.random.default_rng(31)
        mu0 = rng.uniform(0.2, 1.0, atm.ncol); alb = np.full((kd0.ngpt, atm.ncol), 0.07); inc = np.repeat(kd0.solar_source[:, None], atm.ncol, axis=1)
        fo = orc.sw_solver_2stream(atm.top_at_1, R["tau"], R["ssa"], R["g"], mu0, alb, alb, inc, do_broadband=True)
        up = be.asarray
        fh = be.sw_solver_2stream(atm.top_at_1, up(sw["tau"]), up(sw["ssa"]), up(sw["g"]), up(mu0), up(alb), up(alb), up(inc), do_broadband=True)
        for k in ("flux_up", "flux_dn", "flux_dir"):
            e = cases.rel_err(N(fh[k]), fo[k])
            assert e <= 1e-7, f"sw {k}: {e:.3e}"
    return want, c1 + c2


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) every entry on irregular k-distributions
# 70 columns: 64 x 4 workgroups, a partial wavefront, 30 layers (no multiple of 4) to 35 km (four neighbouring layers fit a box of
# table nodes only when they are thin); 193 and 300: 256 x 1 workgroups, a partial block
@pytest.mark.parametrize("kind", ["lw", "sw"])
# spread: columns +-35 % / +-12 K apart (every lane of the gather kernels in another table cell; the windowed kernel hands most
# workgroups back); otherwise columns alike, so that the windowed kernel itself walks the irregular chunks
@pytest.mark.parametrize("variant,ncol,nlay,top_at_1,spread", [("whole", 70, 30, False, False), ("fits", 193, 30, True, True), ("cuts", 300, 22, False, False)],
                         ids=["whole-70", "fits-193-top-spread", "cuts-300"])
def test_every_entry_on_irregular_kdists(variant, ncol, nlay, top_at_1, spread, kind, capfd, hip_f64, oracle_f64):
    kd0, atm, col_dry, col_gas, _ = gc.family_case(oracle_f64, "irregular", kind, ncol, nlay, variant=variant, top_at_1=top_at_1, spread=spread,
                                                   z_top=35.e3 if ncol < 192 else 70.e3)
    want, census = check_every_entry(hip_f64, oracle_f64, capfd, "irregular", kd0, atm, col_dry, col_gas)
    geom, nblk = grid_of(ncol, nlay)
    nz = parts_of(nblk, kd0.ngpt)
    assert census and nz > 1 and all(c["total"] == nblk * nz for c in census), census
    ncmax = (kd0.ngpt + GCH - 1) // GCH + kd0.nbnd
    if variant == "cuts":        # more runs than the tables hold: the regular cut, whose chunks over a flavor change are handed back
        assert gc.chunk_runs(kd0) > ncmax and want["regular"] == 1 and want["nchunk"] == (kd0.ngpt + GCH - 1) // GCH
        assert all(c["chunk form"] > 0 for c in census)
    else:                        # band-aligned chunks off the multiples of 16: part 0 takes the whole range
        assert gc.chunk_runs(kd0) == want["nchunk"] <= ncmax and want["regular"] == 0
    if variant == "fits":
        assert all(c["chunk form"] == 0 for c in census)
    if variant == "whole":       # the whole-spectrum interval: every upper-regime chunk of another flavor than g-point 1's is unusable
        assert want["bad"][0][-1] == 0 and want["bad"][1][-1] > 0 and all(c["chunk form"] > 0 for c in census)
    if not spread:               # both kernels contribute to one array (band-aligned chunks: at most one entry per workgroup)
        assert all(0 < c["handed"] < (c["total"] if want["regular"] else nblk) for c in census), census


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) every hand-back reason, by design
def run_windowed_form(be, capfd, kd0, atm, col_dry, col_gas):
    """The fullest windowed form of the kind: (outputs, census of the one launch)."""
    H = Hip(be, kd0, atm, col_dry, col_gas)
    out, census = windowed(capfd, H.lw_fractions if kd0.kind == "lw" else H.sw_direct)
    assert len(census) == 1, census
    return out, census[0]


def match_reference(family, kd0, atm, col_dry, col_gas, out, f32=False, work=np.float64):
    R = gc.reference_outputs(kd0, atm, col_dry, col_gas, np.float64, work)
    for k in (("tau",) + LW_KEYS) if kd0.kind == "lw" else ("tau", "ssa"):
        close(family, k, out[k], R[k], f32=f32, what=kd0.kind)
    return R


@pytest.mark.parametrize("kind", ["lw", "sw"])
@pytest.mark.parametrize("reason", [0, 1, 2, 4])
def test_hand_back_for_spread_within_a_workgroup(reason, kind, capfd, hip_f64, oracle_f64):
    ncol, nlay = 300, 12
    kd0 = gc.irregular_kdist(kind, variant="fits", npres=59 if reason == 1 else 20)
    atm = gc.census_atmosphere(reason, kd0, ncol, nlay)
    col_dry, col_gas = gc.gas_columns(oracle_f64, kd0, atm)
    gc.assert_clear_of_nodes(kd0, atm.p_lay, atm.t_lay, col_gas)
    out, c = run_windowed_form(hip_f64, capfd, kd0, atm, col_dry, col_gas)
    print(c)
    geom, nblk = grid_of(ncol, nlay)
    assert geom == 1 and c["total"] == nblk * parts_of(nblk, kd0.ngpt) > nblk
    assert c[REASONS[reason]] > 0, c
    # (band-aligned chunks: part 0 hands back "the whole range", one entry per workgroup)
    if reason == 2:      # the one layer at the tropopause, in both column blocks
        assert c["handed"] == c["regimes"] == 2, c
    else:                # the wide block of the layers; the 44 columns behind it are alike and stay with the windowed kernel
        assert c["handed"] == c[REASONS[reason]] <= nlay, c
        assert c["handed"] >= (nlay - 2 if reason != 4 else nlay // 3), c      # (the top layers leave the pressure table; eta: the flavors with ozone or n2o)
    match_reference("irregular", kd0, atm, col_dry, col_gas, out)


@pytest.mark.parametrize("kind", ["lw", "sw"])
@pytest.mark.parametrize("variant", ["span", "many"])
def test_hand_back_for_chunk_form_in_one_regime(variant, kind, capfd, hip_f64, oracle_f64):
    """An interval over two bands of different flavors, or 13 contributors on one band, in the LOWER list only: the lower regime's
    workgroups come back, the upper regime's stay."""
    ncol, nlay = 300, 12
    kd0 = gc.irregular_kdist(kind, variant=variant)
    atm = synthetic.make_atmosphere(ncol, nlay, nbnd_lw=kd0.nbnd, nbnd_sw=kd0.nbnd, seed=13)
    col_dry, col_gas = gc.gas_columns(oracle_f64, kd0, atm)
    gc.assert_clear_of_nodes(kd0, atm.p_lay, atm.t_lay, col_gas)
    out, c = run_windowed_form(hip_f64, capfd, kd0, atm, col_dry, col_gas)
    print(c)
    nlist = NXW if kind == "lw" else NCW
    want = check_windowed_tables(hip_f64, kd0, nlist, with_bands=(kind == "lw"), with_lims=False)
    assert want["bad"][0][-1] > 0 and want["bad"][1][-1] == 0 and want["regular"] == 0
    tropo = ref.interpolation(kd0, atm.p_lay, atm.t_lay, col_gas)["tropo"]
    blocks = [tropo[:, :256], tropo[:, 256:]]
    n_lower = sum(int(b.all(axis=1).sum()) for b in blocks); n_upper = sum(int((~b).all(axis=1).sum()) for b in blocks)
    assert n_lower > 0 and n_upper > 0 and n_lower + n_upper == 2 * nlay
    assert c["chunk form"] == c["handed"] == n_lower, (c, n_lower)
    match_reference("irregular", kd0, atm, col_dry, col_gas, out)


@pytest.mark.parametrize("kind", ["lw", "sw"])
@pytest.mark.parametrize("bands", ["16-per-band", "band-aligned"])
def test_mixed_hand_backs_with_the_chunk_loop_split_over_parts(bands, kind, capfd, hip_f64, oracle_f64):
    """70 columns: 2 x 8 workgroups of 64 columns x 4 layers, the chunk loop split over four parts. The first 64 columns swing in
    ozone (eta spread), the 6 behind them are alike (the tropopause rows come back, the others stay). 16-g-point bands: a part is
    a range of chunks and is handed back alone; band-aligned chunks: part 0 takes them all and hands back "the whole range". Either
    way the gather kernel redoes the entries in its shares."""
    ncol, nlay = 70, 30
    if bands == "16-per-band":
        kd0 = synthetic.make_kdist(kind, ngpt=80, nbnd=5, npres=20, nflav=4, nminor_lower=9, nminor_upper=5)
    else:
        kd0 = gc.irregular_kdist(kind, variant="fits")
    atm = gc.census_atmosphere(4, kd0, ncol, nlay, wide=64, z_top=35.e3)     # (thin layers: four of them fit a box of table nodes)
    col_dry, col_gas = gc.gas_columns(oracle_f64, kd0, atm)
    gc.assert_clear_of_nodes(kd0, atm.p_lay, atm.t_lay, col_gas)
    out, c = run_windowed_form(hip_f64, capfd, kd0, atm, col_dry, col_gas)
    print(c)
    want = check_windowed_tables(hip_f64, kd0, NXW if kind == "lw" else NCW, with_bands=(kind == "lw"), with_lims=False)
    geom, nblk = grid_of(ncol, nlay)
    nz = parts_of(nblk, kd0.ngpt)
    assert geom == 0 and nblk == 16 and nz == 4 and c["total"] == nblk * nz
    assert want["regular"] == (1 if bands == "16-per-band" else 0)
    assert c["eta"] > 0 and c["regimes"] > 0 and 0 < c["handed"] < (c["total"] if want["regular"] else nblk), c
    match_reference("regular" if bands == "16-per-band" else "irregular", kd0, atm, col_dry, col_gas, out)


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) table edges
@pytest.mark.parametrize("kind", ["lw", "sw"])
def test_table_edges_column_by_column(kind, capfd, hip_f64, oracle_f64):
    """Neighbouring columns take the edge patterns in turn: every lane of a wavefront clamps, extrapolates or falls back differently."""
    kd0, atm, col_dry, col_gas, _ = gc.family_case(oracle_f64, "edges", kind, 193, 30)
    check_every_entry(hip_f64, oracle_f64, capfd, "edges", kd0, atm, col_dry, col_gas, fluxes=False)


@pytest.mark.parametrize("kind", ["lw", "sw"])
@pytest.mark.parametrize("patterns", [("p_high", "p_low"), ("t_low", "t_high"), ("no_second", "no_both")], ids=lambda p: "+".join(p))
def test_table_edges_workgroup_by_workgroup(patterns, kind, capfd, hip_f64, oracle_f64):
    """The 256 columns of a workgroup share a pattern (the 44 behind them the other): the windowed kernel itself stages boxes at the
    first and last pressure nodes, beyond both ends of temp_ref, and at eta = 1 and the col_mix fall-back."""
    ncol, nlay = 300, 30
    kd0, atm, col_dry, col_gas, _ = gc.family_case(oracle_f64, "edges", kind, ncol, nlay, variant="fits", block=256, patterns=patterns)
    out, c = run_windowed_form(hip_f64, capfd, kd0, atm, col_dry, col_gas)
    print(c)
    R = match_reference("edges", kd0, atm, col_dry, col_gas, out)
    geom, nblk = grid_of(ncol, nlay)
    assert geom == 1 and c["total"] == nblk * 4 and c["handed"] <= nblk // 4, c
    pos = ref.positions(kd0, atm.p_lay, atm.t_lay, col_gas)
    fpress, ftemp, eta = pos["press"] - R["it_jpress"], pos["temp"] - R["it_jtemp"], pos["eta"] / (kd0.neta - 1)
    if patterns[0] == "p_high":
        assert fpress[:, :256].min() < -0.5 and fpress[:, 256:].max() > 1.3
    elif patterns[0] == "t_low":
        assert ftemp[:, :256].min() < -0.5 and ftemp[:, 256:].max() > 1.3
    else:
        assert (eta[:, :, :256] == 1).any() and (R["it_col_mix"][:, :, 256:] == 0).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) fp32
@pytest.mark.parametrize("kind", ["lw", "sw"])
@pytest.mark.parametrize("family", ["irregular", "edges"])
def test_fp32_direct_and_fractions_forms(family, kind, capfd, hip_f32, oracle_f64):
    kd0, atm, col_dry, col_gas, _ = gc.family_case(oracle_f64, family, kind, 193, 30, np.float32)
    kd32 = kd0.astype(np.float32)
    R = gc.reference_outputs(kd32, atm, col_dry, col_gas, np.float64, work=np.float32)
    H = Hip(hip_f32, kd0, atm, col_dry, col_gas)
    if kind == "lw":
        for what, fn in (("gather", lambda: gather_only(hip_f32, H.lw_direct)), ("windowed", H.lw_direct)):
            close(family, "tau", fn(), R["tau"], f32=True, what="lw_direct " + what)
        pd = H.planck_direct()
        for k in ("lay_src", "lev_src", "sfc_src", "sfc_src_jac"):
            close(family, k, pd[k], R[k], f32=True, what="planck_source_direct")
        for what, fr in (("planck_fractions", H.planck_fractions()), ("lw_fractions", windowed(capfd, H.lw_fractions)[0])):
            for k in LW_KEYS + (("tau",) if "tau" in fr else ()):
                close(family, k, fr[k], R[k], f32=True, what=what)
    else:
        for what, sw in (("gather", gather_only(hip_f32, H.sw_direct)), ("windowed", H.sw_direct())):
            for k in ("tau", "ssa"):
                close(family, k, sw[k], R[k], f32=True, what="sw_direct " + what)
