"""The longdouble LW two-stream truth of tests/lw2s_truth.py, pinned without a GPU: closed forms, the layer against mpmath at 60 digits,
the conditions on the inputs that tests/test_gpu_lw2s_truth.py relies on, how far the two numpy models sit from it regime by regime, the
list of unresolved cells, and a demonstration on model arithmetic alone that the GPU test's bound rejects wrong kernels.

Norm: lw_ref.profile_error per (g-point, column) profile and quantity, in eps of the dtype. Bound of the GPU test: per regime and
quantity 8 x max(E_regime, 32 eps), E_regime the regrouped model's worst error against the same truth (lw_ref.bound_eps).

The record that is asserted (RECORD, within a factor of 2 either way: the worst error over lw2s_truth.CASES, the entries general /
fused / null and runs with and without incident flux, at lw2s_truth.SEED; measured on a CPU, nothing here runs on a GPU):

    regime              fp64 regrouped   fp64 written    fp32 regrouped   fp32 written
    opaque              2.6 eps          2.2 eps         2.4 eps          2.1 eps
    moderate            3.6              19              3.4              18
    moderate_cloud      4.6              1.6e2           4.4              83
    wide                4.7              8.9e3           4.9              1.3e4
    switch              1.1e2            2.4e6           1.2e2            3.4e6
    near_conservative   1.1e2            1.4e6           1.3e2            8.7e5
    thin_lit            1.6e2            1.9e9           1.2e2            8.0e7
    conservative        3.3e3            1.1e10          3.5e2            1.5e8
    thin_unlit          7.4e3            7.7e10          1.2e4            1.2e10
    thin_dark           1.8e4            2.5e10          3.6e4            4.6e10
  by quantity, regrouped: flux_up is at most 1.6e2 eps in every regime but conservative (fp64 3.3e3, fp32 3.4e2); the figures beyond
  that are flux_dn's where it is layer emission alone (thin_unlit 7.4e3 / 1.2e4, thin_dark 1.8e4 / 3.6e4).

This is the weakness of the per-g-point yardstick of tests/test_gpu_lw_2stream.py written down: the as-written form it compares with
(lw2s_ref.solve) is 2e6 ... 8e10 eps from truth on every thin g-point -- an error of order one in fp32 and of 1e-9 ... 1e-5 in fp64 -- so its
tolerances (2.1e-8 fp64, 9.1e-2 fp32, in a norm over the array's largest value) are the reference's error, and a kernel wrong by a percent
on a thin g-point passes it. The regrouped form is within 2e2 eps wherever a flux is lit and within 4e4 where flux_dn is layer emission alone.

Unresolved cells (UNRESOLVED, asserted from the regrouped model alone): a (regime, quantity, dtype) cell whose bound exceeds 1e-2 of the
profile's largest flux tests nothing. They are flux_dn of thin_dark and thin_unlit in fp32 and nothing else: the regrouped formula leaves
an absolute error of a few eps in c, and (lev_bot - lev_top) c against a layer emission of tau G lev is eps (lev_bot - lev_top)/(tau G lev),
of order one at tau = 1e-7 in fp32. In fp64 the largest bound is 8 x 1.8e4 eps = 3.2e-11. The conservative regime would be a third
unresolved cell in fp32 with the wide range of optical depths; its range is narrowed for fp32 instead (lw2s_truth.CONSERVATIVE_F32).

What the bound catches (test_bound_rejects_wrong_models, a perturbed regrouped model in place of a kernel, general entry, at every
case): exp off by 2^-40 (fp64) / 2^-18 (fp32) in (thin_lit, flux_dn), by at least 99 x / 2.9 x the bound; the thin-layer switch at 1e-7 in (switch, flux_dn); the term
(lev_bot - lev_top) c dropped in (moderate, flux_up). lw2s_truth's SENSITIVITY note says how the draws were shaped for it."""
import mpmath
import numpy as np
import pytest

import lw_ref
import lw2s_truth as T
from lw2s_truth import CASES, IDS, SHAPES, REGIMES, QUANTITIES, NGPT, NBND, as_dict

L = np.longdouble
EPS_L = np.finfo(L).eps
EPS64 = np.finfo(np.float64).eps
RECORD = {("f64", "regrouped"): dict(opaque=2.6, moderate=3.6, moderate_cloud=4.6, wide=4.7, switch=1.1e2, near_conservative=1.1e2, thin_lit=1.6e2,
                                     conservative=3.3e3, thin_unlit=7.4e3, thin_dark=1.8e4),
          ("f64", "written"): dict(opaque=2.2, moderate=19., moderate_cloud=1.6e2, wide=8.9e3, switch=2.4e6, near_conservative=1.4e6, thin_lit=1.9e9,
                                   conservative=1.1e10, thin_unlit=7.7e10, thin_dark=2.5e10),
          ("f32", "regrouped"): dict(opaque=2.4, moderate=3.4, moderate_cloud=4.4, wide=4.9, switch=1.2e2, near_conservative=1.3e2, thin_lit=1.2e2,
                                     conservative=3.5e2, thin_unlit=1.2e4, thin_dark=3.6e4),
          ("f32", "written"): dict(opaque=2.1, moderate=18., moderate_cloud=83., wide=1.3e4, switch=3.4e6, near_conservative=8.7e5, thin_lit=8.0e7,
                                   conservative=1.5e8, thin_unlit=1.2e10, thin_dark=4.6e10)}
UNRESOLVED = {("thin_dark", "flux_dn", "f32"), ("thin_unlit", "flux_dn", "f32")}
EXP_REL = {"f64": 2.0**-40, "f32": 2.0**-18}
REJECTED_IN = {"exp_rel": ("thin_lit", "flux_dn"), "thin_switch": ("switch", "flux_dn"), "drop_c": ("moderate", "flux_up")}
MIN_PROFILES = 9


def test_longdouble_is_wider_than_the_runs():
    assert EPS_L < 1.1e-19, "np.longdouble is not the 80-bit format: the truth would be no more precise than the fp64 run"


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------
def test_h_factor_series_and_closed_form_agree_at_the_hand_over():
    """both forms on [0.5, 1.5] against each other: the closed form loses at most five bits there (h(0.5) = -0.03 from terms of 1)"""
    y = np.linspace(L(0.5), L(1.5), 401, dtype=L)
    term = y * y / 6
    series = -term
    for n in range(2, 80):
        term = -term * y * n / ((n - 1) * (n + 2))
        series -= term
    closed = 2 * (-np.expm1(-y)) / y - 1 - np.exp(-y)
    assert np.max(np.abs(series - closed) / np.abs(closed)) <= 256 * EPS_L
    assert np.max(np.abs(T.h_factor(y) - closed) / np.abs(closed)) <= 256 * EPS_L
    small = L(1e-3)
    assert abs(T.h_factor(small) - (-small**2 / 6 + small**3 / 12 - small**4 / 40)) <= 1e-3**5
    assert T.h_factor(L(0)) == 0
    assert abs(T.h_factor(L(1e4)) - (L(2e-4) - 1)) <= 4 * EPS_L


@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
def test_isothermal_cavity(top_at_1):
    """every source B, incident flux pi B: flux_up = flux_dn = pi B at every level for any tau, ssa, g and emissivity. The residue of the
    thin-layer switch, as tests/test_gpu_lw_2stream.py states it: a layer at or below 1e-8 transmits exp(-D tau) but emits nothing, so
    the closure holds up to D x the sum of tau over those layers (here 3 layers of 1e-9: 5e-9), and exactly without them"""
    rng = np.random.default_rng(11)
    ngpt, nlay, ncol = 4, 23, 5
    shp = (ngpt, nlay, ncol)
    tau = 10.0**rng.uniform(-7, 1.5, shp)
    tau[:, [0, 9]] = 0.0
    ssa, g = rng.uniform(0, 1, shp), rng.uniform(-0.5, 0.95, shp)
    ssa[0] = 1.0
    ssa[1] = 0.0
    B = rng.uniform(5, 40, (ngpt, 1, ncol))
    lev = np.broadcast_to(B, (ngpt, nlay + 1, ncol))
    emis = rng.uniform(0.5, 1, (ngpt, ncol))
    want = T.PI_L * B.astype(L)
    for below in (False, True):
        tau_run = tau.copy()
        if below:
            tau_run[:, [3, 4, 15]] = 1e-9
        up, dn = T.solve_truth(tau_run, ssa, g, lev, emis, B[:, 0], np.pi * B[:, 0], top_at_1)
        resid = max(float(np.max(np.abs(up - want) / want)), float(np.max(np.abs(dn - want) / want)))
        # (the incident flux pi B is given in float64: its rounding, up to eps/2 of fp64 each for pi and the product, is the tolerance)
        assert resid <= (1.66 * 3e-9 * 1.01 if below else EPS64), (below, resid)
        assert (resid > 1e-10) == below


def test_one_thick_absorbing_layer_against_its_analytic_value():
    """ssa = 0: Rdif = 0, Tdif = exp(-D tau), src_up = pi ((Z + lev_top) - Tdif (Z + lev_bot)) with Z = (lev_bot - lev_top)/(D tau); at
    tau = 2 nothing in those expressions cancels"""
    tau, lt, lb, emis, ssrc, inc = 2.0, 12.5, 31.0, 0.9, 30.0, 2.5
    one = lambda x, shape: np.full(shape, x, dtype=np.float64)
    for top_at_1 in (True, False):
        lev = np.array([lt, lb] if top_at_1 else [lb, lt]).reshape(1, 2, 1)
        up, dn = T.solve_truth(one(tau, (1, 1, 1)), one(0, (1, 1, 1)), one(0.3, (1, 1, 1)), lev, one(emis, (1, 1)), one(ssrc, (1, 1)), one(inc, (1, 1)), top_at_1)
        top, sfc = (0, 1) if top_at_1 else (1, 0)
        tr = np.exp(-(T.D_L * L(tau)))
        Z = (L(lb) - L(lt)) / (T.D_L * L(tau))
        s_up = T.PI_L * ((Z + lt) - tr * (Z + lb))
        s_dn = T.PI_L * ((-Z + lb) - tr * (-Z + lt))
        dn_sfc = L(inc) * tr + s_dn
        up_sfc = dn_sfc * (1 - L(emis)) + T.PI_L * L(emis) * L(ssrc)
        want = {"dn_top": L(inc), "dn_sfc": dn_sfc, "up_sfc": up_sfc, "up_top": up_sfc * tr + s_up}
        got = {"dn_top": dn[0, top, 0], "dn_sfc": dn[0, sfc, 0], "up_sfc": up[0, sfc, 0], "up_top": up[0, top, 0]}
        for k in want:
            assert abs(got[k] - want[k]) <= 32 * EPS_L * abs(want[k]), (top_at_1, k)


def test_the_two_orientations_mirror_each_other():
    dt, shape = "f64", SHAPES["f64"][0]
    I = T.inputs(dt, *shape)
    a = T.solve_truth(I["tau"], I["ssa"], I["g"], I["lev"], I["emis"], I["ssrc"], I["inc"], False)
    b = T.solve_truth(*(np.ascontiguousarray(I[k][:, ::-1]) for k in ("tau", "ssa", "g", "lev")), I["emis"], I["ssrc"], I["inc"], True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y[:, ::-1])
    for form in ("regrouped", "written"):
        a = T.solve_model(I["tau"], I["ssa"], I["g"], I["lev"], I["emis"], I["ssrc"], I["inc"], False, form)
        b = T.solve_model(*(np.ascontiguousarray(I[k][:, ::-1]) for k in ("tau", "ssa", "g", "lev")), I["emis"], I["ssrc"], I["inc"], True, form)
        for x, y in zip(a, b):
            assert np.array_equal(x, y[:, ::-1])


def test_combine_truth_by_hand():
    gb = np.array([1, 2, 2], dtype=np.int32)
    tau_g = np.array([0.5, 0.0, 0.25]).reshape(3, 1, 1)
    cld = tuple(np.array(v).reshape(2, 1, 1) for v in ([0.0, 0.75], [0.3, 1.0], [0.7, 0.2]))
    tau, ssa, g = T.combine_truth(tau_g, cld, gb)
    assert tau.dtype == L and list(tau.ravel()) == [0.5, 0.75, 1.0] and list(ssa.ravel()) == [0.0, 1.0, 0.75]
    assert np.allclose(g.ravel().astype(float), [0.7, 0.2, 0.2])
    tau, ssa, g = T.combine_truth(tau_g, None, gb)
    assert list(tau.ravel()) == [0.5, 0.0, 0.25] and not ssa.any() and not g.any()


# ---- the truth's layer against mpmath ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_truth_layer_against_the_formulas_as_written_at_60_digits(dt):
    """Every layer of the smallest shape (all regimes): Rdif, Tdif absolutely, src_up, src_dn over pi max(lev) min(1, tau) (their relative
    error means nothing where a conservative layer emits nothing), against the as-written formulas in mpmath at 60 digits. Bound: 1/16 eps
    of fp64. The floor of k^2 and the switch are taken as the run's dtype holds 1e-12 and 1e-8."""
    mp = mpmath.mp.clone()
    mp.dps = 60
    mpf = mp.mpf
    F = T.np_dtype(dt)
    I = T.inputs(dt, *SHAPES[dt][0])
    tau, ssa, g, lev = (I[k] for k in ("tau", "ssa", "g", "lev"))
    thick = tau > F(T.TAU_THIN)
    conv = lambda a: np.asarray(a).astype(L)
    got = T.truth_layer(conv(tau), conv(ssa), conv(g), conv(lev[:, :-1]), conv(lev[:, 1:]), thick, L(F(T.K2_MIN)))
    D, k2min, pi = mpf("1.66"), mpf(float(F(T.K2_MIN))), mp.pi
    to_mp = lambda x: mpf(float(x))                                    # a float32 / float64 widens exactly
    worst = dict.fromkeys(REGIMES, 0.0)
    for ig, reg in enumerate(T.GPOINT_REGIMES):
        for il in range(tau.shape[1]):
            for ic in range(tau.shape[2]):
                t, w, gg, lt, lb = (to_mp(a[ig, il, ic]) for a in (tau, ssa, g, lev[:, :-1], lev[:, 1:]))
                gamma1, gamma2 = D * (1 - w * (1 + gg) / 2), D * w * (1 - gg) / 2
                k = mp.sqrt(max((gamma1 - gamma2) * (gamma1 + gamma2), k2min))
                e1 = mp.exp(-t * k)
                e2 = e1 * e1
                rt = 1 / (k * (1 + e2) + gamma1 * (1 - e2))
                R, Tr = rt * gamma2 * (1 - e2), 2 * rt * k * e1
                if thick[ig, il, ic]:
                    Z = (lb - lt) / (t * (gamma1 + gamma2))
                    su = pi * ((Z + lt) - R * (-Z + lt) - Tr * (Z + lb))
                    sd = pi * ((-Z + lb) - R * (Z + lb) - Tr * (-Z + lt))
                else:
                    su = sd = mpf(0)
                scale = pi * max(lt, lb) * min(mpf(1), t)
                errs = [abs(mpf_from_L(mp, got[0][ig, il, ic]) - R), abs(mpf_from_L(mp, got[1][ig, il, ic]) - Tr)]
                if scale > 0:
                    errs += [abs(mpf_from_L(mp, got[2][ig, il, ic]) - su) / scale, abs(mpf_from_L(mp, got[3][ig, il, ic]) - sd) / scale]
                else:
                    assert got[2][ig, il, ic] == 0 and got[3][ig, il, ic] == 0
                worst[reg] = max(worst[reg], float(max(errs)) / EPS64)
    print(f"LW2STRUTH truth layer vs mpmath {dt}: " + ", ".join(f"{r} {w:.2g}" for r, w in worst.items() if r != "thin_unlit") + " eps of fp64")
    for r, w in worst.items():
        assert w <= 1. / 16., (r, w)


def mpf_from_L(mp, x):
    """a longdouble as an mpf, exactly: its float64 head and the float64 remainder"""
    hi = np.float64(x)
    return mp.mpf(float(hi)) + mp.mpf(float(np.float64(x - L(hi))))


# ---- the conditions the GPU tests rely on -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_every_regime_is_populated_and_inside_its_interval(dt):
    F = T.np_dtype(dt)
    ranges = T.regime_ranges(dt)
    sw = F(T.TAU_THIN)
    assert len(set(s[1] for s in SHAPES[dt])) == 10 and all(9 <= s[0] <= 20 for s in SHAPES[dt]) and any(s[0] % 2 for s in SHAPES[dt])
    for ncol, nlay in SHAPES[dt]:
        I = T.inputs(dt, ncol, nlay)
        reg = T.regimes(dt, ncol, nlay)
        assert I["tau"].dtype == F and reg.shape == (NGPT, ncol) and all(not v.flags.writeable for v in I.values())
        for r in set(T.GPOINT_REGIMES):
            assert int((reg == r).sum()) >= MIN_PROFILES, (ncol, nlay, r)
        assert set(T.regimes(dt, ncol, nlay, False)[T.GPOINT_REGIMES.index("thin_lit")]) == {"thin_unlit"}
        tau, ssa, g = I["tau"], I["ssa"], I["g"]
        assert np.array_equal(tau, I["tau_g"] + I["tau_c"][I["gb"] - 1])                        # the combined tau as the run's dtype holds it
        # no tau, combined or given, within 4 ulp of the thin-layer switch
        for t in (tau, I["tau_g"], I["tau_c"]):
            assert not np.any(np.abs(t.astype(L) - L(sw)) <= 4 * np.spacing(sw)), (ncol, nlay)
        for ig, r in enumerate(T.GPOINT_REGIMES):
            lo, hi = ranges[r]
            x = tau[ig].astype(np.float64)
            body = np.ones(nlay, dtype=bool)
            if r in ("conservative", "wide"):
                body[[0, nlay // 2, nlay - 1]] = False
                assert np.all(x[~body] == 0)
            if r == "switch":
                body = np.arange(nlay) % 3 != 1
                assert set(np.unique(x[~body])) <= {0.0, float(F(1e-9))} and np.all(x[~body] < sw / 4) and (~body).sum() >= nlay // 3
                assert np.all(x[body] > sw)
            if r == "opaque":
                body[1:3] = False
                with np.errstate(under="ignore"):
                    e1, e0 = np.exp(-(tau[ig, 1] * F(1.66))), np.exp(-(tau[ig, 2] * F(1.66)))
                assert np.all((e1 > 0) & (e1 < np.finfo(F).tiny)) and np.all(e0 == 0) and np.all(ssa[ig, 1:3] == 0)
            assert x[body].min() >= lo and x[body].max() <= hi, (ncol, nlay, ig, r, x[body].min(), x[body].max())
            if r in ("thin_dark", "moderate"):
                assert not ssa[ig].any()
            if r in ("thin_lit", "switch", "moderate_cloud", "opaque"):
                assert np.all(ssa[ig][body] > 0) and ssa[ig].max() <= 0.9 and g[ig].min() >= -0.3 and g[ig].max() <= 0.9
            if r == "near_conservative":
                assert np.all((1 - ssa[ig].astype(L)) >= 0.9e-4) and np.all((1 - ssa[ig].astype(L)) <= 1.1e-2)
            if r == "conservative":
                assert np.all(ssa[ig][body] == 1) and not I["tau_g"][ig].any()
            if r == "wide":
                cloudy = np.count_nonzero(I["tau_c"][I["gb"][ig] - 1]) / (nlay * ncol)
                assert 0.08 <= cloudy <= 0.35, cloudy
        # SENSITIVITY: the switch band is isothermal per column, its second g-point has neither incident flux nor surface emission and
        # half of its layers above the switch lie below 1e-7
        sws = [ig for ig, r in enumerate(T.GPOINT_REGIMES) if r == "switch"]
        assert np.all(I["lev"][sws] == I["lev"][sws][:, :1]) and sws[1] == T.UNLIT_SURFACE and not I["ssrc"][sws[1]].any() and np.all(I["ssrc"][sws[0]] > 0)
        x = tau[sws[1]][np.arange(nlay) % 3 != 1]
        assert 0.3 <= np.mean(x <= 1e-7) and np.mean(x <= 1e-7) <= 0.99 and np.all((x <= 1e-7).any(axis=0))
        assert np.all(I["lev"][T.GPOINT_REGIMES.index("thin_dark")] > 0)
        assert np.all(I["emis"][:, ::3] == 1) and np.all(np.delete(I["emis"], np.s_[::3], axis=1) < 1)
        lit = [ig for ig in range(NGPT) if ig not in T.DARK_GPOINTS]
        assert np.all(I["inc"][list(T.DARK_GPOINTS)] == 0) and np.all(I["inc"][lit] > 0) and 0 in T.DARK_GPOINTS
        # bands: uneven, contiguous, one regime each; thin_dark (ill-conditioned) and moderate (well-conditioned) each fill a band
        assert sorted(set(int(h - l + 1) for l, h in I["band_lims"])) == [1, 2, 3] and NBND == 9
        for ib in range(NBND):
            assert np.all(I["gb"][T.band_gpoints(ib)] == ib + 1) and len(set(T.GPOINT_REGIMES[i] for i in T.band_gpoints(ib))) == 1
    assert T.column_regimes(T.regimes(dt, 9, 80))[0] == "thin_dark" and T.column_regimes(T.regimes(dt, 9, 80, False)[1:])[0] == "thin_unlit"
    lit = [ig for ig, r in enumerate(T.GPOINT_REGIMES) if r == "thin_lit"]                    # SENSITIVITY: the lapse of the thin_lit band
    assert np.all(np.diff(T.inputs(dt, 9, 80)["lev"][lit].astype(L), axis=1) > 0)


# ---- the models' distance from truth, the unresolved cells, the bound with a model in place of a kernel ----------------------------------------
def _cell_errors(dt, shape, top_at_1, entry, with_inc, form, hooks=()):
    """{(regime, quantity): worst error in eps} of a model on a case, per g-point"""
    eps = np.finfo(T.np_dtype(dt)).eps
    reg = T.regimes(dt, *shape, with_inc)
    tr, m = T.truth(dt, *shape, top_at_1, entry, with_inc), T.model(dt, *shape, top_at_1, entry, with_inc, form, hooks)
    out = {}
    for q, a, t in zip(QUANTITIES, m, tr):
        assert np.isfinite(a).all() or form == "written", (q, entry)
        e = lw_ref.profile_error(np.nan_to_num(a, nan=np.inf), t) / eps
        for r in REGIMES:
            if (reg == r).any():
                out[(r, q)] = float(e[reg == r].max())
    return out


@pytest.fixture(scope="module")
def table():
    """worst[(dt, form)][(regime, quantity)] over every case, entry and run with / without incident flux"""
    worst = {}
    for dt, shape, top_at_1 in CASES:
        for form in ("regrouped", "written"):
            w = worst.setdefault((dt, form), {})
            for entry in T.ENTRIES:
                for with_inc in (True, False):
                    for cell, e in _cell_errors(dt, shape, top_at_1, entry, with_inc, form).items():
                        w[cell] = max(w.get(cell, 0.0), e)
    return worst


def test_models_stay_inside_the_recorded_table(table):
    for (dt, form), w in table.items():
        per_regime = {r: max(e for (rr, q), e in w.items() if rr == r) for r in REGIMES}
        print(f"LW2STRUTH E_regime {dt} {form}: " + ", ".join(f"{r} {e:.2g}" for r, e in per_regime.items()) + " eps")
        for q in QUANTITIES:
            print(f"LW2STRUTH     {q}: " + ", ".join(f"{r} {w[(r, q)]:.2g}" for r in REGIMES))
    for (dt, form), w in table.items():
        for r in REGIMES:
            e = max(v for (rr, q), v in w.items() if rr == r)
            assert RECORD[(dt, form)][r] / 2 <= e <= RECORD[(dt, form)][r] * 2, (dt, form, r, e)
    assert list(REGIMES) == sorted(REGIMES, key=RECORD[("f64", "regrouped")].get)        # the order column_regimes relies on


def test_unresolved_cells_are_the_listed_ones(table):
    """from the regrouped model alone: the cells whose bound 8 x max(E_regime, 32 eps) exceeds 1e-2 of the profile's largest flux"""
    found, largest = set(), {"f64": 0.0, "f32": 0.0}
    for (dt, form), w in table.items():
        if form != "regrouped":
            continue
        eps = float(np.finfo(T.np_dtype(dt)).eps)
        for (r, q), e in w.items():
            frac = lw_ref.bound_eps(e) * eps
            if frac > T.UNRESOLVED_FRACTION:
                found.add((r, q, dt))
            else:
                largest[dt] = max(largest[dt], frac)
    print(f"LW2STRUTH unresolved cells: {sorted(found)}; the largest resolved bound: fp64 {largest['f64']:.2g}, fp32 {largest['f32']:.2g} of the flux")
    assert found == UNRESOLVED
    assert all(dt == "f32" and q == "flux_dn" and r in ("thin_dark", "thin_unlit") for r, q, dt in found)


def _verdict(dt, shape, top_at_1, entry, with_inc, hooks=(), quiet=True):
    rep = T.report(dt, label="model", quiet=quiet)
    rep.check(f"model{dict(hooks) or ''} {entry} {shape} top_at_1={top_at_1} inc={with_inc}",
              as_dict(T.model(dt, *shape, top_at_1, entry, with_inc, "regrouped", hooks)), as_dict(T.model(dt, *shape, top_at_1, entry, with_inc)),
              as_dict(T.truth(dt, *shape, top_at_1, entry, with_inc)), T.regimes(dt, *shape, with_inc))
    return rep


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_bound_rejects_wrong_models(dt, shape, top_at_1):
    """general entry with incident flux: the plain model is inside the bound in every cell; each perturbed one is outside in the cell
    REJECTED_IN names"""
    _verdict(dt, shape, top_at_1, "general", True, quiet=False).done()
    for hooks in ((("exp_rel", EXP_REL[dt]),), (("thin_switch", 1e-7),), (("drop_c", True),)):
        rep = _verdict(dt, shape, top_at_1, "general", True, hooks)
        cell = REJECTED_IN[hooks[0][0]]
        k, e, b = rep.worst[(cell[1], cell[0])]
        print(f"LW2STRUTH {dt} {shape} top_at_1={top_at_1} {hooks[0][0]}: {cell} model {k:.3g} eps, bound {b:.3g} eps, outside in {sorted(rep.outside_cells)}")
        assert cell in rep.outside_cells, (hooks, sorted(rep.outside_cells))


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_plain_model_passes_in_the_summed_forms(dt, shape, top_at_1):
    """the sums of the fused entry (all g-points; the thin_dark, moderate and conservative bands alone): the model summed in g-point order in the run's
    dtype, the truth in longdouble; a column takes the regime lw2s_truth.column_regimes gives it"""
    rep = T.report(dt, label="model", quiet=True)
    for entry in ("fused", "null"):
        for with_inc in (True, False):
            reg = T.regimes(dt, *shape, with_inc)
            m, t = T.model(dt, *shape, top_at_1, entry, with_inc), T.truth(dt, *shape, top_at_1, entry, with_inc)
            for gpts in (np.arange(NGPT), T.band_gpoints(0), T.band_gpoints(3), T.band_gpoints(6)):
                rep.check(f"sum of g-points {gpts.tolist()}", as_dict(m, gpts, True), as_dict(m, gpts, True), as_dict(t, gpts), T.column_regimes(reg[gpts]))
    rep.done()
    assert [set(T.column_regimes(reg[T.band_gpoints(ib)])) for ib in (0, 3, 6)] == [{"thin_dark"}, {"moderate"}, {"conservative"}]
