"""The longdouble LW no-scattering solve of tests/lw_ref.py, pinned without a GPU: closed forms, the conditions on the inputs that
tests/test_gpu_lw_truth.py relies on, how far the CPU oracle and a numpy model sit from it regime by regime, and a demonstration, on
reference-side arithmetic alone, that the bound of the GPU test rejects wrong kernels.

Norm: lw_ref.profile_error, one number per (g-point, column) profile and quantity (flux_up, flux_dn, flux_up_jac separately): the largest
|got - truth| over the levels over the profile's largest truth value of that quantity, in units of the dtype's eps. Regimes:
lw_ref.GPOINT_REGIMES, one per g-point (lw_ref.regime_ranges); every regime holds at least 9 profiles at every shape (the smallest column
count), thin and seam twice as many.

The record that is asserted (RECORD: the oracle's worst error over the shapes, orientations, quantities and angle sets of lw_ref.CASES
at lw_ref.SEED = 5151; the oracle must stay below 8 x these). Measured on a CPU; nothing in this file runs on a GPU.

    regime        fp64 oracle vs truth     fp32 oracle vs truth
    opaque        1.2 eps                  1.4 eps
    moderate      4.7 eps                  4.9 eps
    thin_dark     4.2e2 eps                9.4 eps
    plain         6.0e3 eps                43 eps
    thin          1.3e4 eps                97 eps
    hot_layer     1.6e4 eps                1.6e2 eps
    just_thick    4.7e5 eps                45 eps
    seam          6.6e6 eps                3.4e2 eps

The fp64 column follows the cancellation in fact = (1 - trans)/tl - trans, which costs 2 eps / tl^2 just above the switch
tl = eps^(1/4) = 1.2e-4 (seam, just_thick) and eps / tl in 1 - trans below it (thin); where every layer is moderately thick or opaque the
reference is at rounding level. Within a regime the figure varies by up to 11 x from shape to shape (fp64 thin: 1.2e3 ... 1.3e4 eps, seam
1.3e6 ... 6.6e6; fp32 hot_layer: 17 ... 155), which is why the GPU test measures E_regime on ITS inputs instead of quoting this table.

Reference spread. lw_ref.model (numpy in the run's dtype, numpy's exp where the oracle calls the C library's) is a second draw of the same
rounding noise: at every case, regime and quantity each of the two is within 8 x max(the other, 32 eps) -- the model never beyond 0.76
of that, so no bound of the GPU test rests on one lucky draw of the oracle. No seed had to be skipped: seam and just_thick showed no
heavy-tailed outlier at 5151.

What the bound catches (test_bound_rejects_wrong_kernels, with lw_ref.model in place of a kernel and the bound 8 x max(E_regime, 32 eps)
of the GPU test, a regime counting as rejected when any of its quantities is outside): exp off by a relative 2^-40 (fp64) / 2^-18 (fp32)
is rejected in moderate, plain, seam and thin at every case -- the smallest excess over the bound is 2.1e2 / 2.6e3 / 1.9e3 / 6.2e3 x in fp64
and 1.7 / 8.6 / 25 / 37 x in fp32 -- and the series without its last term in thin_dark (4.1e3 x in fp64, 2.1 x in fp32). The unperturbed
model passes everywhere. lw_ref's SENSITIVITY note says how the thin_dark and moderate draws were shaped for the two fp32 figures."""
import numpy as np
import pytest

import lw_ref
from lw_ref import CASES, IDS, SHAPES, REGIMES, QUANTITIES, NGPT, NBND, as_dict

L = np.longdouble
EPS_L = np.finfo(L).eps
RECORD = {"f64": dict(opaque=1.2, moderate=4.7, thin_dark=4.2e2, plain=6.0e3, thin=1.3e4, hot_layer=1.6e4, just_thick=4.7e5, seam=6.6e6),
          "f32": dict(opaque=1.4, moderate=4.9, thin_dark=9.4, plain=43., thin=97., hot_layer=1.6e2, just_thick=45., seam=3.4e2)}
EXP_REL = {"f64": 2.0**-40, "f32": 2.0**-18}
CONFIGS = [("1", True), ("1", False), ("3", True), ("3", False), ("opt", True)]        # (angles, with incident flux)
MIN_PROFILES = 9


def test_longdouble_is_wider_than_the_runs():
    assert EPS_L < 1.1e-19, "np.longdouble is not the 80-bit format: the truth would be no more precise than the fp64 run"


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------
def test_source_factor_series_and_closed_form_agree_at_the_hand_over():
    """Both forms on [0.3, 0.7], whichever side of 0.5 lw_ref.source_factor takes them from, against each other: the closed form loses
    at most three bits to its subtraction there (fact is 0.12 ... 0.19 of its terms), so 64 eps of longdouble"""
    t = np.linspace(L(0.3), L(0.7), 401, dtype=L)
    term = t / 2
    series = term.copy()
    for k in range(2, 60):
        term = -term * t * k / ((k - 1) * (k + 1))
        series += term
    closed = -np.expm1(-t) / t - np.exp(-t)
    assert np.max(np.abs(series - closed) / closed) <= 64 * EPS_L
    got = lw_ref.source_factor(t)
    assert np.array_equal(got[t < 0.5], lw_ref.source_factor(t[t < 0.5]))
    assert np.max(np.abs(got - closed) / closed) <= 64 * EPS_L
    # the first terms by hand, and the limits
    small = L(1e-3)
    assert abs(lw_ref.source_factor(small) - (small / 2 - small**2 / 3 + small**3 / 8 - small**4 / 30)) <= 1e-3**5
    assert lw_ref.source_factor(L(0)) == 0
    assert abs(lw_ref.source_factor(L(1e4)) - L(1e-4)) <= EPS_L


def _one(x, shape):
    return np.full(shape, x, dtype=np.float64)


@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
def test_one_isothermal_layer(top_at_1):
    """lay = lev = B: the layer emits pi B (1 - trans) both ways whatever fact is; the surface reflects 1 - emis of it"""
    tau, D, B, emis, ssrc, inc, sjac = 0.37, 1.66, 21.5, 0.9, 30.0, 2.5, 0.4
    up, dn, jac = lw_ref.solve(_one(D, (1, 1, 1)), np.ones(1), _one(tau, (1, 1, 1)), _one(B, (1, 1, 1)), _one(B, (1, 2, 1)), _one(emis, (1, 1)),
                               _one(ssrc, (1, 1)), _one(inc, (1, 1)), _one(sjac, (1, 1)), top_at_1)
    top, sfc = (0, 1) if top_at_1 else (1, 0)
    pi = L(np.pi) + L(1.2246467991473532e-16)
    tr = np.exp(-(L(tau) * L(D)))
    want_dn_sfc = L(inc) * tr + pi * L(B) * (1 - tr)
    want_up_sfc = want_dn_sfc * (1 - L(emis)) + pi * L(emis) * L(ssrc)
    want = {"dn_top": L(inc), "dn_sfc": want_dn_sfc, "up_sfc": want_up_sfc, "up_top": want_up_sfc * tr + pi * L(B) * (1 - tr),
            "jac_sfc": pi * L(emis) * L(sjac), "jac_top": pi * L(emis) * L(sjac) * tr}
    got = {"dn_top": dn[0, top, 0], "dn_sfc": dn[0, sfc, 0], "up_sfc": up[0, sfc, 0], "up_top": up[0, top, 0], "jac_sfc": jac[0, sfc, 0],
           "jac_top": jac[0, top, 0]}
    for k in want:
        assert abs(got[k] - want[k]) <= 16 * EPS_L * abs(want[k]), k


def test_transparent_columns_return_the_boundary_values():
    """tau = 0 everywhere: flux_dn = inc_flux x the sum of the weights at every level, flux_up = its reflection plus the surface's emission"""
    rng = np.random.default_rng(3)
    ngpt, nlay, ncol = 3, 7, 4
    w = lw_ref.W_THREE
    sec = rng.uniform(1.2, 3.0, (3, ngpt, ncol))
    emis, ssrc, inc, sjac = rng.uniform(0.8, 1, (ngpt, ncol)), rng.uniform(5, 40, (ngpt, ncol)), rng.uniform(0, 5, (ngpt, ncol)), rng.uniform(0.1, 0.6, (ngpt, ncol))
    up, dn, jac = lw_ref.solve(sec, w, np.zeros((ngpt, nlay, ncol)), rng.uniform(5, 40, (ngpt, nlay, ncol)), rng.uniform(5, 40, (ngpt, nlay + 1, ncol)),
                               emis, ssrc, inc, sjac, False)
    pi = L(np.pi) + L(1.2246467991473532e-16)
    sw = w.astype(L).sum()
    want_dn = (inc.astype(L) * sw)[:, None, :]
    want_up = (inc.astype(L) * (1 - emis.astype(L)) * sw + pi * sw * emis.astype(L) * ssrc.astype(L))[:, None, :]
    want_jac = (pi * sw * emis.astype(L) * sjac.astype(L))[:, None, :]
    for got, want in ((dn, want_dn), (up, want_up), (jac, want_jac)):
        assert np.max(np.abs(got - want) / want) <= 16 * EPS_L


def test_opaque_column():
    """tau D = 2e5 in every layer: trans is an exact 0 in longdouble and fact = 1/tl, so the flux leaving a layer is
    pi (lev + 2 (lay - lev)/tl) with the level it leaves through, whatever lies behind; the Jacobian is zero above the surface"""
    rng = np.random.default_rng(4)
    ngpt, nlay, ncol = 2, 5, 3
    tau = np.full((ngpt, nlay, ncol), 1e5)
    lay, lev = rng.uniform(5, 40, (ngpt, nlay, ncol)), rng.uniform(5, 40, (ngpt, nlay + 1, ncol))
    up, dn, jac = lw_ref.solve(np.full((1, ngpt, ncol), 2.0), np.ones(1), tau, lay, lev, np.full((ngpt, ncol), 0.9), np.full((ngpt, ncol), 30.0),
                               np.full((ngpt, ncol), 3.0), np.full((ngpt, ncol), 0.5), True)
    assert np.exp(L(-2e5)) == 0
    pi = L(np.pi) + L(1.2246467991473532e-16)
    tl = L(2e5)
    want_dn = pi * (lev[:, 1:].astype(L) + 2 * (lay.astype(L) - lev[:, 1:].astype(L)) / tl)
    want_up = pi * (lev[:, :-1].astype(L) + 2 * (lay.astype(L) - lev[:, :-1].astype(L)) / tl)
    assert np.max(np.abs(dn[:, 1:] - want_dn) / want_dn) <= 16 * EPS_L
    assert np.max(np.abs(up[:, :-1] - want_up) / want_up) <= 16 * EPS_L
    assert np.all(jac[:, :-1] == 0) and np.all(jac[:, -1] > 0)


def test_planck_sources_and_optimal_secants_by_hand():
    pfrac = np.array([[[0.25], [0.81], [0.04]], [[0.5], [0.5], [0.5]]])                      # (2, 3, 1)
    blay = np.array([[[10.], [20.], [30.]], [[1.], [2.], [3.]]]); blev = np.array([[[1.], [2.], [3.], [4.]], [[5.], [6.], [7.], [8.]]])
    gb = np.array([2, 1], dtype=np.int32)
    lay, lev = lw_ref.planck_sources(pfrac, blay, blev, gb, L)
    assert lay.dtype == L and np.allclose(lay[:, :, 0].astype(float), [[0.25, 2 * 0.81, 3 * 0.04], [5., 10., 15.]])
    assert np.allclose(lev[0, :, 0].astype(float), [0.25 * 5, 0.45 * 6, 0.18 * 7, 0.04 * 8])
    assert np.allclose(lev[1, :, 0].astype(float), [0.5 * 1, 0.5 * 2, 0.5 * 3, 0.5 * 4])
    fit = np.array([[0.1, -0.2], [1.6, 1.7]])
    sec = lw_ref.optimal_secants(np.array([[[0.5], [0.25], [0.25]], [[2.], [0.], [0.]]]), fit, gb)
    assert sec.shape == (1, 2, 1) and sec.dtype == np.float64
    assert np.allclose(sec[0, :, 0], [-0.2 * np.exp(-1.0) + 1.7, 0.1 * np.exp(-2.0) + 1.6], rtol=1e-15)


def test_profile_error_and_column_regimes_by_hand():
    truth = np.zeros((2, 3, 2), dtype=L); truth[0, :, 0] = [1, 2, 4]; truth[0, :, 1] = [1, 1, 1]; truth[1, :, 0] = [0, 0, 8]; truth[1, :, 1] = [2, 2, 2]
    got = truth.astype(np.float64).copy(); got[0, 1, 0] += 0.5; got[1, 0, 1] -= 0.25
    assert np.array_equal(lw_ref.profile_error(got, truth), [[0.125, 0.0], [0.0, 0.125]])
    summed = got.sum(axis=0)
    assert np.array_equal(lw_ref.profile_error(summed, truth), [0.5 / 12, 0.25 / 3])
    with pytest.raises(ValueError):
        lw_ref.profile_error(summed[:2], truth)
    reg = np.array([["opaque", "thin"], ["seam", "moderate"], ["plain", "thin_dark"]])
    assert list(lw_ref.column_regimes(reg)) == ["seam", "thin"]
    assert lw_ref.bound_eps(1.0) == 256.0 and lw_ref.bound_eps(100.0) == 800.0


# ---- the conditions the GPU tests rely on ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_every_regime_is_populated_and_inside_its_interval(dt):
    F = lw_ref.np_dtype(dt)
    T = L(lw_ref.tau_thres(dt))
    ranges = lw_ref.regime_ranges(dt)
    for ncol, nlay in SHAPES[dt]:
        I = lw_ref.inputs(dt, ncol, nlay)
        reg = lw_ref.regimes(dt, ncol, nlay)
        assert I["tau"].dtype == F and reg.shape == (NGPT, ncol)
        for r in REGIMES:
            assert int((reg == r).sum()) >= MIN_PROFILES, (ncol, nlay, r)
        secants = np.concatenate([lw_ref.angles_of(dt, ncol, nlay, a)[0] for a in lw_ref.ANGLES]).astype(L)      # (5, ngpt, ncol)
        assert secants.min() >= lw_ref.D_MIN and secants.max() <= lw_ref.D_MAX
        tl = I["tau"].astype(L)[None] * secants[:, :, None, :]                                                    # every secant of the tests
        for ig, r in enumerate(lw_ref.GPOINT_REGIMES):
            lo, hi = ranges[r]
            x = tl[:, ig]
            assert x.min() >= lo and x.max() <= hi, (ncol, nlay, ig, r, float(x.min()), float(x.max()))
            if r in ("thin_dark", "thin"):
                assert x.max() < T                                      # the series branch alone
            if r == "just_thick":
                assert x.min() > T                                      # the cancelling branch alone
            if r == "seam":                                             # both branches in every profile, for every secant
                assert np.all((x > T).any(axis=1)) and np.all((x <= T).any(axis=1))
            if r in ("plain", "hot_layer"):
                assert np.all(I["tau"][ig][[0, nlay // 2, nlay - 1]] == 0) and np.count_nonzero(I["tau"][ig] == 0) == 3 * ncol
        dark = lw_ref.GPOINT_REGIMES.index("thin_dark")
        assert np.all(I["lev"][dark] == 0) and np.all(I["inc"][dark] == 0) and np.all(I["lay"][dark] > 0)
        hot = [ig for ig, r in enumerate(lw_ref.GPOINT_REGIMES) if r in ("hot_layer", "moderate")]
        assert np.all(I["gb"][hot] == 4) and np.allclose(I["blay"][3], 4.0 * (I["blev"][3, :-1] + I["blev"][3, 1:]), rtol=1e-6)
        caps = np.array(lw_ref.MODERATE_CAPS)[np.arange(ncol) % 4]
        xm = tl[:, lw_ref.GPOINT_REGIMES.index("moderate")].max(axis=(0, 1))
        assert np.all(xm <= caps) and set(np.arange(ncol) % 4) == {0, 1, 2, 3}
        assert np.all(I["emis"][:, ::3] == 1) and np.all(np.delete(I["emis"], np.s_[::3], axis=1) < 1)
        lit = [ig for ig in range(NGPT) if ig not in lw_ref.DARK_GPOINTS]
        assert np.all(I["inc"][list(lw_ref.DARK_GPOINTS)] == 0) and np.all(I["inc"][lit] > 0)
        # opaque, with the one-angle secant: a denormal transmissivity in layer 1 and an exact zero in layer 2
        op = lw_ref.GPOINT_REGIMES.index("opaque")
        with np.errstate(under="ignore"):
            t1, t2 = np.exp(-(I["tau"][op, 1] * I["sec1"][0, op])), np.exp(-(I["tau"][op, 2] * I["sec1"][0, op]))
        assert np.all((t1 > 0) & (t1 < np.finfo(F).tiny)) and np.all(t2 == 0)
        # bands: uneven, contiguous, thin_dark alone
        assert [int(h - l + 1) for l, h in I["band_lims"]] == [1, 3, 4, 2] and NBND == 4
        assert all(np.all(I["gb"][lw_ref.band_gpoints(ib)] == ib + 1) for ib in range(NBND))


# ---- the reference's own distance from truth -----------------------------------------------------------------------------------------------
def _errors(fluxes, truth, eps):
    return {q: lw_ref.profile_error(a, t) / eps for q, a, t in zip(QUANTITIES, fluxes, truth)}


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_oracle_stays_inside_the_recorded_table_and_agrees_with_the_model(dt, shape, top_at_1, oracle_built):
    eps = np.finfo(lw_ref.np_dtype(dt)).eps
    reg = lw_ref.regimes(dt, *shape)
    worst = dict.fromkeys(REGIMES, 0.0)
    for angles, with_inc in CONFIGS:
        truth = lw_ref.truth(dt, *shape, top_at_1, angles, with_inc, False)
        eo = _errors(lw_ref.oracle(dt, *shape, top_at_1, angles, with_inc), truth, eps)
        em = _errors(lw_ref.model(dt, *shape, top_at_1, angles, with_inc), truth, eps)
        for q in QUANTITIES:
            for r in REGIMES:
                o, m = float(eo[q][reg == r].max()), float(em[q][reg == r].max())
                worst[r] = max(worst[r], o)
                assert m <= lw_ref.bound_eps(o) and o <= lw_ref.bound_eps(m), (angles, with_inc, q, r, o, m)
    print(f"oracle vs truth {dt} {shape} top_at_1={top_at_1}: " + ", ".join(f"{r} {w:.3g}" for r, w in worst.items()) + " eps")
    for r, w in worst.items():
        assert w <= 8 * RECORD[dt][r], (r, w)


# ---- the bound of the GPU test, with a model in place of a kernel ---------------------------------------------------------------------------
def _verdict(dt, shape, top_at_1, angles, with_inc, from_fractions, **hooks):
    """The regimes in which the GPU test's bound rejects lw_ref.model(**hooks), per-g-point fluxes"""
    rep = lw_ref.Report(dt, label="model", quiet=True)
    rep.check("model", as_dict(lw_ref.model(dt, *shape, top_at_1, angles, with_inc, **hooks)), as_dict(lw_ref.oracle(dt, *shape, top_at_1, angles, with_inc)),
              as_dict(lw_ref.truth(dt, *shape, top_at_1, angles, with_inc, from_fractions)), lw_ref.regimes(dt, *shape))
    return rep


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_bound_rejects_wrong_kernels(dt, shape, top_at_1, oracle_built):
    """At every case, angle set and for both truths (sources given / formed from the fractions in longdouble): the unperturbed model is
    inside the bound in every regime and quantity; with exp off by 2^-40 / 2^-18 it is outside in moderate, plain, seam and thin; with
    the series one term short it is outside in thin_dark"""
    for angles, with_inc in CONFIGS:
        for from_fractions in (False, True):
            what = (angles, with_inc, from_fractions)
            _verdict(dt, shape, top_at_1, angles, with_inc, from_fractions).done()
            out = _verdict(dt, shape, top_at_1, angles, with_inc, from_fractions, exp_rel=EXP_REL[dt]).outside
            assert {"moderate", "plain", "seam", "thin"} <= out, (what, out)
            out = _verdict(dt, shape, top_at_1, angles, with_inc, from_fractions, short_series=True).outside
            assert "thin_dark" in out, (what, out)


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_unperturbed_model_passes_in_the_summed_forms(dt, shape, top_at_1, oracle_built):
    """The g-point sums of the fused forms (all g-points; each band): model and oracle summed in g-point order in the run's dtype, the
    truth in longdouble, a column taking the regime lw_ref.column_regimes gives it"""
    reg = lw_ref.regimes(dt, *shape)
    rep = lw_ref.Report(dt, label="model", quiet=True)
    for angles in ("1", "3", "opt"):
        m, o, t = (f(dt, *shape, top_at_1, angles, True) for f in (lw_ref.model, lw_ref.oracle, lw_ref.truth))
        for gpts in [np.arange(NGPT)] + ([lw_ref.band_gpoints(ib) for ib in range(NBND)] if angles == "1" else []):
            rep.check(f"sum of g-points {gpts.tolist()}, angles {angles}", as_dict(m, gpts, True), as_dict(o, gpts, True), as_dict(t, gpts),
                      lw_ref.column_regimes(reg[gpts]))
    rep.done()
    assert set(lw_ref.column_regimes(reg)) == {"seam"} and set(lw_ref.column_regimes(reg[lw_ref.band_gpoints(0)])) == {"thin_dark"}
