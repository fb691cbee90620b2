"""The longdouble truth of the rescaled LW solver (tests/lw1r_truth.py), pinned without a GPU: closed forms, the layer against mpmath at
60 digits, the conditions on the inputs that tests/test_gpu_lw1r_truth.py relies on, how far the model (tests/lw1r_ref.solve) sits from
it regime by regime, the (empty) list of unresolved cells, and a demonstration on model arithmetic alone that the GPU test's bound
rejects wrong kernels.

Norm: lw_ref.profile_error per (g-point, column) profile and quantity (flux_up, flux_dn, flux_up_jac), in eps of the dtype. Bound of the
GPU test: per regime and quantity 8 x max(E_regime, 32 eps), E_regime the model's worst error against the same truth.

The record that is asserted (RECORD, within a factor of 2 either way: the model's worst error over lw1r_truth.CASES, the entries general
(one and three angles) / fused / null, runs with and without incident flux and the three quantities, at lw1r_truth.SEED; measured on a
CPU, nothing here runs on a GPU):

    regime              fp64 model vs truth (flux_up, flux_dn, flux_up_jac)      fp32 model vs truth
    moderate            4.6 eps (4.6, 4, 1.2)                                    12 eps (12, 12, 1.2)
    thin_dark           4.3e+02 eps (1.7e+02, 4.3e+02, 17)                       11 eps (11, 11, 4.8)
    opaque              5e+02 eps (87, 5e+02, 1.1)                               33 eps (15, 33, 1.1)
    moderate_cloud      1.6e+03 eps (7.6e+02, 1.6e+03, 1.3)                      75 eps (75, 57, 1.4)
    conservative        2.2e+03 eps (2.2e+03, 1.9e+03, 1.6)                      41 eps (41, 37, 2.2)
    wide                4.8e+03 eps (4.8e+03, 4.8e+03, 2)                        1.1e+02 eps (1.1e+02, 1.1e+02, 2.7)
    thin_lit            1.5e+04 eps (31, 1.5e+04, 16)                            1.9e+02 eps (23, 1.9e+02, 18)
    near_conservative   1.1e+05 eps (1.3e+04, 1.1e+05, 5)                        6e+02 eps (1.7e+02, 6e+02, 9.2)
    just_thick          2e+06 eps (4.4e+04, 2e+06, 11)                           3.4e+02 eps (1.7e+02, 3.4e+02, 2.8)
    seam                5.9e+06 eps (1.8e+05, 5.9e+06, 14)                       4.7e+02 eps (2.8e+02, 4.7e+02, 5.8)

The fp64 column follows lw_ref's: the cancellation of fact = (1 - tr)/tl - tr just above the switch tl = eps^(1/4) (seam, just_thick:
2 eps/tl^2) and of 1 - tr below it (thin_lit). near_conservative and opaque are the fused entry's: the model combines gas and cloud in
the run's dtype and the truth in longdouble, and one rounding of ssa is eps/(1 - ssa) of st (with ssa given, the general entry's model is
at 2 eps in both). That is what the fp32
per-g-point tolerance of tests/test_gpu_lw_rescaled.py (3.8e-4, in a norm over the array's largest value) is made of. No cell is
unresolved: the largest bound, 8 x the largest entry, is 1.0e-8 of a flux in fp64 and 5.7e-4 in fp32.

What the bound catches (test_bound_rejects_wrong_models, a perturbed model in place of a kernel, general entry with one angle at every
case and with three on the two smallest shapes): exp off by 2^-40 (fp64) / 2^-18 (fp32) in (thin_lit, flux_dn) and (moderate, flux_up) -- the smallest excess over
the bound is 4.2e3 / 2.1e2 x in fp64 and 22 / 1.6 x in fp32; the series one term short in (thin_dark, flux_dn), 3.7e3 x / 1.9 x; Cn
with 0.5 in place of 0.4 in (moderate_cloud, flux_up), 5e11 x / 1e3 x. lw1r_truth's SENSITIVITY note says how the draws were shaped."""
import mpmath
import numpy as np
import pytest

import lw_ref
import lw1r_ref
import lw1r_truth as T
from lw1r_truth import CASES, IDS, SHAPES, REGIMES, QUANTITIES, NGPT, NBND, as_dict

L = np.longdouble
EPS_L = np.finfo(L).eps
EPS64 = np.finfo(np.float64).eps
RECORD = {"f64": dict(moderate=4.6, thin_dark=430.0, opaque=500.0, moderate_cloud=1600.0, conservative=2200.0, wide=4800.0, thin_lit=15000.0, near_conservative=110000.0, just_thick=2000000.0, seam=5900000.0),
          "f32": dict(moderate=12.0, thin_dark=11.0, opaque=33.0, moderate_cloud=75.0, conservative=41.0, wide=110.0, thin_lit=190.0, near_conservative=600.0, just_thick=340.0, seam=470.0)}
UNRESOLVED = set()
EXP_REL = {"f64": 2.0**-40, "f32": 2.0**-18}
REJECTED_IN = {"exp_rel": [("thin_lit", "flux_dn"), ("moderate", "flux_up")], "short_series": [("thin_dark", "flux_dn")],
               "cn_coef": [("moderate_cloud", "flux_up")]}
MIN_PROFILES = 9


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
def test_isothermal_cavity(top_at_1):
    """every source B, incident flux pi B, one angle of weight 1: the bracket of each adjustment vanishes and flux_up = flux_dn = pi B
    at every level, for any tau, ssa, g (g = 1 with ssa = 1 included: st = 0) and emissivity. This solver has no thin-layer switch that
    cuts emission, so there is no residue (tests/test_gpu_lw_2stream.py states one for the two-stream solver's)."""
    rng = np.random.default_rng(12)
    ngpt, nlay, ncol = 4, 23, 5
    shp = (ngpt, nlay, ncol)
    tau = 10.0**rng.uniform(-7, 1.5, shp)
    tau[:, [0, 9]] = 0.0
    ssa, g = rng.uniform(0, 1, shp), rng.uniform(-0.5, 0.95, shp)
    ssa[0] = 1.0
    g[0, 5] = 1.0
    ssa[1] = 0.0
    B = rng.uniform(5, 40, (ngpt, 1, ncol))
    ones = np.ones((ngpt, nlay + 1, ncol))
    up, dn, jac = T.solve_truth(np.full((1, ngpt, ncol), 1.66), np.ones(1), tau, ssa, g, (B * ones)[:, 1:], B * ones, rng.uniform(0.5, 1, (ngpt, ncol)), B[:, 0],
                                np.pi * B[:, 0], None, top_at_1)
    want = T.lw2s_truth.PI_L * B.astype(L)
    # (the incident flux pi B is given in float64: its rounding is the tolerance)
    assert max(float(np.max(np.abs(up - want) / want)), float(np.max(np.abs(dn - want) / want))) <= EPS64
    assert not jac.any()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_without_scattering_it_is_lw_ref_solve(dt):
    """ssa = 0: st = 1, Cn = 0, and truth and model are lw_ref's, one and three angles, fluxes and Jacobian"""
    shape = SHAPES[dt][0]
    I = T.inputs(dt, *shape)
    zero = np.zeros_like(I["tau"])
    for angles in ("1", "3"):
        sec, w = T.angles_of(dt, *shape, angles)
        for top_at_1 in (False, True):
            a = T.solve_truth(sec, w, I["tau"], zero, I["g"], I["lay"], I["lev"], I["emis"], I["ssrc"], I["inc"], I["sjac"], top_at_1)
            b = lw_ref.solve(sec, w, I["tau"], I["lay"], I["lev"], I["emis"], I["ssrc"], I["inc"], I["sjac"], top_at_1)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
            a = T.solve_model(sec, w, I["tau"], zero, I["g"], I["lay"], I["lev"], I["emis"], I["ssrc"], I["inc"], I["sjac"], top_at_1)
            b = lw1r_ref.solve(sec, w, I["tau"], zero, I["g"], I["lay"], I["lev"], I["emis"], I["ssrc"], I["inc"], top_at_1, I["sjac"])
            for x, y in zip(a, b):
                assert np.array_equal(x, y)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_model_is_lw1r_ref_and_the_orientations_mirror(dt):
    shape = SHAPES[dt][1]
    I = T.inputs(dt, *shape)
    flip = lambda k: np.ascontiguousarray(I[k][:, ::-1])
    for angles in ("1", "3"):
        sec, w = T.angles_of(dt, *shape, angles)
        a = T.model(dt, *shape, False, "general", angles, True)
        b = lw1r_ref.solve(sec, w, I["tau"], I["ssa"], I["g"], I["lay"], I["lev"], I["emis"], I["ssrc"], I["inc"], False, I["sjac"])
        c = T.solve_model(sec, w, flip("tau"), flip("ssa"), flip("g"), flip("lay"), flip("lev"), I["emis"], I["ssrc"], I["inc"], I["sjac"], True)
        t0 = T.truth(dt, *shape, False, "general", angles, True)
        t1 = T.solve_truth(sec, w, flip("tau"), flip("ssa"), flip("g"), flip("lay"), flip("lev"), I["emis"], I["ssrc"], I["inc"], I["sjac"], True)
        for x, y, z, u, v in zip(a, b, c, t0, t1):
            assert np.array_equal(x, y) and np.array_equal(x, z[:, ::-1]) and np.array_equal(u, v[:, ::-1])


# ---- the truth's layer against mpmath ---------------------------------------------------------------------------------------------------
def _mpf(mp, x):
    hi = np.float64(x)
    return mp.mpf(float(hi)) + mp.mpf(float(np.float64(x - L(hi))))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_truth_layer_against_the_formulas_as_written_at_60_digits(dt):
    """Every layer of the smallest shape (all regimes), one-angle secant: tr and Cn absolutely, sdn and sup over max(lay, lev) min(1, tl),
    against the formulas as written (fact = (1 - tr)/tl - tr) in mpmath at 60 digits. Bound: 1/16 eps of fp64."""
    mp = mpmath.mp.clone()
    mp.dps = 60
    mpf = mp.mpf
    F = T.np_dtype(dt)
    I = T.inputs(dt, *SHAPES[dt][0])
    tau, ssa, g, lay, lev = (I[k] for k in ("tau", "ssa", "g", "lay", "lev"))
    conv = lambda a: np.asarray(a).astype(L)
    D = I["sec1"][0][:, None, :]
    tiny = np.finfo(F).tiny
    got = T.truth_layer(conv(tau), conv(ssa), conv(g), conv(D), conv(lay), conv(lev[:, :-1]), conv(lev[:, 1:]), tiny)
    worst = dict.fromkeys(REGIMES, 0.0)
    for ig, reg in enumerate(T.GPOINT_REGIMES):
        for il in range(tau.shape[1]):
            for ic in range(tau.shape[2]):
                t, w, gg, ly, lt, lb = (mpf(float(a[ig, il, ic])) for a in (tau, ssa, g, lay, lev[:, :-1], lev[:, 1:]))
                wb = w * (1 - gg) / 2
                st = 1 - w + wb
                cn = mpf("0.4") * wb / max(st, 3 * mpf(float(tiny)))
                tl = t * mpf(float(D[ig, 0, ic])) * st
                tr = mp.exp(-tl)
                fact = (1 - tr) / tl - tr if tl > 0 else mpf(0)
                sdn = (1 - tr) * lb + 2 * fact * (ly - lb)
                sup = (1 - tr) * lt + 2 * fact * (ly - lt)
                scale = max(ly, lt, lb) * min(mpf(1), tl)
                errs = [abs(_mpf(mp, got[0][ig, il, ic]) - tr), abs(_mpf(mp, got[3][ig, il, ic]) - cn)]
                if scale > 0:
                    errs += [abs(_mpf(mp, got[1][ig, il, ic]) - sdn) / scale, abs(_mpf(mp, got[2][ig, il, ic]) - sup) / scale]
                else:
                    assert got[1][ig, il, ic] == 0 and got[2][ig, il, ic] == 0
                worst[reg] = max(worst[reg], float(max(errs)) / EPS64)
    print(f"LW1RTRUTH truth layer vs mpmath {dt}: " + ", ".join(f"{r} {w:.2g}" for r, w in worst.items()) + " eps of fp64")
    for r, w in worst.items():
        assert w <= 1. / 16., (r, w)


# ---- the conditions the GPU tests rely on -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_every_regime_is_populated_and_inside_its_interval(dt):
    F = T.np_dtype(dt)
    Tsw = L(lw_ref.tau_thres(dt))
    ranges = T.regime_ranges(dt)
    assert len(set(s[1] for s in SHAPES[dt])) == 11 and all(9 <= s[0] <= 20 for s in SHAPES[dt]) and any(s[0] % 2 for s in SHAPES[dt])
    for ncol, nlay in SHAPES[dt]:
        I = T.inputs(dt, ncol, nlay)
        reg = T.regimes(dt, ncol, nlay)
        assert I["tau"].dtype == F and reg.shape == (NGPT, ncol) and all(not v.flags.writeable for v in I.values())
        for r in REGIMES:
            assert int((reg == r).sum()) >= MIN_PROFILES, (ncol, nlay, r)
        tau, ssa, g = (I[k].astype(L) for k in ("tau", "ssa", "g"))
        assert np.array_equal(I["tau"], I["tau_g"] + I["tau_c"][I["gb"] - 1])
        st = 1 - ssa + ssa * (1 - g) / 2
        secants = np.concatenate([I["sec1"], I["sec3"]]).astype(L)
        assert secants.min() >= T.D_MIN and secants.max() <= T.D_MAX
        tl = (tau * st)[None] * secants[:, :, None, :]                                                   # every secant of the tests
        for ig, r in enumerate(T.GPOINT_REGIMES):
            lo, hi = ranges[r]
            x = tl[:, ig]
            assert x.min() >= lo * (1 - 1e-5) and x.max() <= hi * (1 + 1e-5), (ncol, nlay, ig, r, float(x.min()), float(x.max()))
            if r in ("thin_dark", "thin_lit"):
                assert x.max() < Tsw
            if r == "just_thick":
                assert x.min() > Tsw
            if r == "seam":
                assert np.all((x > Tsw).any(axis=1)) and np.all((x <= Tsw).any(axis=1))
            if r in ("conservative", "wide"):
                assert np.all(I["tau"][ig][[0, nlay // 2, nlay - 1]] == 0)
            if r in ("thin_dark", "moderate"):
                assert not I["ssa"][ig].any()
            if r in ("thin_lit", "seam", "just_thick", "moderate_cloud", "opaque"):
                assert np.all(I["ssa"][ig][I["tau"][ig] > 0] > 0) and I["ssa"][ig].max() <= 0.9 * (1 + 1e-5) and I["g"][ig].min() >= -0.3 and I["g"][ig].max() <= 0.9
            if r == "near_conservative":
                assert np.all(1 - ssa[ig] >= 0.9e-4) and np.all(1 - ssa[ig] <= 1.1e-2)
            if r == "conservative":
                assert np.all(I["ssa"][ig][I["tau"][ig] > 0] == 1) and not I["tau_g"][ig].any()
                fw = list(T.FORWARD_LAYERS)
                assert np.all(I["g"][ig][fw] == 1) and np.all(st[ig][fw] == 0) and np.all(I["tau"][ig][fw] > 0)      # Cn's max(st, 3 tiny) bites
            if r == "wide":
                cloudy = np.count_nonzero(I["tau_c"][I["gb"][ig] - 1]) / (nlay * ncol)
                assert 0.08 <= cloudy <= 0.35, cloudy
        op = T.GPOINT_REGIMES.index("opaque")                                                           # a denormal transmissivity, then an exact 0
        with np.errstate(under="ignore"):
            stF = (F(1) - I["ssa"][op] + I["ssa"][op] * (F(1) - I["g"][op]) * F(0.5))
            t1, t2 = np.exp(-(I["tau"][op, 1] * I["sec1"][0, op] * stF[1])), np.exp(-(I["tau"][op, 2] * I["sec1"][0, op] * stF[2]))
        assert np.all((t1 > 0) & (t1 < np.finfo(F).tiny)) and np.all(t2 == 0)
        for ib in T.HOT_BANDS:                                                                          # SENSITIVITY: the hot layers
            assert np.allclose(I["blay"][ib], 4.0 * (I["blev"][ib, :-1] + I["blev"][ib, 1:]), rtol=1e-6) and T.BANDS[ib][0] in ("thin_dark", "moderate")
        assert np.all(I["lev"] > 0) and np.all(I["lay"] > 0)
        assert np.all(I["emis"][:, ::3] == 1) and np.all(np.delete(I["emis"], np.s_[::3], axis=1) < 1)
        lit = [ig for ig in range(NGPT) if ig not in T.DARK_GPOINTS]
        assert np.all(I["inc"][list(T.DARK_GPOINTS)] == 0) and np.all(I["inc"][lit] > 0)
        assert all(T.GPOINT_REGIMES[ig] == "thin_dark" for ig in T.DARK_GPOINTS[:2])
        # bands: uneven, contiguous, one regime each; seam (ill-conditioned) and moderate (well-conditioned) each fill a band
        assert sorted(set(int(h - l + 1) for l, h in I["band_lims"])) == [1, 2, 3] and NBND == 10
        for ib in range(NBND):
            assert np.all(I["gb"][T.band_gpoints(ib)] == ib + 1) and len(set(T.GPOINT_REGIMES[i] for i in T.band_gpoints(ib))) == 1
    assert T.column_regimes(T.regimes(dt, 9, 80))[0] == "seam"


# ---- the model's distance from truth, the unresolved cells, the bound with a model in place of a kernel ------------------------------------
CONFIGS = [("general", "1"), ("general", "3"), ("fused", "1"), ("null", "1")]


@pytest.fixture(scope="module")
def table():
    """worst[dt][(regime, quantity)] over every case, entry, angle set and run with / without incident flux"""
    worst = {"f64": {}, "f32": {}}
    for dt, shape, top_at_1 in CASES:
        eps = np.finfo(T.np_dtype(dt)).eps
        reg = T.regimes(dt, *shape)
        for entry, angles in CONFIGS:
            for with_inc in (True, False):
                tr, m = T.truth(dt, *shape, top_at_1, entry, angles, with_inc), T.model(dt, *shape, top_at_1, entry, angles, with_inc)
                for q, a, t in zip(QUANTITIES, m, tr):
                    assert np.isfinite(a).all()
                    e = lw_ref.profile_error(a, t) / eps
                    for r in REGIMES:
                        worst[dt][(r, q)] = max(worst[dt].get((r, q), 0.0), float(e[reg == r].max()))
    return worst


def test_model_stays_inside_the_recorded_table(table):
    for dt, w in table.items():
        for q in QUANTITIES:
            print(f"LW1RTRUTH E_regime {dt} {q}: " + ", ".join(f"{r} {w[(r, q)]:.2g}" for r in REGIMES) + " eps")
    for dt, w in table.items():
        for r in REGIMES:
            e = max(w[(r, q)] for q in QUANTITIES)
            assert RECORD[dt][r] / 2 <= e <= RECORD[dt][r] * 2, (dt, r, e)
    assert list(REGIMES) == sorted(REGIMES, key=RECORD["f64"].get)                       # the order column_regimes relies on


def test_no_cell_is_unresolved(table):
    found, largest = set(), {}
    for dt, w in table.items():
        eps = float(np.finfo(T.np_dtype(dt)).eps)
        for (r, q), e in w.items():
            frac = lw_ref.bound_eps(e) * eps
            largest[dt] = max(largest.get(dt, 0.0), frac)
            if frac > T.UNRESOLVED_FRACTION:
                found.add((r, q, dt))
    print(f"LW1RTRUTH unresolved cells: {sorted(found)}; the largest bound: fp64 {largest['f64']:.2g}, fp32 {largest['f32']:.2g} of the flux")
    assert found == UNRESOLVED


def _verdict(dt, shape, top_at_1, angles, hooks=(), quiet=True):
    rep = T.report(dt, label="model", quiet=quiet)
    rep.check(f"model{dict(hooks) or ''} general {shape} top_at_1={top_at_1} angles={angles}", as_dict(T.model(dt, *shape, top_at_1, "general", angles, True, hooks)),
              as_dict(T.model(dt, *shape, top_at_1, "general", angles, True)), as_dict(T.truth(dt, *shape, top_at_1, "general", angles, True)),
              T.regimes(dt, *shape))
    return rep


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_bound_rejects_wrong_models(dt, shape, top_at_1):
    """general entry, one angle (and three on the two smallest shapes): the plain model is inside the bound in every cell; each
    perturbed one is outside in the cells REJECTED_IN names"""
    for angles in (("1", "3") if shape in SHAPES[dt][:T.BOTH_ORIENTATIONS] else ("1",)):
        _verdict(dt, shape, top_at_1, angles, quiet=angles != "1").done()
        for hooks in ((("exp_rel", EXP_REL[dt]),), (("short_series", True),), (("cn_coef", 0.5),)):
            rep = _verdict(dt, shape, top_at_1, angles, hooks)
            for cell in REJECTED_IN[hooks[0][0]]:
                k, e, b = rep.worst[(cell[1], cell[0])]
                print(f"LW1RTRUTH {dt} {shape} top_at_1={top_at_1} angles={angles} {hooks[0][0]}: {cell} model {k:.3g} eps, bound {b:.3g} eps")
                assert cell in rep.outside_cells, (hooks, angles, sorted(rep.outside_cells))


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_plain_model_passes_in_the_summed_forms(dt, shape, top_at_1):
    """the sums of the fused entry and of do_broadband (all g-points; the thin_dark, seam and moderate bands alone)"""
    rep = T.report(dt, label="model", quiet=True)
    reg = T.regimes(dt, *shape)
    for entry, angles in CONFIGS:
        m, t = T.model(dt, *shape, top_at_1, entry, angles, True), T.truth(dt, *shape, top_at_1, entry, angles, True)
        for gpts in (np.arange(NGPT), T.band_gpoints(0), T.band_gpoints(2), T.band_gpoints(4)):
            rep.check(f"sum of g-points {gpts.tolist()}", as_dict(m, gpts, True), as_dict(m, gpts, True), as_dict(t, gpts), T.column_regimes(reg[gpts]))
    rep.done()
    assert [set(T.column_regimes(reg[T.band_gpoints(ib)])) for ib in (0, 2, 4)] == [{"thin_dark"}, {"seam"}, {"moderate"}]
