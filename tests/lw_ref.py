"""Extended-precision truth for the LW no-scattering solvers (rrx_lw_solver_noscat and its Planck-lite forms _fractions, _fractions_jac,
_fractions_byband, _fractions_angles, _fractions_optimal), written from the formulas. It is the yardstick of
tests/test_gpu_lw_truth.py and is itself checked in tests/test_lw_ref.py; every other LW comparison of the suite is between two
evaluations in the same precision, in a norm (cases.rel_err) that hides everything far below the array's largest flux.

  layer      tl = tau D, trans = exp(-tl), fact(tl) = (1 - trans)/tl - trans,
             s_dn = (1 - trans) lev_below + 2 fact (lay - lev_below), s_up = (1 - trans) lev_above + 2 fact (lay - lev_above)
  transport  dn(top) = inc_flux / pi (or 0), dn' = trans dn + s_dn downwards; up(sfc) = dn(sfc) (1 - emis) + emis sfc_src,
             up' = trans up + s_up upwards; jac(sfc) = emis sfc_src_jac, jac' = trans jac
  fluxes     sum over the angles of pi w (up, dn, jac)

The builds under test (kernels and CPU oracle alike) evaluate fact by the closed form above tau_thres = eps^(1/4) of their dtype and by
the three-term series tl (1/2 - tl/3 + tl^2/8) below. The truth does NOT: solve() evaluates the mathematical function, source_factor()
-- the series sum_{k>=1} (-1)^(k+1) k t^k / (k+1)! to convergence below t = 0.5, the closed form through expm1 above -- so that the
truncation of the builds' series and the position of their switch are under test. (The switched formula run in longdouble is no truth:
just above longdouble's own switch, 1.8e-5, its cancellation leaves 7e-10 of fact.) 1 - trans is -expm1(-tl).

model() is the builds' formula in the run's dtype with numpy: a second sample, beside the oracle, of what rounding does to these
inputs. Its hooks perturb exp by a relative factor and drop the last series term; tests/test_lw_ref.py uses them to show that the bound
of tests/test_gpu_lw_truth.py rejects such kernels.

Arrays follow hip_kernels.py: C-contiguous with reversed dimensions, tau(ncol, nlay, ngpt) <-> shape (ngpt, nlay, ncol); secants
(nmus, ngpt, ncol), weights (nmus). Layers and levels are in memory order; top_at_1 says which end is the top of the atmosphere."""
import contextlib
import functools

import numpy as np

L = np.longdouble
QUANTITIES = ("flux_up", "flux_dn", "flux_up_jac")

# ---- the seeded inputs of the truth tests (tests/test_lw_ref.py, tests/test_gpu_lw_truth.py) ------------------------------------------
# (ncol, nlay): the smallest shapes that reach each tiling of lw_fused_broadband, launch_scan and the serial kernel, checked against
# csrc/rrx_solver_lw.hip. Fused fp64 forms have 16 x 4 lanes and W waves per column group, need = ceil((nlay + 1) / (4 W)) layers per
# lane out of K = 2, 4, 6, 9; the general kernel (launch_scan) has need = ceil((nlay + 1) / 16) out of K = 2, 4, 6, 9, 12, 17.
#   fp64  (11, 15)   fused W = 4, K = 2                                      scan K = 2
#         (11, 40)   fused W = 4, K = 4                                      scan K = 4
#         (19, 140)  fused W = 4, K = 9 (production)                         scan K = 9
#         (9, 200)   fused W = 8, 16 x 4 lanes, K = 9 (need 7)               scan K = 17
#         (9, 300)   fused W = 8, 8 x 8 lanes, K = 5 out of 5, 7, 9          serial kernel (need 19 > 17)
#   fp32  (12, 15)   two columns per lane, W = 4, K = 2                      scan V = 4, K = 2
#         (20, 140)  two columns per lane, W = 4, K = 9                      scan V = 4, K = 9
#         (12, 150)  four columns per lane, 8 x 8 lanes, W = 4, K = 5        scan V = 4, K = 12
#                    (the two-column form needs 10 > 9; this form takes 144 ... 159 layers)
#         (10, 200)  two columns per lane, W = 8, 16 x 4 lanes, K = 9        scan V = 2, K = 17
#         (10, 300)  two columns per lane, W = 8, 8 x 8 lanes, K = 5         serial kernel
#         (11, 15)   odd count: one column per lane, W = 4, K = 2            scan V = 1, K = 2
#         (9, 200)   odd and tall: the one-column form needs 13 > 9, the fused form declines; general route (scan V = 1, K = 17) + sums
# rrx_set_lw_variant(15) puts the one-column form first for fp32: it takes the shapes of up to 143 layers and declines the others.
SHAPES = {"f64": [(11, 15), (11, 40), (19, 140), (9, 200), (9, 300)],
          "f32": [(12, 15), (20, 140), (12, 150), (10, 200), (10, 300), (11, 15), (9, 200)]}
BOTH_ORIENTATIONS = 2          # the first two shapes of each dtype run with top_at_1 False and True, the others with False
CASES = [(dt, s, top) for dt in ("f64", "f32") for i, s in enumerate(SHAPES[dt]) for top in ((False, True) if i < BOTH_ORIENTATIONS else (False,))]
IDS = [f"{dt}-{s[0]}x{s[1]}-top{int(t)}" for dt, s, t in CASES]

# One regime per g-point, ten g-points in four uneven bands (1 + 3 + 4 + 2). REGIMES is ordered by the reference's own error against
# truth in fp64, smallest first (the table of tests/test_lw_ref.py); column_regimes() gives a g-point sum the last of its members.
REGIMES = ("opaque", "moderate", "thin_dark", "plain", "thin", "hot_layer", "just_thick", "seam")
GPOINT_REGIMES = ("thin_dark", "thin", "seam", "just_thick", "opaque", "plain", "thin", "seam", "moderate", "hot_layer")
GPOINT_BANDS = np.array([1, 2, 2, 2, 3, 3, 3, 3, 4, 4], dtype=np.int32)
BAND_LIMS = np.array([[1, 1], [2, 4], [5, 8], [9, 10]], dtype=np.int32)        # 1-based, inclusive
NGPT, NBND = len(GPOINT_REGIMES), len(BAND_LIMS)
DARK_GPOINTS = (0, 6, 7)       # no incident flux even when the run has one: thin_dark, the second thin, the second seam
# every secant of the tests lies in [D_MIN, D_MAX]: the one-angle Gauss secant D_ONE, the drawn three-angle secants, the optimal-angle
# fit. The regimes bound tau D for EVERY such D, so a profile keeps its regime whatever the entry and its angles.
D_MIN, D_MAX, D_ONE = 1.6, 1.7, 1. / 0.6096748751
W_THREE = np.array([0.0437820218, 0.3875796738, 0.5686383044])
# The seed of the first measurement; tests/test_lw_ref.py holds the oracle to the table it recorded with it, at every shape, and found
# no heavy-tailed outlier in seam or just_thick (were one to appear after a change of the inputs: take the next seed and say so here,
# as sw2s_ref.SEED does). The choice looks at the oracle and at the inputs alone, never at a kernel.
SEED = 5151


def np_dtype(dt):
    return np.float64 if dt == "f64" else np.float32


def tau_thres(dt):
    """The switch of the source factor in the builds of this dtype, as a value of that dtype"""
    F = np_dtype(dt)
    return np.sqrt(np.sqrt(F(np.finfo(F).eps)))


def regime_ranges(dt):
    """regime -> (lo, hi): the interval that tau D of every layer lies in for every secant in [D_MIN, D_MAX]. plain and hot_layer also
    hold layers of tau = 0; opaque reaches beyond the underflow of exp."""
    T = float(tau_thres(dt))
    big = 1.5e3 if dt == "f64" else 2e2
    return dict(thin_dark=(T / 10, T), thin=(T / 1000, T), seam=(T / 2, 2 * T), just_thick=(T, 10 * T), moderate=(0.3, 5.0),
                opaque=(3.0, big * D_MAX / D_MIN), plain=(0.0, 1e2 * D_MAX), hot_layer=(0.0, 1e2 * D_MAX))


# SENSITIVITY. Two draws are shaped so that the bound of tests/test_gpu_lw_truth.py, 8 x max(E_regime, 32 eps), can tell a wrong kernel
# from a rounding-level one in fp32 too; both stay inside the regime's interval and neither looks at a kernel.
#   thin_dark  flux_dn is sum 2 fact lay, and a series without its last term t^3/8 is off by <t^3> / (4 <t>) of it. Drawn uniformly from
#              [T/10, T) that is 0.13 T^2 = 3.6e2 eps in fp32, 1.4 x the floor of the bound; drawn as T (1 - 0.9 u^3) it is 0.19 T^2.
#   moderate   a relative error d of exp moves omt by -d trans and fact by -d trans (1/t + 1): 26 d of fact at t = 0.3, 2.8 d at 1, less
#              than d from 2 on. With level and layer sources of the same size the terms of the layers differ in sign and 2 ... 6 d of
#              the flux remain, below the floor of the bound for d = 2^-18 = 32 eps in fp32; and one layer of t >= 2 replaces what came
#              through it by its own, insensitive source. So moderate shares the band of hot_layer (the term 2 fact lay dominates the
#              source, every layer's error has the same sign) and is drawn log-uniformly from [0.3, cap] with the cap cycling through
#              MODERATE_CAPS over the columns: a quarter of the profiles has every layer below 0.6 (about 20 d of the flux), a quarter
#              spans the whole interval.
MODERATE_CAPS = (0.6, 1.2, 2.5, 5.0)


def _draw_tau(rng, regime, dt, nlay, ncol):
    lo, hi = regime_ranges(dt)[regime]
    shp = (nlay, ncol)
    if regime in ("plain", "hot_layer"):                       # cases.tall_inputs' optical depths, three layers of tau = 0: both ends
        tau = 10.0**rng.uniform(-6, 2, shp)                    # (one of them is the top in either orientation) and the middle
        tau[[0, nlay // 2, nlay - 1]] = 0.0
        return tau
    a, b = lo / D_MIN * (1 + 1e-6), hi / D_MAX * (1 - 1e-6)    # tau D in [lo, hi] for every D, the rounding to fp32 included
    if regime in ("thin", "opaque"):                           # three decades: log-uniform
        tau = np.exp(rng.uniform(np.log(a), np.log(b), shp))
    elif regime == "moderate":                                 # log-uniform up to a cap that cycles over the columns, see SENSITIVITY
        cap = np.array(MODERATE_CAPS)[np.arange(ncol) % len(MODERATE_CAPS)] / D_MAX * (1 - 1e-6)
        tau = np.exp(rng.uniform(np.log(a), np.log(cap)[None, :], shp))
    elif regime == "thin_dark":                                # towards the switch, see SENSITIVITY
        tau = b - (b - a) * rng.uniform(0., 1., shp)**3
    else:
        tau = rng.uniform(a, b, shp)
    if regime == "opaque":                                     # with the one-angle secant: a denormal trans, then an exact 0
        tau[1] = (725.0 if dt == "f64" else 95.0) / D_ONE
        tau[2] = (1.5e3 if dt == "f64" else 2e2) / D_ONE
    return tau


@functools.lru_cache(maxsize=None)
def inputs(dt, ncol, nlay):
    """The seeded inputs of one shape in the precision of the run, shared by the tests and read-only:
         gb, band_lims      GPOINT_BANDS, BAND_LIMS
         tau                (ngpt, nlay, ncol), g-point ig in the regime GPOINT_REGIMES[ig] (regime_ranges)
         pfrac, blay, blev  Planck-lite sources; band 1 (thin_dark) has B_lev = 0, band 4 (moderate, hot_layer) B_lay = 8 x the mean
                            of the layer's two B_lev
         lay, lev           the sources formed from them in the run's dtype with numpy (planck_sources), for the entries that take sources
         emis               U(0.8, 1), exactly 1 in every third column; ssrc, sjac as tests/test_gpu_lw_angles.py draws them
         inc                U(0, 5), zero in DARK_GPOINTS
         sec1, w1           the one-angle Gauss secant and weight; sec3, w3: three angles with secants drawn per g-point and column
                            from [D_MIN, D_MAX] and the Gauss weights
         fit                (2, nbnd) optimal-angle fit with D = fit0 exp(-S) + fit1 in [D_MIN, D_MAX]"""
    F = np_dtype(dt)
    rng = np.random.default_rng(SEED)
    shp = (NGPT, nlay, ncol)
    tau = np.stack([_draw_tau(rng, r, dt, nlay, ncol) for r in GPOINT_REGIMES])
    blev = rng.uniform(5., 40., (NBND, nlay + 1, ncol))
    blay = rng.uniform(5., 40., (NBND, nlay, ncol))
    blev[0] = 0.0
    blay[3] = 8.0 * 0.5 * (blev[3, :-1] + blev[3, 1:])
    emis = rng.uniform(0.8, 1.0, (NGPT, ncol))
    emis[:, ::3] = 1.0
    inc = rng.uniform(0., 5., (NGPT, ncol))
    inc[list(DARK_GPOINTS)] = 0.0
    d = dict(gb=GPOINT_BANDS, band_lims=BAND_LIMS, tau=tau, pfrac=rng.uniform(0.05, 1.0, shp), blay=blay, blev=blev, emis=emis,
             ssrc=rng.uniform(5., 40., (NGPT, ncol)), sjac=rng.uniform(0.1, 0.6, (NGPT, ncol)), inc=inc,
             sec1=np.full((1, NGPT, ncol), D_ONE), w1=np.ones(1), sec3=rng.uniform(D_MIN + 0.005, D_MAX - 0.005, (3, NGPT, ncol)), w3=W_THREE,
             fit=np.stack([rng.uniform(-0.03, 0.03, NBND), rng.uniform(D_MIN + 0.035, D_MAX - 0.035, NBND)]))
    d = {k: (np.ascontiguousarray(v.astype(F)) if v.dtype.kind == "f" else v) for k, v in d.items()}
    d["lay"], d["lev"] = planck_sources(d["pfrac"], d["blay"], d["blev"], d["gb"])
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def regimes(dt, ncol, nlay):
    """The regime of each (g-point, column) profile of inputs(dt, ncol, nlay), (ngpt, ncol) strings"""
    out = np.ascontiguousarray(np.broadcast_to(np.array(GPOINT_REGIMES, dtype="U12")[:, None], (NGPT, ncol)))
    out.setflags(write=False)
    return out


def column_regimes(reg, regimes=REGIMES):
    """The regime of a column's g-point SUM, (ncol,): among the profiles that enter it, the one where the reference is farthest from
    truth (the last in `regimes`, lw_ref's own REGIMES unless a follow-up module passes its tuple)"""
    rank = np.vectorize(regimes.index)(reg)
    return np.array(regimes, dtype="U20")[rank.max(axis=0)]


# ---- Planck-lite sources and optimal-angle secants -------------------------------------------------------------------------------------
def planck_sources(pfrac, blay, blev, gpoint_bands, dtype=None):
    """(lay_source, lev_source) as rrx_planck_sources_from_fractions forms them: lay = pfrac B_lay; lev = sqrt(pfrac pfrac') B_lev at the
    interior levels, pfrac B_lev at the two ends. In `dtype` (default: the arrays' own; np.longdouble for the truth)."""
    dtype = np.dtype(pfrac.dtype if dtype is None else dtype)
    p, bl, bv = (np.asarray(a).astype(dtype) for a in (pfrac, blay, blev))
    ib = np.asarray(gpoint_bands) - 1
    ngpt, nlay, ncol = p.shape
    b = bv[ib]
    lev = np.empty((ngpt, nlay + 1, ncol), dtype=dtype)
    lev[:, 0] = p[:, 0] * b[:, 0]
    lev[:, nlay] = p[:, nlay - 1] * b[:, nlay]
    lev[:, 1:nlay] = np.sqrt(p[:, 1:] * p[:, :-1]) * b[:, 1:nlay]
    return p * bl[ib], lev


def optimal_secants(tau, fit, gpoint_bands):
    """D = fit0 exp(-sum of tau over the layers) + fit1 of the g-point's band, formed in longdouble from the inputs as they are and
    rounded to their dtype: (1, ngpt, ncol), the secants that truth, oracle, model and kernel all solve with"""
    ib = np.asarray(gpoint_bands) - 1
    S = np.asarray(tau).astype(L).sum(axis=1)
    f = np.asarray(fit).astype(L)
    return np.ascontiguousarray((f[0][ib][:, None] * np.exp(-S) + f[1][ib][:, None]).astype(tau.dtype)[None])


# ---- the solve ---------------------------------------------------------------------------------------------------------------------------
def source_factor(t):
    """fact(t) = (1 - exp(-t))/t - exp(-t) for t >= 0 in longdouble: the series to convergence below 0.5 (alternating, terms falling
    by more than t/2 each: no cancellation), the closed form above (at 0.5 it loses two bits to its subtraction)"""
    t = np.asarray(t, dtype=L)
    ts = np.where(t < L(0.5), t, L(0))
    term = ts / L(2)                                           # k = 1: t / 2!
    s = term.copy()
    for k in range(2, 40):                                     # term_k = -term_(k-1) t k / ((k - 1)(k + 1))
        term = -term * ts * L(k) / (L(k - 1) * L(k + 1))
        s += term
    tb = np.where(t < L(0.5), L(1), t)
    closed = -np.expm1(-tb) / tb - np.exp(-tb)
    return np.where(t < L(0.5), s, closed)


def _model_layer(tl, thres, exp_rel, short_series):
    """trans, 1 - trans and fact as the builds evaluate them, in tl's dtype"""
    F = tl.dtype.type
    tr = np.exp(-tl)
    if exp_rel:
        tr = tr * F(1 + exp_rel)
    omt = F(1) - tr
    with np.errstate(divide="ignore", invalid="ignore"):
        thick = omt / tl - tr
    series = tl * (F(.5) + tl * F(-1. / 3.)) if short_series else tl * (F(.5) + tl * (F(-1. / 3.) + tl * F(1. / 8.)))
    return tr, omt, np.where(tl > thres, thick, series)


def _solve(dtype, secants, weights, tau, lay_source, lev_source, sfc_emis, sfc_src, inc_flux, sfc_src_jac, top_at_1, layer):
    dtype = np.dtype(dtype)
    F = dtype.type
    conv = lambda a: np.asarray(a).astype(dtype)
    secants, weights, tau, lay, lev = conv(secants), conv(weights), conv(tau), conv(lay_source), conv(lev_source)
    emis, ssrc = conv(sfc_emis), conv(sfc_src)
    ngpt, nlay, ncol = tau.shape
    nmus = weights.shape[0]
    if not 1 <= nmus <= 4 or secants.shape != (nmus, ngpt, ncol):
        raise ValueError(f"secants {secants.shape} / weights {weights.shape}: need (nmus, ngpt, ncol) = (1..4, {ngpt}, {ncol}) and (nmus,)")
    if not top_at_1:
        tau, lay, lev = tau[:, ::-1], lay[:, ::-1], lev[:, ::-1]
    pi = F(np.pi) if dtype != np.dtype(L) else L(np.pi) + L(1.2246467991473532e-16)          # (pi to longdouble: double + its tail)
    shape = (ngpt, nlay + 1, ncol)
    out = [np.zeros(shape, dtype=dtype) for _ in range(3)]
    for imu in range(nmus):
        tr, omt, fact = layer(tau * secants[imu][:, None, :])
        sdn = omt * lev[:, 1:] + F(2) * fact * (lay - lev[:, 1:])
        sup = omt * lev[:, :-1] + F(2) * fact * (lay - lev[:, :-1])
        dn = np.empty(shape, dtype=dtype); up = np.empty(shape, dtype=dtype); jac = np.empty(shape, dtype=dtype)
        dn[:, 0] = F(0) if inc_flux is None else conv(inc_flux) / pi
        for i in range(nlay):
            dn[:, i + 1] = tr[:, i] * dn[:, i] + sdn[:, i]
        up[:, nlay] = dn[:, nlay] * (F(1) - emis) + emis * ssrc
        jac[:, nlay] = emis * (conv(sfc_src_jac) if sfc_src_jac is not None else F(0))
        for i in range(nlay - 1, -1, -1):
            up[:, i] = tr[:, i] * up[:, i + 1] + sup[:, i]
            jac[:, i] = tr[:, i] * jac[:, i + 1]
        scale = pi * weights[imu]
        for acc, a in zip(out, (up, dn, jac)):
            acc += scale * a
    if not top_at_1:
        out = [a[:, ::-1] for a in out]
    return tuple(np.ascontiguousarray(a) for a in out)


def solve(secants, weights, tau, lay_source, lev_source, sfc_emis, sfc_src, inc_flux=None, sfc_src_jac=None, top_at_1=False):
    """The truth: per-g-point flux_up, flux_dn, flux_up_jac, (ngpt, nlay+1, ncol) each in memory order, in np.longdouble from the inputs
    as they are (widening them is exact), with the mathematical source factor. sfc_src_jac None: a zero Jacobian."""
    def layer(tl):
        return np.exp(-tl), -np.expm1(-tl), source_factor(tl)
    return _solve(L, secants, weights, tau, lay_source, lev_source, sfc_emis, sfc_src, inc_flux, sfc_src_jac, top_at_1, layer)


def solve_model(secants, weights, tau, lay_source, lev_source, sfc_emis, sfc_src, inc_flux=None, sfc_src_jac=None, top_at_1=False,
                exp_rel=0.0, short_series=False):
    """The builds' formulas (switch at eps^(1/4), three-term series, 1 - trans by subtraction) in tau's dtype with numpy. exp_rel: every
    exp is multiplied by 1 + exp_rel; short_series: the series loses its last term."""
    thres = np.sqrt(np.sqrt(np.finfo(tau.dtype).eps))
    return _solve(tau.dtype, secants, weights, tau, lay_source, lev_source, sfc_emis, sfc_src, inc_flux, sfc_src_jac, top_at_1,
                  lambda tl: _model_layer(tl, thres, exp_rel, short_series))


# ---- the cases of the tests: angles is "1" (the one-angle Gauss secant), "3" (three drawn secants) or "opt" (optimal-angle secants) ------
ANGLES = ("1", "3", "opt")


def angles_of(dt, ncol, nlay, angles):
    """(secants (nmus, ngpt, ncol), weights (nmus)) in the run's dtype"""
    I = inputs(dt, ncol, nlay)
    if angles == "opt":
        return optimal_secants(I["tau"], I["fit"], I["gb"]), I["w1"]
    return {"1": (I["sec1"], I["w1"]), "3": (I["sec3"], I["w3"])}[angles]


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def truth(dt, ncol, nlay, top_at_1, angles="1", with_inc=True, from_fractions=True):
    """Per-g-point longdouble (flux_up, flux_dn, flux_up_jac) of a case, computed once and read-only. from_fractions: the sources are
    formed in longdouble from pfrac, B_lay, B_lev (the Planck-lite entries' inputs); otherwise they are I["lay"], I["lev"] as given (the
    inputs of rrx_lw_solver_noscat)."""
    I = inputs(dt, ncol, nlay)
    sec, w = angles_of(dt, ncol, nlay, angles)
    lay, lev = planck_sources(I["pfrac"], I["blay"], I["blev"], I["gb"], L) if from_fractions else (I["lay"], I["lev"])
    return _frozen(solve(sec, w, I["tau"], lay, lev, I["emis"], I["ssrc"], I["inc"] if with_inc else None, I["sjac"], top_at_1))


@functools.lru_cache(maxsize=None)
def model(dt, ncol, nlay, top_at_1, angles="1", with_inc=True, exp_rel=0.0, short_series=False):
    """solve_model on the case, sources formed in the run's dtype"""
    I = inputs(dt, ncol, nlay)
    sec, w = angles_of(dt, ncol, nlay, angles)
    return _frozen(solve_model(sec, w, I["tau"], I["lay"], I["lev"], I["emis"], I["ssrc"], I["inc"] if with_inc else None, I["sjac"],
                               top_at_1, exp_rel, short_series))


@functools.lru_cache(maxsize=None)
def oracle(dt, ncol, nlay, top_at_1, angles="1", with_inc=True):
    """The CPU oracle's per-g-point (flux_up, flux_dn, flux_up_jac) on the case, sources formed in the run's dtype; computed once"""
    import oracle_py
    orc = oracle_py.CpuKernels("oracle", np_dtype(dt))
    I = inputs(dt, ncol, nlay)
    sec, w = angles_of(dt, ncol, nlay, angles)
    r = orc.lw_solver_noscat(bool(top_at_1), sec, w, I["tau"], I["lay"], I["lev"], I["emis"], I["ssrc"],
                             inc_flux=I["inc"] if with_inc else None, do_jacobians=True, sfc_src_jac=I["sjac"])
    return _frozen(tuple(np.ascontiguousarray(orc.to_numpy(r[k])) for k in QUANTITIES))


# ---- norm and bound ------------------------------------------------------------------------------------------------------------------------
def ordered_sum(a, gpts=None):
    """g-point sum in g-point order in the array's dtype (rrx_sum_broadband's and rrx_sum_byband's order)"""
    a = a if gpts is None else a[gpts]
    out = np.zeros(a.shape[1:], dtype=a.dtype)
    for ig in range(a.shape[0]):
        out = out + a[ig]
    return out


def profile_error(got, truth_q):
    """One number per profile for ONE quantity: the largest |got - truth| over the levels, divided by the profile's largest |truth| of that
    quantity. (ngpt, nlev, ncol) arrays give (ngpt, ncol). A summed `got` (nlev, ncol) gives (ncol,): a truth that still has its g-point
    axis is summed over it in longdouble first. A plain ratio; divide by the dtype's eps for units of eps."""
    got = np.asarray(got).astype(L)
    truth_q = np.asarray(truth_q).astype(L)
    if truth_q.ndim == got.ndim + 1:
        truth_q = truth_q.sum(axis=0)
    if truth_q.shape != got.shape:
        raise ValueError((got.shape, truth_q.shape))
    err = np.max(np.abs(got - truth_q), axis=-2)
    scale = np.max(np.abs(truth_q), axis=-2)
    return (err / np.maximum(scale, np.finfo(L).tiny)).astype(np.float64)


# The bound of tests/test_gpu_lw_truth.py: per regime and quantity, kernel <= MARGIN x max(E_regime, FLOOR_EPS eps), E_regime being the
# oracle's worst error in that regime. Margin and floor are those of tests/test_gpu_sw_truth.py, for its reasons: exp_neg is documented
# at <= 1.3 ulp against libm's 1, fast_rcp replaces the division, the scans re-associate the recurrences; the floor keeps a lucky
# small sample of the reference from setting a meaningless bound.
MARGIN, FLOOR_EPS = 8.0, 32.0


def bound_eps(oracle_eps):
    return MARGIN * max(float(oracle_eps), FLOOR_EPS)


class Report:
    """Prints every figure of a test, then asserts them all. `got` is a kernel's output -- or, in tests/test_lw_ref.py, a model's.
    The follow-up modules (tests/lw2s_truth.py, tests/lw1r_truth.py) pass their own regime tuple, quantity tuple, print prefix and the
    name of what stands behind E_regime; with fraction=True a line also gives the bound as a plain fraction of the profile's largest
    flux. The defaults are this module's, unchanged."""
    def __init__(self, dt, label="kernel", quiet=False, regimes=REGIMES, quantities=QUANTITIES, prefix="LWTRUTH", ref_name="oracle",
                 fraction=False):
        self.dt, self.eps, self.label, self.quiet = dt, float(np.finfo(np_dtype(dt)).eps), label, quiet
        self.regimes, self.quantities, self.prefix, self.ref_name, self.fraction = regimes, quantities, prefix, ref_name, fraction
        self.failures, self.outside, self.outside_cells, self.worst = [], set(), set(), {}

    def check(self, what, got, orc, truth_, reg):
        """got, orc: dicts quantity -> per-g-point (ngpt, nlev, ncol) or summed (nlev, ncol) arrays of the run's dtype; truth_: the same
        keys (or more), per g-point longdouble; reg: the regime of each profile of got"""
        for q in self.quantities:
            if q not in got:
                continue
            k = profile_error(got[q], truth_[q]) / self.eps
            e = profile_error(orc[q], truth_[q]) / self.eps
            assert k.shape == reg.shape == e.shape, (k.shape, e.shape, reg.shape)
            if not np.isfinite(np.asarray(got[q], dtype=np.float64)).all():
                self.failures.append(f"{what} {q}: not finite")
            for r in self.regimes:
                m = reg == r
                if not m.any():
                    continue
                kc, ec = float(k[m].max()), float(e[m].max())
                bound = bound_eps(ec)
                if not self.quiet:
                    print(f"{self.prefix} {what} {q} {self.dt} {r} n={int(m.sum())}: {self.label} {kc:.4g} eps, {self.ref_name} {ec:.4g} eps, "
                          f"ratio {kc / max(ec, 1e-300):.3g}, bound {bound:.4g} eps" + (f" = {bound * self.eps:.3g} of the largest flux" if self.fraction else ""))
                key = (q, r)
                if kc > self.worst.get(key, (-1.0,))[0]:
                    self.worst[key] = (kc, ec, bound)
                if not kc <= bound:
                    self.outside.add(r)
                    self.outside_cells.add((r, q))
                    self.failures.append(f"{what} {q} {r}: {self.label} {kc:.4g} eps > {bound:.4g} eps ({self.ref_name} {ec:.4g} eps)")

    def done(self):
        assert not self.failures, "\n".join(self.failures)


@contextlib.contextmanager
def one_range(be):
    """the fused forms of a backend without the g-point split"""
    be.set_broadband_min_groups(1)
    be.set_broadband_gsplit(1)
    try:
        yield
    finally:
        be.set_broadband_min_groups(512)
        be.set_broadband_gsplit(0)


def splits(be):
    """the two ways the GPU truth tests run every fused form: (label, context manager)"""
    return (("automatic split", contextlib.nullcontext()), ("one range", one_range(be)))


def as_dict(fluxes, gpts=None, summed=False):
    """(flux_up, flux_dn, flux_up_jac) -> dict by quantity; gpts: only these g-points; summed: their ordered_sum"""
    out = {}
    for q, a in zip(QUANTITIES, fluxes):
        a = a if gpts is None else a[gpts]
        out[q] = ordered_sum(a) if summed else a
    return out


def band_gpoints(ib):
    """0-based g-point indices of band ib (0-based)"""
    lo, hi = BAND_LIMS[ib]
    return np.arange(lo - 1, hi)
