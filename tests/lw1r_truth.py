"""Extended-precision truth and run-precision model for the rescaled LW no-scattering solver (rrx_lw_solver_noscat_rescaled and
rrx_lw_solver_noscat_fractions_rescaled), written from the formulas of DESIGN 4.11 and of the header of
csrc/rrx_solver_lw1r.hip. A follow-up to tests/lw_ref.py: its longdouble layer (source_factor, expm1), norm, bound, Report, ordered_sum,
column_regimes, planck_sources and the draws of its regimes are used as they are. It is the yardstick of tests/test_gpu_lw1r_truth.py and
is itself checked in tests/test_lw1r_truth.py.

  layer      wb = ssa (1 - g)/2, st = 1 - ssa + wb, Cn = 0.4 wb / max(st, 3 tiny), tl = tau D st, tr = exp(-tl), An = 1 - tr^2,
             fact(tl) = (1 - tr)/tl - tr, sdn = (1 - tr) lev_below + 2 fact (lay - lev_below), sup likewise with lev_above
  pass 1     dn(top) = inc_flux / pi (or 0), dn[i+1] = tr dn[i] + sdn;   surface: up[nlay] = dn[nlay] (1 - emis) + emis sfc_src
  pass 2     up[i] = tr up[i+1] + sup + Cn (An dn[i] - tr sdn - sup)                       (pass 1's dn)
  pass 3     dn[i+1] = tr dn[i] + sdn + Cn (An up[i+1] - tr sup - sdn)                     (pass 2's up)
  Jacobian   J[nlay] = emis sfc_src_jac, J[i] = tr J[i+1];   fluxes: the sum over the 1 ... 4 angles of pi w (up, dn, J)

THE TRUTH (solve_truth, np.longdouble, inputs widened exactly) evaluates the mathematical function: fact by lw_ref.source_factor (not the
builds' switch at eps^(1/4) and three-term series), 1 - tr = -expm1(-tl), An = -expm1(-2 tl); `tiny` is the run's dtype's. For the fused
entry gas and band cloud are combined and the sources formed in longdouble (lw2s_truth.combine_truth, lw_ref.planck_sources).
THE MODEL (solve_model) is tests/lw1r_ref.solve as it stands when no hook is set (asserted bit for bit in tests/test_lw1r_truth.py); hooks:
exp_rel (every exp times 1 + exp_rel), short_series (the series loses its last term), cn_coef (another value for the 0.4).

Arrays follow hip_kernels.py: tau(ncol, nlay, ngpt) <-> shape (ngpt, nlay, ncol); secants (nmus, ngpt, ncol), weights (nmus); band clouds
(nbnd, nlay, ncol). Layers and levels are in memory order; top_at_1 says which end is the top of the atmosphere."""
import functools

import numpy as np

import lw_ref
import lw1r_ref
import lw2s_ref
import lw2s_truth
from lw_ref import L, np_dtype, planck_sources, ordered_sum, D_MIN, D_MAX, D_ONE, W_THREE, QUANTITIES, as_dict  # noqa: F401

PREFIX = "LW1RTRUTH"
CN_COEF = 0.4

# ---- shapes ------------------------------------------------------------------------------------------------------------------------------
# (ncol, nlay): the smallest layer counts that reach each tiling of lw1r_fused / launch_lw1r (csrc/rrx_solver_lw1r.hip), checked against
# their with_k lists: need = ceil((nlay + 1) / ((64 / CLT) W)) layers per lane, the first K >= need of the tiling's list.
#   nlay   fp64 (8 x 8 lanes)                              fp32
#   15     W = 2 (NW = 4), need 1, K = 2                    16 x 4 lanes, W = 4 (NW = 4): need 1, K = 2
#   40     need 3, K = 4                                    need 3, K = 4
#   80     need 6, K = 6                                    need 6, K = 6
#   140    need 9, K = 9 (to 143 layers)                    need 9, K = 9 (to 143)
#   150    W = 4, need 5, K = 5 (144 ... 287)               16 x 4 lanes, W = 8: need 5, K = 5 (144 ... 287)
#   200    W = 4, need 7, K = 7                             need 7, K = 7
#   280    W = 4, need 9, K = 9                             need 9, K = 9
#   300    W = 8, need 5, K = 5 (288 ... 575)               8 x 8 lanes, W = 8: K = 5
#   400    need 7, K = 7                                    K = 7
#   500    need 8, K = 9                                    K = 9
#   600    need 10: no tiling; the materialised route ([tau | ssa | g | lay_source | lev_source] and the general solve)
# Columns: 9 ... 20, odd counts among them; a column group is 8 (fp64; fp32 from 288 layers) or 16 columns: every count but 16 leaves one
# part-filled.
SHAPES = {dt: [(11, 15), (12, 40), (9, 80), (19, 140), (13, 150), (10, 200), (9, 280), (9, 300), (20, 400), (9, 500), (9, 600)] for dt in ("f64", "f32")}
BOTH_ORIENTATIONS = 2
CASES = [(dt, s, top) for dt in ("f64", "f32") for i, s in enumerate(SHAPES[dt]) for top in ((False, True) if i < BOTH_ORIENTATIONS else (False,))]
IDS = [f"{dt}-{s[0]}x{s[1]}-top{int(t)}" for dt, s, t in CASES]

# ---- regimes -----------------------------------------------------------------------------------------------------------------------------
# One regime per g-point, the same in every column, one regime per band; the layout of lw2s_truth.BANDS with seam and just_thick where
# the two-stream solver's switch band stands (this solver's only switch is the source factor's, at eps^(1/4)). A band with a cloud holds one
# g-point, so that tau D st of the combination can be drawn: 15 g-points in ten uneven bands. A regime is an interval of tl = tau D st that
# holds for every secant in [D_MIN, D_MAX] (lw_ref.regime_ranges of the lw_ref regime in BASE) and a scattering class. REGIMES is ordered by
# the model's own error against truth in fp64, smallest first (the table of tests/test_lw1r_truth.py).
BANDS = (("thin_dark", 2), ("thin_lit", 1), ("seam", 1), ("just_thick", 1), ("moderate", 3), ("moderate_cloud", 1), ("near_conservative", 1),
         ("conservative", 1), ("opaque", 1), ("wide", 3))
BASE = dict(thin_dark="thin_dark", thin_lit="thin", seam="seam", just_thick="just_thick", moderate="moderate", moderate_cloud="moderate",
            near_conservative="moderate", conservative="plain", opaque="opaque", wide="plain")
REGIMES = ("moderate", "thin_dark", "opaque", "moderate_cloud", "conservative", "wide", "thin_lit", "near_conservative", "just_thick", "seam")
GPOINT_REGIMES = tuple(r for r, n in BANDS for _ in range(n))
NGPT, NBND = len(GPOINT_REGIMES), len(BANDS)
GPOINT_BANDS = np.array([ib + 1 for ib, (r, n) in enumerate(BANDS) for _ in range(n)], dtype=np.int32)
BAND_LIMS = np.array([[int(np.flatnonzero(GPOINT_BANDS == ib + 1)[0]) + 1, int(np.flatnonzero(GPOINT_BANDS == ib + 1)[-1]) + 1] for ib in range(NBND)],
                     dtype=np.int32)
DARK_GPOINTS = (0, 1, 6, 14)      # no incident flux even when the run has one: both thin_dark, the second moderate, the last wide
HOT_BANDS = (0, 4)                # B_lay = 8 x the mean of the layer's two B_lev: thin_dark and moderate (SENSITIVITY)
FORWARD_LAYERS = (3, 5)           # conservative: g = 1 there, st = 0 and Cn's max(st, 3 tiny) bites
# The seed of the first measurement, by lw_ref.SEED's rule (tests/test_lw1r_truth.py holds the model to the table recorded with it; no
# heavy-tailed outlier appeared in seam or just_thick). The choice looks at the model and the inputs alone, never at a kernel.
SEED = 7171


def regime_ranges(dt):
    """regime -> (lo, hi): the interval that tl = tau D st of every layer lies in for every secant in [D_MIN, D_MAX]: lw_ref.regime_ranges of
    the BASE regime (thin_lit: (T/1000, T) with T = eps^(1/4), i.e. 1.2e-7 ... 1.2e-4 in fp64; thin_dark (T/10, T); seam (T/2, 2T);
    just_thick (T, 10T); the moderate ones (0.3, 5); opaque from 3 to beyond the underflow of exp; conservative and wide hold layers of
    tau = 0), wide with room for its clouds of tau <= 10"""
    base = lw_ref.regime_ranges(dt)
    out = {r: base[BASE[r]] for r in REGIMES}
    out["wide"] = (0.0, 1.1e2 * D_MAX)
    return out


# SENSITIVITY (how the draws make the bound 8 x max(E_regime, 32 eps) reject the perturbed models in fp32 too; inputs and models alone):
#   exp off by d    lw_ref's note: moderate has hot layers (the term 2 fact lay dominates, every layer's error has one sign) and is drawn
#                   with lw_ref's caps on tl, a quarter of the profiles below 0.6 throughout: about 20 d of the flux.
#   short series    thin_dark keeps lw_ref's draw towards the switch, tl = T (1 - 0.9 u^3), and has hot layers on lit levels: the missing
#                   t^3/8 is t^2/4 of fact, and 2 fact (lay - lev) is 7/8 of a source of about t (lev + 7 lev): 0.19 T^2 = 4e2 ... 5e2 eps.
#   Cn with 0.5     nothing to shape: a quarter of the adjustment, which is of the order of the flux in moderate_cloud.
def _draw(rng, regime, n, dt, nlay, ncol):
    """(tau_g (n, nlay, ncol), tau_c, ssa_c, g_c (nlay, ncol)) of one band in float64; X below is the target tau st"""
    shp = (nlay, ncol)
    X = np.stack([lw_ref._draw_tau(rng, BASE[regime], dt, nlay, ncol) for _ in range(n)])
    ssa_c, g_c = rng.uniform(0.0, 0.9, shp), rng.uniform(-0.3, 0.9, shp)
    if regime in ("thin_dark", "moderate"):                                    # no cloud: st = 1
        return X, np.zeros(shp), ssa_c, g_c
    if regime == "wide":                                                       # clouds in a fifth of the cells, none where tau = 0
        tau_c = np.where((rng.uniform(0, 1, shp) < 0.2) & (X[0] > 0), 10.0**rng.uniform(-2, 1, shp), 0.0)
        return X, tau_c, ssa_c, g_c
    ssa = ssa_c                                                                # the combination's ssa; the cloud's own is at least that
    if regime == "near_conservative":
        ssa = 1.0 - np.exp(rng.uniform(np.log(1.1e-4), np.log(0.9e-2), shp))
    if regime == "conservative":
        ssa = np.ones(shp)
        g_c[list(FORWARD_LAYERS)] = 1.0
    st = 1.0 - ssa + ssa * (1.0 - g_c) * 0.5
    tau = X[0] / np.where(st > 0, st, 1.0)
    own = np.ones(shp) if regime in ("near_conservative", "conservative") else ssa + (1.0 - ssa) * rng.uniform(0, 1, shp)
    tau_c = tau * ssa / np.where(own > 0, own, 1.0)
    tau_g = np.zeros(shp) if regime == "conservative" else tau - tau_c
    return tau_g[None], tau_c, own, g_c


@functools.lru_cache(maxsize=None)
def inputs(dt, ncol, nlay):
    """The seeded inputs of one shape in the precision of the run, shared and read-only: gb, band_lims; tau_g (ngpt, nlay, ncol) and the band
    cloud tau_c, ssa_c, g_c (nbnd, nlay, ncol); pfrac, blay, blev (HOT_BANDS: B_lay = 8 x the mean of the two B_lev); tau, ssa, g, lay, lev:
    the general entry's inputs, combined and formed in the run's dtype with numpy; emis U(0.8, 1), 1 in every third column; ssrc, sjac;
    inc U(0.1, 5), zero in DARK_GPOINTS; sec1, w1, sec3, w3 as lw_ref.inputs has them"""
    F = np_dtype(dt)
    rng = np.random.default_rng(SEED)
    drawn = [_draw(rng, r, n, dt, nlay, ncol) for r, n in BANDS]
    tau_g = np.concatenate([d[0] for d in drawn])
    cld = tuple(np.stack([d[i] for d in drawn]) for i in (1, 2, 3))
    shp = (NGPT, nlay, ncol)
    blev = rng.uniform(5., 40., (NBND, nlay + 1, ncol))
    blay = rng.uniform(5., 40., (NBND, nlay, ncol))
    for ib in HOT_BANDS:
        blay[ib] = 8.0 * 0.5 * (blev[ib, :-1] + blev[ib, 1:])
    emis = rng.uniform(0.8, 1.0, (NGPT, ncol))
    emis[:, ::3] = 1.0
    inc = rng.uniform(0.1, 5., (NGPT, ncol))
    inc[list(DARK_GPOINTS)] = 0.0
    d = dict(gb=GPOINT_BANDS, band_lims=BAND_LIMS, tau_g=tau_g, tau_c=cld[0], ssa_c=cld[1], g_c=cld[2], pfrac=rng.uniform(0.05, 1.0, shp), blay=blay,
             blev=blev, emis=emis, ssrc=rng.uniform(5., 40., (NGPT, ncol)), sjac=rng.uniform(0.1, 0.6, (NGPT, ncol)), inc=inc,
             sec1=np.full((1, NGPT, ncol), D_ONE), w1=np.ones(1), sec3=rng.uniform(D_MIN + 0.005, D_MAX - 0.005, (3, NGPT, ncol)), w3=W_THREE)
    d = {k: (np.ascontiguousarray(v.astype(F)) if v.dtype.kind == "f" else v) for k, v in d.items()}
    d["tau"], d["ssa"], d["g"] = (np.ascontiguousarray(a) for a in lw2s_ref.combine(d["tau_g"], (d["tau_c"], d["ssa_c"], d["g_c"]), d["gb"]))
    d["lay"], d["lev"] = planck_sources(d["pfrac"], d["blay"], d["blev"], d["gb"])
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def regimes(dt, ncol, nlay):
    out = np.ascontiguousarray(np.broadcast_to(np.array(GPOINT_REGIMES, dtype="U20")[:, None], (NGPT, ncol)))
    out.setflags(write=False)
    return out


def column_regimes(reg):
    return lw_ref.column_regimes(reg, REGIMES)


def band_gpoints(ib):
    lo, hi = BAND_LIMS[ib]
    return np.arange(lo - 1, hi)


def angles_of(dt, ncol, nlay, angles):
    I = inputs(dt, ncol, nlay)
    return {"1": (I["sec1"], I["w1"]), "3": (I["sec3"], I["w3"])}[angles]


# ---- the solve ---------------------------------------------------------------------------------------------------------------------------
def scattering_factors(ssa, g, tiny, cn_coef):
    """st, Cn in the arrays' dtype; cn_coef is a value of that dtype"""
    F = ssa.dtype.type
    wb = ssa * (F(1) - g) * F(0.5)
    st = F(1) - ssa + wb
    return st, cn_coef * wb / np.maximum(st, F(3) * tiny)


def _truth_layers(tau, ssa, g, D, tiny):
    """tr, 1 - tr, fact, An, Cn in longdouble"""
    st, cn = scattering_factors(ssa, g, L(tiny), L(4) / L(10))             # (0.4 to longdouble, not the double 0.4 widened)
    tl = tau * D * st
    with np.errstate(under="ignore"):
        return np.exp(-tl), -np.expm1(-tl), lw_ref.source_factor(tl), -np.expm1(-L(2) * tl), cn


def _model_layers(tau, ssa, g, D, exp_rel, short_series, cn_coef):
    """the same five in the arrays' dtype as lw1r_ref.layers and lw1r_ref.solve evaluate them"""
    F = tau.dtype.type
    st, cn = scattering_factors(ssa, g, np.finfo(tau.dtype).tiny, F(cn_coef))
    tl = tau * D * st
    with np.errstate(under="ignore"):
        tr = lw1r_ref.exp(-tl)
    if exp_rel:
        tr = tr * F(1 + exp_rel)
    thres = np.sqrt(np.sqrt(np.finfo(tau.dtype).eps))
    omt = F(1) - tr
    with np.errstate(divide="ignore", invalid="ignore"):
        thick = omt / tl - tr
    series = tl * (F(0.5) + tl * F(-1. / 3.)) if short_series else tl * (F(0.5) + tl * (F(-1. / 3.) + tl * F(1. / 8.)))
    with np.errstate(under="ignore"):
        return tr, omt, np.where(tl > thres, thick, series), F(1) - tr * tr, cn


def truth_layer(tau, ssa, g, D, lay, lev_top, lev_bot, tiny):
    """tr, sdn, sup, Cn of every layer in longdouble (all arguments longdouble but `tiny`, the run's dtype's): what
    tests/test_lw1r_truth.py compares with mpmath"""
    tr, omt, fact, an, cn = _truth_layers(tau, ssa, g, D, tiny)
    return tr, omt * lev_bot + L(2) * fact * (lay - lev_bot), omt * lev_top + L(2) * fact * (lay - lev_top), cn


def _solve(dtype, layers, secants, weights, tau, ssa, g, lay_source, lev_source, sfc_emis, sfc_src, inc_flux, sfc_src_jac, top_at_1):
    dtype = np.dtype(dtype)
    F = dtype.type
    conv = lambda a: np.asarray(a).astype(dtype)
    secants, weights, tau, ssa, g, lay, lev = (conv(a) for a in (secants, weights, tau, ssa, g, lay_source, lev_source))
    emis, ssrc = conv(sfc_emis), conv(sfc_src)
    if not top_at_1:
        tau, ssa, g, lay, lev = tau[:, ::-1], ssa[:, ::-1], g[:, ::-1], lay[:, ::-1], lev[:, ::-1]
    ngpt, nlay, ncol = tau.shape
    pi = F(np.pi) if dtype != np.dtype(L) else lw2s_truth.PI_L
    shape = (ngpt, nlay + 1, ncol)
    out = [np.zeros(shape, dtype=dtype) for _ in range(3)]
    lev_top, lev_bot = lev[:, :-1], lev[:, 1:]
    with np.errstate(under="ignore"):
        for imu in range(weights.shape[0]):
            tr, omt, fact, an, cn = layers(tau, ssa, g, secants[imu][:, None, :])
            sdn = omt * lev_bot + F(2) * fact * (lay - lev_bot)
            sup = omt * lev_top + F(2) * fact * (lay - lev_top)
            dn = np.empty(shape, dtype=dtype); up = np.empty(shape, dtype=dtype); jac = np.empty(shape, dtype=dtype)
            dn[:, 0] = F(0) if inc_flux is None else conv(inc_flux) / pi
            for i in range(nlay):
                dn[:, i + 1] = tr[:, i] * dn[:, i] + sdn[:, i]
            up[:, nlay] = dn[:, nlay] * (F(1) - emis) + emis * ssrc
            jac[:, nlay] = emis * (conv(sfc_src_jac) if sfc_src_jac is not None else F(0))
            for i in range(nlay - 1, -1, -1):
                up[:, i] = tr[:, i] * up[:, i + 1] + sup[:, i] + cn[:, i] * (an[:, i] * dn[:, i] - tr[:, i] * sdn[:, i] - sup[:, i])
                jac[:, i] = tr[:, i] * jac[:, i + 1]
            for i in range(nlay):
                dn[:, i + 1] = tr[:, i] * dn[:, i] + sdn[:, i] + cn[:, i] * (an[:, i] * up[:, i + 1] - tr[:, i] * sup[:, i] - sdn[:, i])
            scale = pi * weights[imu]
            for acc, a in zip(out, (up, dn, jac)):
                acc += scale * a
    if not top_at_1:
        out = [a[:, ::-1] for a in out]
    return tuple(np.ascontiguousarray(a) for a in out)


def solve_truth(secants, weights, tau, ssa, g, lay_source, lev_source, sfc_emis, sfc_src, inc_flux=None, sfc_src_jac=None, top_at_1=False,
                run_dtype=None):
    """The truth: per-g-point (flux_up, flux_dn, flux_up_jac) in longdouble from the inputs as they are; run_dtype (default: tau's own)
    gives `tiny`"""
    tiny = np.finfo(np.dtype(tau.dtype if run_dtype is None else run_dtype)).tiny
    return _solve(L, lambda t, w, gg, D: _truth_layers(t, w, gg, D, tiny), secants, weights, tau, ssa, g, lay_source, lev_source, sfc_emis, sfc_src,
                  inc_flux, sfc_src_jac, top_at_1)


def solve_model(secants, weights, tau, ssa, g, lay_source, lev_source, sfc_emis, sfc_src, inc_flux=None, sfc_src_jac=None, top_at_1=False,
                exp_rel=0.0, short_series=False, cn_coef=CN_COEF):
    """lw1r_ref.solve in tau's dtype, with the hooks"""
    return _solve(tau.dtype, lambda t, w, gg, D: _model_layers(t, w, gg, D, exp_rel, short_series, cn_coef), secants, weights, tau, ssa, g,
                  lay_source, lev_source, sfc_emis, sfc_src, inc_flux, sfc_src_jac, top_at_1)


# ---- the cases of the tests: entry "general" (inputs as given), "fused" (combined in longdouble by the truth) or "null" (no cloud) ---------
ENTRIES = ("general", "fused", "null")


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def truth(dt, ncol, nlay, top_at_1, entry="general", angles="1", with_inc=True):
    I = inputs(dt, ncol, nlay)
    sec, w = angles_of(dt, ncol, nlay, angles)
    inc = I["inc"] if with_inc else None
    if entry == "general":
        return _frozen(solve_truth(sec, w, I["tau"], I["ssa"], I["g"], I["lay"], I["lev"], I["emis"], I["ssrc"], inc, I["sjac"], top_at_1))
    cld = None if entry == "null" else (I["tau_c"], I["ssa_c"], I["g_c"])
    tau, ssa, g = lw2s_truth.combine_truth(I["tau_g"], cld, I["gb"])
    lay, lev = planck_sources(I["pfrac"], I["blay"], I["blev"], I["gb"], L)
    return _frozen(solve_truth(sec, w, tau, ssa, g, lay, lev, I["emis"], I["ssrc"], inc, I["sjac"], top_at_1, run_dtype=np_dtype(dt)))


@functools.lru_cache(maxsize=None)
def model(dt, ncol, nlay, top_at_1, entry="general", angles="1", with_inc=True, hooks=()):
    I = inputs(dt, ncol, nlay)
    sec, w = angles_of(dt, ncol, nlay, angles)
    tau, ssa, g = (I["tau"], I["ssa"], I["g"]) if entry != "null" else lw2s_ref.combine(I["tau_g"], None, I["gb"])
    return _frozen(solve_model(sec, w, tau, ssa, g, I["lay"], I["lev"], I["emis"], I["ssrc"], I["inc"] if with_inc else None, I["sjac"], top_at_1,
                               **dict(hooks)))


def report(dt, label="kernel", quiet=False):
    return lw_ref.Report(dt, label, quiet, regimes=REGIMES, quantities=QUANTITIES, prefix=PREFIX, ref_name="model", fraction=True)


UNRESOLVED_FRACTION = 1e-2
