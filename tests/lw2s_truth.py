"""Extended-precision truth and run-precision models for the LW two-stream solver with cloud scattering (rrx_lw_solver_2stream and
rrx_lw_solver_2stream_fractions), written from the formulas of DESIGN 4.10 and of the header of csrc/rrx_solver_lw2s.hip.
A follow-up to tests/lw_ref.py, whose norm (profile_error), bound (bound_eps, MARGIN, FLOOR_EPS), Report, ordered_sum, column_regimes and
planck_sources it uses. It is the yardstick of tests/test_gpu_lw2s_truth.py and is itself checked in tests/test_lw2s_truth.py (closed
forms, the layer against mpmath at 60 digits, the conditions on the inputs, the models' distance from it).

  layer    gamma1 = D (1 - ssa (1 + g)/2), gamma2 = D ssa (1 - g)/2, D = 1.66, k = sqrt(max((gamma1 - gamma2)(gamma1 + gamma2), 1e-12)),
           e1 = exp(-tau k), e2 = e1^2, RT = 1/(k (1 + e2) + gamma1 (1 - e2)), Rdif = RT gamma2 (1 - e2), Tdif = 2 RT k e1
  sources  tau > 1e-8: Z = (lev_bot - lev_top)/(tau (gamma1 + gamma2)), src_up = pi ((Z + lev_top) - Rdif (-Z + lev_top) - Tdif (Z + lev_bot)),
           src_dn = pi ((-Z + lev_bot) - Rdif (Z + lev_bot) - Tdif (-Z + lev_top)); thinner layers: both 0
  adding   the SW solver's diffuse recurrences; surface albedo 1 - emis, source pi emis sfc_src; flux_dn(top) = inc_flux

THE TRUTH (solve_truth, np.longdouble, the inputs widened exactly) evaluates that function without its cancellations:
  gamma1 - gamma2 = D (1 - ssa) and gamma1 + gamma2 = D (1 - ssa g) are formed algebraically (subtracting the gammas loses
  eps_L/(1 - ssa): no truth near ssa = 1); gamma1 is half their sum. The floor k^2 >= 1e-12 and the switch tau > 1e-8 are part of the
  function: both are kept, the switch as a comparison of tau and 1e-8 AS THE RUN'S DTYPE HOLDS THEM (for the fused entry tau is
  fl(tau_gas + tau_cloud)). u = 1 - e1 = -expm1(-x), m = 1 - e2 = -expm1(-2x), x = tau k.
  1 - Tdif = RT (k u^2 + gamma1 m);  c := (1 + Rdif - Tdif)/(tau G) - 1 = RT ((k u^2/(tau G) - gamma1 m) + k h(2x)),  G = gamma1 + gamma2,
  h(y) = 2 (1 - e^-y)/y - 1 - e^-y: below y = 1 the series -sum_{n>=2} (n - 1)(-y)^n/(n + 1)! to convergence (alternating, falling
  terms: no cancellation), above it the closed form through expm1 (h(1) = -0.10 from terms of size 1: three bits).
  src_up = pi ((lev_bot - lev_top) c + lev_bot (1 - Tdif) - Rdif lev_top), src_dn = pi (-(lev_bot - lev_top) c + lev_top (1 - Tdif) - Rdif lev_bot).
  The adding recurrences are sequential. For the fused entry gas and band cloud are combined in longdouble (tau = tau_g + tau_c,
  ssa = tau_c ssa_c/tau, g = g_c) and the level sources are formed in longdouble (lw_ref.planck_sources).

THE MODELS (solve_model, the run's dtype, numpy, the C library's exp, true division, sequential recurrences):
  form="regrouped"  the formulas of the header of rrx_solver_lw2s.hip (u through expm1, m = u (1 + e1), c = RT ((k u^2/(tau G) - gamma1 m)
                    + (m/tau - k (1 + e2)))): what stands behind E_regime in the bound of the GPU test
  form="written"    tests/lw2s_ref.solve as it stands: today's yardstick of tests/test_gpu_lw_2stream.py
  hooks (regrouped) exp_rel: e1 is multiplied by 1 + exp_rel, and u = 1 - e1 from x = 1/4 on (below, the header's series does not see
                    exp); thin_switch: another value for the 1e-8; drop_c: the term (lev_bot - lev_top) c left out.

Arrays follow hip_kernels.py: tau(ncol, nlay, ngpt) <-> shape (ngpt, nlay, ncol); band clouds (nbnd, nlay, ncol). Layers and levels are
in memory order; top_at_1 says which end is the top of the atmosphere. inputs() and regime_ranges() are documented where they stand."""
import functools

import numpy as np

import lw_ref
import lw1r_ref
import lw2s_ref
from lw_ref import L, np_dtype, planck_sources, ordered_sum, profile_error, bound_eps  # noqa: F401

QUANTITIES = ("flux_up", "flux_dn")
PREFIX = "LW2STRUTH"
D_L = L(166) / L(100)
PI_L = L(np.pi) + L(1.2246467991473532e-16)
TAU_THIN, K2_MIN = 1e-8, 1e-12

# ---- shapes ------------------------------------------------------------------------------------------------------------------------------
# (ncol, nlay): the smallest layer counts that reach each tiling of lw2s_fused / launch_lw2s (csrc/rrx_solver_lw2s.hip), checked against
# their with_k lists: need = ceil((nlay + 1) / ((64 / CLT) W)) layers per lane, the first K >= need of the tiling's list.
#   nlay   fp64 (8 x 8 lanes)                      fp32
#   15     W = 2, need 1,  K = 2                    16 x 4 lanes, W = 4, NW = 4: need 1, K = 2
#   40     W = 2, need 3,  K = 4                    need 3, K = 4
#   80     W = 2, need 6,  K = 6                    need 6, K = 6
#   140    W = 2, need 9,  K = 9                    need 9, K = 9 (to 143 layers)
#   180    W = 2, need 12, K = 12 (to 191)          16 x 4 lanes, W = 4, NW = 8: need 12, K = 12 (144 ... 191)
#   200    W = 4, need 7,  K = 9 (192 ... 287)      8 x 8 lanes, W = 4: need 7, K = 9
#   300    W = 8, need 5,  K = 5                    8 x 8 lanes, W = 8: K = 5
#   400    W = 8, need 7,  K = 7                    K = 7
#   500    W = 8, need 8,  K = 9 (to 575)           K = 9
#   600    need 10: no tiling; the materialised route (gas + cloud, level sources, lw_2stream_serial_kernel, g-point sums)
# Columns: 9 ... 20, odd counts among them; a column group is 8 (fp64) or 16 (fp32, up to 191 layers) columns, so every count but 16
# leaves one part-filled.
SHAPES = {dt: [(11, 15), (12, 40), (9, 80), (19, 140), (13, 180), (10, 200), (9, 300), (20, 400), (9, 500), (9, 600)] for dt in ("f64", "f32")}
BOTH_ORIENTATIONS = 2          # the two smallest shapes of each dtype run with top_at_1 False and True, the others with False
CASES = [(dt, s, top) for dt in ("f64", "f32") for i, s in enumerate(SHAPES[dt]) for top in ((False, True) if i < BOTH_ORIENTATIONS else (False,))]
IDS = [f"{dt}-{s[0]}x{s[1]}-top{int(t)}" for dt, s, t in CASES]

# ---- regimes -----------------------------------------------------------------------------------------------------------------------------
# One regime per g-point and the same in every column; a band holds one regime (the band cloud is shared by its g-points). 15 g-points in
# nine uneven bands. REGIMES is ordered by the regrouped model's own error against truth in fp64, smallest first (the table of
# tests/test_lw2s_truth.py); lw_ref.column_regimes(reg, REGIMES) gives a g-point sum the last of its members. thin_unlit is what the
# thin_lit g-points are called in a run without incident flux: their flux_dn is then layer emission alone, as thin_dark's always is.
BANDS = (("thin_dark", 1), ("thin_lit", 2), ("switch", 2), ("moderate", 2), ("moderate_cloud", 2), ("near_conservative", 1),
         ("conservative", 1), ("opaque", 1), ("wide", 3))
REGIMES = ("opaque", "moderate", "moderate_cloud", "wide", "switch", "near_conservative", "thin_lit", "conservative", "thin_unlit", "thin_dark")
GPOINT_REGIMES = tuple(r for r, n in BANDS for _ in range(n))
NGPT, NBND = len(GPOINT_REGIMES), len(BANDS)
GPOINT_BANDS = np.array([ib + 1 for ib, (r, n) in enumerate(BANDS) for _ in range(n)], dtype=np.int32)
BAND_LIMS = np.array([[int(np.flatnonzero(GPOINT_BANDS == ib + 1)[0]) + 1, int(np.flatnonzero(GPOINT_BANDS == ib + 1)[-1]) + 1] for ib in range(NBND)],
                     dtype=np.int32)                                            # 1-based, inclusive
# no incident flux even when the run has one: thin_dark, the second switch (which has no surface emission either: both of its fluxes are
# layer emission alone), the second moderate, the last wide
DARK_GPOINTS = (0, 4, 6, 14)
UNLIT_SURFACE = 4
# The seed of the first measurement, chosen by lw_ref.SEED's rule: tests/test_lw2s_truth.py holds the regrouped model to the table it
# recorded with it at every shape; were a heavy-tailed outlier to appear after a change of the inputs, take the next seed and say so
# here. The choice looks at the models and the inputs alone, never at a kernel.
SEED = 6161


# conservative in fp32 is narrower than the wide range of the table: with the wide range the regrouped MODEL alone is 1.9e4 eps from truth at
# 600 layers (8 x that is 1.9e-2 of the flux: an unresolved cell, tests/test_lw2s_truth.py) -- a column of 600 conservative layers of
# tau up to 30 passes 1e-3 of what enters it, and each layer's rounding in Rdif + Tdif = 1 is a source of eps of what it holds. The range is
# narrowed for that dtype (the total depth of the column falls by 30), not the list of unresolved cells extended; the k floor and ssa = 1
# bite at every tau.
CONSERVATIVE_F32 = (1e-4, 1.0)


def regime_ranges(dt):
    """regime -> (lo, hi): the interval that the optical depth of every layer lies in (as the run's dtype holds the sum of gas and
    cloud), layers of exactly 0 or 1e-9 apart (switch: a third of the layers; conservative, wide: three layers of 0). The same in both
    dtypes but for opaque, which reaches to the underflow of exp in each.
      thin_*            (1e-7, 1e-4)
      switch            (1.2e-8, 1e-6): above the thin-layer switch 1e-8 and more than 4 ulp from it
      moderate*, near_conservative   (0.05, 3)
      conservative, wide             (1e-4, 10^1.5); conservative in fp32 (1e-4, 1), see CONSERVATIVE_F32
      opaque            (4, 400 / 60), one layer at tau D = 725 / 95 (a denormal e1) and one at 1500 / 200 (e1 = 0 exactly)"""
    big = 400.0 if dt == "f64" else 60.0
    thin, mod, wide = (1e-7, 1e-4), (0.05, 3.0), (1e-4, 10.0**1.5)
    cons = wide if dt == "f64" else CONSERVATIVE_F32
    return dict(thin_dark=thin, thin_lit=thin, thin_unlit=thin, switch=(1.2e-8, 1e-6), moderate=mod, moderate_cloud=mod, near_conservative=mod,
                conservative=cons, opaque=(4.0, big), wide=wide)


# SENSITIVITY: how the draws are shaped so that the bound 8 x max(E_regime, 32 eps) tells the perturbed models of
# tests/test_lw2s_truth.py from the plain one in fp32 too. It looks at the inputs and the models alone.
#   exp off by d   Tdif = 2 k e1/(k (1 + e1^2) + gamma1 m) is stationary in e1 at e1 = 1 and carries at most d elsewhere, and below x = 1/4
#                  the header's series for u does not see exp: no flux amplifies d = 32 eps (fp32) beyond the 8 x 32 eps of the bound
#                  through Rdif, Tdif or 1 - Tdif. What does see it is the cancelling pair of c, m/tau - k (1 + e2) = -k d + O(x^2): an
#                  absolute d/2 in c, against a natural rounding of about one eps there, times (lev_bot - lev_top). With level sources
#                  drawn independently per level both sum like random walks over the layers and their ratio, 16, is too close to the
#                  margin of 8 to show at every shape. So the thin_lit band has a lapse (B_lev rises monotonically from 5 to 40, x a factor
#                  per column, pfrac constant over the layers): the terms of exp's error then add coherently, 16 eps x 35 pi of a flux_dn
#                  of inc_flux <= 5 at every nlay, while the roundings still add at random and leave E_regime of (thin_lit, flux_dn)
#                  near the floor.
#   switch at 1e-7 the layers of 1e-8 < tau <= 1e-7 lose their emission, 1e-7 of a lit flux: invisible in fp32 next to any surface or
#                  incident flux. So the second switch g-point has neither (inc_flux = 0, sfc_src = 0), and the band is isothermal per
#                  column (B_lev and the g-points' pfrac constant over the levels): lev_bot - lev_top = 0, the term with c vanishes and what
#                  is left, lev (1 - Tdif - Rdif), is good to a few eps of the emission -- both fluxes of that g-point are layer emission
#                  alone and resolved in both dtypes. Half of its layers lie below 1e-7.
#   drop_c         (lev_bot - lev_top) c is a third of a moderate layer's emission with level sources drawn from U(5, 40): nothing to shape.
def _loguniform(rng, a, b, shp):
    return np.exp(rng.uniform(np.log(a), np.log(b), shp))


def _draw_band(rng, regime, n, dt, nlay, ncol):
    """(tau_g (n, nlay, ncol), tau_c, ssa_c, g_c (nlay, ncol)) of one band in float64"""
    lo, hi = regime_ranges(dt)[regime]
    a, b = lo * (1 + 1e-6), hi * (1 - 1e-6)
    shp = (nlay, ncol)
    zero = np.zeros(shp)
    ssa_c, g_c = rng.uniform(0.0, 0.9, shp), rng.uniform(-0.3, 0.9, shp)
    if regime in ("thin_dark", "moderate"):                                   # no scattering: the band has no cloud
        return _loguniform(rng, a, b, (n,) + shp), zero, ssa_c, g_c
    if regime == "near_conservative":                                         # 1 - ssa = tau_g/(tau_g + tau_c) log-uniform in (1e-4, 1e-2)
        T, d = _loguniform(rng, a, b, shp), _loguniform(rng, 1.1e-4, 0.9e-2, shp)
        return (T * d)[None], T * (1 - d), np.ones(shp), g_c
    if regime == "conservative":                                              # no gas, ssa_c = 1: ssa = 1 exactly
        tau_c = _loguniform(rng, a, b, shp)
        tau_c[[0, nlay // 2, nlay - 1]] = 0.0
        return np.zeros((n,) + shp), tau_c, np.ones(shp), g_c
    if regime == "wide":                                                      # today's builder: clouds in a fifth of the cells
        tau_g = _loguniform(rng, a, b / 2, (n,) + shp)
        tau_c = np.where(rng.uniform(0, 1, shp) < 0.2, _loguniform(rng, 1e-2, b / 2, shp), 0.0)
        tau_g[:, [0, nlay // 2, nlay - 1]] = 0.0
        tau_c[[0, nlay // 2, nlay - 1]] = 0.0
        return tau_g, tau_c, ssa_c, g_c
    # cloud-like: the band's cloud is a share of the thinnest g-point's total, every total inside the interval
    if regime == "switch" and n == 2:
        T = np.stack([_loguniform(rng, a, b, shp), _loguniform(rng, a, 80.0 * a, shp)])      # the second: half of the layers below 1e-7
    else:
        T = _loguniform(rng, a, b, (n,) + shp)
    tau_c = rng.uniform(0.1, 0.9, shp) * T.min(axis=0)
    tau_g = T - tau_c
    if regime == "switch":                                                    # a third of the layers far below the switch: 0 or 1e-9
        low = np.arange(nlay) % 3 == 1
        tau_c[low] = 0.0
        tau_g[:, low] = np.where(np.arange(nlay)[low] % 2 == 0, 1e-9, 0.0)[None, :, None]
    if regime == "opaque":                                                    # pure gas there: k = D, e1 = exp(-tau D)
        tau_c[1:3] = 0.0
        tau_g[:, 1] = (725.0 if dt == "f64" else 95.0) / 1.66
        tau_g[:, 2] = (1.5e3 if dt == "f64" else 2e2) / 1.66
    return tau_g, tau_c, ssa_c, g_c


@functools.lru_cache(maxsize=None)
def inputs(dt, ncol, nlay):
    """The seeded inputs of one shape in the precision of the run, shared by the tests and read-only:
         gb, band_lims       GPOINT_BANDS, BAND_LIMS
         tau_g               (ngpt, nlay, ncol) gas optical depth;  cld = (tau_c, ssa_c, g_c), (nbnd, nlay, ncol) each
         pfrac, blev         Planck-lite level sources; the switch band is isothermal per column and the thin_lit band has a lapse, B_lev
                             rising from 5 to 40 over the levels (SENSITIVITY)
         tau, ssa, g, lev    the general entry's inputs: gas + cloud and the level sources formed in the run's dtype with numpy
                             (lw2s_ref.combine, lw_ref.planck_sources), as the materialised route forms them
         emis                U(0.8, 1), exactly 1 in every third column; ssrc U(5, 40), 0 in g-point UNLIT_SURFACE
         inc                 U(0, 5), zero in DARK_GPOINTS"""
    F = np_dtype(dt)
    rng = np.random.default_rng(SEED)
    drawn = [_draw_band(rng, r, n, dt, nlay, ncol) for r, n in BANDS]
    tau_g = np.concatenate([d[0] for d in drawn])
    cld = tuple(np.stack([d[i] for d in drawn]) for i in (1, 2, 3))
    pfrac = rng.uniform(0.05, 1.0, (NGPT, nlay, ncol))
    blev = rng.uniform(5., 40., (NBND, nlay + 1, ncol))
    sw = [ig for ig, r in enumerate(GPOINT_REGIMES) if r == "switch"]
    pfrac[sw] = pfrac[sw][:, :1]
    blev[GPOINT_BANDS[sw[0]] - 1] = blev[GPOINT_BANDS[sw[0]] - 1][:1]
    lit = [ig for ig, r in enumerate(GPOINT_REGIMES) if r == "thin_lit"]                      # a lapse: B_lev rises from 5 to 40 (SENSITIVITY)
    pfrac[lit] = pfrac[lit][:, :1]
    blev[GPOINT_BANDS[lit[0]] - 1] = np.linspace(5., 40., nlay + 1)[:, None] * rng.uniform(0.8, 1.2, (1, ncol))
    emis = rng.uniform(0.8, 1.0, (NGPT, ncol))
    emis[:, ::3] = 1.0
    inc = rng.uniform(0.1, 5., (NGPT, ncol))
    inc[list(DARK_GPOINTS)] = 0.0
    ssrc = rng.uniform(5., 40., (NGPT, ncol))
    ssrc[UNLIT_SURFACE] = 0.0
    d = dict(gb=GPOINT_BANDS, band_lims=BAND_LIMS, tau_g=tau_g, tau_c=cld[0], ssa_c=cld[1], g_c=cld[2], pfrac=pfrac, blev=blev, emis=emis,
             ssrc=ssrc, inc=inc)
    d = {k: (np.ascontiguousarray(v.astype(F)) if v.dtype.kind == "f" else v) for k, v in d.items()}
    d["tau"], d["ssa"], d["g"] = (np.ascontiguousarray(a) for a in lw2s_ref.combine(d["tau_g"], (d["tau_c"], d["ssa_c"], d["g_c"]), d["gb"]))
    d["lev"] = planck_sources(d["pfrac"], np.zeros_like(d["blev"][:, 1:]), d["blev"], d["gb"])[1]
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def regimes(dt, ncol, nlay, with_inc=True):
    """The regime of each (g-point, column) profile, (ngpt, ncol) strings; without incident flux thin_lit is called thin_unlit"""
    names = [("thin_unlit" if (r == "thin_lit" and not with_inc) else r) for r in GPOINT_REGIMES]
    out = np.ascontiguousarray(np.broadcast_to(np.array(names, dtype="U20")[:, None], (NGPT, ncol)))
    out.setflags(write=False)
    return out


def column_regimes(reg):
    return lw_ref.column_regimes(reg, REGIMES)


def band_gpoints(ib):
    lo, hi = BAND_LIMS[ib]
    return np.arange(lo - 1, hi)


# ---- the layer ---------------------------------------------------------------------------------------------------------------------------
def h_factor(y):
    """h(y) = 2 (1 - e^-y)/y - 1 - e^-y for y >= 0 in longdouble"""
    y = np.asarray(y, dtype=L)
    ys = np.where(y < L(1), y, L(0))
    term = ys * ys / L(6)                                          # t_2 = (2 - 1) y^2 / 3!;  t_(n+1) = -t_n y n / ((n - 1)(n + 2))
    s = -term
    for n in range(2, 60):
        term = -term * ys * L(n) / (L(n - 1) * L(n + 2))
        s -= term
    yb = np.where(y < L(1), L(1), y)
    closed = L(2) * (-np.expm1(-yb)) / yb - L(1) - np.exp(-yb)
    return np.where(y < L(1), s, closed)


def truth_layer(tau, ssa, g, lev_top, lev_bot, thick, k2_min=L(K2_MIN)):
    """Rdif, Tdif, src_up, src_dn of every layer in longdouble (all arguments longdouble but `thick`, the outcome of the thin-layer
    switch in the run's dtype)"""
    one, two = L(1), L(2)
    gd, gs = D_L * (one - ssa), D_L * (one - ssa * g)              # gamma1 - gamma2, gamma1 + gamma2
    gamma1, gamma2 = (gs + gd) / two, D_L * ssa * (one - g) / two
    k = np.sqrt(np.maximum(gd * gs, k2_min))
    x = tau * k
    with np.errstate(under="ignore"):
        e1, e2, u, m = np.exp(-x), np.exp(-two * x), -np.expm1(-x), -np.expm1(-two * x)
        rt = one / (k * (one + e2) + gamma1 * m)
        rdif, tdif = rt * gamma2 * m, two * rt * k * e1
        omt = rt * (k * u * u + gamma1 * m)
        ts = np.where(thick, tau, one)
        c = rt * ((k * u * u / (ts * gs) - gamma1 * m) + k * h_factor(two * x))
        dc = (lev_bot - lev_top) * c
        su = PI_L * (dc + lev_bot * omt - rdif * lev_top)
        sd = PI_L * (-dc + lev_top * omt - rdif * lev_bot)
    zero = L(0)
    return rdif, tdif, np.where(thick, su, zero), np.where(thick, sd, zero)


def model_layer(tau, ssa, g, lev_top, lev_bot, exp_rel=0.0, thin_switch=TAU_THIN, drop_c=False):
    """The same four in the arrays' dtype by the regrouped formulas of the header of rrx_solver_lw2s.hip"""
    F = tau.dtype.type
    Dd, one, two = F(1.66), F(1), F(2)
    gamma1 = Dd * (one - F(.5) * ssa * (one + g))
    gamma2 = Dd * F(.5) * ssa * (one - g)
    gsum = gamma1 + gamma2
    k = np.sqrt(np.maximum((gamma1 - gamma2) * gsum, F(K2_MIN)))
    x = tau * k
    with np.errstate(under="ignore"):
        e1 = lw1r_ref.exp(-x)
        u = -np.expm1(-x)
        if exp_rel:
            e1 = e1 * F(1 + exp_rel)
            u = np.where(x < F(.25), u, one - e1)
        m = u * (one + e1)
        kp = k * (one + e1 * e1)
        rt = one / (kp + gamma1 * m)
        ku2, g1m = k * u * u, gamma1 * m
        rdif, tdif = rt * gamma2 * m, rt * two * k * e1
        omt = rt * (ku2 + g1m)
        thick = tau > F(thin_switch)
        ts = np.where(thick, tau, one)
        c = rt * ((ku2 / (ts * gsum) - g1m) + (m / ts - kp))
        dc = F(0) * c if drop_c else (lev_bot - lev_top) * c
        pi = F(np.pi)
        su = pi * (dc + (lev_bot * omt - rdif * lev_top))
        sd = pi * ((lev_top * omt - rdif * lev_bot) - dc)
    return rdif, tdif, np.where(thick, su, F(0)), np.where(thick, sd, F(0))


def adding(rdif, tdif, s_up, s_dn, sfc_emis, sfc_src, inc_flux, pi):
    """The adding recurrences, sequentially, in the arrays' dtype; layers and levels in sweep order from the top. (flux_up, flux_dn)"""
    dtype = rdif.dtype
    one = dtype.type(1)
    ngpt, nlay, ncol = rdif.shape
    alb = np.empty((ngpt, nlay + 1, ncol), dtype=dtype); src = np.empty_like(alb); den = np.empty_like(rdif)
    alb[:, nlay] = one - sfc_emis
    src[:, nlay] = pi * sfc_emis * sfc_src
    for s in range(nlay - 1, -1, -1):
        den[:, s] = one / (one - rdif[:, s] * alb[:, s + 1])
        src[:, s] = s_up[:, s] + tdif[:, s] * den[:, s] * (src[:, s + 1] + alb[:, s + 1] * s_dn[:, s])
        alb[:, s] = rdif[:, s] + tdif[:, s] * tdif[:, s] * alb[:, s + 1] * den[:, s]
    up = np.empty_like(alb); dn = np.empty_like(alb)
    dn[:, 0] = dtype.type(0) if inc_flux is None else inc_flux
    up[:, 0] = dn[:, 0] * alb[:, 0] + src[:, 0]
    for s in range(nlay):
        dn[:, s + 1] = (tdif[:, s] * dn[:, s] + rdif[:, s] * src[:, s + 1] + s_dn[:, s]) * den[:, s]
        up[:, s + 1] = dn[:, s + 1] * alb[:, s + 1] + src[:, s + 1]
    return up, dn


def _oriented(arrays, top_at_1):
    return arrays if top_at_1 else tuple(a[:, ::-1] for a in arrays)


def solve_truth(tau, ssa, g, lev_source, sfc_emis, sfc_src, inc_flux=None, top_at_1=True, thick=None, run_dtype=None):
    """The truth: per-g-point (flux_up, flux_dn), (ngpt, nlay+1, ncol) longdouble in memory order, from the inputs as they are
    (widening is exact). thick: the outcome of the thin-layer switch per layer; default: tau > 1e-8 as run_dtype (default: tau's own
    dtype) holds both."""
    if thick is None:
        F = np.dtype(tau.dtype if run_dtype is None else run_dtype).type
        thick = np.asarray(tau).astype(F) > F(TAU_THIN)
    F = np.dtype(tau.dtype if run_dtype is None else run_dtype).type
    k2 = L(F(K2_MIN)) if F is not L else L(K2_MIN)
    conv = lambda a: None if a is None else np.asarray(a).astype(L)
    tau, ssa, g, lev, thick = _oriented((conv(tau), conv(ssa), conv(g), conv(lev_source), np.asarray(thick)), top_at_1)
    r, t, su, sd = truth_layer(tau, ssa, g, lev[:, :-1], lev[:, 1:], thick, k2)
    with np.errstate(under="ignore"):
        up, dn = adding(r, t, su, sd, conv(sfc_emis), conv(sfc_src), conv(inc_flux), PI_L)
    return tuple(np.ascontiguousarray(a) for a in _oriented((up, dn), top_at_1))


def solve_model(tau, ssa, g, lev_source, sfc_emis, sfc_src, inc_flux=None, top_at_1=True, form="regrouped", **hooks):
    """A model in tau's dtype: form "regrouped" (hooks exp_rel, thin_switch, drop_c) or "written" (lw2s_ref.solve as it stands)"""
    if form == "written":
        assert not hooks
        with np.errstate(under="ignore", over="ignore", invalid="ignore"):
            return lw2s_ref.solve(tau, ssa, g, lev_source, sfc_emis, sfc_src, inc_flux, top_at_1)
    assert form == "regrouped", form
    tau, ssa, g, lev = _oriented((tau, ssa, g, lev_source), top_at_1)
    r, t, su, sd = model_layer(tau, ssa, g, lev[:, :-1], lev[:, 1:], **hooks)
    with np.errstate(under="ignore"):
        up, dn = adding(r, t, su, sd, sfc_emis, sfc_src, inc_flux, tau.dtype.type(np.pi))
    return tuple(np.ascontiguousarray(a) for a in _oriented((up, dn), top_at_1))


def combine_truth(tau_g, cld, gpoint_bands):
    """gas + band cloud in longdouble: tau = tau_g + tau_c, ssa = tau_c ssa_c/tau (0 where tau = 0), g = g_c. cld None: ssa = g = 0"""
    tg = np.asarray(tau_g).astype(L)
    if cld is None:
        return tg, np.zeros_like(tg), np.zeros_like(tg)
    ib = np.asarray(gpoint_bands) - 1
    tc, wc, gc = (np.asarray(a).astype(L)[ib] for a in cld)
    tau = tg + tc
    return tau, tc * wc / np.where(tau > 0, tau, L(1)), gc


# ---- the cases of the tests ---------------------------------------------------------------------------------------------------------------
# entry: "general" (rrx_lw_solver_2stream on I["tau"], I["ssa"], I["g"], I["lev"] as given), "fused" (rrx_lw_solver_2stream_fractions:
# gas, band cloud and Planck-lite sources, combined in longdouble by the truth and in the run's dtype by the model) or "null" (the fused
# entry with null cloud arrays: pure absorption by the gas)
ENTRIES = ("general", "fused", "null")


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _cloud(I, entry):
    return None if entry == "null" else (I["tau_c"], I["ssa_c"], I["g_c"])


@functools.lru_cache(maxsize=None)
def truth(dt, ncol, nlay, top_at_1, entry="general", with_inc=True):
    """Per-g-point longdouble (flux_up, flux_dn) of a case, computed once and read-only"""
    I = inputs(dt, ncol, nlay)
    F = np_dtype(dt)
    inc = I["inc"] if with_inc else None
    if entry == "general":
        return _frozen(solve_truth(I["tau"], I["ssa"], I["g"], I["lev"], I["emis"], I["ssrc"], inc, top_at_1))
    cld = _cloud(I, entry)
    tau, ssa, g = combine_truth(I["tau_g"], cld, I["gb"])
    thick = lw2s_ref.combine(I["tau_g"], cld, I["gb"])[0] > F(TAU_THIN)          # fl(tau_gas + tau_cloud) against fl(1e-8)
    lev = planck_sources(I["pfrac"], np.zeros_like(I["blev"][:, 1:]), I["blev"], I["gb"], L)[1]
    return _frozen(solve_truth(tau, ssa, g, lev, I["emis"], I["ssrc"], inc, top_at_1, thick=thick, run_dtype=F))


@functools.lru_cache(maxsize=None)
def model(dt, ncol, nlay, top_at_1, entry="general", with_inc=True, form="regrouped", hooks=()):
    """solve_model on the case, everything formed in the run's dtype; hooks: a tuple of (name, value) pairs"""
    I = inputs(dt, ncol, nlay)
    inc = I["inc"] if with_inc else None
    tau, ssa, g = (I["tau"], I["ssa"], I["g"]) if entry != "null" else lw2s_ref.combine(I["tau_g"], None, I["gb"])
    return _frozen(solve_model(tau, ssa, g, I["lev"], I["emis"], I["ssrc"], inc, top_at_1, form, **dict(hooks)))


def as_dict(fluxes, gpts=None, summed=False):
    out = {}
    for q, a in zip(QUANTITIES, fluxes):
        a = a if gpts is None else a[gpts]
        out[q] = ordered_sum(a) if summed else a
    return out


def report(dt, label="kernel", quiet=False):
    return lw_ref.Report(dt, label, quiet, regimes=REGIMES, quantities=QUANTITIES, prefix=PREFIX, ref_name="model", fraction=True)


# A (regime, quantity, dtype) cell whose bound exceeds this fraction of the profile's largest flux tests nothing: "unresolved"
UNRESOLVED_FRACTION = 1e-2
