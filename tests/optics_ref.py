"""Plain numpy statements of what the kernels between gas optics and the solvers compute (csrc/rrx_misc.hip): cloud optics in its three
forms, aerosol optics, the full g-point increments, delta scaling, the broadband sum and net, col_dry and the TOA source kernels.
The references of tests/test_gpu_optics_kernels.py, themselves checked against the goldens of the reference's CPU classes and on
hand-written cases by tests/test_optics_ref.py.

Arrays follow the package's convention (synthetic.py): C-contiguous numpy arrays with the dimensions of the column-major C ABI
reversed, e.g. the ABI's tau(ncol, nlay, nbnd) is an array of shape (nbnd, nlay, ncol).

A function with a compute type `ctype` evaluates the kernel's expressions, operation by operation and in the kernel's order, in
that type: np.longdouble gives the truth; the arrays' own dtype gives the *working-precision evaluation* -- every operation rounded
once, nothing fused -- whose distance from the truth (`e_ref`) is the yardstick of the kernels' tolerance. Constants the kernel
holds in its own precision (9.81, the floors, the physical constants of col_dry) are rounded to the arrays' dtype first in both
evaluations: they are inputs. The functions without `ctype` are one exactly defined operation per element in the arrays' dtype."""
import numpy as np

# {0-based index into aermr01..11, hydrophilic?, 0-based table column}: the species in the order in which the kernel adds them
# (aerosol_species_table of csrc/rrx_misc.hip: SS1 SS2 SS3 DU1 DU2 DU3 OM1 OM2 BC1 BC2 SU)
AEROSOL_SPECIES = [(0, True, 0), (1, True, 1), (2, True, 2), (3, False, 0), (4, False, 7), (5, False, 5),
                   (7, False, 9), (6, True, 3), (8, False, 10), (9, False, 10), (10, True, 4)]


def eps_of(dt):
    return np.finfo(dt).eps


def floor_of(dt):
    """3*tiny of the stand-alone increment and delta-scale kernels, formed in the arrays' dtype"""
    dt = np.dtype(dt)
    return dt.type(3.) * np.finfo(dt).tiny


def delta_scale(tau, ssa, g, ctype):
    """rrx_delta_scale_2str_k: f = g*g, wf = ssa*f; tau*(1 - wf), (ssa - wf)/max(3*tiny, 1 - wf), (g - f)/max(3*tiny, 1 - f)"""
    floor = ctype(floor_of(tau.dtype))
    t, w, gg = (x.astype(ctype) for x in (tau, ssa, g))
    one = ctype(1.)
    f = gg*gg
    wf = w*f
    return t*(one - wf), (w - wf)/np.maximum(floor, one - wf), (gg - f)/np.maximum(floor, one - f)


def increment_1scalar(tau1, tau2):
    """rrx_increment_1scalar_by_1scalar: one addition"""
    return tau1 + tau2


def increment_2stream(t1, w1, g1, t2, w2, g2, ctype):
    """rrx_increment_2stream_by_2stream: tau = t1 + t2; ssa = (t1*w1 + t2*w2)/max(3*tiny, tau); g = ((t1*w1)*g1 + (t2*w2)*g2) /
    max(t1*w1 + t2*w2, 3*tiny). With ctype = the arrays' dtype, tau is the kernel's tau bit for bit (one addition)."""
    floor = ctype(floor_of(t1.dtype))
    a, wa, ga, b, wb, gb = (x.astype(ctype) for x in (t1, w1, g1, t2, w2, g2))
    tau = a + b
    scat = (a*wa) + (b*wb)
    g = ((a*wa*ga) + (b*wb*gb)) / np.maximum(scat, floor)
    ssa = scat / np.maximum(floor, tau)
    return tau, ssa, g


def sum_broadband(gpt_flux):
    """rrx_sum_broadband: (ngpt, nlev, ncol) -> (nlev, ncol), added in ascending g-point order starting from +0.0 (so a column of
    -0.0 sums to +0.0, and ngpt = 0 gives zeros)"""
    s = np.zeros(gpt_flux.shape[1:], dtype=gpt_flux.dtype)
    for ig in range(gpt_flux.shape[0]):
        s = s + gpt_flux[ig]
    return s


def net_broadband(flux_dn, flux_up):
    """rrx_net_broadband_precalc: one subtraction"""
    return flux_dn - flux_up


def spread_col(solar_source, ncol):
    """rrx_spread_col: toa_src (ngpt, ncol) = solar_source(igpt) on every column"""
    return np.ascontiguousarray(np.broadcast_to(solar_source[:, None], (solar_source.shape[0], ncol)))


def scaling_to_subset(toa_src, tsi_scaling):
    """rrx_scaling_to_subset: toa_src(igpt, icol) * tsi_scaling(icol), one multiplication"""
    return toa_src * tsi_scaling[None, :]


def toa_source(solar_source, tsi_scaling, ncol):
    """rrx_toa_source: solar_source(igpt) * tsi_scaling(icol), one multiplication; tsi_scaling = None: spread_col"""
    if tsi_scaling is None:
        return spread_col(solar_source, ncol)
    return solar_source[:, None] * tsi_scaling[None, :]


def col_dry(vmr_h2o, plev, ctype):
    """rrx_get_col_dry: vmr_h2o (nlay, ncol), plev (nlay+1, ncol), either column order:
    m_air = (m_dry + m_h2o*h)/(1 + h); col_dry = ((10*|dp|)*avogad) / (((1000*m_air)*100)*g0) / (1 + h)"""
    dt = vmr_h2o.dtype
    g0, avogad, m_dry, m_h2o = (ctype(dt.type(c)) for c in (9.80665, 6.02214076e23, 0.028964, 0.018016))
    p, h = plev.astype(ctype), vmr_h2o.astype(ctype)
    one = ctype(1.)
    dp = np.abs(p[:-1] - p[1:])
    m_air = (m_dry + m_h2o*h) / (one + h)
    cd = ctype(10.)*dp*avogad / (ctype(1000.)*m_air*ctype(100.)*g0)
    return cd / (one + h)


def size_table_position(re, lwr, upr, nsize, cloudy):
    """Where a particle size sits in a table of nsize equidistant nodes from lwr to upr: (index, x) with index the 1-based upper
    node of the interval, clamped to 1 .. nsize-1, and x = (re - lwr)/step. The step and x are formed in the arrays' dtype, as the
    host entry and the kernel form them. Cells that are not cloudy get (1, 0), whatever their size holds."""
    dt = re.dtype
    step = (dt.type(upr) - dt.type(lwr)) / (dt.type(nsize) - dt.type(1.))
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.where(cloudy, (re - dt.type(lwr)) / step, dt.type(0.)).astype(dt)
    index = np.clip(np.trunc(x).astype(np.int64) + 1, 1, nsize - 1)         # int() of C truncates toward zero
    return index, x


def cloud_optics(lut, clwp, ciwp, reliq, deice, ctype):
    """rrx_cloud_optics_2str, rrx_cloud_optics_1scl and rrx_cloud_optics_2str_delta on (nlay, ncol) water paths and sizes; lut as
    synthetic.make_cloud_lut gives it (tables (nbnd, nsize)). Returns ((tau, ssa, g), tau_1scl, (tau, ssa, g) delta-scaled), each
    array (nbnd, nlay, ncol) in ctype.

    Per phase and band, with i the clamped index and f = x - (i-1): tau_p = cwp*(ext[i-1] + f*(ext[i] - ext[i-1])), tau_p*ssa_p and
    tau_p*ssa_p*g_p alike; a phase with water path <= 0 contributes exact zeros. Outside the table the first / last interval is
    extrapolated. Two-stream: tau = sum, ssa = sum(tau*ssa)/max(tau, eps), g = sum(tau*ssa*g)/max(sum(tau*ssa), eps) with the
    machine epsilon; the delta step with the floor 3*tiny; 1-scalar: (tau_l - tau_l*ssa_l) + (tau_i - tau_i*ssa_i)."""
    dt = clwp.dtype
    eps, floor, one, zero = ctype(eps_of(dt)), ctype(floor_of(dt)), ctype(1.), ctype(0.)

    def phase(cwp, re, lwr, upr, nsize, names):
        cloudy = cwp > 0
        index, x = size_table_position(re, lut[lwr], lut[upr], int(lut[nsize]), cloudy)
        f = x.astype(ctype) - (index - 1).astype(ctype)
        w = cwp.astype(ctype)
        out = []
        prev = None
        for name in names:
            tab = np.asarray(lut[name]).astype(dt).astype(ctype)            # (nbnd, nsize), rounded to the arrays' dtype first
            lo, hi = tab[:, index-1], tab[:, index]                          # (nbnd, nlay, ncol)
            v = lo + f*(hi - lo)
            prev = w*v if prev is None else prev*v
            out.append(np.where(cloudy, prev, zero))
        return out

    lt, lts, ltsg = phase(clwp, reliq, "radliq_lwr", "radliq_upr", "nsize_liq", ("lut_extliq", "lut_ssaliq", "lut_asyliq"))
    it, its, itsg = phase(ciwp, deice, "diamice_lwr", "diamice_upr", "nsize_ice", ("lut_extice", "lut_ssaice", "lut_asyice"))
    t, tsc, tsg = lt + it, lts + its, ltsg + itsg
    ssa = tsc / np.maximum(t, eps)
    g = tsg / np.maximum(tsc, eps)
    tau_1scl = (lt - lts) + (it - its)
    f = g*g
    wf = ssa*f
    delta = (t*(one - wf), (ssa - wf)/np.maximum(floor, one - wf), (g - f)/np.maximum(floor, one - f))
    return (t, ssa, g), tau_1scl, delta


def humidity_class(rh_upper, rh):
    """0-based humidity class: the first upper bound >= rh, the last class where rh lies above every bound (the kernel's loop: step on
    while the bound is < rh and a next class exists)"""
    nhum = len(rh_upper)
    if nhum == 1:
        return np.zeros(rh.shape, dtype=np.int64)
    below = rh_upper[:nhum-1].reshape((-1,) + (1,)*rh.ndim) < rh[None]      # bound < rh: not this class
    return np.where(below.all(axis=0), nhum - 1, np.argmin(below, axis=0))


def aerosol_optics(lut, aermr, rh, plev, ctype):
    """rrx_aerosol_optics: aermr = the 11 mixing ratios aermr01..11, each a field (nlay, ncol) or a profile (nlay,); rh (nlay, ncol);
    plev (nlay+1, ncol), either column order; lut as synthetic.make_aerosol_lut gives it, in the arrays' dtype. Returns tau, ssa, g
    (nbnd, nlay, ncol) in ctype: per species od = (mmr*(|dp|/9.81))*mext, summed in the kernel's species order from zero into tau,
    sum(od*ssa) and sum((od*ssa)*g); ssa = sum(od*ssa)/max(tau, eps), g = sum(od*ssa*g)/max(sum(od*ssa), eps)."""
    dt = rh.dtype
    eps = ctype(eps_of(dt))
    nlay, ncol = rh.shape
    ihum = humidity_class(np.asarray(lut["rh_upper"]).astype(dt), rh)
    p = plev.astype(ctype)
    dpg = np.abs(p[:-1] - p[1:]) / ctype(dt.type(9.81))
    nbnd = lut["mext_phobic"].shape[-1]
    tab = {k: np.asarray(v).astype(dt).astype(ctype) for k, v in lut.items()}
    t, ts, tsg = (np.zeros((nbnd, nlay, ncol), dtype=ctype) for _ in range(3))
    for im, philic, col in AEROSOL_SPECIES:
        m = aermr[im].astype(ctype)
        od = (m if m.ndim == 2 else m[:, None]) * dpg
        if philic:
            look = lambda name: np.moveaxis(tab[name + "_philic"][col][ihum], -1, 0)        # (nbnd, nlay, ncol)
        else:
            look = lambda name: tab[name + "_phobic"][col][:, None, None]
        local = od[None] * look("mext")
        t = t + local
        ts = ts + local*look("ssa")
        tsg = tsg + local*look("ssa")*look("g")
    return t, ts / np.maximum(t, eps), tsg / np.maximum(ts, eps)


# ---- the tolerance of a kernel, from the reference alone -----------------------------------------------------------------------
E_REF_CAP = 16.0        # epsilons: above this the working-precision evaluation itself is ill-conditioned and the bound would hide errors


def rel_errors(values, truth, scale=None):
    """(largest |values - truth|/|scale| over the elements with scale != 0, in machine epsilons of values' dtype; whether every
    element whose truth is 0 is exactly 0 in values). scale = None: the truth itself."""
    truth = np.asarray(truth, dtype=np.longdouble)
    scale = np.abs(truth if scale is None else np.asarray(scale, dtype=np.longdouble))
    v = np.asarray(values)
    zero = truth == 0
    zeros_exact = bool((v[zero] == 0).all())
    m = (scale != 0) & ~zero
    if not m.any():
        return 0.0, zeros_exact
    err = np.max(np.abs(v[m].astype(np.longdouble) - truth[m]) / scale[m])
    return float(err / np.longdouble(np.finfo(v.dtype).eps)), zeros_exact


def kernel_bound(e_ref):
    """in epsilons: 2*e_ref (the kernel rounds like the working-precision evaluation except where a multiply and an add are fused,
    which removes a rounding but moves the worst case to other elements) + 2 (the fp32 quotient's allowance)"""
    return 2.0*e_ref + 2.0


# ---- inputs of the tolerance cases, shared by the CPU test of e_ref and the GPU tests ---------------------------------------------
def out_of_table_sizes(lwr, upr, nsize):
    """every node of the table, and 0.5 and 2.5 steps below and above it"""
    step = (upr - lwr)/(nsize - 1)
    nodes = lwr + step*np.arange(nsize)
    nodes[-1] = upr
    return np.concatenate([nodes, [lwr - 0.5*step, lwr - 2.5*step, upr + 0.5*step, upr + 2.5*step]])


def cloud_inputs(lut, nlay, ncol, rng, dtype):
    """(clwp, ciwp, reliq, deice), each (nlay, ncol): sizes uniform over the table; water paths 10**U(-3, 2.5), about 30 % of the
    cells cloud-free per phase (water path 0). Where the cells are enough (100 or more), the last ones hold, in cloudy cells, every
    node of both tables (both ends among them) and 0.5 / 2.5 steps outside on either side."""
    sl = out_of_table_sizes(lut["radliq_lwr"], lut["radliq_upr"], lut["nsize_liq"])
    si = out_of_table_sizes(lut["diamice_lwr"], lut["diamice_upr"], lut["nsize_ice"])
    nspec = max(len(sl), len(si))
    n = nlay*ncol
    reliq = rng.uniform(lut["radliq_lwr"], lut["radliq_upr"], n)
    deice = rng.uniform(lut["diamice_lwr"], lut["diamice_upr"], n)
    clwp, ciwp = (10.0**rng.uniform(-3, 2.5, n) * (rng.uniform(0., 1., n) >= 0.3) for _ in range(2))
    if n >= 100:
        reliq[n-nspec:n-nspec+len(sl)] = sl
        deice[n-nspec:n-nspec+len(si)] = si
        clwp[n-nspec:] = 10.0**rng.uniform(-3, 2.5, nspec)
        ciwp[n-nspec:] = 10.0**rng.uniform(-3, 2.5, nspec)
    return tuple(np.ascontiguousarray(a.astype(dtype)).reshape(nlay, ncol) for a in (clwp, ciwp, reliq, deice))


def hand_cloud_case(dtype):
    """(lut, clwp, ciwp, reliq, deice) of one band and 8 cells whose every intermediate value is a short binary fraction. Liquid
    nodes at 2, 4, 6 (step 2), ice nodes at 10, 20, 30. Liquid water path 2 on the sizes 4 (the middle node), 2 and 6 (the ends), -3
    (2.5 steps below: index clamped to 1, weight -2.5) and 11 (2.5 steps above: index 2, weight 3.5); a cloud-free cell (water paths 0
    and -1) with garbage sizes; an ice-only cell, its liquid path -1 and its radius NaN; a cell with both phases."""
    a = lambda *v: np.array([v], dtype=np.float64)
    lut = dict(radliq_lwr=2., radliq_upr=6., diamice_lwr=10., diamice_upr=30., nsize_liq=3, nsize_ice=3,
               lut_extliq=a(4., 2., 1.5), lut_ssaliq=a(.5, .25, .75), lut_asyliq=a(.5, .5, .25),
               lut_extice=a(1., .5, .25), lut_ssaice=a(.5, .5, .5), lut_asyice=a(.5, .5, .5))
    nan = np.nan
    clwp = np.array([[2., 2., 2., 2., 2., 0., -1., 2.]], dtype=dtype)
    reliq = np.array([[4., 2., 6., -3., 11., nan, nan, 4.]], dtype=dtype)
    ciwp = np.array([[0., 0., 0., 0., 0., -1., 1., 1.]], dtype=dtype)
    deice = np.array([[nan, -1e30, 20., 20., 20., -1e30, 20., 20.]], dtype=dtype)
    return lut, clwp, ciwp, reliq, deice


def aerosol_inputs(lut, nlay, ncol, top_at_1, kinds, rng, dtype):
    """(aermr list of 11, rh (nlay, ncol), plev (nlay+1, ncol)). kinds: "fields", "profiles" or "mixed" mixing ratios. The humidity
    holds every class bound, 0 and 1.05 (above the last bound) in its first cells."""
    rh = rng.uniform(0., 1., (nlay, ncol))
    special = np.concatenate([np.asarray(lut["rh_upper"], dtype=np.float64), [0., 1.05]])
    flat = rh.reshape(-1)
    k = min(len(special), flat.size)
    flat[:k] = special[:k]
    dp = rng.uniform(50., 5000., (nlay, ncol))
    plev = 100. + np.concatenate([np.zeros((1, ncol)), np.cumsum(dp, axis=0)])          # grows with the index: top first
    if not top_at_1:
        plev = plev[::-1]
    aermr = []
    for a in range(11):
        field = kinds == "fields" or (kinds == "mixed" and a % 2 == 0)
        aermr.append(np.ascontiguousarray((10.0**rng.uniform(-12, -7, (nlay, ncol) if field else (nlay,))).astype(dtype)))
    return aermr, np.ascontiguousarray(rh.astype(dtype)), np.ascontiguousarray(plev.astype(dtype))


def two_stream_inputs(shape, rng, dtype):
    """tau = 10**U(-4, 1.5), ssa in [0, 1], g in [0, 0.9]"""
    return tuple(np.ascontiguousarray(a.astype(dtype)) for a in
                 (10.0**rng.uniform(-4, 1.5, shape), rng.uniform(0., 1., shape), rng.uniform(0., .9, shape)))


def col_dry_inputs(nlay, ncol, top_at_1, rng, dtype):
    """(vmr_h2o in [0, 0.04] (nlay, ncol), plev (nlay+1, ncol))"""
    dp = rng.uniform(50., 5000., (nlay, ncol))
    plev = 100. + np.concatenate([np.zeros((1, ncol)), np.cumsum(dp, axis=0)])
    if not top_at_1:
        plev = plev[::-1]
    return np.ascontiguousarray(rng.uniform(0., 0.04, (nlay, ncol)).astype(dtype)), np.ascontiguousarray(plev.astype(dtype))
