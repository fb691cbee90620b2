"""Plain numpy statements of what the column-ordering kernels (csrc/rrx_columns.hip) and the glue kernels (csrc/rrx_misc.hip) compute:
the references of tests/test_gpu_support_kernels.py, themselves checked on hand-written cases by tests/test_support_ref.py.

Arrays follow the package's convention (synthetic.py): C-contiguous numpy arrays with the dimensions of the column-major C ABI
reversed, e.g. the ABI's gpt_flux(ncol, nlev, ngpt) is an array of shape (ngpt, nlev, ncol)."""
import numpy as np


# ---- column order ------------------------------------------------------------------------------------------------------------
def sort_perm(key, npad):
    """rrx_sort_columns: the stable ascending order of key, then npad repeats of its last entry"""
    order = np.argsort(key, kind="stable").astype(np.int32)
    return np.concatenate([order, np.full(npad, order[-1], dtype=np.int32)])


def identity_perm(ncol, npad):
    """rrx_identity_columns: perm[i] = min(i, ncol-1)"""
    return np.minimum(np.arange(ncol + npad), ncol - 1).astype(np.int32)


def run_ratios(key, block):
    """(max - min)/mean of every FULL run of `block` consecutive keys, in float64; a trailing partial run is left out"""
    nfull = len(key) // block
    runs = np.asarray(key[:nfull*block], dtype=np.float64).reshape(nfull, block)
    if nfull == 0:
        return np.zeros(0)
    return (runs.max(axis=1) - runs.min(axis=1)) / runs.mean(axis=1)


def column_spread(key, block, threshold):
    """rrx_column_spread: 1 where some full run of `block` consecutive keys has max - min > threshold*mean, else 0"""
    return int(bool((run_ratios(key, block) > threshold).any()))


def spread_run(n, ratio, mean_level, rng):
    """n keys (float64) whose (max - min)/mean is `ratio`, up to rounding: level*(1 + r*u) with u in [0, 1] holding both 0 and 1,
    so max - min = level*r and mean = level*(1 + r*mean(u)), hence r = ratio/(1 - ratio*mean(u))"""
    u = rng.uniform(0., 1., n)
    if n >= 2:
        i, j = rng.choice(n, 2, replace=False)
        u[i], u[j] = 0., 1.
    else:
        u[:] = 0.
    r = ratio / (1. - ratio*u.mean())
    return mean_level*(1. + r*u)


def gather_cols(a, perm):
    """rrx_gather_cols: out(i, r) = in(perm[i], r); the column is the LAST axis of the numpy array"""
    return np.ascontiguousarray(a[..., perm])


def scatter_cols(src, perm, n, dst):
    """rrx_scatter_cols: dst(perm[i], r) = src(i, r) for i < n, the rest of dst as it was (returns a copy)"""
    out = dst.copy()
    out[..., perm[:n]] = src[..., :n]
    return out


def gather_lastdim(a, perm):
    """rrx_gather_lastdim: out(b, i) = in(b, perm[i]) for ABI arrays (n1, ncol), i.e. numpy arrays (ncol, n1): rows are picked"""
    return np.ascontiguousarray(a[perm, :])


# ---- glue --------------------------------------------------------------------------------------------------------------------
def subset_nd(a, starts, sub_dims):
    """rrx_subset_nd as include/Array.h calls it. a: numpy array whose axes are the ABI's dimensions REVERSED; starts (0-based) and
    sub_dims are in the ABI's order (first = fastest). A dimension of extent 1 in `a` is broadcast over its sub_dims entry (its
    start is not used); every other dimension is sliced. Returns (out, strides, spread): the expected block (axes reversed like
    a), and the element strides and spread flags (ABI order) the call takes."""
    dims = a.shape[::-1]
    ndim = len(dims)
    strides = [int(np.prod(dims[:d], dtype=np.int64)) for d in range(ndim)]
    spread = [int(dims[d] == 1) for d in range(ndim)]
    out = a
    for d in range(ndim):
        axis = ndim - 1 - d
        if spread[d]:
            out = np.repeat(out, sub_dims[d], axis=axis)
        else:
            out = np.take(out, np.arange(starts[d], starts[d] + sub_dims[d]), axis=axis)
    return np.ascontiguousarray(out), strides, spread


def band_layout(sizes):
    """(nbnd, 2) int32 1-based inclusive g-point limits of consecutive bands of the given sizes; a size of 0 is an empty band
    (hi = lo - 1; after the last g-point its lo is ngpt + 1)"""
    lims, g = [], 1
    for n in sizes:
        lims.append((g, g + n - 1)); g += n
    return np.array(lims, dtype=np.int32).reshape(-1, 2)


def sum_byband(gpt, lims):
    """rrx_sum_byband: per band the sum of its g-points' (ngpt, ...) slabs, added in g-point order starting from the band's first
    g-point (not from zero: a -0.0 stays -0.0); an empty band (hi < lo) is exact zeros and reads nothing"""
    out = np.zeros((len(lims),) + gpt.shape[1:], dtype=gpt.dtype)
    for ib, (lo, hi) in enumerate(lims):
        if hi < lo:
            continue
        s = gpt[lo-1].copy()
        for ig in range(lo, hi):
            s = s + gpt[ig]
        out[ib] = s
    return out


def net_byband(dn, up, lims):
    """rrx_net_byband_full: per band the sum of (dn - up) over its g-points, in g-point order; empty bands are exact zeros"""
    out = np.zeros((len(lims),) + dn.shape[1:], dtype=dn.dtype)
    for ib, (lo, hi) in enumerate(lims):
        if hi < lo:
            continue
        s = dn[lo-1] - up[lo-1]
        for ig in range(lo, hi):
            s = s + (dn[ig] - up[ig])
        out[ib] = s
    return out


def gpoint_band(lims, ngpt):
    """0-based band of every g-point, -1 for the g-points that lie in no band"""
    gb = np.full(ngpt, -1, dtype=np.int64)
    for ib, (lo, hi) in enumerate(lims):
        gb[lo-1:hi] = ib
    return gb


def expand_and_transpose(arr, lims, ngpt, out):
    """rrx_expand_and_transpose: arr (ncol, nbnd) -> (ngpt, ncol), every g-point of a band gets the band's value; the g-points of
    no band keep what `out` held (returns a copy)"""
    out = out.copy()
    for ig, ib in enumerate(gpoint_band(lims, ngpt)):
        if ib >= 0:
            out[ig] = arr[:, ib]
    return out


def inc_1scalar_bybnd(tau, tau_bnd, lims):
    """rrx_inc_1scalar_by_1scalar_bybnd: tau(gpt) + tau_bnd(band of gpt), one addition; g-points of no band untouched"""
    out = tau.copy()
    for ig, ib in enumerate(gpoint_band(lims, tau.shape[0])):
        if ib >= 0:
            out[ig] = tau[ig] + tau_bnd[ib]
    return out


def inc_2stream_bybnd(t1, w1, g1, t2, w2, g2, lims, eps):
    """rrx_inc_2stream_by_2stream_bybnd: tau = tau1 + tau2 in the arrays' own precision (one addition: exact reference); ssa and g
    from the kernel's expressions evaluated in np.longdouble (returned as longdouble; see the test for the tolerance). The
    g-points of no band keep their values."""
    T, W, G = t1.copy(), w1.astype(np.longdouble), g1.astype(np.longdouble)
    for ig, ib in enumerate(gpoint_band(lims, t1.shape[0])):
        if ib < 0:
            continue
        a, wa, ga, b, wb, gb_ = (x.astype(np.longdouble) for x in (t1[ig], w1[ig], g1[ig], t2[ib], w2[ib], g2[ib]))
        scat = a*wa + b*wb
        G[ig] = (a*wa*ga + b*wb*gb_) / np.maximum(scat, eps)
        W[ig] = scat / np.maximum(eps, a + b)
        T[ig] = t1[ig] + t2[ib]
    return T, W, G


def get_from_subset(fulls, subs, col_s):
    """rrx_get_from_subset: columns col_s .. col_s+ncol_in-1 (1-based) of every full array take the subset array; the rest stays"""
    out = [f.copy() for f in fulls]
    for f, s in zip(out, subs):
        f[..., col_s-1:col_s-1+s.shape[-1]] = s
    return out


def fill_gases(col_dry, vmrs):
    """rrx_fill_gases_all / the rrx_fill_gases loop: col_gas (ngas+1, nlay, ncol), slot 0 = col_dry, slot i = vmr_i*col_dry (one
    multiplication in the arrays' precision). vmrs: scalars as (1, 1), profiles as (nlay, 1), fields as (nlay, ncol) arrays"""
    out = np.empty((len(vmrs) + 1,) + col_dry.shape, dtype=col_dry.dtype)
    out[0] = col_dry
    for i, v in enumerate(vmrs):
        out[i+1] = np.broadcast_to(v, col_dry.shape) * col_dry
    return out


def heating_rate(flux_net, plev, g_over_cp):
    """-(g/cp) * (F[k+1] - F[k]) / (p[k+1] - p[k]) in np.longdouble from the given (already rounded) inputs; (nlev, ncol) arrays"""
    F, p = flux_net.astype(np.longdouble), plev.astype(np.longdouble)
    return -np.longdouble(g_over_cp) * (F[1:] - F[:-1]) / (p[1:] - p[:-1])
