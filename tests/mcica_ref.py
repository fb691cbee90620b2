"""numpy restatement of the McICA cloud sampling (csrc/rrx_mcica.hip): Philox4x32-10, the 24-bit uniform, the
overlap walk and the sampled increments. Arrays are in the package's tensor convention: cloud_frac (nlay, ncol), alpha
(nlay-1, ncol), g-point arrays (ngpt, nlay, ncol), band arrays (nbnd, nlay, ncol), masks uint8 (ngpt, nlay, ncol)."""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four, key: two arrays (or scalars) of 32-bit words, broadcast together; returns the four output words (uint32)."""
    c = [np.asarray(x).astype(np.uint64) & _M32 for x in ctr]
    k = [np.asarray(x).astype(np.uint64) & _M32 for x in key]
    c = list(np.broadcast_arrays(*c))
    for r in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k[0]) & _M32, p1 & _M32, ((p0 >> np.uint64(32)) ^ c[3] ^ k[1]) & _M32, p0 & _M32]
        k = [(k[0] + np.uint64(PHILOX_W0)) & _M32, (k[1] + np.uint64(PHILOX_W1)) & _M32]
    return [x.astype(np.uint32) for x in c]


def uniform(x, dtype):
    """(x >> 9) + 0.5, times 2^-23: exact in float32 and float64, in (0, 1)."""
    F = np.dtype(dtype).type
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(dtype) + F(0.5)) * F(2.0 ** -23)


def draws(seed, domain, which, col_id, ngpt, nlay, dtype):
    """The uniform of every cell: (ngpt, nlay, ncol). which = 0: rank draw u, 1: overlap draw v."""
    col_id = np.asarray(col_id, dtype=np.int64)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    ig = np.arange(ngpt, dtype=np.int64)[:, None, None]
    il = np.arange(nlay, dtype=np.int64)[None, :, None]
    ic = col_id[None, None, :]
    shape = (ngpt, nlay, col_id.size)
    words = philox4x32_10((np.broadcast_to(ic, shape), np.broadcast_to(ig, shape), np.broadcast_to(il // 4, shape),
                           np.full(shape, 2*domain + which, dtype=np.int64)), key)
    sel = np.broadcast_to(il % 4, shape)
    x = np.choose(sel, words)
    return uniform(x, dtype)


def cloud_mask(cloud_frac, alpha, seed, domain, col_id, ngpt):
    """uint8 (ngpt, nlay, ncol). alpha None: maximum-random overlap; else exponential-random in the two-draw form."""
    cloud_frac = np.asarray(cloud_frac)
    dtype = cloud_frac.dtype
    F = dtype.type
    nlay, ncol = cloud_frac.shape
    u = draws(seed, domain, 0, col_id, ngpt, nlay, dtype)
    v = draws(seed, domain, 1, col_id, ngpt, nlay, dtype)
    mask = np.zeros((ngpt, nlay, ncol), dtype=np.uint8)
    rank = u[:, 0, :].copy()
    for ilay in range(nlay):
        if ilay > 0:
            a = np.ones((ncol,), dtype=dtype) if alpha is None else np.asarray(alpha, dtype=dtype)[ilay-1]
            keep = (cloud_frac[ilay-1] > 0)[None, :] & (v[:, ilay, :] < a[None, :])
            rank = np.where(keep, rank, u[:, ilay, :])
        f = cloud_frac[ilay][None, :]
        mask[:, ilay, :] = (f > 0) & (rank > F(1) - f)
    return mask


def band_of_gpt(band_lims, ngpt):
    """0-based band of every g-point from (nbnd, 2) 1-based inclusive limits; -1 for the g-points of no band."""
    out = np.full((ngpt,), -1, dtype=np.int64)
    for ib, (lo, hi) in enumerate(np.asarray(band_lims)):
        for ig in range(int(lo), int(hi) + 1):
            if 1 <= ig <= ngpt and out[ig-1] < 0:
                out[ig-1] = ib
    return out


def expand_bands(arr_bnd, band_lims, ngpt):
    """(nbnd, nlay, ncol) -> (ngpt, nlay, ncol); zeros in the g-points of no band."""
    b = band_of_gpt(band_lims, ngpt)
    out = np.zeros((ngpt,) + arr_bnd.shape[1:], dtype=arr_bnd.dtype)
    out[b >= 0] = arr_bnd[b[b >= 0]]
    return out


def sampled_mask(mask, band_lims):
    """The cells an increment touches: cloudy and inside a band."""
    b = band_of_gpt(band_lims, mask.shape[0])
    return (mask != 0) & (b >= 0)[:, None, None]


def increment_1scalar(tau, cld_tau, mask, band_lims):
    hit = sampled_mask(mask, band_lims)
    return np.where(hit, tau + expand_bands(cld_tau, band_lims, tau.shape[0]), tau)


def inc_2str(tau1, ssa1, g1, tau2, ssa2, g2):
    """increment_2stream_by_2stream's arithmetic (eps = 3 * the smallest normal number), operation for operation."""
    eps = np.finfo(tau1.dtype).tiny * tau1.dtype.type(3.)
    tau12 = tau1 + tau2
    tauscat12 = (tau1 * ssa1) + (tau2 * ssa2)
    g = ((tau1 * ssa1 * g1) + (tau2 * ssa2 * g2)) / np.maximum(tauscat12, eps)
    ssa = tauscat12 / np.maximum(eps, tau12)
    return tau12, ssa, g


def increment_2stream(tau, ssa, g, cld_tau, cld_ssa, cld_g, mask, band_lims):
    hit = sampled_mask(mask, band_lims)
    ng = tau.shape[0]
    t, w, gg = inc_2str(tau, ssa, g, expand_bands(cld_tau, band_lims, ng), expand_bands(cld_ssa, band_lims, ng),
                        expand_bands(cld_g, band_lims, ng))
    return np.where(hit, t, tau), np.where(hit, w, ssa), np.where(hit, gg, g)
