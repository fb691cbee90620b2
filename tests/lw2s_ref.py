"""numpy restatement of the LW two-stream solver with scattering (rrx_lw_solver_2stream), in the arrays' own dtype. It
is the yardstick of tests/test_gpu_lw_2stream.py and is itself checked by hand-written cases in tests/test_lw2s_ref.py.

Arrays follow hip_kernels.py: C-contiguous with reversed dimensions, tau(ncol, nlay, ngpt) <-> shape (ngpt, nlay, ncol). Layers and
levels are in memory order; top_at_1 says which end is the top of the atmosphere."""
import numpy as np

D = 1.66
TAU_THIN = 1e-8
K2_MIN = 1e-12


def two_stream(tau, ssa, g):
    """Rdif, Tdif, gamma1 + gamma2 of a layer (lw_two_stream)"""
    dt = tau.dtype.type
    gamma1 = dt(D) * (dt(1) - dt(0.5) * ssa * (dt(1) + g))
    gamma2 = dt(D) * dt(0.5) * ssa * (dt(1) - g)
    k = np.sqrt(np.maximum((gamma1 - gamma2) * (gamma1 + gamma2), dt(K2_MIN)))
    e1 = np.exp(-tau * k)
    e2 = e1 * e1
    rt = dt(1) / (k * (dt(1) + e2) + gamma1 * (dt(1) - e2))
    return rt * gamma2 * (dt(1) - e2), rt * dt(2) * k * e1, gamma1 + gamma2


def sources(tau, gsum, rdif, tdif, lev_top, lev_bot):
    """src_up, src_dn of a layer (lw_source_2str); both 0 where tau <= 1e-8"""
    dt = tau.dtype.type
    thick = tau > dt(TAU_THIN)
    z = (lev_bot - lev_top) / np.where(thick, tau * gsum, dt(1))
    pi = dt(np.pi)
    up = pi * ((z + lev_top) - rdif * (-z + lev_top) - tdif * (z + lev_bot))
    dn = pi * ((-z + lev_bot) - rdif * (z + lev_bot) - tdif * (-z + lev_top))
    return np.where(thick, up, dt(0)), np.where(thick, dn, dt(0))


def solve(tau, ssa, g, lev_source, sfc_emis, sfc_src, inc_flux=None, top_at_1=True):
    """Per-g-point fluxes (flux_up, flux_dn), (ngpt, nlay+1, ncol) each, in memory order"""
    dt = tau.dtype.type
    if not top_at_1:
        tau, ssa, g, lev_source = tau[:, ::-1], ssa[:, ::-1], g[:, ::-1], lev_source[:, ::-1]
    ngpt, nlay, ncol = tau.shape
    rdif, tdif, gsum = two_stream(tau, ssa, g)
    s_up, s_dn = sources(tau, gsum, rdif, tdif, lev_source[:, :-1], lev_source[:, 1:])
    alb = np.empty((ngpt, nlay + 1, ncol), dtype=tau.dtype); src = np.empty_like(alb); den = np.empty_like(tau)
    alb[:, nlay] = dt(1) - sfc_emis
    src[:, nlay] = dt(np.pi) * sfc_emis * sfc_src
    for s in range(nlay - 1, -1, -1):                        # the SW solver's adding recurrences, diffuse part
        den[:, s] = dt(1) / (dt(1) - rdif[:, s] * alb[:, s + 1])
        src[:, s] = s_up[:, s] + tdif[:, s] * den[:, s] * (src[:, s + 1] + alb[:, s + 1] * s_dn[:, s])
        alb[:, s] = rdif[:, s] + tdif[:, s] * tdif[:, s] * alb[:, s + 1] * den[:, s]
    up = np.empty_like(alb); dn = np.empty_like(alb)
    dn[:, 0] = dt(0) if inc_flux is None else inc_flux
    up[:, 0] = dn[:, 0] * alb[:, 0] + src[:, 0]
    for s in range(nlay):
        dn[:, s + 1] = (tdif[:, s] * dn[:, s] + rdif[:, s] * src[:, s + 1] + s_dn[:, s]) * den[:, s]
        up[:, s + 1] = dn[:, s + 1] * alb[:, s + 1] + src[:, s + 1]
    if not top_at_1:
        up, dn = up[:, ::-1], dn[:, ::-1]
    return np.ascontiguousarray(up), np.ascontiguousarray(dn)


def broadband(gpt):
    """g-point sum in g-point order, in the array's dtype (rrx_sum_broadband's order)"""
    out = np.zeros(gpt.shape[1:], dtype=gpt.dtype)
    for ig in range(gpt.shape[0]):
        out += gpt[ig]
    return out


def level_sources(pfrac, blev, gpoint_bands):
    """lev_source as rrx_planck_sources_from_fractions writes it: sqrt(pfrac pfrac') B_lev, first / last level pfrac B_lev"""
    ngpt, nlay, ncol = pfrac.shape
    b = blev[np.asarray(gpoint_bands) - 1]
    out = np.empty((ngpt, nlay + 1, ncol), dtype=pfrac.dtype)
    out[:, 0] = pfrac[:, 0] * b[:, 0]
    out[:, nlay] = pfrac[:, nlay - 1] * b[:, nlay]
    out[:, 1:nlay] = np.sqrt(pfrac[:, 1:] * pfrac[:, :-1]) * b[:, 1:nlay]
    return out


def combine(tau_g, cld, gpoint_bands):
    """gas (tau_g, 0, 0) + band cloud (tau_c, ssa_c, g_c): the arithmetic of rrx_inc_2stream_by_2stream_bybnd. cld None: ssa = g = 0"""
    dt = tau_g.dtype.type
    if cld is None:
        return tau_g, np.zeros_like(tau_g), np.zeros_like(tau_g)
    ib = np.asarray(gpoint_bands) - 1
    tc, wc, gc = (np.asarray(a)[ib] for a in cld)
    eps = np.finfo(tau_g.dtype).tiny * dt(3)
    tau = tau_g + tc
    scat = tc * wc
    return tau, scat / np.maximum(eps, tau), (scat * gc) / np.maximum(scat, eps)


def solve_fractions(tau_g, pfrac, blev, gpoint_bands, cld, sfc_emis, sfc_src, inc_flux=None, top_at_1=True):
    """Broadband fluxes of rrx_lw_solver_2stream_fractions, (nlay+1, ncol) each"""
    tau, ssa, g = combine(tau_g, cld, gpoint_bands)
    up, dn = solve(tau, ssa, g, level_sources(pfrac, blev, gpoint_bands), sfc_emis, sfc_src, inc_flux, top_at_1)
    return broadband(up), broadband(dn)
