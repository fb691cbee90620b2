"""numpy restatement of the rescaled LW no-scattering solver (rrx_lw_solver_noscat_rescaled), in the arrays' own
dtype. It is the yardstick of tests/test_gpu_lw_rescaled.py and is itself checked in tests/test_lw1r_ref.py.

Arrays follow hip_kernels.py: C-contiguous with reversed dimensions, tau(ncol, nlay, ngpt) <-> shape (ngpt, nlay, ncol); secants
(nmus, ngpt, ncol), weights (nmus). Layers and levels are in memory order; top_at_1 says which end is the top of the atmosphere."""
import math

import numpy as np

from lw2s_ref import broadband, combine, level_sources  # noqa: F401  (re-exported: the fused entry's inputs are formed the same way)


def layer_sources(pfrac, blay, gpoint_bands):
    """lay_source as rrx_planck_sources_from_fractions writes it: pfrac B_lay"""
    return pfrac * blay[np.asarray(gpoint_bands) - 1]


_libm_exp = np.frompyfunc(math.exp, 1, 1)


def exp(x):
    """exp in the array's dtype. float64: the C library's, element by element -- numpy's vector routine differs from it in the last
    bit here and there, and the thick branch of the source factor, (1 - tr)/tl - tr, multiplies that bit by up to 1/tau_thres = 8e3
    (against the CPU oracle, which calls the C library: 6.5e-13 of a flux with numpy's routine)"""
    return _libm_exp(x).astype(np.float64) if x.dtype == np.float64 else np.exp(x)


def layers(tau, ssa, g, D, lay_source, lev_top, lev_bot):
    """tr, sdn, sup, Cn of every layer for the secant D (ngpt, 1, ncol)"""
    dt = tau.dtype.type
    wb = ssa * (dt(1) - g) * dt(0.5)
    st = dt(1) - ssa + wb
    cn = dt(0.4) * wb / np.maximum(st, dt(3) * np.finfo(tau.dtype).tiny)
    tl = tau * D * st
    tr = exp(-tl)
    thres = np.sqrt(np.sqrt(np.finfo(tau.dtype).eps))
    with np.errstate(divide="ignore", invalid="ignore"):
        thick = (dt(1) - tr) / tl - tr
    fact = np.where(tl > thres, thick, tl * (dt(0.5) + tl * (dt(-1. / 3.) + tl * dt(1. / 8.))))
    sdn = (dt(1) - tr) * lev_bot + dt(2) * fact * (lay_source - lev_bot)
    sup = (dt(1) - tr) * lev_top + dt(2) * fact * (lay_source - lev_top)
    return tr, sdn, sup, cn


def solve(secants, weights, tau, ssa, g, lay_source, lev_source, sfc_emis, sfc_src, inc_flux=None, top_at_1=True, sfc_src_jac=None,
          rescale=True):
    """Per-g-point fluxes (flux_up, flux_dn[, flux_up_jac]), (ngpt, nlay+1, ncol) each, in memory order, summed over the angles.
    rescale=False: pass 1 and an unadjusted pass 2 on the optical depths as given (rrx_lw_solver_noscat)."""
    dt = tau.dtype.type
    if not top_at_1:
        tau, ssa, g, lay_source, lev_source = tau[:, ::-1], ssa[:, ::-1], g[:, ::-1], lay_source[:, ::-1], lev_source[:, ::-1]
    ngpt, nlay, ncol = tau.shape
    pi = dt(np.pi)
    shape = (ngpt, nlay + 1, ncol)
    flux_up = np.zeros(shape, dtype=tau.dtype); flux_dn = np.zeros(shape, dtype=tau.dtype); flux_jac = np.zeros(shape, dtype=tau.dtype)
    if not rescale:
        ssa = np.zeros_like(tau); g = np.zeros_like(tau)
    for imu in range(weights.shape[0]):
        tr, sdn, sup, cn = layers(tau, ssa, g, secants[imu][:, None, :], lay_source, lev_source[:, :-1], lev_source[:, 1:])
        an = dt(1) - tr * tr
        dn = np.empty(shape, dtype=tau.dtype); up = np.empty(shape, dtype=tau.dtype); jac = np.empty(shape, dtype=tau.dtype)
        dn[:, 0] = dt(0) if inc_flux is None else inc_flux / pi
        for i in range(nlay):                                   # pass 1
            dn[:, i + 1] = tr[:, i] * dn[:, i] + sdn[:, i]
        up[:, nlay] = dn[:, nlay] * (dt(1) - sfc_emis) + sfc_emis * sfc_src
        jac[:, nlay] = sfc_emis * (sfc_src_jac if sfc_src_jac is not None else dt(0))
        for i in range(nlay - 1, -1, -1):                       # pass 2
            up[:, i] = tr[:, i] * up[:, i + 1] + sup[:, i] + cn[:, i] * (an[:, i] * dn[:, i] - tr[:, i] * sdn[:, i] - sup[:, i])
            jac[:, i] = tr[:, i] * jac[:, i + 1]
        if rescale:
            for i in range(nlay):                               # pass 3
                dn[:, i + 1] = tr[:, i] * dn[:, i] + sdn[:, i] + cn[:, i] * (an[:, i] * up[:, i + 1] - tr[:, i] * sup[:, i] - sdn[:, i])
        scale = pi * weights[imu]
        flux_up += scale * up; flux_dn += scale * dn; flux_jac += scale * jac
    out = [flux_up, flux_dn] + ([flux_jac] if sfc_src_jac is not None else [])
    if not top_at_1:
        out = [a[:, ::-1] for a in out]
    return tuple(np.ascontiguousarray(a) for a in out)


def solve_fractions(secants, weights, tau_g, pfrac, blay, blev, gpoint_bands, cld, sfc_emis, sfc_src, inc_flux=None, top_at_1=True):
    """Broadband fluxes of rrx_lw_solver_noscat_fractions_rescaled, (nlay+1, ncol) each"""
    tau, ssa, g = combine(tau_g, cld, gpoint_bands)
    up, dn = solve(secants, weights, tau, ssa, g, layer_sources(pfrac, blay, gpoint_bands), level_sources(pfrac, blev, gpoint_bands),
                   sfc_emis, sfc_src, inc_flux, top_at_1)
    return broadband(up), broadband(dn)
