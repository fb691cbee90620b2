"""Launcher-level orchestration of one LW / SW solve, generic over a backend object.

Mirrors, call for call, what the reference's host classes do around the kernel launchers:
  Radiation_solver_longwave::solve_gpu   /root/reference/src_test/Radiation_solver.cu:419-680
  Radiation_solver_shortwave::solve_gpu  /root/reference/src_test/Radiation_solver.cu:683-950
  Gas_optics_rrtmgp_gpu::gas_optics / compute_gas_taus / source   /root/reference/src_cuda/Gas_optics_rrtmgp.cu:907-1201
  Rte_lw_gpu::rte_lw                     /root/reference/src_cuda/Rte_lw.cu:60-136
  Rte_sw_gpu::rte_sw                     /root/reference/src_cuda/Rte_sw.cu:116-161
  Fluxes_broadband_gpu::reduce           /root/reference/src_cuda/Fluxes.cu:39-54

The backend is either HipKernels (product path, torch CUDA tensors) or, in tests only, a CPU checker from
oracle/oracle_py.py (numpy). This module never imports the oracle.
"""
import contextlib
import os
import time

import numpy as np

# Gauss-Jacobi-5 quadrature, R. J. Hogan 2023 (values as in /root/reference/src/Rte_lw.cpp:140-152); (n_angles, point)
MAX_GAUSS_PTS = 4
GAUSS_DS = np.array([
    [1./0.6096748751, 0., 0., 0.],
    [1./0.2509907356, 1/0.7908473988, 0., 0.],
    [1./0.1024922169, 1/0.4417960320, 1./0.8633751621, 0.],
    [1./0.0454586727, 1/0.2322334416, 1./0.5740198775, 1./0.903077597]])
GAUSS_WTS = np.array([
    [1., 0., 0., 0.],
    [0.2300253764, 0.7699746236, 0., 0.],
    [0.0437820218, 0.3875796738, 0.5686383044, 0.],
    [0.0092068785, 0.1285704278, 0.4323381850, 0.4298845087]])


def upload_atmosphere(be, atm):
    from .synthetic import Atmosphere
    out = {}
    for k, v in atm.__dict__.items():
        if isinstance(v, np.ndarray):
            out[k] = be.asarray(v)
        elif isinstance(v, dict):
            out[k] = {n: be.asarray(a) for n, a in v.items()}
        else:
            out[k] = v
    return Atmosphere(**out)


def _sfc_lay(atm):
    # /root/reference/src_cuda/Gas_optics_rrtmgp.cu:1190 : play(1,1) > play(1,nlay) ? 1 : nlay
    return atm.nlay if atm.top_at_1 else 1


def gas_state(be, kd, atm, col_dry=None, interpolate=True):
    """col_dry, col_gas and the interpolation state shared by the optical-depth and source kernels. interpolate=False:
    the consumers compute the interpolation state themselves (the "direct" entry points), nothing is materialised."""
    if col_dry is None:
        col_dry = be.get_col_dry(atm.vmr["h2o"], atm.p_lev)
    col_gas = be.fill_gases(kd, atm.vmr, col_dry)
    it = be.interpolation(kd, atm.p_lay, atm.t_lay, col_gas) if interpolate else None
    return col_dry, col_gas, it


def _use_direct(be, direct):
    return hasattr(be, "gas_optics_lw_direct") if direct is None else bool(direct)


def solve_lw(be, kd, atm, col_dry=None, cloud_lut=None, n_gauss_angles=1, do_broadband=False, keep=False, direct=None, lite=None,
             fuse_clouds=True):
    """lite (default: broadband mode with one angle on a backend that has it): Planck fractions + band Planck functions, the
    sources are formed inside the broadband solver (the "Planck-lite" chain); keep=True materialises them for the caller."""
    ncol, nlay, ngpt = atm.ncol, atm.nlay, kd.ngpt
    direct = _use_direct(be, direct)
    if lite is None:
        lite = direct and do_broadband and n_gauss_angles == 1 and hasattr(be, "planck_fractions")
    col_dry, col_gas, it = gas_state(be, kd, atm, col_dry, interpolate=not direct)

    fr = None
    # all-sky on the direct path: the by-band cloud optical depth is added where tau is stored (one pass less over the g-point array)
    tau_cld = be.cloud_optics_1scl(cloud_lut, atm.lwp, atm.iwp, atm.rel, atm.dei) if cloud_lut is not None else None
    fused = tau_cld if (direct and fuse_clouds) else None
    if direct:          # product default: interpolation recomputed inside the two consumers, no intermediate arrays
        if lite:        # tau and the Planck-lite outputs in one pass over the cells
            tau = be.empty((ngpt, nlay, ncol))
            fr = be.gas_optics_lw_fractions(kd, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, _sfc_lay(atm), col_gas, tau, by_band=fused)
            src = dict(sfc_src=fr["sfc_src"], sfc_src_jac=fr["sfc_src_jac"], lay_src=None, lev_src=None)
            if keep:
                src["lay_src"], src["lev_src"] = be.planck_sources_from_fractions(kd, fr)
        else:
            tau = be.gas_optics_lw_direct(kd, atm.p_lay, atm.t_lay, col_gas, be.empty((ngpt, nlay, ncol)), by_band=fused)
            src = be.planck_source_direct(kd, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, _sfc_lay(atm), col_gas)
    else:
        if hasattr(be, "compute_tau_absorption_set"):
            tau = be.compute_tau_absorption_set(kd, it, atm.p_lay, atm.t_lay, col_gas, be.empty((ngpt, nlay, ncol)))
        else:
            tau = be.zeros((ngpt, nlay, ncol))
            be.compute_tau_absorption(kd, it, atm.p_lay, atm.t_lay, col_gas, tau)
        src = be.compute_planck_source(kd, it, atm.t_lay, atm.t_lev, atm.t_sfc, _sfc_lay(atm))

    if tau_cld is not None and fused is None:
        be.inc_1scalar_by_1scalar_bybnd(tau, tau_cld, kd.band_lims_gpt)

    sfc_emis_gpt = be.expand_and_transpose(kd.band_lims_gpt, atm.emis_sfc, ngpt)
    gauss_Ds = be.asarray(GAUSS_DS)
    weights = be.asarray(np.ascontiguousarray(GAUSS_WTS[n_gauss_angles-1, :n_gauss_angles]))
    secants = be.lw_secants_array(ncol, ngpt, n_gauss_angles, MAX_GAUSS_PTS, gauss_Ds)

    if fr is not None:
        r = be.lw_solver_noscat_fractions(atm.top_at_1, kd, secants, weights, tau, fr, sfc_emis_gpt)
    else:
        r = be.lw_solver_noscat(atm.top_at_1, secants, weights, tau, src["lay_src"], src["lev_src"],
                                sfc_emis_gpt, src["sfc_src"], None, do_broadband=do_broadband)
    if do_broadband:
        flux_up, flux_dn = r["flux_up"], r["flux_dn"]
    else:
        flux_up = be.sum_broadband(r["flux_up"])
        flux_dn = be.sum_broadband(r["flux_dn"])
    flux_net = be.net_broadband_precalc(flux_dn, flux_up)
    out = dict(flux_up=flux_up, flux_dn=flux_dn, flux_net=flux_net)
    if keep:
        out.update(tau=tau, lay_src=src["lay_src"], lev_src=src["lev_src"], sfc_src=src["sfc_src"],
                   gpt_flux_up=r.get("flux_up"), gpt_flux_dn=r.get("flux_dn"), interp=it, col_gas=col_gas)
    return out


def solve_sw(be, kd, atm, col_dry=None, cloud_lut=None, delta_cloud=False, do_broadband=False, fused_gas=None, keep=False, direct=None,
             aerosol_lut=None, delta_aerosol=False, fuse_clouds=True):
    ncol, nlay, ngpt = atm.ncol, atm.nlay, kd.ngpt
    if fused_gas is None:
        fused_gas = hasattr(be, "gas_optics_sw_fused")
    direct = bool(fused_gas) and _use_direct(be, direct)
    col_dry, col_gas, it = gas_state(be, kd, atm, col_dry, interpolate=not direct)

    # clear sky: the asymmetry parameter of the gas optics is identically zero; the HIP entry points take "no g array"
    # natively (nothing written by the gas optics, nothing read by the solver)
    g_zero = bool(fused_gas and cloud_lut is None and aerosol_lut is None and getattr(be, "supports_null_g", False))
    cld = None
    if cloud_lut is not None:
        cld = be.cloud_optics_2str(cloud_lut, atm.lwp, atm.iwp, atm.rel, atm.dei)
        if delta_cloud:
            be.delta_scale_2str_k(*cld)
    fused = cld if (direct and fuse_clouds) else None          # added where the gas optics is stored
    if fused_gas:
        tau = be.empty((ngpt, nlay, ncol)); ssa = be.empty((ngpt, nlay, ncol))
        g = None if g_zero else be.empty((ngpt, nlay, ncol))
        if direct:
            be.gas_optics_sw_direct(kd, atm.p_lay, atm.t_lay, col_gas, col_dry, tau, ssa, g, by_band=fused)
        else:
            be.gas_optics_sw_fused(kd, it, atm.p_lay, atm.t_lay, col_gas, col_dry, tau, ssa, g)
    else:
        tau_abs = be.zeros((ngpt, nlay, ncol))
        be.compute_tau_absorption(kd, it, atm.p_lay, atm.t_lay, col_gas, tau_abs)
        tau_ray = be.compute_tau_rayleigh(kd, it, col_dry, col_gas)
        tau, ssa, g = be.combine_abs_and_rayleigh(tau_abs, tau_ray)

    toa_src = be.spread_col(ncol, kd.solar_source)
    be.scaling_to_subset(toa_src, atm.tsi_scaling)

    if cld is not None and fused is None:
        be.inc_2stream_by_2stream_bybnd(tau, ssa, g, *cld, kd.band_lims_gpt)

    if aerosol_lut is not None:
        # /root/reference/src_test/Radiation_solver.cu:794-809
        ta, wa, ga = be.aerosol_optics(aerosol_lut, [atm.aermr["aermr%02d" % i] for i in range(1, 12)], atm.rh, atm.p_lev)
        if delta_aerosol:
            be.delta_scale_2str_k(ta, wa, ga)
        be.inc_2stream_by_2stream_bybnd(tau, ssa, g, ta, wa, ga, kd.band_lims_gpt)

    alb_dir = be.expand_and_transpose(kd.band_lims_gpt, atm.sfc_alb_dir, ngpt)
    alb_dif = be.expand_and_transpose(kd.band_lims_gpt, atm.sfc_alb_dif, ngpt)

    r = be.sw_solver_2stream(atm.top_at_1, tau, ssa, g, atm.mu0, alb_dir, alb_dif, toa_src, None, do_broadband=do_broadband)
    if do_broadband:
        flux_up, flux_dn, flux_dir = r["flux_up"], r["flux_dn"], r["flux_dir"]
    else:
        flux_up = be.sum_broadband(r["flux_up"])
        flux_dn = be.sum_broadband(r["flux_dn"])
        flux_dir = be.sum_broadband(r["flux_dir"])
    flux_net = be.net_broadband_precalc(flux_dn, flux_up)
    out = dict(flux_up=flux_up, flux_dn=flux_dn, flux_dn_dir=flux_dir, flux_net=flux_net)
    if keep:
        out.update(tau=tau, ssa=ssa, g=be.zeros((ngpt, nlay, ncol)) if g is None else g, toa_src=toa_src, gpt_flux_up=r.get("flux_up"),
                   gpt_flux_dn=r.get("flux_dn"), gpt_flux_dir=r.get("flux_dir"))
    return out


def spectral_allocation(inc, P, min_per_gpt=1):
    """m (ngpt,) int64, photons per pixel of every g-point: P dealt over the active g-points (inc > 0) in proportion to inc by
    largest remainders on the shares inc_g / sum(inc) in float64, ties to the lower g. Every active g-point gets at least min_per_gpt
    (no g-point with flux is left out: the estimator stays unbiased), an inactive one 0. Raises when P < min_per_gpt x the number of
    active g-points."""
    inc = np.asarray(inc, dtype=np.float64).reshape(-1)
    P, floor = int(P), int(min_per_gpt)
    if np.any(inc < 0) or not np.all(np.isfinite(inc)):
        raise ValueError("spectral_allocation: inc must be finite and >= 0")
    if floor < 0:
        raise ValueError("spectral_allocation: min_per_gpt must be >= 0")
    active = inc > 0
    n_active = int(active.sum())
    if P < floor*n_active or (P > 0 and n_active == 0) or P < 0:
        raise ValueError(f"spectral_allocation: P = {P} photons per pixel cannot give {floor} to each of {n_active} active g-points")
    m = np.where(active, floor, 0).astype(np.int64)
    free = active.copy()                                   # the g-points that the floor does not bind
    # the floor binds a g-point whose proportional share of what the others leave is below it: take those out, deal the rest again
    while True:
        rest = P - int(m[~free].sum())
        total = float(inc[free].sum())
        if not free.any() or total <= 0.0:
            break
        quota = np.where(free, rest * (inc / total), 0.0)
        bound = free & (quota < floor)
        if not bound.any():
            break
        free &= ~bound
    if free.any():
        rest = P - int(m[~free].sum())
        quota = np.where(free, rest * (inc / float(inc[free].sum())), 0.0)
        base = np.floor(quota).astype(np.int64)
        m = np.where(free, base, m)
        left = rest - int(base[free].sum())
        remainder = np.where(free, quota - base, -1.0)
        order = np.argsort(-remainder, kind="stable")      # (stable: ties go to the lower g)
        m[order[:left]] += 1
    # (the floor never binds everywhere: the shares of the free g-points add up to what is left, which is at least their floors)
    assert int(m.sum()) == P and np.all(m[active] >= floor) and not m[~active].any()
    return m


def spectral_photon_list(inc_dir, inc_dif, m, ncol, dtype):
    """What rrx_raytracer_sw_spectral forms from m (ngpt,) photons per pixel, in the precision dtype: photon_end (ngpt+1,) int64,
    weight0, dif_frac (ngpt,) and the common unit U = S / P (flux = counts 2^-32 U). weight0[g] = (inc_g / F(m_g)) / (S / F(P)),
    S the sum of inc_g = inc_dir[g] + inc_dif[g] over the g-points with m_g > 0 in index order, P = sum(m)."""
    dt = np.dtype(dtype)
    F = dt.type
    m = np.asarray(m, dtype=np.int64).reshape(-1)
    inc_dir, inc_dif = np.asarray(inc_dir, dtype=dt).reshape(-1), np.asarray(inc_dif, dtype=dt).reshape(-1)
    if np.any(m < 0):
        raise ValueError("spectral_photon_list: photons_per_pixel_gpt is negative")
    photon_end = np.concatenate([[0], np.cumsum(m * int(ncol))]).astype(np.int64)
    P, S = int(m.sum()), F(0.)
    for g in range(m.size):
        if m[g] > 0:
            if not inc_dir[g] + inc_dif[g] > 0:
                raise ValueError(f"spectral_photon_list: g-point {g} has photons and no incident flux")
            S = F(S + F(inc_dir[g] + inc_dif[g]))
    U = F(S / F(P)) if P > 0 else F(0.)
    weight0, dif_frac = np.zeros(m.size, dtype=dt), np.zeros(m.size, dtype=dt)
    for g in range(m.size):
        if m[g] > 0:
            inc = F(inc_dir[g] + inc_dif[g])
            weight0[g] = F(F(inc / F(m[g])) / U)
            dif_frac[g] = F(inc_dif[g] / inc)
    return photon_end, weight0, dif_frac, U


def raytrace_sw(be, kd_sw, atm, nx, ny, dx, dy, dz, azimuth, photons_per_pixel, seed, cloud_lut=None, kn_grid=None,
                independent_column=False, sfc_albedo=None, max_events=None, phase_table=None, n_domain=None, z_lev=None,
                aerosol_lut=None, allocation=None, min_per_gpt=1):
    """3-D shortwave surface / top fluxes and absorption from the forward Monte Carlo ray tracer (rrx_raytracer_sw).

    The atmosphere's columns are the pixels of an nx x ny domain (column = ix + nx iy) of cells dx x dy x dz metres, periodic in x
    and y, under one sun: mu0 and tsi_scaling must be the same in every column. The clear per-g-point SW gas optics and (with
    cloud_lut) the band cloud optics, not delta-scaled, feed the tracer; inc_dir[g] = solar_source[g] tsi_scaling mu0, no diffuse
    incident flux. azimuth: direction of travel of the direct beam, radians from +x. kn_grid = (knx, kny, knz) dividing (nx, ny,
    nlay), default one block per cell. sfc_albedo (ncol,): default the atmosphere's, which must then be the same in every band and
    for direct and diffuse light (the tracer's surface is Lambertian with one broadband albedo per pixel).
    phase_table (phase_tables.PhaseTable, needs cloud_lut): cloud scatters by the tabulated phase function of the liquid radius
    atm.rel in place of Henyey-Greenstein.
    n_domain < atm.nlay with z_lev (nlay+1,), the heights of the atmosphere's levels in metres in array order: the
    lowest n_domain layers are the grid (of thickness dz) and the layers above are a horizontally uniform background up to TOA, taken
    from column 0, with the thicknesses of z_lev; kn_grid then divides (nx, ny, n_domain) and inc_dir is incident at TOA.
    aerosol_lut: the chain's band aerosol optics be.aerosol_optics(aerosol_lut, aermr01..11, rh, p_lev), not
    delta-scaled (as the cloud is not), are a third scattering species of the tracer (rrx_raytracer_sw_aer), Henyey-Greenstein with
    its own asymmetry parameter; with n_domain the layers above the grid carry column 0's aerosol.
    Returns sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up (ncol,) in W m-2, abs_dir, abs_dif (nlay, ncol) in W m-3 and n_capped; with
    n_domain also toa_up, tod_dn_dir, tod_dn_dif (ncol,) in W m-2 and bg_abs_dir, bg_abs_dif (nbg,) in W m-3 of a domain-wide layer,
    counted upward from the domain top (abs_dir, abs_dif are then (n_domain, ncol), and tod_up is the flux through the domain top).
    allocation="flux" (DESIGN 4.19): photons_per_pixel is the TOTAL over all g-points, dealt by spectral_allocation(inc_dir,
    photons_per_pixel, min_per_gpt) in proportion to the incident flux, and all g-points are traced in one launch per chunk
    (rrx_raytracer_sw_spectral, ngpt <= 1024). The same dictionary comes back. allocation=None: every g-point gets photons_per_pixel."""
    if allocation not in (None, "flux"):
        raise ValueError(f"raytrace_sw: allocation is None or 'flux', got {allocation!r}")
    if n_domain is not None and kn_grid is None:
        kn_grid = (nx, ny, int(n_domain))
    tau, ssa, cld, sfc_albedo, mu0, inc_dir, kn_grid, aer = _raytracer_inputs("raytrace_sw", be, kd_sw, atm, nx, ny, cloud_lut, kn_grid,
                                                                              sfc_albedo, aerosol_lut)
    m = spectral_allocation(inc_dir, photons_per_pixel, min_per_gpt) if allocation == "flux" else None
    tau, ssa, cld, phase, medium = _raytracer_medium("raytrace_sw", be, atm, tau, ssa, cld, aer, cloud_lut, phase_table, n_domain, z_lev)
    scene = (tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, np.zeros_like(inc_dir), kn_grid)
    kw = dict(top_at_1=atm.top_at_1, independent_column=independent_column, cloud=cld, band_lims=kd_sw.band_lims_gpt, max_events=max_events,
              phase=phase)
    if allocation == "flux":
        r = be.raytracer_sw_spectral(*scene, m, seed, **kw, background=medium.get("background"), aerosol=medium.get("aerosol"))
    elif medium:
        r = be.raytracer_sw_bg(*scene, photons_per_pixel, seed, **kw, **medium)
    else:
        r = be.raytracer_sw(*scene, photons_per_pixel, seed, **kw)
    return r if n_domain is not None else {k: v for k, v in r.items() if k not in be.RT_BG_COUNTS}


def render_sw(be, kd_sw, atm, nx, ny, dx, dy, dz, azimuth, camera, rays_per_pixel, seed, cloud_lut=None, kn_grid=None,
              sfc_albedo=None, max_events=None, phase_table=None, n_domain=None, z_lev=None, aerosol_lut=None, allocation=None,
              min_per_gpt=1, channels=None):
    """Shortwave radiances for a virtual camera or a flux sensor from the backward Monte Carlo ray tracer (rrx_raytracer_bw, DESIGN
    4.15): the twin of raytrace_sw, on the same domain, sun, optics and albedo, with the same checks. camera: camera.perspective /
    fisheye / orthographic / flux_sensor. Returns radiance (npy, npx) in W m-2 sr-1 (scattered and reflected sunlight; the sun's
    disk is not imaged), n_capped and n_clamped. phase_table, n_domain, z_lev, aerosol_lut: as in raytrace_sw; with a background the camera may
    sit inside it, and the orthographic and the downward flux sensor start at clamp(position.z, domain top, TOA).
    allocation="flux" (DESIGN 4.21): rays_per_pixel is the TOTAL over all g-points, dealt by spectral_allocation(inc_dir,
    rays_per_pixel, min_per_gpt) in proportion to the incident flux; the rays of all g-points are traced in one launch per chunk and
    tallied by band (rrx_camera_render_spectral, ngpt <= 1024). channels then says what the sensor sees: None, broadband radiance
    (npy, npx) as without allocation; "bands", radiance by band (nbnd, npy, npx); an array (nchan, nbnd), such as
    camera.band_weights gives, (nchan, npy, npx). allocation=None: every g-point gets rays_per_pixel, broadband only."""
    if allocation not in (None, "flux"):
        raise ValueError(f"render_sw: allocation is None or 'flux', got {allocation!r}")
    if allocation is None and channels is not None:
        raise ValueError("render_sw: channels needs allocation='flux' (the per-g-point loop tallies broadband only)")
    if n_domain is not None and kn_grid is None:
        kn_grid = (nx, ny, int(n_domain))
    tau, ssa, cld, sfc_albedo, mu0, inc_dir, kn_grid, aer = _raytracer_inputs("render_sw", be, kd_sw, atm, nx, ny, cloud_lut, kn_grid,
                                                                              sfc_albedo, aerosol_lut)
    if allocation == "flux":
        nbnd = int(kd_sw.band_lims_gpt.shape[0])
        if channels is None:
            M = np.ones((1, nbnd))
        elif isinstance(channels, str):
            if channels != "bands":
                raise ValueError(f"render_sw: channels is None, 'bands' or an array (nchan, nbnd), got {channels!r}")
            M = np.eye(nbnd)
        else:
            M = np.asarray(channels, dtype=np.float64)
            if M.ndim != 2 or M.shape[1] != nbnd:
                raise ValueError(f"render_sw: channels is (nchan, nbnd = {nbnd}), got {M.shape}")
        m = spectral_allocation(inc_dir, rays_per_pixel, min_per_gpt)
    tau, ssa, cld, phase, medium = _raytracer_medium("render_sw", be, atm, tau, ssa, cld, aer, cloud_lut, phase_table, n_domain, z_lev)
    scene = (tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, kn_grid, camera)
    kw = dict(top_at_1=atm.top_at_1, cloud=cld, max_events=max_events, phase=phase)
    if allocation == "flux":
        r = be.camera_render_spectral(*scene, m, seed, kd_sw.band_lims_gpt, M, **kw, background=medium.get("background"),
                                      aerosol=medium.get("aerosol"))
        if channels is None:
            r["radiance"] = r["radiance"][0]
        return r
    if medium:
        return be.raytracer_bw_bg(*scene, rays_per_pixel, seed, band_lims=kd_sw.band_lims_gpt, **kw, **medium)
    return be.raytracer_bw(*scene, rays_per_pixel, seed, band_lims=kd_sw.band_lims_gpt, **kw)


def emission_allocation(e, lay_max, top_radiance, P, min_per_gpt=1):
    """render_lw(allocation="emission"): m (ngpt,) int64 = spectral_allocation(e, P, min_per_gpt) with e_g the surface emission of
    g-point g summed over the columns. A g-point with e_g = 0 gets no rays and is left out of the result, so it is refused when its
    largest lay_src, lay_max[g], or its top_radiance[g] (None: 0) is positive: the result would be biased."""
    e = np.asarray(e, dtype=np.float64).reshape(-1)
    lay_max = np.asarray(lay_max, dtype=np.float64).reshape(-1)
    top = np.zeros(e.size) if top_radiance is None else np.asarray(top_radiance, dtype=np.float64).reshape(-1)
    if lay_max.size != e.size or top.size != e.size:
        raise ValueError(f"render_lw: lay_src and top_radiance are per g-point (ngpt = {e.size}), got {lay_max.size}, {top.size}")
    bad = np.flatnonzero((e == 0) & ((lay_max > 0) | (top > 0)))
    if bad.size:
        raise ValueError(f"render_lw: g-point {int(bad[0])} has no surface emission, so allocation='emission' gives it no rays, but its "
                         "lay_src or top_radiance is positive: it would be left out of the result")
    return spectral_allocation(e, P, min_per_gpt)


def render_lw(be, kd_lw, atm, nx, ny, dx, dy, dz, camera, rays_per_pixel, seed, cloud_lut=None, kn_grid=None, sfc_emis=None,
              max_events=None, channels=None, top_radiance=None, allocation=None, min_per_gpt=1):
    """Longwave radiances for a virtual camera or a flux sensor from the backward Monte Carlo ray tracer with thermal emission
    (rrx_thermal_render): the twin of render_sw on the LW chain's own arrays: the clear g-point tau of
    gas_optics_lw_direct (the gas does not scatter), the Planck sources of planck_source_direct (lay_src, constant within a cell, and
    sfc_src) and, with cloud_lut (the LW table), the band cloud triple of cloud_optics_2str. sfc_emis: (ncol,), one broadband
    emissivity per pixel; None takes atm.emis_sfc, which must then be the same in every band. top_radiance: None (0) or (ngpt,), the
    isotropic downward radiance at the domain top per g-point, which closes the medium when the grid does not reach TOA. channels:
    None, broadband radiance (npy, npx); "bands", radiance by band (nbnd, npy, npx); an array (nchan, nbnd), applied to the band
    radiances, (nchan, npy, npx). Returns radiance in W m-2 sr-1, n_capped and n_clamped. With a camera.flux_sensor pi x radiance is
    the irradiance of the pixel in W m-2 (pi x the mean radiance over the hemisphere): the surface downwelling (facing up) or the
    outgoing longwave at the domain top (facing down). Every g-point gets rays_per_pixel rays.
    allocation="emission" (DESIGN 4.24): rays_per_pixel is the TOTAL over all g-points, dealt by spectral_allocation(e, rays_per_pixel,
    min_per_gpt) in proportion to e_g, the sum over the columns of sfc_src[g] (taken on the host in float64); the rays of all g-points
    are traced in one launch per chunk and tallied by band (rrx_thermal_render_spectral, ngpt <= 1024), and channels becomes the
    matrix of that one call. The same dictionary comes back. A g-point with e_g = 0 gets no rays and is left out: it is refused
    when its lay_src or top_radiance is positive (Planck sources never are where the surface's is 0)."""
    if allocation not in (None, "emission"):
        raise ValueError(f"render_lw: allocation is None or 'emission', got {allocation!r}")
    ncol, nlay, ngpt = atm.ncol, atm.nlay, kd_lw.ngpt
    if ncol != nx*ny:
        raise ValueError(f"render_lw: ncol = {ncol} is not nx ny = {nx}*{ny}")
    nbnd = int(kd_lw.band_lims_gpt.shape[0])
    M = None
    if isinstance(channels, str):
        if channels != "bands":
            raise ValueError(f"render_lw: channels is None, 'bands' or an array (nchan, nbnd), got {channels!r}")
    elif channels is not None:
        M = np.asarray(channels, dtype=be.np_dtype)
        if M.ndim != 2 or M.shape[1] != nbnd:
            raise ValueError(f"render_lw: channels is (nchan, nbnd = {nbnd}), got {M.shape}")
    if sfc_emis is None:
        emis = be.to_numpy(atm.emis_sfc)
        if np.any(emis != emis[:, :1]):
            raise ValueError("render_lw: the atmosphere's emissivity differs between bands; pass sfc_emis")
        sfc_emis = np.ascontiguousarray(emis[:, 0])
    sfc_emis = be.asarray(sfc_emis)
    kn_grid = (nx, ny, nlay) if kn_grid is None else tuple(int(k) for k in kn_grid)

    _, col_gas, _ = gas_state(be, kd_lw, atm, None, interpolate=False)
    tau = be.gas_optics_lw_direct(kd_lw, atm.p_lay, atm.t_lay, col_gas, be.empty((ngpt, nlay, ncol)))
    src = be.planck_source_direct(kd_lw, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, _sfc_lay(atm), col_gas)
    cld = be.cloud_optics_2str(cloud_lut, atm.lwp, atm.iwp, atm.rel, atm.dei) if cloud_lut is not None else None
    if allocation == "emission":
        e = be.to_numpy(src["sfc_src"]).astype(np.float64).sum(axis=1)
        lay_max = be.to_numpy(src["lay_src"].reshape(ngpt, -1).max(dim=1).values) if np.any(e == 0) else np.zeros(ngpt)
        m = emission_allocation(e, lay_max, top_radiance, rays_per_pixel, min_per_gpt)
        matrix = np.ones((1, nbnd)) if channels is None else np.eye(nbnd) if M is None else M
        r = be.thermal_render_spectral(tau, None, nx, ny, dx, dy, dz, sfc_emis, src["lay_src"], src["sfc_src"], kn_grid, camera, m, seed,
                                       kd_lw.band_lims_gpt, matrix, top_at_1=atm.top_at_1, cloud=cld, max_events=max_events,
                                       top_radiance=top_radiance)
        if channels is None:
            r["radiance"] = r["radiance"][0]
        return r
    r = be.thermal_render(tau, None, nx, ny, dx, dy, dz, sfc_emis, src["lay_src"], src["sfc_src"], kn_grid, camera, rays_per_pixel, seed,
                          top_at_1=atm.top_at_1, cloud=cld, band_lims=kd_lw.band_lims_gpt, max_events=max_events,
                          top_radiance=top_radiance, by_band=channels is not None)
    if M is not None:
        band = r["radiance"]
        r["radiance"] = (be.asarray(M) @ band.reshape(nbnd, -1)).reshape(M.shape[0], *band.shape[1:])
    return r


def absorbed_emission(tau, lay_src, band_lims, cld):
    """heating_lw(allocation="emission"): e (ngpt,) float64 on the host, e_g = sum over the cells of tau_abs lay_src[g] with
    tau_abs = tau + cld_tau (1 - cld_ssa) of the g-point's band (the gas does not scatter): the power that the atmosphere emits in g
    per unit horizontal area, up to 4 pi / ncol. Formed on the device in float64; ngpt numbers are copied."""
    tau_abs = tau.double()
    if cld is not None:
        tau_abs = tau_abs.clone()
        lims = band_lims.cpu().numpy()
        for b in range(lims.shape[0]):
            tau_abs[int(lims[b, 0]) - 1:int(lims[b, 1])] += (cld[0][b].double()*(1.0 - cld[1][b].double()))[None]
    return (tau_abs*lay_src.double()).flatten(1).sum(dim=1).cpu().numpy()


def heating_allocation(e, sfc_max, top_radiance, P, min_per_gpt=1):
    """heating_lw(allocation="emission"): m (ngpt,) int64 = spectral_allocation(e, P, min_per_gpt) with e_g the power that the
    atmosphere emits in g-point g (absorbed_emission). A g-point with e_g = 0 gets no rays and is left out of the result, so it is
    refused when its largest sfc_src, sfc_max[g], or its top_radiance[g] (None: 0) is positive: the result would be biased."""
    e = np.asarray(e, dtype=np.float64).reshape(-1)
    sfc_max = np.asarray(sfc_max, dtype=np.float64).reshape(-1)
    top = np.zeros(e.size) if top_radiance is None else np.asarray(top_radiance, dtype=np.float64).reshape(-1)
    if sfc_max.size != e.size or top.size != e.size:
        raise ValueError(f"heating_lw: sfc_src and top_radiance are per g-point (ngpt = {e.size}), got {sfc_max.size}, {top.size}")
    bad = np.flatnonzero((e == 0) & ((sfc_max > 0) | (top > 0)))
    if bad.size:
        raise ValueError(f"heating_lw: g-point {int(bad[0])} has no emission in the atmosphere, so allocation='emission' gives it no rays, "
                         "but its sfc_src or top_radiance is positive: it would be left out of the result")
    return spectral_allocation(e, P, min_per_gpt)


def heating_lw(be, kd_lw, atm, nx, ny, dx, dy, dz, rays_per_cell, seed, cloud_lut=None, kn_grid=None, sfc_emis=None, max_events=None,
               top_radiance=None, allocation=None, min_per_gpt=1, p_lev=None):
    """3-D longwave heating from the thermal ray tracer's cell sensors (rrx_heating3d_render), on the chain of
    render_lw: the clear g-point tau of gas_optics_lw_direct (the gas does not scatter), the Planck sources of planck_source_direct
    and, with cloud_lut, the band cloud triple of cloud_optics_2str; sfc_emis and top_radiance as in render_lw. Returns flux_conv
    (nlay, ncol) in W m-2, the net radiative power that every cell takes up per unit horizontal area (negative: it cools), n_capped,
    n_clamped, rays_per_cell_gpt (ngpt,) and, given p_lev (nlay+1, ncol) in Pa, heating_rate = g/cp flux_conv / |dp| in K s-1.
    allocation=None: every g-point gets rays_per_cell rays per cell. allocation="emission": rays_per_cell is the TOTAL over all
    g-points, dealt by spectral_allocation(e, rays_per_cell, min_per_gpt) in proportion to e_g = sum over the cells of
    tau_abs lay_src[g], the power that the atmosphere emits in g; a g-point with e_g = 0 gets no rays, and is refused when its sfc_src
    or top_radiance is positive. What this allocation gains in variance over the equal split has not been measured."""
    if allocation not in (None, "emission"):
        raise ValueError(f"heating_lw: allocation is None or 'emission', got {allocation!r}")
    ncol, nlay, ngpt = atm.ncol, atm.nlay, kd_lw.ngpt
    if ncol != nx*ny:
        raise ValueError(f"heating_lw: ncol = {ncol} is not nx ny = {nx}*{ny}")
    if sfc_emis is None:
        emis = be.to_numpy(atm.emis_sfc)
        if np.any(emis != emis[:, :1]):
            raise ValueError("heating_lw: the atmosphere's emissivity differs between bands; pass sfc_emis")
        sfc_emis = np.ascontiguousarray(emis[:, 0])
    sfc_emis = be.asarray(sfc_emis)
    kn_grid = (nx, ny, nlay) if kn_grid is None else tuple(int(k) for k in kn_grid)

    _, col_gas, _ = gas_state(be, kd_lw, atm, None, interpolate=False)
    tau = be.gas_optics_lw_direct(kd_lw, atm.p_lay, atm.t_lay, col_gas, be.empty((ngpt, nlay, ncol)))
    src = be.planck_source_direct(kd_lw, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, _sfc_lay(atm), col_gas)
    cld = be.cloud_optics_2str(cloud_lut, atm.lwp, atm.iwp, atm.rel, atm.dei) if cloud_lut is not None else None
    if allocation == "emission":
        e = absorbed_emission(tau, src["lay_src"], kd_lw.band_lims_gpt, cld)
        sfc_max = be.to_numpy(src["sfc_src"].max(dim=1).values) if np.any(e == 0) else np.zeros(ngpt)
        m = heating_allocation(e, sfc_max, top_radiance, rays_per_cell, min_per_gpt)
    else:
        m = np.full(ngpt, int(rays_per_cell), dtype=np.int64)
    r = be.thermal_heating_render(tau, None, nx, ny, dx, dy, dz, sfc_emis, src["lay_src"], src["sfc_src"], kn_grid, m, seed,
                                  kd_lw.band_lims_gpt, top_at_1=atm.top_at_1, cloud=cld, max_events=max_events, top_radiance=top_radiance)
    r["rays_per_cell_gpt"] = m
    if p_lev is not None:
        p_lev = be.asarray(p_lev)
        if tuple(p_lev.shape) != (nlay + 1, ncol):
            raise ValueError(f"heating_lw: p_lev is (nlay+1, ncol) = {(nlay + 1, ncol)}, got {tuple(p_lev.shape)}")
        r["heating_rate"] = (9.80665/1004.64)*r["flux_conv"]/(p_lev[1:] - p_lev[:-1]).abs()
    return r


def _raytracer_medium(who, be, atm, tau, ssa, cld, aer, cloud_lut, phase_table, n_domain, z_lev):
    """What raytrace_sw and render_sw do with the chain's optics before they call the binding: with n_domain the split into the
    grid's arrays and a Background, the phase table with the (grid's) radius, and the medium that goes to the binding as keywords:
    none (the plain methods), aerosol= alone (the _bg methods on the whole atmosphere), or background= and aerosol= (split)."""
    background, rel = None, None
    if n_domain is not None:
        tau, ssa, cld, rel, background, aer = _raytracer_split(who, be, atm, tau, ssa, cld, n_domain, z_lev, aer)
    phase = _raytracer_phase(who, atm, cloud_lut, phase_table, rel)
    medium = dict(background=background, aerosol=aer) if background is not None else dict(aerosol=aer) if aer is not None else {}
    return tau, ssa, cld, phase, medium


def _raytracer_phase(who, atm, cloud_lut, phase_table, rel=None):
    """The table with the cells' radius: the liquid effective radius atm.rel (nlay, ncol), as in the reference (rel: that of the
    grid's layers when the atmosphere is split into a grid and a background)."""
    if phase_table is None:
        return None
    if cloud_lut is None:
        raise ValueError(f"{who}: a phase table needs cloud_lut (the table replaces the phase function of the cloud optics)")
    return phase_table.with_radius(atm.rel if rel is None else rel)


class Background:
    """The background atmosphere of the ray tracers, counted upward from the domain top: dz (nbg,) on the host, tau, ssa (ngpt, nbg)
    and cloud and aerosol, None or (tau, ssa, g) of (nbnd, nbg) each, on the device."""
    def __init__(self, dz, tau, ssa, cloud=None, aerosol=None):
        self.dz, self.tau, self.ssa, self.cloud, self.aerosol = dz, tau, ssa, cloud, aerosol


def _raytracer_split(who, be, atm, tau, ssa, cld, n_domain, z_lev, aer=None):
    """The lowest n_domain layers as the grid's arrays (in the atmosphere's layer order) and the layers above as a Background from
    column 0; also the grid's part of atm.rel. The aerosol triple is cut like the cloud's."""
    nlay, n_domain = atm.nlay, int(n_domain)
    if not 1 <= n_domain < nlay:
        raise ValueError(f"{who}: n_domain must be in [1, nlay = {nlay})")
    if z_lev is None:
        raise ValueError(f"{who}: n_domain needs z_lev (nlay+1,), the heights of the levels")
    z_lev = np.asarray(z_lev, dtype=np.float64).reshape(-1)
    if z_lev.size != nlay + 1:
        raise ValueError(f"{who}: z_lev is (nlay+1,) = ({nlay + 1},), got {z_lev.size}")
    # array layers of the grid, and of the background counted upward from the domain top
    grid = slice(nlay - n_domain, nlay) if atm.top_at_1 else slice(0, n_domain)
    above = list(range(nlay - n_domain - 1, -1, -1)) if atm.top_at_1 else list(range(n_domain, nlay))
    dz_bg = np.abs(z_lev[1:] - z_lev[:-1])[above].astype(be.np_dtype)
    if not np.all(dz_bg > 0):
        raise ValueError(f"{who}: z_lev must be strictly monotonic")
    column0 = lambda t: t[:, above, 0].contiguous()
    background = Background(dz_bg, column0(tau), column0(ssa), None if cld is None else tuple(column0(c) for c in cld),
                            None if aer is None else tuple(column0(c) for c in aer))
    part = lambda t: t[:, grid, :].contiguous()
    rel = atm.rel[grid, :].contiguous() if getattr(atm, "rel", None) is not None else None
    return (part(tau), part(ssa), None if cld is None else tuple(part(c) for c in cld), rel, background,
            None if aer is None else tuple(part(c) for c in aer))


def _raytracer_inputs(who, be, kd_sw, atm, nx, ny, cloud_lut, kn_grid, sfc_albedo, aerosol_lut=None):
    """What both ray tracers take from the chain: the clear g-point tau, ssa, the band cloud triple (or None), the albedo (ncol,),
    the one mu0, inc_dir (ngpt,) on the host, the k_null grid and the band aerosol triple (or None); one sun and one albedo are
    checked."""
    ncol, nlay, ngpt = atm.ncol, atm.nlay, kd_sw.ngpt
    if ncol != nx*ny:
        raise ValueError(f"{who}: ncol = {ncol} is not nx ny = {nx}*{ny}")
    mu0 = be.to_numpy(atm.mu0).reshape(-1)
    tsi = be.to_numpy(atm.tsi_scaling).reshape(-1)
    if np.any(mu0 != mu0[0]) or np.any(tsi != tsi[0]):
        raise ValueError(f"{who}: mu0 and tsi_scaling must be the same in every column (one sun for the domain)")
    if sfc_albedo is None:
        a_dir, a_dif = be.to_numpy(atm.sfc_alb_dir), be.to_numpy(atm.sfc_alb_dif)
        if np.any(a_dir != a_dif) or np.any(a_dif != a_dif[:, :1]):
            raise ValueError(f"{who}: the atmosphere's albedo differs between bands or between direct and diffuse; pass sfc_albedo")
        sfc_albedo = np.ascontiguousarray(a_dif[:, 0])
    sfc_albedo = be.asarray(sfc_albedo)
    kn_grid = (nx, ny, nlay) if kn_grid is None else tuple(int(k) for k in kn_grid)

    col_dry, col_gas, _ = gas_state(be, kd_sw, atm, None, interpolate=False)
    tau = be.empty((ngpt, nlay, ncol)); ssa = be.empty((ngpt, nlay, ncol))
    g = None if getattr(be, "supports_null_g", False) else be.empty((ngpt, nlay, ncol))
    be.gas_optics_sw_direct(kd_sw, atm.p_lay, atm.t_lay, col_gas, col_dry, tau, ssa, g)
    cld = be.cloud_optics_2str(cloud_lut, atm.lwp, atm.iwp, atm.rel, atm.dei) if cloud_lut is not None else None

    F = be.np_dtype.type
    inc_dir = (be.to_numpy(kd_sw.solar_source).astype(be.np_dtype) * F(tsi[0])) * F(mu0[0])
    aer = None
    if aerosol_lut is not None:
        aer = tuple(be.aerosol_optics(aerosol_lut, [atm.aermr["aermr%02d" % i] for i in range(1, 12)], atm.rh, atm.p_lev))
    return tau, ssa, cld, sfc_albedo, float(mu0[0]), inc_dir, kn_grid, aer


_STEP_ATMOSPHERE = None


def _step_atmosphere_type():
    """synthetic.Atmosphere with the per-column fields of ResidentSolver(mu0_lay= / altitude= / ref_altitude=) (private to the step)."""
    global _STEP_ATMOSPHERE
    if _STEP_ATMOSPHERE is None:
        import dataclasses
        from .synthetic import Atmosphere
        _STEP_ATMOSPHERE = dataclasses.make_dataclass("StepAtmosphere", [(n, object, None) for n in ("mu0_lay", "altitude", "ref_altitude")],
                                                      bases=(Atmosphere,))
    return _STEP_ATMOSPHERE


# The LW solve of a resident step takes exactly one form. In order of precedence: name -> (the option that chooses it, the options it
# admits beside that one, why it admits no others). ResidentSolver.resolve_options reads the rules from here and step() dispatches on
# the name. The last two forms refuse nothing: whatever they could not serve has chosen a form above them.
_LW_FORMS = {
    "per_gpoint": ("do_broadband=False", {"n_gauss_angles > 1"}, "only the broadband LW solvers, fed by the Planck-lite chain, have that form"),
    "rescaled": ("lw_rescaling=True", set(), "the rescaled LW solver has one broadband form with one fixed angle"),
    "two_stream": ("lw_scattering=True", set(), "the two-stream LW solver has one broadband form without quadrature angles"),
    "optimal": ("optimal_angles=True", {"jacobian=True"}, "optimal angles are one angle and have no by-band form"),
    "byband": ("byband=True", set(), "no by-band Jacobians and no by-band form with several angles"),
    "angles": ("n_gauss_angles > 1", {"jacobian=True"}, None),
    "fractions": ("do_broadband=True", {"jacobian=True"}, None),
}


class ResidentSolver:
    """One full clear-sky LW+SW solve per ``step()`` with every buffer allocated once (what a host model keeps
    resident between radiation calls, cf. the cached subsets in /root/reference/src_test/Radiation_solver.cu:450-466).
    HIP backend only; used by bench.py and the full-size tests. ``stage_events`` (torch.cuda.Event pairs on the
    launch stream) give per-stage device durations without synchronising inside the step.

    The options, beside do_broadband (fused broadband solvers; the LW sources are then formed inside the solver from Planck fractions
    and band Planck functions, the "Planck-lite" chain) and overlap (the LW and SW chains on two streams):
    cloud_luts: all-sky (BASELINE C5), (lw_lut, sw_lut) of cloud optics; clouds are added by band where the gas optics is stored,
      delta-scaled in SW.
    byband: the step also fills self.bnd_fluxes (lw_up/lw_dn/lw_net/sw_up/sw_dn/sw_dir/sw_net, (nbnd, nlev, ncol) each, the caller's
      column order) from the fused solvers' by-band form; the seven broadband arrays come from the same solves.
    jacobian: the step also fills self.lw_flux_up_jac (nlev, ncol, the caller's column order), the surface-temperature Jacobian of the
      LW upward flux [W m-2 K-1] from the same fused solve; the seven broadband arrays stay bit for bit those without it.
    n_gauss_angles: LW quadrature angles (1..4, Gauss-Jacobi-5 nodes); more than one takes the several-angle form of the fused solver
      (lw_solver_noscat_fractions_angles), which has no by-band outputs.
    optimal_angles: the one LW angle's secant is the k-distribution's optimal-angle fit of the column's total optical depth per
      g-point (upstream's compute_optimal_angles / lw_Ds), formed inside the fused solver (lw_solver_noscat_fractions_optimal);
      keep_secants: the step also fills self.lw_secants (ngpt, ncol of the step), the secants that solve used.
    lw_scattering: the LW chain lets clouds scatter -- clear gas optics, LW cloud tau / ssa / g by band (cloud_optics_2str on the LW
      table, not delta-scaled) and the fused two-stream solver (lw_solver_2stream_fractions); without cloud LUTs the same solver with
      ssa = 0. One solve without quadrature angles.
    lw_rescaling: the LW chain treats cloud scattering by rescaling -- the same inputs and the fused no-scattering solve on rescaled
      optical depths with one correction sweep (lw_solver_noscat_fractions_rescaled); without cloud LUTs the same solver with ssa = 0.
    cloud_fraction: McICA cloud sampling. (nlay, ncol) cloud fractions in the caller's column order; each step runs the
      CLEAR gas optics and then rrx_mcica_increment_*, which gives every g-point its own sub-column and adds the band cloud properties
      in the cloudy cells only. cloud_overlap: "max_ran", or "exp_ran" with overlap_param (nlay-1, ncol), the overlap parameter between
      array layers l and l+1. The mask is redrawn every step from the current self.mcica_seed (a host advances it between calls;
      domain 0 = LW, 1 = SW); a column's draws are keyed by mcica_col_offset + its index in the caller's order, so sorting, padding
      and sharding do not change them. The fields stay attributes: replace or update them between steps.
    mu0_lay / altitude / ref_altitude: mu0 by layer, the SW solver takes a cosine of the solar zenith angle per layer.
      mu0_lay: (nlay, ncol) in the caller's column order, used as it is. altitude: (nlay, ncol) layer altitudes in metres, with
      ref_altitude (ncol, default 0) the altitude at which atm.mu0 holds: every step forms mu0_lay on the device from the current
      atm.mu0 by the spherical-geometry correction (zenith_angle_spherical_correction). The fields stay attributes: replace or update
      them between steps. They are per-column fields (_COLUMN_FIELDS): sorted, padded and gathered to the sunlit columns with the
      others. The sunlit list is made from atm.mu0 in either case; the LW chain does not see any of this.
    sunlit, sort_columns: see __init__."""

    STAGES = ("lw_gas_optics", "lw_planck", "lw_solver", "lw_reduce", "sw_gas_optics", "sw_solver", "sw_reduce")

    @staticmethod
    def resolve_options(atm, kd_lw, do_broadband=False, cloud_luts=None, byband=False, sunlit=False, jacobian=False, n_gauss_angles=1,
                        optimal_angles=False, lw_scattering=False, lw_rescaling=False, cloud_fraction=None, cloud_overlap="max_ran",
                        overlap_param=None, mu0_lay=None, altitude=None, ref_altitude=None):
        """The option rules of ResidentSolver, in this one place: returns the name of the LW form (a key of _LW_FORMS) that the options
        choose, or raises ValueError. Reads atm.nlay / atm.ncol and kd_lw.optimal_angle_fit; needs no backend and no device."""
        if mu0_lay is not None and altitude is not None:
            raise ValueError("ResidentSolver: mu0_lay and altitude are two ways to the same thing: give one")
        if ref_altitude is not None and altitude is None:
            raise ValueError("ResidentSolver: ref_altitude without altitude")
        for name, v, want in (("mu0_lay", mu0_lay, (atm.nlay, atm.ncol)), ("altitude", altitude, (atm.nlay, atm.ncol)),
                              ("ref_altitude", ref_altitude, (atm.ncol,)), ("cloud_fraction", cloud_fraction, (atm.nlay, atm.ncol)),
                              ("overlap_param", overlap_param, (atm.nlay-1, atm.ncol))):
            if v is not None and tuple(v.shape) != want:
                raise ValueError(f"ResidentSolver: {name} {tuple(v.shape)} is not {want}")
        if altitude is not None and bool((altitude < (0. if ref_altitude is None else ref_altitude)).any()):
            raise ValueError("ResidentSolver: an altitude lies below its column's reference altitude")
        if cloud_fraction is None:
            if overlap_param is not None:
                raise ValueError("ResidentSolver: overlap_param without cloud_fraction")
        else:
            if cloud_luts is None:
                raise ValueError("ResidentSolver: cloud_fraction needs cloud_luts (the cloud optics whose band properties are sampled)")
            if cloud_overlap not in ("max_ran", "exp_ran"):
                raise ValueError(f"ResidentSolver: cloud_overlap = {cloud_overlap!r} is not 'max_ran' or 'exp_ran'")
            if (cloud_overlap == "exp_ran") != (overlap_param is not None):
                raise ValueError("ResidentSolver: cloud_overlap='exp_ran' takes overlap_param (nlay-1, ncol), 'max_ran' takes none")
            for flag, name in ((lw_scattering, "lw_scattering=True"), (lw_rescaling, "lw_rescaling=True"), (sunlit, "sunlit=True")):
                if flag:
                    raise ValueError(f"ResidentSolver: cloud_fraction with {name} is not supported (the scattering LW solvers combine "
                                     "the band clouds themselves; the sunlit-only SW chain does not carry the column identities)")
        if not 1 <= int(n_gauss_angles) <= 4:
            raise ValueError(f"ResidentSolver: n_gauss_angles = {n_gauss_angles} is outside 1..4")
        given = [name for name, on in (("lw_rescaling=True", lw_rescaling), ("lw_scattering=True", lw_scattering),
                                       ("optimal_angles=True", optimal_angles), ("byband=True", byband),
                                       ("n_gauss_angles > 1", int(n_gauss_angles) > 1), ("jacobian=True", jacobian)) if on]
        form = "per_gpoint" if not do_broadband else next((f for f, rule in _LW_FORMS.items() if rule[0] in given), "fractions")
        chooser, admits, why = _LW_FORMS[form]
        for name in given:
            if name != chooser and name not in admits:
                raise ValueError(f"ResidentSolver: {chooser} with {name} is not supported ({why})")
        if form == "optimal" and getattr(kd_lw, "optimal_angle_fit", None) is None:
            raise ValueError("ResidentSolver: optimal_angles=True needs a LW k-distribution with optimal_angle_fit")
        return form

    def __init__(self, be, kd_lw, kd_sw, atm, do_broadband=False, overlap=False, cloud_luts=None, sort_columns=None, byband=False,
                 sunlit=False, jacobian=False, n_gauss_angles=1, optimal_angles=False, keep_secants=False, lw_scattering=False,
                 lw_rescaling=False, cloud_fraction=None, cloud_overlap="max_ran", overlap_param=None, mcica_seed=0, mcica_col_offset=0,
                 mu0_lay=None, altitude=None, ref_altitude=None, planet_radius=6.37123e6):
        import torch
        self.torch = torch
        self.lw_form = self.resolve_options(
            atm, kd_lw, do_broadband=do_broadband, cloud_luts=cloud_luts, byband=byband, sunlit=sunlit, jacobian=jacobian,
            n_gauss_angles=n_gauss_angles, optimal_angles=optimal_angles, lw_scattering=lw_scattering, lw_rescaling=lw_rescaling,
            cloud_fraction=cloud_fraction, cloud_overlap=cloud_overlap, overlap_param=overlap_param, mu0_lay=mu0_lay, altitude=altitude,
            ref_altitude=ref_altitude)
        self.be, self.kd_lw, self.kd_sw, self.atm = be, kd_lw, kd_sw, atm
        self.do_broadband, self.cloud_luts = do_broadband, cloud_luts
        self.lite = do_broadband                 # the Planck-lite chain feeds every broadband LW solver
        self.g_zero = cloud_luts is None         # clear sky: g == 0 is neither written nor read
        self.byband, self.jacobian, self.sunlit = bool(byband), bool(jacobian), bool(sunlit)
        self.n_gauss_angles, self.optimal_angles = int(n_gauss_angles), bool(optimal_angles)
        self.keep_secants = bool(keep_secants) and self.optimal_angles
        self.lw_scattering, self.lw_rescaling = bool(lw_scattering), bool(lw_rescaling)
        self.cloud_fraction, self.overlap_param = cloud_fraction, overlap_param
        self.mcica_seed, self.mcica_col_offset = int(mcica_seed), int(mcica_col_offset)
        self.mu0_lay, self.altitude, self.ref_altitude, self.planet_radius = mu0_lay, altitude, ref_altitude, float(planet_radius)
        # Column sorting. The windowed gas optics stages ONE box of LUT nodes per 256 neighbouring cells; columns that differ much in
        # pressure (RFMIP-like sites, --col-spread) do not fit one box and fall back to the gather kernels (+40 % per step at +-35 %
        # pressure spread). Columns are independent, so the step may process them in any order: sorted by surface pressure, neighbours
        # are alike again. The inputs are gathered into sorted order at the top of the step and the seven broadband flux arrays
        # scattered back at its end (0.5 ms per step at C4: ~30 gathers of (nlay, ncol) arrays). "auto" (default, or
        # RRX_SORT_COLUMNS): decided once from the initial atmosphere -- on when the surface pressure varies by more than 20 % inside
        # some 256-column block, about one cell of the LUT's pressure grid (ln p spacing 0.2): below that the boxes still fit and
        # sorting costs more than it brings (measured: +-5 % spread 15.1 ms unsorted, 15.6 sorted; +-35 %: 19.4 -> 16.0 ms).
        if sort_columns is None:
            sort_columns = os.environ.get("RRX_SORT_COLUMNS", "auto")
        if sort_columns == "auto":
            ps = atm.p_lev[-1 if atm.top_at_1 else 0]
            nb = (atm.ncol // 256) * 256
            if nb >= 256:
                blk = ps[:nb].reshape(-1, 256)
                sort_columns = bool((((blk.max(dim=1).values - blk.min(dim=1).values) / blk.mean(dim=1)) > 0.2).any().item())
            else:
                sort_columns = False
        self.sort_columns = bool(sort_columns) and str(sort_columns) != "0"
        # Padding: the step runs on a multiple of 16 columns -- the rows of the (col, lay, gpt) intermediates then start on 128-B lines
        # (16 385 columns cost 20 % more than 16 384 otherwise); the extra columns repeat the last one and are dropped when the fluxes
        # go back to the caller's order. One gather index serves sorting and padding, built once and applied to an explicit list of
        # per-column fields: refresh_column_order() rebuilds it when the host model's pressures have changed enough to matter.
        pad16 = bool(int(os.environ.get("RRX_PAD_COLUMNS", "1"))) and atm.ncol > 16
        self.npad = (16 - atm.ncol % 16) if (pad16 and atm.ncol % 16 != 0) else 0
        self.ncol_caller = atm.ncol
        self.perm = None
        if self.sort_columns or self.npad:
            self.refresh_column_order()
        # overlap: LW and SW chains are independent, so they can run on two HIP streams and share the chip (the gather-
        # bound gas-optics kernels of one chain fill in next to the HBM-bound solver of the other)
        self.overlap = overlap
        self.streams = [torch.cuda.Stream(device=be.device), torch.cuda.Stream(device=be.device)] if overlap else None

        # ---- what a step owns -------------------------------------------------------------------------------------------------
        ncol, nlay = atm.ncol + self.npad, atm.nlay              # columns of a step (padded)
        ng_l, ng_s = kd_lw.ngpt, kd_sw.ngpt
        e = be.empty
        self.col_dry = e((nlay, ncol))
        self.col_dry2 = None                                     # the SW chain's own when overlapping (allocated by the first step)
        # LW gas optics: optical depth and the sources as the form's solver takes them
        if do_broadband:
            self.lw = dict(tau=e((ng_l, nlay, ncol)), pfrac=e((ng_l, nlay, ncol)), blay=e((kd_lw.nbnd, nlay, ncol)),
                           blev=e((kd_lw.nbnd, nlay+1, ncol)), sfc_src=e((ng_l, ncol)), sfc_src_jac=e((ng_l, ncol)))
        else:
            self.lw = dict(tau=e((ng_l, nlay, ncol)), lay_src=e((ng_l, nlay, ncol)), lev_src=e((ng_l, nlay+1, ncol)),
                           sfc_src=e((ng_l, ncol)), sfc_src_jac=e((ng_l, ncol)))
        self.sw = dict(tau=e((ng_s, nlay, ncol)), ssa=e((ng_s, nlay, ncol)), g=e((ng_s, nlay, ncol)))
        if not do_broadband:                                     # fluxes per g-point, summed by the reduce stage
            self.lw.update(gpt_up=e((ng_l, nlay+1, ncol)), gpt_dn=e((ng_l, nlay+1, ncol)))
            self.sw.update(gpt_up=e((ng_s, nlay+1, ncol)), gpt_dn=e((ng_s, nlay+1, ncol)), gpt_dir=e((ng_s, nlay+1, ncol)))
        # packed broadband outputs: LW up/dn/net + SW up/dn/dir/net  (7, nlev, ncol) -> one all-gather; the *_sorted twins hold the
        # step's own column order when that is not the caller's
        self.fluxes = e((7, nlay+1, atm.ncol))
        self.fluxes_sorted = e((7, nlay+1, ncol)) if self.perm is not None else None
        self.lw_flux_up_jac = e((nlay+1, atm.ncol)) if self.jacobian else None
        self.jac_sorted = e((nlay+1, ncol)) if (self.jacobian and self.perm is not None) else None
        # packed band outputs: LW up/dn/net (3, nbnd_lw, nlev, ncol), SW up/dn/dir/net (4, nbnd_sw, nlev, ncol)
        self.bnd_lw = self.bnd_sw = self.bnd_lw_sorted = self.bnd_sw_sorted = None
        self.bnd_fluxes = None
        if self.byband:
            self.bnd_lw = e((3, kd_lw.nbnd, nlay+1, atm.ncol)); self.bnd_sw = e((4, kd_sw.nbnd, nlay+1, atm.ncol))
            if self.perm is not None:
                self.bnd_lw_sorted = e((3, kd_lw.nbnd, nlay+1, ncol)); self.bnd_sw_sorted = e((4, kd_sw.nbnd, nlay+1, ncol))
            self.bnd_fluxes = dict(lw_up=self.bnd_lw[0], lw_dn=self.bnd_lw[1], lw_net=self.bnd_lw[2],
                                   sw_up=self.bnd_sw[0], sw_dn=self.bnd_sw[1], sw_dir=self.bnd_sw[2], sw_net=self.bnd_sw[3])
        # the chains' flux targets, in the step's column order, as views made once (a step indexes them some twenty times, and
        # making a tensor view each time is host work that shows in the 1.7 ms step at 2 048 columns)
        own = self.perm is None
        self._F = tuple(self.fluxes if own else self.fluxes_sorted)
        self._BL = tuple(self.bnd_lw if own else self.bnd_lw_sorted) if self.byband else None
        self._BS = tuple(self.bnd_sw if own else self.bnd_sw_sorted) if self.byband else None
        # sunlit-only SW: every step lists the columns with mu0 > 0 on the device (in the step's own column order), gathers the SW
        # inputs of those columns into the buffers below, runs the SW chain on that many columns (views of the full-size SW buffers)
        # and scatters the SW fluxes back with zeros in the night columns. The host needs the count to size the launches: it is
        # copied to pinned memory at the top of the step and waited for only once the LW chain has been enqueued. All columns
        # sunlit: the plain SW path, bit for bit.
        if self.sunlit:
            # (padded to a multiple of 16 like the plain step: at most ncol rounded up to 16, which the step's buffers hold)
            self.sun_pad = 16 if pad16 else 1
            nmax = -(-atm.ncol // self.sun_pad) * self.sun_pad
            assert nmax <= ncol
            self.sun_perm = be.int_empty((nmax,))
            self.sun_count = be.int_empty((1,))
            self.sun_count_host = torch.empty((1,), dtype=torch.int32, pin_memory=True)
            self.sun_event = torch.cuda.Event()
            self.sun_wait_ms = 0.0      # host time spent waiting for the count, summed over the steps
            self.sun_in = {}            # gathered SW inputs, (..., ncol) fields at full width
            for k in self._SW_FIELDS:
                v = getattr(self._step_atmosphere(), k, None)
                if v is not None and (cloud_luts is not None or k not in ("lwp", "iwp", "rel", "dei")):
                    self.sun_in[k] = e(tuple(v.shape[:-1]) + (ncol,) if self._COLUMN_FIELDS[k] < 0 else (ncol,) + tuple(v.shape[1:]))
            self.sun_vmr = {n: e((nlay, ncol)) for n, t in atm.vmr.items() if hasattr(t, "dim") and t.dim() == 2}
            self.sun_fluxes = e((4, nlay+1, ncol))
            self.sun_bnd = e((4, kd_sw.nbnd, nlay+1, ncol)) if self.byband else None
        self.weights = be.asarray(np.ascontiguousarray(GAUSS_WTS[self.n_gauss_angles-1, :self.n_gauss_angles]))
        self.gauss_Ds = be.asarray(GAUSS_DS)
        # secants and the band -> g-point expansion of emissivity / albedos: buffers allocated once, the launches themselves are
        # part of every step (rte_lw / rte_sw of the reference run them per solve: src_cuda/Rte_lw.cu:70-110, Rte_sw.cu:57-100)
        self.secants = e((self.n_gauss_angles, ng_l, ncol))
        self.optimal_fit = be.optimal_fit_abi(kd_lw) if self.optimal_angles else None
        self.lw_secants = e((ng_l, ncol)) if self.keep_secants else None
        self.sfc_emis_gpt = e((ng_l, ncol)); self.alb_dir = e((ng_s, ncol)); self.alb_dif = e((ng_s, ncol))
        self.mu0_lay_step = e((nlay, ncol)) if self.altitude is not None else None      # the step's corrected cosines
        self.events = self._rec = None



    def enable_stage_events(self, nsteps):
        ev = self.torch.cuda.Event
        self.events = [{s: (ev(enable_timing=True), ev(enable_timing=True)) for s in self.STAGES} for _ in range(nsteps)]
        self._istep = 0

    def stage_ms(self):
        out = {s: [] for s in self.STAGES}
        for rec in self.events[:self._istep]:
            for s, (a, b) in rec.items():
                out[s].append(a.elapsed_time(b))
        return {s: float(np.mean(v)) for s, v in out.items() if v}

    # per-column fields of an Atmosphere and the axis their column index sits on (everything else is shared by all columns)
    _COLUMN_FIELDS = {"p_lay": -1, "p_lev": -1, "t_lay": -1, "t_lev": -1, "t_sfc": 0, "mu0": 0, "tsi_scaling": 0,
                      "emis_sfc": 0, "sfc_alb_dir": 0, "sfc_alb_dif": 0, "lwp": -1, "iwp": -1, "rel": -1, "dei": -1, "rh": -1,
                      "mu0_lay": -1, "altitude": -1, "ref_altitude": 0}

    _SW_FIELDS = ("p_lay", "p_lev", "t_lay", "mu0", "tsi_scaling", "sfc_alb_dir", "sfc_alb_dif", "lwp", "iwp", "rel", "dei",
                  "mu0_lay", "altitude", "ref_altitude")

    def _step_atmosphere(self):
        """The caller's atmosphere; with mu0_lay= / altitude=, a view of it that carries the solver's own per-column fields (mu0_lay,
        altitude, ref_altitude) beside the atmosphere's, so that the gathers below take them along. The fields exist on that view
        only: the solver's arguments are the one way in, an Atmosphere has no such fields."""
        if self.mu0_lay is None and self.altitude is None:
            return self.atm
        return _step_atmosphere_type()(**self.atm.__dict__, mu0_lay=self.mu0_lay, altitude=self.altitude, ref_altitude=self.ref_altitude)

    @staticmethod
    def _cols(t, n):
        """The leading part of a (..., ncol) buffer as a contiguous (..., n) tensor."""
        lead = tuple(t.shape[:-1])
        return t.view(-1)[:int(np.prod(lead, dtype=np.int64))*n].view(lead + (n,))

    @staticmethod
    def _rows(t, n):
        """The leading part of an (ncol, ...) buffer as a contiguous (n, ...) tensor."""
        rest = tuple(t.shape[1:])
        return t.view(-1)[:int(np.prod(rest, dtype=np.int64))*n].view((n,) + rest)

    def _sunlit_atmosphere(self, n_out):
        """The SW inputs of the columns sun_perm[:n_out], gathered on the device into the resident buffers (views of n_out columns)."""
        be, a, perm = self.be, self._step_atmosphere(), self.sun_perm
        out = dict(a.__dict__)         # (fields the SW chain does not read stay as they are)
        out["ncol"] = n_out
        for k, buf in self.sun_in.items():
            v = getattr(a, k, None)
            if v is None:                  # (a field of the solver's that the host has taken away since)
                continue
            if self._COLUMN_FIELDS[k] < 0 or v.dim() == 1:        # column fastest: (..., ncol) or (ncol,)
                out[k] = be.gather_cols(perm, v, self._cols(buf, n_out) if self._COLUMN_FIELDS[k] < 0 else buf[:n_out])
            else:                                                  # column slowest: (ncol, nbnd)
                out[k] = be.gather_lastdim(perm, v, self._rows(buf, n_out))
        out["vmr"] = {n: (be.gather_cols(perm, t, self._cols(self.sun_vmr[n], n_out)) if n in self.sun_vmr else t)
                      for n, t in a.vmr.items()}
        return type(a)(**out)

    def refresh_column_order(self):
        """(Re)build the gather index of a step: ascending surface pressure when sorting, the caller's order otherwise, padded with
        repeats of its last entry. Call it again when the pressures have changed enough to matter; the index is reused otherwise."""
        torch = self.torch
        a = self.atm
        if self.sort_columns:
            perm = torch.argsort(a.p_lev[-1 if a.top_at_1 else 0])
        else:
            perm = torch.arange(a.ncol, device=a.p_lev.device)
        if self.npad:
            perm = torch.cat([perm, perm[-1:].expand(self.npad)])
        self.perm = perm.contiguous()
        self.perm_i32 = self.perm.to(torch.int32)        # (the order of the sunlit-column list: the HIP entries take int32)

    def _gathered_atmosphere(self):
        """The atmosphere with its columns in the order (and count) of self.perm."""
        a, perm = self._step_atmosphere(), self.perm
        out = {}
        for k, v in a.__dict__.items():
            if k == "ncol":
                out[k] = int(perm.numel())
            elif k in self._COLUMN_FIELDS and v is not None:
                out[k] = v.index_select(v.dim() - 1 if self._COLUMN_FIELDS[k] < 0 else 0, perm)
            elif isinstance(v, dict):      # vmr / aermr: (nlay, ncol) fields are per column, profiles (nlay,) and scalars are shared
                out[k] = {n: (t.index_select(1, perm) if (hasattr(t, "dim") and t.dim() == 2) else t) for n, t in v.items()}
            else:
                out[k] = v
        return type(a)(**out)

    def _mark(self, stage, end=False):
        if self._rec is not None:
            self._rec[stage][1 if end else 0].record(self.torch.cuda.current_stream(self.be.device))   # the chain's stream when overlapping

    def _chain_stream(self, ichain, main):
        """The context a chain is enqueued in: its own stream, behind what main holds so far, when overlapping."""
        if not self.overlap:
            return contextlib.nullcontext()
        self.streams[ichain].wait_stream(main)
        return self.torch.cuda.stream(self.streams[ichain])

    def step(self):
        be, atm = self.be, self._step_atmosphere()
        perm = self.perm
        if perm is not None:
            atm = self._gathered_atmosphere()
        if self.overlap and self.col_dry2 is None:
            self.col_dry2 = be.empty(tuple(self.col_dry.shape))
        self._rec = None
        if self.events is not None and self._istep < len(self.events):
            self._rec = self.events[self._istep]
            self._istep += 1
        mcica = None
        if self.cloud_fraction is not None:     # the sampled fields in the step's column order, and the identities that go with it
            cfrac, alpha, col_id = self.cloud_fraction, self.overlap_param, None
            if perm is not None:
                cfrac = cfrac.index_select(1, perm)
                alpha = None if alpha is None else alpha.index_select(1, perm)
                col_id = self.perm_i32 + self.mcica_col_offset
            mcica = (cfrac, alpha, col_id)
        F, BL, BS = self._F, self._BL, self._BS
        J = self.lw_flux_up_jac if perm is None else self.jac_sorted
        main = self.torch.cuda.current_stream(be.device)
        if self.sunlit:               # the column list and its count, on the device; the count travels to pinned host memory
            n = self.ncol_caller
            be.sunlit_columns(self.atm.mu0, None if perm is None else self.perm_i32[:n], self.sun_pad, perm=self.sun_perm, count=self.sun_count)
            self.sun_count_host.copy_(self.sun_count, non_blocking=True)
            self.sun_event.record(main)
        with self._chain_stream(0, main):
            self._lw_chain(atm, self.col_dry, self.lw, F, J, BL, mcica)
        sw_day = False                # this step's SW chain runs on the sunlit columns only
        with self._chain_stream(1, main):
            self._mark("sw_gas_optics")
            col_dry = self.col_dry2 if self.overlap else self.col_dry
            if self.sunlit:
                t0 = time.perf_counter()
                self.sun_event.synchronize()      # the LW chain is enqueued by now; the count was ready long before
                self.sun_wait_ms += (time.perf_counter() - t0) * 1e3
                n_day = int(self.sun_count_host[0])
                sw_day = n_day < self.ncol_caller
            if sw_day:      # the gathered inputs, views of n_out columns of the SW buffers, the sunlit targets (no McICA: refused)
                n_out = -(-n_day // self.sun_pad) * self.sun_pad
                self._sw_chain(self._sunlit_atmosphere(n_out) if n_day else None, self._cols(col_dry, n_out),
                               {k: self._cols(v, n_out) for k, v in self.sw.items()}, self._cols(self.alb_dir, n_out),
                               self._cols(self.alb_dif, n_out), self._cols(self.sun_fluxes, n_out),
                               self._cols(self.sun_bnd, n_out) if self.byband else None, None, n_day=n_day)
            else:
                self._sw_chain(atm, col_dry, self.sw, self.alb_dir, self.alb_dif, F[3:], BS, mcica)
        if self.overlap:
            main.wait_stream(self.streams[0]); main.wait_stream(self.streams[1])
        if perm is not None:                              # back to the caller's column order (padding columns dropped)
            n = self.ncol_caller
            nf = 3 if sw_day else 7                       # (a sunlit-only SW chain has written the caller's order already)
            self.fluxes[:nf].index_copy_(2, perm[:n], self.fluxes_sorted[:nf, :, :n])
            if self.jacobian:
                self.lw_flux_up_jac.index_copy_(1, perm[:n], J[:, :n])
            if self.byband:
                self.bnd_lw.index_copy_(3, perm[:n], self.bnd_lw_sorted[..., :n])
                if not sw_day:
                    self.bnd_sw.index_copy_(3, perm[:n], self.bnd_sw_sorted[..., :n])
        return self.fluxes

    def _lw_chain(self, atm, col_dry, buf, F, J, BL, mcica):
        """The LW launches of a step on atm's columns: gas optics into buf, the solve of self.lw_form, fluxes into F[0:3] (up, dn,
        net) and, where the form has them, J (Jacobian) and BL (by band). mcica: None or (cloud fraction, overlap parameter,
        column identities) in atm's column order."""
        be, kd, mark = self.be, self.kd_lw, self._mark
        form = self.lw_form
        mark("lw_gas_optics")
        be.get_col_dry(atm.vmr["h2o"], atm.p_lev, out=col_dry)
        col_gas = be.fill_gases(kd, atm.vmr, col_dry)
        tc = cld = None
        if self.cloud_luts is not None and form in ("two_stream", "rescaled"):      # tau, ssa, g by band: the solver combines them itself
            cld = be.cloud_optics_2str(self.cloud_luts[0], atm.lwp, atm.iwp, atm.rel, atm.dei)
        elif self.cloud_luts is not None:     # /root/reference/src_test/Radiation_solver.cu:497-512
            tc = be.cloud_optics_1scl(self.cloud_luts[0], atm.lwp, atm.iwp, atm.rel, atm.dei)
        # all-sky: the by-band cloud optical depth is added where the gas optics is stored; McICA adds it afterwards, cell by cell
        fused = tc if mcica is None else None
        if form == "per_gpoint":
            be.gas_optics_lw_direct(kd, atm.p_lay, atm.t_lay, col_gas, buf["tau"], by_band=fused)
        else:
            be.gas_optics_lw_fractions(kd, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, _sfc_lay(atm), col_gas, buf["tau"], out=buf,
                                       by_band=fused)
        if tc is not None and mcica is not None:
            be.mcica_increment_1scalar(buf["tau"], tc, kd.band_lims_gpt, mcica[0], mcica[1], self.mcica_seed, 0, mcica[2], self.mcica_col_offset)
        mark("lw_gas_optics", True)
        mark("lw_planck")
        if form == "per_gpoint":                  # (the broadband forms got their fractions with the optical depths)
            be.planck_source_direct(kd, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, _sfc_lay(atm), col_gas, out=buf)
        mark("lw_planck", True)
        mark("lw_solver")
        if form not in ("optimal", "two_stream"):      # (neither solver reads a secants array)
            be.lw_secants_array(atm.ncol, kd.ngpt, self.n_gauss_angles, MAX_GAUSS_PTS, self.gauss_Ds, out=self.secants)
        be.expand_and_transpose(kd.band_lims_gpt, atm.emis_sfc, kd.ngpt, out=self.sfc_emis_gpt)
        top, sec, wts, tau, emis = atm.top_at_1, self.secants, self.weights, buf["tau"], self.sfc_emis_gpt
        if form == "rescaled":
            be.lw_solver_noscat_fractions_rescaled(top, kd, sec, wts, tau, buf, emis, cloud=cld, flux_up=F[0], flux_dn=F[1])
        elif form == "two_stream":
            be.lw_solver_2stream_fractions(top, kd, tau, buf, emis, cloud=cld, flux_up=F[0], flux_dn=F[1])
        elif form == "optimal":
            be.lw_solver_noscat_fractions_optimal(top, kd, wts, tau, buf, emis, fit=self.optimal_fit, flux_up=F[0], flux_dn=F[1],
                                                  flux_up_jac=J, jacobian=self.jacobian, secants_out=self.lw_secants)
        elif form == "byband":
            be.lw_solver_noscat_fractions_byband(top, kd, sec, wts, tau, buf, emis,
                                                 out=dict(bnd_flux_up=BL[0], bnd_flux_dn=BL[1], bnd_flux_net=BL[2], flux_up=F[0], flux_dn=F[1]))
        elif form == "angles":
            be.lw_solver_noscat_fractions_angles(top, kd, sec, wts, tau, buf, emis, flux_up=F[0], flux_dn=F[1], flux_up_jac=J,
                                                 jacobian=self.jacobian)
        elif form == "fractions" and self.jacobian:
            be.lw_solver_noscat_fractions_jac(top, kd, sec, wts, tau, buf, emis, flux_up=F[0], flux_dn=F[1], flux_up_jac=J)
        elif form == "fractions":
            be.lw_solver_noscat_fractions(top, kd, sec, wts, tau, buf, emis, flux_up=F[0], flux_dn=F[1])
        else:
            be.lw_solver_noscat(top, sec, wts, tau, buf["lay_src"], buf["lev_src"], emis, buf["sfc_src"],
                                out=dict(flux_up=buf["gpt_up"], flux_dn=buf["gpt_dn"]))
        mark("lw_solver", True)
        mark("lw_reduce")
        if form == "per_gpoint":
            be.sum_broadband(buf["gpt_up"], out=F[0]); be.sum_broadband(buf["gpt_dn"], out=F[1])
        be.net_broadband_precalc(F[1], F[0], out=F[2])
        mark("lw_reduce", True)

    def _sw_chain(self, atm, col_dry, buf, alb_dir, alb_dif, F, BS, mcica, n_day=None):
        """The SW launches of a step on atm's columns, after the caller's mark("sw_gas_optics"): gas optics into buf, the solve, fluxes
        into F (up, dn, dir, net) and with byband into BS. mcica as in _lw_chain. n_day: atm holds the sunlit columns only (n_day of
        them, padded), and F / BS are scattered to the caller's arrays with zeros in the night columns; 0 = all dark, atm is not read."""
        be, kd, mark = self.be, self.kd_sw, self._mark
        if n_day == 0:                # all dark: no SW launches, only the zero fill
            mark("sw_gas_optics", True); mark("sw_solver"); mark("sw_solver", True); mark("sw_reduce")
            self._sunlit_scatter(0, 0, BS)
            mark("sw_reduce", True)
            return
        be.get_col_dry(atm.vmr["h2o"], atm.p_lev, out=col_dry)
        col_gas = be.fill_gases(kd, atm.vmr, col_dry)
        # clear sky: the asymmetry parameter is identically zero; the fused broadband solver takes "no g" natively
        gbuf = None if (self.g_zero and self.do_broadband) else buf["g"]
        cld = None
        if self.cloud_luts is not None:     # Radiation_solver.cu:773-792
            cld = be.cloud_optics_2str(self.cloud_luts[1], atm.lwp, atm.iwp, atm.rel, atm.dei, delta_scale=True)
        # all-sky: the by-band cloud properties are added where the gas optics is stored; McICA adds them afterwards, cell by cell
        be.gas_optics_sw_direct(kd, atm.p_lay, atm.t_lay, col_gas, col_dry, buf["tau"], buf["ssa"], gbuf, by_band=cld if mcica is None else None)
        toa = be.toa_source(atm.ncol, kd.solar_source, atm.tsi_scaling)     # spread_col + scaling_to_subset, one launch
        if cld is not None and mcica is not None:
            be.mcica_increment_2stream(buf["tau"], buf["ssa"], gbuf, *cld, kd.band_lims_gpt, mcica[0], mcica[1], self.mcica_seed, 1, mcica[2],
                                       self.mcica_col_offset)
        mark("sw_gas_optics", True)
        mark("sw_solver")
        be.expand_and_transpose(kd.band_lims_gpt, atm.sfc_alb_dir, kd.ngpt, out=alb_dir)
        be.expand_and_transpose(kd.band_lims_gpt, atm.sfc_alb_dif, kd.ngpt, out=alb_dif)
        mu0_lay = getattr(atm, "mu0_lay", None)      # (a field of the step's view: None without mu0_lay= / altitude=)
        if self.altitude is not None:     # the sun rises with altitude: this step's cosines from the current mu0
            mu0_lay = be.zenith_angle_spherical_correction(atm.mu0, atm.altitude, atm.ref_altitude, self.planet_radius,
                                                           out=self._cols(self.mu0_lay_step, atm.ncol))
        if self.do_broadband:
            out = dict(flux_up=F[0], flux_dn=F[1], flux_dir=F[2])
        else:
            out = dict(flux_up=buf["gpt_up"], flux_dn=buf["gpt_dn"], flux_dir=buf["gpt_dir"])
        if self.byband:
            out.update(bnd_flux_up=BS[0], bnd_flux_dn=BS[1], bnd_flux_dir=BS[2], bnd_flux_net=BS[3])
        top, tau, ssa = atm.top_at_1, buf["tau"], buf["ssa"]
        if mu0_lay is not None and self.byband:
            be.sw_solver_2stream_byband_mu0lay(top, tau, ssa, gbuf, mu0_lay, alb_dir, alb_dif, toa, kd.band_lims_gpt, out=out)
        elif mu0_lay is not None:
            be.sw_solver_2stream_mu0lay(top, tau, ssa, gbuf, mu0_lay, alb_dir, alb_dif, toa, do_broadband=self.do_broadband, out=out)
        elif self.byband:
            be.sw_solver_2stream_byband(top, tau, ssa, gbuf, atm.mu0, alb_dir, alb_dif, toa, kd.band_lims_gpt, out=out)
        else:
            be.sw_solver_2stream(top, tau, ssa, gbuf, atm.mu0, alb_dir, alb_dif, toa, do_broadband=self.do_broadband, out=out)
        mark("sw_solver", True)
        mark("sw_reduce")
        if not self.do_broadband:
            be.sum_broadband(buf["gpt_up"], out=F[0]); be.sum_broadband(buf["gpt_dn"], out=F[1]); be.sum_broadband(buf["gpt_dir"], out=F[2])
        be.net_broadband_precalc(F[1], F[0], out=F[3])
        if n_day is not None:                 # back to the caller's columns, zeros in the night ones
            self._sunlit_scatter(n_day, atm.ncol, BS)
        mark("sw_reduce", True)

    def _sunlit_scatter(self, n_day, n_out, BSd):
        """SW fluxes of the sunlit columns (sun_fluxes, BSd: n_out columns in sun_perm order) into the caller's arrays, zeros elsewhere."""
        be = self.be
        be.scatter_cols_fill(n_day, self.sun_perm, self._cols(self.sun_fluxes, n_out), self.fluxes[3:7])
        if self.byband:
            be.scatter_cols_fill(n_day, self.sun_perm, BSd, self.bnd_sw)

