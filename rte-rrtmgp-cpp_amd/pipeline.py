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
import ctypes
import os
import time

import numpy as np

from ._ffi import BoolArg

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


def raytrace_sw(be, kd_sw, atm, nx, ny, dx, dy, dz, azimuth, photons_per_pixel, seed, cloud_lut=None, kn_grid=None,
                independent_column=False, sfc_albedo=None, max_events=None):
    """3-D shortwave surface / top fluxes and absorption from the forward Monte Carlo ray tracer (rrx_raytracer_sw).

    The atmosphere's columns are the pixels of an nx x ny domain (column = ix + nx iy) of cells dx x dy x dz metres, periodic in x
    and y, under one sun: mu0 and tsi_scaling must be the same in every column. The clear per-g-point SW gas optics and (with
    cloud_lut) the band cloud optics, not delta-scaled, feed the tracer; inc_dir[g] = solar_source[g] tsi_scaling mu0, no diffuse
    incident flux. azimuth: direction of travel of the direct beam, radians from +x. kn_grid = (knx, kny, knz) dividing (nx, ny,
    nlay), default one block per cell. sfc_albedo (ncol,): default the atmosphere's, which must then be the same in every band and
    for direct and diffuse light (the tracer's surface is Lambertian with one broadband albedo per pixel).
    Returns sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up (ncol,) in W m-2, abs_dir, abs_dif (nlay, ncol) in W m-3 and n_capped."""
    ncol, nlay, ngpt = atm.ncol, atm.nlay, kd_sw.ngpt
    if ncol != nx*ny:
        raise ValueError(f"raytrace_sw: ncol = {ncol} is not nx ny = {nx}*{ny}")
    mu0 = be.to_numpy(atm.mu0).reshape(-1)
    tsi = be.to_numpy(atm.tsi_scaling).reshape(-1)
    if np.any(mu0 != mu0[0]) or np.any(tsi != tsi[0]):
        raise ValueError("raytrace_sw: mu0 and tsi_scaling must be the same in every column (one sun for the domain)")
    if sfc_albedo is None:
        a_dir, a_dif = be.to_numpy(atm.sfc_alb_dir), be.to_numpy(atm.sfc_alb_dif)
        if np.any(a_dir != a_dif) or np.any(a_dif != a_dif[:, :1]):
            raise ValueError("raytrace_sw: the atmosphere's albedo differs between bands or between direct and diffuse; pass sfc_albedo")
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
    return be.raytracer_sw(tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, float(mu0[0]), azimuth, inc_dir, np.zeros_like(inc_dir), kn_grid,
                           photons_per_pixel, seed, top_at_1=atm.top_at_1, independent_column=independent_column, cloud=cld,
                           band_lims=kd_sw.band_lims_gpt, max_events=max_events)


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


class ResidentSolver:
    """One full clear-sky LW+SW solve per ``step()`` with every buffer allocated once (what a host model keeps
    resident between radiation calls, cf. the cached subsets in /root/reference/src_test/Radiation_solver.cu:450-466).
    HIP backend only; used by bench.py and the full-size tests. ``stage_events`` (torch.cuda.Event pairs on the
    launch stream) give per-stage device durations without synchronising inside the step."""

    STAGES = ("lw_gas_optics", "lw_planck", "lw_solver", "lw_reduce", "sw_gas_optics", "sw_solver", "sw_reduce")

    def __init__(self, be, kd_lw, kd_sw, atm, do_broadband=False, overlap=False, cloud_luts=None, sort_columns=None, byband=False,
                 sunlit=False, jacobian=False, n_gauss_angles=1, optimal_angles=False, keep_secants=False, lw_scattering=False,
                 lw_rescaling=False, cloud_fraction=None, cloud_overlap="max_ran", overlap_param=None, mcica_seed=0, mcica_col_offset=0,
                 mu0_lay=None, altitude=None, ref_altitude=None, planet_radius=6.37123e6):
        import torch
        self.torch = torch
        # mu0 by layer: the SW solver takes a cosine of the solar zenith angle per layer. mu0_lay: (nlay, ncol) in the
        # caller's column order, used as it is. altitude: (nlay, ncol) layer altitudes in metres, with ref_altitude (ncol, default 0) the
        # altitude at which atm.mu0 holds: every step forms mu0_lay on the device from the current atm.mu0 by the spherical-geometry
        # correction (zenith_angle_spherical_correction). The fields stay attributes: replace or update them between steps. They are
        # per-column fields (_COLUMN_FIELDS): sorted, padded and gathered to the sunlit columns with the others. The sunlit list is
        # made from atm.mu0 in either case; the LW chain does not see any of this.
        self.mu0_lay, self.altitude, self.ref_altitude, self.planet_radius = mu0_lay, altitude, ref_altitude, float(planet_radius)
        if mu0_lay is not None and altitude is not None:
            raise ValueError("ResidentSolver: mu0_lay and altitude are two ways to the same thing: give one")
        if ref_altitude is not None and altitude is None:
            raise ValueError("ResidentSolver: ref_altitude without altitude")
        for name, v, want in (("mu0_lay", mu0_lay, (atm.nlay, atm.ncol)), ("altitude", altitude, (atm.nlay, atm.ncol)),
                              ("ref_altitude", ref_altitude, (atm.ncol,))):
            if v is not None and tuple(v.shape) != want:
                raise ValueError(f"ResidentSolver: {name} {tuple(v.shape)} is not {want}")
        if altitude is not None and bool((altitude < (0. if ref_altitude is None else ref_altitude)).any()):
            raise ValueError("ResidentSolver: an altitude lies below its column's reference altitude")
        # cloud_fraction: McICA cloud sampling. (nlay, ncol) cloud fractions in the caller's column order; each step runs
        # the CLEAR gas optics and then rrx_mcica_increment_*, which gives every g-point its own sub-column and adds the band cloud
        # properties in the cloudy cells only. cloud_overlap: "max_ran", or "exp_ran" with overlap_param (nlay-1, ncol), the overlap
        # parameter between array layers l and l+1. The mask is redrawn every step from the current self.mcica_seed (a host advances it
        # between calls; domain 0 = LW, 1 = SW); a column's draws are keyed by mcica_col_offset + its index in the caller's order, so
        # sorting, padding and sharding do not change them. The fields stay attributes: replace or update them between steps.
        self.cloud_fraction, self.overlap_param = cloud_fraction, overlap_param
        self.mcica_seed, self.mcica_col_offset = int(mcica_seed), int(mcica_col_offset)
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
            if tuple(cloud_fraction.shape) != (atm.nlay, atm.ncol):
                raise ValueError(f"ResidentSolver: cloud_fraction {tuple(cloud_fraction.shape)} is not (nlay, ncol) = {(atm.nlay, atm.ncol)}")
            if overlap_param is not None and tuple(overlap_param.shape) != (atm.nlay-1, atm.ncol):
                raise ValueError(f"ResidentSolver: overlap_param {tuple(overlap_param.shape)} is not (nlay-1, ncol) = {(atm.nlay-1, atm.ncol)}")
            for flag, name in ((lw_scattering, "lw_scattering=True"), (lw_rescaling, "lw_rescaling=True"), (sunlit, "sunlit=True")):
                if flag:
                    raise ValueError(f"ResidentSolver: cloud_fraction with {name} is not supported (the scattering LW solvers combine "
                                     "the band clouds themselves; the sunlit-only SW chain does not carry the column identities)")
        # lw_rescaling: the LW chain treats cloud scattering by rescaling -- clear gas optics, LW cloud tau / ssa / g by band
        # (cloud_optics_2str on the LW table, not delta-scaled) and the fused no-scattering solve on rescaled optical depths with one
        # correction sweep (lw_solver_noscat_fractions_rescaled); without cloud LUTs the same solver with ssa = 0. One angle, broadband:
        # no by-band form, no Jacobian, no several or optimal angles, and not together with lw_scattering.
        self.lw_rescaling = bool(lw_rescaling)
        if self.lw_rescaling:
            for flag, name in ((lw_scattering, "lw_scattering=True"), (byband, "byband=True"), (jacobian, "jacobian=True"),
                               (int(n_gauss_angles) > 1, "n_gauss_angles > 1"), (optimal_angles, "optimal_angles=True")):
                if flag:
                    raise ValueError(f"ResidentSolver: lw_rescaling=True with {name} is not supported (the rescaled LW solver has "
                                     "one broadband form with one fixed angle)")
        # lw_scattering: the LW chain lets clouds scatter -- clear gas optics, LW cloud tau / ssa / g by band (cloud_optics_2str on the LW
        # table, not delta-scaled) and the fused two-stream solver (lw_solver_2stream_fractions); without cloud LUTs the same solver with
        # ssa = 0. One solve without quadrature angles: no by-band form, no Jacobian, no several or optimal angles.
        self.lw_scattering = bool(lw_scattering)
        if self.lw_scattering:
            for flag, name in ((byband, "byband=True"), (jacobian, "jacobian=True"), (int(n_gauss_angles) > 1, "n_gauss_angles > 1"),
                               (optimal_angles, "optimal_angles=True")):
                if flag:
                    raise ValueError(f"ResidentSolver: lw_scattering=True with {name} is not supported (the two-stream LW solver has "
                                     "one broadband form without quadrature angles)")
        # byband: the step also fills self.bnd_fluxes (lw_up/lw_dn/lw_net/sw_up/sw_dn/sw_dir/sw_net, (nbnd, nlev, ncol) each, the
        # caller's column order) from the fused solvers' by-band form; the seven broadband arrays come from the same solves
        self.byband = bool(byband)
        # jacobian: the step also fills self.lw_flux_up_jac (nlev, ncol, the caller's column order), the surface-temperature Jacobian
        # of the LW upward flux [W m-2 K-1] from the same fused solve; the seven broadband arrays stay bit for bit those without it
        self.jacobian = bool(jacobian)
        # n_gauss_angles: LW quadrature angles (1..4, Gauss-Jacobi-5 nodes); more than one takes the several-angle form of the fused
        # solver (lw_solver_noscat_fractions_angles), which has no by-band outputs
        self.n_gauss_angles = int(n_gauss_angles)
        if not 1 <= self.n_gauss_angles <= 4:
            raise ValueError(f"ResidentSolver: n_gauss_angles = {n_gauss_angles} is outside 1..4")
        if self.n_gauss_angles > 1 and self.byband:
            raise ValueError("ResidentSolver: byband=True with n_gauss_angles > 1 is not supported (no by-band form with several angles)")
        if self.jacobian and self.byband:
            raise ValueError("ResidentSolver: jacobian=True with byband=True is not supported (no by-band Jacobians)")
        # optimal_angles: the one LW angle's secant is the k-distribution's optimal-angle fit of the column's total optical depth per
        # g-point (upstream's compute_optimal_angles / lw_Ds), formed inside the fused solver (lw_solver_noscat_fractions_optimal);
        # keep_secants: the step also fills self.lw_secants (ngpt, ncol of the step), the secants that solve used
        self.optimal_angles = bool(optimal_angles)
        self.keep_secants = bool(keep_secants) and self.optimal_angles
        if self.optimal_angles:
            if self.n_gauss_angles > 1:
                raise ValueError("ResidentSolver: optimal_angles=True with n_gauss_angles > 1 is not supported (optimal angles are one angle)")
            if self.byband:
                raise ValueError("ResidentSolver: optimal_angles=True with byband=True is not supported (no by-band form with optimal angles)")
            if getattr(kd_lw, "optimal_angle_fit", None) is None:
                raise ValueError("ResidentSolver: optimal_angles=True needs a LW k-distribution with optimal_angle_fit")
        # Column sorting. The windowed gas optics stages ONE box of LUT nodes per 256 neighbouring cells; columns
        # that differ much in pressure (RFMIP-like sites, --col-spread) do not fit one box and fall back to the gather kernels
        # (+40 % per step at +-35 % pressure spread). Columns are independent, so the step may process them in any order: sorted by
        # surface pressure, neighbours are alike again. The inputs are gathered into sorted order at the top of the step and the seven
        # broadband flux arrays scattered back at its end (0.5 ms per step at C4: ~30 gathers of (nlay, ncol) arrays). "auto" (default,
        # or RRX_SORT_COLUMNS): decided once from the initial atmosphere -- on when the surface pressure varies by more than 20 % inside
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
        # Padding (round 4): the step runs on a multiple of 16 columns -- the rows of the (col, lay, gpt) intermediates then start on
        # 128-B lines (16 385 columns cost 20 % more than 16 384 otherwise); the extra columns repeat the last one and are dropped
        # when the fluxes go back to the caller's order. One gather index serves both (built once, not per step, and
        # applied to an explicit list of per-column fields): refresh_column_order() rebuilds it when the host model's pressures
        # have changed enough to matter.
        pad = bool(int(os.environ.get("RRX_PAD_COLUMNS", "1"))) and atm.ncol > 16 and atm.ncol % 16 != 0
        self.npad = (16 - atm.ncol % 16) if pad else 0
        self.ncol_caller = atm.ncol
        self.perm = None
        self.atm = atm
        if self.sort_columns or self.npad:
            self.refresh_column_order()
        # overlap: LW and SW chains are independent, so they can run on two HIP streams and share the chip (the gather-
        # bound gas-optics kernels of one chain fill in next to the HBM-bound solver of the other)
        self.overlap = overlap
        self.streams = [torch.cuda.Stream(device=be.device), torch.cuda.Stream(device=be.device)] if overlap else None
        self.be, self.kd_lw, self.kd_sw, self.atm = be, kd_lw, kd_sw, atm
        self.do_broadband = do_broadband
        # all-sky (BASELINE C5): (lw_lut, sw_lut) of cloud optics; clouds are added by band after the gas optics, delta-scaled in SW
        self.cloud_luts = cloud_luts
        self.fuse_clouds = bool(int(os.environ.get("RRX_FUSE_CLOUDS", "1")))
        self.g_zero = cloud_luts is None and bool(int(os.environ.get("RRX_G_ZERO", "1")))     # clear sky: g == 0 is neither written nor read
        self.direct = bool(int(os.environ.get("RRX_DIRECT", "1")))     # interpolation state recomputed inside its consumers
        # broadband mode: Planck fractions + band Planck functions, sources formed inside the LW solver ("Planck-lite" chain)
        self.lite = self.direct and do_broadband and bool(int(os.environ.get("RRX_LITE", "1")))
        if self.byband and not self.lite:
            raise ValueError("ResidentSolver(byband=True) needs do_broadband=True and the Planck-lite chain (RRX_DIRECT, RRX_LITE)")
        if self.jacobian and not self.lite:
            raise ValueError("ResidentSolver(jacobian=True) needs do_broadband=True and the Planck-lite chain (RRX_DIRECT, RRX_LITE)")
        if self.lw_rescaling and not self.lite:
            raise ValueError("ResidentSolver(lw_rescaling=True) needs do_broadband=True and the Planck-lite chain (RRX_DIRECT, RRX_LITE)")
        if self.lw_scattering and not self.lite:
            raise ValueError("ResidentSolver(lw_scattering=True) needs do_broadband=True and the Planck-lite chain (RRX_DIRECT, RRX_LITE)")
        if self.optimal_angles and not self.lite:
            raise ValueError("ResidentSolver(optimal_angles=True) needs do_broadband=True and the Planck-lite chain (RRX_DIRECT, RRX_LITE)")
        ncol, nlay = atm.ncol + self.npad, atm.nlay              # columns of a step (padded)
        ng_l, ng_s = kd_lw.ngpt, kd_sw.ngpt
        e = be.empty
        self.col_dry = e((nlay, ncol))
        if self.lite:
            self.lw = dict(tau=e((ng_l, nlay, ncol)), pfrac=e((ng_l, nlay, ncol)), blay=e((kd_lw.nbnd, nlay, ncol)),
                           blev=e((kd_lw.nbnd, nlay+1, ncol)), sfc_src=e((ng_l, ncol)), sfc_src_jac=e((ng_l, ncol)))
        else:
            self.lw = dict(tau=e((ng_l, nlay, ncol)), lay_src=e((ng_l, nlay, ncol)), lev_src=e((ng_l, nlay+1, ncol)),
                           sfc_src=e((ng_l, ncol)), sfc_src_jac=e((ng_l, ncol)))
        self.sw = dict(tau=e((ng_s, nlay, ncol)), ssa=e((ng_s, nlay, ncol)), g=e((ng_s, nlay, ncol)))
        if not do_broadband:
            self.lw.update(gpt_up=e((ng_l, nlay+1, ncol)), gpt_dn=e((ng_l, nlay+1, ncol)))
            self.sw.update(gpt_up=e((ng_s, nlay+1, ncol)), gpt_dn=e((ng_s, nlay+1, ncol)), gpt_dir=e((ng_s, nlay+1, ncol)))
        # packed broadband outputs: LW up/dn/net + SW up/dn/dir/net  (7, nlev, ncol) -> one all-gather
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
        # sunlit-only SW: every step lists the columns with mu0 > 0 on the device (in the step's own column order), gathers the SW
        # inputs of those columns into the buffers below, runs the SW chain on that many columns (views of the full-size SW buffers)
        # and scatters the SW fluxes back with zeros in the night columns. The host needs the count to size the launches: it is
        # copied to pinned memory at the top of the step and waited for only once the LW chain has been enqueued. All columns
        # sunlit: the plain SW path, bit for bit.
        self.sunlit = bool(sunlit)
        if self.sunlit:
            # (padded to a multiple of 16 like the plain step: at most ncol rounded up to 16, which the step's buffers hold)
            self.sun_pad = 16 if (bool(int(os.environ.get("RRX_PAD_COLUMNS", "1"))) and atm.ncol > 16) else 1
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
        self.events = None
        self.col_dry2 = None

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
        from .synthetic import Atmosphere
        be, a, perm = self.be, self._step_atmosphere(), self.sun_perm
        out = dict(a.__dict__)         # (fields the SW chain does not read stay as they are)
        out["ncol"] = n_out
        for k, buf in self.sun_in.items():
            v = getattr(a, k, None)
            if v is None:                  # (a field of the solver's that the host has taken away since)
                continue
            if self._COLUMN_FIELDS[k] < 0 or v.dim() == 1:        # column fastest: (..., ncol) or (ncol,)
                o = self._cols(buf, n_out) if self._COLUMN_FIELDS[k] < 0 else buf[:n_out]
                nrest = int(np.prod(v.shape[:-1], dtype=np.int64)) if v.dim() > 1 else 1
                be._c("gather_cols", n_out, ctypes.c_ulonglong(nrest), perm, a.ncol, v, o)
            else:                                                  # column slowest: (ncol, nbnd)
                o = self._rows(buf, n_out)
                be._c("gather_lastdim", int(v.shape[1]), n_out, perm, v, o)
            out[k] = o
        vmr = {}
        for n, t in a.vmr.items():
            if n in self.sun_vmr:
                o = self._cols(self.sun_vmr[n], n_out)
                be._c("gather_cols", n_out, ctypes.c_ulonglong(t.shape[0]), perm, a.ncol, t, o)
                vmr[n] = o
            else:
                vmr[n] = t
        out["vmr"] = vmr
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
        from .synthetic import Atmosphere
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

    def step(self):
        be, atm = self.be, self._step_atmosphere()
        perm = self.perm
        if perm is not None:
            atm = self._gathered_atmosphere()
        if self.overlap and self.col_dry2 is None:
            self.col_dry2 = be.empty(tuple(self.col_dry.shape))
        rec = None
        if self.events is not None and self._istep < len(self.events):
            rec = self.events[self._istep]
            self._istep += 1

        def mark(stage, end=False):
            if rec is not None:
                rec[stage][1 if end else 0].record(self.torch.cuda.current_stream(be.device))   # the chain's stream when overlapping

        ncol, nlay = atm.ncol, atm.nlay
        mcica = self.cloud_fraction is not None
        if mcica:     # the sampled fields in the step's column order, and the identities that go with it
            cfrac, alpha = self.cloud_fraction, self.overlap_param
            col_id = None
            if perm is not None:
                cfrac = cfrac.index_select(1, perm)
                alpha = None if alpha is None else alpha.index_select(1, perm)
                col_id = self.perm_i32 + self.mcica_col_offset
        F = self.fluxes if perm is None else self.fluxes_sorted
        J = self.lw_flux_up_jac if perm is None else self.jac_sorted
        BL = self.bnd_lw if perm is None else self.bnd_lw_sorted
        BS = self.bnd_sw if perm is None else self.bnd_sw_sorted
        main = self.torch.cuda.current_stream(be.device)
        sw_day = False                # this step's SW chain runs on the sunlit columns only
        if self.sunlit:               # the column list and its count, on the device; the count travels to pinned host memory
            n = self.ncol_caller
            be.sunlit_columns(self.atm.mu0, None if perm is None else self.perm_i32[:n], self.sun_pad, perm=self.sun_perm, count=self.sun_count)
            self.sun_count_host.copy_(self.sun_count, non_blocking=True)
            self.sun_event.record(main)
        for ichain, (kind, kd, buf) in enumerate((("lw", self.kd_lw, self.lw), ("sw", self.kd_sw, self.sw))):
            if self.overlap:
                self.streams[ichain].wait_stream(main)
                ctx = self.torch.cuda.stream(self.streams[ichain])
                ctx.__enter__()
            mark(kind + "_gas_optics")
            col_dry = self.col_dry2 if (self.overlap and ichain == 1) else self.col_dry
            if kind == "sw" and self.sunlit:
                t0 = time.perf_counter()
                self.sun_event.synchronize()      # the LW chain is enqueued by now; the count was ready long before
                self.sun_wait_ms += (time.perf_counter() - t0) * 1e3
                n_day = int(self.sun_count_host[0])
                sw_day = n_day < self.ncol_caller
                if sw_day:
                    n_out = -(-n_day // self.sun_pad) * self.sun_pad
                    FS = [None, None, None] + list(self._cols(self.sun_fluxes, n_out))
                    BSd = self._cols(self.sun_bnd, n_out) if self.byband else None
                    if n_day == 0:                # all dark: no SW launches, only the zero fill
                        mark("sw_gas_optics", True); mark("sw_solver"); mark("sw_solver", True); mark("sw_reduce")
                        self._sunlit_scatter(0, 0, BSd)
                        mark("sw_reduce", True)
                        if self.overlap:
                            ctx.__exit__(None, None, None)
                        continue
                    atm_full, ncol_full = atm, ncol
                    atm, ncol = self._sunlit_atmosphere(n_out), n_out
                    col_dry = self._cols(col_dry, n_out)
                    buf = {k: self._cols(v, n_out) for k, v in buf.items()}
                    alb_dir, alb_dif = self._cols(self.alb_dir, n_out), self._cols(self.alb_dif, n_out)
                    F_full, BS_full = F, BS
                    F, BS = FS, BSd
            be._c("get_col_dry", ncol, nlay, atm.vmr["h2o"], atm.p_lev, col_dry)
            col_gas = be.fill_gases(kd, atm.vmr, col_dry)
            it = None if self.direct else be.interpolation(kd, atm.p_lay, atm.t_lay, col_gas)
            # all-sky: the by-band cloud properties are computed first and added where the gas optics is stored (fused); with
            # RRX_FUSE_CLOUDS=0 by the reference's separate increment kernels afterwards
            fuse = self.cloud_luts is not None and self.direct and self.fuse_clouds and not mcica
            if kind == "lw":
                tc = cld_lw = None
                if self.cloud_luts is not None and (self.lw_scattering or self.lw_rescaling):      # tau, ssa, g by band: the solver combines them itself
                    cld_lw = be.cloud_optics_2str(self.cloud_luts[0], atm.lwp, atm.iwp, atm.rel, atm.dei)
                elif self.cloud_luts is not None:     # /root/reference/src_test/Radiation_solver.cu:497-512
                    tc = be.cloud_optics_1scl(self.cloud_luts[0], atm.lwp, atm.iwp, atm.rel, atm.dei)
                if self.lite:
                    be.gas_optics_lw_fractions(kd, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, _sfc_lay(atm), col_gas, buf["tau"], out=buf,
                                               by_band=tc if fuse else None)
                elif self.direct:
                    be.gas_optics_lw_direct(kd, atm.p_lay, atm.t_lay, col_gas, buf["tau"], by_band=tc if fuse else None)
                else:
                    be.compute_tau_absorption_set(kd, it, atm.p_lay, atm.t_lay, col_gas, buf["tau"])
                if tc is not None and mcica:
                    be.mcica_increment_1scalar(buf["tau"], tc, kd.band_lims_gpt, cfrac, alpha, self.mcica_seed, 0, col_id, self.mcica_col_offset)
                elif tc is not None and not fuse:
                    be.inc_1scalar_by_1scalar_bybnd(buf["tau"], tc, kd.band_lims_gpt)
                mark("lw_gas_optics", True)
                mark("lw_planck")
                srcs = None if self.lite else dict(sfc_src=buf["sfc_src"], lay_src=buf["lay_src"], lev_src=buf["lev_src"], sfc_src_jac=buf["sfc_src_jac"])
                if self.lite:
                    pass                                   # the fractions came with the optical depths
                elif self.direct:
                    be.planck_source_direct(kd, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, _sfc_lay(atm), col_gas, out=srcs)
                else:
                    be.compute_planck_source(kd, it, atm.t_lay, atm.t_lev, atm.t_sfc, _sfc_lay(atm), out=srcs)
                mark("lw_planck", True)
                mark("lw_solver")
                if not (self.optimal_angles or self.lw_scattering):      # (neither solver reads a secants array)
                    be._c("lw_secants_array", ncol, kd.ngpt, self.n_gauss_angles, MAX_GAUSS_PTS, self.gauss_Ds, self.secants)
                be._c("expand_and_transpose", ncol, kd.nbnd, kd.band_lims_gpt, atm.emis_sfc, self.sfc_emis_gpt)
                if self.lw_rescaling:
                    be.lw_solver_noscat_fractions_rescaled(atm.top_at_1, kd, self.secants, self.weights, buf["tau"], buf, self.sfc_emis_gpt,
                                                           cloud=cld_lw, flux_up=F[0], flux_dn=F[1])
                elif self.lw_scattering:
                    be.lw_solver_2stream_fractions(atm.top_at_1, kd, buf["tau"], buf, self.sfc_emis_gpt, cloud=cld_lw,
                                                   flux_up=F[0], flux_dn=F[1])
                elif self.optimal_angles:
                    be.lw_solver_noscat_fractions_optimal(atm.top_at_1, kd, self.weights, buf["tau"], buf, self.sfc_emis_gpt,
                                                          fit=self.optimal_fit, flux_up=F[0], flux_dn=F[1], flux_up_jac=J,
                                                          jacobian=self.jacobian, secants_out=self.lw_secants)
                elif self.byband:
                    be.lw_solver_noscat_fractions_byband(atm.top_at_1, kd, self.secants, self.weights, buf["tau"], buf, self.sfc_emis_gpt,
                                                         out=dict(bnd_flux_up=BL[0], bnd_flux_dn=BL[1], bnd_flux_net=BL[2],
                                                                  flux_up=F[0], flux_dn=F[1]))
                elif self.lite and self.n_gauss_angles > 1:
                    be.lw_solver_noscat_fractions_angles(atm.top_at_1, kd, self.secants, self.weights, buf["tau"], buf, self.sfc_emis_gpt,
                                                         flux_up=F[0], flux_dn=F[1], flux_up_jac=J, jacobian=self.jacobian)
                elif self.jacobian:
                    be.lw_solver_noscat_fractions_jac(atm.top_at_1, kd, self.secants, self.weights, buf["tau"], buf, self.sfc_emis_gpt,
                                                      flux_up=F[0], flux_dn=F[1], flux_up_jac=J)
                elif self.lite:
                    be.lw_solver_noscat_fractions(atm.top_at_1, kd, self.secants, self.weights, buf["tau"], buf, self.sfc_emis_gpt,
                                                  flux_up=F[0], flux_dn=F[1])
                elif self.do_broadband:
                    be._c("lw_solver_noscat", ncol, nlay, kd.ngpt, BoolArg(atm.top_at_1), self.n_gauss_angles, self.secants, self.weights,
                          buf["tau"], buf["lay_src"], buf["lev_src"], self.sfc_emis_gpt, buf["sfc_src"], None, None, None,
                          BoolArg(True), F[0], F[1], BoolArg(False), None, None)
                else:
                    be.lw_solver_noscat_into(atm.top_at_1, self.secants, self.weights, buf["tau"], buf["lay_src"],
                                             buf["lev_src"], self.sfc_emis_gpt, buf["sfc_src"], buf["gpt_up"], buf["gpt_dn"])
                mark("lw_solver", True)
                mark("lw_reduce")
                if not self.do_broadband:
                    be.sum_broadband(buf["gpt_up"], out=F[0]); be.sum_broadband(buf["gpt_dn"], out=F[1])
                be.net_broadband_precalc(F[1], F[0], out=F[2])
                mark("lw_reduce", True)
            else:
                if not sw_day:
                    alb_dir, alb_dif = self.alb_dir, self.alb_dif
                # clear sky: the asymmetry parameter is identically zero; the fused broadband solver takes "no g" natively
                gbuf = None if (self.g_zero and self.do_broadband) else buf["g"]
                cld = None
                if self.cloud_luts is not None:     # Radiation_solver.cu:773-792
                    cld = be.cloud_optics_2str(self.cloud_luts[1], atm.lwp, atm.iwp, atm.rel, atm.dei, delta_scale=True)
                if self.direct:
                    be.gas_optics_sw_direct(kd, atm.p_lay, atm.t_lay, col_gas, col_dry, buf["tau"], buf["ssa"], gbuf, by_band=cld if fuse else None)
                else:
                    be.gas_optics_sw_fused(kd, it, atm.p_lay, atm.t_lay, col_gas, col_dry, buf["tau"], buf["ssa"], gbuf)
                toa = be.toa_source(ncol, kd.solar_source, atm.tsi_scaling)     # spread_col + scaling_to_subset, one launch
                if cld is not None and mcica:
                    be.mcica_increment_2stream(buf["tau"], buf["ssa"], gbuf, *cld, kd.band_lims_gpt, cfrac, alpha, self.mcica_seed, 1, col_id,
                                               self.mcica_col_offset)
                elif cld is not None and not fuse:
                    be.inc_2stream_by_2stream_bybnd(buf["tau"], buf["ssa"], gbuf, *cld, kd.band_lims_gpt)
                mark("sw_gas_optics", True)
                mark("sw_solver")
                be._c("expand_and_transpose", ncol, kd.nbnd, kd.band_lims_gpt, atm.sfc_alb_dir, alb_dir)
                be._c("expand_and_transpose", ncol, kd.nbnd, kd.band_lims_gpt, atm.sfc_alb_dif, alb_dif)
                mu0_lay = getattr(atm, "mu0_lay", None)      # (a field of the step's view: None without mu0_lay= / altitude=)
                if self.altitude is not None:     # the sun rises with altitude: this step's cosines from the current mu0
                    mu0_lay = be.zenith_angle_spherical_correction(atm.mu0, atm.altitude, atm.ref_altitude, self.planet_radius,
                                                                   out=self._cols(self.mu0_lay_step, ncol))
                if mu0_lay is not None and self.byband:
                    be.sw_solver_2stream_byband_mu0lay(atm.top_at_1, buf["tau"], buf["ssa"], gbuf, mu0_lay, alb_dir, alb_dif, toa,
                                                       kd.band_lims_gpt, out=dict(bnd_flux_up=BS[0], bnd_flux_dn=BS[1], bnd_flux_dir=BS[2],
                                                                                  bnd_flux_net=BS[3], flux_up=F[3], flux_dn=F[4], flux_dir=F[5]))
                elif mu0_lay is not None:
                    be.sw_solver_2stream_mu0lay(atm.top_at_1, buf["tau"], buf["ssa"], gbuf, mu0_lay, alb_dir, alb_dif, toa,
                                                do_broadband=self.do_broadband,
                                                out=dict(flux_up=F[3], flux_dn=F[4], flux_dir=F[5]) if self.do_broadband else
                                                dict(flux_up=buf["gpt_up"], flux_dn=buf["gpt_dn"], flux_dir=buf["gpt_dir"]))
                elif self.byband:
                    be.sw_solver_2stream_byband(atm.top_at_1, buf["tau"], buf["ssa"], gbuf, atm.mu0, alb_dir, alb_dif, toa,
                                                kd.band_lims_gpt, out=dict(bnd_flux_up=BS[0], bnd_flux_dn=BS[1], bnd_flux_dir=BS[2],
                                                                           bnd_flux_net=BS[3], flux_up=F[3], flux_dn=F[4], flux_dir=F[5]))
                elif self.do_broadband:
                    be._c("sw_solver_2stream", ncol, nlay, kd.ngpt, BoolArg(atm.top_at_1), buf["tau"], buf["ssa"], gbuf, atm.mu0,
                          alb_dir, alb_dif, toa, None, None, None, BoolArg(False), None,
                          BoolArg(True), F[3], F[4], F[5])
                else:
                    be.sw_solver_2stream_into(atm.top_at_1, buf["tau"], buf["ssa"], gbuf, atm.mu0, alb_dir, alb_dif,
                                              toa, buf["gpt_up"], buf["gpt_dn"], buf["gpt_dir"])
                mark("sw_solver", True)
                mark("sw_reduce")
                if not self.do_broadband:
                    be.sum_broadband(buf["gpt_up"], out=F[3]); be.sum_broadband(buf["gpt_dn"], out=F[4]); be.sum_broadband(buf["gpt_dir"], out=F[5])
                be.net_broadband_precalc(F[4], F[3], out=F[6])
                if sw_day:                        # back to the caller's columns, zeros in the night ones
                    self._sunlit_scatter(n_day, ncol, BS)
                    atm, ncol, F, BS = atm_full, ncol_full, F_full, BS_full
                mark("sw_reduce", True)
            if self.overlap:
                ctx.__exit__(None, None, None)
        if self.overlap:
            main.wait_stream(self.streams[0]); main.wait_stream(self.streams[1])
        if perm is not None:                              # back to the caller's column order (padding columns dropped)
            n = self.ncol_caller
            nf = 3 if sw_day else 7                       # (a sunlit-only SW chain has written the caller's order already)
            self.fluxes[:nf].index_copy_(2, perm[:n], F[:nf, :, :n])
            F = self.fluxes
            if self.jacobian:
                self.lw_flux_up_jac.index_copy_(1, perm[:n], J[:, :n])
            if self.byband:
                self.bnd_lw.index_copy_(3, perm[:n], BL[..., :n])
                if not sw_day:
                    self.bnd_sw.index_copy_(3, perm[:n], BS[..., :n])
        return F

    def _sunlit_scatter(self, n_day, n_out, BSd):
        """SW fluxes of the sunlit columns (sun_fluxes, BSd: n_out columns in sun_perm order) into the caller's arrays, zeros elsewhere."""
        be = self.be
        be.scatter_cols_fill(n_day, self.sun_perm, self._cols(self.sun_fluxes, n_out), self.fluxes[3:7])
        if self.byband:
            be.scatter_cols_fill(n_day, self.sun_perm, BSd, self.bnd_sw)
