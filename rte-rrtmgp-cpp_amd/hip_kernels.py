"""Python view of the C ABI of librrx_hip.so (include/rrx_hip.h), operating on torch CUDA tensors.

This is plumbing for tests and bench.py: torch supplies device memory, streams and torch.distributed; every
number is produced by the hand-written HIP kernels behind the C ABI. There is NO CPU fallback: importing this
module without the built library, or calling it without a GPU, raises.

Array convention (see synthetic.py): tensors are C-contiguous with reversed dimensions, so their memory is the
reference's column-major layout, e.g. tau(ncol,nlay,ngpt) <-> tensor shape (ngpt, nlay, ncol).
"""
import ctypes
import os
import numpy as np
import torch

from ._ffi import Lib, PtrArg, HEADER_PATH
from .raytracer_args import RtScene

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librrx_hip.so")


def load_library():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The product path has no CPU fallback.")
    return ctypes.CDLL(LIB_PATH)


class HipKernels:
    """Backend object with the launcher-level interface used by pipeline.py (same method names as the
    test-only CPU backends in oracle/oracle_py.py)."""
    name = "hip"

    def __init__(self, dtype=np.float64, device="cuda:0", stream=None):
        if not torch.cuda.is_available():
            raise RuntimeError("HipKernels needs a GPU (no CPU fallback on the product path)")
        self.np_dtype = np.dtype(dtype)
        self.sfx = "_f64" if self.np_dtype == np.float64 else "_f32"
        self.tdtype = torch.float64 if self.np_dtype == np.float64 else torch.float32
        self.device = torch.device(device)
        load_library()
        # every call is checked against the entry's declaration in include/rrx_hip.h before it reaches the library (_ffi.py)
        self.lib = Lib(LIB_PATH, self.np_dtype, returns_status=True, header=HEADER_PATH,
                       error_fn=lambda: self.lib.call("rrx_last_error").decode())
        self.stream = stream          # torch.cuda.Stream or None (= torch current stream)

    # ---- memory helpers -------------------------------------------------------------------------
    def _st(self):
        s = self.stream if self.stream is not None else torch.cuda.current_stream(self.device)
        return PtrArg(s.cuda_stream)

    def asarray(self, a):
        if isinstance(a, torch.Tensor):
            return a
        a = np.ascontiguousarray(a)
        if a.dtype.kind == "f":
            a = a.astype(self.np_dtype)
        return torch.from_numpy(a).to(self.device)

    def to_numpy(self, t):
        return t.detach().cpu().numpy()

    def empty(self, shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.tdtype, device=self.device)

    def zeros(self, shape, dtype=None):
        return torch.zeros(shape, dtype=dtype or self.tdtype, device=self.device)

    def int_empty(self, shape):
        return torch.empty(shape, dtype=torch.int32, device=self.device)

    def bool_empty(self, shape):
        return torch.empty(shape, dtype=torch.int8, device=self.device)

    def synchronize(self):
        torch.cuda.synchronize(self.device)

    def upload_kdist(self, kd):
        from .synthetic import KDist
        out = {}
        for k, v in kd.__dict__.items():
            out[k] = self.asarray(v) if isinstance(v, np.ndarray) else v
        out["extras"] = {n: self.asarray(a) for n, a in kd.extras.items()}          # (optimal_angle_fit)
        return KDist(**out)

    def _c(self, name, *args):
        return self.lib.call("rrx_" + name + self.sfx, *args, self._st())

    # ---- solvers ----------------------------------------------------------------------------------
    def lw_secants_array(self, ncol, ngpt, n_quad, max_pts, gauss_Ds, out=None):
        out = self.empty((n_quad, ngpt, ncol)) if out is None else out
        self._c("lw_secants_array", ncol, ngpt, n_quad, max_pts, gauss_Ds, out)
        return out

    def _lw_noscat(self, entry, top_at_1, secants, weights, tau, scat, lay_source, lev_source, sfc_emis, sfc_src, inc_flux,
                   do_broadband, do_jacobians, sfc_src_jac, out):
        """The argument list of rrx_lw_solver_noscat and, with scat = (ssa, g), of its _rescaled twin. out=: preallocated flux_up /
        flux_dn [/ flux_up_jac]; the fluxes are (nlev, ncol) in broadband mode and (ngpt, nlev, ncol) otherwise."""
        ngpt, nlay, ncol = tau.shape
        if out is None:
            shape = (nlay+1, ncol) if do_broadband else (ngpt, nlay+1, ncol)
            out = dict(flux_up=self.empty(shape), flux_dn=self.empty(shape))
            if do_jacobians:
                out["flux_up_jac"] = self.empty((ngpt, nlay+1, ncol))
        fl = (out["flux_up"], out["flux_dn"])
        per_gpt, loc = ((None, None), fl) if do_broadband else (fl, (None, None))
        self._c(entry, ncol, nlay, ngpt, top_at_1, weights.shape[0], secants, weights, tau, *scat, lay_source, lev_source,
                sfc_emis, sfc_src, inc_flux, *per_gpt, do_broadband, *loc, do_jacobians, sfc_src_jac,
                out.get("flux_up_jac"))
        return out

    def lw_solver_noscat(self, top_at_1, secants, weights, tau, lay_source, lev_source, sfc_emis, sfc_src,
                         inc_flux=None, do_broadband=False, do_jacobians=False, sfc_src_jac=None, out=None):
        return self._lw_noscat("lw_solver_noscat", top_at_1, secants, weights, tau, (), lay_source, lev_source, sfc_emis, sfc_src,
                               inc_flux, do_broadband, do_jacobians, sfc_src_jac, out)

    def lw_solver_noscat_into(self, top_at_1, secants, weights, tau, lay_source, lev_source, sfc_emis, sfc_src,
                              flux_up, flux_dn):
        """Allocation-free form used inside timed regions."""
        self.lw_solver_noscat(top_at_1, secants, weights, tau, lay_source, lev_source, sfc_emis, sfc_src,
                              out=dict(flux_up=flux_up, flux_dn=flux_dn))

    def _sw_2stream(self, entry, top_at_1, tau, ssa, g, mu0, sfc_alb_dir, sfc_alb_dif, inc_flux_dir, inc_flux_dif, do_broadband, out):
        """The argument list of rrx_sw_solver_2stream and its _mu0lay twin (mu0 per column or per layer)."""
        ngpt, nlay, ncol = tau.shape
        if out is None:
            shape = (nlay+1, ncol) if do_broadband else (ngpt, nlay+1, ncol)
            out = {k: self.empty(shape) for k in ("flux_up", "flux_dn", "flux_dir")}
        fl = (out["flux_up"], out["flux_dn"], out["flux_dir"])
        per_gpt, loc = ((None, None, None), fl) if do_broadband else (fl, (None, None, None))
        self._c(entry, ncol, nlay, ngpt, top_at_1, tau, ssa, g, mu0, sfc_alb_dir, sfc_alb_dif, inc_flux_dir, *per_gpt,
                inc_flux_dif is not None, inc_flux_dif, do_broadband, *loc)
        return out

    def sw_solver_2stream(self, top_at_1, tau, ssa, g, mu0, sfc_alb_dir, sfc_alb_dif, inc_flux_dir,
                          inc_flux_dif=None, do_broadband=False, out=None):
        """g may be None (asymmetry identically zero). out=: preallocated flux_up/dn/dir, (nlev, ncol) in broadband mode and
        (ngpt, nlev, ncol) otherwise."""
        if mu0.dim() == 2:          # (nlay, ncol) CPU-style: the GPU boundary takes mu0(ncol)
            mu0 = mu0[0].contiguous()
        return self._sw_2stream("sw_solver_2stream", top_at_1, tau, ssa, g, mu0, sfc_alb_dir, sfc_alb_dif, inc_flux_dir, inc_flux_dif,
                                do_broadband, out)

    def sw_solver_2stream_into(self, top_at_1, tau, ssa, g, mu0, sfc_alb_dir, sfc_alb_dif, inc_flux_dir,
                               flux_up, flux_dn, flux_dir):
        self.sw_solver_2stream(top_at_1, tau, ssa, g, mu0, sfc_alb_dir, sfc_alb_dif, inc_flux_dir,
                               out=dict(flux_up=flux_up, flux_dn=flux_dn, flux_dir=flux_dir))

    def _byband_out(self, out, names, nbnd, nlay, ncol, net, broadband):
        """The outputs of a by-band solver entry: out as given, or bnd_flux_<name> (nbnd, nlev, ncol) for the names [and net], and
        with broadband flux_<name> (nlev, ncol)."""
        if out is None:
            out = {"bnd_flux_" + k: self.empty((nbnd, nlay+1, ncol)) for k in names + (("net",) if net else ())}
            if broadband:
                out.update({"flux_" + k: self.empty((nlay+1, ncol)) for k in names})
        return out

    def _sw_2stream_byband(self, entry, top_at_1, tau, ssa, g, mu0, sfc_alb_dir, sfc_alb_dif, inc_flux_dir, band_lims, inc_flux_dif,
                           out, net, broadband):
        ngpt, nlay, ncol = tau.shape
        nbnd = band_lims.shape[0]
        out = self._byband_out(out, ("up", "dn", "dir"), nbnd, nlay, ncol, net, broadband)
        self._c(entry, ncol, nlay, ngpt, nbnd, top_at_1, tau, ssa, g, mu0,
                sfc_alb_dir, sfc_alb_dif, inc_flux_dir, inc_flux_dif is not None, inc_flux_dif, band_lims,
                out["bnd_flux_up"], out["bnd_flux_dn"], out["bnd_flux_dir"], out.get("bnd_flux_net"),
                out.get("flux_up"), out.get("flux_dn"), out.get("flux_dir"))
        return out

    def sw_solver_2stream_byband(self, top_at_1, tau, ssa, g, mu0, sfc_alb_dir, sfc_alb_dif, inc_flux_dir, band_lims,
                                 inc_flux_dif=None, out=None, net=True, broadband=True):
        """By-band fluxes from the fused broadband solver: bnd_flux_up/dn/dir (nbnd, nlev, ncol), bnd_flux_net = dn - up, and the
        broadband flux_up/dn/dir (the band sums added in band order). band_lims: (nbnd, 2) int32, 1-based inclusive g-point limits.
        out=: a dict of preallocated tensors under those keys (missing optional keys are not written)."""
        if mu0.dim() == 2:
            mu0 = mu0[0].contiguous()
        return self._sw_2stream_byband("sw_solver_2stream_byband", top_at_1, tau, ssa, g, mu0, sfc_alb_dir, sfc_alb_dif, inc_flux_dir,
                                       band_lims, inc_flux_dif, out, net, broadband)

    # mu0 by layer: mu0_lay is (nlay, ncol), every layer of a column with its own cosine
    def _mu0_lay(self, mu0_lay, tau):
        if tuple(mu0_lay.shape) != tuple(tau.shape[1:]):
            raise ValueError(f"mu0_lay must be (nlay, ncol) = ({tau.shape[1]}, {tau.shape[2]}), got {tuple(mu0_lay.shape)}")
        return mu0_lay

    def sw_solver_2stream_mu0lay(self, top_at_1, tau, ssa, g, mu0_lay, sfc_alb_dir, sfc_alb_dif, inc_flux_dir,
                                 inc_flux_dif=None, do_broadband=False, out=None):
        """sw_solver_2stream with the cosine of the solar zenith angle per layer; g and out= as there."""
        return self._sw_2stream("sw_solver_2stream_mu0lay", top_at_1, tau, ssa, g, self._mu0_lay(mu0_lay, tau), sfc_alb_dir, sfc_alb_dif,
                                inc_flux_dir, inc_flux_dif, do_broadband, out)

    def sw_solver_2stream_byband_mu0lay(self, top_at_1, tau, ssa, g, mu0_lay, sfc_alb_dir, sfc_alb_dif, inc_flux_dir, band_lims,
                                        inc_flux_dif=None, out=None, net=True, broadband=True):
        """sw_solver_2stream_byband with the cosine of the solar zenith angle per layer; outputs as there."""
        return self._sw_2stream_byband("sw_solver_2stream_byband_mu0lay", top_at_1, tau, ssa, g, self._mu0_lay(mu0_lay, tau), sfc_alb_dir,
                                       sfc_alb_dif, inc_flux_dir, band_lims, inc_flux_dif, out, net, broadband)

    def zenith_angle_spherical_correction(self, ref_mu, alt, ref_alt=None, planet_radius=6.37123e6, out=None):
        """mu0_lay (nlay, ncol) from the cosine ref_mu (ncol) that holds at altitude ref_alt (ncol, None = 0) and the layer
        altitudes alt (nlay, ncol), metres: the sun rises with altitude over a spherical planet; ref_mu <= 0 is passed through."""
        nlay, ncol = alt.shape
        if tuple(ref_mu.shape) != (ncol,) or (ref_alt is not None and tuple(ref_alt.shape) != (ncol,)):
            raise ValueError("ref_mu and ref_alt must be (ncol)")
        if out is None:
            out = self.empty((nlay, ncol))
        self._c("zenith_angle_spherical_correction", ncol, nlay, ref_alt, ref_mu, alt, planet_radius, out)
        return out

    # ---- gas optics -------------------------------------------------------------------------------
    def interpolation(self, kd, play, tlay, col_gas):
        nlay, ncol = play.shape
        r = dict(
            jtemp=self.int_empty((nlay, ncol)), jpress=self.int_empty((nlay, ncol)),
            tropo=self.bool_empty((nlay, ncol)),
            jeta=self.int_empty((kd.nflav, nlay, ncol, 2)),
            col_mix=self.empty((kd.nflav, nlay, ncol, 2)),
            fminor=self.empty((kd.nflav, nlay, ncol, 2, 2)),
            fmajor=self.empty((kd.nflav, nlay, ncol, 2, 2, 2)))
        self._c("interpolation", ncol, nlay, kd.ngas, kd.nflav, kd.neta, kd.npres, kd.ntemp, *self._direct_args(kd), play, tlay, col_gas,
                r["jtemp"], r["fmajor"], r["fminor"], r["col_mix"], r["tropo"], r["jeta"], r["jpress"])
        return r

    def _absorption_args(self, kd, it, play, tlay, col_gas):
        return self._minor_args(kd, play) + (it["tropo"], it["col_mix"], it["fmajor"], it["fminor"], play, tlay, col_gas)

    def compute_tau_absorption(self, kd, it, play, tlay, col_gas, tau):
        self._c("compute_tau_absorption", *self._absorption_args(kd, it, play, tlay, col_gas),
                it["jeta"], it["jtemp"], it["jpress"], tau)
        return tau

    def compute_tau_absorption_set(self, kd, it, play, tlay, col_gas, tau):
        """tau = major + minor (no zero fill, no read-back); same arithmetic as compute_tau_absorption on a zeroed tau"""
        self._c("compute_tau_absorption_set", *self._absorption_args(kd, it, play, tlay, col_gas),
                it["jeta"], it["jtemp"], it["jpress"], tau)
        return tau

    def gas_optics_sw_fused(self, kd, it, play, tlay, col_gas, col_dry, tau, ssa, g):
        self._c("gas_optics_sw_fused", *self._absorption_args(kd, it, play, tlay, col_gas), col_dry,
                it["jeta"], it["jtemp"], it["jpress"], kd.krayl, tau, ssa, g)

    # "direct" forms: interpolation state computed inside the consumer (no intermediate arrays)
    def _direct_args(self, kd):
        return (kd.flavor, kd.press_ref_log, kd.temp_ref, kd.press_ref_log_delta, kd.temp_ref_min, kd.temp_ref_delta, kd.press_ref_trop_log,
                kd.vmr_ref)

    def _minor_args(self, kd, play):
        nlay, ncol = play.shape
        return (ncol, nlay, kd.nbnd, kd.ngpt, kd.ngas, kd.nflav, kd.neta, kd.npres, kd.ntemp,
                kd.minor_limits_gpt_lower.shape[0], kd.kminor_lower.shape[0],
                kd.minor_limits_gpt_upper.shape[0], kd.kminor_upper.shape[0], kd.idx_h2o,
                kd.gpoint_flavor, kd.band_lims_gpt, kd.kmajor, kd.kminor_lower, kd.kminor_upper,
                kd.minor_limits_gpt_lower, kd.minor_limits_gpt_upper,
                kd.minor_scales_with_density_lower, kd.minor_scales_with_density_upper,
                kd.scale_by_complement_lower, kd.scale_by_complement_upper,
                kd.idx_minor_lower, kd.idx_minor_upper, kd.idx_minor_scaling_lower, kd.idx_minor_scaling_upper,
                kd.kminor_start_lower, kd.kminor_start_upper)

    def gas_optics_lw_direct(self, kd, play, tlay, col_gas, tau, by_band=None):
        """by_band: optical depth per band (nbnd, nlay, ncol) -- clouds -- added where tau is stored (the _allsky entry)"""
        if by_band is None:
            self._c("gas_optics_lw_direct", *self._minor_args(kd, play), *self._direct_args(kd), play, tlay, col_gas, tau)
        else:
            self._c("gas_optics_lw_direct_allsky", *self._minor_args(kd, play), *self._direct_args(kd), play, tlay, col_gas, tau, by_band)
        return tau

    def gas_optics_sw_direct(self, kd, play, tlay, col_gas, col_dry, tau, ssa, g, by_band=None):
        """by_band: (tau, ssa, g) per band (nbnd, nlay, ncol) -- clouds, aerosols -- combined with the gas optics where it is stored"""
        if by_band is None:
            self._c("gas_optics_sw_direct", *self._minor_args(kd, play), *self._direct_args(kd), play, tlay, col_gas, col_dry,
                    kd.krayl, tau, ssa, g)
        else:
            self._c("gas_optics_sw_direct_allsky", *self._minor_args(kd, play), *self._direct_args(kd), play, tlay, col_gas, col_dry,
                    kd.krayl, tau, ssa, g, *by_band)

    def _planck_sources(self, kd, nlay, ncol):
        return dict(sfc_src=self.empty((kd.ngpt, ncol)), lay_src=self.empty((kd.ngpt, nlay, ncol)),
                    lev_src=self.empty((kd.ngpt, nlay+1, ncol)), sfc_src_jac=self.empty((kd.ngpt, ncol)))

    def _planck_lite(self, kd, nlay, ncol):
        return dict(pfrac=self.empty((kd.ngpt, nlay, ncol)), blay=self.empty((kd.nbnd, nlay, ncol)),
                    blev=self.empty((kd.nbnd, nlay+1, ncol)), sfc_src=self.empty((kd.ngpt, ncol)), sfc_src_jac=self.empty((kd.ngpt, ncol)))

    def planck_source_direct(self, kd, play, tlay, tlev, tsfc, sfc_lay, col_gas, out=None):
        nlay, ncol = tlay.shape
        out = self._planck_sources(kd, nlay, ncol) if out is None else out
        self._c("planck_source_direct", ncol, nlay, kd.nbnd, kd.ngpt, kd.ngas, kd.nflav, kd.neta, kd.npres, kd.ntemp, kd.nPlanckTemp,
                play, tlay, tlev, tsfc, sfc_lay, col_gas, *self._direct_args(kd),
                kd.gpoint_bands, kd.band_lims_gpt, kd.planck_frac, kd.totplnk_delta, kd.totplnk, kd.gpoint_flavor,
                out["sfc_src"], out["lay_src"], out["lev_src"], out["sfc_src_jac"])
        return out

    # "Planck-lite" LW chain: fractions + band Planck functions, sources formed inside the broadband solver
    def planck_fractions(self, kd, play, tlay, tlev, tsfc, sfc_lay, col_gas, out=None):
        nlay, ncol = tlay.shape
        out = self._planck_lite(kd, nlay, ncol) if out is None else out
        self._c("planck_fractions", ncol, nlay, kd.nbnd, kd.ngpt, kd.ngas, kd.nflav, kd.neta, kd.npres, kd.ntemp, kd.nPlanckTemp,
                play, tlay, tlev, tsfc, sfc_lay, col_gas, *self._direct_args(kd),
                kd.gpoint_bands, kd.band_lims_gpt, kd.planck_frac, kd.totplnk_delta, kd.totplnk, kd.gpoint_flavor,
                out["pfrac"], out["blay"], out["blev"], out["sfc_src"], out["sfc_src_jac"])
        return out

    def gas_optics_lw_fractions(self, kd, play, tlay, tlev, tsfc, sfc_lay, col_gas, tau, out=None, by_band=None):
        """tau and the Planck-lite outputs in one pass (rrx_gas_optics_lw_fractions); by_band as in gas_optics_lw_direct"""
        nlay, ncol = tlay.shape
        out = self._planck_lite(kd, nlay, ncol) if out is None else out
        a = self._minor_args(kd, play)
        extra = () if by_band is None else (by_band,)
        self._c("gas_optics_lw_fractions" + ("" if by_band is None else "_allsky"), *a[:9], kd.nPlanckTemp, *a[9:16], kd.gpoint_bands, *a[16:],
                *self._direct_args(kd), play, tlay, tlev, tsfc, sfc_lay, col_gas, kd.planck_frac, kd.totplnk_delta, kd.totplnk,
                tau, out["pfrac"], out["blay"], out["blev"], out["sfc_src"], out["sfc_src_jac"], *extra)
        return out

    def planck_sources_from_fractions(self, kd, fr, lay_src=None, lev_src=None):
        ngpt, nlay, ncol = fr["pfrac"].shape
        lay_src = self.empty((ngpt, nlay, ncol)) if lay_src is None else lay_src
        lev_src = self.empty((ngpt, nlay+1, ncol)) if lev_src is None else lev_src
        self._c("planck_sources_from_fractions", ncol, nlay, ngpt, kd.gpoint_bands, fr["pfrac"], fr["blay"], fr["blev"], lay_src, lev_src)
        return lay_src, lev_src

    def lw_solver_noscat_fractions(self, top_at_1, kd, secants, weights, tau, fr, sfc_emis, inc_flux=None, flux_up=None, flux_dn=None):
        ngpt, nlay, ncol = tau.shape
        flux_up = self.empty((nlay+1, ncol)) if flux_up is None else flux_up
        flux_dn = self.empty((nlay+1, ncol)) if flux_dn is None else flux_dn
        self._c("lw_solver_noscat_fractions", ncol, nlay, ngpt, top_at_1, secants, weights, tau,
                fr["pfrac"], fr["blay"], fr["blev"], kd.gpoint_bands, sfc_emis, fr["sfc_src"], inc_flux, flux_up, flux_dn)
        return dict(flux_up=flux_up, flux_dn=flux_dn)

    def lw_solver_noscat_fractions_jac(self, top_at_1, kd, secants, weights, tau, fr, sfc_emis, inc_flux=None, flux_up=None, flux_dn=None,
                                       flux_up_jac=None):
        """lw_solver_noscat_fractions plus flux_up_jac (nlev, ncol), the surface-temperature Jacobian of the upward flux
        [W m-2 K-1] from the same solve (fr["sfc_src_jac"] as gas_optics_lw_fractions writes it); the fluxes are bit for bit those of
        lw_solver_noscat_fractions"""
        ngpt, nlay, ncol = tau.shape
        flux_up = self.empty((nlay+1, ncol)) if flux_up is None else flux_up
        flux_dn = self.empty((nlay+1, ncol)) if flux_dn is None else flux_dn
        flux_up_jac = self.empty((nlay+1, ncol)) if flux_up_jac is None else flux_up_jac
        self._c("lw_solver_noscat_fractions_jac", ncol, nlay, ngpt, top_at_1, secants, weights, tau,
                fr["pfrac"], fr["blay"], fr["blev"], kd.gpoint_bands, sfc_emis, fr["sfc_src"], inc_flux, flux_up, flux_dn,
                fr["sfc_src_jac"], flux_up_jac)
        return dict(flux_up=flux_up, flux_dn=flux_dn, flux_up_jac=flux_up_jac)

    def lw_solver_noscat_fractions_angles(self, top_at_1, kd, secants, weights, tau, fr, sfc_emis, inc_flux=None, flux_up=None,
                                          flux_dn=None, flux_up_jac=None, jacobian=False):
        """lw_solver_noscat_fractions [_jac with jacobian=True] for the nmus = 1..4 quadrature angles of secants (nmus, ngpt, ncol)
        and weights (nmus), in one kernel: each g-point is read once and solved nmus times. One angle gives the bits of the
        one-angle entries."""
        ngpt, nlay, ncol = tau.shape
        nmus = int(weights.shape[0])
        if tuple(secants.shape) != (nmus, ngpt, ncol):
            raise ValueError(f"secants {tuple(secants.shape)} is not (nmus, ngpt, ncol) = {(nmus, ngpt, ncol)}")
        flux_up = self.empty((nlay+1, ncol)) if flux_up is None else flux_up
        flux_dn = self.empty((nlay+1, ncol)) if flux_dn is None else flux_dn
        out = dict(flux_up=flux_up, flux_dn=flux_dn)
        if jacobian:
            out["flux_up_jac"] = self.empty((nlay+1, ncol)) if flux_up_jac is None else flux_up_jac
        self._c("lw_solver_noscat_fractions_angles", ncol, nlay, ngpt, top_at_1, nmus, secants, weights, tau,
                fr["pfrac"], fr["blay"], fr["blev"], kd.gpoint_bands, sfc_emis, fr["sfc_src"], inc_flux, flux_up, flux_dn,
                fr["sfc_src_jac"] if jacobian else None, out.get("flux_up_jac"))
        return out

    @staticmethod
    def optimal_fit_abi(kd):
        """kd.optimal_angle_fit (2, nbnd) in the C ABI's layout: (2, nbnd) with the first index fastest, i.e. a (nbnd, 2) tensor"""
        if getattr(kd, "optimal_angle_fit", None) is None:
            raise ValueError("the k-distribution carries no optimal_angle_fit")
        return kd.optimal_angle_fit.t().contiguous()

    def lw_optimal_secants(self, kd, tau, fit=None, secants=None):
        """Optimal-angle secants (ngpt, ncol) of tau (ngpt, nlay, ncol): D = fit[0, b]*exp(-sum of tau over the layers) + fit[1, b]
        for the band b of the g-point. fit: optimal_fit_abi(kd) (default) or a (nbnd, 2) tensor of one's own."""
        ngpt, nlay, ncol = tau.shape
        fit = self.optimal_fit_abi(kd) if fit is None else fit
        secants = self.empty((ngpt, ncol)) if secants is None else secants
        self._c("lw_optimal_secants", ncol, nlay, ngpt, fit.shape[0], kd.gpoint_bands, fit, tau, secants)
        return secants

    def lw_solver_noscat_fractions_optimal(self, top_at_1, kd, weights, tau, fr, sfc_emis, fit=None, inc_flux=None, flux_up=None,
                                           flux_dn=None, flux_up_jac=None, jacobian=False, secants_out=None, keep_secants=False):
        """lw_solver_noscat_fractions [_jac with jacobian=True] for one angle whose secant is the optimal-angle fit, formed inside the
        fused kernel from the g-point it holds. weights: (1,). keep_secants / secants_out: the (ngpt, ncol) secants the solve used come
        back under "secants"."""
        ngpt, nlay, ncol = tau.shape
        if int(weights.shape[0]) != 1:
            raise ValueError("optimal angles are one quadrature angle: weights must hold one value")
        fit = self.optimal_fit_abi(kd) if fit is None else fit
        flux_up = self.empty((nlay+1, ncol)) if flux_up is None else flux_up
        flux_dn = self.empty((nlay+1, ncol)) if flux_dn is None else flux_dn
        out = dict(flux_up=flux_up, flux_dn=flux_dn)
        if jacobian:
            out["flux_up_jac"] = self.empty((nlay+1, ncol)) if flux_up_jac is None else flux_up_jac
        if secants_out is None and keep_secants:
            secants_out = self.empty((ngpt, ncol))
        if secants_out is not None:
            out["secants"] = secants_out
        self._c("lw_solver_noscat_fractions_optimal", ncol, nlay, ngpt, fit.shape[0], top_at_1, weights, tau,
                fr["pfrac"], fr["blay"], fr["blev"], kd.gpoint_bands, fit, sfc_emis, fr["sfc_src"], inc_flux, flux_up, flux_dn,
                fr["sfc_src_jac"] if jacobian else None, out.get("flux_up_jac"), secants_out)
        return out

    def lw_flux_up_adjust(self, flux_up_jac, t_sfc_old, t_sfc_new, flux_up, flux_net=None):
        """Host-model update in place: flux_up += jac*(t_new - t_old), flux_net -= the same (when given); (nlev, ncol) arrays"""
        nlev, ncol = flux_up_jac.shape
        self._c("lw_flux_up_adjust", ncol, nlev, flux_up_jac, t_sfc_old, t_sfc_new, flux_up, flux_net)
        return flux_up

    MATH_PRIMITIVES = ("exp_neg", "exp_neg_table", "fast_rcp", "sqrt_pos", "sqrt_nonneg")

    def math_selftest(self, primitive, x, out=None):
        """Test entry (rrx_math_selftest): one of the solvers' device math primitives (MATH_PRIMITIVES, csrc/rrx_common.h) applied
        element-wise to the 1-D tensor x"""
        if primitive not in self.MATH_PRIMITIVES:
            raise ValueError(f"{primitive!r} is not one of {self.MATH_PRIMITIVES}")
        if x.dim() != 1 or not x.is_contiguous():
            raise ValueError("math_selftest: x must be a contiguous 1-D tensor")
        out = torch.empty_like(x) if out is None else out
        self._c("math_selftest", self.MATH_PRIMITIVES.index(primitive), x.shape[0], x, out)
        return out

    def lw_solver_noscat_fractions_byband(self, top_at_1, kd, secants, weights, tau, fr, sfc_emis, inc_flux=None, out=None,
                                          net=True, broadband=True, band_lims=None, gpoint_bands=None):
        """By-band fluxes of lw_solver_noscat_fractions: bnd_flux_up/dn (nbnd, nlev, ncol), bnd_flux_net = dn - up, and the broadband
        flux_up/dn (the band sums added in band order). band_lims / gpoint_bands default to the k-distribution's. out=: a dict of
        preallocated tensors under those keys (missing optional keys are not written)."""
        ngpt, nlay, ncol = tau.shape
        band_lims = kd.band_lims_gpt if band_lims is None else band_lims
        gpoint_bands = kd.gpoint_bands if gpoint_bands is None else gpoint_bands
        nbnd = band_lims.shape[0]
        out = self._byband_out(out, ("up", "dn"), nbnd, nlay, ncol, net, broadband)
        self._c("lw_solver_noscat_fractions_byband", ncol, nlay, ngpt, nbnd, top_at_1, secants, weights, tau,
                fr["pfrac"], fr["blay"], fr["blev"], gpoint_bands, band_lims, sfc_emis, fr["sfc_src"], inc_flux,
                out["bnd_flux_up"], out["bnd_flux_dn"], out.get("bnd_flux_net"), out.get("flux_up"), out.get("flux_dn"))
        return out

    def lw_solver_2stream(self, top_at_1, tau, ssa, g, lev_source, sfc_emis, sfc_src, inc_flux=None, do_broadband=False,
                          flux_up=None, flux_dn=None):
        """LW two-stream solver with scattering, general entry (rrx_lw_solver_2stream): tau, ssa, g (ngpt, nlay, ncol), lev_source
        (ngpt, nlay+1, ncol), sfc_emis / sfc_src / inc_flux (ngpt, ncol). Fluxes per g-point (ngpt, nlev, ncol), or their g-point
        sums (nlev, ncol) with do_broadband."""
        ngpt, nlay, ncol = tau.shape
        shape = (nlay+1, ncol) if do_broadband else (ngpt, nlay+1, ncol)
        flux_up = self.empty(shape) if flux_up is None else flux_up
        flux_dn = self.empty(shape) if flux_dn is None else flux_dn
        gpt = (None, None) if do_broadband else (flux_up, flux_dn)
        loc = (flux_up, flux_dn) if do_broadband else (None, None)
        self._c("lw_solver_2stream", ncol, nlay, ngpt, top_at_1, tau, ssa, g, lev_source, sfc_emis, sfc_src, inc_flux, *gpt, do_broadband,
                *loc)
        return dict(flux_up=flux_up, flux_dn=flux_dn)

    def lw_solver_2stream_fractions(self, top_at_1, kd, tau, fr, sfc_emis, cloud=None, inc_flux=None, flux_up=None, flux_dn=None,
                                    band_lims=None, gpoint_bands=None):
        """The same solve from Planck-lite inputs in one kernel, broadband fluxes (nlev, ncol): tau = clear gas optical depth
        (ngpt, nlay, ncol), fr = the Planck-lite outputs (pfrac, blev, sfc_src), cloud = None (pure absorption) or (tau, ssa, g) by
        band, (nbnd, nlay, ncol) each, combined with the gas inside the kernel."""
        ngpt, nlay, ncol = tau.shape
        band_lims = kd.band_lims_gpt if band_lims is None else band_lims
        gpoint_bands = kd.gpoint_bands if gpoint_bands is None else gpoint_bands
        flux_up = self.empty((nlay+1, ncol)) if flux_up is None else flux_up
        flux_dn = self.empty((nlay+1, ncol)) if flux_dn is None else flux_dn
        ct, cw, cg = (None, None, None) if cloud is None else cloud
        self._c("lw_solver_2stream_fractions", ncol, nlay, ngpt, band_lims.shape[0], top_at_1, tau, fr["pfrac"], fr["blev"],
                gpoint_bands, band_lims, ct, cw, cg, sfc_emis, fr["sfc_src"], inc_flux, flux_up, flux_dn)
        return dict(flux_up=flux_up, flux_dn=flux_dn)

    def lw_solver_noscat_rescaled(self, top_at_1, secants, weights, tau, ssa, g, lay_source, lev_source, sfc_emis, sfc_src,
                                  inc_flux=None, do_broadband=False, do_jacobians=False, sfc_src_jac=None, out=None):
        """No-scattering LW solve on rescaled optical depths with one correction sweep, general entry
        (rrx_lw_solver_noscat_rescaled): the arguments of lw_solver_noscat plus ssa, g (ngpt, nlay, ncol)."""
        return self._lw_noscat("lw_solver_noscat_rescaled", top_at_1, secants, weights, tau, (ssa, g), lay_source, lev_source, sfc_emis,
                               sfc_src, inc_flux, do_broadband, do_jacobians, sfc_src_jac, out)

    def lw_solver_noscat_fractions_rescaled(self, top_at_1, kd, secants, weights, tau, fr, sfc_emis, cloud=None, inc_flux=None,
                                            flux_up=None, flux_dn=None, band_lims=None, gpoint_bands=None):
        """The same solve for one angle from Planck-lite inputs in one kernel, broadband fluxes (nlev, ncol): tau = clear gas optical
        depth (ngpt, nlay, ncol), fr = the Planck-lite outputs (pfrac, blay, blev, sfc_src), cloud = None (ssa = 0) or (tau, ssa, g)
        by band, (nbnd, nlay, ncol) each, combined with the gas inside the kernel."""
        ngpt, nlay, ncol = tau.shape
        band_lims = kd.band_lims_gpt if band_lims is None else band_lims
        gpoint_bands = kd.gpoint_bands if gpoint_bands is None else gpoint_bands
        flux_up = self.empty((nlay+1, ncol)) if flux_up is None else flux_up
        flux_dn = self.empty((nlay+1, ncol)) if flux_dn is None else flux_dn
        ct, cw, cg = (None, None, None) if cloud is None else cloud
        self._c("lw_solver_noscat_fractions_rescaled", ncol, nlay, ngpt, band_lims.shape[0], top_at_1, secants, weights,
                tau, fr["pfrac"], fr["blay"], fr["blev"], gpoint_bands, band_lims, ct, cw, cg, sfc_emis, fr["sfc_src"], inc_flux,
                flux_up, flux_dn)
        return dict(flux_up=flux_up, flux_dn=flux_dn)

    def compute_tau_rayleigh(self, kd, it, col_dry, col_gas):
        nlay, ncol = col_dry.shape
        tr = self.empty((kd.ngpt, nlay, ncol))
        self._c("compute_tau_rayleigh", ncol, nlay, kd.nbnd, kd.ngpt, kd.ngas, kd.nflav, kd.neta, kd.npres, kd.ntemp,
                kd.gpoint_flavor, kd.band_lims_gpt, kd.krayl, kd.idx_h2o, col_dry, col_gas,
                it["fminor"], it["jeta"], it["tropo"], it["jtemp"], tr)
        return tr

    def combine_abs_and_rayleigh(self, tau_abs, tau_ray):
        ngpt, nlay, ncol = tau_abs.shape
        tau = self.empty(tau_abs.shape); ssa = self.empty(tau_abs.shape); g = self.empty(tau_abs.shape)
        self._c("combine_abs_and_rayleigh", ncol, nlay, ngpt, tau_abs, tau_ray, tau, ssa, g)
        return tau, ssa, g

    def compute_planck_source(self, kd, it, tlay, tlev, tsfc, sfc_lay, out=None):
        nlay, ncol = tlay.shape
        out = self._planck_sources(kd, nlay, ncol) if out is None else out
        self._c("compute_planck_source", ncol, nlay, kd.nbnd, kd.ngpt, kd.nflav, kd.neta, kd.npres, kd.ntemp, kd.nPlanckTemp,
                tlay, tlev, tsfc, sfc_lay, it["fmajor"], it["jeta"], it["tropo"], it["jtemp"], it["jpress"],
                kd.gpoint_bands, kd.band_lims_gpt, kd.planck_frac, kd.temp_ref_min, kd.totplnk_delta,
                kd.totplnk, kd.gpoint_flavor, out["sfc_src"], out["lay_src"], out["lev_src"], out["sfc_src_jac"])
        return out

    # ---- stand-alone boundary conditions and transposes (launcher parity with the reference's namespaces) ----
    def apply_BC(self, nlay, top_at_1, flux_dn, inc_flux=None, factor=None):
        ngpt, nlev, ncol = flux_dn.shape
        if inc_flux is None:
            self._c("apply_BC_0", ncol, nlay, ngpt, top_at_1, flux_dn)
        elif factor is None:
            self._c("apply_BC_gpt", ncol, nlay, ngpt, top_at_1, inc_flux, flux_dn)
        else:
            self._c("apply_BC_factor", ncol, nlay, ngpt, top_at_1, inc_flux, factor, flux_dn)
        return flux_dn

    def reorder123x321(self, arr_in):
        ni, nj, nk = arr_in.shape
        out = self.empty((nk, nj, ni))
        self._c("reorder123x321", ni, nj, nk, arr_in, out)
        return out

    def reorder12x21(self, arr_in):
        ni, nj = arr_in.shape
        out = self.empty((nj, ni))
        self._c("reorder12x21", ni, nj, arr_in, out)
        return out

    # ---- optical props / fluxes -----------------------------------------------------------------------
    def increment_1scalar_by_1scalar(self, tau_inout, tau_in):
        ngpt, nlay, ncol = tau_inout.shape
        self._c("increment_1scalar_by_1scalar", ncol, nlay, ngpt, tau_inout, tau_in)

    def increment_2stream_by_2stream(self, t1, w1, g1, t2, w2, g2):
        ngpt, nlay, ncol = t1.shape
        self._c("increment_2stream_by_2stream", ncol, nlay, ngpt, t1, w1, g1, t2, w2, g2)

    def inc_1scalar_by_1scalar_bybnd(self, tau_inout, tau_in, band_lims):
        ngpt, nlay, ncol = tau_inout.shape
        self._c("inc_1scalar_by_1scalar_bybnd", ncol, nlay, ngpt, tau_inout, tau_in, band_lims.shape[0], band_lims)

    def inc_2stream_by_2stream_bybnd(self, t1, w1, g1, t2, w2, g2, band_lims):
        ngpt, nlay, ncol = t1.shape
        self._c("inc_2stream_by_2stream_bybnd", ncol, nlay, ngpt, t1, w1, g1, t2, w2, g2, band_lims.shape[0], band_lims)

    # McICA cloud sampling (rrx_mcica_*): cloud_frac (nlay, ncol), alpha None (maximum-random) or (nlay-1, ncol) (exponential-random),
    # col_id None (identity = col_id0 + column) or an int32 tensor (ncol,) of global column indices; mask: None, True (allocated)
    # or a uint8 tensor (ngpt, nlay, ncol). The g-point arrays are updated in place in the cloudy cells only; returns the mask or None.
    def _mcica_args(self, cloud_frac, alpha, seed, domain, col_id, col_id0, ngpt, mask):
        nlay, ncol = cloud_frac.shape
        if alpha is not None and tuple(alpha.shape) != (max(nlay-1, 0), ncol):
            raise ValueError(f"mcica: alpha {tuple(alpha.shape)} is not (nlay-1, ncol) = {(nlay-1, ncol)}")
        if col_id is not None and (col_id.dtype != torch.int32 or col_id.numel() != ncol):
            raise TypeError("mcica: col_id is an int32 tensor of ncol entries")
        if mask is True:
            mask = torch.empty((ngpt, nlay, ncol), dtype=torch.uint8, device=self.device)
        elif mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (ngpt, nlay, ncol)):
            raise TypeError("mcica: mask is a uint8 tensor (ngpt, nlay, ncol)")
        head = (cloud_frac, alpha, int(seed) & 0xFFFFFFFFFFFFFFFF, domain, col_id, col_id0)
        return head, mask

    def mcica_increment_1scalar(self, tau, cld_tau, band_lims, cloud_frac, alpha=None, seed=0, domain=0, col_id=None, col_id0=0, mask=None):
        ngpt, nlay, ncol = tau.shape
        head, mask = self._mcica_args(cloud_frac, alpha, seed, domain, col_id, col_id0, ngpt, mask)
        self._c("mcica_increment_1scalar", ncol, nlay, ngpt, band_lims.shape[0], band_lims, *head, tau, cld_tau, mask)
        return mask

    def mcica_increment_2stream(self, tau, ssa, g, cld_tau, cld_ssa, cld_g, band_lims, cloud_frac, alpha=None, seed=0, domain=0,
                                col_id=None, col_id0=0, mask=None):
        ngpt, nlay, ncol = tau.shape
        head, mask = self._mcica_args(cloud_frac, alpha, seed, domain, col_id, col_id0, ngpt, mask)
        self._c("mcica_increment_2stream", ncol, nlay, ngpt, band_lims.shape[0], band_lims, *head, tau, ssa, g,
                cld_tau, cld_ssa, cld_g, mask)
        return mask

    def mcica_cloud_mask(self, ngpt, cloud_frac, alpha=None, seed=0, domain=0, col_id=None, col_id0=0, mask=True):
        nlay, ncol = cloud_frac.shape
        head, mask = self._mcica_args(cloud_frac, alpha, seed, domain, col_id, col_id0, ngpt, mask)
        self._c("mcica_cloud_mask", ncol, nlay, ngpt, *head, mask)
        return mask

    # The Monte Carlo ray tracers. Every wrapper below gathers its arguments into a raytracer_args.RtScene, makes
    # or accepts the outputs, calls the entry the scene names with the scene's argument groups, and unpacks.
    #   tau, ssa (ngpt, nz, ncol) with ncol = nx ny, x fastest; sfc_albedo (ncol,); kn_grid = (knx, kny, knz);
    #   cloud: None or (tau, ssa, g), (nbnd, nz, ncol) each, with band_lims (nbnd, 2);
    #   phase: None (Henyey-Greenstein from cld_g) or an object with mu (nmu,), phase, cdf (nbnd, nre, nmu), re0, dre and cld_re
    #     (nz, ncol), such as phase_tables.PhaseTable (the rrx_*_phase twins of the four plain entries);
    #   background: None (nbg = 0) or an object with dz (nbg,) numbers on the host, tau, ssa (ngpt, nbg), cloud, None or (tau, ssa, g)
    #     of (nbnd, nbg) each, and aerosol likewise, everything counted upward from the domain top (the rrx_*_bg entries);
    #   aerosol: None or the grid's band triple (tau, ssa, g) of (nbnd, nz, ncol) each, a third scattering species. The wrappers with
    #     aerosol= go through the rrx_*_aer entries when it or background.aerosol is given; a triple of None is given too: NULL
    #     pointers.
    # Counts are int64 tensors holding the unsigned 64-bit tallies (units of 2^-32 photon).
    RT_COUNTS = ("sfc_dn_dir", "sfc_dn_dif", "sfc_up", "tod_up", "abs_dir", "abs_dif")
    RT_BG_COUNTS = ("toa_up", "tod_dn_dir", "tod_dn_dif", "bg_abs_dir", "bg_abs_dif")
    RT_MAX_EVENTS = 1 << 22

    def rt_phase_tables(self, mu, phase_raw):
        """phase, cdf (nbnd, nre, nmu) from the nodes mu (nmu,) and phase_raw (nbnd, nre, nmu) >= 0 of any normalisation."""
        nbnd, nre, nmu = phase_raw.shape
        phase, cdf = self.empty((nbnd, nre, nmu)), self.empty((nbnd, nre, nmu))
        self._c("rt_phase_tables", nmu, nre, nbnd, mu, phase_raw, phase, cdf)
        return phase, cdf

    def _rt_phase_array(self, entry, table, ibnd, values, re):
        nbnd, nre, nmu = table.phase.shape
        out = self.empty(tuple(values.shape))
        self._c(entry, values.numel(), nmu, nre, nbnd, ibnd, table.re0, table.dre, table.mu, table.phase, table.cdf, values, re, out)
        return out

    def rt_phase_sample(self, table, ibnd, u, re):
        """The cosines that the tracers draw from the uniforms u in cells of radius re (the same shape), band ibnd (0-based)."""
        return self._rt_phase_array("rt_phase_sample", table, ibnd, u, re)

    def rt_phase_eval(self, table, ibnd, cs, re):
        """P(cs) at radius re: the density of rt_phase_sample."""
        return self._rt_phase_array("rt_phase_eval", table, ibnd, cs, re)

    def _rt_zeros(self, **shapes):
        return {k: torch.zeros(shape, dtype=torch.int64, device=self.device) for k, shape in shapes.items()}

    def rt_zero_counts(self, nz, ncol):
        return self._rt_zeros(**{k: (ncol,) for k in self.RT_COUNTS[:4]}, **{k: (nz, ncol) for k in self.RT_COUNTS[4:]}, n_capped=(1,))

    def rt_zero_counts_bg(self, nz, ncol, nbg):
        return {**self.rt_zero_counts(nz, ncol), **self._rt_zeros(**{k: (ncol,) for k in self.RT_BG_COUNTS[:3]},
                                                                  **{k: (max(nbg, 1),) for k in self.RT_BG_COUNTS[3:]})}

    def rt_bw_zero_counts(self, npix):
        return self._rt_zeros(counts=(npix,), n_capped=(1,), n_clamped=(1,))

    def camera_zero_counts(self, nbnd, npix):
        return self._rt_zeros(counts=(nbnd, npix), n_capped=(1,), n_clamped=(1,))

    def rt_counts_to_flux(self, counts, scale, out):
        """out += counts 2^-32 scale"""
        self._c("rt_counts_to_flux", counts.numel(), counts, scale, out)
        return out

    # What the wrappers share beside the scene.
    def _rt_per_gpt(self, ngpt, **arrays):
        """the (ngpt,) host arrays of a loop: the precision's numbers, photons_per_pixel_gpt and rays_per_pixel_gpt int64"""
        out = [np.ascontiguousarray(a, dtype=np.int64 if k.endswith("_per_pixel_gpt") else self.np_dtype).reshape(-1) for k, a in arrays.items()]
        if any(a.size != ngpt for a in out):
            raise ValueError(f"raytracer: {', '.join(arrays)} {'is' if len(out) == 1 else 'are'} (ngpt,)")
        return out

    def _rt_list(self, ngpt, unit, first, n, **arrays):
        """The concatenated list of a spectral single-launch entry on the device: its ends (ngpt+1,) int64, the first of arrays, and
        the (ngpt,) numbers per g-point, the others; the range [first, first + n) must lie within it."""
        (name, end), *weights = arrays.items()
        end = np.ascontiguousarray(np.asarray(end, dtype=np.int64).reshape(-1))
        host = [np.ascontiguousarray(np.asarray(a, dtype=self.np_dtype).reshape(-1)) for _, a in weights]
        if end.size != ngpt + 1 or any(a.size != ngpt for a in host):
            raise ValueError(f"raytracer: {name} is (ngpt+1,) and {', '.join(k for k, _ in weights)} {'is' if len(host) == 1 else 'are'} (ngpt,)")
        if end[0] != 0 or np.any(np.diff(end) < 0):
            raise ValueError(f"raytracer: {name} must start at 0 and must not descend")
        if first + n > int(end[-1]):
            raise ValueError(f"raytracer: the range [{first}, {first + n}) ends beyond the list of {int(end[-1])} {unit}")
        return [torch.as_tensor(a, device=self.device) for a in (end, *host)]

    def _rt_chan_weights(self, chan_weights, nbnd):
        """chan_weights (nchan, nbnd): a tensor as it is, anything else as a host array of the precision"""
        M = chan_weights if torch.is_tensor(chan_weights) else np.ascontiguousarray(np.asarray(chan_weights, dtype=self.np_dtype))
        if M.ndim != 2 or M.shape[1] != nbnd:
            raise ValueError(f"raytracer: chan_weights is (nchan, nbnd = {nbnd}), got {tuple(M.shape)}")
        return M

    def _rt_sensor(self, camera):
        """a sensor (camera.Camera, or any object with type, npx, npy, fov, position, e_w, e_h, e_d) as the backward entries take it"""
        numbers = np.concatenate([np.asarray(v, dtype=np.float64).reshape(3) for v in (camera.position, camera.e_w, camera.e_h, camera.e_d)])
        return (int(camera.type), int(camera.npx), int(camera.npy), camera.fov, np.ascontiguousarray(numbers.astype(self.np_dtype)))

    def _rt_radiance(self, shape):
        """(radiance, n_capped, n_clamped): the outputs of a backward loop"""
        return (self.empty(shape), *self._rt_zeros(n_capped=(1,), n_clamped=(1,)).values())

    # ---- k_null and the background's profile
    def _rt_k_null(self, entry, tau, igpt, nx, ny, dz, kn_grid, top_at_1, cloud, band_lims, aerosol, tail):
        sc = RtScene(self, band_lims).set_grid(tau, nx, ny, dz, kn_grid, top_at_1, cloud).set_aerosol(aerosol)
        knx, kny, knz = sc.kn
        out = self.empty((knz, kny, knx) if igpt is not None else (sc.ngpt, knz, kny, knx))
        self._c(entry, *sc.dims, *(() if igpt is None else (igpt,)), top_at_1, tau, sc.lims("k_null"), sc.cloud[0], dz, *sc.kn, out, *((sc.aer[0],) if tail else ()))
        return out

    def rt_k_null(self, tau, igpt, nx, ny, dz, kn_grid, top_at_1, cloud=None, band_lims=None, aerosol=None):
        """k_null (knz, kny, knx), kn counted upward from the surface, for g-point igpt (0-based). aerosol=: None, or the grid's
        aerosol triple (rrx_rt_k_null_aer; a triple of None: its NULL pointer)."""
        return self._rt_k_null("rt_k_null" if aerosol is None else "rt_k_null_aer", tau, igpt, nx, ny, dz, kn_grid, top_at_1, cloud, band_lims,
                               aerosol, aerosol is not None)

    def rt_k_null_all(self, tau, nx, ny, dz, kn_grid, top_at_1, cloud=None, band_lims=None, aerosol=None):
        """k_null (ngpt, knz, kny, knx): slice g is rt_k_null(..., igpt=g, aerosol=...) (ngpt <= 1024)"""
        return self._rt_k_null("rt_k_null_all", tau, None, nx, ny, dz, kn_grid, top_at_1, cloud, band_lims, aerosol, True)

    def rt_bg_profile(self, background, igpt, band_lims=None, aerosol=None):
        """The profile (5, nbg+1) of g-point igpt: k_ext, k_sca, k_sca_cld, g, tau_above. aerosol=: the background's aerosol triple
        (a triple of None: no aerosol aloft) gives the profile (7, nbg+1) of rrx_rt_bg_profile_aer, which the _aer trace entries
        take: k_sca_aer and g_aer behind the five rows."""
        sc = RtScene(self, band_lims).set_background(background, aerosol=aerosol)
        sc.need_lims("a background cloud triple", "bg_cloud")
        sc.need_lims("a background aerosol triple", "bg_aer")
        out = self.empty((5 if aerosol is None else 7, sc.nbg + 1))
        self._c("rt_bg_profile" if aerosol is None else "rt_bg_profile_aer", sc.nbg, background.tau.shape[0], sc.nbnd, igpt, sc.dz_bg,
                sc.bg_tau, sc.bg_ssa, sc.lims("profile"), *sc.bg_cloud, out, *(() if aerosol is None else sc.bg_aer))
        return out

    def rt_bg_profile_all(self, background, band_lims=None):
        """The profile (ngpt, 7, nbg+1): slice g is rt_bg_profile(background, g, band_lims, aerosol=the background's triple)"""
        sc = RtScene(self, band_lims).set_background(background)
        sc.need_lims("a background cloud or aerosol triple", "bg_cloud", "bg_aer")
        ngpt = background.tau.shape[0]
        out = self.empty((ngpt, 7, sc.nbg + 1))
        self._c("rt_bg_profile_all", sc.nbg, ngpt, sc.nbnd, sc.dz_bg, sc.bg_tau, sc.bg_ssa, sc.lims("profile"), *sc.bg_cloud, out, *sc.bg_aer)
        return out

    # ---- the forward tracer (rrx_rt_trace_counts, rrx_raytracer_sw and their forms)
    def _rt_fw_counts(self, sc, grid, counts):
        """(the counts of a forward single launch, made when None; the entry's tally arguments)"""
        if counts is None:
            counts = self.rt_zero_counts(sc.nz, sc.ncol) if grid else self.rt_zero_counts_bg(sc.nz, sc.ncol, sc.nbg)
        return counts, tuple(counts[k] for k in (*self.RT_COUNTS, "n_capped", *(() if grid else self.RT_BG_COUNTS)))

    def _rt_trace_counts(self, grid, tau, ssa, igpt, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, kn_grid, k_null, seed,
                         photon0, nphotons, top_at_1, independent_column, cloud, band_lims, counts, max_events, phase, background=None,
                         bg_profile=None, aerosol=None):
        sc = RtScene(self, band_lims).set_grid(tau, nx, ny, dz, kn_grid, top_at_1, cloud, ssa, dx, dy, sfc_albedo, mu0, azimuth, independent_column)
        sc.set_medium("trace", "rt_trace_counts", phase, background, aerosol, grid=grid, igpt=igpt, bg_profile=bg_profile)
        counts, tallies = self._rt_fw_counts(sc, grid, counts)
        self._c(sc.entry, *sc.dims, igpt, *sc.flags, *sc.grid("trace"), inc_dir, inc_dif, *sc.kn, k_null,
                *sc.run(seed, max_events, photon0, nphotons), *tallies, *sc.table, *sc.bg_tail, *sc.aer_tail("trace"))
        return counts

    def rt_trace_counts(self, tau, ssa, igpt, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, kn_grid, k_null, seed,
                        photon0, nphotons, top_at_1=False, independent_column=False, cloud=None, band_lims=None, counts=None,
                        max_events=None, phase=None):
        """Adds the photons [photon0, photon0 + nphotons) of g-point igpt into counts (rt_zero_counts; made when None)."""
        return self._rt_trace_counts(True, tau, ssa, igpt, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, kn_grid, k_null, seed,
                                     photon0, nphotons, top_at_1, independent_column, cloud, band_lims, counts, max_events, phase)

    def rt_trace_counts_bg(self, tau, ssa, igpt, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, kn_grid, k_null, seed,
                           photon0, nphotons, top_at_1=False, independent_column=False, cloud=None, band_lims=None, counts=None,
                           max_events=None, phase=None, background=None, bg_profile=None, aerosol=None):
        """rt_trace_counts with a background: bg_profile is rt_bg_profile's for igpt (made when None). The counts gain RT_BG_COUNTS.
        With aerosol= or background.aerosol it is rrx_rt_trace_counts_aer: k_null is then rt_k_null's with
        aerosol= and bg_profile the 7-row profile."""
        return self._rt_trace_counts(False, tau, ssa, igpt, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, kn_grid, k_null, seed,
                                     photon0, nphotons, top_at_1, independent_column, cloud, band_lims, counts, max_events, phase, background,
                                     bg_profile, aerosol)

    def rt_trace_counts_spectral(self, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, photon_end, weight0, dif_frac, kn_grid, k_null,
                                 seed, photon0, nphotons, top_at_1=False, independent_column=False, cloud=None, band_lims=None, counts=None,
                                 max_events=None, phase=None, background=None, bg_profile=None, aerosol=None):
        """Adds the photons [photon0, photon0 + nphotons) of the concatenated list into counts (rt_zero_counts_bg; made when None).
        photon_end (ngpt+1,) int64, weight0, dif_frac (ngpt,): arrays on the host, checked and uploaded here; k_null is
        rt_k_null_all's and bg_profile rt_bg_profile_all's (made when None)."""
        sc = RtScene(self, band_lims).set_grid(tau, nx, ny, dz, kn_grid, top_at_1, cloud, ssa, dx, dy, sfc_albedo, mu0, azimuth, independent_column)
        lists = self._rt_list(sc.ngpt, "photons", photon0, nphotons, photon_end=photon_end, weight0=weight0, dif_frac=dif_frac)
        sc.set_medium("trace", "rt_trace_counts", phase, background, aerosol, spectral=True, bg_profile=bg_profile)
        counts, tallies = self._rt_fw_counts(sc, False, counts)
        self._c(sc.entry, *sc.dims, *sc.flags, *sc.grid("trace"), *lists, *sc.kn, k_null, *sc.run(seed, max_events, photon0, nphotons),
                *tallies, *sc.table, *sc.bg_tail, *sc.aer_tail("trace"))
        return counts

    def _rt_sw_loop(self, grid, spectral, photons, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, kn_grid, seed,
                    top_at_1, independent_column, cloud, band_lims, max_events, phase, background=None, aerosol=None):
        """raytracer_sw, raytracer_sw_bg (photons: photons_per_pixel) and raytracer_sw_spectral (photons: photons_per_pixel_gpt)"""
        sc = RtScene(self, band_lims).set_grid(tau, nx, ny, dz, kn_grid, top_at_1, cloud, ssa, dx, dy, sfc_albedo, mu0, azimuth, independent_column)
        per_gpt = self._rt_per_gpt(sc.ngpt, inc_dir=inc_dir, inc_dif=inc_dif, **({"photons_per_pixel_gpt": photons} if spectral else {}))
        sc.set_medium("loop", "raytracer_sw", phase, background, aerosol, grid=grid, spectral=spectral)
        # the grid's six are written by the entry; the background's five are added to (and stay zeros without a background)
        out = {k: self.empty((sc.ncol,)) for k in self.RT_COUNTS[:4]}
        out.update({k: self.empty((sc.nz, sc.ncol)) for k in self.RT_COUNTS[4:]})
        if not grid:
            out.update({k: self.zeros((sc.ncol,)) for k in self.RT_BG_COUNTS[:3]})
            out.update({k: self.zeros((sc.nbg,)) for k in self.RT_BG_COUNTS[3:]})
        n_capped = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self._c(sc.entry, *sc.dims, *sc.flags, *sc.grid("loop"), *per_gpt[:2], *sc.kn, per_gpt[2] if spectral else photons,
                *sc.run(seed, max_events), *(out[k] for k in self.RT_COUNTS), n_capped,
                *(() if grid else (out[k] if sc.nbg else None for k in self.RT_BG_COUNTS)), *sc.table, *sc.bg_medium, *sc.aer_tail("arrays"))
        out["n_capped"] = int(n_capped.item())
        return out

    def raytracer_sw(self, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, kn_grid, photons_per_pixel, seed,
                     top_at_1=False, independent_column=False, cloud=None, band_lims=None, max_events=None, phase=None):
        """The spectral loop in one call. inc_dir, inc_dif: (ngpt,) numbers on the host. Returns the four surface / top fluxes
        (ncol,) in W m-2, abs_dir / abs_dif (nz, ncol) in W m-3 and n_capped (int)."""
        return self._rt_sw_loop(True, False, photons_per_pixel, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, kn_grid,
                                seed, top_at_1, independent_column, cloud, band_lims, max_events, phase)

    def raytracer_sw_bg(self, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, kn_grid, photons_per_pixel, seed,
                        top_at_1=False, independent_column=False, cloud=None, band_lims=None, max_events=None, phase=None,
                        background=None, aerosol=None):
        """raytracer_sw with a background. Beside its outputs: toa_up, tod_dn_dir, tod_dn_dif (ncol,) in W m-2 and bg_abs_dir,
        bg_abs_dif (nbg,) in W m-3 of a domain-wide layer (zeros without a background). With aerosol= or
        background.aerosol it is rrx_raytracer_sw_aer."""
        return self._rt_sw_loop(False, False, photons_per_pixel, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, kn_grid,
                                seed, top_at_1, independent_column, cloud, band_lims, max_events, phase, background, aerosol)

    def raytracer_sw_spectral(self, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, kn_grid, photons_per_pixel_gpt,
                              seed, top_at_1=False, independent_column=False, cloud=None, band_lims=None, max_events=None, phase=None,
                              background=None, aerosol=None):
        """raytracer_sw_bg with photons_per_pixel_gpt (ngpt,) photons per pixel of each g-point (pipeline.spectral_allocation deals
        them by flux) in place of photons_per_pixel, all g-points in one trace launch per chunk. The same outputs."""
        return self._rt_sw_loop(False, True, photons_per_pixel_gpt, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif,
                                kn_grid, seed, top_at_1, independent_column, cloud, band_lims, max_events, phase, background, aerosol)

    # ---- the backward tracer (rrx_rt_bw_trace_counts, rrx_raytracer_bw and their forms): the scene arguments of the
    # forward tracer, k_null from rt_k_null, and a sensor
    def _rt_bw_trace_counts(self, grid, tau, ssa, igpt, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, kn_grid, k_null, camera, seed, ray0, nrays,
                            top_at_1, cloud, band_lims, counts, max_events, phase, background=None, bg_profile=None, aerosol=None):
        sc = RtScene(self, band_lims).set_grid(tau, nx, ny, dz, kn_grid, top_at_1, cloud, ssa, dx, dy, sfc_albedo, mu0, azimuth)
        sensor = self._rt_sensor(camera)
        sc.set_medium("trace", "rt_bw_trace_counts", phase, background, aerosol, grid=grid, igpt=igpt, bg_profile=bg_profile)
        counts = self.rt_bw_zero_counts(sensor[1]*sensor[2]) if counts is None else counts
        self._c(sc.entry, *sc.dims, igpt, sc.flags[0], *sc.grid("trace"), *sc.kn, k_null, *sensor, *sc.run(seed, max_events, ray0, nrays),
                counts["counts"], counts["n_capped"], counts["n_clamped"], *sc.table, *sc.bg_tail, *sc.aer_tail("trace"))
        return counts

    def rt_bw_trace_counts(self, tau, ssa, igpt, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, kn_grid, k_null, camera, seed, ray0, nrays,
                           top_at_1=False, cloud=None, band_lims=None, counts=None, max_events=None, phase=None):
        """Adds the rays [ray0, ray0 + nrays) of g-point igpt into counts (rt_bw_zero_counts; made when None): counts (npix,),
        n_capped, n_clamped, int64 tensors holding unsigned 64-bit numbers."""
        return self._rt_bw_trace_counts(True, tau, ssa, igpt, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, kn_grid, k_null, camera, seed, ray0,
                                        nrays, top_at_1, cloud, band_lims, counts, max_events, phase)

    def rt_bw_trace_counts_bg(self, tau, ssa, igpt, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, kn_grid, k_null, camera, seed, ray0, nrays,
                              top_at_1=False, cloud=None, band_lims=None, counts=None, max_events=None, phase=None, background=None,
                              bg_profile=None, aerosol=None):
        """rt_bw_trace_counts with a background: bg_profile is rt_bg_profile's for igpt (made when None). With aerosol= or
        background.aerosol it is rrx_rt_bw_trace_counts_aer: k_null is then rt_k_null's with aerosol= and
        bg_profile the 7-row profile."""
        return self._rt_bw_trace_counts(False, tau, ssa, igpt, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, kn_grid, k_null, camera, seed, ray0,
                                        nrays, top_at_1, cloud, band_lims, counts, max_events, phase, background, bg_profile, aerosol)

    def _rt_bw_loop(self, grid, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, kn_grid, camera, rays_per_pixel, seed,
                    top_at_1, cloud, band_lims, max_events, phase, background=None, aerosol=None):
        sc = RtScene(self, band_lims).set_grid(tau, nx, ny, dz, kn_grid, top_at_1, cloud, ssa, dx, dy, sfc_albedo, mu0, azimuth)
        inc_dir, = self._rt_per_gpt(sc.ngpt, inc_dir=inc_dir)
        sc.set_medium("loop", "raytracer_bw", phase, background, aerosol, grid=grid)
        sensor = self._rt_sensor(camera)
        radiance, n_capped, n_clamped = self._rt_radiance((sensor[2], sensor[1]))
        self._c(sc.entry, *sc.dims, sc.flags[0], *sc.grid("loop"), inc_dir, *sc.kn, *sensor, rays_per_pixel, *sc.run(seed, max_events),
                radiance, n_capped, n_clamped, *sc.table, *sc.bg_medium, *sc.aer_tail("pointers"))
        return dict(radiance=radiance, n_capped=int(n_capped.item()), n_clamped=int(n_clamped.item()))

    def raytracer_bw(self, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, kn_grid, camera, rays_per_pixel, seed,
                     top_at_1=False, cloud=None, band_lims=None, max_events=None, phase=None):
        """The spectral loop in one call. inc_dir: (ngpt,) numbers on the host. Returns radiance (npy, npx) in W m-2 sr-1, n_capped and
        n_clamped (ints)."""
        return self._rt_bw_loop(True, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, kn_grid, camera, rays_per_pixel, seed,
                                top_at_1, cloud, band_lims, max_events, phase)

    def raytracer_bw_bg(self, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, kn_grid, camera, rays_per_pixel, seed,
                        top_at_1=False, cloud=None, band_lims=None, max_events=None, phase=None, background=None, aerosol=None):
        """raytracer_bw with a background: radiance (npy, npx) in W m-2 sr-1, n_capped and n_clamped (ints). With aerosol= or
        background.aerosol it is rrx_raytracer_bw_aer."""
        return self._rt_bw_loop(False, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, kn_grid, camera, rays_per_pixel, seed,
                                top_at_1, cloud, band_lims, max_events, phase, background, aerosol)

    # The backward tracer with the rays of all g-points in one launch, counts by band and a channel matrix (rrx_camera_trace_counts_spectral,
    # rrx_camera_channels, rrx_camera_render_spectral). Built on the aerosol form like the forward spectral entries; band_lims
    # is always needed (the counts are kept by band). ngpt <= 1024.
    def camera_trace_counts_spectral(self, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, ray_end, weight0, kn_grid, k_null, camera,
                                     seed, ray0, nrays, band_lims, top_at_1=False, cloud=None, counts=None, max_events=None, phase=None,
                                     background=None, bg_profile=None, aerosol=None):
        """Adds the rays [ray0, ray0 + nrays) of the concatenated list into counts (camera_zero_counts; made when None): counts
        (nbnd, npix), n_capped, n_clamped. ray_end (ngpt+1,) int64 and weight0 (ngpt,): arrays on the host, checked and uploaded here;
        k_null is rt_k_null_all's and bg_profile rt_bg_profile_all's (made when None)."""
        sc = RtScene(self, band_lims, camera=True).set_grid(tau, nx, ny, dz, kn_grid, top_at_1, cloud, ssa, dx, dy, sfc_albedo, mu0, azimuth)
        sensor = self._rt_sensor(camera)
        lists = self._rt_list(sc.ngpt, "rays", ray0, nrays, ray_end=ray_end, weight0=weight0)
        sc.set_medium("trace", "camera_trace_counts", phase, background, aerosol, spectral=True, bg_profile=bg_profile)
        counts = self.camera_zero_counts(sc.nbnd, sensor[1]*sensor[2]) if counts is None else counts
        self._c(sc.entry, *sc.dims, sc.flags[0], *sc.grid("camera"), *lists, *sc.kn, k_null, *sensor, *sc.run(seed, max_events, ray0, nrays),
                counts["counts"], counts["n_capped"], counts["n_clamped"], *sc.table, *sc.bg_tail, *sc.aer_tail("trace"))
        return counts

    def camera_channels(self, counts, chan_weights, scale, out=None):
        """out (nchan, npix) = scale x chan_weights (nchan, nbnd) @ (counts (nbnd, npix) 2^-32), the sum in band order"""
        nbnd, npix = counts.shape
        M = self.asarray(self._rt_chan_weights(chan_weights, nbnd))
        out = self.empty((M.shape[0], npix)) if out is None else out
        self._c("camera_channels", npix, nbnd, int(M.shape[0]), counts, M, scale, out)
        return out

    def camera_render_spectral(self, tau, ssa, nx, ny, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, kn_grid, camera, rays_per_pixel_gpt, seed,
                               band_lims, chan_weights, top_at_1=False, cloud=None, max_events=None, phase=None, background=None,
                               aerosol=None):
        """raytracer_bw_bg with rays_per_pixel_gpt (ngpt,) rays per pixel of each g-point (pipeline.spectral_allocation deals them by
        flux) in place of rays_per_pixel, all g-points in one trace launch per chunk, and chan_weights (nchan, nbnd) on the host, the
        matrix from bands to channels. Returns radiance (nchan, npy, npx) in W m-2 sr-1, n_capped and n_clamped (ints)."""
        sc = RtScene(self, band_lims, camera=True).set_grid(tau, nx, ny, dz, kn_grid, top_at_1, cloud, ssa, dx, dy, sfc_albedo, mu0, azimuth)
        inc_dir, = self._rt_per_gpt(sc.ngpt, inc_dir=inc_dir)
        rays, = self._rt_per_gpt(sc.ngpt, rays_per_pixel_gpt=rays_per_pixel_gpt)
        M = self._rt_chan_weights(np.asarray(chan_weights), sc.nbnd)
        sc.set_medium("loop", "camera_render", phase, background, aerosol, spectral=True)
        sensor = self._rt_sensor(camera)
        radiance, n_capped, n_clamped = self._rt_radiance((M.shape[0], sensor[2], sensor[1]))
        self._c(sc.entry, *sc.dims, sc.flags[0], *sc.grid("camera"), inc_dir, *sc.kn, *sensor, rays, *sc.run(seed, max_events),
                int(M.shape[0]), M, radiance, n_capped, n_clamped, *sc.table, *sc.bg_medium, *sc.aer_tail("pointers"))
        return dict(radiance=radiance, n_capped=int(n_capped.item()), n_clamped=int(n_clamped.item()))

    # Thermal emission in the backward tracer (rrx_thermal_trace_counts, rrx_thermal_render): the grid form of the backward
    # tracer's scene without a sun. ssa: (ngpt, nz, ncol) or None for a gas that does not scatter; sfc_emis (ncol,); the sources are
    # radiances in W m-2 sr-1: lay_src (ngpt, nz, ncol), sfc_src (ngpt, ncol); k_null from rt_k_null.
    def _thermal_scene(self, tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, kn_grid, top_at_1, cloud, band_lims):
        """(the gathered scene; tau ... sfc_src in the header's order)"""
        sc = RtScene(self, band_lims).set_grid(tau, nx, ny, dz, kn_grid, top_at_1, cloud, ssa, dx, dy, sfc_emis)
        if tuple(lay_src.shape) != tuple(tau.shape) or tuple(sfc_src.shape) != (sc.ngpt, sc.ncol) or tuple(sfc_emis.shape) != (sc.ncol,):
            raise ValueError(f"thermal: lay_src is (ngpt, nz, ncol) = {tuple(tau.shape)}, sfc_src (ngpt, ncol) and sfc_emis (ncol,), got "
                             f"{tuple(lay_src.shape)}, {tuple(sfc_src.shape)}, {tuple(sfc_emis.shape)}")
        return sc, (sc.tau, sc.ssa, sc.lims("trace"), *sc.cloud, *sc.geometry[:4], lay_src, sfc_src)

    def thermal_trace_counts(self, tau, ssa, igpt, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, top_radiance, kn_grid, k_null, camera, seed,
                             ray0, nrays, top_at_1=False, cloud=None, band_lims=None, counts=None, max_events=None):
        """Adds the rays [ray0, ray0 + nrays) of g-point igpt into counts (rt_bw_zero_counts; made when None): counts (npix,), n_capped,
        n_clamped, int64 tensors holding unsigned 64-bit numbers. top_radiance: one number, the isotropic downward radiance at the domain
        top. Radiance of the g-point = counts 2^-32 / rays_per_pixel."""
        sc, scene = self._thermal_scene(tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, kn_grid, top_at_1, cloud, band_lims)
        sensor = self._rt_sensor(camera)
        counts = self.rt_bw_zero_counts(sensor[1]*sensor[2]) if counts is None else counts
        self._c("thermal_trace_counts", *sc.dims, igpt, sc.flags[0], *scene, float(top_radiance), *sc.kn, k_null, *sensor,
                *sc.run(seed, max_events, ray0, nrays), counts["counts"], counts["n_capped"], counts["n_clamped"])
        return counts

    def thermal_render(self, tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, kn_grid, camera, rays_per_pixel, seed, top_at_1=False,
                       cloud=None, band_lims=None, max_events=None, top_radiance=None, by_band=False):
        """The loop over all g-points in one call. top_radiance: None (0) or (ngpt,) numbers on the host. Returns radiance in W m-2 sr-1,
        (npy, npx), or with by_band (which needs band_lims) (nbnd, npy, npx), n_capped and n_clamped (ints). With a flux sensor
        pi x radiance is the irradiance of the pixel."""
        sc, scene = self._thermal_scene(tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, kn_grid, top_at_1, cloud, band_lims)
        if by_band and band_lims is None:
            raise ValueError("thermal: by_band needs band_lims")
        if top_radiance is not None:
            top_radiance, = self._rt_per_gpt(sc.ngpt, top_radiance=top_radiance)
        sensor = self._rt_sensor(camera)
        radiance, n_capped, n_clamped = self._rt_radiance((sc.nbnd, sensor[2], sensor[1]) if by_band else (sensor[2], sensor[1]))
        lims = band_lims if by_band else scene[2]
        self._c("thermal_render", *sc.dims, sc.flags[0], *scene[:2], lims, *scene[3:], top_radiance, *sc.kn, *sensor, rays_per_pixel,
                *sc.run(seed, max_events), by_band, radiance, n_capped, n_clamped)
        return dict(radiance=radiance, n_capped=int(n_capped.item()), n_clamped=int(n_clamped.item()))

    # The thermal tracer with the rays of all g-points in one launch, counts by band and a channel matrix
    # (rrx_thermal_trace_counts_spectral, rrx_thermal_render_spectral). band_lims is always needed (the counts are kept by
    # band); the counts are converted by camera_channels. ngpt <= 1024.
    def _thermal_spectral_scene(self, who, tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, kn_grid, top_at_1, cloud, band_lims):
        """(the gathered scene; tau ... sfc_src with band_lims whether there is cloud or not)"""
        if band_lims is None:
            raise ValueError(f"thermal: {who} needs band_lims (the counts are kept by band)")
        sc, scene = self._thermal_scene(tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, kn_grid, top_at_1, cloud, band_lims)
        return sc, (*scene[:2], band_lims, *scene[3:])

    def thermal_trace_counts_spectral(self, tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, top_radiance, ray_end, weight0, kn_grid,
                                      k_null, camera, seed, ray0, nrays, band_lims, top_at_1=False, cloud=None, counts=None, max_events=None):
        """Adds the rays [ray0, ray0 + nrays) of the concatenated list into counts (camera_zero_counts; made when None): counts
        (nbnd, npix), n_capped, n_clamped. ray_end (ngpt+1,) int64, weight0 (ngpt,) and top_radiance, None (0) or (ngpt,): arrays on the
        host, checked and uploaded here; k_null is rt_k_null_all's."""
        sc, scene = self._thermal_spectral_scene("thermal_trace_counts_spectral", tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src,
                                                 kn_grid, top_at_1, cloud, band_lims)
        sensor = self._rt_sensor(camera)
        if top_radiance is None:
            top, lists = None, self._rt_list(sc.ngpt, "rays", ray0, nrays, ray_end=ray_end, weight0=weight0)
        else:
            *lists, top = self._rt_list(sc.ngpt, "rays", ray0, nrays, ray_end=ray_end, weight0=weight0, top_radiance=top_radiance)
        counts = self.camera_zero_counts(sc.nbnd, sensor[1]*sensor[2]) if counts is None else counts
        self._c("thermal_trace_counts_spectral", *sc.dims, sc.flags[0], *scene, top, *lists, *sc.kn, k_null, *sensor,
                *sc.run(seed, max_events, ray0, nrays), counts["counts"], counts["n_capped"], counts["n_clamped"])
        return counts

    def thermal_render_spectral(self, tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, kn_grid, camera, rays_per_pixel_gpt, seed,
                                band_lims, chan_weights, top_at_1=False, cloud=None, max_events=None, top_radiance=None):
        """thermal_render with rays_per_pixel_gpt (ngpt,) rays per pixel of each g-point (pipeline.spectral_allocation deals them by
        emission) in place of rays_per_pixel, all g-points in one trace launch per chunk, and chan_weights (nchan, nbnd) on the host, the
        matrix from bands to channels. A g-point with no rays is left out of the result. Returns radiance (nchan, npy, npx) in
        W m-2 sr-1, n_capped and n_clamped (ints)."""
        sc, scene = self._thermal_spectral_scene("thermal_render_spectral", tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src,
                                                 kn_grid, top_at_1, cloud, band_lims)
        rays, = self._rt_per_gpt(sc.ngpt, rays_per_pixel_gpt=rays_per_pixel_gpt)
        if top_radiance is not None:
            top_radiance, = self._rt_per_gpt(sc.ngpt, top_radiance=top_radiance)
        M = self._rt_chan_weights(np.asarray(chan_weights), sc.nbnd)
        sensor = self._rt_sensor(camera)
        radiance, n_capped, n_clamped = self._rt_radiance((M.shape[0], sensor[2], sensor[1]))
        self._c("thermal_render_spectral", *sc.dims, sc.flags[0], *scene, top_radiance, *sc.kn, *sensor, rays, *sc.run(seed, max_events),
                int(M.shape[0]), M, radiance, n_capped, n_clamped)
        return dict(radiance=radiance, n_capped=int(n_capped.item()), n_clamped=int(n_clamped.item()))

    # 3-D longwave heating from cell sensors (rrx_heating3d_counts, rrx_heating3d_counts_spectral,
    # rrx_heating3d_render): the thermal tracer's scene without a sensor. Ray r belongs to cell r mod (nx ny nz);
    # counts (nz, ncol) are int64 tensors holding SIGNED 64-bit numbers in units of 2^-32 W m-2, in the layout of lay_src[g].
    def thermal_heating_zero_counts(self, nz, ncol):
        return self._rt_zeros(counts=(nz, ncol), n_capped=(1,), n_clamped=(1,))

    def thermal_heating_counts(self, tau, ssa, igpt, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, top_radiance, kn_grid, k_null, seed,
                               ray0, nrays, top_at_1=False, cloud=None, band_lims=None, counts=None, max_events=None):
        """Adds the rays [ray0, ray0 + nrays) of g-point igpt into counts (thermal_heating_zero_counts; made when None): counts
        (nz, ncol), n_capped, n_clamped. top_radiance: one number. With m rays per cell flux_conv of the g-point = counts 2^-32 / m."""
        sc, scene = self._thermal_scene(tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, kn_grid, top_at_1, cloud, band_lims)
        counts = self.thermal_heating_zero_counts(sc.nz, sc.ncol) if counts is None else counts
        self._c("heating3d_counts", *sc.dims, igpt, sc.flags[0], *scene, float(top_radiance), *sc.kn, k_null,
                *sc.run(seed, max_events, ray0, nrays), counts["counts"], counts["n_capped"], counts["n_clamped"])
        return counts

    def thermal_heating_counts_spectral(self, tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, top_radiance, ray_end, weight0, kn_grid,
                                        k_null, seed, ray0, nrays, band_lims, top_at_1=False, cloud=None, counts=None, max_events=None):
        """Adds the rays [ray0, ray0 + nrays) of the concatenated list into counts (thermal_heating_zero_counts; made when None): one
        (nz, ncol) for all g-points, n_capped, n_clamped. ray_end (ngpt+1,) int64, weight0 (ngpt,) and top_radiance, None (0) or
        (ngpt,): arrays on the host, checked and uploaded here; k_null is rt_k_null_all's."""
        sc, scene = self._thermal_spectral_scene("thermal_heating_counts_spectral", tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src,
                                                 kn_grid, top_at_1, cloud, band_lims)
        if top_radiance is None:
            top, lists = None, self._rt_list(sc.ngpt, "rays", ray0, nrays, ray_end=ray_end, weight0=weight0)
        else:
            *lists, top = self._rt_list(sc.ngpt, "rays", ray0, nrays, ray_end=ray_end, weight0=weight0, top_radiance=top_radiance)
        counts = self.thermal_heating_zero_counts(sc.nz, sc.ncol) if counts is None else counts
        self._c("heating3d_counts_spectral", *sc.dims, sc.flags[0], *scene, top, *lists, *sc.kn, k_null,
                *sc.run(seed, max_events, ray0, nrays), counts["counts"], counts["n_capped"], counts["n_clamped"])
        return counts

    def thermal_heating_render(self, tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src, kn_grid, rays_per_cell_gpt, seed, band_lims,
                               top_at_1=False, cloud=None, max_events=None, top_radiance=None):
        """rays_per_cell_gpt (ngpt,) rays per cell of each g-point, all g-points in one trace launch per chunk, one conversion. A g-point
        with no rays is left out of the result. Returns flux_conv (nz, ncol) in W m-2, the net radiative power that a cell takes up per
        unit horizontal area, n_capped and n_clamped (ints)."""
        sc, scene = self._thermal_spectral_scene("thermal_heating_render", tau, ssa, nx, ny, dx, dy, dz, sfc_emis, lay_src, sfc_src,
                                                 kn_grid, top_at_1, cloud, band_lims)
        rays = np.ascontiguousarray(rays_per_cell_gpt, dtype=np.int64).reshape(-1)
        if rays.size != sc.ngpt:
            raise ValueError("thermal: rays_per_cell_gpt is (ngpt,)")
        if top_radiance is not None:
            top_radiance, = self._rt_per_gpt(sc.ngpt, top_radiance=top_radiance)
        flux_conv, n_capped, n_clamped = self._rt_radiance((sc.nz, sc.ncol))
        self._c("heating3d_render", *sc.dims, sc.flags[0], *scene, top_radiance, *sc.kn, rays, *sc.run(seed, max_events),
                flux_conv, n_capped, n_clamped)
        return dict(flux_conv=flux_conv, n_capped=int(n_capped.item()), n_clamped=int(n_clamped.item()))

    def delta_scale_2str_k(self, tau, ssa, g):
        ngpt, nlay, ncol = tau.shape
        self._c("delta_scale_2str_k", ncol, nlay, ngpt, tau, ssa, g)

    def sum_broadband(self, gpt_flux, out=None):
        ngpt, nlev, ncol = gpt_flux.shape
        out = self.empty((nlev, ncol)) if out is None else out
        self._c("sum_broadband", ncol, nlev, ngpt, gpt_flux, out)
        return out

    def net_broadband_precalc(self, flux_dn, flux_up, out=None):
        nlev, ncol = flux_dn.shape
        out = self.empty((nlev, ncol)) if out is None else out
        self._c("net_broadband_precalc", ncol, nlev, flux_dn, flux_up, out)
        return out

    def heating_rate(self, flux_net, plev, g_over_cp=9.80665/1004.64):
        nlev, ncol = flux_net.shape
        out = self.empty((nlev-1, ncol))
        self._c("heating_rate", ncol, nlev-1, g_over_cp, flux_net, plev, out)
        return out

    def sum_byband(self, gpt_flux, band_lims):
        ngpt, nlev, ncol = gpt_flux.shape
        nbnd = band_lims.shape[0]
        out = self.empty((nbnd, nlev, ncol))
        self._c("sum_byband", ncol, nlev, ngpt, nbnd, band_lims, gpt_flux, out)
        return out

    def net_byband_full(self, gpt_dn, gpt_up, band_lims):
        ngpt, nlev, ncol = gpt_dn.shape
        nbnd = band_lims.shape[0]
        out = self.empty((nbnd, nlev, ncol))
        self._c("net_byband_full", ncol, nlev, ngpt, nbnd, band_lims, gpt_dn, gpt_up, out)
        return out

    # ---- host-class helpers --------------------------------------------------------------------------
    def get_col_dry(self, vmr_h2o, plev, out=None):
        nlay, ncol = vmr_h2o.shape
        out = self.empty((nlay, ncol)) if out is None else out
        self._c("get_col_dry", ncol, nlay, vmr_h2o, plev, out)
        return out

    @staticmethod
    def _vmr_dims(name, v, nlay, ncol):
        """(dim1, dim2) of a gas concentration as rrx_fill_gases[_all] take it: a scalar (any tensor of one element) is (1, 1), a profile
        (nlay,) or (nlay, 1) is (1, nlay), a field (nlay, ncol) is (ncol, nlay); any other shape is refused."""
        shape = tuple(v.shape)
        if v.numel() == 1:
            return 1, 1
        if shape in ((nlay,), (nlay, 1)):
            return 1, nlay
        if shape == (nlay, ncol):
            return ncol, nlay
        raise ValueError(f"fill_gases: {name} has shape {shape}; expected a scalar, a profile ({nlay},) or ({nlay}, 1), "
                         f"or a field ({nlay}, {ncol})")

    def fill_gases(self, kd, vmr_by_name, col_dry):
        """col_gas(ncol,nlay,0:ngas): slot 0 = col_dry, slot i = vmr_i * col_dry
        (/root/reference/src_cuda/Gas_optics_rrtmgp.cu:392-422,1023-1028). A concentration is a scalar, a profile (nlay,) or
        (nlay, 1) shared by all columns, or a field (nlay, ncol)."""
        nlay, ncol = col_dry.shape
        col_gas = self.empty((kd.ngas+1, nlay, ncol))
        vs = [vmr_by_name[name] for name in kd.gas_names]
        dims = [self._vmr_dims(name, v, nlay, ncol) for name, v in zip(kd.gas_names, vs)]
        if len(vs) <= 32:                      # one launch for all gases
            self._c("fill_gases_all", ncol, nlay, len(vs), (ctypes.c_void_p * len(vs))(*[v.data_ptr() for v in vs]),
                    (ctypes.c_int * len(vs))(*[d[0] for d in dims]), (ctypes.c_int * len(vs))(*[d[1] for d in dims]), col_gas, col_dry)
            return col_gas
        vmr = self.empty((kd.ngas, nlay, ncol))
        self._c("fill_gases", ncol, nlay, ncol, nlay, kd.ngas, 0, vmr, col_dry, col_gas, col_dry)
        for i, (v, (d1, d2)) in enumerate(zip(vs, dims), start=1):
            self._c("fill_gases", ncol, nlay, d1, d2, kd.ngas, i, vmr, v, col_gas, col_dry)
        return col_gas

    def expand_and_transpose(self, band_lims, arr_in, ngpt, out=None):
        ncol, nbnd = arr_in.shape
        out = self.empty((ngpt, ncol)) if out is None else out
        self._c("expand_and_transpose", ncol, nbnd, band_lims, arr_in, out)
        return out

    def spread_col(self, ncol, solar_source):
        out = self.empty((solar_source.shape[0], ncol))
        self._c("spread_col", ncol, solar_source.shape[0], out, solar_source)
        return out

    def toa_source(self, ncol, solar_source, tsi_scaling):
        """spread_col + scaling_to_subset in one launch: toa_src(igpt, icol) = solar_source(igpt) * tsi_scaling(icol)."""
        out = self.empty((solar_source.shape[0], ncol))
        self._c("toa_source", ncol, solar_source.shape[0], out, solar_source, tsi_scaling)
        return out

    def scaling_to_subset(self, toa_src, tsi_scaling):
        ngpt, ncol = toa_src.shape
        self._c("scaling_to_subset", ncol, ngpt, toa_src, tsi_scaling)

    def cloud_optics_2str(self, lut, clwp, ciwp, reliq, deice, delta_scale=False):
        """delta_scale: cloud_optics followed by delta_scale_2str_k in one pass (the same bits)."""
        nlay, ncol = clwp.shape
        nbnd = lut["lut_extliq"].shape[0]
        tau = self.empty((nbnd, nlay, ncol)); ssa = self.empty((nbnd, nlay, ncol)); g = self.empty((nbnd, nlay, ncol))
        self._c("cloud_optics_2str_delta" if delta_scale else "cloud_optics_2str", ncol, nlay, nbnd, lut["nsize_liq"], lut["nsize_ice"],
                lut["radliq_lwr"], lut["radliq_upr"], lut["diamice_lwr"], lut["diamice_upr"],
                lut["lut_extliq"], lut["lut_ssaliq"], lut["lut_asyliq"], lut["lut_extice"], lut["lut_ssaice"], lut["lut_asyice"],
                clwp, ciwp, reliq, deice, tau, ssa, g)
        return tau, ssa, g

    def aerosol_optics(self, lut, aermr, rh, plev):
        """CAMS aerosol optics per band (src_cuda/Aerosol_optics.cu). aermr: aermr01..11, each (nlay, ncol) or an (nlay,)
        profile shared by all columns (read in place, not broadcast)."""
        nlay, ncol = rh.shape
        nphobic, nbnd = lut["mext_phobic"].shape
        nphilic, nhum = lut["mext_philic"].shape[:2]
        if len(aermr) != 11:
            raise ValueError("aerosol optics needs the 11 mixing ratios aermr01..aermr11")
        for m in aermr:
            if tuple(m.shape) not in ((nlay, ncol), (nlay,)):
                raise ValueError("aerosol mixing ratio must be (nlay, ncol) or (nlay,)")
        ptrs = (ctypes.c_void_p * 11)(*[m.data_ptr() for m in aermr])
        per_col = (ctypes.c_int * 11)(*[1 if m.dim() == 2 else 0 for m in aermr])
        tau = self.empty((nbnd, nlay, ncol)); ssa = self.empty((nbnd, nlay, ncol)); g = self.empty((nbnd, nlay, ncol))
        self._c("aerosol_optics", ncol, nlay, nbnd, nhum, nphobic, nphilic, ptrs, per_col, rh, plev, lut["rh_upper"],
                lut["mext_phobic"], lut["ssa_phobic"], lut["g_phobic"], lut["mext_philic"], lut["ssa_philic"], lut["g_philic"],
                tau, ssa, g)
        return tau, ssa, g

    def cloud_optics_1scl(self, lut, clwp, ciwp, reliq, deice):
        nlay, ncol = clwp.shape
        nbnd = lut["lut_extliq"].shape[0]
        tau = self.empty((nbnd, nlay, ncol))
        self._c("cloud_optics_1scl", ncol, nlay, nbnd, lut["nsize_liq"], lut["nsize_ice"],
                lut["radliq_lwr"], lut["radliq_upr"], lut["diamice_lwr"], lut["diamice_upr"],
                lut["lut_extliq"], lut["lut_ssaliq"], lut["lut_asyliq"], lut["lut_extice"], lut["lut_ssaice"], lut["lut_asyice"],
                clwp, ciwp, reliq, deice, tau)
        return tau

    def upload_lut(self, lut):
        return {k: (self.asarray(v) if isinstance(v, np.ndarray) else v) for k, v in lut.items()}

    def get_from_subset(self, ncol, nlay, nbnd, ncol_in, col_s_in, fulls, subs):
        n = len(fulls)
        PA = ctypes.c_void_p * 4
        pf = PA(*[f.data_ptr() for f in fulls] + [0]*(4-n))
        ps = PA(*[s.data_ptr() for s in subs] + [0]*(4-n))
        self._c("get_from_subset", ncol, nlay, nbnd, ncol_in, col_s_in, n, pf, ps)

    def subset_cols(self, arr, col_s, ncol_sub):
        ncol_full = arr.shape[-1]
        nrest = int(np.prod(arr.shape[:-1])) if arr.dim() > 1 else 1
        out = self.empty(tuple(arr.shape[:-1]) + (ncol_sub,))
        self._c("subset_cols", ncol_full, nrest, col_s, ncol_sub, arr, out)
        return out

    def gather_cols(self, perm, src, out):
        """out[..., i] = src[..., perm[i]] for every column of out; column-last tensors with the same leading shape, perm int32."""
        nrest = int(np.prod(src.shape[:-1], dtype=np.int64)) if src.dim() > 1 else 1
        self._c("gather_cols", out.shape[-1], nrest, perm, src.shape[-1], src, out)
        return out

    def gather_lastdim(self, perm, src, out):
        """out[i, :] = src[perm[i], :] for every row of out; column-first (ncol, n1) tensors, perm int32."""
        self._c("gather_lastdim", src.shape[1], out.shape[0], perm, src, out)
        return out

    def sunlit_columns(self, mu0, order=None, pad_to=1, perm=None, count=None):
        """Stable list of the columns with mu0 > 0 (of `order`, an int32 index tensor, or of 0..ncol-1), padded to a multiple of
        pad_to by repeats of the last one. Returns (perm, count): int32 device tensors, count[0] = the unpadded count. perm= / count=:
        preallocated outputs (perm holds at least ncol rounded up to pad_to entries)."""
        ncol = int(order.numel()) if order is not None else int(mu0.shape[-1])
        for t in (order, perm, count):
            if t is not None and t.dtype != torch.int32:
                raise TypeError("sunlit_columns: order, perm and count are int32 tensors")
        if perm is None:
            perm = self.int_empty((max(-(-ncol // pad_to) * pad_to, 1),))
        if count is None:
            count = self.int_empty((1,))
        self._c("sunlit_columns", ncol, mu0, order, pad_to, perm, count)
        return perm, count

    def scatter_cols_fill(self, n, perm, src, dst):
        """dst[..., perm[i]] = src[..., i] for i < n, zeros in every other column of dst; column-last tensors (any leading shape,
        contiguous), src with at least n columns."""
        nrest = int(np.prod(dst.shape[:-1])) if dst.dim() > 1 else 1
        if perm.dtype != torch.int32:
            raise TypeError("scatter_cols_fill: perm is an int32 tensor")
        if tuple(src.shape[:-1]) != tuple(dst.shape[:-1]) or not (src.is_contiguous() and dst.is_contiguous()):
            raise ValueError("scatter_cols_fill: src and dst must be contiguous with the same leading shape")
        self._c("scatter_cols_fill", n, nrest, perm, src.shape[-1], src, dst.shape[-1], dst)
        return dst

    supports_null_g = True      # gas_optics_sw_fused / sw_solver_2stream accept g = None (asymmetry identically zero)

    def set_broadband_min_groups(self, n):
        """column groups needed before do_broadband takes the fused one-kernel form (default 512; 1 = always)"""
        self.lib.call("rrx_set_broadband_min_groups", n)

    def set_broadband_gsplit(self, n):
        self.lib.call("rrx_set_broadband_gsplit", n)

    def set_variant(self, lw=None, sw=None):
        if lw is not None:
            self.lib.call("rrx_set_lw_variant", lw)
        if sw is not None:
            self.lib.call("rrx_set_sw_variant", sw)
