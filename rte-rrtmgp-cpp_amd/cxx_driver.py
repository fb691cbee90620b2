"""bench.py --driver cxx / tests: the C++ host classes (Radiation_solver_longwave / _shortwave::solve_gpu, the reference's class
structure: include_test/Radiation_solver.h) driven from Python on device arrays torch owns, through the C entry points of
rte-rrtmgp-cpp_amd/host/src_test/cxx_driver_api.cpp in librte_rrtmgp_hip[_sp].so. The k-distributions travel as the files the
reference's driver reads (synthetic_files.write_case)."""
import ctypes
import os
import tempfile

import numpy as np

from . import synthetic_files

HERE = os.path.dirname(os.path.abspath(__file__))


class CxxDriver:
    def __init__(self, be, kd_lw0, kd_sw0, atm, cloud_luts0=None, column_block=16384, broadband=True, sort_mode=-1, pad=True,
                 sunlit=False, jacobian=False, n_gauss_angles=1, optimal_angles=False, lw_scattering=False,
                 lw_rescaling=False, cloud_fraction=None, cloud_overlap="max_ran", overlap_param=None, mcica_seed=0, mcica_col_offset=0,
                 altitude=None, ref_altitude=None, planet_radius=6.37123e6):
        import torch
        self.torch, self.be, self.atm = torch, be, atm
        self.f64 = be.np_dtype == np.float64
        path = os.path.join(HERE, "lib", "librte_rrtmgp_hip.so" if self.f64 else "librte_rrtmgp_hip_sp.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build the host layer (make -C rte-rrtmgp-cpp_amd/host [PRECISION=sp])")
        self.lib = ctypes.CDLL(path)
        self.lib.rrx_cxx_driver_create.restype = ctypes.c_void_p
        self.lib.rrx_cxx_driver_error.restype = ctypes.c_char_p
        self.dir = tempfile.mkdtemp(prefix="rrx_cxx_")
        synthetic_files.write_kdist(os.path.join(self.dir, "coefficients_lw.nc"), kd_lw0)
        synthetic_files.write_kdist(os.path.join(self.dir, "coefficients_sw.nc"), kd_sw0)
        if cloud_luts0 is not None:
            synthetic_files.write_cloud_lut(os.path.join(self.dir, "cloud_coefficients_lw.nc"), cloud_luts0[0])
            synthetic_files.write_cloud_lut(os.path.join(self.dir, "cloud_coefficients_sw.nc"), cloud_luts0[1])
        self.clouds = cloud_luts0 is not None
        names = list(atm.vmr.keys())
        arr = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
        self.h = self.lib.rrx_cxx_driver_create(self.dir.encode(), len(names), arr, int(self.clouds), int(bool(atm.top_at_1)))
        if not self.h:
            raise RuntimeError("rrx_cxx_driver_create: " + self.lib.rrx_cxx_driver_error().decode())
        self.h = ctypes.c_void_p(self.h)
        self._check(self.lib.rrx_cxx_driver_settings(self.h, int(column_block), int(broadband), int(sort_mode), int(pad)))
        if sunlit:                                  # SW on the columns with mu0 > 0 only, zeros elsewhere (set_sunlit_columns)
            self._check(self.lib.rrx_cxx_sunlit_columns(self.h, 1))
        # n_gauss_angles: LW quadrature angles, 1..4 (set_gauss_angles; the default launches what it always did)
        self.n_gauss_angles = int(n_gauss_angles)
        if self.n_gauss_angles != 1:
            self._check(self.lib.rrx_cxx_lw_gauss_angles(self.h, self.n_gauss_angles))
        # optimal_angles: the one LW angle's secant from the coefficient file's optimal_angle_fit (set_optimal_angles)
        self.optimal_angles = bool(optimal_angles)
        if self.optimal_angles:
            self._check(self.lib.rrx_cxx_lw_optimal_angles(self.h, 1))
        # lw_scattering: LW two-stream solve with cloud scattering (set_lw_scattering); the refused pairs fail at the first step
        self.lw_scattering = bool(lw_scattering)
        if self.lw_scattering:
            self._check(self.lib.rrx_cxx_lw_scattering(self.h, 1))
        # lw_rescaling: LW no-scattering solve on rescaled optical depths with one correction sweep (set_lw_rescaling); the refused
        # pairs fail at the first step
        self.lw_rescaling = bool(lw_rescaling)
        if self.lw_rescaling:
            self._check(self.lib.rrx_cxx_lw_rescaling(self.h, 1))
        # jacobian: each step also fills self.lw_flux_up_jac (nlev, ncol), d lw_flux_up / d t_sfc [W m-2 K-1] (set_jacobian)
        self.jacobian = bool(jacobian)
        if self.jacobian:
            self._check(self.lib.rrx_cxx_lw_jacobian(self.h, 1))
        # cloud_fraction: McICA cloud sampling (set_cloud_sampling of both solvers), as pipeline.ResidentSolver takes it; the tensors
        # are borrowed by the solvers, set self.mcica_seed to advance the mask between steps
        self.cloud_fraction, self.overlap_param, self.cloud_overlap = cloud_fraction, overlap_param, cloud_overlap
        self.mcica_seed, self.mcica_col_offset = int(mcica_seed), int(mcica_col_offset)
        if cloud_fraction is not None:
            if cloud_overlap not in ("max_ran", "exp_ran"):
                raise ValueError(f"CxxDriver: cloud_overlap = {cloud_overlap!r} is not 'max_ran' or 'exp_ran'")
            self._set_cloud_sampling()
        # altitude: the SW solve takes a cosine of the solar zenith angle per layer, corrected for the planet's curvature from mu0
        # (set_spherical_mu0), as pipeline.ResidentSolver(altitude=, ref_altitude=) does; the tensors are borrowed by the solver
        self.altitude, self.ref_altitude = altitude, ref_altitude
        if ref_altitude is not None and altitude is None:
            raise ValueError("CxxDriver: ref_altitude without altitude")
        if altitude is not None:
            if tuple(altitude.shape) != (atm.nlay, atm.ncol) or (ref_altitude is not None and tuple(ref_altitude.shape) != (atm.ncol,)):
                raise ValueError("CxxDriver: altitude must be (nlay, ncol) and ref_altitude (ncol)")
            self._check(self.lib.rrx_cxx_spherical_mu0(
                self.h, ctypes.c_void_p(altitude.data_ptr()), atm.ncol, atm.nlay,
                ctypes.c_void_p(ref_altitude.data_ptr() if ref_altitude is not None else 0), ctypes.c_double(float(planet_radius))))
        for n, t in atm.vmr.items():                # (nlay, ncol) tensors = (ncol, nlay) arrays; profiles (nlay,) = (1, nlay)
            n1, n2 = (t.shape[1], t.shape[0]) if t.dim() == 2 else ((1, t.shape[0]) if t.dim() == 1 else (1, 1))
            self._check(self.lib.rrx_cxx_driver_set_gas(self.h, n.encode(), ctypes.c_void_p(t.data_ptr()), n1, n2))
        self.nbnd_lw, self.nbnd_sw = kd_lw0.nbnd, kd_sw0.nbnd
        self.fluxes = be.empty((7, atm.nlay + 1, atm.ncol))
        self.lw_flux_up_jac = be.empty((atm.nlay + 1, atm.ncol)) if self.jacobian else None
        self.sort_columns = sort_mode

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError("cxx driver: " + self.lib.rrx_cxx_driver_error().decode())

    def _set_cloud_sampling(self):
        f, al = self.cloud_fraction, self.overlap_param
        self._check(self.lib.rrx_cxx_cloud_sampling(
            self.h, ctypes.c_void_p(f.data_ptr()), int(f.shape[1]), int(f.shape[0]), 1 if self.cloud_overlap == "exp_ran" else 0,
            ctypes.c_void_p(al.data_ptr() if al is not None else 0), ctypes.c_ulonglong(self.mcica_seed & 0xFFFFFFFFFFFFFFFF),
            self.mcica_col_offset))
        self._seed_set = self.mcica_seed

    def step(self):
        a = self.atm
        if self.cloud_fraction is not None and self._seed_set != self.mcica_seed:
            self._set_cloud_sampling()
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
        st = ctypes.c_void_p(self.torch.cuda.current_stream(self.be.device).cuda_stream)
        cl = (a.lwp, a.iwp, a.rel, a.dei) if self.clouds else (None, None, None, None)
        out7 = (ctypes.c_void_p * 7)(*[self.fluxes[i].data_ptr() for i in range(7)])      # the solvers write into the packed tensor
        self._check(self.lib.rrx_cxx_driver_solve(self.h, a.ncol, a.nlay, self.nbnd_lw, self.nbnd_sw, p(a.p_lay), p(a.p_lev), p(a.t_lay), p(a.t_lev),
                                                  p(a.t_sfc), p(a.emis_sfc), p(a.sfc_alb_dir), p(a.sfc_alb_dif), p(a.tsi_scaling), p(a.mu0),
                                                  p(cl[0]), p(cl[1]), p(cl[2]), p(cl[3]), out7, st))
        if self.jacobian:
            self._check(self.lib.rrx_cxx_lw_flux_up_jac(self.h, p(self.lw_flux_up_jac), st))
        return self.fluxes

    def close(self):
        if self.h:
            self.lib.rrx_cxx_driver_destroy(self.h)
            self.h = None
