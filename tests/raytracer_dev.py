"""What the GPU tests of the ray tracers (test_gpu_raytracer.py, test_gpu_raytracer_bw.py, test_gpu_raytracer_phase.py) share: a
raytracer_ref.Scene on the device, and the trace and solve entries of a backend called with a scene's numbers. phase: a
phase_tables table with the cells' radius, or None for Henyey-Greenstein."""
import numpy as np


def _be(dt, hip_f64, hip_f32):
    return hip_f64 if dt == "f64" else hip_f32


def _dev(be, sc):
    A = be.asarray
    return dict(tau=A(sc.tau), ssa=A(sc.ssa), alb=A(sc.sfc_albedo), cloud=None if sc.cloud is None else tuple(A(c) for c in sc.cloud),
                lims=None if sc.band_lims is None else A(sc.band_lims))


def _u64(be, t):
    return be.to_numpy(t).view(np.uint64)


def k_null(be, sc, d, g):
    return be.rt_k_null(d["tau"], g, sc.nx, sc.ny, sc.dz, sc.kn_grid, sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"])


def forward(be, sc, d, g, photon0, nphotons, phase=None, kn=None, counts=None, inc_dif=None, max_events=None):
    kn = k_null(be, sc, d, g) if kn is None else kn
    return be.rt_trace_counts(d["tau"], d["ssa"], g, sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, float(sc.inc_dir[g]),
                              float(sc.inc_dif[g]) if inc_dif is None else inc_dif, sc.kn_grid, kn, sc.seed, photon0, nphotons,
                              top_at_1=sc.top_at_1, independent_column=sc.independent_column, cloud=d["cloud"], band_lims=d["lims"],
                              counts=counts, max_events=max_events, phase=phase)


def backward(be, sc, d, sensor, g, ray0, nrays, phase=None, kn=None, counts=None, max_events=None):
    kn = k_null(be, sc, d, g) if kn is None else kn
    return be.rt_bw_trace_counts(d["tau"], d["ssa"], g, sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, sc.kn_grid, kn,
                                 sensor, sc.seed, ray0, nrays, top_at_1=sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"], counts=counts,
                                 max_events=max_events, phase=phase)


def solve_fw(be, sc, d, ppp, phase=None, max_events=None):
    """rrx_raytracer_sw: the fluxes as numpy arrays, n_capped as it is"""
    r = be.raytracer_sw(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, sc.inc_dir, sc.inc_dif, sc.kn_grid,
                        ppp, sc.seed, top_at_1=sc.top_at_1, independent_column=sc.independent_column, cloud=d["cloud"], band_lims=d["lims"],
                        max_events=max_events, phase=phase)
    return {k: (be.to_numpy(v) if k != "n_capped" else v) for k, v in r.items()}


def solve_bw(be, sc, d, sensor, rpp, phase=None, max_events=None):
    return be.raytracer_bw(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, sc.inc_dir, sc.kn_grid,
                           sensor, rpp, sc.seed, top_at_1=sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"], max_events=max_events,
                           phase=phase)
