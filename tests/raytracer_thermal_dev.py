"""What the GPU tests of the thermal ray tracer (test_gpu_raytracer_thermal.py) share: a raytracer_thermal_ref.ThermalScene on the
device and one call per method of a backend, made with the scene's numbers. A scene whose gas does not scatter is given as a NULL
ssa."""
import numpy as np

from raytracer_dev import _be, _u64, _triple          # noqa: F401  (the tests take _be and _u64 from here)


def dev(be, sc):
    A = be.asarray
    return dict(tau=A(sc.tau), ssa=A(sc.ssa) if sc.gas_scatters else None, cloud=_triple(be, sc.cloud),
                lims=None if sc.band_lims is None else A(sc.band_lims), emis=A(sc.sfc_emis), lay_src=A(sc.lay_src), sfc_src=A(sc.sfc_src))


def k_null(be, sc, d, g):
    return be.rt_k_null(d["tau"], g, sc.nx, sc.ny, sc.dz, sc.kn_grid, sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"])


def trace(be, sc, d, sensor, g, ray0, nrays, kn=None, counts=None, max_events=None):
    """rrx_thermal_trace_counts"""
    kn = k_null(be, sc, d, g) if kn is None else kn
    return be.thermal_trace_counts(d["tau"], d["ssa"], g, sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["emis"], d["lay_src"], d["sfc_src"],
                                   float(sc.top_radiance[g]), sc.kn_grid, kn, sensor, sc.seed, ray0, nrays, top_at_1=sc.top_at_1,
                                   cloud=d["cloud"], band_lims=d["lims"], counts=counts, max_events=max_events)


def render(be, sc, d, sensor, rpp, by_band=False, max_events=None, lims="own"):
    """rrx_thermal_render"""
    return be.thermal_render(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["emis"], d["lay_src"], d["sfc_src"], sc.kn_grid, sensor,
                             rpp, sc.seed, top_at_1=sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"] if isinstance(lims, str) else lims,
                             max_events=max_events, top_radiance=np.asarray(sc.top_radiance), by_band=by_band)


def clean(be, c):
    """the counts of a trace that capped and clamped nothing"""
    assert int(_u64(be, c["n_capped"])[0]) == 0 and int(_u64(be, c["n_clamped"])[0]) == 0
    return _u64(be, c["counts"])


def ranges(be, sc, d, sensor, g, n_ranges, rays_per_range):
    """the counts of n_ranges disjoint ray ranges of rays_per_range rays per pixel each, (n_ranges, npix)"""
    kn = k_null(be, sc, d, g)
    per = rays_per_range*sensor.npix
    return np.stack([clean(be, trace(be, sc, d, sensor, g, r*per, per, kn=kn)) for r in range(n_ranges)])
