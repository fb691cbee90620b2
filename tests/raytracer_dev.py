"""What the GPU tests of the ray tracers (test_gpu_raytracer*.py) share: a raytracer_ref.Scene and Background on the device, and
one call per trace, solve and camera method of a backend, made with a scene's numbers. phase: a phase_tables table with the cells'
radius, or None for Henyey-Greenstein.

Which C entry a call reaches is the caller's choice, and several tests are about it:
  - forward, backward, solve_fw, solve_bw: rrx_rt_trace_counts, rrx_rt_bw_trace_counts, rrx_raytracer_sw, rrx_raytracer_bw (their
    _phase forms with a table). No background, no aerosol; k_null is rrx_rt_k_null's.
  - the _bg helpers with aer=False: the rrx_*_bg entries. The scene's aerosol is not passed, the background goes without its own
    (NoAerosol), k_null is rrx_rt_k_null's and the profile has 5 rows.
  - the _bg helpers with aer=True, and the spectral helpers: the rrx_*_aer entries and the spectral ones, which are built on them.
    They get the scene's aerosol triple, NO_TRIPLE (three NULL pointers) when the scene has none, and the background's own;
    k_null is rrx_rt_k_null_aer's and the profile has 7 rows.
dbg None is nbg = 0 in every one of them."""
import numpy as np

from rte_rrtmgp_cpp_amd import phase_tables
import raytracer_phase_scenes as PS

NO_TRIPLE = (None, None, None)


def _be(dt, hip_f64, hip_f32):
    return hip_f64 if dt == "f64" else hip_f32


def _triple(be, t):
    return None if t is None else tuple(be.asarray(c) for c in t)


def _dev(be, sc):
    """the scene on the device; aer: its aerosol triple as the _aer entries take it"""
    A = be.asarray
    return dict(tau=A(sc.tau), ssa=A(sc.ssa), alb=A(sc.sfc_albedo), cloud=_triple(be, sc.cloud),
                lims=None if sc.band_lims is None else A(sc.band_lims), aer=NO_TRIPLE if sc.aerosol is None else _triple(be, sc.aerosol))


class DevBackground:
    def __init__(self, be, bg):
        self.dz = np.ascontiguousarray(bg.dz, dtype=be.np_dtype)
        self.tau, self.ssa = be.asarray(bg.tau), be.asarray(bg.ssa)
        self.cloud, self.aerosol = _triple(be, bg.cloud), _triple(be, bg.aerosol)


class NoAerosol:
    """a device background without its aerosol: what the _bg entries see"""
    def __init__(self, dbg):
        self.dz, self.tau, self.ssa, self.cloud, self.aerosol = dbg.dz, dbg.tau, dbg.ssa, dbg.cloud, None


def dev(be, sc, bg):
    """the scene and its background (None for none) on the device"""
    return _dev(be, sc), (None if bg is None else DevBackground(be, bg))


def _medium(d, dbg, aer):
    """background= and aerosol= of a _bg method"""
    if aer:
        return dict(background=dbg, aerosol=d["aer"])
    return dict(background=None if dbg is None else NoAerosol(dbg), aerosol=None)


def device_table(be, sc, raw=None):
    """the double Henyey-Greenstein tables of raytracer_phase_scenes (or raw: mu, phase) with a radius for every cell of the scene"""
    t = phase_tables.build(be, *(PS.double_hg33() if raw is None else raw), PS.RE0, PS.DRE)
    return t.with_radius(be.asarray(PS.cell_radii(sc, be.np_dtype)))


def _u64(be, t):
    return be.to_numpy(t).view(np.uint64)


def numbers(be, c):
    return {k: _u64(be, v) for k, v in c.items()}


def clean(be, c):
    """the counts of a backward trace that capped and clamped nothing"""
    assert int(_u64(be, c["n_capped"])[0]) == 0 and int(_u64(be, c["n_clamped"])[0]) == 0
    return _u64(be, c["counts"])


def _fluxes(be, r):
    return {k: (be.to_numpy(v) if k != "n_capped" else v) for k, v in r.items()}


def k_null(be, sc, d, g, aer=False):
    return be.rt_k_null(d["tau"], g, sc.nx, sc.ny, sc.dz, sc.kn_grid, sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"],
                        aerosol=d["aer"] if aer else None)


def k_null_all(be, sc, d):
    return be.rt_k_null_all(d["tau"], sc.nx, sc.ny, sc.dz, sc.kn_grid, sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"], aerosol=d["aer"])


# ---- the forward tracer

def forward(be, sc, d, g, photon0, nphotons, phase=None, kn=None, counts=None, inc_dif=None, max_events=None):
    kn = k_null(be, sc, d, g) if kn is None else kn
    return be.rt_trace_counts(d["tau"], d["ssa"], g, sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, float(sc.inc_dir[g]),
                              float(sc.inc_dif[g]) if inc_dif is None else inc_dif, sc.kn_grid, kn, sc.seed, photon0, nphotons,
                              top_at_1=sc.top_at_1, independent_column=sc.independent_column, cloud=d["cloud"], band_lims=d["lims"],
                              counts=counts, max_events=max_events, phase=phase)


def forward_bg(be, sc, d, dbg, g, photon0, nphotons, phase=None, counts=None, aer=False, max_events=None):
    return be.rt_trace_counts_bg(d["tau"], d["ssa"], g, sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, float(sc.inc_dir[g]),
                                 float(sc.inc_dif[g]), sc.kn_grid, k_null(be, sc, d, g, aer), sc.seed, photon0, nphotons, top_at_1=sc.top_at_1,
                                 independent_column=sc.independent_column, cloud=d["cloud"], band_lims=d["lims"], counts=counts, phase=phase,
                                 max_events=max_events, **_medium(d, dbg, aer))


def forward_spectral(be, sc, d, dbg, lists, photon0, n, phase=None, counts=None, kn=None):
    """lists: photon_end, weight0, dif_frac"""
    pe, w0, df = lists
    return be.rt_trace_counts_spectral(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, pe, w0, df,
                                       sc.kn_grid, k_null_all(be, sc, d) if kn is None else kn, sc.seed, photon0, n, top_at_1=sc.top_at_1,
                                       independent_column=sc.independent_column, cloud=d["cloud"], band_lims=d["lims"], counts=counts,
                                       phase=phase, **_medium(d, dbg, True))


def solve_fw(be, sc, d, ppp, phase=None, max_events=None):
    """rrx_raytracer_sw: the fluxes as numpy arrays, n_capped as it is"""
    return _fluxes(be, be.raytracer_sw(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, sc.inc_dir, sc.inc_dif,
                                       sc.kn_grid, ppp, sc.seed, top_at_1=sc.top_at_1, independent_column=sc.independent_column,
                                       cloud=d["cloud"], band_lims=d["lims"], max_events=max_events, phase=phase))


def solve_fw_bg(be, sc, d, dbg, ppp, phase=None, aer=False):
    return _fluxes(be, be.raytracer_sw_bg(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, sc.inc_dir,
                                          sc.inc_dif, sc.kn_grid, ppp, sc.seed, top_at_1=sc.top_at_1, independent_column=sc.independent_column,
                                          cloud=d["cloud"], band_lims=d["lims"], phase=phase, **_medium(d, dbg, aer)))


def solve_fw_spectral(be, sc, d, dbg, m, phase=None):
    """m: (ngpt,) photons per pixel"""
    return _fluxes(be, be.raytracer_sw_spectral(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, sc.inc_dir,
                                                sc.inc_dif, sc.kn_grid, m, sc.seed, top_at_1=sc.top_at_1,
                                                independent_column=sc.independent_column, cloud=d["cloud"], band_lims=d["lims"], phase=phase,
                                                **_medium(d, dbg, True)))


# ---- the backward tracer

def backward(be, sc, d, sensor, g, ray0, nrays, phase=None, kn=None, counts=None, max_events=None):
    kn = k_null(be, sc, d, g) if kn is None else kn
    return be.rt_bw_trace_counts(d["tau"], d["ssa"], g, sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, sc.kn_grid, kn,
                                 sensor, sc.seed, ray0, nrays, top_at_1=sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"], counts=counts,
                                 max_events=max_events, phase=phase)


def backward_bg(be, sc, d, dbg, sensor, g, ray0, nrays, phase=None, counts=None, aer=False, max_events=None):
    return be.rt_bw_trace_counts_bg(d["tau"], d["ssa"], g, sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, sc.kn_grid,
                                    k_null(be, sc, d, g, aer), sensor, sc.seed, ray0, nrays, top_at_1=sc.top_at_1, cloud=d["cloud"],
                                    band_lims=d["lims"], counts=counts, phase=phase, max_events=max_events, **_medium(d, dbg, aer))


def backward_spectral(be, sc, d, dbg, sensor, lists, ray0, n, phase=None, counts=None, kn=None):
    """lists: ray_end, weight0"""
    ray_end, w0 = lists
    return be.camera_trace_counts_spectral(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, ray_end, w0,
                                           sc.kn_grid, k_null_all(be, sc, d) if kn is None else kn, sensor, sc.seed, ray0, n, d["lims"],
                                           top_at_1=sc.top_at_1, cloud=d["cloud"], counts=counts, phase=phase, **_medium(d, dbg, True))


def solve_bw(be, sc, d, sensor, rpp, phase=None, max_events=None):
    return be.raytracer_bw(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, sc.inc_dir, sc.kn_grid,
                           sensor, rpp, sc.seed, top_at_1=sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"], max_events=max_events,
                           phase=phase)


def solve_bw_bg(be, sc, d, dbg, sensor, rpp, phase=None, aer=False):
    return be.raytracer_bw_bg(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, sc.inc_dir, sc.kn_grid,
                              sensor, rpp, sc.seed, top_at_1=sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"], phase=phase,
                              **_medium(d, dbg, aer))


def render_spectral(be, sc, d, dbg, sensor, m, M, phase=None):
    """m: (ngpt,) rays per pixel; M: the channel matrix. radiance comes back as a numpy array (nchan, npix)"""
    r = be.camera_render_spectral(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, sc.inc_dir, sc.kn_grid,
                                  sensor, m, sc.seed, d["lims"], M, top_at_1=sc.top_at_1, cloud=d["cloud"], phase=phase,
                                  **_medium(d, dbg, True))
    rad = be.to_numpy(r["radiance"])
    r["radiance"] = rad.reshape(rad.shape[0], -1)
    return r
