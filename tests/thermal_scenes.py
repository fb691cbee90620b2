"""The fixed-seed scenes of the thermal ray tracer's tests (test_raytracer_thermal_ref.py on the CPU, test_gpu_raytracer_thermal.py on
the GPU) as raytracer_thermal_ref.ThermalScene objects, at the size of raytracer_scenes.general: 8 x 4 x 6 cells, 2 g-points, 2 bands,
a k_null grid coarser than the grid so that null collisions occur. gas_scatters False: the device is given a NULL ssa (the scene
holds zeros, which restate it bit for bit). Also what the tests derive from a scene without tracing: the Schwarzschild expectation
of clear_columns under a nadir view, and the standard error of disjoint ray ranges."""
import math

import numpy as np

import raytracer_ref as R
import raytracer_scenes as FS
from raytracer_thermal_ref import ThermalScene
from rte_rrtmgp_cpp_amd import camera as C

SEED = 0x7e41a15eed012345
S_G = (12.0, 3.5)          # the cavity's radiance per g-point, W m-2 sr-1
RANGES = 16                # disjoint ray ranges of the statistical tests
BAND_LIMS = np.array([[1, 1], [2, 2]], dtype=np.int32)


def _arr(a, dtype):
    return np.ascontiguousarray(np.asarray(a).astype(dtype))


def _scene(dtype, tau, ssa, cloud, top_at_1, seed, lay_src, sfc_src, sfc_emis, top_radiance, gas_scatters):
    nx, ny, nz = 8, 4, 6
    medium = R.Scene(nx=nx, ny=ny, nz=nz, dx=100.0, dy=140.0, dz=60.0, tau=_arr(tau, dtype), ssa=_arr(ssa, dtype),
                     sfc_albedo=_arr(np.zeros(nx*ny), dtype), mu0=1.0, azimuth=0.0, inc_dir=_arr([0., 0.], dtype), inc_dif=_arr([0., 0.], dtype),
                     kn_grid=(2, 2, 3), cloud=cloud, band_lims=BAND_LIMS if cloud is not None else None, top_at_1=top_at_1, seed=seed)
    sc = ThermalScene(medium, _arr(lay_src, dtype), _arr(sfc_src, dtype), _arr(sfc_emis, dtype), _arr(top_radiance, dtype))
    sc.gas_scatters = gas_scatters
    return sc


def clear_columns(dtype):
    """No cloud and a gas that does not scatter (NULL ssa): tau differs per column and layer, lay_src per layer and g-point, the
    surface source per g-point; sfc_emis 0.9 everywhere; nothing comes down through the top. top_at_1 False."""
    nx, ny, nz = 8, 4, 6
    rng = np.random.default_rng(231)
    tau = rng.uniform(0.05, 0.5, (2, nz, nx*ny))
    lay = np.repeat(rng.uniform(2.0, 9.0, (2, nz, 1)), nx*ny, axis=2)
    sfc = np.repeat(np.array([[14.0], [6.0]]), nx*ny, axis=1)
    return _scene(dtype, tau, np.zeros_like(tau), None, False, SEED, lay, sfc, np.full(nx*ny, 0.9), [0., 0.], False)


def cavity(dtype):
    """raytracer_scenes.general's gas (ssa 0.3 - 0.999, so Rayleigh scattering runs) and cloud (ssa up to 0.999), sfc_emis spread over
    [0.3, 1], and every source and top_radiance[g] equal to S_G[g]: a black-body cavity, whose radiance is S_G[g] in every direction
    from every point. top_at_1 True."""
    g = FS.general(dtype)
    ncol = g.ncol
    emis = np.linspace(0.3, 1.0, ncol)[np.random.default_rng(232).permutation(ncol)]
    S = np.asarray(S_G)
    return _scene(dtype, g.tau, g.ssa, g.cloud, True, SEED + 1, np.broadcast_to(S[:, None, None], g.tau.shape),
                  np.broadcast_to(S[:, None], (2, ncol)), emis, S, True)


def cavity_black(dtype):
    """The cavity's sources with sfc_emis = 1 and no cloud: what the 1-D LW solver is given column by column (T3)."""
    sc = cavity(dtype)
    return _scene(dtype, sc.tau, np.zeros_like(sc.tau), None, True, SEED + 1, sc.lay_src, sc.sfc_src, np.ones(sc.ncol), sc.top_radiance, False)


def general_lw(dtype):
    """Cloud in a third of the cells, a gas with a little scattering (ssa below 0.3), and sources that vary in all three directions:
    lay_src per cell, sfc_src and sfc_emis per pixel, a top radiance per g-point. top_at_1 False."""
    g = FS.general(dtype)
    nz, ncol = g.nz, g.ncol
    rng = np.random.default_rng(233)
    ssa = rng.uniform(0.0, 0.3, (2, nz, ncol))
    lay = rng.uniform(1.0, 10.0, (2, nz, ncol))
    sfc = rng.uniform(8.0, 16.0, (2, ncol))
    emis = rng.uniform(0.5, 1.0, ncol)
    return _scene(dtype, g.tau, ssa, g.cloud, False, SEED + 2, lay, sfc, emis, [1.5, 0.25], True)


# ---- sensors: 6 x 4 pixels for the comparisons ray for ray, 3 x 2 for the statistical ones (the domain is 800 x 560 x 360 m)
def sensors(npx, npy):
    return {"perspective": C.perspective(npx, npy, (330., 250., 170.), yaw=0.6, pitch=-0.5, roll=0.2, fov=math.radians(70.)),
            "fisheye": C.fisheye(npx, npy, (420., 130., 0.)),
            "orthographic": C.orthographic(npx, npy, yaw=2.0, pitch=-1.0)}


def cavity_sensors():
    """a perspective camera inside the domain, a fisheye at the surface, a slant orthographic view and both flux sensors"""
    return {**sensors(3, 2), "flux_up": C.flux_sensor(3, 2, up=True), "flux_down": C.flux_sensor(3, 2, up=False)}


CAVITY_RAYS = 8192         # rays per pixel and g-point in T2 / T3: test_raytracer_thermal_ref.py holds the restatement's standard error
                           # of RANGES ranges of them below 1 % of S_G for every sensor
T1_RAYS = 4096             # rays per pixel and g-point in T1


def standard_error(parts, rays_per_range):
    """(mean radiance, its standard error) per pixel from the counts of disjoint ray ranges, (ranges, npix)"""
    r = parts.astype(np.float64) * 2.0**-32 / rays_per_range
    return r.mean(axis=0), r.std(axis=0, ddof=1) / math.sqrt(r.shape[0])


# ---- T1: the Schwarzschild expectation of clear_columns under the nadir orthographic camera with one pixel per column
def _march_up(sc, g, x0, y0, ux, uy, uz):
    """The Schwarzschild integral in float64, exact cell by cell, along the paths from the surface points (x0, y0, 0) upward in the
    directions (ux, uy, uz > 0) through the periodic grid to the domain top: sum over the cells crossed of
    B_cell (1 - exp(-dtau)) exp(-tau before) (nothing comes in at the top of clear_columns). No scattering."""
    s = sc.medium
    nx, ny, nz = s.nx, s.ny, s.nz
    k_ext = (s.tau[g].astype(np.float64) / s.dz).reshape(nz, ny, nx)
    B = sc.lay_src[g].astype(np.float64).reshape(nz, ny, nx)
    if s.top_at_1:
        k_ext, B = k_ext[::-1], B[::-1]
    n = x0.size
    i = np.clip(np.floor(x0/s.dx).astype(np.int64), 0, nx-1); j = np.clip(np.floor(y0/s.dy).astype(np.int64), 0, ny-1)
    k = np.zeros(n, dtype=np.int64)
    with np.errstate(divide="ignore"):
        tx = np.where(ux > 0, ((i+1)*s.dx - x0)/ux, np.where(ux < 0, (i*s.dx - x0)/ux, np.inf))
        ty = np.where(uy > 0, ((j+1)*s.dy - y0)/uy, np.where(uy < 0, (j*s.dy - y0)/uy, np.inf))
        dtx, dty = np.where(ux != 0, s.dx/np.abs(ux), np.inf), np.where(uy != 0, s.dy/np.abs(uy), np.inf)
    tz, dtz = s.dz/uz, s.dz/uz
    t, tau, L = np.zeros(n), np.zeros(n), np.zeros(n)
    go = np.arange(n)
    while go.size:
        tn = np.minimum(tz[go], np.minimum(tx[go], ty[go]))
        dtau = k_ext[k[go], j[go], i[go]]*(tn - t[go])
        L[go] += B[k[go], j[go], i[go]]*(-np.expm1(-dtau))*np.exp(-tau[go])
        tau[go] += dtau
        t[go] = tn
        ax = np.where((tz[go] <= tx[go]) & (tz[go] <= ty[go]), 2, np.where(tx[go] <= ty[go], 0, 1))
        m = go[ax == 0]; i[m] = (i[m] + np.where(ux[m] > 0, 1, -1)) % nx; tx[m] += dtx[m]
        m = go[ax == 1]; j[m] = (j[m] + np.where(uy[m] > 0, 1, -1)) % ny; ty[m] += dty[m]
        m = go[ax == 2]; k[m] += 1; tz[m] += dtz[m]
        go = go[(k[go] < nz) & (tau[go] < 80.0)]          # (beyond 80 optical depths nothing is left to add: exp(-80) = 2e-35)
    return L


def schwarzschild_expected(sc, g, samples=8192, batches=16):
    """(L, se) per pixel, float64, for the nadir orthographic camera with npx, npy = nx, ny:
        L = eps B_s exp(-tau_col) + sum_k B_k (1 - exp(-tau_k)) exp(-tau_above,k) + (1 - eps) exp(-tau_col) D
    with the column's own numbers in closed form. D, the reflected term, is the cosine-weighted mean over the upper hemisphere and over
    the pixel's surface points of the downwelling radiance: the same Schwarzschild formula along the Lambertian return through the
    columns that the slant path crosses (_march_up; an upward path ends at the top, so there is one reflection). That mean has no
    closed form; it is taken over `samples` fixed-seed paths per pixel, and se is its standard error from `batches` batches, times
    (1 - eps) exp(-tau_col): the reference's own error, which the test adds to its bound."""
    s = sc.medium
    nx, ny, nz, ncol = s.nx, s.ny, s.nz, s.ncol
    tau = s.tau[g].astype(np.float64)
    B = sc.lay_src[g].astype(np.float64)
    if s.top_at_1:
        tau, B = tau[::-1], B[::-1]
    above = np.concatenate([np.cumsum(tau[::-1], axis=0)[::-1][1:], np.zeros((1, ncol))])          # the layers over layer k, k upward
    tau_col = tau.sum(axis=0)
    eps = sc.sfc_emis.astype(np.float64)
    L = eps*sc.sfc_src[g].astype(np.float64)*np.exp(-tau_col) + np.sum(B*(-np.expm1(-tau))*np.exp(-above), axis=0)
    rng = np.random.default_rng(1000 + g)
    pix = np.repeat(np.arange(ncol), samples)
    x0 = (pix % nx + rng.uniform(size=pix.size))*s.dx
    y0 = (pix // nx + rng.uniform(size=pix.size))*s.dy
    mu = np.sqrt(1.0 - rng.uniform(size=pix.size))          # in (0, 1]
    phi = 2.0*math.pi*rng.uniform(size=pix.size)
    sn = np.sqrt(1.0 - mu*mu)
    D = _march_up(sc, g, x0, y0, sn*np.cos(phi), sn*np.sin(phi), mu).reshape(ncol, batches, samples//batches).mean(axis=2)
    back = (1.0 - eps)*np.exp(-tau_col)
    return L + back*D.mean(axis=1), back*D.std(axis=1, ddof=1)/math.sqrt(batches)
