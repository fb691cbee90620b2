"""The fixed-seed scenes and sensors of the tests of the thermal tracer with the rays of all g-points in one launch
(test_raytracer_thermal_spectral_ref.py and test_thermal_spectral_abi.py on the CPU, test_gpu_raytracer_thermal_spectral.py on the
GPU) as raytracer_thermal_ref.ThermalScene objects, on the medium of raytracer_spectral_scenes.plain: 4 x 4 x 6 cells,
5 g-points in 2 bands (g-points 1-3 and 4-5), a coarse k_null grid, cloud. The sources vary per cell and span a factor of 80 between
the g-points; g-point 2 (0-based) emits nothing, so that it gets no rays and its range of the ray list is empty. The sensors have
6 x 4 pixels. The statistical bound is derived in schwarzschild_sigma, not measured."""
import math

import numpy as np

import raytracer_scenes as S
import raytracer_spectral_scenes as SS
from raytracer_ref import Scene
from raytracer_thermal_ref import ThermalScene
from rte_rrtmgp_cpp_amd import camera as C

NGPT, NBND, LIMS, EMPTY = SS.NGPT, SS.NBND, SS.LIMS, SS.EMPTY
ACTIVE = (0, 1, 3, 4)
BANDS = ((0, 1, 2), (3, 4))          # the g-points of the two bands
NPX, NPY = 6, 4
NPIX = NPX*NPY
S_G = (40.0, 0.5, 0.0, 15.0, 2.25)   # the level of every source of a g-point, W m-2 sr-1: g-point 2 is dark; 40 / 0.5 = 80
STAT_RAYS = 256                      # rays per pixel of the unbiasedness test, dealt by emission
_arr = S._arr


def _thermal(medium, lay_src, sfc_src, sfc_emis, top_radiance, gas_scatters):
    dt = medium.dtype
    sc = ThermalScene(medium, _arr(lay_src, dt), _arr(sfc_src, dt), _arr(sfc_emis, dt), _arr(top_radiance, dt))
    sc.gas_scatters = gas_scatters
    return sc


def general(dtype, top_at_1=True, cloud=True, gas_scatters=True):
    """raytracer_spectral_scenes.plain's gas (ssa 0.3 - 0.999) and cloud, sources per cell and per pixel at the levels S_G, sfc_emis per
    pixel in [0.5, 1], a top radiance of a tenth of S_G. cloud False: no cloud triple (band_lims is still given: the counts are kept
    by band). gas_scatters False: the device is given a NULL ssa, the scene holds zeros."""
    medium, _ = SS.plain(dtype, top_at_1)
    if not cloud:
        medium.cloud = None
    if not gas_scatters:
        medium.ssa = _arr(np.zeros_like(medium.tau), dtype)
    rng = np.random.default_rng(2401)
    level = np.asarray(S_G)
    lay = rng.uniform(0.5, 1.0, medium.tau.shape)*level[:, None, None]
    sfc = rng.uniform(1.0, 1.5, (NGPT, medium.ncol))*level[:, None]
    emis = rng.uniform(0.5, 1.0, medium.ncol)
    return _thermal(medium, lay, sfc, emis, 0.1*level, gas_scatters)


def emission(sc):
    """e_g: the sum over the columns of sfc_src[g] in float64, what render_lw(allocation="emission") deals the rays by"""
    return sc.sfc_src.astype(np.float64).sum(axis=1)


def sensors(sc):
    """a perspective camera inside the domain, a slant orthographic one and a flux sensor at the surface"""
    lx, ly, top = sc.nx*sc.dx, sc.ny*sc.dy, sc.nz*sc.dz
    return {"inside": C.perspective(NPX, NPY, (0.3*lx, 0.6*ly, 0.4*top), yaw=0.6, pitch=-0.5, roll=0.2, fov=math.radians(70.)),
            "slant": C.orthographic(NPX, NPY, yaw=2.0, pitch=-1.0),
            "flux": C.flux_sensor(NPX, NPY, up=True)}


# ---- the unbiasedness test: Schwarzschild's sum in a gas that only absorbs, where every ray deposits exactly once

def schwarzschild(dtype):
    """4 x 4 x 6 cells, horizontally uniform; a gas that only absorbs (NULL ssa), no cloud; k_null grid = grid; sfc_emis = 1; nothing
    comes down through the top; for the nadir orthographic sensor. In a block that is one cell k_null = k_ext, so f_no_abs is exactly
    0 at a collision: the ray deposits lay_src there and ends; one that reaches the surface deposits sfc_src and ends."""
    nx, ny, nz = 4, 4, 6
    rng = np.random.default_rng(2402)
    tau = np.repeat(rng.uniform(0.05, 0.5, (NGPT, nz, 1)), nx*ny, axis=2)
    level = np.asarray(S_G)
    lay = np.repeat(rng.uniform(0.4, 1.0, (NGPT, nz, 1)), nx*ny, axis=2)*level[:, None, None]
    sfc = np.repeat(1.3*level[:, None], nx*ny, axis=1)
    medium = Scene(nx=nx, ny=ny, nz=nz, dx=100.0, dy=130.0, dz=80.0, tau=_arr(tau, dtype), ssa=_arr(np.zeros_like(tau), dtype),
                   sfc_albedo=_arr(np.zeros(nx*ny), dtype), mu0=1.0, azimuth=0.0, inc_dir=_arr(np.zeros(NGPT), dtype),
                   inc_dif=_arr(np.zeros(NGPT), dtype), kn_grid=(nx, ny, nz), cloud=None, band_lims=LIMS, top_at_1=False,
                   independent_column=False, seed=S.SEED + 62, aerosol=None)
    return _thermal(medium, lay, sfc, np.ones(nx*ny), np.zeros(NGPT), False)


def nadir():
    return C.orthographic(NPX, NPY)


def schwarzschild_expected(sc):
    """(L, V) (ngpt,) in float64: the mean and the variance of the one deposit of a ray of g-point g. The ray comes straight down from
    the top: it collides in layer k (counted upward) with probability exp(-tau_above,k) (1 - exp(-tau_k)) and deposits B_k, or reaches
    the surface with probability exp(-tau_col) and deposits sfc_src; the probabilities add up to 1. L_g is Schwarzschild's sum,
    V_g = sum p d^2 - L_g^2."""
    tau = sc.tau.astype(np.float64)[:, :, 0]          # (top_at_1 False: layer k upward)
    B = sc.lay_src.astype(np.float64)[:, :, 0]
    above = np.concatenate([np.cumsum(tau[:, ::-1], axis=1)[:, ::-1][:, 1:], np.zeros((NGPT, 1))], axis=1)
    p = np.exp(-above)*(-np.expm1(-tau))
    p_sfc = np.exp(-tau.sum(axis=1))
    B_sfc = sc.sfc_src.astype(np.float64)[:, 0]
    assert np.allclose(p.sum(axis=1) + p_sfc, 1.0, rtol=0, atol=1e-14)
    L = (p*B).sum(axis=1) + p_sfc*B_sfc
    V = (p*B*B).sum(axis=1) + p_sfc*B_sfc*B_sfc - L*L
    return L, V


def schwarzschild_sigma(sc, m):
    """(the expected radiance of a pixel by band (nbnd,), its standard deviation (nbnd,)) in W m-2 sr-1. A pixel gets m_g rays of
    g-point g, independent, each with one deposit of mean weight0_g L_g; the band's radiance is U times the sum of the deposits of its
    g-points and U weight0_g = 1 / m_g: the mean is sum_g L_g whatever m is, and sigma^2 = sum_g V_g / m_g, over the band's g-points
    with m_g > 0 (a g-point without rays must emit nothing: L_g = 0)."""
    L, V = schwarzschild_expected(sc)
    m = np.asarray(m, dtype=np.float64)
    assert all(m[g] > 0 or L[g] == 0 for g in range(NGPT))
    mean = np.array([sum(L[g] for g in band) for band in BANDS])
    var = np.array([sum(V[g]/m[g] for g in band if m[g] > 0) for band in BANDS])
    return mean, np.sqrt(var)
