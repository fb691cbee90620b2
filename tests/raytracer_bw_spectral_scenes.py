"""The fixed-seed scenes and sensors of the tests of the backward tracer with the rays of all g-points in one launch
(test_raytracer_bw_spectral_ref.py and test_raytracer_bw_spectral_abi.py on the CPU, test_gpu_raytracer_bw_spectral.py on the GPU;
DESIGN 4.21), built on raytracer_spectral_scenes: 4 x 4 x 6 cells, 5 g-points in 2 bands (g-points 1-3 and 4-5), g-point 2 (0-based)
dark, so that its range of the ray list is empty, incident fluxes that span a factor of 80, a 3-layer background and aerosol
(general), or neither (plain). The sensors have 6 x 4 pixels. The statistical bound is derived in bernoulli_sigma, not measured."""
import math

import numpy as np

import raytracer_bw_ref as B
import raytracer_scenes as S
import raytracer_spectral_scenes as SS
from raytracer_ref import Scene

NGPT, NBND, LIMS, INC, EMPTY, ONE = SS.NGPT, SS.NBND, SS.LIMS, SS.INC, SS.EMPTY, SS.ONE
ACTIVE = (0, 1, 3, 4)
BANDS = ((0, 1, 2), (3, 4))          # the g-points of the two bands
NPX, NPY = 6, 4
ALBEDO = 0.4


def general(dtype, top_at_1=True):
    return SS.general(dtype, top_at_1)


def plain(dtype, top_at_1=True):
    return SS.plain(dtype, top_at_1)


def sensors(sc):
    """a perspective camera inside the domain, a slant and a nadir orthographic one, and a flux sensor at the surface"""
    lx, ly, top = sc.nx*sc.dx, sc.ny*sc.dy, sc.nz*sc.dz
    inside = B.Sensor(0, NPX, NPY, 0.0, (0.3*lx, 0.6*ly, 0.4*top), (0.6, 0., 0.2), (0., 0.6, 0.1), (0.3, 0.2, 0.9))
    return {"inside": inside, "slant": B.orthographic(NPX, NPY, (0.5, -0.3, -0.8)), "nadir": B.orthographic(NPX, NPY, (0., 0., -1.)),
            "flux": B.flux_sensor(NPX, NPY, True)}


def bernoulli(dtype):
    """The Bernoulli surface of raytracer_bw_scenes (S1) with the 5 g-points of this file: horizontally uniform, purely absorbing
    layers, no cloud, no aerosol, no background, k_null grid = grid (the first collision ends a ray), a uniform albedo of 0.4, for
    the nadir orthographic sensor. A ray of g-point g reaches the surface with probability p_g = exp(-tau_g) and then deposits
    exactly c_g = albedo mu0/pi exp(-tau_g/mu0); reflected, it meets no scatterer: one deposit at the most."""
    nx, ny, nz = 4, 4, 6
    rng = np.random.default_rng(2101)
    tau = np.repeat(rng.uniform(0.02, 0.3, (NGPT, nz, 1)), nx*ny, axis=2)
    arr = S._arr
    return Scene(nx=nx, ny=ny, nz=nz, dx=100.0, dy=130.0, dz=80.0, tau=arr(tau, dtype), ssa=arr(np.zeros_like(tau), dtype),
                 sfc_albedo=arr(np.full(nx*ny, ALBEDO), dtype), mu0=0.5, azimuth=0.9, inc_dir=arr(INC, dtype),
                 inc_dif=arr(np.zeros(NGPT), dtype), kn_grid=(nx, ny, nz), cloud=None, band_lims=LIMS, top_at_1=False,
                 independent_column=False, seed=S.SEED + 51, aerosol=None)


def bernoulli_expected(sc):
    """(p, c) (ngpt,) in float64"""
    tau = sc.tau.astype(np.float64).sum(axis=1)[:, 0]
    mu0 = float(sc.dtype.type(sc.mu0))
    return np.exp(-tau), ALBEDO*mu0/math.pi*np.exp(-tau/mu0)


def bernoulli_sigma(sc, m, weight0, U):
    """(the expected radiance of a pixel by band (nbnd,), its standard deviation (nbnd,)) in W m-2 sr-1. A pixel gets m_g rays of
    g-point g; each deposits weight0_g c_g with probability p_g and nothing otherwise, independently, and the band's radiance is
    U/mu0 times the sum of the deposits of its g-points: mean = U/mu0 sum_g m_g weight0_g c_g p_g, which is 1/mu0 sum_g inc_g c_g p_g
    whatever m is (m_g U weight0_g = inc_g), and sigma^2 = (U/mu0)^2 sum_g m_g (weight0_g c_g)^2 p_g (1 - p_g)."""
    p, c = bernoulli_expected(sc)
    mu0 = float(sc.dtype.type(sc.mu0))
    w = float(U)/mu0*np.asarray(weight0, dtype=np.float64)*c
    m = np.asarray(m, dtype=np.float64)
    mean = np.array([sum(m[g]*w[g]*p[g] for g in band) for band in BANDS])
    var = np.array([sum(m[g]*w[g]*w[g]*p[g]*(1.0 - p[g]) for g in band) for band in BANDS])
    return mean, np.sqrt(var)
