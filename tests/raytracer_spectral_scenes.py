"""The fixed-seed scenes of the tests of the forward tracer with all g-points in one launch (test_raytracer_spectral_ref.py and
test_raytracer_spectral_abi.py on the CPU, test_gpu_raytracer_spectral.py on the GPU) as (raytracer_ref.Scene,
raytracer_ref.Background or None) pairs: 5 g-points in 2 bands (g-points 1-3 and 4-5), g-point 2 (0-based) without incident
flux, so that its range of the photon list is empty, and incident fluxes that span a factor of 80. The statistical bound is derived
in beer_sigma, not measured."""
import numpy as np

import raytracer_scenes as S
from raytracer_ref import Scene, Background

NGPT, NBND = 5, 2
LIMS = np.array([[1, 3], [4, 5]], dtype=np.int32)
INC = (800.0, 10.0, 0.0, 300.0, 45.0)          # g-point 2 is dark; 800 / 10 = 80
EMPTY = 2
DZ_BG = (300.0, 1250.0, 4100.0)
ONE = 1 << 32
_arr = S._arr


def general(dtype, top_at_1=True, nx=4, ny=4, nz=6, kn=(2, 2, 3), dif_share=0.2):
    """Gas ssa 0.3 - 0.999, cloud in a third of the cells, a haze in half of them (band 2 only), albedo 0.3, a diffuse incident share
    that differs between the g-points, a coarse k_null grid, and a scattering 3-layer background with an empty middle layer, a thin
    cloud on top in band 2 and aerosol in the lowest layer."""
    rng = np.random.default_rng(1901)
    ncol = nx*ny
    tau = rng.uniform(0.02, 0.4, (NGPT, nz, ncol))
    ssa = rng.uniform(0.3, 0.999, (NGPT, nz, ncol))
    cloud = S._cloud(rng, NBND, nz, ncol, 1./3., (0.9, 0.999), dtype)
    hazy = rng.uniform(0., 1., (nz, ncol)) < 0.5
    at = np.zeros((NBND, nz, ncol))
    at[1] = np.where(hazy, rng.uniform(0.2, 1.5, (nz, ncol)), 0.0)
    aer = (_arr(at, dtype), _arr(rng.uniform(0.85, 0.99, at.shape), dtype), _arr(rng.uniform(0.6, 0.75, at.shape), dtype))
    inc = np.array(INC)
    share = dif_share*np.array([1.0, 0.5, 0.0, 1.5, 0.0])
    sc = Scene(nx=nx, ny=ny, nz=nz, dx=100.0, dy=140.0, dz=60.0, tau=_arr(tau, dtype), ssa=_arr(ssa, dtype),
               sfc_albedo=_arr(np.full(ncol, 0.3), dtype), mu0=0.8, azimuth=4.0, inc_dir=_arr(inc*(1 - share), dtype),
               inc_dif=_arr(inc*share, dtype), kn_grid=kn, cloud=cloud, band_lims=LIMS, top_at_1=top_at_1, independent_column=False,
               seed=S.SEED + 41, aerosol=aer)
    bt = rng.uniform(0.05, 0.3, (NGPT, 3)); bt[:, 1] = 0.0
    bw = rng.uniform(0.5, 0.999, (NGPT, 3))
    bc = (_arr([[0., 0., 0.], [0., 0., 0.4]], dtype), _arr([[0.9, 0.9, 0.9], [0.9, 0.9, 0.95]], dtype),
          _arr([[0.8, 0.8, 0.8], [0.8, 0.8, 0.85]], dtype))
    ba = (_arr([[0.25, 0., 0.], [0.4, 0., 0.]], dtype), _arr([[0.9, 0.9, 0.9], [0.95, 0.9, 0.9]], dtype),
          _arr([[0.7, 0.7, 0.7], [0.65, 0.7, 0.7]], dtype))
    bg = Background(dz=_arr(DZ_BG, dtype), tau=_arr(bt, dtype), ssa=_arr(bw, dtype), cloud=bc, aerosol=ba)
    return sc, bg


def wide(dtype, top_at_1=False):
    """general on 8 x 4 x 6 cells with a (4, 2, 2) k_null grid: 32 columns, so that a list of a few photons per pixel fills more
    than one workgroup"""
    return general(dtype, top_at_1, nx=8, ny=4, nz=6, kn=(4, 2, 2))


def plain(dtype, top_at_1=True):
    """The variant without a background and without aerosol (nbg = 0, NULL triples); the tests run it with a phase table."""
    sc, _ = general(dtype, top_at_1)
    sc.aerosol = None
    return sc, None


def setup(dtype, top_at_1, nx=4, ny=2, nz=4, kn=(2, 1, 2), nbg=3):
    """The scene of the set-up kernels' tests: 3 g-points in 2 bands (1-2 and 3), cloud in a third and aerosol in half of the cells,
    both in both bands, under nbg background layers with cloud and aerosol; nothing is traced. The default k_null grid has blocks of
    2 x 2 x 2 cells."""
    rng = np.random.default_rng(1903)
    ncol = nx*ny
    tau = rng.uniform(0.02, 0.4, (3, nz, ncol))
    cloud = S._cloud(rng, NBND, nz, ncol, 1./3., (0.9, 0.999), dtype)
    at = np.where(rng.uniform(0., 1., (NBND, nz, ncol)) < 0.5, rng.uniform(0.2, 1.5, (NBND, nz, ncol)), 0.0)
    aer = (_arr(at, dtype), _arr(rng.uniform(0.85, 0.99, at.shape), dtype), _arr(rng.uniform(0.6, 0.75, at.shape), dtype))
    sc = Scene(nx=nx, ny=ny, nz=nz, dx=100.0, dy=140.0, dz=60.0, tau=_arr(tau, dtype), ssa=_arr(rng.uniform(0.3, 0.999, tau.shape), dtype),
               sfc_albedo=_arr(np.full(ncol, 0.3), dtype), mu0=0.8, azimuth=4.0, inc_dir=_arr(INC[:3], dtype), inc_dif=_arr(np.zeros(3), dtype),
               kn_grid=kn, cloud=cloud, band_lims=np.array([[1, 2], [3, 3]], dtype=np.int32), top_at_1=top_at_1, seed=S.SEED + 43, aerosol=aer)
    triple = lambda lo, hi: tuple(_arr(rng.uniform(a, b, (NBND, nbg)), dtype) for a, b in ((0.05, 0.4), lo, hi))
    bg = Background(dz=_arr(DZ_BG[:nbg], dtype), tau=_arr(rng.uniform(0.05, 0.3, (3, nbg)), dtype), ssa=_arr(rng.uniform(0.5, 0.999, (3, nbg)), dtype),
                    cloud=triple((0.9, 0.999), (0.8, 0.85)), aerosol=triple((0.85, 0.99), (0.6, 0.75)))
    return sc, bg


def beer(dtype):
    """A clear scene for the unbiasedness test: purely absorbing gas in the grid and the background, no cloud, no aerosol, a black
    surface, independent columns that differ, direct light only: sfc_dn_dir of a pixel is the sum over g of Bernoulli means with
    p_g = exp(-tau_g/mu0)."""
    nx, ny, nz = 4, 4, 6
    rng = np.random.default_rng(1902)
    ncol = nx*ny
    tau = rng.uniform(0.02, 0.35, (NGPT, nz, ncol))
    sc = Scene(nx=nx, ny=ny, nz=nz, dx=120.0, dy=90.0, dz=50.0, tau=_arr(tau, dtype), ssa=_arr(np.zeros_like(tau), dtype),
               sfc_albedo=_arr(np.zeros(ncol), dtype), mu0=0.6, azimuth=0.7, inc_dir=_arr(INC, dtype), inc_dif=_arr(np.zeros(NGPT), dtype),
               kn_grid=(2, 2, 3), cloud=None, band_lims=LIMS, top_at_1=True, independent_column=True, seed=S.SEED + 42, aerosol=None)
    bt = rng.uniform(0.02, 0.3, (NGPT, 3)); bt[:, 1] = 0.0
    bg = Background(dz=_arr(DZ_BG, dtype), tau=_arr(bt, dtype), ssa=_arr(np.zeros((NGPT, 3)), dtype), cloud=None, aerosol=None)
    return sc, bg


def beer_expected(sc, bg):
    """p (ngpt, ncol) in float64: the direct transmittance of every column and g-point"""
    t = sc.tau.astype(np.float64).sum(axis=1) + bg.tau.astype(np.float64).sum(axis=1)[:, None]
    return np.exp(-t / float(sc.dtype.type(sc.mu0)))


def beer_sigma(sc, bg, m, weight0, U):
    """(the expected sfc_dn_dir (ncol,), its standard deviation (ncol,)) in W m-2. A pixel gets m_g photons of g-point g, each of
    which deposits U weight0_g with probability p_g (the weight stays 1 in a purely absorbing medium until the roulette ends the
    photon, and the roulette keeps the mean: the arrival is a Bernoulli variable of mean p_g whatever the order of absorption and
    roulette, and its deposit is either 0 or U weight0_g, so that its variance is at most (U weight0_g)^2 p_g (1 - p_g)); the photons
    are independent, so sigma^2 <= sum_g (U weight0_g)^2 m_g p_g (1 - p_g). The mean is sum_g m_g U weight0_g p_g = sum_g inc_g p_g."""
    p = beer_expected(sc, bg)
    w = float(U)*np.asarray(weight0, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    mean = ((m*w)[:, None]*p).sum(axis=0)
    var = ((m*w*w)[:, None]*p*(1.0 - p)).sum(axis=0)
    return mean, np.sqrt(var)
