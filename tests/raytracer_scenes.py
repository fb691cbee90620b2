"""The fixed-seed scenes of the ray tracer tests (test_raytracer_ref.py on the CPU, test_gpu_raytracer.py on the GPU), as
raytracer_ref.Scene objects, and the derived statistical bound: a tally whose per-photon contribution lies in [0, 1] and has mean p
has a standard deviation of at most sqrt(p (1 - p) / N) over N photons; the tests allow 5 of these."""
import math

import numpy as np

from raytracer_ref import Scene

SEED = 0x5eed0123456789ab
INC_DIR = (800.0, 300.0)          # two g-points with different incident flux


def sigma(p, n):
    return np.sqrt(np.clip(p*(1.0 - p), 0.0, None) / n)


def _arr(a, dtype):
    return np.ascontiguousarray(np.asarray(a).astype(dtype))


def beer(dtype, kn_is_grid, top_at_1=True):
    """A: pure absorption, black surface, direct beam only, columns that differ, independent columns."""
    nx, ny, nz = 4, 4, 6
    rng = np.random.default_rng(101)
    tau = rng.uniform(0.02, 0.5, (2, nz, nx*ny))
    return Scene(nx=nx, ny=ny, nz=nz, dx=120.0, dy=90.0, dz=50.0, tau=_arr(tau, dtype), ssa=_arr(np.zeros_like(tau), dtype),
                 sfc_albedo=_arr(np.zeros(nx*ny), dtype), mu0=0.6, azimuth=0.7, inc_dir=_arr(INC_DIR, dtype), inc_dif=_arr([0., 0.], dtype),
                 kn_grid=(nx, ny, nz) if kn_is_grid else (1, 1, 1), top_at_1=top_at_1, independent_column=True, seed=SEED)


def slant(dtype):
    """B: horizontally uniform absorbing layers in 3-D mode under a slant sun whose azimuth lies along neither axis."""
    nx, ny, nz = 8, 4, 6
    rng = np.random.default_rng(102)
    tau = np.repeat(rng.uniform(0.02, 0.3, (2, nz, 1)), nx*ny, axis=2)
    return Scene(nx=nx, ny=ny, nz=nz, dx=100.0, dy=130.0, dz=80.0, tau=_arr(tau, dtype), ssa=_arr(np.zeros_like(tau), dtype),
                 sfc_albedo=_arr(np.zeros(nx*ny), dtype), mu0=0.5, azimuth=0.9, inc_dir=_arr(INC_DIR, dtype), inc_dif=_arr([0., 0.], dtype),
                 kn_grid=(4, 2, 3), top_at_1=False, independent_column=False, seed=SEED + 1)


def shadow(dtype, along, top_at_1):
    """C: one opaque absorbing block (tau = 50 per cell, three cells long in the direction of travel, two wide) in one layer of an
    otherwise empty domain; tan(theta) = dx/dz; the beam travels along +x (along = "x") or +y ("y")."""
    nx, ny, nz = (8, 4, 6) if along == "x" else (4, 8, 6)
    k_up = 3                                              # the block's layer, counted upward from the surface
    tau = np.zeros((2, nz, ny, nx))
    lay = nz - 1 - k_up if top_at_1 else k_up
    if along == "x":
        tau[:, lay, 1:3, 1:4] = 50.0
    else:
        tau[:, lay, 1:4, 1:3] = 50.0
    tau = tau.reshape(2, nz, nx*ny)
    return Scene(nx=nx, ny=ny, nz=nz, dx=100.0, dy=100.0, dz=100.0, tau=_arr(tau, dtype), ssa=_arr(np.zeros_like(tau), dtype),
                 sfc_albedo=_arr(np.zeros(nx*ny), dtype), mu0=math.cos(math.atan(1.0)), azimuth=0.0 if along == "x" else math.pi/2,
                 inc_dir=_arr(INC_DIR, dtype), inc_dif=_arr([0., 0.], dtype), kn_grid=(nx, ny, nz), top_at_1=top_at_1,
                 independent_column=False, seed=SEED + 2)


def _cloud(rng, nbnd, nz, ncol, share, ssa_range, dtype):
    cloudy = rng.uniform(0., 1., (nbnd, nz, ncol)) < share
    cloudy[:] = cloudy[0]
    ct = np.where(cloudy, rng.uniform(1.0, 6.0, (nbnd, nz, ncol)), 0.0)
    cw = rng.uniform(*ssa_range, (nbnd, nz, ncol))
    cg = rng.uniform(0.80, 0.87, (nbnd, nz, ncol))
    return _arr(ct, dtype), _arr(cw, dtype), _arr(cg, dtype)


def conservative(dtype):
    """D: gas ssa = 1, cloud ssa = 1 and g = 0.85, a checkerboard albedo of 0 and 1: every weight stays 0 or 1."""
    nx, ny, nz = 4, 4, 6
    rng = np.random.default_rng(104)
    tau = rng.uniform(0.05, 0.3, (2, nz, nx*ny))
    ct, _, _ = _cloud(rng, 2, nz, nx*ny, 0.3, (1.0, 1.0), dtype)
    cloud = (ct, _arr(np.ones_like(ct), dtype), _arr(np.full_like(ct, 0.85), dtype))
    ix, iy = np.arange(nx*ny) % nx, np.arange(nx*ny) // nx
    return Scene(nx=nx, ny=ny, nz=nz, dx=150.0, dy=150.0, dz=100.0, tau=_arr(tau, dtype), ssa=_arr(np.ones_like(tau), dtype),
                 sfc_albedo=_arr((ix + iy) % 2, dtype), mu0=0.7, azimuth=2.2, inc_dir=_arr(INC_DIR, dtype), inc_dif=_arr([200., 0.], dtype),
                 kn_grid=(2, 2, 2), cloud=cloud, band_lims=np.array([[1, 1], [2, 2]], dtype=np.int32), top_at_1=False,
                 independent_column=False, seed=SEED + 3)


def general(dtype):
    """E: ssa 0.3 - 0.999, cloud in a third of the cells, albedo 0.3 (the roulette runs), a diffuse incident share of 0.2, a coarse
    k_null grid, 3-D mode."""
    nx, ny, nz = 8, 4, 6
    rng = np.random.default_rng(105)
    tau = rng.uniform(0.02, 0.4, (2, nz, nx*ny))
    ssa = rng.uniform(0.3, 0.999, (2, nz, nx*ny))
    cloud = _cloud(rng, 2, nz, nx*ny, 1./3., (0.9, 0.999), dtype)
    inc = np.array(INC_DIR)
    return Scene(nx=nx, ny=ny, nz=nz, dx=100.0, dy=140.0, dz=60.0, tau=_arr(tau, dtype), ssa=_arr(ssa, dtype),
                 sfc_albedo=_arr(np.full(nx*ny, 0.3), dtype), mu0=0.8, azimuth=4.0, inc_dir=_arr(0.8*inc, dtype), inc_dif=_arr(0.2*inc, dtype),
                 kn_grid=(2, 2, 3), cloud=cloud, band_lims=np.array([[1, 1], [2, 2]], dtype=np.int32), top_at_1=True,
                 independent_column=False, seed=SEED + 4)


def beer_expected(scene):
    """exp(-sum tau / mu0) per g-point and pixel, (ngpt, ncol), in float64"""
    return np.exp(-scene.tau.astype(np.float64).sum(axis=1) / float(scene.mu0))
