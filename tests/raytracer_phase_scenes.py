"""The fixed tables, radii and inputs of the phase-table tests (test_raytracer_phase_ref.py on the CPU, test_gpu_raytracer_phase.py
on the GPU), on the scenes of raytracer_scenes.py: raw tables (nbnd = 2, nre, nmu) in float64 with their radius grids, the cell
radii of the `general` scene, and the uniforms / radii that the array entries are probed with."""
import numpy as np

import raytracer_phase_ref as P
import raytracer_scenes as S

NBND = 2
RE0, DRE = 4.0, 3.0          # the radius grid of every test table with nre > 1: 4, 7, 10


def isotropic(nodes, nre):
    """P = 1 on nodes {-1, 1} (nodes = 2) or {-1, -1/2, 0, 1/2, 1} (nodes = 5), raw value 3 (the builder normalises)"""
    mu = np.array([-1., 1.]) if nodes == 2 else np.array([-1., -0.5, 0., 0.5, 1.])
    return mu, np.full((NBND, nre, mu.size), 3.0)


def double_hg33():
    """33 non-uniform nodes, 3 radii, 2 bands: a forward peak that sharpens with the radius and a backward lobe"""
    mu = P.nodes(33, 2.5)
    raw = np.empty((NBND, 3, 33))
    for b in range(NBND):
        for i, (g1, g2, share) in enumerate(((0.70, -0.30, 0.90), (0.80, -0.40, 0.93), (0.88, -0.50, 0.96))):
            raw[b, i] = (1.0 + 0.5*b) * P.double_hg(mu, g1 - 0.02*b, g2, share)
    return mu, raw


def double_hg33_two_radii():
    mu, raw = double_hg33()
    return mu, np.ascontiguousarray(raw[:, ::2])


def hg1800(g=0.85, nre=3, spread=0.0):
    """1 800 nodes dense towards +1 (the last spacing, 2/1799^2 = 6.2e-7, is ten fp32 steps: the nodes stay distinct in fp32); HG(g + spread (ire - (nre-1)/2)) per radius, each radius with a normalisation of its own"""
    mu = P.nodes(1800, 2.0)
    raw = np.empty((NBND, nre, 1800))
    for i in range(nre):
        raw[:, i] = (0.5 + i) * P.hg(mu, g + spread*(i - 0.5*(nre - 1)))
    return mu, raw


def cell_radii(scene, dtype, seed=7):
    """(nz, ncol): across the grid 4 .. 10, below and above it, on its nodes"""
    rng = np.random.default_rng(seed)
    re = rng.uniform(2.0, 13.0, (scene.nz, scene.ncol))
    re[0, :4] = (4.0, 7.0, 10.0, 1.0)
    return np.ascontiguousarray(re.astype(dtype))


def cell_radii_with_nan(scene, dtype):
    re = cell_radii(scene, dtype)
    re[1, ::5] = np.nan
    return re


def general_g(dtype, g):
    """the general scene with cld_g = g in every cell"""
    sc = S.general(dtype)
    sc.cloud = (sc.cloud[0], sc.cloud[1], np.full_like(sc.cloud[2], g))
    return sc


def probe_u(table, ibnd, dtype):
    """the 24-bit uniform's smallest and largest values, every node's CDF value on each radius (and its neighbours in dtype), a
    regular ladder"""
    F = np.dtype(dtype).type
    tiny, big = F((0 + 0.5) * 2.0**-23), F(((1 << 23) - 1 + 0.5) * 2.0**-23)
    c = table.cdf[ibnd].reshape(-1).astype(dtype)
    c = c[(c > 0) & (c < 1)]
    u = np.concatenate([[tiny, big], c, np.nextafter(c, F(0.)), np.nextafter(c, F(1.)), np.linspace(0.001, 0.999, 499).astype(dtype)])
    return np.clip(u, tiny, big).astype(dtype)


def probe_re(dtype):
    """the grid's ends and nodes, outside it, inside it, NaN"""
    return np.array([4.0, 7.0, 10.0, 1.0, 25.0, 4.75, 8.5, 9.999, np.nan], dtype=dtype)


def probe_pairs(table, ibnd, dtype):
    """(u, re) sorted by u within each radius: every u with every radius"""
    u = np.sort(probe_u(table, ibnd, dtype))
    re = probe_re(dtype)
    return np.tile(u, re.size), np.repeat(re, u.size)
