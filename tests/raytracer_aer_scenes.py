"""The fixed-seed scenes of the aerosol tests (test_raytracer_aer_ref.py on the numpy restatement, test_gpu_raytracer_aer.py on the
GPU) as (raytracer_ref.Scene, raytracer_ref.Background) pairs with aerosol on the grid of raytracer_bg_scenes: 4 x 3 x 4
cells, a (2, 1, 2) k_null grid, 3 background layers of unequal thickness, 2 g-points in 2 bands. The statistical bound is that of
raytracer_scenes.sigma: five sigma of a per-photon contribution in [0, 1]."""
import numpy as np

import raytracer_scenes as S
import raytracer_bg_scenes as SB

NX, NY, NZ, KN, DZ_BG, LIMS = SB.NX, SB.NY, SB.NZ, SB.KN, SB.DZ_BG, SB.LIMS
_arr = S._arr
ONE = 1 << 32
PPP_BEER = 2048
# forward against backward: the restatement's own run of the general direct scene stays far below these (test_raytracer_aer_ref.py)
MAX_EVENTS = 1 << 16


def zeros(dtype, nbg=3):
    """aerosol triples of zeros for the grid and the background"""
    z = _arr(np.zeros((2, NZ, NX*NY)), dtype)
    zb = _arr(np.zeros((2, nbg)), dtype)
    return (z, z.copy(), z.copy()), (zb, zb.copy(), zb.copy())


def general(dtype, top_at_1=True, inc_dif=(160., 60.)):
    """general of raytracer_bg_scenes with a haze in about half of the grid's cells, band 2 only (band 1 has tau_a = 0), ssa_a
    0.85 - 0.99, g_a 0.6 - 0.75. Cell 0 of the lowest layer holds aerosol alone (no gas, no cloud), the cell beside it all three
    species. The lowest background layer carries aerosol in both bands."""
    sc, bg = SB.general(dtype, top_at_1, inc_dif)
    rng = np.random.default_rng(1801)
    ncol = NX*NY
    hazy = rng.uniform(0., 1., (NZ, ncol)) < 0.5
    low = NZ - 1 if top_at_1 else 0
    hazy[low, 0] = hazy[low, 1] = True
    at = np.zeros((2, NZ, ncol))
    at[1] = np.where(hazy, rng.uniform(0.2, 1.5, (NZ, ncol)), 0.0)
    aw = rng.uniform(0.85, 0.99, (2, NZ, ncol))
    ag = rng.uniform(0.6, 0.75, (2, NZ, ncol))
    tau, ssa = sc.tau.copy(), sc.ssa.copy()
    ct, cw, cg = (c.copy() for c in sc.cloud)
    tau[:, low, 0] = 0.; ct[:, low, 0] = 0.                      # aerosol alone
    tau[:, low, 1] = 0.3; ct[:, low, 1] = 2.0                    # all three species
    sc.tau, sc.ssa, sc.cloud = tau, ssa, (ct, cw, cg)
    bg_aer = (_arr([[0.25, 0., 0.], [0.4, 0., 0.]], dtype), _arr([[0.9, 0.9, 0.9], [0.95, 0.9, 0.9]], dtype),
              _arr([[0.7, 0.7, 0.7], [0.65, 0.7, 0.7]], dtype))
    sc.aerosol, bg.aerosol = (_arr(at, dtype), _arr(aw, dtype), _arr(ag, dtype)), bg_aer
    return sc, bg


def general_direct(dtype, top_at_1=True):
    """general without diffuse incident light and with a background of gas and aerosol: forward against backward"""
    sc, bg = general(dtype, top_at_1, inc_dif=(0., 0.))
    bg.cloud = None
    return sc, bg


def swap(dtype, top_at_1=True):
    """((scene A, background A), (scene B, background B)): general of raytracer_bg_scenes with its band triple T as cloud and no
    aerosol (A), and with no cloud and T as aerosol (B), in the grid and in the background."""
    a, b = SB.general(dtype, top_at_1), SB.general(dtype, top_at_1)
    b[0].aerosol, b[1].aerosol = b[0].cloud, b[1].cloud
    b[0].cloud, b[1].cloud = None, None
    return a, b


def beer(dtype, independent_column=False):
    """A purely absorbing aerosol (ssa_a = 0) in the grid and the background, over a black surface, with empty gas: sfc_dn_dir per
    pixel is a Bernoulli mean with p = exp(-sum(tau_a)/mu0). Horizontally uniform, so that the slant beam sees the same path in 3-D."""
    sc, bg = SB.absorbing(dtype, independent_column)
    rng = np.random.default_rng(1802)
    ncol = NX*NY
    at = np.repeat(rng.uniform(0.05, 0.3, (2, NZ, 1)), ncol, axis=2)
    z = np.zeros((2, NZ, ncol))
    bg.tau = _arr(np.zeros((2, 3)), dtype)
    bg_aer = (_arr([[0.2, 0.0, 0.35], [0.05, 0.0, 0.6]], dtype), _arr(np.zeros((2, 3)), dtype), _arr(np.full((2, 3), 0.7), dtype))
    sc.aerosol, bg.aerosol = (_arr(at, dtype), _arr(z, dtype), _arr(np.full_like(z, 0.7), dtype)), bg_aer
    return sc, bg


def beer_expected(sc, bg):
    """p (ngpt,) in float64: the bands are the g-points"""
    t = sc.aerosol[0].astype(np.float64)[:, :, 0].sum(axis=1) + bg.aerosol[0].astype(np.float64).sum(axis=1)
    return np.exp(-t / float(sc.dtype.type(sc.mu0)))


def check_beer(sc, bg, g, c, ppp, label):
    """sfc_dn_dir per pixel and its domain mean within 5 sigma of p; nothing is lost; the worst deviation in sigmas"""
    p = float(beer_expected(sc, bg)[g])
    got = c["sfc_dn_dir"].astype(np.float64) / ONE / ppp
    dev = np.abs(got - p) / S.sigma(p, ppp)
    dev_mean = abs(got.mean() - p) / S.sigma(p, ppp*sc.ncol)
    worst = max(float(dev.max()), float(dev_mean))
    print(f"raytracer_aer beer {label} g-point {g}: p = {p:.4f}, worst deviation {worst:.2f} sigma (bound 5)")
    assert np.all(dev <= 5) and dev_mean <= 5, (label, g, float(dev.max()), float(dev_mean))
    # what does not arrive was absorbed, by the aerosol alone, in the grid and aloft (the roulette keeps the sum only in the mean)
    assert c["abs_dir"].any() and c["bg_abs_dir"].any() and int(c["bg_abs_dir"][1]) == 0
    for name in ("toa_up", "tod_up", "tod_dn_dif", "sfc_dn_dif", "sfc_up", "bg_abs_dif", "abs_dif"):
        assert not c[name].any(), name
    return worst


def conservative(dtype):
    """conservative of raytracer_bg_scenes with a conservative aerosol (ssa_a = 1) in the grid and the background"""
    sc, bg = SB.conservative(dtype)
    rng = np.random.default_rng(1803)
    ncol = NX*NY
    at = np.where(rng.uniform(0., 1., (2, NZ, ncol)) < 0.5, rng.uniform(0.2, 1.0, (2, NZ, ncol)), 0.0)
    aer = (_arr(at, dtype), _arr(np.ones_like(at), dtype), _arr(np.full_like(at, 0.7), dtype))
    bg_aer = (_arr([[0.2, 0., 0.1], [0., 0., 0.3]], dtype), _arr(np.ones((2, 3)), dtype), _arr(np.full((2, 3), 0.7), dtype))
    sc.aerosol, bg.aerosol = aer, bg_aer
    return sc, bg


def aerosol_only(dtype):
    """A scene whose only scatterer is aerosol: absorbing gas (ssa = 0), a cloud that only absorbs (ssa_c = 0, so that a phase
    table has a cloud to belong to), a scattering aerosol in the grid and the background."""
    sc, bg = general(dtype)
    sc.ssa = _arr(np.zeros_like(sc.ssa), dtype)
    sc.cloud = (sc.cloud[0], _arr(np.zeros_like(sc.cloud[1]), dtype), sc.cloud[2])
    bg.ssa = _arr(np.zeros_like(bg.ssa), dtype)
    bg.cloud = None
    return sc, bg
