"""The fixed-seed scenes of the background-atmosphere tests (test_raytracer_bg_ref.py on the numpy restatement,
test_gpu_raytracer_bg.py on the GPU) as (raytracer_ref.Scene, raytracer_ref.Background) pairs. The basic shape is a
4 x 3 x 4 grid with a (2, 1, 2) k_null grid under 3 background layers of unequal thickness, one of them with k_ext = 0, and 2
g-points in 2 bands. The statistical bound is that of raytracer_scenes.sigma: five sigma of a per-photon contribution in [0, 1]."""
import math

import numpy as np

import raytracer_scenes as S
import raytracer_bw_ref as B
from raytracer_ref import Scene, Background, profile

NX, NY, NZ = 4, 3, 4
KN = (2, 1, 2)
DZ_BG = (300.0, 1250.0, 4100.0)          # metres, counted upward from the domain top
LIMS = np.array([[1, 1], [2, 2]], dtype=np.int32)
_arr = S._arr


def _scene(dtype, tau, ssa, albedo, seed, cloud=None, top_at_1=False, independent_column=False, inc_dif=(0., 0.), mu0=0.7, kn=KN):
    ncol = NX*NY
    return Scene(nx=NX, ny=NY, nz=NZ, dx=110.0, dy=140.0, dz=70.0, tau=_arr(tau, dtype), ssa=_arr(ssa, dtype),
                 sfc_albedo=_arr(np.broadcast_to(albedo, (ncol,)), dtype), mu0=mu0, azimuth=2.4, inc_dir=_arr(S.INC_DIR, dtype),
                 inc_dif=_arr(inc_dif, dtype), kn_grid=kn, cloud=cloud, band_lims=LIMS, top_at_1=top_at_1,
                 independent_column=independent_column, seed=seed)


def _bg(dtype, tau, ssa, cloud=None, dz=DZ_BG):
    return Background(dz=_arr(dz, dtype), tau=_arr(tau, dtype), ssa=_arr(ssa, dtype), cloud=cloud)


def general(dtype, top_at_1=True, inc_dif=(160., 60.)):
    """Cloud in a third of the grid's cells, gas ssa 0.3 - 0.999, albedo 0.3, a diffuse share; a scattering background whose
    middle layer is empty (k_ext = 0) and whose top layer carries a thin cloud in band 2."""
    rng = np.random.default_rng(1701)
    ncol = NX*NY
    tau = rng.uniform(0.02, 0.4, (2, NZ, ncol))
    ssa = rng.uniform(0.3, 0.999, (2, NZ, ncol))
    cloud = S._cloud(rng, 2, NZ, ncol, 1./3., (0.9, 0.999), dtype)
    sc = _scene(dtype, tau, ssa, 0.3, S.SEED + 21, cloud=cloud, top_at_1=top_at_1, inc_dif=inc_dif, mu0=0.8)
    sc.inc_dir = _arr(0.8*np.array(S.INC_DIR), dtype)
    bt = np.array([[0.15, 0.0, 0.08], [0.3, 0.0, 0.12]])
    bw = np.array([[0.9, 0.5, 0.97], [0.6, 0.5, 0.999]])
    bc = (_arr([[0., 0., 0.], [0., 0., 0.4]], dtype), _arr([[0.9, 0.9, 0.9], [0.9, 0.9, 0.95]], dtype),
          _arr([[0.8, 0.8, 0.8], [0.8, 0.8, 0.85]], dtype))
    return sc, _bg(dtype, bt, bw, bc)


def general_direct(dtype, top_at_1=True):
    """general without diffuse incident light and with a Rayleigh-scattering (clear) background: forward against backward"""
    sc, bg = general(dtype, top_at_1, inc_dif=(0., 0.))
    bg.cloud = None
    return sc, bg


def absorbing(dtype, independent_column=False):
    """A purely absorbing background over an empty grid and a black surface: sfc_dn_dir and tod_dn_dir per pixel are Bernoulli
    means with p = exp(-tau_bg/mu0)."""
    ncol = NX*NY
    zero = np.zeros((2, NZ, ncol))
    sc = _scene(dtype, zero, zero, 0.0, S.SEED + 22, independent_column=independent_column, mu0=0.6)
    return sc, _bg(dtype, [[0.2, 0.0, 0.35], [0.05, 0.0, 0.6]], np.zeros((2, 3)))


def absorbing_expected(sc, bg):
    """p (ngpt,) in float64"""
    return np.exp(-bg.tau.astype(np.float64).sum(axis=1) / float(sc.dtype.type(sc.mu0)))


def conservative(dtype):
    """ssa = 1 everywhere (gas and cloud, grid and background), albedo 1: no weight ever falls below 1, nothing is absorbed and
    every photon leaves through TOA."""
    rng = np.random.default_rng(1703)
    ncol = NX*NY
    tau = rng.uniform(0.05, 0.3, (2, NZ, ncol))
    ct, _, _ = S._cloud(rng, 2, NZ, ncol, 0.3, (1.0, 1.0), dtype)
    cloud = (ct, _arr(np.ones_like(ct), dtype), _arr(np.full_like(ct, 0.85), dtype))
    sc = _scene(dtype, tau, np.ones_like(tau), 1.0, S.SEED + 23, cloud=cloud, inc_dif=(200., 0.))
    bc = (_arr([[0.3, 0., 0.], [0., 0., 0.2]], dtype), _arr(np.ones((2, 3)), dtype), _arr(np.full((2, 3), 0.85), dtype))
    return sc, _bg(dtype, [[0.1, 0.0, 0.2], [0.25, 0.0, 0.05]], np.ones((2, 3)), bc)


def split(dtype):
    """A horizontally uniform scattering column over a black surface, (A) as a 6-cell grid and (B) as its lowest 4 cells plus 2
    background layers of the grid's thickness: ((scene A, None), (scene B, background B))."""
    rng = np.random.default_rng(1704)
    ncol = NX*NY
    col_tau = rng.uniform(0.1, 0.5, (2, 6, 1))
    col_ssa = rng.uniform(0.6, 0.95, (2, 6, 1))
    tau6, ssa6 = np.repeat(col_tau, ncol, axis=2), np.repeat(col_ssa, ncol, axis=2)
    a = Scene(nx=NX, ny=NY, nz=6, dx=110.0, dy=140.0, dz=70.0, tau=_arr(tau6, dtype), ssa=_arr(ssa6, dtype),
              sfc_albedo=_arr(np.zeros(ncol), dtype), mu0=0.7, azimuth=2.4, inc_dir=_arr(S.INC_DIR, dtype), inc_dif=_arr([0., 0.], dtype),
              kn_grid=(2, 1, 3), top_at_1=False, seed=S.SEED + 24)
    b = _scene(dtype, tau6[:, :4], ssa6[:, :4], 0.0, S.SEED + 25)
    b.cloud = None
    bg = _bg(dtype, col_tau[:, 4:, 0], col_ssa[:, 4:, 0], dz=(70.0, 70.0))
    return (a, None), (b, bg)


def shadow(dtype, along, top_at_1):
    """S2 of raytracer_bw_scenes under a purely absorbing background"""
    import raytracer_bw_scenes as BS
    sc = BS.shadow(dtype, along, top_at_1)
    return sc, _bg(dtype, [[0.2, 0.0, 0.35], [0.05, 0.0, 0.6]], np.zeros((2, 3)))


def cameras(sc, bg):
    """the sensors of the ray-for-ray test: a perspective camera inside the grid, one inside background layer 1, and a nadir
    orthographic camera above TOA (it starts at TOA)"""
    lx, ly, top = sc.nx*sc.dx, sc.ny*sc.dy, sc.nz*sc.dz
    inside = B.Sensor(0, 4, 3, 0.0, (0.3*lx, 0.6*ly, 0.4*top), (0.6, 0., 0.2), (0., 0.6, 0.1), (0.3, 0.2, 0.9))
    aloft = B.Sensor(0, 4, 3, 0.0, (0.7*lx, 0.2*ly, top + float(bg.dz[0]) + 0.3*float(bg.dz[1])), (0.7, 0., 0.), (0., 0.7, 0.), (0.2, -0.1, -1.0))
    nadir = B.orthographic(4, 3, (0., 0., -1.))
    nadir.position = (0., 0., 1.0e9)
    return {"inside": inside, "aloft": aloft, "nadir": nadir}


def flux_sensors(sc):
    """sensor -> the forward tally it measures: at the surface facing up, and at TOA facing down (position.z above every TOA)"""
    at_toa = B.flux_sensor(sc.nx, sc.ny, False)
    at_toa.position = (0., 0., 1.0e9)
    return {"sfc_dn_dif": B.flux_sensor(sc.nx, sc.ny, True), "toa_up": at_toa}


def two_sided(p_a, n_a, p_b, n_b):
    """|p_a - p_b| in combined sigmas"""
    return abs(p_a - p_b) / math.sqrt(S.sigma(p_a, n_a)**2 + S.sigma(p_b, n_b)**2)


# ---- the comparisons that the restatement's tests and the GPU tests share

ONE = 1 << 32
PPP_ABSORBING = 2048
PPP_SPLIT = 1024
PPP_CONSERVATIVE = 64


def check_absorbing(sc, bg, g, c, ppp, label):
    """sfc_dn_dir and tod_dn_dir per pixel and their domain means within 5 sigma of exp(-tau_bg/mu0); the worst deviation in sigmas"""
    p = float(absorbing_expected(sc, bg)[g])
    worst = 0.0
    for name in ("sfc_dn_dir", "tod_dn_dir"):
        got = c[name].astype(np.float64) / ONE / ppp
        dev = np.abs(got - p) / S.sigma(p, ppp)
        dev_mean = abs(got.mean() - p) / S.sigma(p, ppp*sc.ncol)
        worst = max(worst, float(dev.max()), float(dev_mean))
        assert np.all(dev <= 5) and dev_mean <= 5, (label, name, g, float(dev.max()), float(dev_mean))
    # every weight is 0 or 1 and nothing is lost: absorbed in the background or down through the domain top and onto the surface
    # (the slant beam crosses the empty grid: the pixel at the surface is the one at the domain top only in independent columns)
    assert int(c["sfc_dn_dir"].sum()) == int(c["tod_dn_dir"].sum())
    assert not sc.independent_column or np.array_equal(c["sfc_dn_dir"], c["tod_dn_dir"])
    assert int(c["bg_abs_dir"].sum()) + int(c["sfc_dn_dir"].sum()) == ppp*sc.ncol*ONE
    for name in ("toa_up", "tod_up", "tod_dn_dif", "sfc_dn_dif", "sfc_up", "bg_abs_dif", "abs_dir", "abs_dif"):
        assert not c[name].any(), name
    assert int(c["bg_abs_dir"][1]) == 0          # the layer with k_ext = 0 is crossed without a collision
    print(f"raytracer_bg absorbing {label} g-point {g}: p = {p:.4f}, worst deviation {worst:.2f} sigma (bound 5)")
    return worst


def check_conservative(c, nphotons, label):
    assert c["n_capped"] == 0
    assert int(c["toa_up"].sum()) == nphotons*ONE, label
    through_top = int(c["tod_dn_dir"].sum()) + int(c["tod_dn_dif"].sum()) - int(c["tod_up"].sum())
    onto_surface = int(c["sfc_dn_dir"].sum()) + int(c["sfc_dn_dif"].sum()) - int(c["sfc_up"].sum())
    assert through_top == onto_surface == 0, label
    for name in ("abs_dir", "abs_dif", "bg_abs_dir", "bg_abs_dif"):
        assert not c[name].any(), name
    assert c["tod_up"].any() and c["sfc_up"].any()


def split_means(ca, cb, ppp, ncol):
    """(name, p_a, p_b) of the domain means that the two forms of the column share: the surface fluxes and the flux out of the top"""
    n = ppp*ncol
    return [(name, float(ca[ka].sum()) / ONE / n, float(cb[kb].sum()) / ONE / n)
            for name, ka, kb in (("sfc_dn_dir", "sfc_dn_dir", "sfc_dn_dir"), ("sfc_dn_dif", "sfc_dn_dif", "sfc_dn_dif"),
                                 ("toa_up", "tod_up", "toa_up"))]


def check_split(ca, cb, ppp, ncol, g, label):
    worst = 0.0
    for name, pa, pb in split_means(ca, cb, ppp, ncol):
        dev = two_sided(pa, ppp*ncol, pb, ppp*ncol)
        worst = max(worst, dev)
        assert pa > 0 and pb > 0 and dev <= 5, (label, name, g, pa, pb, dev)
    print(f"raytracer_bg split {label} g-point {g}: worst difference {worst:.2f} combined sigma (bound 5)")
    return worst


def shadow_full_count(sc, bg, g, rays):
    F = sc.dtype.type
    prof = profile(sc, bg, g)
    t = np.exp(-(F(0.) + prof[4, bg.nbg]/F(sc.mu0)))
    d = ((F(0.5)*F(sc.mu0)) / F(B.PI)) * t
    return rays * int(np.rint(np.float64(d) * float(ONE)))
