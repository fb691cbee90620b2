"""The fixed-seed scenes of the tests of the thermal tracer's cell sensors (test_raytracer_heating_ref.py and
test_thermal_heating_abi.py on the CPU, test_gpu_raytracer_heating.py on the GPU) as raytracer_thermal_ref.ThermalScene
objects. They build on thermal_spectral_scenes (4 x 4 x 6 cells, 5 g-points in 2 bands, g-point 2 (0-based) emits nothing) and, for
the energy closure, on thermal_scenes.general_lw. Also what the tests derive from a scene without tracing: the slab's truth, from
Schwarzschild's solution in extended precision."""
import math

import numpy as np

import thermal_scenes as TS
import thermal_spectral_scenes as TSS
from raytracer_ref import Scene
from raytracer_thermal_ref import ThermalScene

NGPT, NBND, LIMS, EMPTY, ACTIVE, BANDS, S_G = TSS.NGPT, TSS.NBND, TSS.LIMS, TSS.EMPTY, TSS.ACTIVE, TSS.BANDS, TSS.S_G
RANGES = TS.RANGES         # disjoint ray ranges of the statistical tests
NX, NY, NZ = 4, 4, 6
NCELL = NX*NY*NZ
SLAB_RAYS = 8192           # rays per cell, g-point and range of H1: 16 ranges of them hold the standard error of a cell below 2 % of the
                           # largest layer value (test_raytracer_heating_ref.py measures it on plain numpy before the GPU test relies on it)
CLOSURE_RAYS = 1024         # rays per cell (and per pixel of the flux sensors), g-point and range of H2
_arr = TSS._arr


def general(dtype, top_at_1=True, cloud=True, gas_scatters=True):
    """thermal_spectral_scenes.general: cloud, a scattering gas, sources per cell and pixel at the levels S_G, sfc_emis in [0.5, 1], a top
    radiance of a tenth of S_G"""
    return TSS.general(dtype, top_at_1, cloud, gas_scatters)


def cavity(dtype, top_at_1=True):
    """general's medium (cloud, gas scattering, sfc_emis < 1) with every source and top_radiance[g] equal to S_G[g]: a black-body
    cavity, in which no cell gains or loses anything"""
    sc = general(dtype, top_at_1)
    level = np.asarray(S_G)
    emis = np.minimum(np.asarray(sc.sfc_emis, dtype=np.float64), 0.95)
    out = ThermalScene(sc.medium, _arr(np.broadcast_to(level[:, None, None], sc.tau.shape), dtype),
                       _arr(np.broadcast_to(level[:, None], (NGPT, sc.ncol)), dtype), _arr(emis, dtype), _arr(level, dtype))
    out.gas_scatters = True
    return out


# ---- H1: the slab
SLAB_TAU = (3.0, 1.0, 0.3, 0.1, 0.03, 0.01)          # the layers' optical depths of g-point 0, upward from the surface


def slab(dtype):
    """4 x 4 x 6 cells, horizontally uniform; a gas that only absorbs (NULL ssa), no cloud; k_null grid = grid; sfc_emis = 1; a top
    radiance of a fifth of S_G. The layers' optical depths span 0.01 ... 3 (in another order per g-point) and the sources differ by
    layer. top_at_1 False."""
    rng = np.random.default_rng(2501)
    base = np.asarray(SLAB_TAU)
    tau = np.stack([base, base[::-1], np.roll(base, 2), np.roll(base[::-1], 1), np.roll(base, 4)])
    level = np.asarray(S_G)
    lay = rng.uniform(0.4, 1.0, (NGPT, NZ))*level[:, None]
    rep = lambda a: np.repeat(a[:, :, None], NX*NY, axis=2)
    medium = Scene(nx=NX, ny=NY, nz=NZ, dx=100.0, dy=130.0, dz=80.0, tau=_arr(rep(tau), dtype), ssa=_arr(np.zeros((NGPT, NZ, NX*NY)), dtype),
                   sfc_albedo=_arr(np.zeros(NX*NY), dtype), mu0=1.0, azimuth=0.0, inc_dir=_arr(np.zeros(NGPT), dtype),
                   inc_dif=_arr(np.zeros(NGPT), dtype), kn_grid=(NX, NY, NZ), cloud=None, band_lims=LIMS, top_at_1=False,
                   independent_column=False, seed=TSS.S.SEED + 71, aerosol=None)
    sc = ThermalScene(medium, _arr(rep(lay), dtype), _arr(np.repeat(1.3*level[:, None], NX*NY, axis=1), dtype), _arr(np.ones(NX*NY), dtype),
                      _arr(0.2*level, dtype))
    sc.gas_scatters = False
    return sc


def slab_truth(sc, nodes=256):
    """flux_conv (ngpt, nz) of the slab in W m-2, float64 from np.longdouble: the difference of the net level fluxes,
    (F_dn - F_up)(top of the layer) - (F_dn - F_up)(its bottom). The level radiances are Schwarzschild's solution per mu: upward from
    the black surface, I(l+1) = I(l) t + B_l (1 - t) with t = exp(-tau_l / mu), downward from top_radiance likewise; the fluxes are
    2 pi int_0^1 I mu dmu by Gauss-Legendre quadrature with `nodes` nodes on (0, 1)."""
    L = np.longdouble
    x, w = np.polynomial.legendre.leggauss(nodes)
    mu, w = (L(x) + 1)/2, L(w)/2
    tau = sc.tau.astype(L)[:, :, 0]          # (top_at_1 False: layer k upward)
    B = sc.lay_src.astype(L)[:, :, 0]
    ngpt, nz = tau.shape
    up = np.zeros((ngpt, nz + 1, nodes), dtype=L)
    dn = np.zeros((ngpt, nz + 1, nodes), dtype=L)
    up[:, 0] = sc.sfc_src.astype(L)[:, :1]
    dn[:, nz] = np.asarray(sc.top_radiance, dtype=L)[:, None]
    for k in range(nz):
        t = np.exp(-tau[:, k, None]/mu[None])
        up[:, k+1] = up[:, k]*t + B[:, k, None]*(1 - t)
    for k in range(nz - 1, -1, -1):
        t = np.exp(-tau[:, k, None]/mu[None])
        dn[:, k] = dn[:, k+1]*t + B[:, k, None]*(1 - t)
    net = 2*L(np.pi)*((dn - up)*(mu*w)[None, None]).sum(axis=2)
    return (net[:, 1:] - net[:, :-1]).astype(np.float64)


def by_layer(cells, sc):
    """(..., ncell) in the layout of lay_src -> (..., nz, ncol) with the layer counted upward from the surface"""
    out = np.asarray(cells).reshape(*np.shape(cells)[:-1], sc.nz, sc.ncol)
    return out[..., ::-1, :] if sc.top_at_1 else out


# ---- H2: the energy closure
def closure_scene(dtype):
    """thermal_scenes.general_lw: 8 x 4 x 6 cells, 2 g-points, cloud, a scattering gas, sources per cell, an emissivity per pixel"""
    return TS.general_lw(dtype)


def boundary_net(sc, rad_sfc, rad_top):
    """(F_dn - F_up) at the top minus (F_dn - F_up) at the surface, W m-2, the mean over the columns, (...,) from the radiances
    (..., ncol) of the two flux sensors with one pixel per column, summed over the g-points: the surface one faces up and sees
    F_dn,sfc = pi rad_sfc, the top one faces down and sees F_up,top = pi rad_top; F_up,sfc = eps pi B_s + (1 - eps) F_dn,sfc per pixel
    and F_dn,top = pi top_radiance."""
    eps = sc.sfc_emis.astype(np.float64)
    B_s = sc.sfc_src.astype(np.float64).sum(axis=0)
    dn_sfc, up_top = math.pi*np.asarray(rad_sfc, dtype=np.float64), math.pi*np.asarray(rad_top, dtype=np.float64)
    up_sfc = eps*math.pi*B_s + (1.0 - eps)*dn_sfc
    dn_top = math.pi*float(np.sum(sc.top_radiance.astype(np.float64)))
    return ((dn_top - up_top) - (dn_sfc - up_sfc)).mean(axis=-1)
