"""numpy restatement of aerosol as a third scattering species of the two ray tracers (csrc/rrx_rt_common.h, the AER instantiations of
csrc/rrx_raytracer.hip and csrc/rrx_raytracer_bw.hip), in the scene's precision. Only what differs from the tracers
without aerosol is stated here:
  - the aerosol part of a cell: k_ext = ((tau + tau_c) + tau_a)/dz, k_sca = ((tau ssa + tau_c ssa_c) + tau_a ssa_a)/dz,
    k_sca_aer = (tau_a ssa_a)/dz (AerGrid, collide; collide_bg in a background layer), the k_ext that the backward tracer's walk
    to the sun sums (AerGrid.k_ext) and k_null, the block maximum of that k_ext;
  - the 7-row profile of the background (profile) and its medium (AerMedium);
  - the species draw from the one uniform u that is drawn today (collision_outcome): cloud iff u k_sca < k_sca_cld, otherwise
    aerosol iff u k_sca < k_sca_cld + k_sca_aer, otherwise gas;
  - the aerosol species, Henyey-Greenstein with min(g_a, 1 - eps) in the grid and aloft, with a phase table too, for the new
    direction and for the backward deposit (WithAerosol: the cloud species on the cloud lanes, the aerosol's on the aerosol lanes).
Everything else - the Philox streams, the draw order, the crossings, the surface, the two event loops with their optional
background, the walk - is raytracer_bg_ref's, run with these steps in place of raytracer_ref.collide, collision_outcome and Grid
and of raytracer_bg_ref.collide_bg and Medium (the steps context below). No event loop is restated.

An AerScene is a raytracer_ref.Scene with aerosol, None or (tau, ssa, g) of (nbnd, nz, ncol) each; an AerBackground a
raytracer_bg_ref.Background with aerosol, None or (tau, ssa, g) of (nbnd, nbg) each."""
import contextlib
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np

import raytracer_ref as R
import raytracer_bg_ref as BG


@dataclass
class AerScene(R.Scene):
    aerosol: Optional[tuple] = None


@dataclass
class AerBackground(BG.Background):
    aerosol: Optional[tuple] = None


def _band(scene, igpt):
    """the 0-based band of g-point igpt, -1 when it lies in none"""
    return int(R.band_of_gpt(scene.band_lims, scene.tau.shape[0])[igpt])


def _aerosol_of(obj):
    return getattr(obj, "aerosol", None)


def _hg(g, dt):
    s = object.__new__(R.HenyeyGreenstein)
    s.gc, s.g_max = g, dt.type(1.) - np.finfo(dt).eps
    return s


class WithAerosol:
    """The species of a medium with aerosol: `cloud` (Henyey-Greenstein or a table) on the lanes drawn as cloud, Henyey-Greenstein
    with g_a on the lanes drawn as aerosol (self.aerosol: a mask over the lanes of the pass, set by collision_outcome)."""
    def __init__(self, cloud, g_a, dt):
        self.cloud, self.hg, self.aerosol = cloud, _hg(g_a, dt), None

    def cos(self, cell, u):
        return np.where(self.aerosol, self.hg.cos(cell, u), self.cloud.cos(cell, u))

    def density(self, cell, cs):
        return np.where(self.aerosol, self.hg.density(cell, cs), self.cloud.density(cell, cs))


def _grid_aerosol(scene, igpt):
    """(tau_a, ssa_a, g_a) by cell of one g-point: zeros without aerosol or where the g-point lies in no band"""
    dt = scene.dtype
    aer = _aerosol_of(scene)
    ib = _band(scene, igpt) if aer is not None else -1
    if ib < 0:
        none = np.zeros(scene.nz*scene.ncol, dtype=dt)
        return none, none, none
    return tuple(np.asarray(c[ib], dtype=dt).reshape(-1) for c in aer)


def k_null(scene, igpt):
    """rrx_rt_k_null_aer: (knz, kny, knx), the maximum of ((tau + tau_c) + tau_a)/dz over each block"""
    s = scene
    F = s.dtype.type
    ib = R.band_of(s, igpt)
    tc = s.cloud[0][ib] if ib >= 0 else np.zeros_like(s.tau[igpt])
    ta = _grid_aerosol(s, igpt)[0].reshape(s.tau[igpt].shape)
    k_ext = (((s.tau[igpt] + tc) + ta) / F(s.dz)).reshape(s.nz, s.ny, s.nx)
    if s.top_at_1:
        k_ext = k_ext[::-1]
    knx, kny, knz = s.kn_grid
    return np.ascontiguousarray(k_ext.reshape(knz, s.nz//knz, kny, s.ny//kny, knx, s.nx//knx).max(axis=(1, 3, 5)))


def profile(scene, bg, igpt):
    """(7, nbg+1) of rrx_rt_bg_profile_aer: k_ext, k_sca, k_sca_cld, g, tau_above, k_sca_aer, g_aer"""
    dt = scene.dtype
    F = dt.type
    nbg = bg.nbg
    zeros = np.zeros(nbg, dtype=dt)
    ib = _band(scene, igpt) if bg.cloud is not None else -1
    ia = _band(scene, igpt) if _aerosol_of(bg) is not None else -1
    t, w0, dz = bg.tau[igpt].astype(dt), bg.ssa[igpt].astype(dt), np.asarray(bg.dz, dtype=dt)
    tc, wc, gc = (c[ib].astype(dt) for c in bg.cloud) if ib >= 0 else (zeros, zeros, zeros)
    ta, wa, ga = (c[ia].astype(dt) for c in bg.aerosol) if ia >= 0 else (zeros, zeros, zeros)
    g_max = F(1.) - np.finfo(dt).eps
    out = np.zeros((7, nbg + 1), dtype=dt)
    out[0, :nbg] = ((t + tc) + ta) / dz
    out[1, :nbg] = ((t*w0 + tc*wc) + ta*wa) / dz
    out[2, :nbg] = (tc*wc) / dz
    out[3, :nbg] = np.minimum(gc, g_max)
    layer = (t + tc) + ta
    for b in range(nbg + 1):
        above = F(0.)
        for l in range(0 if b == nbg else b + 1, nbg):
            above = above + layer[l]
        out[4, b] = above
    out[5, :nbg] = (ta*wa) / dz
    out[6, :nbg] = np.minimum(ga, g_max)
    return out


class AerGrid(R.Grid):
    """raytracer_ref.Grid with the scene's aerosol: its arrays by cell, the k_ext and k_null with tau_a, and the two species"""
    def __init__(self, scene, igpt, table=None, independent_column=False):
        super().__init__(scene, igpt, table, independent_column)
        self.aer_tau, self.aer_ssa, aer_g = _grid_aerosol(scene, igpt)
        self.species = WithAerosol(self.species, aer_g, scene.dtype)
        self.k_null = k_null(scene, igpt)

    def k_ext(self, cell):
        return ((self.tau[cell] + self.cld_tau[cell]) + self.aer_tau[cell]) / self.dz


class AerMedium(BG.Medium):
    """raytracer_bg_ref.Medium with the rows of the 7-row profile and the two species of the layers"""
    def __init__(self, G, bg, igpt):
        super().__init__(G, bg, igpt)
        if self.nbg:
            dt = G.scene.dtype
            self.k_ext, self.k_sca, self.k_sca_cld, g, self.tau_above, self.k_sca_aer, g_aer = profile(G.scene, bg, igpt)
            self.species = WithAerosol(_hg(g, dt), g_aer, dt)


def collide(G, p, h):
    """raytracer_ref.collide with the aerosol part of the cell; the species travels with the cell for collision_outcome"""
    F = p.x.dtype.type
    one, zero = F(1.), F(0.)
    x_lo, x_hi, y_lo, y_hi, z_lo, z_hi = p.faces
    dn_ = p.tau / p.kn_val
    if not G.independent_column:
        p.x = np.where(h, np.clip(p.x + p.ux*dn_, x_lo, x_hi), p.x)
        p.y = np.where(h, np.clip(p.y + p.uy*dn_, y_lo, y_hi), p.y)
    p.z = np.where(h, np.clip(p.z + p.uz*dn_, z_lo, z_hi), p.z)
    i, j, k = R.fine_cell(p.x, G.dx, p.i_n, G.rx), R.fine_cell(p.y, G.dy, p.j_n, G.ry), R.fine_cell(p.z, G.dz, p.k_n, G.rz)
    cell = G.cell(i, j, k)
    t, w0, tc, wc, ta, wa = G.tau[cell], G.ssa[cell], G.cld_tau[cell], G.cld_ssa[cell], G.aer_tau[cell], G.aer_ssa[cell]
    k_ext = G.k_ext(cell)
    k_sca = ((t*w0 + tc*wc) + ta*wa) / G.dz
    k_sca_cld = (tc*wc) / G.dz
    k_sca_aer = (ta*wa) / G.dz
    f_no_abs = np.clip(one - (k_ext - k_sca)/p.kn_val, zero, one)
    return SimpleNamespace(i=i, j=j, k=k, cell=cell, k_ext=k_ext, k_sca=k_sca, k_sca_cld=k_sca_cld, k_sca_aer=k_sca_aer,
                           f_no_abs=f_no_abs, species=G.species)


def collide_bg(M, q, h, frozen):
    """raytracer_bg_ref.collide_bg (the layer's k_ext and k_sca hold the aerosol's share already) with the layer's k_sca_aer"""
    c = _steps_of_bg["collide_bg"](M, q, h, frozen)
    c.k_sca_aer, c.species = M.k_sca_aer[c.cell], M.species
    return c


def collision_outcome(pt, a, p, h, c):
    """raytracer_ref.collision_outcome with the three-way species draw from the same uniform. Returns the masks of the lanes that
    scatter and that scatter by a particle (cloud or aerosol: the lanes that take the species' cosine and density, not Rayleigh's);
    which of the two it is goes to the species."""
    dt = pt.dtype
    zero = dt.type(0.)
    p.w = np.where(h, p.w*c.f_no_abs, p.w)
    R.roulette(pt, a, p.w, h)
    live = h & (p.w > zero)
    p.alive[h & ~live] = False
    u = np.zeros(a.size, dtype=dt); u[live] = pt.draw(a[live])
    sc = live & (u*(c.k_sca + (p.kn_val - c.k_ext)) < c.k_sca)
    u = np.zeros(a.size, dtype=dt); u[sc] = pt.draw(a[sc])
    cloud = sc & (u*c.k_sca < c.k_sca_cld)
    aerosol = sc & ~cloud & (u*c.k_sca < c.k_sca_cld + c.k_sca_aer)
    pt.cloud_scatterings += int(cloud.sum())
    pt.aerosol_scatterings = getattr(pt, "aerosol_scatterings", 0) + int(aerosol.sum())
    c.species.aerosol = aerosol
    return sc, cloud | aerosol


_steps_of_ref = {k: getattr(R, k) for k in ("Grid", "collide", "collision_outcome")}
_steps_of_bg = {k: getattr(BG, k) for k in ("Medium", "collide_bg")}


@contextlib.contextmanager
def steps():
    """the event loops of raytracer_bg_ref run with the steps of this file"""
    mine = globals()
    try:
        R.Grid, R.collide, R.collision_outcome = AerGrid, mine["collide"], mine["collision_outcome"]
        BG.Medium, BG.collide_bg = AerMedium, mine["collide_bg"]
        yield
    finally:
        for k, v in _steps_of_ref.items():
            setattr(R, k, v)
        for k, v in _steps_of_bg.items():
            setattr(BG, k, v)


def trace_counts(scene, bg, igpt, photon0, nphotons, max_events=1 << 20, table=None):
    """rrx_rt_trace_counts_aer: what raytracer_bg_ref.trace_counts returns"""
    with steps():
        return BG.trace_counts(scene, bg, igpt, photon0, nphotons, max_events, table)


def raytracer_sw(scene, bg, photons_per_pixel, max_events=1 << 20):
    """rrx_raytracer_sw_aer (without a table): what raytracer_bg_ref.raytracer_sw returns"""
    with steps():
        return BG.raytracer_sw(scene, bg, photons_per_pixel, max_events)


def trace_counts_bw(scene, bg, sensor, igpt, ray0, nrays, max_events=1 << 20, ranges=1, table=None):
    """rrx_rt_bw_trace_counts_aer: what raytracer_bg_ref.trace_counts_bw returns"""
    with steps():
        return BG.trace_counts_bw(scene, bg, sensor, igpt, ray0, nrays, max_events, ranges, table)


def raytracer_bw(scene, bg, sensor, rays_per_pixel, max_events=1 << 20):
    """rrx_raytracer_bw_aer (without a table): what raytracer_bg_ref.raytracer_bw returns"""
    with steps():
        return BG.raytracer_bw(scene, bg, sensor, rays_per_pixel, max_events)
