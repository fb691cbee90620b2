"""numpy restatement of the Monte Carlo ray tracers (csrc/rrx_raytracer.hip, csrc/rrx_raytracer_bw.hip, csrc/rrx_rt_common.h,
DESIGN 4.14-4.21): the same Philox stream, the same draw order and the same arithmetic, operation for operation, vectorised over the
photons or rays (every pass of the loop is one event of every one still alive). Arrays are in the package's tensor convention: tau,
ssa (ngpt, nz, ncol), the cloud and aerosol triples (nbnd, nz, ncol), sfc_albedo (ncol,), ncol = nx ny with x fastest; counts are
uint64 in units of 2^-32 photon.

This file states the medium once - the grid of a g-point (Grid) and the background between the domain top and TOA (Medium), each
with its cloud and aerosol terms - and the transport steps that the two tracers share, under the device functions' names where
there is one, and then the forward tracer's event loop (trace_counts) and solve (raytracer_sw). raytracer_bw_ref.py runs its rays
through the same medium and steps. Background, phase table, aerosol and deposit weight are arguments or fields, None or 1 where
there is none: the g-point forms, the _bg and _aer forms and the spectral forms (raytracer_spectral_ref.py,
raytracer_bw_spectral_ref.py) are calls of the same loop. The contract of every step is the draw order and the association of every
expression: it draws exactly the uniforms that its docstring names, for that selection, in that sequence. Every lane has its own
Philox stream, so the order in which the grid's and the background's lanes of a pass are served does not matter.

The cloud species is Henyey-Greenstein from cld_g, or a table of raytracer_phase_ref.py (csrc/rrx_rt_phase.h) with cld_re inside
the grid; the aerosol's is Henyey-Greenstein with min(g_a, 1 - eps). A Background is counted upward from the domain top whatever
the scene's top_at_1 is: dz (nbg,), tau, ssa (ngpt, nbg), cloud and aerosol None or (tau, ssa, g) of (nbnd, nbg) each."""
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np

from mcica_ref import philox4x32_10, uniform, band_of_gpt
import raytracer_phase_ref as P

TWO_PI = 6.283185307179586
COUNT_NAMES = ("sfc_dn_dir", "sfc_dn_dif", "sfc_up", "tod_up", "abs_dir", "abs_dif")
BG_COUNT_NAMES = ("toa_up", "tod_dn_dir", "tod_dn_dif", "bg_abs_dir", "bg_abs_dif")
ALL_COUNTS = COUNT_NAMES + BG_COUNT_NAMES


@dataclass
class Scene:
    nx: int
    ny: int
    nz: int
    dx: float
    dy: float
    dz: float
    tau: np.ndarray
    ssa: np.ndarray
    sfc_albedo: np.ndarray
    mu0: float
    azimuth: float
    inc_dir: np.ndarray                       # (ngpt,)
    inc_dif: np.ndarray
    kn_grid: tuple
    cloud: Optional[tuple] = None             # (tau, ssa, g), (nbnd, nz, ncol) each
    band_lims: Optional[np.ndarray] = None    # (nbnd, 2), 1-based inclusive
    top_at_1: bool = False
    independent_column: bool = False
    seed: int = 0
    aerosol: Optional[tuple] = None           # (tau, ssa, g), (nbnd, nz, ncol) each

    @property
    def ncol(self):
        return self.nx * self.ny

    @property
    def dtype(self):
        return self.tau.dtype


@dataclass
class Background:
    dz: np.ndarray
    tau: np.ndarray
    ssa: np.ndarray
    cloud: Optional[tuple] = None
    aerosol: Optional[tuple] = None

    @property
    def nbg(self):
        return int(np.asarray(self.dz).size)


def band_of(scene, igpt, triple):
    """the 0-based band of g-point igpt for a cloud or aerosol triple: -1 without the triple or where the g-point lies in no band"""
    if triple is None:
        return -1
    return int(band_of_gpt(scene.band_lims, scene.tau.shape[0])[igpt])


def by_cell(scene, igpt, triple):
    """(tau, ssa, g) by cell of one g-point, (nz ncol,) each: zeros without the triple or where the g-point lies in no band"""
    ib = band_of(scene, igpt, triple)
    if ib < 0:
        none = np.zeros(scene.nz*scene.ncol, dtype=scene.dtype)
        return none, none, none
    return tuple(np.asarray(c[ib], dtype=scene.dtype).reshape(-1) for c in triple)


def k_null(scene, igpt):
    """rrx_rt_k_null, rrx_rt_k_null_aer: (knz, kny, knx), kn counted upward from the surface: the maximum of
    k_ext = ((tau + tau_c) + tau_a)/dz over each block."""
    F = scene.dtype.type
    tc, ta = (by_cell(scene, igpt, t)[0].reshape(scene.tau[igpt].shape) for t in (scene.cloud, scene.aerosol))
    k_ext = (((scene.tau[igpt] + tc) + ta) / F(scene.dz)).reshape(scene.nz, scene.ny, scene.nx)
    if scene.top_at_1:
        k_ext = k_ext[::-1]
    knx, kny, knz = scene.kn_grid
    return np.ascontiguousarray(k_ext.reshape(knz, scene.nz//knz, kny, scene.ny//kny, knx, scene.nx//knx).max(axis=(1, 3, 5)))


def to_count(weight):
    return np.rint(weight.astype(np.float64) * 4294967296.0).astype(np.uint64)


def sun_direction(scene):
    F = scene.dtype.type
    mu0, az = float(F(scene.mu0)), float(F(scene.azimuth))
    st = math.sqrt(max(0.0, 1.0 - mu0*mu0))
    return F(st*math.cos(az)), F(st*math.sin(az)), -F(scene.mu0)


# ---- the species of the particles: the cosine of a scattering angle from one uniform, and the density towards a direction. Both
# evaluate on all lanes of a pass (cell: the lanes' cells, or their background layers); neither draws.

class HenyeyGreenstein:
    """g by cell or by layer, taken as min(g, 1 - eps)"""
    def __init__(self, g, dt):
        self.gc, self.g_max = g, dt.type(1.) - np.finfo(dt).eps

    def cos(self, cell, u):
        F = u.dtype.type
        one, half = F(1.), F(0.5)
        g = np.minimum(self.gc[cell], self.g_max)
        iso = np.abs(g) < F(1.e-6)
        gs = np.where(iso, half, g)
        sh = (one - gs*gs) / ((one - gs) + (F(2.)*gs)*u)
        return np.where(iso, F(2.)*u - one, ((one + gs*gs) - sh*sh) / (F(2.)*gs))

    def density(self, cell, cs):
        one = cs.dtype.type(1.)
        g = np.minimum(self.gc[cell], self.g_max)
        qq = (one + g*g) - (cs.dtype.type(2.)*g)*cs
        return (one - g*g) / (qq*np.sqrt(qq))


class Tabulated:
    """table: a raytracer_phase_ref.Table with cld_re (nz, ncol); cld_g is not read"""
    def __init__(self, scene, ib, table):
        dt = scene.dtype
        self.table, self.ib = table, max(ib, 0)
        self.re = np.asarray(table.cld_re, dtype=dt).reshape(-1) if ib >= 0 else np.zeros(scene.nz*scene.ncol, dtype=dt)

    def cos(self, cell, u):
        return P.sample(self.table, self.ib, self.re[cell], u)

    def density(self, cell, cs):
        return P.evaluate(self.table, self.ib, self.re[cell], cs)


class Species:
    """The two particle species of a medium: cloud (Henyey-Greenstein or a table) and aerosol (Henyey-Greenstein). aerosol: the mask
    of the lanes whose scatterer collision_outcome drew as aerosol; the others take the cloud's."""
    def __init__(self, cloud, aerosol):
        self.cloud, self.aerosol = cloud, aerosol

    def cos(self, cell, u, aerosol):
        return np.where(aerosol, self.aerosol.cos(cell, u), self.cloud.cos(cell, u))

    def density(self, cell, cs, aerosol):
        return np.where(aerosol, self.aerosol.density(cell, cs), self.cloud.density(cell, cs))


# ---- the medium of one g-point: the grid, and the background above it

class Grid:
    """One g-point of a scene in the scene's precision: the cells and the k_null blocks, the optical properties by cell (the
    cloud's and the aerosol's are zeros where the scene has none or the g-point lies in no band) and the two species.
    independent_column: no horizontal transport."""
    def __init__(self, scene, igpt, table=None, independent_column=False):
        s = scene
        dt = s.dtype
        F = dt.type
        self.scene, self.independent_column = s, bool(independent_column)
        knx, kny, knz = s.kn_grid
        self.rx, self.ry, self.rz = s.nx//knx, s.ny//kny, s.nz//knz
        self.dx, self.dy, self.dz = F(s.dx), F(s.dy), F(s.dz)
        self.kdx, self.kdy, self.kdz = F(self.rx)*self.dx, F(self.ry)*self.dy, F(self.rz)*self.dz
        self.len_x, self.len_y, self.z_top = F(knx)*self.kdx, F(kny)*self.kdy, F(knz)*self.kdz
        self.tau, self.ssa = s.tau[igpt].reshape(-1), s.ssa[igpt].reshape(-1)
        self.cld_tau, self.cld_ssa, cld_g = by_cell(s, igpt, s.cloud)
        self.aer_tau, self.aer_ssa, aer_g = by_cell(s, igpt, s.aerosol)
        ib = band_of(s, igpt, s.cloud)
        self.species = Species(HenyeyGreenstein(cld_g, dt) if table is None else Tabulated(s, ib, table), HenyeyGreenstein(aer_g, dt))
        self.albedo = np.asarray(s.sfc_albedo, dtype=dt)
        self.k_null = k_null(s, igpt)

    def cell(self, i, j, k):
        """cell = icol + ncol*lay of the fine cell (i, j, k), k counted upward from the surface"""
        s = self.scene
        lay = s.nz - 1 - k if s.top_at_1 else k
        return i + j*s.nx + s.ncol*lay

    def k_ext(self, cell):
        """what a collision meets, and what the backward tracer's walk to the sun sums"""
        return ((self.tau[cell] + self.cld_tau[cell]) + self.aer_tau[cell]) / self.dz


def levels(scene, bg):
    """z (nbg+1,): z[0] = F(knz) (F(nz/knz) dz), z[b+1] = z[b] + dz[b] in the scene's precision"""
    dt = scene.dtype
    F = dt.type
    knz = scene.kn_grid[2]
    z = np.zeros(bg.nbg + 1, dtype=dt)
    z[0] = F(knz)*(F(scene.nz//knz)*F(scene.dz))
    for b in range(bg.nbg):
        z[b+1] = z[b] + F(bg.dz[b])
    return z


def profile(scene, bg, igpt, aerosol=True):
    """(7, nbg+1) of rrx_rt_bg_profile_aer: k_ext, k_sca, k_sca_cld, g, tau_above, k_sca_aer, g_aer. aerosol=False: the (5, nbg+1)
    of rrx_rt_bg_profile, which is not given the background's aerosol (without one, the first 5 rows of the 7)."""
    dt = scene.dtype
    F = dt.type
    nbg = bg.nbg
    zeros = np.zeros(nbg, dtype=dt)
    ib = band_of(scene, igpt, bg.cloud)
    ia = band_of(scene, igpt, bg.aerosol if aerosol else None)
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
    return out if aerosol else out[:5]


class Medium:
    """The background of one g-point above a Grid (bg None: nbg = 0, TOA is the domain top): the levels, the rows of the profile,
    and the Henyey-Greenstein species of the layers (the phase table applies inside the grid only)."""
    def __init__(self, G, bg, igpt):
        s = G.scene
        dt = s.dtype
        self.G, self.nbg, self.knz = G, (bg.nbg if bg is not None else 0), s.kn_grid[2]
        if self.nbg:
            self.z = levels(s, bg)
            self.k_ext, self.k_sca, self.k_sca_cld, g, self.tau_above, self.k_sca_aer, g_aer = profile(s, bg, igpt)
            self.species = Species(HenyeyGreenstein(g, dt), HenyeyGreenstein(g_aer, dt))
        self.z_toa = self.z[self.nbg] if self.nbg else G.z_top


class Particles:
    """The photons or rays [first, first + n) of one launch: each one's Philox stream (Stream of rrx_rt_common.h: counter
    (c0, c1, c2, nd >> 2), word nd & 3; the forward tracer's c2 is igpt, the backward one's igpt | 0x80000000), after start() their
    state, and the tallies n_capped, events (collisions + crossings), cloud_scatterings and aerosol_scatterings."""
    def __init__(self, first, n, c2, seed, dtype):
        self.index = np.uint64(first) + np.arange(int(n), dtype=np.uint64)
        self.c0, self.c1, self.c2 = self.index & np.uint64(0xFFFFFFFF), self.index >> np.uint64(32), int(c2)
        self.key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        self.nd = np.zeros(int(n), dtype=np.int64)
        self.dtype = dtype
        self.n_capped = self.events = self.cloud_scatterings = self.aerosol_scatterings = 0

    def draw(self, sel):
        """one draw for sel: the next uniform of each"""
        if sel.size == 0:
            return np.zeros(0, dtype=self.dtype)
        w = philox4x32_10((self.c0[sel], self.c1[sel], np.full(sel.size, self.c2, dtype=np.int64), self.nd[sel] >> 2), self.key)
        x = np.choose(self.nd[sel] & 3, w)
        self.nd[sel] += 1
        return uniform(x, self.dtype)

    def start(self, x, y, z, ux, uy, uz, i_n, j_n, k_n, alive, **more):
        """positions, directions and k_null blocks; weight 1, no free path pending; more: what else a tracer keeps per particle"""
        n, dt = self.nd.size, self.dtype
        self.state = dict(x=x, y=y, z=z, ux=ux, uy=uy, uz=uz, i_n=i_n, j_n=j_n, k_n=k_n, alive=alive, w=np.ones(n, dtype=dt),
                          tau=np.zeros(n, dtype=dt), pend=np.zeros(n, dtype=bool), **more)
        self.nev = np.zeros(n, dtype=np.int64)

    def passes(self, max_events):
        """No draw. Every pass is one event of every particle still alive: yields their indices a and their state p (arrays over a),
        and stores p afterwards. A particle that has had max_events events is dropped and counted in n_capped."""
        alive = self.state["alive"]
        while alive.any():
            a = np.nonzero(alive)[0]
            capped = self.nev[a] >= max_events
            self.n_capped += int(capped.sum())
            alive[a[capped]] = False
            a = a[~capped]
            if a.size == 0:
                continue
            self.nev[a] += 1
            self.events += a.size
            p = SimpleNamespace(**{k: v[a] for k, v in self.state.items()})
            yield a, p
            for k, v in self.state.items():
                v[a] = getattr(p, k)


def lambert(pt, sel, sign):
    """two draws for sel: mu^2, then phi. The cosine-weighted direction about the vertical, sign = -1 downward, +1 upward"""
    F = pt.dtype.type
    mu = np.sqrt(pt.draw(sel))
    phi = F(TWO_PI) * pt.draw(sel)
    sn = np.sqrt(F(1.) - mu*mu)
    return sn*np.cos(phi), sn*np.sin(phi), sign*mu


def fine_cell(pos, d, blk, r):
    """no draw: the fine cell of a coordinate inside block blk of r cells of width d"""
    return np.clip((pos / d).astype(np.int64), blk*r, blk*r + r - 1)


def cross(G, pt, a, p):
    """One draw for the lanes of the pass without a pending free path: tau = -log u. Then the distances to the faces of the k_null
    block and, on the lanes whose tau outlasts the block (p.crossed; the others collide inside it), the step to the nearest face
    and into the next block with the periodic wrap. Returns the masks of the lanes that left through the top (dropped here) and
    that reached the surface (z and what happens there are the caller's). A lane that no face stops is dropped and counted."""
    dt = pt.dtype
    F = dt.type
    zero, inf = F(0.), F(np.inf)
    knx, kny, knz = G.scene.kn_grid
    kdx, kdy, kdz = G.kdx, G.kdy, G.kdz
    ic = G.independent_column
    x, y, z, ux, uy, uz, tau, i_n, j_n, k_n = p.x, p.y, p.z, p.ux, p.uy, p.uz, p.tau, p.i_n, p.j_n, p.k_n
    x_lo, x_hi = i_n.astype(dt)*kdx, (i_n+1).astype(dt)*kdx
    y_lo, y_hi = j_n.astype(dt)*kdy, (j_n+1).astype(dt)*kdy
    z_lo, z_hi = k_n.astype(dt)*kdz, (k_n+1).astype(dt)*kdz

    def dist(pos, u, lo, hi):
        return np.where(u > zero, (hi - pos)/u, np.where(u < zero, (lo - pos)/u, inf)).astype(dt)
    sz = dist(z, uz, z_lo, z_hi)
    sx = np.full(a.size, inf, dtype=dt) if ic else dist(x, ux, x_lo, x_hi)
    sy = np.full(a.size, inf, dtype=dt) if ic else dist(y, uy, y_lo, y_hi)
    d_max = np.minimum(sz, np.minimum(sx, sy))
    axis = np.where((sz <= sx) & (sz <= sy), 2, np.where(sx <= sy, 0, 1))
    kn_val = G.k_null[k_n, j_n, i_n]
    fresh = ~p.pend
    tau[fresh] = -np.log(pt.draw(a[fresh]))
    pend = np.zeros(a.size, dtype=bool)
    empty = ~(kn_val > zero)
    tau_cell = np.where(empty, zero, d_max*kn_val).astype(dt)
    crossed = empty | (tau >= tau_cell)

    lost = crossed & ~(d_max < inf)
    pt.n_capped += int(lost.sum())
    p.alive[lost] = False
    c = crossed & ~lost
    tau = np.where(c, tau - tau_cell, tau)
    pend[c] = True
    if not ic:
        x = np.where(c, np.clip(x + ux*d_max, x_lo, x_hi), x)
        y = np.where(c, np.clip(y + uy*d_max, y_lo, y_hi), y)
    z = np.where(c, np.clip(z + uz*d_max, z_lo, z_hi), z)
    m = c & (axis == 0) & (ux > zero)
    i_n = np.where(m, np.where(i_n + 1 == knx, 0, i_n + 1), i_n); x = np.where(m, i_n.astype(dt)*kdx, x)
    m = c & (axis == 0) & ~(ux > zero)
    i_n = np.where(m, np.where(i_n == 0, knx - 1, i_n - 1), i_n); x = np.where(m, (i_n+1).astype(dt)*kdx, x)
    m = c & (axis == 1) & (uy > zero)
    j_n = np.where(m, np.where(j_n + 1 == kny, 0, j_n + 1), j_n); y = np.where(m, j_n.astype(dt)*kdy, y)
    m = c & (axis == 1) & ~(uy > zero)
    j_n = np.where(m, np.where(j_n == 0, kny - 1, j_n - 1), j_n); y = np.where(m, (j_n+1).astype(dt)*kdy, y)
    up, dn = c & (axis == 2) & (uz > zero), c & (axis == 2) & ~(uz > zero)
    top, sfc = up & (k_n == knz - 1), dn & (k_n == 0)
    m = up & ~top
    k_n = np.where(m, k_n + 1, k_n); z = np.where(m, k_n.astype(dt)*kdz, z)
    m = dn & ~sfc
    k_n = np.where(m, k_n - 1, k_n); z = np.where(m, (k_n+1).astype(dt)*kdz, z)
    p.alive[top] = False
    p.x, p.y, p.z, p.tau, p.pend, p.i_n, p.j_n, p.k_n = x, y, z, tau, pend, i_n, j_n, k_n
    p.crossed, p.kn_val, p.faces = crossed, kn_val, (x_lo, x_hi, y_lo, y_hi, z_lo, z_hi)
    return top, sfc


def roulette(pt, a, w, m):
    """one draw for the lanes of m whose weight is below 1/2: it becomes 1 with probability w, else 0"""
    F = pt.dtype.type
    r = m & (w < F(0.5))
    u = pt.draw(a[r])
    w[r] = np.where(u > w[r], F(0.), F(1.))


def collide(G, p, h):
    """No draw. The move of the lanes h to their collision; then, on all lanes of the pass, the fine cell there and its k_ext,
    k_sca, k_sca_cld, k_sca_aer and the share f_no_abs of the weight that a collision leaves."""
    F = p.x.dtype.type
    one, zero = F(1.), F(0.)
    x_lo, x_hi, y_lo, y_hi, z_lo, z_hi = p.faces
    dn_ = p.tau / p.kn_val
    if not G.independent_column:
        p.x = np.where(h, np.clip(p.x + p.ux*dn_, x_lo, x_hi), p.x)
        p.y = np.where(h, np.clip(p.y + p.uy*dn_, y_lo, y_hi), p.y)
    p.z = np.where(h, np.clip(p.z + p.uz*dn_, z_lo, z_hi), p.z)
    i, j, k = fine_cell(p.x, G.dx, p.i_n, G.rx), fine_cell(p.y, G.dy, p.j_n, G.ry), fine_cell(p.z, G.dz, p.k_n, G.rz)
    cell = G.cell(i, j, k)
    t, w0, tc, wc, ta, wa = G.tau[cell], G.ssa[cell], G.cld_tau[cell], G.cld_ssa[cell], G.aer_tau[cell], G.aer_ssa[cell]
    k_ext = G.k_ext(cell)
    k_sca = ((t*w0 + tc*wc) + ta*wa) / G.dz
    k_sca_cld = (tc*wc) / G.dz
    k_sca_aer = (ta*wa) / G.dz
    f_no_abs = np.clip(one - (k_ext - k_sca)/p.kn_val, zero, one)
    return SimpleNamespace(i=i, j=j, k=k, cell=cell, k_ext=k_ext, k_sca=k_sca, k_sca_cld=k_sca_cld, k_sca_aer=k_sca_aer, f_no_abs=f_no_abs)


def collision_outcome(pt, a, p, h, c):
    """w *= f_no_abs on the lanes h, then up to three draws: the roulette; for the survivors, scattering or a null collision; for
    those that scatter, one uniform u for the species: cloud iff u k_sca < k_sca_cld, otherwise aerosol iff
    u k_sca < k_sca_cld + k_sca_aer, otherwise gas. Returns the masks of the lanes that scatter, by cloud, and by aerosol."""
    dt = pt.dtype
    zero = dt.type(0.)
    p.w = np.where(h, p.w*c.f_no_abs, p.w)
    roulette(pt, a, p.w, h)
    live = h & (p.w > zero)
    p.alive[h & ~live] = False
    u = np.zeros(a.size, dtype=dt); u[live] = pt.draw(a[live])
    sc = live & (u*(c.k_sca + (p.kn_val - c.k_ext)) < c.k_sca)
    u = np.zeros(a.size, dtype=dt); u[sc] = pt.draw(a[sc])
    cloud = sc & (u*c.k_sca < c.k_sca_cld)
    aerosol = sc & ~cloud & (u*c.k_sca < c.k_sca_cld + c.k_sca_aer)
    pt.cloud_scatterings += int(cloud.sum())
    pt.aerosol_scatterings += int(aerosol.sum())
    return sc, cloud, aerosol


def rayleigh_cos(u):
    """no draw: the root of mu^3 + 3 mu = 2 q, q = 4u - 2"""
    F = u.dtype.type
    one = F(1.)
    q = F(4.)*u - F(2.)
    A = np.cbrt(q + np.sqrt(one + q*q))
    return A - one/A


def rotate_direction(pt, a, sc, cos_s, ux, uy, uz):
    """one draw for the lanes sc: phi (0 on the others). The direction at the angle acos(cos_s) from (ux, uy, uz), on the lanes sc"""
    dt = pt.dtype
    F = dt.type
    one, zero = F(1.), F(0.)
    sin_s = np.sqrt(np.maximum(zero, one - cos_s*cos_s))
    phi = np.zeros(a.size, dtype=dt); phi[sc] = F(TWO_PI) * pt.draw(a[sc])
    cp, sp = np.cos(phi), np.sin(phi)
    vert = np.abs(uz) > F(0.99999)
    den = np.sqrt(np.where(vert, one, one - uz*uz))
    vx = np.where(vert, sin_s*cp, (sin_s*((ux*uz)*cp - uy*sp))/den + ux*cos_s)
    vy = np.where(vert, sin_s*sp, (sin_s*((uy*uz)*cp + ux*sp))/den + uy*cos_s)
    vz = np.where(vert, np.where(uz > zero, cos_s, -cos_s), uz*cos_s - (sin_s*cp)*den)
    nrm = np.sqrt((vx*vx + vy*vy) + vz*vz)
    return np.where(sc, vx/nrm, ux).astype(dt), np.where(sc, vy/nrm, uy).astype(dt), np.where(sc, vz/nrm, uz).astype(dt)


def scatter_direction(pt, a, sc, cloud, aerosol, species, cell, ux, uy, uz):
    """two draws for the lanes sc: u -> the cosine of the scattering angle (the species' on the lanes cloud and aerosol, Rayleigh
    on the others; u = 1/2 on the lanes that do not scatter), then rotate_direction's"""
    dt = pt.dtype
    F = dt.type
    u = np.full(a.size, F(0.5), dtype=dt); u[sc] = pt.draw(a[sc])
    cos_s = np.clip(np.where(cloud | aerosol, species.cos(cell, u, aerosol), rayleigh_cos(u)), F(-1.), F(1.)).astype(dt)
    return rotate_direction(pt, a, sc, cos_s, ux, uy, uz)


def sun_density(species, cell, cs, cloud, aerosol):
    """no draw: the phase function towards the sun at the cosine cs, the species' on the lanes cloud and aerosol, Rayleigh's on
    the others (the backward tracer's deposit)"""
    F = cs.dtype.type
    return np.where(cloud | aerosol, species.density(cell, cs, aerosol), F(0.75)*(F(1.) + cs*cs))


# ---- the steps of a lane inside a background layer, and the passage through the domain top in both directions

def enter_grid(pos, length, kd, nblk):
    """no draw: a coordinate that comes down into the grid, wrapped, with its block, clamped into it"""
    dt = pos.dtype
    pos = (pos - np.floor(pos/length)*length).astype(dt)
    blk = np.clip((pos/kd).astype(np.int64), 0, nblk - 1)
    return np.clip(pos, blk.astype(dt)*kd, (blk+1).astype(dt)*kd), blk


def wrapped_cell(pos, length, d, n):
    return np.clip(((pos - np.floor(pos/length)*length) / d).astype(np.int64), 0, n - 1)


def cross_bg(M, pt, a, q, frozen):
    """cross for lanes inside background layers: one draw (tau = -log u) for the lanes without a pending free path, the distance
    to the z face, and on the lanes whose tau outlasts the layer the step to the face: into the next layer, out through TOA (the
    mask toa: dropped here) or down to the domain top (the mask enter: the grid's block, the wrap and z are set here). x and y run
    unwrapped and unclamped (not at all when frozen)."""
    dt = pt.dtype
    F = dt.type
    zero, inf = F(0.), F(np.inf)
    G = M.G
    knx, kny, knz = G.scene.kn_grid
    b = q.k_n - knz
    z_lo, z_hi, kn_val = M.z[b], M.z[b+1], M.k_ext[b]
    sz = np.where(q.uz > zero, (z_hi - q.z)/q.uz, np.where(q.uz < zero, (z_lo - q.z)/q.uz, inf)).astype(dt)
    d_max = np.minimum(sz, np.minimum(inf, inf))
    tau = q.tau
    fresh = ~q.pend
    tau[fresh] = -np.log(pt.draw(a[fresh]))
    pend = np.zeros(a.size, dtype=bool)
    empty = ~(kn_val > zero)
    tau_cell = np.where(empty, zero, d_max*kn_val).astype(dt)
    crossed = empty | (tau >= tau_cell)
    lost = crossed & ~(d_max < inf)
    pt.n_capped += int(lost.sum())
    q.alive[lost] = False
    c = crossed & ~lost
    tau = np.where(c, tau - tau_cell, tau)
    pend[c] = True
    x, y = q.x, q.y
    if not frozen:
        x = np.where(c, x + q.ux*d_max, x)
        y = np.where(c, y + q.uy*d_max, y)
    z = np.where(c, np.clip(q.z + q.uz*d_max, z_lo, z_hi), q.z)
    up, dn = c & (q.uz > zero), c & ~(q.uz > zero)
    toa, enter = up & (b == M.nbg - 1), dn & (b == 0)
    k_n, i_n, j_n = q.k_n.copy(), q.i_n.copy(), q.j_n.copy()
    m = up & ~toa
    k_n[m] += 1; z = np.where(m, M.z[np.minimum(b + 1, M.nbg)], z)
    m = dn & ~enter
    k_n[m] -= 1; z = np.where(m, M.z[b], z)
    q.alive[toa] = False
    if enter.any():
        if not frozen:
            xe, ie = enter_grid(x[enter], G.len_x, G.kdx, knx)
            ye, je = enter_grid(y[enter], G.len_y, G.kdy, kny)
            x[enter], i_n[enter], y[enter], j_n[enter] = xe, ie, ye, je
        k_n[enter] = knz - 1
        z = np.where(enter, G.z_top, z)
    q.x, q.y, q.z, q.tau, q.pend, q.i_n, q.j_n, q.k_n = x.astype(dt), y.astype(dt), z.astype(dt), tau.astype(dt), pend, i_n, j_n, k_n
    q.crossed, q.kn_val, q.layer, q.z_hi = crossed, kn_val, b, z_hi
    return toa, enter


def collide_bg(M, q, h, frozen):
    """collide for lanes inside background layers: the move of the lanes h, and the layer's k_ext, k_sca, k_sca_cld, k_sca_aer,
    f_no_abs (cell: the layer)"""
    dt = q.x.dtype
    one, zero = dt.type(1.), dt.type(0.)
    b = q.layer
    dn_ = q.tau / q.kn_val
    if not frozen:
        q.x = np.where(h, q.x + q.ux*dn_, q.x).astype(dt)
        q.y = np.where(h, q.y + q.uy*dn_, q.y).astype(dt)
    q.z = np.where(h, np.clip(q.z + q.uz*dn_, M.z[b], M.z[b+1]), q.z).astype(dt)
    k_ext, k_sca, k_sca_cld, k_sca_aer = q.kn_val, M.k_sca[b], M.k_sca_cld[b], M.k_sca_aer[b]
    f_no_abs = np.clip(one - (k_ext - k_sca)/q.kn_val, zero, one)
    return SimpleNamespace(cell=b, k_ext=k_ext, k_sca=k_sca, k_sca_cld=k_sca_cld, k_sca_aer=k_sca_aer, f_no_abs=f_no_abs)


def through_the_top(M, q, top):
    """the lanes that cross dropped at the domain top go on into layer 0 (with a background); the last step of the grid's event,
    whose steps look at every lane's block"""
    if M.nbg and top.any():
        q.alive[top] = True
        q.k_n[top] = M.knz
        q.z[top] = M.z[0]


def events(pt, max_events, knz, grid_event, bg_event):
    """The event loop of both tracers: every pass deals its lanes a, with their state, to the grid's event or the background's
    by their block."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a, p in pt.passes(max_events):
            above = p.k_n >= knz
            for m, event in ((~above, grid_event), (above, bg_event)):
                if m.any():
                    q = SimpleNamespace(**{k: getattr(p, k)[m] for k in pt.state})
                    event(a[m], q)
                    for k in pt.state:
                        getattr(p, k)[m] = getattr(q, k)


# ---- the tallies of the forward tracer and their conversion to fluxes

def tallies(scene, bg, dtype):
    """zeros by ALL_COUNTS: (ncol,) at the surface, the domain top and TOA, abs_*: (nz, ncol), bg_abs_*: (nbg,)"""
    nbg = bg.nbg if bg is not None else 0
    out = {k: np.zeros(scene.ncol, dtype=dtype) for k in COUNT_NAMES[:4] + BG_COUNT_NAMES[:3]}
    out.update({k: np.zeros((scene.nz, scene.ncol), dtype=dtype) for k in COUNT_NAMES[4:]})
    out.update({k: np.zeros(nbg, dtype=dtype) for k in BG_COUNT_NAMES[3:]})
    return out


def counts_to_flux(counts, scale, out):
    F = out.dtype.type
    return out + (counts.astype(np.float64) * 2.0**-32).astype(out.dtype) * F(scale)


def add_fluxes(flux, counts, scale, scene, bg):
    """flux += counts 2^-32 scale in W m-2; abs_*: W m-3, bg_abs_*: W m-3 of a domain-wide layer"""
    F = scene.dtype.type
    for k in COUNT_NAMES[:4] + BG_COUNT_NAMES[:3]:
        flux[k] = counts_to_flux(counts[k], scale, flux[k])
    for k in COUNT_NAMES[4:]:
        flux[k] = counts_to_flux(counts[k], scale / F(scene.dz), flux[k])
    for k in BG_COUNT_NAMES[3:]:
        for b in range(flux[k].size):
            flux[k][b:b+1] = counts_to_flux(counts[k][b:b+1], (scale / F(bg.dz[b])) / F(scene.ncol), flux[k][b:b+1])


def trace_counts(scene, igpt, photon0, nphotons, max_events=1 << 20, table=None, bg=None, weight0=1):
    """The photons [photon0, photon0 + nphotons) of g-point igpt (rrx_rt_trace_counts and its _phase, _bg and _aer forms; with
    weight0, the photons of one g-point in rrx_rt_trace_counts_spectral). table: a raytracer_phase_ref.Table with cld_re for the
    cloud inside the grid; bg: a Background, None for a medium that ends at the domain top; weight0: every deposit is
    to_count(w weight0), in the scene's precision. Returns the counts by ALL_COUNTS (abs_*: (nz, ncol); toa_up, tod_dn_*: (ncol,),
    zeros without a background; bg_abs_*: (nbg,)), n_capped, events (collisions + crossings of all photons), cloud_scatterings and
    aerosol_scatterings."""
    s = scene
    dt = s.dtype
    F = dt.type
    nx, ncol = s.nx, s.ncol
    knz = s.kn_grid[2]
    ic = bool(s.independent_column)
    G = Grid(s, igpt, table, ic)
    M = Medium(G, bg, igpt)
    one, zero = F(1.), F(0.)
    sun_x, sun_y, sun_z = sun_direction(s)
    dif_frac = F(s.inc_dif[igpt]) / (F(s.inc_dir[igpt]) + F(s.inc_dif[igpt]))

    out = tallies(s, bg, np.uint64)

    def add(name, idx, weight):
        np.add.at(out[name].reshape(-1), idx, to_count(weight*F(weight0)))

    def add_kind(names, kind, idx, weight):
        add(names[0], idx[kind == 0], weight[kind == 0])
        add(names[1], idx[kind == 1], weight[kind == 1])

    # ---- start: at the top of the medium, three draws (x, y, direct or diffuse) and the diffuse photons' lambert
    N = int(nphotons)
    pt = Particles(photon0, N, igpt, s.seed, dt)
    everyone = np.arange(N)
    pix = (pt.index % np.uint64(ncol)).astype(np.int64)
    ix, iy = pix % nx, pix // nx
    IN, JN = ix // G.rx, iy // G.ry
    KN = np.full(N, knz + M.nbg - 1, dtype=np.int64)
    X = np.clip((ix.astype(dt) + pt.draw(everyone))*G.dx, IN.astype(dt)*G.kdx, (IN+1).astype(dt)*G.kdx)
    Y = np.clip((iy.astype(dt) + pt.draw(everyone))*G.dy, JN.astype(dt)*G.kdy, (JN+1).astype(dt)*G.kdy)
    Z = np.full(N, M.z_toa, dtype=dt)
    KIND = (pt.draw(everyone) < dif_frac).astype(np.int64)
    UX, UY, UZ = np.full(N, sun_x, dtype=dt), np.full(N, sun_y, dtype=dt), np.full(N, sun_z, dtype=dt)
    d = np.nonzero(KIND == 1)[0]
    UX[d], UY[d], UZ[d] = lambert(pt, d, F(-1.))
    pt.start(X, Y, Z, UX, UY, UZ, IN, JN, KN, np.ones(N, dtype=bool), kind=KIND)

    def grid_event(a, p):
        top, sfc = cross(G, pt, a, p)
        pixel = fine_cell(p.x, G.dx, p.i_n, G.rx) + nx*fine_cell(p.y, G.dy, p.j_n, G.ry)
        add("tod_up", pixel[top], p.w[top])
        if sfc.any():
            p.z = np.where(sfc, zero, p.z)
            add_kind(("sfc_dn_dir", "sfc_dn_dif"), p.kind[sfc], pixel[sfc], p.w[sfc])
            p.w = np.where(sfc, p.w*G.albedo[pixel], p.w)
            add("sfc_up", pixel[sfc], p.w[sfc])
            roulette(pt, a, p.w, sfc)
            live = sfc & (p.w > zero)
            p.ux[live], p.uy[live], p.uz[live] = lambert(pt, a[live], one)
            p.kind[live] = 1
            p.pend[live] = False
            p.alive[sfc & ~live] = False
        h = ~p.crossed
        if h.any():
            c = collide(G, p, h)
            add_kind(("abs_dir", "abs_dif"), p.kind[h], c.cell[h], (p.w*(one - c.f_no_abs))[h])
            sc, cloud, aerosol = collision_outcome(pt, a, p, h, c)
            if sc.any():
                p.ux, p.uy, p.uz = scatter_direction(pt, a, sc, cloud, aerosol, G.species, c.cell, p.ux, p.uy, p.uz)
                p.kind[sc] = 1
        through_the_top(M, p, top)

    def bg_event(a, q):
        toa, enter = cross_bg(M, pt, a, q, ic)
        add("toa_up", (wrapped_cell(q.x, G.len_x, G.dx, nx) + nx*wrapped_cell(q.y, G.len_y, G.dy, s.ny))[toa], q.w[toa])
        if enter.any():
            pixel = fine_cell(q.x, G.dx, q.i_n, G.rx) + nx*fine_cell(q.y, G.dy, q.j_n, G.ry)
            add_kind(("tod_dn_dir", "tod_dn_dif"), q.kind[enter], pixel[enter], q.w[enter])
        h = ~q.crossed
        if h.any():
            c = collide_bg(M, q, h, ic)
            add_kind(("bg_abs_dir", "bg_abs_dif"), q.kind[h], c.cell[h], (q.w*(one - c.f_no_abs))[h])
            sc, cloud, aerosol = collision_outcome(pt, a, q, h, c)
            if sc.any():
                q.ux, q.uy, q.uz = scatter_direction(pt, a, sc, cloud, aerosol, M.species, c.cell, q.ux, q.uy, q.uz)
                q.kind[sc] = 1

    events(pt, max_events, knz, grid_event, bg_event)
    return dict(out, n_capped=pt.n_capped, events=pt.events, cloud_scatterings=pt.cloud_scatterings,
                aerosol_scatterings=pt.aerosol_scatterings)


def direct_optical_path(scene, igpt, x_sfc, y_sfc):
    """Geometry only, no random numbers: the optical path of the direct beam from the domain top to the surface point
    (x_sfc, y_sfc), through the periodic k_ext field of the gas and the cloud of g-point igpt, in float64 (the straight line cut at
    every cell face)."""
    s = scene
    ib = band_of(s, igpt, s.cloud)
    tc = s.cloud[0][ib] if ib >= 0 else np.zeros_like(s.tau[igpt])
    k_ext = ((s.tau[igpt].astype(np.float64) + tc) / s.dz).reshape(s.nz, s.ny, s.nx)
    if s.top_at_1:
        k_ext = k_ext[::-1]
    mu0 = float(s.mu0)
    st = math.sqrt(max(0.0, 1.0 - mu0*mu0))
    ux, uy, uz = st*math.cos(s.azimuth), st*math.sin(s.azimuth), -mu0
    length = s.nz*s.dz / mu0                       # from the top (t = 0) to the surface (t = length)
    x0, y0 = x_sfc - ux*length, y_sfc - uy*length
    cuts = [0.0, length]
    cuts += [(s.nz*s.dz - k*s.dz) / mu0 for k in range(1, s.nz)]
    for u, p0, d in ((ux, x0, s.dx), (uy, y0, s.dy)):
        if u != 0.0:
            lo, hi = sorted((p0, p0 + u*length))
            cuts += [(m*d - p0)/u for m in range(math.ceil(lo/d), math.floor(hi/d) + 1)]
    cuts = np.clip(np.unique(np.array(cuts)), 0.0, length)
    mid, seg = 0.5*(cuts[1:] + cuts[:-1]), np.diff(cuts)
    i = np.floor((x0 + ux*mid)/s.dx).astype(np.int64) % s.nx
    j = np.floor((y0 + uy*mid)/s.dy).astype(np.int64) % s.ny
    k = np.clip(np.floor((s.nz*s.dz + uz*mid)/s.dz).astype(np.int64), 0, s.nz-1)
    return float(np.sum(k_ext[k, j, i]*seg))


def pixel_path_range(scene, igpt, nsub=5):
    """(min, max) over each pixel, (ncol,) each, of direct_optical_path on an nsub x nsub lattice of surface points that includes
    the pixel's edges (moved inward by 1e-9 of its width)."""
    s = scene
    f = np.linspace(1e-9, 1.0 - 1e-9, nsub)
    lo, hi = np.full(s.ncol, np.inf), np.zeros(s.ncol)
    for pix in range(s.ncol):
        ix, iy = pix % s.nx, pix // s.nx
        t = [direct_optical_path(s, igpt, (ix + fx)*s.dx, (iy + fy)*s.dy) for fx in f for fy in f]
        lo[pix], hi[pix] = min(t), max(t)
    return lo, hi


def raytracer_sw(scene, photons_per_pixel, max_events=1 << 20, bg=None):
    """The spectral loop of rrx_raytracer_sw and its _bg and _aer forms (without a table): broadband fluxes by ALL_COUNTS (W m-2;
    abs_*: W m-3; bg_abs_*: W m-3 of a domain-wide layer), n_capped, and events per g-point."""
    s = scene
    F = s.dtype.type
    ngpt = s.tau.shape[0]
    flux = tallies(s, bg, s.dtype)
    n_capped, events = 0, np.zeros(ngpt, dtype=np.int64)
    for g in range(ngpt):
        inc = F(s.inc_dir[g]) + F(s.inc_dif[g])
        if not inc > 0:
            continue
        c = trace_counts(s, g, 0, photons_per_pixel*s.ncol, max_events, bg=bg)
        add_fluxes(flux, c, inc / F(photons_per_pixel), s, bg)
        n_capped += c["n_capped"]
        events[g] = c["events"]
    flux["n_capped"] = n_capped
    flux["events"] = events
    return flux
