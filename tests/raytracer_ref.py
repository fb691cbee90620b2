"""numpy restatement of the forward Monte Carlo ray tracer (csrc/rrx_raytracer.hip): the same Philox stream, the same
draw order and the same arithmetic, operation for operation, vectorised over the photons (every pass of the loop is one event of
every photon still alive). Arrays are in the package's tensor convention: tau, ssa (ngpt, nz, ncol), the cloud triple
(nbnd, nz, ncol), sfc_albedo (ncol,), ncol = nx ny with x fastest; counts are uint64 in units of 2^-32 photon.

The transport steps that the two tracers share (csrc/rrx_rt_common.h) are stated once, here, under the device functions' names
where there is one; raytracer_bw_ref.py runs its rays through the same steps. The contract of every step is the draw order and the
association of every expression: it draws exactly the uniforms that its docstring names, for that selection, in that sequence. The
cloud species is Henyey-Greenstein from cld_g, or a table of raytracer_phase_ref.py (csrc/rrx_rt_phase.h) with cld_re."""
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np

from mcica_ref import philox4x32_10, uniform, band_of_gpt
import raytracer_phase_ref as P

TWO_PI = 6.283185307179586
COUNT_NAMES = ("sfc_dn_dir", "sfc_dn_dif", "sfc_up", "tod_up", "abs_dir", "abs_dif")


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

    @property
    def ncol(self):
        return self.nx * self.ny

    @property
    def dtype(self):
        return self.tau.dtype


def band_of(scene, igpt):
    if scene.cloud is None:
        return -1
    return int(band_of_gpt(scene.band_lims, scene.tau.shape[0])[igpt])


def k_null(scene, igpt):
    """(knz, kny, knx), kn counted upward from the surface: the maximum of k_ext = (tau + tau_c)/dz over each block."""
    F = scene.dtype.type
    ib = band_of(scene, igpt)
    tc = scene.cloud[0][ib] if ib >= 0 else np.zeros_like(scene.tau[igpt])
    k_ext = ((scene.tau[igpt] + tc) / F(scene.dz)).reshape(scene.nz, scene.ny, scene.nx)
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


# ---- the cloud species: the cosine of a scattering angle from one uniform, and the density towards a direction. Both evaluate on
# all lanes of a pass (cell: the lanes' cells); neither draws.

class HenyeyGreenstein:
    def __init__(self, scene, ib):
        dt = scene.dtype
        self.gc = scene.cloud[2][ib].reshape(-1) if ib >= 0 else np.zeros(scene.nz*scene.ncol, dtype=dt)
        self.g_max = dt.type(1.) - np.finfo(dt).eps

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


class Grid:
    """One g-point of a scene in the scene's precision: the cells and the k_null blocks, the optical properties by cell (the cloud's
    are zeros where the g-point lies in no band) and the cloud species. independent_column: no horizontal transport."""
    def __init__(self, scene, igpt, table=None, independent_column=False):
        s = scene
        dt = s.dtype
        F = dt.type
        self.scene, self.independent_column = s, bool(independent_column)
        knx, kny, knz = s.kn_grid
        self.rx, self.ry, self.rz = s.nx//knx, s.ny//kny, s.nz//knz
        self.dx, self.dy, self.dz = F(s.dx), F(s.dy), F(s.dz)
        self.kdx, self.kdy, self.kdz = F(self.rx)*self.dx, F(self.ry)*self.dy, F(self.rz)*self.dz
        ib = band_of(s, igpt)
        self.tau, self.ssa = s.tau[igpt].reshape(-1), s.ssa[igpt].reshape(-1)
        none = np.zeros(s.nz*s.ncol, dtype=dt)
        self.cld_tau, self.cld_ssa = (c[ib].reshape(-1) for c in s.cloud[:2]) if ib >= 0 else (none, none)
        self.species = HenyeyGreenstein(s, ib) if table is None else Tabulated(s, ib, table)
        self.albedo = np.asarray(s.sfc_albedo, dtype=dt)
        self.k_null = k_null(s, igpt)

    def cell(self, i, j, k):
        """cell = icol + ncol*lay of the fine cell (i, j, k), k counted upward from the surface"""
        s = self.scene
        lay = s.nz - 1 - k if s.top_at_1 else k
        return i + j*s.nx + s.ncol*lay

    def k_ext(self, cell):
        return (self.tau[cell] + self.cld_tau[cell]) / self.dz


class Particles:
    """The photons or rays [first, first + n) of one launch: each one's Philox stream (Stream of rrx_rt_common.h: counter
    (c0, c1, c2, nd >> 2), word nd & 3; the forward tracer's c2 is igpt, the backward one's igpt | 0x80000000), after start() their
    state, and the tallies n_capped, events (collisions + crossings) and cloud_scatterings."""
    def __init__(self, first, n, c2, seed, dtype):
        self.index = np.uint64(first) + np.arange(int(n), dtype=np.uint64)
        self.c0, self.c1, self.c2 = self.index & np.uint64(0xFFFFFFFF), self.index >> np.uint64(32), int(c2)
        self.key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        self.nd = np.zeros(int(n), dtype=np.int64)
        self.dtype = dtype
        self.n_capped = self.events = self.cloud_scatterings = 0

    def draw(self, sel):
        """one draw for sel: the next uniform of each"""
        if sel.size == 0:
            return np.zeros(0, dtype=self.dtype)
        w = philox4x32_10((self.c0[sel], self.c1[sel], np.full(sel.size, self.c2, dtype=np.int64), self.nd[sel] >> 2), self.key)
        x = np.choose(self.nd[sel] & 3, w)
        self.nd[sel] += 1
        return uniform(x, self.dtype)

    def start(self, x, y, z, ux, uy, uz, i_n, j_n, k_n, alive):
        """positions, directions and k_null blocks; weight 1, no free path pending"""
        n, dt = self.nd.size, self.dtype
        self.state = dict(x=x, y=y, z=z, ux=ux, uy=uy, uz=uz, i_n=i_n, j_n=j_n, k_n=k_n, alive=alive, w=np.ones(n, dtype=dt),
                          tau=np.zeros(n, dtype=dt), pend=np.zeros(n, dtype=bool))
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
    k_sca, k_sca_cld and the share f_no_abs of the weight that a collision leaves."""
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
    t, w0, tc, wc = G.tau[cell], G.ssa[cell], G.cld_tau[cell], G.cld_ssa[cell]
    k_ext = G.k_ext(cell)
    k_sca = (t*w0 + tc*wc) / G.dz
    k_sca_cld = (tc*wc) / G.dz
    f_no_abs = np.clip(one - (k_ext - k_sca)/p.kn_val, zero, one)
    return SimpleNamespace(i=i, j=j, k=k, cell=cell, k_ext=k_ext, k_sca=k_sca, k_sca_cld=k_sca_cld, f_no_abs=f_no_abs)


def collision_outcome(pt, a, p, h, c):
    """w *= f_no_abs on the lanes h, then up to three draws: the roulette; for the survivors, scattering or a null collision; for
    those that scatter, cloud or gas. Returns the masks of the lanes that scatter and that scatter by cloud."""
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
    pt.cloud_scatterings += int(cloud.sum())
    return sc, cloud


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


def scatter_direction(pt, a, sc, cloud, species, cell, ux, uy, uz):
    """two draws for the lanes sc: u -> the cosine of the scattering angle (the cloud species on the lanes cloud, Rayleigh on the
    others; u = 1/2 on the lanes that do not scatter), then rotate_direction's"""
    dt = pt.dtype
    F = dt.type
    u = np.full(a.size, F(0.5), dtype=dt); u[sc] = pt.draw(a[sc])
    cos_s = np.clip(np.where(cloud, species.cos(cell, u), rayleigh_cos(u)), F(-1.), F(1.)).astype(dt)
    return rotate_direction(pt, a, sc, cos_s, ux, uy, uz)


def trace_counts(scene, igpt, photon0, nphotons, max_events=1 << 20, table=None):
    """The photons [photon0, photon0 + nphotons) of g-point igpt; the cloud species is Henyey-Greenstein from cld_g, or table (a
    raytracer_phase_ref.Table with cld_re: rrx_rt_trace_counts_phase). Returns the six count arrays (abs_*: (nz, ncol)), n_capped,
    events (collisions + crossings of all photons) and cloud_scatterings."""
    s = scene
    dt = s.dtype
    F = dt.type
    nx, nz, ncol = s.nx, s.nz, s.ncol
    knz = s.kn_grid[2]
    G = Grid(s, igpt, table, s.independent_column)
    one, zero = F(1.), F(0.)
    sun_x, sun_y, sun_z = sun_direction(s)
    dif_frac = F(s.inc_dif[igpt]) / (F(s.inc_dir[igpt]) + F(s.inc_dif[igpt]))

    out = {k: np.zeros(ncol, dtype=np.uint64) for k in COUNT_NAMES[:4]}
    out.update({k: np.zeros(ncol*nz, dtype=np.uint64) for k in COUNT_NAMES[4:]})

    def add(name, idx, weight):
        np.add.at(out[name], idx, to_count(weight))

    def add_kind(names, kind, idx, weight):
        add(names[0], idx[kind == 0], weight[kind == 0])
        add(names[1], idx[kind == 1], weight[kind == 1])

    # ---- start: at the domain top, three draws (x, y, direct or diffuse) and the diffuse photons' lambert
    N = int(nphotons)
    pt = Particles(photon0, N, igpt, s.seed, dt)
    everyone = np.arange(N)
    pix = (pt.index % np.uint64(ncol)).astype(np.int64)
    ix, iy = pix % nx, pix // nx
    IN, JN, KN = ix // G.rx, iy // G.ry, np.full(N, knz-1, dtype=np.int64)
    X = np.clip((ix.astype(dt) + pt.draw(everyone))*G.dx, IN.astype(dt)*G.kdx, (IN+1).astype(dt)*G.kdx)
    Y = np.clip((iy.astype(dt) + pt.draw(everyone))*G.dy, JN.astype(dt)*G.kdy, (JN+1).astype(dt)*G.kdy)
    Z = np.full(N, F(knz)*G.kdz, dtype=dt)
    KIND = (pt.draw(everyone) < dif_frac).astype(np.int64)
    UX, UY, UZ = np.full(N, sun_x, dtype=dt), np.full(N, sun_y, dtype=dt), np.full(N, sun_z, dtype=dt)
    d = np.nonzero(KIND == 1)[0]
    UX[d], UY[d], UZ[d] = lambert(pt, d, F(-1.))
    pt.start(X, Y, Z, UX, UY, UZ, IN, JN, KN, np.ones(N, dtype=bool))

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a, p in pt.passes(max_events):
            kind = KIND[a]
            top, sfc = cross(G, pt, a, p)
            pixel = fine_cell(p.x, G.dx, p.i_n, G.rx) + nx*fine_cell(p.y, G.dy, p.j_n, G.ry)
            add("tod_up", pixel[top], p.w[top])
            if sfc.any():
                p.z = np.where(sfc, zero, p.z)
                add_kind(("sfc_dn_dir", "sfc_dn_dif"), kind[sfc], pixel[sfc], p.w[sfc])
                p.w = np.where(sfc, p.w*G.albedo[pixel], p.w)
                add("sfc_up", pixel[sfc], p.w[sfc])
                roulette(pt, a, p.w, sfc)
                live = sfc & (p.w > zero)
                p.ux[live], p.uy[live], p.uz[live] = lambert(pt, a[live], one)
                kind[live] = 1
                p.pend[live] = False
                p.alive[sfc & ~live] = False
            h = ~p.crossed
            if h.any():
                c = collide(G, p, h)
                add_kind(("abs_dir", "abs_dif"), kind[h], c.cell[h], (p.w*(one - c.f_no_abs))[h])
                sc, cloud = collision_outcome(pt, a, p, h, c)
                if sc.any():
                    p.ux, p.uy, p.uz = scatter_direction(pt, a, sc, cloud, G.species, c.cell, p.ux, p.uy, p.uz)
                    kind = np.where(sc, 1, kind)
            KIND[a] = kind

    res = {k: v for k, v in out.items()}
    res["abs_dir"] = res["abs_dir"].reshape(nz, ncol)
    res["abs_dif"] = res["abs_dif"].reshape(nz, ncol)
    res["n_capped"] = pt.n_capped
    res["events"] = pt.events
    res["cloud_scatterings"] = pt.cloud_scatterings
    return res


def direct_optical_path(scene, igpt, x_sfc, y_sfc):
    """Geometry only, no random numbers: the optical path of the direct beam from the domain top to the surface point
    (x_sfc, y_sfc), through the periodic k_ext field of g-point igpt, in float64 (the straight line cut at every cell face)."""
    s = scene
    ib = band_of(s, igpt)
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


def counts_to_flux(counts, scale, out):
    F = out.dtype.type
    return out + (counts.astype(np.float64) * 2.0**-32).astype(out.dtype) * F(scale)


def raytracer_sw(scene, photons_per_pixel, max_events=1 << 20):
    """The spectral loop of rrx_raytracer_sw: broadband fluxes (W m-2; absorption W m-3), n_capped, and events per g-point."""
    s = scene
    dt = s.dtype
    F = dt.type
    ngpt = s.tau.shape[0]
    flux = {k: np.zeros(s.ncol, dtype=dt) for k in COUNT_NAMES[:4]}
    flux.update({k: np.zeros((s.nz, s.ncol), dtype=dt) for k in COUNT_NAMES[4:]})
    n_capped, events = 0, np.zeros(ngpt, dtype=np.int64)
    for g in range(ngpt):
        inc = F(s.inc_dir[g]) + F(s.inc_dif[g])
        if not inc > 0:
            continue
        c = trace_counts(s, g, 0, photons_per_pixel*s.ncol, max_events)
        scale = inc / F(photons_per_pixel)
        for k in COUNT_NAMES:
            flux[k] = counts_to_flux(c[k], scale if k in COUNT_NAMES[:4] else scale / F(s.dz), flux[k])
        n_capped += c["n_capped"]
        events[g] = c["events"]
    flux["n_capped"] = n_capped
    flux["events"] = events
    return flux
