"""numpy restatement of the two ray tracers with a background atmosphere between the domain top and TOA (csrc/rrx_rt_common.h,
the BG instantiations of csrc/rrx_raytracer.hip and csrc/rrx_raytracer_bw.hip): the same Philox streams, the same
draw order and the same arithmetic, operation for operation. The transport steps inside the grid are those of raytracer_ref (cross,
collide, collision_outcome, scatter_direction, ...); what is stated here is the background's own: its profile and levels, the event
of a photon or ray inside a background layer, the passage through the domain top in both directions, and the two event loops that
deal the lanes of a pass to the grid's event or the background's. Every lane has its own Philox stream, so the order in which the
two groups of a pass are served does not matter.

A Background is counted upward from the domain top whatever the scene's top_at_1 is: dz (nbg,), tau, ssa (ngpt, nbg), cloud None
or (tau, ssa, g) of (nbnd, nbg) each."""
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np

import raytracer_ref as R
import raytracer_bw_ref as B

BG_COUNT_NAMES = ("toa_up", "tod_dn_dir", "tod_dn_dif", "bg_abs_dir", "bg_abs_dif")
STATE = ("x", "y", "z", "ux", "uy", "uz", "i_n", "j_n", "k_n", "alive", "w", "tau", "pend")


@dataclass
class Background:
    dz: np.ndarray
    tau: np.ndarray
    ssa: np.ndarray
    cloud: Optional[tuple] = None

    @property
    def nbg(self):
        return int(np.asarray(self.dz).size)


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


def profile(scene, bg, igpt):
    """(5, nbg+1) of rrx_rt_bg_profile: k_ext, k_sca, k_sca_cld, g, tau_above"""
    dt = scene.dtype
    F = dt.type
    nbg = bg.nbg
    ib = int(R.band_of_gpt(scene.band_lims, scene.tau.shape[0])[igpt]) if bg.cloud is not None else -1
    t, w0, dz = bg.tau[igpt].astype(dt), bg.ssa[igpt].astype(dt), np.asarray(bg.dz, dtype=dt)
    zeros = np.zeros(nbg, dtype=dt)
    tc, wc, gc = (c[ib].astype(dt) for c in bg.cloud) if ib >= 0 else (zeros, zeros, zeros)
    out = np.zeros((5, nbg + 1), dtype=dt)
    out[0, :nbg] = (t + tc) / dz
    out[1, :nbg] = (t*w0 + tc*wc) / dz
    out[2, :nbg] = (tc*wc) / dz
    out[3, :nbg] = np.minimum(gc, F(1.) - np.finfo(dt).eps)
    layer = t + tc
    for b in range(nbg + 1):
        above = F(0.)
        for l in range(0 if b == nbg else b + 1, nbg):
            above = above + layer[l]
        out[4, b] = above
    return out


class Medium:
    """The background of one g-point beside a raytracer_ref.Grid: the levels, the rows of the profile, and the Henyey-Greenstein
    species of the layers (the phase table applies inside the grid only)."""
    def __init__(self, G, bg, igpt):
        s = G.scene
        dt = s.dtype
        self.G, self.nbg, self.knz = G, (bg.nbg if bg is not None else 0), s.kn_grid[2]
        knx, kny, _ = s.kn_grid
        self.len_x, self.len_y = dt.type(knx)*G.kdx, dt.type(kny)*G.kdy
        self.z_top = dt.type(self.knz)*G.kdz
        if self.nbg:
            self.z = levels(s, bg)
            self.k_ext, self.k_sca, self.k_sca_cld, g, self.tau_above = profile(s, bg, igpt)
            self.species = object.__new__(R.HenyeyGreenstein)
            self.species.gc, self.species.g_max = g, dt.type(1.) - np.finfo(dt).eps
        self.z_toa = self.z[self.nbg] if self.nbg else self.z_top


def _sub(p, m):
    return SimpleNamespace(**{k: getattr(p, k)[m] for k in STATE})


def _put(p, m, q):
    for k in STATE:
        getattr(p, k)[m] = getattr(q, k)


def enter_grid(pos, length, kd, nblk):
    """no draw: a coordinate that comes down into the grid, wrapped, with its block, clamped into it"""
    dt = pos.dtype
    pos = (pos - np.floor(pos/length)*length).astype(dt)
    blk = np.clip((pos/kd).astype(np.int64), 0, nblk - 1)
    return np.clip(pos, blk.astype(dt)*kd, (blk+1).astype(dt)*kd), blk


def wrapped_cell(pos, length, d, n):
    return np.clip(((pos - np.floor(pos/length)*length) / d).astype(np.int64), 0, n - 1)


def cross_bg(M, pt, a, q, frozen):
    """R.cross for lanes inside background layers: one draw (tau = -log u) for the lanes without a pending free path, the distance
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
            xe, ie = enter_grid(x[enter], M.len_x, G.kdx, knx)
            ye, je = enter_grid(y[enter], M.len_y, G.kdy, kny)
            x[enter], i_n[enter], y[enter], j_n[enter] = xe, ie, ye, je
        k_n[enter] = knz - 1
        z = np.where(enter, M.z_top, z)
    q.x, q.y, q.z, q.tau, q.pend, q.i_n, q.j_n, q.k_n = x.astype(dt), y.astype(dt), z.astype(dt), tau.astype(dt), pend, i_n, j_n, k_n
    q.crossed, q.kn_val, q.layer, q.z_hi = crossed, kn_val, b, z_hi
    return toa, enter


def collide_bg(M, q, h, frozen):
    """R.collide for lanes inside background layers: the move of the lanes h, and the layer's k_ext, k_sca, k_sca_cld, f_no_abs"""
    dt = q.x.dtype
    one, zero = dt.type(1.), dt.type(0.)
    b = q.layer
    dn_ = q.tau / q.kn_val
    if not frozen:
        q.x = np.where(h, q.x + q.ux*dn_, q.x).astype(dt)
        q.y = np.where(h, q.y + q.uy*dn_, q.y).astype(dt)
    q.z = np.where(h, np.clip(q.z + q.uz*dn_, M.z[b], M.z[b+1]), q.z).astype(dt)
    k_ext, k_sca, k_sca_cld = q.kn_val, M.k_sca[b], M.k_sca_cld[b]
    f_no_abs = np.clip(one - (k_ext - k_sca)/q.kn_val, zero, one)
    return SimpleNamespace(cell=b, k_ext=k_ext, k_sca=k_sca, k_sca_cld=k_sca_cld, f_no_abs=f_no_abs)


def through_the_top(M, q, top):
    """the lanes that R.cross dropped at the domain top go on into layer 0 (with a background); the last step of the grid's event,
    whose steps look at every lane's block"""
    if M.nbg and top.any():
        q.alive[top] = True
        q.k_n[top] = M.knz
        q.z[top] = M.z[0]


# ---- the forward tracer

def trace_counts(scene, bg, igpt, photon0, nphotons, max_events=1 << 20, table=None):
    """rrx_rt_trace_counts_bg: the six counts of raytracer_ref.trace_counts and BG_COUNT_NAMES (toa_up, tod_dn_*: (ncol,),
    bg_abs_*: (nbg,)), n_capped, events. bg None: the medium without a background."""
    s = scene
    dt = s.dtype
    F = dt.type
    nx, nz, ncol = s.nx, s.nz, s.ncol
    knz = s.kn_grid[2]
    ic = bool(s.independent_column)
    G = R.Grid(s, igpt, table, ic)
    M = Medium(G, bg, igpt)
    one, zero = F(1.), F(0.)
    sun_x, sun_y, sun_z = R.sun_direction(s)
    dif_frac = F(s.inc_dif[igpt]) / (F(s.inc_dir[igpt]) + F(s.inc_dif[igpt]))

    out = {k: np.zeros(ncol, dtype=np.uint64) for k in R.COUNT_NAMES[:4] + BG_COUNT_NAMES[:3]}
    out.update({k: np.zeros(ncol*nz, dtype=np.uint64) for k in R.COUNT_NAMES[4:]})
    out.update({k: np.zeros(M.nbg, dtype=np.uint64) for k in BG_COUNT_NAMES[3:]})

    def add(name, idx, weight):
        np.add.at(out[name], idx, R.to_count(weight))

    def add_kind(names, kind, idx, weight):
        add(names[0], idx[kind == 0], weight[kind == 0])
        add(names[1], idx[kind == 1], weight[kind == 1])

    N = int(nphotons)
    pt = R.Particles(photon0, N, igpt, s.seed, dt)
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
    UX[d], UY[d], UZ[d] = R.lambert(pt, d, F(-1.))
    pt.start(X, Y, Z, UX, UY, UZ, IN, JN, KN, np.ones(N, dtype=bool))

    def grid_event(a, p, kind):
        top, sfc = R.cross(G, pt, a, p)
        pixel = R.fine_cell(p.x, G.dx, p.i_n, G.rx) + nx*R.fine_cell(p.y, G.dy, p.j_n, G.ry)
        add("tod_up", pixel[top], p.w[top])
        if sfc.any():
            p.z = np.where(sfc, zero, p.z)
            add_kind(("sfc_dn_dir", "sfc_dn_dif"), kind[sfc], pixel[sfc], p.w[sfc])
            p.w = np.where(sfc, p.w*G.albedo[pixel], p.w)
            add("sfc_up", pixel[sfc], p.w[sfc])
            R.roulette(pt, a, p.w, sfc)
            live = sfc & (p.w > zero)
            p.ux[live], p.uy[live], p.uz[live] = R.lambert(pt, a[live], one)
            kind[live] = 1
            p.pend[live] = False
            p.alive[sfc & ~live] = False
        h = ~p.crossed
        if h.any():
            c = R.collide(G, p, h)
            add_kind(("abs_dir", "abs_dif"), kind[h], c.cell[h], (p.w*(one - c.f_no_abs))[h])
            sc, cloud = R.collision_outcome(pt, a, p, h, c)
            if sc.any():
                p.ux, p.uy, p.uz = R.scatter_direction(pt, a, sc, cloud, G.species, c.cell, p.ux, p.uy, p.uz)
                kind[sc] = 1
        through_the_top(M, p, top)

    def bg_event(a, q, kind):
        toa, enter = cross_bg(M, pt, a, q, ic)
        add("toa_up", (wrapped_cell(q.x, M.len_x, G.dx, nx) + nx*wrapped_cell(q.y, M.len_y, G.dy, s.ny))[toa], q.w[toa])
        if enter.any():
            pixel = R.fine_cell(q.x, G.dx, q.i_n, G.rx) + nx*R.fine_cell(q.y, G.dy, q.j_n, G.ry)
            add_kind(("tod_dn_dir", "tod_dn_dif"), kind[enter], pixel[enter], q.w[enter])
        h = ~q.crossed
        if h.any():
            c = collide_bg(M, q, h, ic)
            add_kind(("bg_abs_dir", "bg_abs_dif"), kind[h], c.cell[h], (q.w*(one - c.f_no_abs))[h])
            sc, cloud = R.collision_outcome(pt, a, q, h, c)
            if sc.any():
                q.ux, q.uy, q.uz = R.scatter_direction(pt, a, sc, cloud, M.species, c.cell, q.ux, q.uy, q.uz)
                kind[sc] = 1

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a, p in pt.passes(max_events):
            above = p.k_n >= knz
            for m, event in ((~above, grid_event), (above, bg_event)):
                if m.any():
                    q, kind = _sub(p, m), KIND[a[m]]
                    event(a[m], q, kind)
                    _put(p, m, q)
                    KIND[a[m]] = kind

    res = {k: v for k, v in out.items()}
    res["abs_dir"] = res["abs_dir"].reshape(nz, ncol)
    res["abs_dif"] = res["abs_dif"].reshape(nz, ncol)
    res["n_capped"] = pt.n_capped
    res["events"] = pt.events
    return res


def raytracer_sw(scene, bg, photons_per_pixel, max_events=1 << 20):
    """The spectral loop of rrx_raytracer_sw_bg: broadband fluxes (W m-2; abs_*: W m-3; bg_abs_*: W m-3 of a domain-wide layer),
    n_capped, and events per g-point."""
    s = scene
    dt = s.dtype
    F = dt.type
    ngpt = s.tau.shape[0]
    nbg = bg.nbg if bg is not None else 0
    flux = {k: np.zeros(s.ncol, dtype=dt) for k in R.COUNT_NAMES[:4] + BG_COUNT_NAMES[:3]}
    flux.update({k: np.zeros((s.nz, s.ncol), dtype=dt) for k in R.COUNT_NAMES[4:]})
    flux.update({k: np.zeros(nbg, dtype=dt) for k in BG_COUNT_NAMES[3:]})
    n_capped, events = 0, np.zeros(ngpt, dtype=np.int64)
    for g in range(ngpt):
        inc = F(s.inc_dir[g]) + F(s.inc_dif[g])
        if not inc > 0:
            continue
        c = trace_counts(s, bg, g, 0, photons_per_pixel*s.ncol, max_events)
        scale = inc / F(photons_per_pixel)
        for k in R.COUNT_NAMES[:4] + BG_COUNT_NAMES[:3]:
            flux[k] = R.counts_to_flux(c[k], scale, flux[k])
        for k in R.COUNT_NAMES[4:]:
            flux[k] = R.counts_to_flux(c[k], scale / F(s.dz), flux[k])
        for k in BG_COUNT_NAMES[3:]:
            for b in range(nbg):
                flux[k][b:b+1] = R.counts_to_flux(c[k][b:b+1], (scale / F(bg.dz[b])) / F(s.ncol), flux[k][b:b+1])
        n_capped += c["n_capped"]
        events[g] = c["events"]
    flux["n_capped"] = n_capped
    flux["events"] = events
    return flux


# ---- the backward tracer

def trace_counts_bw(scene, bg, sensor, igpt, ray0, nrays, max_events=1 << 20, ranges=1, table=None):
    """rrx_rt_bw_trace_counts_bg: what raytracer_bw_ref.trace_counts returns. bg None: the medium without a background."""
    s = scene
    dt = s.dtype
    F = dt.type
    nx, ny, nz = s.nx, s.ny, s.nz
    knx, kny, knz = s.kn_grid
    G = R.Grid(s, igpt, table)
    M = Medium(G, bg, igpt)
    dx, dy, dz, kdx, kdy, kdz = G.dx, G.dy, G.dz, G.kdx, G.kdy, G.kdz
    len_x, len_y, z_top, z_toa = M.len_x, M.len_y, M.z_top, M.z_toa
    inf = F(np.inf)
    one, zero, half, two = F(1.), F(0.), F(0.5), F(2.)
    pi = F(B.PI)
    mu0 = F(s.mu0)
    sun_x, sun_y, sun_z = R.sun_direction(s)
    vx, vy, vz = -sun_x, -sun_y, -sun_z
    with np.errstate(divide="ignore"):
        dtx = dx/abs(vx) if vx != 0 else inf
        dty = dy/abs(vy) if vy != 0 else inf
        dtz = dz/vz
    tau_bg_sun = M.tau_above[M.nbg]/mu0 if M.nbg else zero
    walk_bound = B.max_walk(s)
    npx, npy = int(sensor.npx), int(sensor.npy)
    npix = npx*npy
    stype = int(sensor.type)
    pos = [F(v) for v in sensor.position]
    ew, eh, ed = ([F(v) for v in e] for e in (sensor.e_w, sensor.e_h, sensor.e_d))
    fov = F(sensor.fov)

    if int(nrays) % int(ranges) != 0:
        raise ValueError("ranges does not divide nrays")
    counts = np.zeros(ranges*npix, dtype=np.uint64)
    n_dep = np.zeros(ranges*npix, dtype=np.int64)
    sum_d = np.zeros(ranges*npix, dtype=np.float64)
    tot = dict(n_clamped=0, walk_cells=0)

    N = int(nrays)
    pt = R.Particles(ray0, N, int(igpt) | 0x80000000, s.seed, dt)

    def first(v, p, i, d):
        if v > 0:
            return np.maximum(zero, ((i+1).astype(dt)*d - p)/v).astype(dt)
        if v < 0:
            return np.maximum(zero, (i.astype(dt)*d - p)/v).astype(dt)
        return np.full(p.size, inf, dtype=dt)

    def transmission(x, y, z, i, j, k):
        """exp(-(tau_walk + tau_bg_sun)) from (x, y, z) in cell (i, j, k) to TOA along -s: the walk of raytracer_bw_ref to the domain
        top and the background's slant path in one exp; also whether the walk stayed within its bound"""
        n = x.size
        i, j, k = i.copy(), j.copy(), k.copy()
        tx, ty, tz = first(vx, x, i, dx), first(vy, y, j, dy), first(vz, z, k, dz)
        t, tsun = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
        steps = np.zeros(n, dtype=np.int64)
        ok = np.ones(n, dtype=bool)
        go = np.arange(n)
        while go.size:
            tn = np.minimum(tz[go], np.minimum(tx[go], ty[go]))
            axis = np.where((tz[go] <= tx[go]) & (tz[go] <= ty[go]), 2, np.where(tx[go] <= ty[go], 0, 1))
            tsun[go] = tsun[go] + G.k_ext(G.cell(i[go], j[go], k[go]))*(tn - t[go])
            t[go] = tn
            m = go[axis == 0]
            i[m] = np.where(i[m] + 1 == nx, 0, i[m] + 1) if vx > 0 else np.where(i[m] == 0, nx - 1, i[m] - 1)
            tx[m] = tx[m] + dtx
            m = go[axis == 1]
            j[m] = np.where(j[m] + 1 == ny, 0, j[m] + 1) if vy > 0 else np.where(j[m] == 0, ny - 1, j[m] - 1)
            ty[m] = ty[m] + dty
            m = go[axis == 2]
            k[m] += 1
            tz[m] = tz[m] + dtz
            steps[go] += 1
            tot["walk_cells"] += go.size
            over = (k[go] != nz) & (steps[go] >= walk_bound)
            ok[go[over]] = False
            go = go[(k[go] != nz) & ~over]
        return np.exp(-(tsun + tau_bg_sun)), ok

    def score(sel_pix, d, ok):
        clamped = ok & (d > F(B.D_MAX))
        tot["n_clamped"] += int(clamped.sum())
        pt.n_capped += int((~ok).sum())
        d = np.where(clamped, F(B.D_MAX), d)
        np.add.at(counts, sel_pix[ok], R.to_count(d[ok]))
        np.add.at(n_dep, sel_pix[ok], 1)
        np.add.at(sum_d, sel_pix[ok], d[ok].astype(np.float64))

    def deposit(sel_pix, dep, x, y, z, i, j, k):
        if dep.size == 0:
            return np.ones(0, dtype=bool)
        tr, ok = transmission(x, y, z, i, j, k)
        score(sel_pix, (dep*tr).astype(dt), ok)
        return ok

    # ---- start: the draws of raytracer_bw_ref; the top of the medium is TOA
    everyone = np.arange(N)
    PIX = (pt.index % np.uint64(npix)).astype(np.int64)
    ipx, ipy = PIX % npx, PIX // npx
    fa = (ipx.astype(dt) + pt.draw(everyone)) / F(npx)
    fb = (ipy.astype(dt) + pt.draw(everyone)) / F(npy)
    SX, SY, SZ = np.full(N, pos[0], dtype=dt), np.full(N, pos[1], dtype=dt), np.full(N, pos[2], dtype=dt)
    if stype in (0, 1):
        if stype == 0:
            ca, cb = two*fa - one, two*fb - one
            q = [(ew[m]*ca + eh[m]*cb) + ed[m] for m in range(3)]
        else:
            th, ph = (fa*fov)*half, F(R.TWO_PI)*fb
            ct, st, cp, sp = np.cos(th), np.sin(th), np.cos(ph), np.sin(ph)
            q = [ed[m]*ct + st*(ew[m]*cp + eh[m]*sp) for m in range(3)]
        nrm = np.sqrt((q[0]*q[0] + q[1]*q[1]) + q[2]*q[2])
        UX, UY, UZ = (q[0]/nrm).astype(dt), (q[1]/nrm).astype(dt), (q[2]/nrm).astype(dt)
    else:
        SX, SY = fa*len_x, fb*len_y
        if stype == 2:
            UX, UY, UZ = np.full(N, ed[0], dtype=dt), np.full(N, ed[1], dtype=dt), np.full(N, ed[2], dtype=dt)
            SZ = np.full(N, np.clip(pos[2], z_top, z_toa), dtype=dt)
        elif ed[2] > 0:
            UX, UY, UZ = R.lambert(pt, everyone, one)
            SZ = np.zeros(N, dtype=dt)
        else:
            UX, UY, UZ = R.lambert(pt, everyone, -one)
            SZ = np.full(N, np.clip(pos[2], z_top, z_toa), dtype=dt)
    ALIVE = np.ones(N, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        above = SZ >= z_toa
        ALIVE[above & ~(UZ < zero)] = False
        mv = above & (UZ < zero) & (SZ > z_toa)
        tmv = np.where(mv, (z_toa - SZ)/np.where(mv, UZ, one), zero).astype(dt)
        SX = np.where(mv, SX + UX*tmv, SX).astype(dt); SY = np.where(mv, SY + UY*tmv, SY).astype(dt)
        SZ = np.where(above, z_toa, SZ).astype(dt)
        inbg = SZ > z_top
        WX = (SX - np.floor(SX/len_x)*len_x).astype(dt); WY = (SY - np.floor(SY/len_y)*len_y).astype(dt)
        IN = np.clip((WX/kdx).astype(np.int64), 0, knx-1); JN = np.clip((WY/kdy).astype(np.int64), 0, kny-1)
        KN = np.clip((SZ/kdz).astype(np.int64), 0, knz-1)
        X = np.clip(WX, IN.astype(dt)*kdx, (IN+1).astype(dt)*kdx)
        Y = np.clip(WY, JN.astype(dt)*kdy, (JN+1).astype(dt)*kdy)
        Z = np.clip(SZ, KN.astype(dt)*kdz, (KN+1).astype(dt)*kdz)
        if inbg.any():
            layer = np.zeros(N, dtype=np.int64)
            for b in range(1, M.nbg):                      # the largest b with z[b] <= height
                layer[SZ >= M.z[b]] = b
            IN[inbg], JN[inbg], KN[inbg] = 0, 0, knz + layer[inbg]
            X[inbg], Y[inbg] = SX[inbg], SY[inbg]
            Z[inbg] = np.clip(SZ, M.z[layer], M.z[np.minimum(layer + 1, M.nbg)])[inbg]
    pt.start(X, Y, Z, UX, UY, UZ, IN, JN, KN, ALIVE)

    def grid_event(a, p, pixel):
        top, sfc = R.cross(G, pt, a, p)
        if sfc.any():
            p.z = np.where(sfc, zero, p.z)
            i, j = R.fine_cell(p.x, dx, p.i_n, G.rx), R.fine_cell(p.y, dy, p.j_n, G.ry)
            p.w = np.where(sfc, p.w*G.albedo[i + nx*j], p.w)
            dep = ((p.w*mu0)/pi).astype(dt)
            hit = np.nonzero(sfc & (dep > zero))[0]
            ok = deposit(pixel[hit], dep[hit], p.x[hit], p.y[hit], p.z[hit], i[hit], j[hit], np.zeros(hit.size, dtype=np.int64))
            p.alive[hit[~ok]] = False
            go = sfc & p.alive
            R.roulette(pt, a, p.w, go)
            live = go & (p.w > zero)
            p.ux[live], p.uy[live], p.uz[live] = R.lambert(pt, a[live], one)
            p.pend[go] = False
            p.alive[go & ~live] = False
        h = ~p.crossed
        if h.any():
            c = R.collide(G, p, h)
            sc, cloud = R.collision_outcome(pt, a, p, h, c)
            if sc.any():
                cs = np.clip(-((p.ux*sun_x + p.uy*sun_y) + p.uz*sun_z), -one, one).astype(dt)
                p_ray = F(0.75)*(one + cs*cs)
                dep = ((p.w*np.where(cloud, G.species.density(c.cell, cs), p_ray))/(F(4.)*pi)).astype(dt)
                hit = np.nonzero(sc)[0]
                ok = deposit(pixel[hit], dep[hit], p.x[hit], p.y[hit], p.z[hit], c.i[hit], c.j[hit], c.k[hit])
                p.alive[hit[~ok]] = False
                sc = sc & p.alive
                p.ux, p.uy, p.uz = R.scatter_direction(pt, a, sc, cloud, G.species, c.cell, p.ux, p.uy, p.uz)
        through_the_top(M, p, top)

    def bg_event(a, q, pixel):
        cross_bg(M, pt, a, q, False)
        h = ~q.crossed
        if h.any():
            c = collide_bg(M, q, h, False)
            sc, cloud = R.collision_outcome(pt, a, q, h, c)
            if sc.any():
                cs = np.clip(-((q.ux*sun_x + q.uy*sun_y) + q.uz*sun_z), -one, one).astype(dt)
                p_ray = F(0.75)*(one + cs*cs)
                dep = ((q.w*np.where(cloud, M.species.density(c.cell, cs), p_ray))/(F(4.)*pi)).astype(dt)
                d = (dep*np.exp(-((c.k_ext*(q.z_hi - q.z) + M.tau_above[c.cell])/mu0))).astype(dt)
                hit = np.nonzero(sc)[0]
                score(pixel[hit], d[hit], np.ones(hit.size, dtype=bool))
                q.ux, q.uy, q.uz = R.scatter_direction(pt, a, sc, cloud, M.species, c.cell, q.ux, q.uy, q.uz)

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a, p in pt.passes(max_events):
            pixel = PIX[a] + npix*(a // (N // ranges))
            above = p.k_n >= knz
            for m, event in ((~above, grid_event), (above, bg_event)):
                if m.any():
                    q = _sub(p, m)
                    event(a[m], q, pixel[m])
                    _put(p, m, q)

    if ranges > 1:
        counts, n_dep, sum_d = counts.reshape(ranges, npix), n_dep.reshape(ranges, npix), sum_d.reshape(ranges, npix)
    return dict(counts=counts, n_dep=n_dep, sum_d=sum_d, n_capped=pt.n_capped, events=pt.events, **tot)


def raytracer_bw(scene, bg, sensor, rays_per_pixel, max_events=1 << 20):
    """The spectral loop of rrx_raytracer_bw_bg: what raytracer_bw_ref.raytracer_bw returns"""
    s = scene
    dt = s.dtype
    F = dt.type
    ngpt = s.tau.shape[0]
    npix = int(sensor.npx)*int(sensor.npy)
    out = dict(radiance=np.zeros(npix, dtype=dt), n_capped=0, n_clamped=0, n_dep=np.zeros((ngpt, npix), dtype=np.int64),
               sum_d=np.zeros((ngpt, npix)), events=np.zeros(ngpt, dtype=np.int64), walk_cells=np.zeros(ngpt, dtype=np.int64))
    for g in range(ngpt):
        if not F(s.inc_dir[g]) > 0:
            continue
        c = trace_counts_bw(s, bg, sensor, g, 0, rays_per_pixel*npix, max_events)
        scale = F(s.inc_dir[g]) / (F(s.mu0)*F(rays_per_pixel))
        out["radiance"] = R.counts_to_flux(c["counts"], scale, out["radiance"])
        out["n_capped"] += c["n_capped"]; out["n_clamped"] += c["n_clamped"]
        out["n_dep"][g], out["sum_d"][g], out["events"][g], out["walk_cells"][g] = c["n_dep"], c["sum_d"], c["events"], c["walk_cells"]
    return out
