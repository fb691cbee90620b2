"""numpy restatement of the backward Monte Carlo ray tracer (csrc/rrx_raytracer_bw.hip): the same Philox stream
(counter word 2 is igpt | 0x80000000), the same draw order and the same arithmetic, operation for operation, vectorised over the
rays. The medium and the transport steps are those of raytracer_ref (as on the device, where both kernels share rrx_rt_common.h);
what is stated here is the backward tracer's own: the sensors, the start, the walk to the sun, the deposits, and the event loop
with them (trace_counts_bw: the g-point form, the _bg and _aer forms, and with weight0 the rays of one g-point of the spectral
form, are calls of it). The walk to the sun is a loop of its own here (on the device it is a state of the event loop): per ray the
operations and their order are the same. Beside the counts it returns, per camera pixel, the number of deposits and their sum,
and the events and sun-walk cells of all rays.

A sensor is any object with type, npx, npy, fov, position, e_w, e_h, e_d (rte_rrtmgp_cpp_amd.camera.Camera, or Sensor below)."""
import math
from dataclasses import dataclass

import numpy as np

import raytracer_ref as R

TWO_PI = R.TWO_PI
PI = 3.141592653589793
D_MAX = 1048576.0


@dataclass
class Sensor:
    type: int
    npx: int
    npy: int
    fov: float
    position: tuple
    e_w: tuple
    e_h: tuple
    e_d: tuple


def orthographic(npx, npy, e_d):
    e_d = np.asarray(e_d, dtype=np.float64)
    return Sensor(2, npx, npy, 0.0, (0., 0., 0.), (1., 0., 0.), (0., 1., 0.), tuple(e_d / np.linalg.norm(e_d)))


def flux_sensor(npx, npy, up):
    return Sensor(3, npx, npy, 0.0, (0., 0., 0.), (1., 0., 0.), (0., 1., 0.), (0., 0., 1. if up else -1.))


def max_walk(scene):
    mu0 = float(scene.dtype.type(scene.mu0))
    tn = math.sqrt(max(0., 1. - mu0*mu0)) / mu0
    h = scene.nz * float(scene.dtype.type(scene.dz))
    return int(scene.nz + math.ceil(h*tn/float(scene.dtype.type(scene.dx))) + math.ceil(h*tn/float(scene.dtype.type(scene.dy))) + 2)


def trace_counts_bw(scene, sensor, igpt, ray0, nrays, max_events=1 << 20, ranges=1, table=None, bg=None, weight0=1):
    """The rays [ray0, ray0 + nrays) of g-point igpt (rrx_rt_bw_trace_counts and its _phase, _bg and _aer forms; with weight0, the
    rays of one g-point in rrx_camera_trace_counts_spectral). table: a raytracer_phase_ref.Table with cld_re for the cloud inside
    the grid; bg: a raytracer_ref.Background, None for a medium that ends at the domain top; weight0: a deposit d is tallied as
    to_count(min(d weight0, D_MAX)), in the scene's precision. Returns counts (npix,) uint64, n_capped, n_clamped, n_dep (npix,)
    and sum_d (npix,) float64, events, walk_cells, cloud_scatterings and aerosol_scatterings (all rays). ranges > 1: the rays are
    tallied as that many consecutive ranges of nrays/ranges rays each, counts, n_dep and sum_d are (ranges, npix) (integer adds:
    the same numbers as one call per range)."""
    s = scene
    dt = s.dtype
    F = dt.type
    nx, ny, nz = s.nx, s.ny, s.nz
    knx, kny, knz = s.kn_grid
    G = R.Grid(s, igpt, table)
    M = R.Medium(G, bg, igpt)
    dx, dy, dz, kdx, kdy, kdz = G.dx, G.dy, G.dz, G.kdx, G.kdy, G.kdz
    len_x, len_y, z_top, z_toa = G.len_x, G.len_y, G.z_top, M.z_toa
    inf = F(np.inf)
    one, zero, half, two = F(1.), F(0.), F(0.5), F(2.)
    pi = F(PI)
    mu0 = F(s.mu0)
    sun_x, sun_y, sun_z = R.sun_direction(s)
    vx, vy, vz = -sun_x, -sun_y, -sun_z
    with np.errstate(divide="ignore"):
        dtx = dx/abs(vx) if vx != 0 else inf
        dty = dy/abs(vy) if vy != 0 else inf
        dtz = dz/vz
    tau_bg_sun = M.tau_above[M.nbg]/mu0 if M.nbg else zero
    walk_bound = max_walk(s)
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
        """the distance along v to the next face of cell i; a negative one is 0"""
        if v > 0:
            return np.maximum(zero, ((i+1).astype(dt)*d - p)/v).astype(dt)
        if v < 0:
            return np.maximum(zero, (i.astype(dt)*d - p)/v).astype(dt)
        return np.full(p.size, inf, dtype=dt)

    def transmission(x, y, z, i, j, k):
        """exp(-(tau_walk + tau_bg_sun)) from (x, y, z) in cell (i, j, k) to TOA along -s: the walk to the domain top and the
        background's slant path in one exp; also whether the walk stayed within its bound"""
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
        """tallies min(d weight0, D_MAX) of the rays ok; the others are counted in n_capped"""
        d = d*F(weight0)
        clamped = ok & (d > F(D_MAX))
        tot["n_clamped"] += int(clamped.sum())
        pt.n_capped += int((~ok).sum())
        d = np.where(clamped, F(D_MAX), d)
        np.add.at(counts, sel_pix[ok], R.to_count(d[ok]))
        np.add.at(n_dep, sel_pix[ok], 1)
        np.add.at(sum_d, sel_pix[ok], d[ok].astype(np.float64))

    def deposit(sel_pix, dep, x, y, z, i, j, k):
        """scores dep T_sun; returns which rays stayed within the walk's bound"""
        if dep.size == 0:
            return np.ones(0, dtype=bool)
        tr, ok = transmission(x, y, z, i, j, k)
        score(sel_pix, (dep*tr).astype(dt), ok)
        return ok

    # ---- start: two draws (the place in the pixel), a flux sensor's lambert, and the move into the medium, whose top is TOA
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
            th, ph = (fa*fov)*half, F(TWO_PI)*fb
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

    def pixel_of(a):
        return PIX[a] + npix*(a // (N // ranges))

    def towards_the_sun(p, c, cloud, aerosol, species):
        """what a scattering sends towards the sun, before the lanes turn: w P(cos of the angle to the sun)/(4 pi)"""
        cs = np.clip(-((p.ux*sun_x + p.uy*sun_y) + p.uz*sun_z), -one, one).astype(dt)
        return ((p.w*R.sun_density(species, c.cell, cs, cloud, aerosol))/(F(4.)*pi)).astype(dt)

    def grid_event(a, p):
        pixel = pixel_of(a)
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
            sc, cloud, aerosol = R.collision_outcome(pt, a, p, h, c)
            if sc.any():
                dep = towards_the_sun(p, c, cloud, aerosol, G.species)
                hit = np.nonzero(sc)[0]
                ok = deposit(pixel[hit], dep[hit], p.x[hit], p.y[hit], p.z[hit], c.i[hit], c.j[hit], c.k[hit])
                p.alive[hit[~ok]] = False
                sc = sc & p.alive
                p.ux, p.uy, p.uz = R.scatter_direction(pt, a, sc, cloud, aerosol, G.species, c.cell, p.ux, p.uy, p.uz)
        R.through_the_top(M, p, top)

    def bg_event(a, q):
        R.cross_bg(M, pt, a, q, False)
        h = ~q.crossed
        if h.any():
            c = R.collide_bg(M, q, h, False)
            sc, cloud, aerosol = R.collision_outcome(pt, a, q, h, c)
            if sc.any():
                dep = towards_the_sun(q, c, cloud, aerosol, M.species)
                d = (dep*np.exp(-((c.k_ext*(q.z_hi - q.z) + M.tau_above[c.cell])/mu0))).astype(dt)
                hit = np.nonzero(sc)[0]
                score(pixel_of(a)[hit], d[hit], np.ones(hit.size, dtype=bool))
                q.ux, q.uy, q.uz = R.scatter_direction(pt, a, sc, cloud, aerosol, M.species, c.cell, q.ux, q.uy, q.uz)

    R.events(pt, max_events, knz, grid_event, bg_event)

    if ranges > 1:
        counts, n_dep, sum_d = counts.reshape(ranges, npix), n_dep.reshape(ranges, npix), sum_d.reshape(ranges, npix)
    return dict(counts=counts, n_dep=n_dep, sum_d=sum_d, n_capped=pt.n_capped, events=pt.events, cloud_scatterings=pt.cloud_scatterings,
                aerosol_scatterings=pt.aerosol_scatterings, **tot)


def raytracer_bw(scene, sensor, rays_per_pixel, max_events=1 << 20, bg=None):
    """The spectral loop of rrx_raytracer_bw and its _bg and _aer forms (without a table): radiance (npix,) in W m-2 sr-1,
    n_capped, n_clamped, and per g-point the number of deposits and their sum per pixel, the events and the sun-walk cells."""
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
        c = trace_counts_bw(s, sensor, g, 0, rays_per_pixel*npix, max_events, bg=bg)
        scale = F(s.inc_dir[g]) / (F(s.mu0)*F(rays_per_pixel))
        out["radiance"] = R.counts_to_flux(c["counts"], scale, out["radiance"])
        out["n_capped"] += c["n_capped"]; out["n_clamped"] += c["n_clamped"]
        out["n_dep"][g], out["sum_d"][g], out["events"][g], out["walk_cells"][g] = c["n_dep"], c["sum_d"], c["events"], c["walk_cells"]
    return out
