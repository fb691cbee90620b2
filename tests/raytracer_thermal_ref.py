"""numpy restatement of the backward Monte Carlo ray tracer with thermal emission (csrc/rrx_raytracer_thermal.hip):
the same Philox stream (counter word 2 is igpt | 0xC0000000), the same draw order and the same arithmetic, operation for operation,
vectorised over the rays. The medium and the transport steps are those of raytracer_ref, imported unchanged (Grid, Particles, cross,
collide, roulette, collision_outcome, scatter_direction, lambert); what is stated here is this tracer's own: the scene with its
sources, the sensor start (that of raytracer_bw_ref without a background), the three deposits and the event loop with them.

A ThermalScene holds the medium as a raytracer_ref.Scene (tau, ssa (ngpt, nz, ncol): ssa zeros restate the device's NULL ssa bit for
bit, t 0 + tc wc = tc wc; the cloud triple; kn_grid; top_at_1; seed; its sfc_albedo, sun and incident fluxes are not read) and the
sources, radiances in W m-2 sr-1: lay_src (ngpt, nz, ncol), sfc_src (ngpt, ncol), sfc_emis (ncol,), top_radiance (ngpt,).
A sensor is any object with type, npx, npy, fov, position, e_w, e_h, e_d."""
from dataclasses import dataclass

import numpy as np

import raytracer_ref as R

TWO_PI = R.TWO_PI
D_MAX = 1048576.0
C2_THERMAL = 0xC0000000


@dataclass
class ThermalScene:
    medium: R.Scene
    lay_src: np.ndarray
    sfc_src: np.ndarray
    sfc_emis: np.ndarray
    top_radiance: np.ndarray

    def __getattr__(self, name):          # nx, ny, nz, dx, dy, dz, tau, ssa, cloud, band_lims, kn_grid, top_at_1, seed, ncol, dtype
        if name == "medium":
            raise AttributeError(name)
        return getattr(self.medium, name)


def trace_counts_thermal(scene, sensor, igpt, ray0, nrays, max_events=1 << 20, ranges=1):
    """The rays [ray0, ray0 + nrays) of g-point igpt (rrx_thermal_trace_counts). Returns counts (npix,) uint64, n_capped, n_clamped,
    n_dep (npix,), the number of deposits d > 0 (a deposit of 0 adds nothing on either side), and sum_d (npix,) float64, their sum,
    events (collisions + crossings of all rays) and deposits (all rays, zeros included). ranges > 1: the rays are tallied as that
    many consecutive ranges of nrays/ranges rays each, counts, n_dep and sum_d are (ranges, npix) (integer adds: the same numbers
    as one call per range)."""
    s = scene.medium
    dt = s.dtype
    F = dt.type
    nx = s.nx
    knx, kny, knz = s.kn_grid
    G = R.Grid(s, igpt)
    dx, dy, kdx, kdy, kdz = G.dx, G.dy, G.kdx, G.kdy, G.kdz
    len_x, len_y, z_top = G.len_x, G.len_y, G.z_top
    one, zero, half, two = F(1.), F(0.), F(0.5), F(2.)
    lay_src = np.asarray(scene.lay_src[igpt], dtype=dt).reshape(-1)
    sfc_src = np.asarray(scene.sfc_src[igpt], dtype=dt).reshape(-1)
    emis = np.asarray(scene.sfc_emis, dtype=dt).reshape(-1)
    top_radiance = F(scene.top_radiance[igpt])
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
    tot = dict(n_clamped=0, deposits=0)

    N = int(nrays)
    pt = R.Particles(ray0, N, int(igpt) | C2_THERMAL, s.seed, dt)
    PIX = (pt.index % np.uint64(npix)).astype(np.int64)

    def pixel_of(a):
        return PIX[a] + npix*(a // (N // ranges))

    def score(sel_pix, d):
        """tallies min(d, D_MAX)"""
        d = d.astype(dt)
        clamped = d > F(D_MAX)
        tot["n_clamped"] += int(clamped.sum())
        tot["deposits"] += d.size
        d = np.where(clamped, F(D_MAX), d)
        np.add.at(counts, sel_pix, R.to_count(d))
        np.add.at(n_dep, sel_pix, (d > zero).astype(np.int64))
        np.add.at(sum_d, sel_pix, d.astype(np.float64))

    # ---- start: two draws (the place in the pixel), a flux sensor's lambert, and the move to the domain top
    everyone = np.arange(N)
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
            SZ = np.full(N, z_top, dtype=dt)
        elif ed[2] > 0:
            UX, UY, UZ = R.lambert(pt, everyone, one)
            SZ = np.zeros(N, dtype=dt)
        else:
            UX, UY, UZ = R.lambert(pt, everyone, -one)
            SZ = np.full(N, z_top, dtype=dt)
    ALIVE = np.ones(N, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        above = SZ >= z_top
        away = above & ~(UZ < zero)          # the ray ends at the top, with what comes down through it (its weight is 1)
        ALIVE[away] = False
        score(pixel_of(everyone[away]), np.full(int(away.sum()), top_radiance, dtype=dt))
        mv = above & (UZ < zero) & (SZ > z_top)
        tmv = np.where(mv, (z_top - SZ)/np.where(mv, UZ, one), zero).astype(dt)
        SX = np.where(mv, SX + UX*tmv, SX).astype(dt); SY = np.where(mv, SY + UY*tmv, SY).astype(dt)
        SZ = np.where(above, z_top, SZ).astype(dt)
        WX = (SX - np.floor(SX/len_x)*len_x).astype(dt); WY = (SY - np.floor(SY/len_y)*len_y).astype(dt)
        IN = np.clip((WX/kdx).astype(np.int64), 0, knx-1); JN = np.clip((WY/kdy).astype(np.int64), 0, kny-1)
        KN = np.clip((SZ/kdz).astype(np.int64), 0, knz-1)
        X = np.clip(WX, IN.astype(dt)*kdx, (IN+1).astype(dt)*kdx)
        Y = np.clip(WY, JN.astype(dt)*kdy, (JN+1).astype(dt)*kdy)
        Z = np.clip(SZ, KN.astype(dt)*kdz, (KN+1).astype(dt)*kdz)
    pt.start(X, Y, Z, UX, UY, UZ, IN, JN, KN, ALIVE)

    # ---- the event loop: every pass is one event of every ray still alive
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a, p in pt.passes(max_events):
            pixel = pixel_of(a)
            top, sfc = R.cross(G, pt, a, p)
            if top.any():
                score(pixel[top], p.w[top]*top_radiance)
            if sfc.any():
                p.z = np.where(sfc, zero, p.z)
                col = R.fine_cell(p.x, dx, p.i_n, G.rx) + nx*R.fine_cell(p.y, dy, p.j_n, G.ry)
                score(pixel[sfc], ((p.w*emis[col])*sfc_src[col])[sfc])
                p.w = np.where(sfc, p.w*(one - emis[col]), p.w)
                R.roulette(pt, a, p.w, sfc)
                live = sfc & (p.w > zero)
                p.ux[live], p.uy[live], p.uz[live] = R.lambert(pt, a[live], one)
                p.pend[live] = False
                p.alive[sfc & ~live] = False
            h = ~p.crossed
            if h.any():
                c = R.collide(G, p, h)
                score(pixel[h], ((p.w*(one - c.f_no_abs))*lay_src[c.cell])[h])
                sc, cloud, aerosol = R.collision_outcome(pt, a, p, h, c)
                if sc.any():
                    p.ux, p.uy, p.uz = R.scatter_direction(pt, a, sc, cloud, aerosol, G.species, c.cell, p.ux, p.uy, p.uz)

    if ranges > 1:
        counts, n_dep, sum_d = counts.reshape(ranges, npix), n_dep.reshape(ranges, npix), sum_d.reshape(ranges, npix)
    return dict(counts=counts, n_dep=n_dep, sum_d=sum_d, n_capped=pt.n_capped, events=pt.events, cloud_scatterings=pt.cloud_scatterings,
                **tot)


def render(scene, sensor, rays_per_pixel, max_events=1 << 20):
    """The loop of rrx_thermal_render: radiance (npix,) in W m-2 sr-1 and radiance_gpt (ngpt, npix), n_capped, n_clamped, and per
    g-point the number of deposits and their sum per pixel, the events and the deposits of all rays."""
    dt = scene.dtype
    F = dt.type
    ngpt = scene.tau.shape[0]
    npix = int(sensor.npx)*int(sensor.npy)
    out = dict(radiance=np.zeros(npix, dtype=dt), radiance_gpt=np.zeros((ngpt, npix), dtype=dt), n_capped=0, n_clamped=0,
               n_dep=np.zeros((ngpt, npix), dtype=np.int64), sum_d=np.zeros((ngpt, npix)), events=np.zeros(ngpt, dtype=np.int64),
               deposits=np.zeros(ngpt, dtype=np.int64))
    for g in range(ngpt):
        c = trace_counts_thermal(scene, sensor, g, 0, rays_per_pixel*npix, max_events)
        scale = F(1.)/F(rays_per_pixel)
        out["radiance"] = R.counts_to_flux(c["counts"], scale, out["radiance"])
        out["radiance_gpt"][g] = R.counts_to_flux(c["counts"], scale, out["radiance_gpt"][g])
        out["n_capped"] += c["n_capped"]; out["n_clamped"] += c["n_clamped"]
        out["n_dep"][g], out["sum_d"][g], out["events"][g], out["deposits"][g] = c["n_dep"], c["sum_d"], c["events"], c["deposits"]
    return out
