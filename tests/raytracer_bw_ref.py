"""numpy restatement of the backward Monte Carlo ray tracer (csrc/rrx_raytracer_bw.hip): the same Philox stream
(counter word 2 is igpt | 0x80000000), the same draw order and the same arithmetic, operation for operation, vectorised over the
rays. It reuses raytracer_ref (Scene, k_null, the sun's direction, to_count). The walk to the sun is a loop of its own here (on the
device it is a state of the event loop): per ray the operations and their order are the same. Beside the counts it returns, per
camera pixel, the number of deposits and their sum, and the events and sun-walk cells of all rays.

A sensor is any object with type, npx, npy, fov, position, e_w, e_h, e_d (rte_rrtmgp_cpp_amd.camera.Camera, or Sensor below)."""
import math
from dataclasses import dataclass

import numpy as np

from mcica_ref import philox4x32_10, uniform
import raytracer_ref as R

TWO_PI = 6.283185307179586
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


def trace_counts(scene, sensor, igpt, ray0, nrays, max_events=1 << 20, ranges=1):
    """The rays [ray0, ray0 + nrays) of g-point igpt. Returns counts (npix,) uint64, n_capped, n_clamped, n_dep (npix,) and
    sum_d (npix,) float64, events and walk_cells (all rays). ranges > 1: the rays are tallied as that many consecutive ranges of
    nrays/ranges rays each, counts, n_dep and sum_d are (ranges, npix) (integer adds: the same numbers as one call per range)."""
    s = scene
    dt = s.dtype
    F = dt.type
    nx, ny, nz, ncol = s.nx, s.ny, s.nz, s.ncol
    knx, kny, knz = s.kn_grid
    rx, ry, rz = nx//knx, ny//kny, nz//knz
    dx, dy, dz = F(s.dx), F(s.dy), F(s.dz)
    kdx, kdy, kdz = F(rx)*dx, F(ry)*dy, F(rz)*dz
    len_x, len_y, z_top = F(knx)*kdx, F(kny)*kdy, F(knz)*kdz
    ib = R.band_of(s, igpt)
    tau_g, ssa_g = s.tau[igpt].reshape(-1), s.ssa[igpt].reshape(-1)
    if ib >= 0:
        ctau, cssa, cg = (c[ib].reshape(-1) for c in s.cloud)
    albedo = np.asarray(s.sfc_albedo, dtype=dt)
    kgrid = R.k_null(s, igpt)
    inf = F(np.inf)
    g_max = F(1.) - np.finfo(dt).eps
    one, zero, half, two = F(1.), F(0.), F(0.5), F(2.)
    pi = F(PI)
    mu0 = F(s.mu0)
    sun_x, sun_y, sun_z = R.sun_direction(s)
    vx, vy, vz = -sun_x, -sun_y, -sun_z
    with np.errstate(divide="ignore"):
        dtx = dx/abs(vx) if vx != 0 else inf
        dty = dy/abs(vy) if vy != 0 else inf
        dtz = dz/vz
    walk_bound = max_walk(s)
    key = (s.seed & 0xFFFFFFFF, (s.seed >> 32) & 0xFFFFFFFF)
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
    tot = dict(n_capped=0, n_clamped=0, events=0, walk_cells=0)

    N = int(nrays)
    r = np.uint64(ray0) + np.arange(N, dtype=np.uint64)
    c0, c1 = r & np.uint64(0xFFFFFFFF), r >> np.uint64(32)
    c2 = int(igpt) | 0x80000000
    nd = np.zeros(N, dtype=np.int64)

    def draw(sel):
        if sel.size == 0:
            return np.zeros(0, dtype=dt)
        w = philox4x32_10((c0[sel], c1[sel], np.full(sel.size, c2, dtype=np.int64), nd[sel] >> 2), key)
        x = np.choose(nd[sel] & 3, w)
        nd[sel] += 1
        return uniform(x, dt)

    def lambert(sel, sign):
        mu = np.sqrt(draw(sel))
        phi = F(TWO_PI) * draw(sel)
        sn = np.sqrt(one - mu*mu)
        return sn*np.cos(phi), sn*np.sin(phi), sign*mu

    def fine(p, d, blk, rr):
        return np.clip((p / d).astype(np.int64), blk*rr, blk*rr + rr - 1)

    def first(v, p, i, d):
        """the distance along v to the next face of cell i; a negative one is 0"""
        if v > 0:
            return np.maximum(zero, ((i+1).astype(dt)*d - p)/v).astype(dt)
        if v < 0:
            return np.maximum(zero, (i.astype(dt)*d - p)/v).astype(dt)
        return np.full(p.size, inf, dtype=dt)

    def transmission(x, y, z, i, j, k):
        """exp(-tau_sun) from (x, y, z) in cell (i, j, k) to the top along -s; also whether the walk stayed within its bound"""
        n = x.size
        i, j, k = i.copy(), j.copy(), k.copy()
        tx, ty, tz = first(vx, x, i, dx), first(vy, y, j, dy), first(vz, z, k, dz)
        t, tsun = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
        steps = np.zeros(n, dtype=np.int64)
        ok = np.ones(n, dtype=bool)
        go = np.arange(n)
        while go.size:
            ii, jj, kk = i[go], j[go], k[go]
            tn = np.minimum(tz[go], np.minimum(tx[go], ty[go]))
            axis = np.where((tz[go] <= tx[go]) & (tz[go] <= ty[go]), 2, np.where(tx[go] <= ty[go], 0, 1))
            lay = nz - 1 - kk if s.top_at_1 else kk
            cell = ii + jj*nx + ncol*lay
            tc = ctau[cell] if ib >= 0 else np.zeros(go.size, dtype=dt)
            tsun[go] = tsun[go] + ((tau_g[cell] + tc) / dz)*(tn - t[go])
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
        return np.exp(-tsun), ok

    def deposit(sel_pix, dep, x, y, z, i, j, k):
        """tallies dep T_sun; returns which rays stayed within the walk's bound"""
        if dep.size == 0:
            return np.ones(0, dtype=bool)
        tr, ok = transmission(x, y, z, i, j, k)
        d = (dep*tr).astype(dt)
        clamped = ok & (d > F(D_MAX))
        tot["n_clamped"] += int(clamped.sum())
        tot["n_capped"] += int((~ok).sum())
        d = np.where(clamped, F(D_MAX), d)
        np.add.at(counts, sel_pix[ok], R.to_count(d[ok]))
        np.add.at(n_dep, sel_pix[ok], 1)
        np.add.at(sum_d, sel_pix[ok], d[ok].astype(np.float64))
        return ok

    # ---- start
    everyone = np.arange(N)
    PIX = (r % np.uint64(npix)).astype(np.int64)
    ipx, ipy = PIX % npx, PIX // npx
    fa = (ipx.astype(dt) + draw(everyone)) / F(npx)
    fb = (ipy.astype(dt) + draw(everyone)) / F(npy)
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
            UX, UY, UZ = lambert(everyone, one)
            SZ = np.zeros(N, dtype=dt)
        else:
            UX, UY, UZ = lambert(everyone, -one)
            SZ = np.full(N, z_top, dtype=dt)
    ALIVE = np.ones(N, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        above = SZ >= z_top
        ALIVE[above & ~(UZ < zero)] = False
        mv = above & (UZ < zero) & (SZ > z_top)
        tmv = np.where(mv, (z_top - SZ)/np.where(mv, UZ, one), zero).astype(dt)
        SX = np.where(mv, SX + UX*tmv, SX).astype(dt); SY = np.where(mv, SY + UY*tmv, SY).astype(dt)
        SZ = np.where(above, z_top, SZ).astype(dt)
        SX = (SX - np.floor(SX/len_x)*len_x).astype(dt); SY = (SY - np.floor(SY/len_y)*len_y).astype(dt)
        IN = np.clip((SX/kdx).astype(np.int64), 0, knx-1); JN = np.clip((SY/kdy).astype(np.int64), 0, kny-1)
        KN = np.clip((SZ/kdz).astype(np.int64), 0, knz-1)
        X = np.clip(SX, IN.astype(dt)*kdx, (IN+1).astype(dt)*kdx)
        Y = np.clip(SY, JN.astype(dt)*kdy, (JN+1).astype(dt)*kdy)
        Z = np.clip(SZ, KN.astype(dt)*kdz, (KN+1).astype(dt)*kdz)
    W = np.ones(N, dtype=dt)
    T = np.zeros(N, dtype=dt)
    PEND = np.zeros(N, dtype=bool)
    NEV = np.zeros(N, dtype=np.int64)

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        while ALIVE.any():
            a = np.nonzero(ALIVE)[0]
            capped = NEV[a] >= max_events
            tot["n_capped"] += int(capped.sum())
            ALIVE[a[capped]] = False
            a = a[~capped]
            if a.size == 0:
                continue
            NEV[a] += 1
            tot["events"] += a.size
            x, y, z, ux, uy, uz, w = X[a], Y[a], Z[a], UX[a], UY[a], UZ[a], W[a]
            i_n, j_n, k_n = IN[a], JN[a], KN[a]
            pixel = PIX[a] + npix*(a // (N // ranges))
            alive = np.ones(a.size, dtype=bool)
            x_lo, x_hi = i_n.astype(dt)*kdx, (i_n+1).astype(dt)*kdx
            y_lo, y_hi = j_n.astype(dt)*kdy, (j_n+1).astype(dt)*kdy
            z_lo, z_hi = k_n.astype(dt)*kdz, (k_n+1).astype(dt)*kdz

            def dist(p, u, lo, hi):
                return np.where(u > zero, (hi - p)/u, np.where(u < zero, (lo - p)/u, inf)).astype(dt)
            sz, sx, sy = dist(z, uz, z_lo, z_hi), dist(x, ux, x_lo, x_hi), dist(y, uy, y_lo, y_hi)
            d_max = np.minimum(sz, np.minimum(sx, sy))
            axis = np.where((sz <= sx) & (sz <= sy), 2, np.where(sx <= sy, 0, 1))
            kn_val = kgrid[k_n, j_n, i_n]
            tau = T[a]
            fresh = ~PEND[a]
            tau[fresh] = -np.log(draw(a[fresh]))
            pend = np.zeros(a.size, dtype=bool)
            empty = ~(kn_val > zero)
            tau_cell = np.where(empty, zero, d_max*kn_val).astype(dt)
            cross = empty | (tau >= tau_cell)

            # ---- crossings
            lost = cross & ~(d_max < inf)
            tot["n_capped"] += int(lost.sum())
            alive[lost] = False
            c = cross & ~lost
            tau = np.where(c, tau - tau_cell, tau)
            pend[c] = True
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
            alive[top] = False
            if sfc.any():
                z = np.where(sfc, zero, z)
                i, j = fine(x, dx, i_n, rx), fine(y, dy, j_n, ry)
                w = np.where(sfc, w*albedo[i + nx*j], w)
                dep = ((w*mu0)/pi).astype(dt)
                hit = np.nonzero(sfc & (dep > zero))[0]
                ok = deposit(pixel[hit], dep[hit], x[hit], y[hit], z[hit], i[hit], j[hit], np.zeros(hit.size, dtype=np.int64))
                alive[hit[~ok]] = False
                go = sfc & alive
                rr = go & (w < half)
                u = draw(a[rr])
                w[rr] = np.where(u > w[rr], zero, one)
                live = go & (w > zero)
                ux[live], uy[live], uz[live] = lambert(a[live], one)
                pend[go] = False
                alive[go & ~live] = False

            # ---- collisions
            h = ~cross
            if h.any():
                dn_ = tau / kn_val
                x = np.where(h, np.clip(x + ux*dn_, x_lo, x_hi), x)
                y = np.where(h, np.clip(y + uy*dn_, y_lo, y_hi), y)
                z = np.where(h, np.clip(z + uz*dn_, z_lo, z_hi), z)
                i, j, k = fine(x, dx, i_n, rx), fine(y, dy, j_n, ry), fine(z, dz, k_n, rz)
                lay = nz - 1 - k if s.top_at_1 else k
                cell = i + j*nx + ncol*lay
                t, w0 = tau_g[cell], ssa_g[cell]
                if ib >= 0:
                    tc, wc, gc = ctau[cell], cssa[cell], cg[cell]
                else:
                    tc = wc = gc = np.zeros(a.size, dtype=dt)
                k_ext = (t + tc) / dz
                k_sca = (t*w0 + tc*wc) / dz
                k_sca_cld = (tc*wc) / dz
                f_no_abs = np.clip(one - (k_ext - k_sca)/kn_val, zero, one)
                w = np.where(h, w*f_no_abs, w)
                rr = h & (w < half)
                u = draw(a[rr])
                w[rr] = np.where(u > w[rr], zero, one)
                live = h & (w > zero)
                alive[h & ~live] = False
                u = np.zeros(a.size, dtype=dt); u[live] = draw(a[live])
                sc = live & (u*(k_sca + (kn_val - k_ext)) < k_sca)
                if sc.any():
                    u = np.zeros(a.size, dtype=dt); u[sc] = draw(a[sc])
                    cloud = sc & (u*k_sca < k_sca_cld)
                    g = np.minimum(gc, g_max)
                    cs = np.clip(-((ux*sun_x + uy*sun_y) + uz*sun_z), -one, one).astype(dt)
                    qq = (one + g*g) - (two*g)*cs
                    p_hg = (one - g*g) / (qq*np.sqrt(qq))
                    p_ray = F(0.75)*(one + cs*cs)
                    dep = ((w*np.where(cloud, p_hg, p_ray))/(F(4.)*pi)).astype(dt)
                    hit = np.nonzero(sc)[0]
                    ok = deposit(pixel[hit], dep[hit], x[hit], y[hit], z[hit], i[hit], j[hit], k[hit])
                    alive[hit[~ok]] = False
                    sc = sc & alive
                    u = np.full(a.size, half, dtype=dt); u[sc] = draw(a[sc])
                    iso = np.abs(g) < F(1.e-6)
                    gs = np.where(iso, half, g)
                    sh = (one - gs*gs) / ((one - gs) + (two*gs)*u)
                    cos_hg = np.where(iso, two*u - one, ((one + gs*gs) - sh*sh) / (two*gs))
                    q = F(4.)*u - two
                    A = np.cbrt(q + np.sqrt(one + q*q))
                    cos_ray = A - one/A
                    cos_s = np.clip(np.where(cloud, cos_hg, cos_ray), -one, one).astype(dt)
                    sin_s = np.sqrt(np.maximum(zero, one - cos_s*cos_s))
                    phi = np.zeros(a.size, dtype=dt); phi[sc] = F(TWO_PI) * draw(a[sc])
                    cp, sp = np.cos(phi), np.sin(phi)
                    vert = np.abs(uz) > F(0.99999)
                    den = np.sqrt(np.where(vert, one, one - uz*uz))
                    wx = np.where(vert, sin_s*cp, (sin_s*((ux*uz)*cp - uy*sp))/den + ux*cos_s)
                    wy = np.where(vert, sin_s*sp, (sin_s*((uy*uz)*cp + ux*sp))/den + uy*cos_s)
                    wz = np.where(vert, np.where(uz > zero, cos_s, -cos_s), uz*cos_s - (sin_s*cp)*den)
                    nrm = np.sqrt((wx*wx + wy*wy) + wz*wz)
                    ux = np.where(sc, wx/nrm, ux).astype(dt); uy = np.where(sc, wy/nrm, uy).astype(dt); uz = np.where(sc, wz/nrm, uz).astype(dt)

            X[a], Y[a], Z[a], UX[a], UY[a], UZ[a], W[a], T[a] = x, y, z, ux, uy, uz, w, tau
            IN[a], JN[a], KN[a], PEND[a], ALIVE[a] = i_n, j_n, k_n, pend, alive

    if ranges > 1:
        counts, n_dep, sum_d = counts.reshape(ranges, npix), n_dep.reshape(ranges, npix), sum_d.reshape(ranges, npix)
    return dict(counts=counts, n_dep=n_dep, sum_d=sum_d, **tot)


def raytracer_bw(scene, sensor, rays_per_pixel, max_events=1 << 20):
    """The spectral loop of rrx_raytracer_bw: radiance (npix,) in W m-2 sr-1, n_capped, n_clamped, and per g-point the number of
    deposits and their sum per pixel, the events and the sun-walk cells."""
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
        c = trace_counts(s, sensor, g, 0, rays_per_pixel*npix, max_events)
        scale = F(s.inc_dir[g]) / (F(s.mu0)*F(rays_per_pixel))
        out["radiance"] = R.counts_to_flux(c["counts"], scale, out["radiance"])
        out["n_capped"] += c["n_capped"]; out["n_clamped"] += c["n_clamped"]
        out["n_dep"][g], out["sum_d"][g], out["events"][g], out["walk_cells"][g] = c["n_dep"], c["sum_d"], c["events"], c["walk_cells"]
    return out
