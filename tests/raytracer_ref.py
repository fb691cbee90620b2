"""numpy restatement of the forward Monte Carlo ray tracer (csrc/rrx_raytracer.hip): the same Philox stream, the same
draw order and the same arithmetic, operation for operation, vectorised over the photons (every pass of the loop is one event of
every photon still alive). Arrays are in the package's tensor convention: tau, ssa (ngpt, nz, ncol), the cloud triple
(nbnd, nz, ncol), sfc_albedo (ncol,), ncol = nx ny with x fastest; counts are uint64 in units of 2^-32 photon."""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from mcica_ref import philox4x32_10, uniform, band_of_gpt

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


def trace_counts(scene, igpt, photon0, nphotons, max_events=1 << 20):
    """The photons [photon0, photon0 + nphotons) of g-point igpt. Returns the six count arrays (abs_*: (nz, ncol)), n_capped and
    events (collisions + crossings of all photons)."""
    s = scene
    dt = s.dtype
    F = dt.type
    nx, ny, nz, ncol = s.nx, s.ny, s.nz, s.ncol
    knx, kny, knz = s.kn_grid
    rx, ry, rz = nx//knx, ny//kny, nz//knz
    dx, dy, dz = F(s.dx), F(s.dy), F(s.dz)
    kdx, kdy, kdz = F(rx)*dx, F(ry)*dy, F(rz)*dz
    ic = bool(s.independent_column)
    ib = band_of(s, igpt)
    tau_g, ssa_g = s.tau[igpt].reshape(-1), s.ssa[igpt].reshape(-1)            # cell = icol + ncol*lay
    if ib >= 0:
        ctau, cssa, cg = (c[ib].reshape(-1) for c in s.cloud)
    albedo = np.asarray(s.sfc_albedo, dtype=dt)
    kgrid = k_null(s, igpt)
    inf = F(np.inf)
    g_max = F(1.) - np.finfo(dt).eps
    one, zero, half = F(1.), F(0.), F(0.5)
    sun_x, sun_y, sun_z = sun_direction(s)
    dif_frac = F(s.inc_dif[igpt]) / (F(s.inc_dir[igpt]) + F(s.inc_dif[igpt]))
    key = (s.seed & 0xFFFFFFFF, (s.seed >> 32) & 0xFFFFFFFF)

    out = {k: np.zeros(ncol, dtype=np.uint64) for k in COUNT_NAMES[:4]}
    out.update({k: np.zeros(ncol*nz, dtype=np.uint64) for k in COUNT_NAMES[4:]})
    n_capped = 0
    events = 0

    N = int(nphotons)
    p = np.uint64(photon0) + np.arange(N, dtype=np.uint64)
    c0, c1 = p & np.uint64(0xFFFFFFFF), p >> np.uint64(32)
    nd = np.zeros(N, dtype=np.int64)

    def draw(sel):
        if sel.size == 0:
            return np.zeros(0, dtype=dt)
        w = philox4x32_10((c0[sel], c1[sel], np.full(sel.size, igpt, dtype=np.int64), nd[sel] >> 2), key)
        x = np.choose(nd[sel] & 3, w)
        nd[sel] += 1
        return uniform(x, dt)

    def lambert(sel, sign):
        mu = np.sqrt(draw(sel))
        phi = F(TWO_PI) * draw(sel)
        sn = np.sqrt(one - mu*mu)
        return sn*np.cos(phi), sn*np.sin(phi), sign*mu

    def fine(pos, d, blk, r):
        return np.clip((pos / d).astype(np.int64), blk*r, blk*r + r - 1)

    def add(name, idx, weight):
        np.add.at(out[name], idx, to_count(weight))

    def add_kind(names, kind, idx, weight):
        add(names[0], idx[kind == 0], weight[kind == 0])
        add(names[1], idx[kind == 1], weight[kind == 1])

    # ---- start
    everyone = np.arange(N)
    pix = (p % np.uint64(ncol)).astype(np.int64)
    ix, iy = pix % nx, pix // nx
    IN, JN, KN = ix // rx, iy // ry, np.full(N, knz-1, dtype=np.int64)
    X = np.clip((ix.astype(dt) + draw(everyone))*dx, IN.astype(dt)*kdx, (IN+1).astype(dt)*kdx)
    Y = np.clip((iy.astype(dt) + draw(everyone))*dy, JN.astype(dt)*kdy, (JN+1).astype(dt)*kdy)
    Z = np.full(N, F(knz)*kdz, dtype=dt)
    KIND = (draw(everyone) < dif_frac).astype(np.int64)
    UX, UY, UZ = np.full(N, sun_x, dtype=dt), np.full(N, sun_y, dtype=dt), np.full(N, sun_z, dtype=dt)
    d = np.nonzero(KIND == 1)[0]
    UX[d], UY[d], UZ[d] = lambert(d, F(-1.))
    W = np.ones(N, dtype=dt)
    T = np.zeros(N, dtype=dt)
    PEND = np.zeros(N, dtype=bool)
    ALIVE = np.ones(N, dtype=bool)
    NEV = np.zeros(N, dtype=np.int64)

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        while ALIVE.any():
            a = np.nonzero(ALIVE)[0]
            capped = NEV[a] >= max_events
            n_capped += int(capped.sum())
            ALIVE[a[capped]] = False
            a = a[~capped]
            if a.size == 0:
                continue
            NEV[a] += 1
            events += a.size
            x, y, z, ux, uy, uz, w, kind = X[a], Y[a], Z[a], UX[a], UY[a], UZ[a], W[a], KIND[a]
            i_n, j_n, k_n = IN[a], JN[a], KN[a]
            alive = np.ones(a.size, dtype=bool)
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
            n_capped += int(lost.sum())
            alive[lost] = False
            c = cross & ~lost
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
            pixel = fine(x, dx, i_n, rx) + nx*fine(y, dy, j_n, ry)
            add("tod_up", pixel[top], w[top])
            alive[top] = False
            if sfc.any():
                z = np.where(sfc, zero, z)
                add_kind(("sfc_dn_dir", "sfc_dn_dif"), kind[sfc], pixel[sfc], w[sfc])
                w = np.where(sfc, w*albedo[pixel], w)
                add("sfc_up", pixel[sfc], w[sfc])
                r = sfc & (w < half)
                u = draw(a[r])
                w[r] = np.where(u > w[r], zero, one)
                live = sfc & (w > zero)
                ux[live], uy[live], uz[live] = lambert(a[live], one)
                kind[live] = 1
                pend[live] = False
                alive[sfc & ~live] = False

            # ---- collisions
            h = ~cross
            if h.any():
                dn_ = tau / kn_val
                if not ic:
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
                add_kind(("abs_dir", "abs_dif"), kind[h], cell[h], (w*(one - f_no_abs))[h])
                w = np.where(h, w*f_no_abs, w)
                r = h & (w < half)
                u = draw(a[r])
                w[r] = np.where(u > w[r], zero, one)
                live = h & (w > zero)
                alive[h & ~live] = False
                u = np.zeros(a.size, dtype=dt); u[live] = draw(a[live])
                sc = live & (u*(k_sca + (kn_val - k_ext)) < k_sca)
                if sc.any():
                    u = np.zeros(a.size, dtype=dt); u[sc] = draw(a[sc])
                    cloud = sc & (u*k_sca < k_sca_cld)
                    u = np.full(a.size, half, dtype=dt); u[sc] = draw(a[sc])
                    g = np.minimum(gc, g_max)
                    iso = np.abs(g) < F(1.e-6)
                    gs = np.where(iso, half, g)
                    sh = (one - gs*gs) / ((one - gs) + (F(2.)*gs)*u)
                    cos_hg = np.where(iso, F(2.)*u - one, ((one + gs*gs) - sh*sh) / (F(2.)*gs))
                    q = F(4.)*u - F(2.)
                    A = np.cbrt(q + np.sqrt(one + q*q))
                    cos_ray = A - one/A
                    cos_s = np.clip(np.where(cloud, cos_hg, cos_ray), F(-1.), one).astype(dt)
                    sin_s = np.sqrt(np.maximum(zero, one - cos_s*cos_s))
                    phi = np.zeros(a.size, dtype=dt); phi[sc] = F(TWO_PI) * draw(a[sc])
                    cp, sp = np.cos(phi), np.sin(phi)
                    vert = np.abs(uz) > F(0.99999)
                    den = np.sqrt(np.where(vert, one, one - uz*uz))
                    vx = np.where(vert, sin_s*cp, (sin_s*((ux*uz)*cp - uy*sp))/den + ux*cos_s)
                    vy = np.where(vert, sin_s*sp, (sin_s*((uy*uz)*cp + ux*sp))/den + uy*cos_s)
                    vz = np.where(vert, np.where(uz > zero, cos_s, -cos_s), uz*cos_s - (sin_s*cp)*den)
                    nrm = np.sqrt((vx*vx + vy*vy) + vz*vz)
                    ux = np.where(sc, vx/nrm, ux).astype(dt); uy = np.where(sc, vy/nrm, uy).astype(dt); uz = np.where(sc, vz/nrm, uz).astype(dt)
                    kind = np.where(sc, 1, kind)

            X[a], Y[a], Z[a], UX[a], UY[a], UZ[a], W[a], KIND[a], T[a] = x, y, z, ux, uy, uz, w, kind, tau
            IN[a], JN[a], KN[a], PEND[a], ALIVE[a] = i_n, j_n, k_n, pend, alive

    res = {k: v for k, v in out.items()}
    res["abs_dir"] = res["abs_dir"].reshape(nz, ncol)
    res["abs_dif"] = res["abs_dif"].reshape(nz, ncol)
    res["n_capped"] = n_capped
    res["events"] = events
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
