"""numpy restatement of the tabulated cloud phase functions of the ray tracers (csrc/rrx_rt_phase.h, rrx_rt_phase.hip):
the table builder, the index, the sampler and the evaluator in the entry's precision, operation for operation, their longdouble
counterparts (the exact inverse and the exact density of the table that is stored), and the event loops of raytracer_ref.py and
raytracer_bw_ref.py with the table in place of Henyey-Greenstein for the cloud species (the loops there compute the cosine inline,
so they are restated here; everything else is imported). Tables are in the package's tensor convention: phase, cdf (nbnd, nre, nmu)."""
from dataclasses import dataclass

import numpy as np

import raytracer_ref as R
from raytracer_ref import COUNT_NAMES, TWO_PI, band_of, k_null, sun_direction, to_count
from raytracer_bw_ref import PI, D_MAX, max_walk
from mcica_ref import philox4x32_10, uniform

LD = np.longdouble


@dataclass
class Table:
    mu: np.ndarray          # (nmu,)
    phase: np.ndarray       # (nbnd, nre, nmu)
    cdf: np.ndarray
    re0: float
    dre: float
    cld_re: np.ndarray = None          # (nz, ncol)

    @property
    def nre(self):
        return self.phase.shape[1]


def nodes(nmu, power=2.0):
    x = np.linspace(0.0, 1.0, nmu)
    mu = 1.0 - 2.0*(1.0 - x)**power
    mu[0], mu[-1] = -1.0, 1.0
    return mu


def hg(mu, g):
    return (1.0 - g*g) / (1.0 + g*g - 2.0*g*np.asarray(mu, dtype=np.float64))**1.5


def double_hg(mu, g1, g2, share):
    return share*hg(mu, g1) + (1.0 - share)*hg(mu, g2)


def hg_cdf(mu, g):
    """1/2 int_{-1}^{mu} HG dmu', analytic"""
    mu = np.asarray(mu, dtype=np.float64)
    return (1.0 - g*g)/(2.0*g) * (1.0/np.sqrt(1.0 + g*g - 2.0*g*mu) - 1.0/(1.0 + g))


def build_tables(mu, phase_raw, dtype, re0=2.5, dre=1.0):
    """rrx_rt_phase_tables: the inputs are rounded to dtype as the device sees them; the trapezoid sums run in double in node order
    (np.cumsum adds sequentially), cdf = F(A_i/A_last), phase = F(raw/(A_last/2))."""
    mu = np.asarray(mu).astype(dtype)
    raw = np.asarray(phase_raw).astype(dtype)
    m, r = mu.astype(np.float64), raw.astype(np.float64)
    seg = (0.5*(r[..., :-1] + r[..., 1:]))*(m[1:] - m[:-1])
    A = np.cumsum(seg, axis=-1)
    total = A[..., -1:]
    cdf = np.concatenate([np.zeros_like(total), A/total], axis=-1).astype(dtype)
    phase = (r/(0.5*total)).astype(dtype)
    return Table(mu=mu, phase=np.ascontiguousarray(phase), cdf=np.ascontiguousarray(cdf), re0=re0, dre=dre)


def index(t, re):
    """(ire, jre, f) of phase_index, in the dtype of re"""
    dt = re.dtype
    F = dt.type
    if t.nre == 1:
        z = np.zeros(re.shape, dtype=np.int64)
        return z, z, np.zeros(re.shape, dtype=dt)
    with np.errstate(invalid="ignore"):
        q = (re - F(t.re0)) / F(t.dre)
        ire = np.fmin(np.fmax(q, F(0.)), F(t.nre - 2)).astype(np.int64)
        f = np.fmin(np.fmax(q - ire.astype(dt), F(0.)), F(1.))
    return ire, ire + 1, f


def sample(t, ibnd, re, u, with_interval=False):
    """phase_sample in the dtype of the table"""
    dt = t.mu.dtype
    F = dt.type
    re, u = np.asarray(re, dtype=dt), np.asarray(u, dtype=dt)
    C, P, mu = t.cdf[ibnd], t.phase[ibnd], t.mu
    ire, jre, f = index(t, re)
    lo = np.zeros(u.shape, dtype=np.int64)
    hi = np.full(u.shape, mu.size - 1, dtype=np.int64)
    while np.any(hi - lo > 1):
        act = hi - lo > 1
        mid = (lo + hi) >> 1
        a, b = C[ire, mid], C[jre, mid]
        le = (a + f*(b - a)) <= u
        lo = np.where(act & le, mid, lo)
        hi = np.where(act & ~le, mid, hi)
    ca, cb = C[ire, lo], C[jre, lo]
    c = ca + f*(cb - ca)
    pa0, pb0, pa1, pb1 = P[ire, lo], P[jre, lo], P[ire, lo+1], P[jre, lo+1]
    p0, p1 = pa0 + f*(pb0 - pa0), pa1 + f*(pb1 - pa1)
    m0, m1 = mu[lo], mu[lo+1]
    r = F(2.)*(u - c)
    s = (p1 - p0) / (m1 - m0)
    den = p0 + np.sqrt(np.maximum(F(0.), p0*p0 + (F(2.)*s)*r))
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = np.where(den > F(0.), (F(2.)*r)/den, F(0.)).astype(dt)
    out = np.minimum(np.maximum(m0 + tt, m0), m1).astype(dt)
    return (out, lo) if with_interval else out


def evaluate(t, ibnd, re, cs):
    """phase_eval in the dtype of the table (cs already in [-1, 1])"""
    dt = t.mu.dtype
    F = dt.type
    re, cs = np.asarray(re, dtype=dt), np.asarray(cs, dtype=dt)
    P, mu = t.phase[ibnd], t.mu
    ire, jre, f = index(t, re)
    lo = np.zeros(cs.shape, dtype=np.int64)
    hi = np.full(cs.shape, mu.size - 1, dtype=np.int64)
    while np.any(hi - lo > 1):
        act = hi - lo > 1
        mid = (lo + hi) >> 1
        le = mu[mid] <= cs
        lo = np.where(act & le, mid, lo)
        hi = np.where(act & ~le, mid, hi)
    m0, m1 = mu[lo], mu[lo+1]
    w = np.fmin(np.fmax((cs - m0) / (m1 - m0), F(0.)), F(1.))
    a0, a1, b0, b1 = P[ire, lo], P[ire, lo+1], P[jre, lo], P[jre, lo+1]
    pa, pb = a0 + w*(a1 - a0), b0 + w*(b1 - b0)
    return (pa + f*(pb - pa)).astype(dt)


# ---- longdouble: the exact inverse and density of the table as it is stored (rounded nodes, phase and cdf), with the index and the
# blend weight computed in longdouble from the same re0, dre

def _ld_blend(t, ibnd, re):
    """the blended phase function and CDF (nmu,) of ONE radius, in longdouble"""
    re = LD(re)
    ire, jre, f = 0, 0, LD(0.)
    if t.nre > 1:
        q = (re - LD(t.re0)) / LD(t.dre)
        if not np.isnan(q):
            ire = int(min(max(q, LD(0.)), LD(t.nre - 2)))
            f = min(max(q - LD(ire), LD(0.)), LD(1.))
        jre = ire + 1
    P, C = t.phase[ibnd].astype(LD), t.cdf[ibnd].astype(LD)
    return P[ire] + f*(P[jre] - P[ire]), C[ire] + f*(C[jre] - C[ire])


def _per_radius(fn, t, ibnd, re, x):
    """fn(mu, Pb, Cb, x) per distinct radius (a NaN radius is one of them)"""
    re, x = np.asarray(re), np.asarray(x).astype(LD)
    out = np.empty(x.shape, dtype=LD)
    mu = t.mu.astype(LD)
    key = np.where(np.isnan(re), -np.inf, re)
    for k in np.unique(key):
        sel = key == k
        Pb, Cb = _ld_blend(t, ibnd, np.nan if k == -np.inf else k)
        out[sel] = fn(mu, Pb, Cb, x[sel])
    return out


def sample_ld(t, ibnd, re, u):
    def fn(mu, Pb, Cb, u):
        i = np.clip(np.searchsorted(Cb, u, side="right") - 1, 0, mu.size - 2)
        r = LD(2.)*(u - Cb[i])
        p0, p1 = Pb[i], Pb[i+1]
        s = (p1 - p0) / (mu[i+1] - mu[i])
        den = p0 + np.sqrt(np.maximum(LD(0.), p0*p0 + LD(2.)*s*r))
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = np.where(den > 0, LD(2.)*r/den, LD(0.))
        return np.clip(mu[i] + tt, mu[i], mu[i+1])
    return _per_radius(fn, t, ibnd, re, u)


def cdf_ld(t, ibnd, re, cs):
    """C(cs) of the blended table: the stored node values plus the exact integral of the linear piece"""
    def fn(mu, Pb, Cb, cs):
        i = np.clip(np.searchsorted(mu, cs, side="right") - 1, 0, mu.size - 2)
        d = cs - mu[i]
        s = (Pb[i+1] - Pb[i]) / (mu[i+1] - mu[i])
        return Cb[i] + LD(0.5)*(Pb[i]*d + LD(0.5)*s*d*d)
    return _per_radius(fn, t, ibnd, re, cs)


def evaluate_ld(t, ibnd, re, cs):
    def fn(mu, Pb, Cb, cs):
        i = np.clip(np.searchsorted(mu, cs, side="right") - 1, 0, mu.size - 2)
        w = np.clip((cs - mu[i]) / (mu[i+1] - mu[i]), 0, 1)
        return Pb[i] + w*(Pb[i+1] - Pb[i])
    return _per_radius(fn, t, ibnd, re, cs)


# ---- the forward event loop (raytracer_ref.trace_counts) with the table for the cloud species

def forward_counts(scene, table, igpt, photon0, nphotons, max_events=1 << 20):
    """rrx_rt_trace_counts_phase with table (a Table with cld_re). The photons [photon0, photon0 + nphotons) of g-point igpt. Returns the six count arrays (abs_*: (nz, ncol)), n_capped and
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
        ctau, cssa = (c[ib].reshape(-1) for c in s.cloud[:2])          # (cld_g is not read)
        cre = np.asarray(table.cld_re, dtype=dt).reshape(-1)
    albedo = np.asarray(s.sfc_albedo, dtype=dt)
    kgrid = k_null(s, igpt)
    inf = F(np.inf)
    one, zero, half = F(1.), F(0.), F(0.5)
    sun_x, sun_y, sun_z = sun_direction(s)
    dif_frac = F(s.inc_dif[igpt]) / (F(s.inc_dir[igpt]) + F(s.inc_dif[igpt]))
    key = (s.seed & 0xFFFFFFFF, (s.seed >> 32) & 0xFFFFFFFF)

    out = {k: np.zeros(ncol, dtype=np.uint64) for k in COUNT_NAMES[:4]}
    out.update({k: np.zeros(ncol*nz, dtype=np.uint64) for k in COUNT_NAMES[4:]})
    n_capped = 0
    events = 0
    cloud_scatterings = 0

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
                    tc, wc, re = ctau[cell], cssa[cell], cre[cell]
                else:
                    tc = wc = re = np.zeros(a.size, dtype=dt)
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
                    cloud_scatterings += int(cloud.sum())
                    u = np.full(a.size, half, dtype=dt); u[sc] = draw(a[sc])
                    cos_tab = sample(table, max(ib, 0), re, u)
                    q = F(4.)*u - F(2.)
                    A = np.cbrt(q + np.sqrt(one + q*q))
                    cos_ray = A - one/A
                    cos_s = np.clip(np.where(cloud, cos_tab, cos_ray), F(-1.), one).astype(dt)
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
    res["cloud_scatterings"] = cloud_scatterings          # (beside what raytracer_ref.trace_counts returns)
    return res


# ---- the backward event loop (raytracer_bw_ref.trace_counts) with the table for the cloud species

def backward_counts(scene, table, sensor, igpt, ray0, nrays, max_events=1 << 20, ranges=1):
    """rrx_rt_bw_trace_counts_phase with table (a Table with cld_re). The rays [ray0, ray0 + nrays) of g-point igpt. Returns counts (npix,) uint64, n_capped, n_clamped, n_dep (npix,) and
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
        ctau, cssa = (c[ib].reshape(-1) for c in s.cloud[:2])          # (cld_g is not read)
        cre = np.asarray(table.cld_re, dtype=dt).reshape(-1)
    albedo = np.asarray(s.sfc_albedo, dtype=dt)
    kgrid = R.k_null(s, igpt)
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
    tot = dict(n_capped=0, n_clamped=0, events=0, walk_cells=0, cloud_scatterings=0)          # (the last beside raytracer_bw_ref's)

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
                    tc, wc, re = ctau[cell], cssa[cell], cre[cell]
                else:
                    tc = wc = re = np.zeros(a.size, dtype=dt)
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
                    tot["cloud_scatterings"] += int(cloud.sum())
                    cs = np.clip(-((ux*sun_x + uy*sun_y) + uz*sun_z), -one, one).astype(dt)
                    p_tab = evaluate(table, max(ib, 0), re, cs)
                    p_ray = F(0.75)*(one + cs*cs)
                    dep = ((w*np.where(cloud, p_tab, p_ray))/(F(4.)*pi)).astype(dt)
                    hit = np.nonzero(sc)[0]
                    ok = deposit(pixel[hit], dep[hit], x[hit], y[hit], z[hit], i[hit], j[hit], k[hit])
                    alive[hit[~ok]] = False
                    sc = sc & alive
                    u = np.full(a.size, half, dtype=dt); u[sc] = draw(a[sc])
                    cos_tab = sample(table, max(ib, 0), re, u)
                    q = F(4.)*u - two
                    A = np.cbrt(q + np.sqrt(one + q*q))
                    cos_ray = A - one/A
                    cos_s = np.clip(np.where(cloud, cos_tab, cos_ray), -one, one).astype(dt)
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
