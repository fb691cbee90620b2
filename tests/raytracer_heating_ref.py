"""numpy restatement of the thermal tracer's cell sensors (csrc/rrx_raytracer_heating.hip): 3-D longwave heating by
emission reciprocity. The same Philox stream (counter word 2 is igpt | 0x40000000), the same draw order and the same arithmetic,
operation for operation, vectorised over the rays. The medium and the transport steps are those of raytracer_ref, imported unchanged
(Grid, Particles, cross, collide, roulette, collision_outcome, scatter_direction, lambert); the scene is a
raytracer_thermal_ref.ThermalScene. What is stated here is this tracer's own: the start in the ray's own cell, the lane's reference
(B0, s0), the three signed deposits, the event loop with them and the tally in int64.

The device sums the rounded deposits of a ray in the lane and adds the sum into the ray's cell when the ray ends; the sums are
integers, so adding every rounded deposit into the cell as it is made gives the same numbers."""
import numpy as np

import raytracer_ref as R
from raytracer_thermal_spectral_ref import ray_list as _sensor_ray_list
from raytracer_spectral_ref import ranges_by_gpt

TWO_PI = R.TWO_PI
FOUR_PI = 12.566370614359172
D_MAX = 1048576.0
C2_HEATING = 0x40000000


def to_count(d):
    """llrint(d 2^32) of deposits already clamped: signed"""
    return np.rint(d.astype(np.float64) * 4294967296.0).astype(np.int64)


def reference(scene, igpt, weight0=None):
    """(B0, s0) by cell (nz ncol,) of g-point igpt in the scene's precision: the source of the cell and
    F(4 pi) ((t (1 - w0)) + (tc (1 - wc))), then times weight0 when one is given (the spectral form)"""
    s = scene.medium
    dt = s.dtype
    F = dt.type
    one = F(1.)
    G = R.Grid(s, igpt)
    s0 = F(FOUR_PI)*((G.tau*(one - G.ssa)) + (G.cld_tau*(one - G.cld_ssa)))
    if weight0 is not None:
        s0 = s0*F(weight0)
    return np.asarray(scene.lay_src[igpt], dtype=dt).reshape(-1), s0.astype(dt)


def trace_counts_heating(scene, igpt, ray0, nrays, max_events=1 << 20, ranges=1, weight0=None):
    """The rays [ray0, ray0 + nrays) of g-point igpt (rrx_heating3d_counts; weight0: the factor on s0 of the spectral form).
    Returns counts (ncell,) int64 in the layout of lay_src, n_capped, n_clamped, n_dep (ncell,), the number of deposits d != 0, and
    sum_abs (ncell,) float64, the sum of |d|, events (collisions + crossings of all rays) and deposits (all rays, zeros included).
    ranges > 1: the rays are tallied as that many consecutive ranges of nrays/ranges rays each, counts, n_dep and sum_abs are
    (ranges, ncell) (integer adds: the same numbers as one call per range)."""
    s = scene.medium
    dt = s.dtype
    F = dt.type
    nx, ny, nz, ncol = s.nx, s.ny, s.nz, s.ncol
    ncell = ncol*nz
    knx, kny, knz = s.kn_grid
    G = R.Grid(s, igpt)
    dx, dy, dz, kdx, kdy, kdz = G.dx, G.dy, G.dz, G.kdx, G.kdy, G.kdz
    one, zero, two = F(1.), F(0.), F(2.)
    lay_src = np.asarray(scene.lay_src[igpt], dtype=dt).reshape(-1)
    sfc_src = np.asarray(scene.sfc_src[igpt], dtype=dt).reshape(-1)
    emis = np.asarray(scene.sfc_emis, dtype=dt).reshape(-1)
    top_radiance = F(scene.top_radiance[igpt])
    B0_cell, s0_cell = reference(scene, igpt, weight0)

    if int(nrays) % int(ranges) != 0:
        raise ValueError("ranges does not divide nrays")
    counts = np.zeros(ranges*ncell, dtype=np.int64)
    n_dep = np.zeros(ranges*ncell, dtype=np.int64)
    sum_abs = np.zeros(ranges*ncell, dtype=np.float64)
    tot = dict(n_clamped=0, deposits=0)

    N = int(nrays)
    pt = R.Particles(ray0, N, int(igpt) | C2_HEATING, s.seed, dt)
    C = (pt.index % np.uint64(ncell)).astype(np.int64)
    I, J, K = C % nx, (C // nx) % ny, C // (nx*ny)
    CELL0 = I + J*nx + ncol*((nz - 1 - K) if s.top_at_1 else K)
    B0, S0 = B0_cell[CELL0], s0_cell[CELL0]

    def slot_of(a):
        return CELL0[a] + ncell*(a // (N // ranges))

    def score(a, d):
        """tallies clamp(d, -D_MAX, D_MAX) of the rays a into their own cells"""
        d = d.astype(dt)
        clamped = np.abs(d) > F(D_MAX)
        tot["n_clamped"] += int(clamped.sum())
        tot["deposits"] += d.size
        d = np.where(clamped, np.copysign(F(D_MAX), d), d)
        slot = slot_of(a)
        np.add.at(counts, slot, to_count(d))
        np.add.at(n_dep, slot, (d != zero).astype(np.int64))
        np.add.at(sum_abs, slot, np.abs(d.astype(np.float64)))

    # ---- start: a cell with s0 == 0 ends its ray at once; the others draw x, y, z, uz, phi
    ALIVE = S0 != zero
    go = np.nonzero(ALIVE)[0]
    SX, SY, SZ = np.zeros(N, dtype=dt), np.zeros(N, dtype=dt), np.zeros(N, dtype=dt)
    UX, UY, UZ = np.zeros(N, dtype=dt), np.zeros(N, dtype=dt), np.full(N, -one, dtype=dt)
    SX[go] = (I[go].astype(dt) + pt.draw(go))*dx
    SY[go] = (J[go].astype(dt) + pt.draw(go))*dy
    SZ[go] = (K[go].astype(dt) + pt.draw(go))*dz
    UZ[go] = one - two*pt.draw(go)
    phi = F(TWO_PI)*pt.draw(go)
    st = np.sqrt(np.maximum(zero, one - UZ[go]*UZ[go]))
    UX[go], UY[go] = st*np.cos(phi), st*np.sin(phi)
    IN = np.clip((SX/kdx).astype(np.int64), 0, knx-1); JN = np.clip((SY/kdy).astype(np.int64), 0, kny-1)
    KN = np.clip((SZ/kdz).astype(np.int64), 0, knz-1)
    X = np.clip(SX, IN.astype(dt)*kdx, (IN+1).astype(dt)*kdx)
    Y = np.clip(SY, JN.astype(dt)*kdy, (JN+1).astype(dt)*kdy)
    Z = np.clip(SZ, KN.astype(dt)*kdz, (KN+1).astype(dt)*kdz)
    pt.start(X, Y, Z, UX, UY, UZ, IN, JN, KN, ALIVE)

    # ---- the event loop: every pass is one event of every ray still alive
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a, p in pt.passes(max_events):
            b0, s0 = B0[a], S0[a]
            top, sfc = R.cross(G, pt, a, p)
            if top.any():
                score(a[top], (p.w*((top_radiance - b0)*s0))[top])
            if sfc.any():
                p.z = np.where(sfc, zero, p.z)
                col = R.fine_cell(p.x, dx, p.i_n, G.rx) + nx*R.fine_cell(p.y, dy, p.j_n, G.ry)
                score(a[sfc], ((p.w*emis[col])*((sfc_src[col] - b0)*s0))[sfc])
                p.w = np.where(sfc, p.w*(one - emis[col]), p.w)
                R.roulette(pt, a, p.w, sfc)
                live = sfc & (p.w > zero)
                p.ux[live], p.uy[live], p.uz[live] = R.lambert(pt, a[live], one)
                p.pend[live] = False
                p.alive[sfc & ~live] = False
            h = ~p.crossed
            if h.any():
                c = R.collide(G, p, h)
                score(a[h], ((p.w*(one - c.f_no_abs))*((lay_src[c.cell] - b0)*s0))[h])
                sc, cloud, aerosol = R.collision_outcome(pt, a, p, h, c)
                if sc.any():
                    p.ux, p.uy, p.uz = R.scatter_direction(pt, a, sc, cloud, aerosol, G.species, c.cell, p.ux, p.uy, p.uz)

    if ranges > 1:
        counts, n_dep, sum_abs = counts.reshape(ranges, ncell), n_dep.reshape(ranges, ncell), sum_abs.reshape(ranges, ncell)
    return dict(counts=counts, n_dep=n_dep, sum_abs=sum_abs, n_capped=pt.n_capped, events=pt.events, **tot)


class _Cells:
    """the cells as the sensor of raytracer_thermal_spectral_ref.ray_list: npx npy = ncell"""
    def __init__(self, scene):
        self.npx, self.npy = scene.ncol*scene.nz, 1


def ray_list(scene, m):
    """ray_end (ngpt+1,) int64, weight0 (ngpt,) in the scene's precision, and U: what rrx_heating3d_render forms from m (ngpt,)
    rays per cell, as rrx_thermal_render_spectral forms them from rays per pixel"""
    return _sensor_ray_list(scene, _Cells(scene), m)


def trace_counts_spectral(scene, ray_end, weight0, ray0, nrays, max_events=1 << 20):
    """rrx_heating3d_counts_spectral: counts (ncell,) int64 of all g-points that the range meets, n_dep, sum_abs, n_capped,
    n_clamped, events and deposits"""
    ncell = scene.ncol*scene.nz
    out = dict(counts=np.zeros(ncell, dtype=np.int64), n_dep=np.zeros(ncell, dtype=np.int64), sum_abs=np.zeros(ncell), n_capped=0,
               n_clamped=0, events=0, deposits=0)
    for g, q0, n in ranges_by_gpt(ray_end, ray0, nrays):
        c = trace_counts_heating(scene, g, q0, n, max_events, weight0=weight0[g])
        for k in out:
            out[k] = out[k] + c[k]
    return out


def counts_to_flux(counts, U, dtype):
    """flux_conv = F(counts 2^-32) U, the conversion of the signed counts"""
    dt = np.dtype(dtype)
    return ((counts.astype(np.float64) * 2.3283064365386963e-10).astype(dt) * dt.type(U)).astype(dt)


def render(scene, m, max_events=1 << 20):
    """rrx_heating3d_render: flux_conv (ncell,) in W m-2 from one conversion with scale = U; also the counts, n_dep, U, weight0"""
    ray_end, weight0, U = ray_list(scene, m)
    c = trace_counts_spectral(scene, ray_end, weight0, 0, int(ray_end[-1]), max_events)
    c.update(flux_conv=counts_to_flux(c["counts"], U, scene.dtype), U=U, weight0=weight0)
    return c
