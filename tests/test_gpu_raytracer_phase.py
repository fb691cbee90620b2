"""GPU tests of the tabulated cloud phase functions of the two ray tracers (csrc/rrx_rt_phase.h, rrx_rt_phase.hip, the rrx_*_phase
entries). Tables, radii and probes: tests/raytracer_phase_scenes.py, on the scenes of raytracer_scenes.py (8 x 4 x 6
cells, two g-points, fixed seeds). The tallies are integers added with integer atomics, so a run that passes once passes always.

  1  an isotropic table is Henyey-Greenstein with g = 0, integer for integer (forward: six count arrays, backward: pixel counts)
  2  the _phase entries without a table give the existing entries' integers
  3  the builder, the sampler and the evaluator on arrays against the numpy restatement (bit for bit) and the longdouble inverse
  4  ray for ray against the numpy restatement, fp64, bounds derived as in test_gpu_raytracer*.py
  5  a tabulated HG(g) against the analytic HG(g) of the existing entries, 5 combined sigma
  6  forward against backward with a peaked table, the S3 idiom, 5 combined sigma
  7  split ranges, a second run, deep lists, the hand loop against the spectral entries, the chain, the C++ classes: the same bits

Observed on an MI355X: see DESIGN.md 4.16."""
import ctypes
import math
import os

import numpy as np
import pytest

import raytracer_ref as R
import raytracer_bw_ref as B
import raytracer_phase_ref as P
import raytracer_phase_scenes as PS
import raytracer_scenes as S
import raytracer_bw_scenes as BS
from raytracer_dev import _be, _dev, _u64, k_null, forward, backward, solve_fw, solve_bw
from rte_rrtmgp_cpp_amd import synthetic, pipeline, phase_tables, camera as C

pytestmark = pytest.mark.gpu
ONE = float(1 << 32)
NAMES = R.COUNT_NAMES
SENSORS = {"perspective": lambda: C.perspective(6, 4, (330., 250., 170.), yaw=0.6, pitch=-0.5, roll=0.2, fov=math.radians(70.)),
           "fisheye": lambda: C.fisheye(6, 4, (420., 130., 0.)),
           "orthographic": lambda: C.orthographic(6, 4, yaw=2.0, pitch=-1.0)}


def table(be, mu, raw, cld_re=None, re0=PS.RE0, dre=PS.DRE):
    t = phase_tables.build(be, mu, raw, re0, dre)
    return t if cld_re is None else t.with_radius(be.asarray(cld_re))


def ref_table(be, mu, raw, cld_re=None):
    t = P.build_tables(mu, raw, be.np_dtype, PS.RE0, PS.DRE)
    t.cld_re = cld_re
    return t


def same_counts(be, a, b, keys):
    for k in keys:
        assert np.array_equal(_u64(be, a[k]), _u64(be, b[k])), k


# ---- 1: an isotropic table is HG with g = 0

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("nre", [1, 3])
@pytest.mark.parametrize("nodes", [2, 5])
def test_1_isotropic_table_is_hg_with_g_zero_integer_for_integer(nodes, nre, dt, hip_f64, hip_f32):
    """-1 + 2u = 2u - 1 and P = 1 with the same draws in the same order: any drift in the draw order, the blend form or the
    inversion changes integers. Radii below, inside and above the grid, and NaN."""
    be = _be(dt, hip_f64, hip_f32)
    sc = PS.general_g(be.np_dtype, 0.0)
    d = _dev(be, sc)
    t = table(be, *PS.isotropic(nodes, nre), cld_re=PS.cell_radii_with_nan(sc, be.np_dtype))
    assert np.all(be.to_numpy(t.phase) == 1.0)
    for g in range(2):
        kn = k_null(be, sc, d, g)
        want = forward(be, sc, d, g, 5, 64*sc.ncol, kn=kn)
        got = forward(be, sc, d, g, 5, 64*sc.ncol, kn=kn, phase=t)
        same_counts(be, want, got, NAMES + ("n_capped",))
        assert all(_u64(be, want[k]).any() for k in NAMES) and int(_u64(be, want["n_capped"])[0]) == 0
        for sensor in (SENSORS["perspective"](), C.flux_sensor(sc.nx, sc.ny, True)):
            n = 32*sensor.npx*sensor.npy
            want = backward(be, sc, d, sensor, g, 3, n, kn=kn)
            got = backward(be, sc, d, sensor, g, 3, n, kn=kn, phase=t)
            same_counts(be, want, got, ("counts", "n_capped", "n_clamped"))
            assert _u64(be, want["counts"]).all()


# ---- 2: no table

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_2_phase_entries_without_a_table_are_the_existing_entries(dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc = S.general(be.np_dtype)
    d = _dev(be, sc)
    dims = (sc.nx, sc.ny, sc.nz, 2, 2)
    none = (0, 0, 0.0, 0.0, None, None, None, None)
    seed = sc.seed & 0xFFFFFFFFFFFFFFFF
    kn = k_null(be, sc, d, 1)
    want = forward(be, sc, d, 1, 0, 32*sc.ncol, kn=kn)
    got = be.rt_zero_counts(sc.nz, sc.ncol)
    be._c("rt_trace_counts_phase", *dims, 1, sc.top_at_1, sc.independent_column, d["tau"], d["ssa"], d["lims"], *d["cloud"], sc.dx, sc.dy, sc.dz,
          d["alb"], sc.mu0, sc.azimuth, float(sc.inc_dir[1]), float(sc.inc_dif[1]), *sc.kn_grid, kn, seed, 0, 32*sc.ncol, be.RT_MAX_EVENTS,
          *(got[k] for k in NAMES), got["n_capped"], *none)
    same_counts(be, want, got, NAMES + ("n_capped",))
    sensor = SENSORS["fisheye"]()
    stype, npx, npy, fov, numbers = be._rt_sensor(sensor)
    want = backward(be, sc, d, sensor, 1, 0, 32*npx*npy, kn=kn)
    got = be.rt_bw_zero_counts(npx*npy)
    be._c("rt_bw_trace_counts_phase", *dims, 1, sc.top_at_1, d["tau"], d["ssa"], d["lims"], *d["cloud"], sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0,
          sc.azimuth, *sc.kn_grid, kn, stype, npx, npy, fov, numbers, seed, 0, 32*npx*npy, be.RT_MAX_EVENTS, got["counts"], got["n_capped"],
          got["n_clamped"], *none)
    same_counts(be, want, got, ("counts", "n_capped", "n_clamped"))
    assert _u64(be, want["counts"]).any()
    # the spectral loops
    F = be.np_dtype
    want = solve_fw(be, sc, d, 8)
    outs = [be.empty((sc.ncol,)) for _ in range(4)] + [be.empty((sc.nz, sc.ncol)) for _ in range(2)]
    n_capped = be.rt_bw_zero_counts(1)["n_capped"]
    be._c("raytracer_sw_phase", *dims, sc.top_at_1, sc.independent_column, d["tau"], d["ssa"], d["lims"], *d["cloud"], sc.dx, sc.dy, sc.dz, d["alb"],
          sc.mu0, sc.azimuth, np.ascontiguousarray(sc.inc_dir, dtype=F), np.ascontiguousarray(sc.inc_dif, dtype=F), *sc.kn_grid, 8, seed,
          be.RT_MAX_EVENTS, *outs, n_capped, *none)
    for k, o in zip(NAMES, outs):
        assert np.array_equal(want[k].view(np.uint8), be.to_numpy(o).view(np.uint8)), k
    want = solve_bw(be, sc, d, sensor, 8)
    radiance, tallies = be.empty((npy, npx)), be.rt_bw_zero_counts(1)
    be._c("raytracer_bw_phase", *dims, sc.top_at_1, d["tau"], d["ssa"], d["lims"], *d["cloud"], sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth,
          np.ascontiguousarray(sc.inc_dir, dtype=F), *sc.kn_grid, stype, npx, npy, fov, numbers, 8, seed, be.RT_MAX_EVENTS, radiance,
          tallies["n_capped"], tallies["n_clamped"], *none)
    assert np.array_equal(be.to_numpy(want["radiance"]).view(np.uint8), be.to_numpy(radiance).view(np.uint8))


# ---- 3: the builder, the sampler and the evaluator on arrays

# Worst deviation of rrx_rt_phase_sample (absolute, in the cosine) and rrx_rt_phase_eval (relative) from the longdouble inverse and
# density of the stored table, as observed on an MI355X, and the bounds of twice the observation. fp32 loses digits in u - C_i where
# the CDF is steep against the 24-bit uniform, but u and C_i are both numbers of the format and their difference is exact, so what
# is seen is the rounding of the blend and of the inverse: about one step of the format in the cosine, two in P.
OBSERVED = {("double_hg33", "f64"): (1.809e-16, 2.761e-16), ("double_hg33", "f32"): (7.683e-08, 1.787e-07),
            ("hg1800", "f64"): (1.432e-16, 2.180e-16), ("hg1800", "f32"): (4.246e-08, 1.153e-07),
            ("hg1800_spread", "f64"): (1.070e-16, 2.614e-16), ("hg1800_spread", "f32"): (6.657e-08, 1.457e-07)}
TABLES = {"double_hg33": PS.double_hg33, "hg1800": PS.hg1800, "hg1800_spread": lambda: PS.hg1800(0.85, 3, 0.03)}


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("which", list(TABLES))
def test_3_builder_sampler_and_evaluator_on_arrays(which, dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    mu, raw = TABLES[which]()
    t = table(be, mu, raw)
    ref = ref_table(be, mu, raw)
    # the builder: double sums in node order, the restatement's bits
    assert np.array_equal(be.to_numpy(t.cdf), ref.cdf) and np.array_equal(be.to_numpy(t.phase), ref.phase)
    assert np.all(ref.cdf[..., 0] == 0) and np.all(ref.cdf[..., -1] == 1) and np.all(np.diff(ref.cdf, axis=-1) >= 0)
    nre = PS.probe_re(be.np_dtype).size
    worst_cos = worst_p = 0.0
    for b in range(PS.NBND):
        u, re = PS.probe_pairs(ref, b, be.np_dtype)
        cos = be.to_numpy(be.rt_phase_sample(t, b, be.asarray(u), be.asarray(re)))
        want, iv = P.sample(ref, b, re, u, with_interval=True)
        assert np.array_equal(cos, want)                                   # the same operations in the same order
        assert np.all(cos >= ref.mu[iv]) and np.all(cos <= ref.mu[iv+1])    # within the interval found
        n = u.size // nre
        assert all(np.all(np.diff(cos[r*n:(r+1)*n]) >= 0) for r in range(nre))          # monotone in u at every radius
        worst_cos = max(worst_cos, float(np.max(np.abs(cos - P.sample_ld(ref, b, re, u)))))
        cs = np.concatenate([ref.mu, 0.5*(ref.mu[1:] + ref.mu[:-1]), cos[:n]]).astype(be.np_dtype)
        cs, rr = np.tile(cs, nre), np.repeat(PS.probe_re(be.np_dtype), cs.size)
        p = be.to_numpy(be.rt_phase_eval(t, b, be.asarray(cs), be.asarray(rr)))
        assert np.array_equal(p, P.evaluate(ref, b, rr, cs))
        exact = P.evaluate_ld(ref, b, rr, cs)
        worst_p = max(worst_p, float(np.max(np.abs(p - exact) / exact)))
    seen_cos, seen_p = OBSERVED[(which, dt)]
    print(f"raytracer phase arrays {which} {dt}: worst |cos - longdouble| = {worst_cos:.3e} (bound {2*seen_cos:.3e}), worst relative "
          f"|P - longdouble| = {worst_p:.3e} (bound {2*seen_p:.3e})")
    assert worst_cos <= 2*seen_cos and worst_p <= 2*seen_p


def test_3b_builder_flags_bad_nodes_and_bad_tables(hip_f64):
    be = hip_f64
    mu, raw = PS.double_hg33()
    for bad_mu, word in ((np.r_[mu[:5], mu[4], mu[6:]], "strictly"), (np.r_[-0.9, mu[1:]], "strictly"), (mu[::-1].copy(), "strictly")):
        with pytest.raises(RuntimeError, match=word):
            phase_tables.build(be, bad_mu, raw)
    for spoil in (lambda r: r.__setitem__((1, 2), 0.0), lambda r: r.__setitem__((0, 0, 3), np.nan), lambda r: r.__setitem__((0, 1, 7), -1.0),
                  lambda r: r.__setitem__((1, 1, 30), np.inf)):
        r = raw.copy(); spoil(r)
        with pytest.raises(RuntimeError, match="integral"):
            phase_tables.build(be, mu, r)
    assert phase_tables.build(be, mu, raw).nre == 3


# ---- 4: ray for ray, fp64

@pytest.fixture(scope="module")
def peaked():
    """the general scene, the double-HG table and radii across the grid, with the restatement's forward result"""
    sc = S.general(np.float64)
    mu, raw = PS.double_hg33()
    re = PS.cell_radii(sc, np.float64)
    return sc, mu, raw, re


def test_4_forward_ray_for_ray(peaked, hip_f64):
    be = hip_f64
    sc, mu, raw, re = peaked
    ref_t = ref_table(be, mu, raw, re)
    ppp = 32
    ref = {k: np.zeros(sc.ncol) for k in NAMES[:4]}
    ref.update({k: np.zeros((sc.nz, sc.ncol)) for k in NAMES[4:]})
    events = np.zeros(2)
    for g in range(2):
        c = R.trace_counts(sc, g, 0, ppp*sc.ncol, table=ref_t)
        assert c["n_capped"] == 0
        scale = (sc.inc_dir[g] + sc.inc_dif[g]) / ppp
        for k in NAMES:
            ref[k] = R.counts_to_flux(c[k], scale if k in NAMES[:4] else scale/sc.dz, ref[k])
        events[g] = c["events"]
    r = solve_fw(be, sc, _dev(be, sc), ppp, phase=table(be, mu, raw, re))
    assert r["n_capped"] == 0
    inc = sc.inc_dir.astype(np.float64) + sc.inc_dif
    tol = float(np.sum(events * 2.0**-33 / ppp * inc))         # each deposit rounds once
    for k in NAMES:
        t = tol if k in NAMES[:4] else tol / sc.dz
        err = float(np.max(np.abs(r[k] - ref[k])))
        print(f"raytracer phase ray for ray {k}: max difference {err:.3e} (bound {t:.3e}), max value {float(np.max(ref[k])):.3e}")
        assert ref[k].any() and err <= t, k
    # the table matters: the Henyey-Greenstein entry on the same scene gives other numbers
    assert not np.array_equal(solve_fw(be, sc, _dev(be, sc), ppp)["tod_up"], r["tod_up"])


@pytest.mark.parametrize("kind", list(SENSORS))
def test_4_backward_ray_for_ray(kind, peaked, hip_f64):
    be = hip_f64
    sc, mu, raw, re = peaked
    ref_t = ref_table(be, mu, raw, re)
    sensor = SENSORS[kind]()
    rpp, npix = 32, 24
    want = np.zeros(npix)
    tol = np.zeros(npix)
    eps = np.finfo(np.float64).eps
    for g in range(2):
        c = B.trace_counts_bw(sc, sensor, g, 0, rpp*npix, table=ref_t)
        assert c["n_capped"] == 0 and c["n_clamped"] == 0
        scale = sc.inc_dir[g] / (sc.mu0*rpp)
        want = R.counts_to_flux(c["counts"], scale, want)
        tol += (c["n_dep"] * 2.0**-32 + 4*eps*c["sum_d"]) * float(sc.inc_dir[g]) / float(sc.mu0) / rpp
    r = solve_bw(be, sc, _dev(be, sc), sensor, rpp, phase=table(be, mu, raw, re))
    assert r["n_capped"] == 0 and r["n_clamped"] == 0
    got = be.to_numpy(r["radiance"]).reshape(-1)
    err = np.abs(got - want)
    print(f"raytracer phase ray for ray {kind}: max difference {float(err.max()):.3e} W m-2 sr-1 (bound there "
          f"{float(tol[np.argmax(err)]):.3e}), worst difference/bound {float(np.max(err/tol)):.3f}")
    assert np.all(want > 0) and np.all(err <= tol)


# ---- 5: a tabulated HG against the analytic one

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_5_tabulated_hg_against_analytic_hg(dt, hip_f64, hip_f32):
    """An 1 800-node table of HG(0.85) against cld_g = 0.85 in every cloudy cell: two independent estimates of (almost) the same
    quantity. Forward: the domain means of the surface and top tallies, per-photon contributions in [0, 1]: sigma of
    raytracer_scenes.sigma for each run, combined. Backward: flux sensors, 16 disjoint ranges each, the standard errors combined. The
    table's own error (the trapezoid rule on 1 800 nodes, 1e-6 of the CDF) is far below the 1e-3 that these sample sizes resolve."""
    be = _be(dt, hip_f64, hip_f32)
    g_hg = 0.85
    sc = PS.general_g(be.np_dtype, g_hg)
    sc.inc_dif = np.zeros_like(sc.inc_dif)
    d = _dev(be, sc)
    t = table(be, *PS.hg1800(g_hg), cld_re=PS.cell_radii(sc, be.np_dtype))
    ppp = 256
    n = ppp*sc.ncol
    per_range = (BS.S3_RAYS//BS.S3_RANGES)*sc.ncol
    worst = 0.0
    for g in range(2):
        kn = k_null(be, sc, d, g)
        a = forward(be, sc, d, g, 0, n, kn=kn)
        b = forward(be, sc, d, g, n, n, kn=kn, phase=t)          # other photons: independent
        for k in ("sfc_dn_dir", "sfc_dn_dif", "sfc_up", "tod_up"):
            pa, pb = _u64(be, a[k]).sum()/ONE/n, _u64(be, b[k]).sum()/ONE/n
            dev = abs(pa - pb) / math.sqrt(S.sigma(pa, n)**2 + S.sigma(pb, n)**2 + 1e-300)
            print(f"raytracer phase 5 {dt} g-point {g} {k}: HG {pa:.5f}, table {pb:.5f}, {dev:.2f} combined sigma (bound 5)")
            assert pa > 0 and dev <= 5, (k, g, dev)
            worst = max(worst, dev)
        for name, sensor in BS.flux_sensors(sc).items():
            ea = np.stack([_u64(be, backward(be, sc, d, sensor, g, r*per_range, per_range, kn=kn)["counts"]) for r in range(BS.S3_RANGES)])
            eb = np.stack([_u64(be, backward(be, sc, d, sensor, g, (BS.S3_RANGES + r)*per_range, per_range, kn=kn, phase=t)["counts"])
                           for r in range(BS.S3_RANGES)])
            ma, mb = ea.mean(axis=1)/ONE, eb.mean(axis=1)/ONE
            se = math.sqrt(ma.var(ddof=1)/BS.S3_RANGES + mb.var(ddof=1)/BS.S3_RANGES)
            dev = abs(ma.mean() - mb.mean()) / se
            print(f"raytracer phase 5 {dt} g-point {g} backward {name}: HG {ma.mean():.5f}, table {mb.mean():.5f}, {dev:.2f} combined sigma (bound 5)")
            assert ma.mean() > 0 and dev <= 5, (name, g, dev)
            worst = max(worst, dev)
    print(f"raytracer phase 5 {dt}: worst {worst:.2f} combined sigma (bound 5)")


# ---- 6: forward against backward with a peaked table

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_6_forward_against_backward_with_a_peaked_table(dt, hip_f64, hip_f32):
    """The S3 idiom of test_gpu_raytracer_bw.py with the double-HG table on two radii: 1 024 photons per pixel against 16 disjoint
    ranges of 64 rays per pixel; domain means and pixels within 5 combined sigma. The forward tracer samples the table, the backward
    tracer samples AND evaluates it: they agree only if the evaluator is the density of the sampler."""
    be = _be(dt, hip_f64, hip_f32)
    sc = BS.general_direct(be.np_dtype)
    d = _dev(be, sc)
    t = table(be, *PS.double_hg33_two_radii(), cld_re=PS.cell_radii(sc, be.np_dtype), re0=4.0, dre=6.0)
    per_range = (BS.S3_RAYS//BS.S3_RANGES)*sc.ncol
    worst = 0.0
    for g in range(2):
        kn = k_null(be, sc, d, g)
        fwd = forward(be, sc, d, g, 0, BS.S3_PHOTONS*sc.ncol, kn=kn, phase=t, inc_dif=0.0)
        assert int(_u64(be, fwd["n_capped"])[0]) == 0
        for name, sensor in BS.flux_sensors(sc).items():
            parts = []
            for r in range(BS.S3_RANGES):
                c = backward(be, sc, d, sensor, g, r*per_range, per_range, kn=kn, phase=t)
                assert int(_u64(be, c["n_capped"])[0]) == 0 and int(_u64(be, c["n_clamped"])[0]) == 0
                parts.append(_u64(be, c["counts"]))
            worst = max(worst, BS.compare_forward_backward(sc, g, name, _u64(be, fwd[name]), np.stack(parts), f"phase {dt}"))
    print(f"raytracer phase 6 {dt}: worst {worst:.2f} combined sigma (bound 5)")


# ---- 7: the same integers and bits by other routes

def test_7_counts_are_additive_reproducible_deep_and_the_loops_are_the_entries(peaked, hip_f64, monkeypatch):
    be = hip_f64
    sc, mu, raw, re = peaked
    d = _dev(be, sc)
    t = table(be, mu, raw, re)
    sensor = SENSORS["perspective"]()
    kn = k_null(be, sc, d, 1)
    n = 32*sc.ncol
    whole = forward(be, sc, d, 1, 0, n, kn=kn, phase=t)
    again = forward(be, sc, d, 1, 0, n, kn=kn, phase=t)
    parts = forward(be, sc, d, 1, 0, n//3, kn=kn, phase=t)
    parts = forward(be, sc, d, 1, n//3, n - n//3, kn=kn, phase=t, counts=parts)
    monkeypatch.setenv("RRX_RT_MAX_BLOCKS", "1")
    deep = forward(be, sc, d, 1, 0, n, kn=kn, phase=t)
    monkeypatch.delenv("RRX_RT_MAX_BLOCKS")
    for other in (again, parts, deep):
        same_counts(be, whole, other, NAMES + ("n_capped",))
    m = 32*sensor.npix
    whole = backward(be, sc, d, sensor, 1, 0, m, kn=kn, phase=t)
    again = backward(be, sc, d, sensor, 1, 0, m, kn=kn, phase=t)
    parts = backward(be, sc, d, sensor, 1, 0, m//3, kn=kn, phase=t)
    parts = backward(be, sc, d, sensor, 1, m//3, m - m//3, kn=kn, phase=t, counts=parts)
    monkeypatch.setenv("RRX_RT_MAX_BLOCKS", "1")
    deep = backward(be, sc, d, sensor, 1, 0, m, kn=kn, phase=t)
    monkeypatch.delenv("RRX_RT_MAX_BLOCKS")
    for other in (again, parts, deep):
        same_counts(be, whole, other, ("counts", "n_capped", "n_clamped"))
    assert _u64(be, whole["counts"]).all()
    # the hand loops against the spectral entries
    F = be.np_dtype.type
    ppp = 16
    flux = {k: be.zeros((sc.ncol,)) for k in NAMES[:4]}
    flux.update({k: be.zeros((sc.nz, sc.ncol)) for k in NAMES[4:]})
    radiance = be.zeros((sensor.npix,))
    for g in range(2):
        c = forward(be, sc, d, g, 0, ppp*sc.ncol, phase=t)
        scale = (F(sc.inc_dir[g]) + F(sc.inc_dif[g])) / F(ppp)
        for k in NAMES:
            be.rt_counts_to_flux(c[k], float(scale if k in NAMES[:4] else scale / F(sc.dz)), flux[k])
        c = backward(be, sc, d, sensor, g, 0, ppp*sensor.npix, phase=t)
        be.rt_counts_to_flux(c["counts"], float(F(sc.inc_dir[g]) / (F(sc.mu0)*F(ppp))), radiance)
    r = solve_fw(be, sc, d, ppp, phase=t)
    for k in NAMES:
        assert np.array_equal(be.to_numpy(flux[k]).view(np.uint8), r[k].view(np.uint8)), k
    rb = solve_bw(be, sc, d, sensor, ppp, phase=t)
    assert np.array_equal(be.to_numpy(radiance).view(np.uint8), be.to_numpy(rb["radiance"]).reshape(-1).view(np.uint8))


def test_7_chain_with_a_phase_table_is_the_entry_on_the_chain_s_own_arrays(hip_f64):
    """pipeline.raytrace_sw / render_sw with phase_table=: the cells' radius is the liquid radius atm.rel; the same bits as the
    entries on arrays made by hand. A table without cloud_lut raises."""
    be = hip_f64
    nx, ny, nlay, n = 4, 4, 12, 8
    kd = be.upload_kdist(synthetic.make_kdist("sw", ngpt=32, nbnd=2, npres=10, nflav=3, nminor_lower=5, nminor_upper=3))
    atm0 = synthetic.make_atmosphere(nx*ny, nlay, nbnd_lw=2, nbnd_sw=2, clouds=True)
    atm = pipeline.upload_atmosphere(be, atm0)
    lut = be.upload_lut(synthetic.make_cloud_lut(2, "sw"))
    dz = 70.e3/nlay
    rel = be.to_numpy(atm.rel)
    mu, raw = PS.double_hg33()
    t = phase_tables.build(be, mu, raw, float(rel[rel > 0].min()) if (rel > 0).any() else 2.5, 2.0)
    cam = C.perspective(5, 3, (800., 700., 20.e3), yaw=0.4, pitch=-1.0, fov=math.radians(50.))
    common = dict(cloud_lut=lut, kn_grid=(2, 2, 3))
    r = pipeline.raytrace_sw(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, n, S.SEED, phase_table=t, **common)
    i = pipeline.render_sw(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, cam, n, S.SEED, phase_table=t, **common)
    assert r["n_capped"] == 0 and i["n_capped"] == 0 and i["n_clamped"] == 0

    _, col_gas, _ = pipeline.gas_state(be, kd, atm, None, interpolate=False)
    col_dry = be.get_col_dry(atm.vmr["h2o"], atm.p_lev)
    tau, ssa = be.empty((32, nlay, nx*ny)), be.empty((32, nlay, nx*ny))
    be.gas_optics_sw_direct(kd, atm.p_lay, atm.t_lay, col_gas, col_dry, tau, ssa, None)
    cld = be.cloud_optics_2str(lut, atm.lwp, atm.iwp, atm.rel, atm.dei)
    assert float(cld[0].max()) > 0
    inc_dir = (be.to_numpy(kd.solar_source) * atm0.tsi_scaling[0]) * atm0.mu0[0]
    alb = be.asarray(atm0.sfc_alb_dif[:, 0].copy())
    tr = t.with_radius(atm.rel)
    want = be.raytracer_sw(tau, ssa, nx, ny, 400.0, 400.0, dz, alb, float(atm0.mu0[0]), 1.1, inc_dir, np.zeros_like(inc_dir), (2, 2, 3), n,
                           S.SEED, top_at_1=atm0.top_at_1, cloud=cld, band_lims=kd.band_lims_gpt, phase=tr)
    for k in NAMES:
        assert np.array_equal(be.to_numpy(r[k]).view(np.uint8), be.to_numpy(want[k]).view(np.uint8)), k
    plain = pipeline.raytrace_sw(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, n, S.SEED, **common)
    assert not np.array_equal(be.to_numpy(plain["tod_up"]), be.to_numpy(r["tod_up"]))
    want = be.raytracer_bw(tau, ssa, nx, ny, 400.0, 400.0, dz, alb, float(atm0.mu0[0]), 1.1, inc_dir, (2, 2, 3), cam, n, S.SEED,
                           top_at_1=atm0.top_at_1, cloud=cld, band_lims=kd.band_lims_gpt, phase=tr)
    assert np.array_equal(be.to_numpy(i["radiance"]).view(np.uint8), be.to_numpy(want["radiance"]).view(np.uint8))
    for fn, args in ((pipeline.raytrace_sw, (n,)), (pipeline.render_sw, (cam, n))):
        with pytest.raises(ValueError, match="cloud_lut"):
            fn(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, *args, S.SEED, phase_table=t)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_7_cxx_classes_with_a_phase_table_give_the_entries_bit_for_bit(dt, hip_f64, hip_f32):
    """Raytracer_gpu / Raytracer_bw_gpu after set_phase_table (through rrx_cxx_trace_rays_phase / rrx_cxx_trace_rays_bw_phase) against
    rrx_raytracer_sw_phase / rrx_raytracer_bw_phase; a refused table comes back as an exception's message."""
    import torch
    be = _be(dt, hip_f64, hip_f32)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so" if dt == "f64" else "librte_rrtmgp_hip_sp.so"))
    lib.rrx_cxx_driver_error.restype = ctypes.c_char_p
    F = ctypes.c_double if dt == "f64" else ctypes.c_float
    sc = S.general(be.np_dtype)
    d = _dev(be, sc)
    mu, raw = PS.double_hg33()
    t = table(be, mu, raw, PS.cell_radii(sc, be.np_dtype))
    sensor = SENSORS["perspective"]()
    n = 16
    Pp = lambda x: ctypes.c_void_p(x.data_ptr())
    H = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    inc_dir = np.ascontiguousarray(sc.inc_dir, dtype=be.np_dtype); inc_dif = np.ascontiguousarray(sc.inc_dif, dtype=be.np_dtype)
    scene = (sc.nx, sc.ny, sc.nz, 2, 2, F(sc.dx), F(sc.dy), F(sc.dz), int(sc.top_at_1))
    optics = (Pp(d["tau"]), Pp(d["ssa"]), Pp(d["lims"]), *(Pp(c) for c in d["cloud"]), Pp(d["alb"]), F(sc.mu0), F(sc.azimuth))

    def tab(dre):
        return (t.nmu, t.nre, F(t.re0), F(dre), Pp(t.mu), Pp(t.phase), Pp(t.cdf), Pp(t.cld_re))

    want = solve_fw(be, sc, d, n, phase=t)
    outs = [be.empty((sc.ncol,)) for _ in range(4)] + [be.empty((sc.nz, sc.ncol)) for _ in range(2)]
    out6 = (ctypes.c_void_p * 6)(*[o.data_ptr() for o in outs])
    n_capped, n_clamped = ctypes.c_ulonglong(99), ctypes.c_ulonglong(99)

    def fw(dre):
        return lib.rrx_cxx_trace_rays_phase(*scene, int(sc.independent_column), *optics, H(inc_dir), H(inc_dif), *sc.kn_grid, ctypes.c_longlong(n),
                                            ctypes.c_ulonglong(sc.seed), be.RT_MAX_EVENTS, out6, ctypes.byref(n_capped), *tab(dre), stream())

    assert fw(t.dre) == 0, lib.rrx_cxx_driver_error().decode()
    torch.cuda.synchronize()
    assert n_capped.value == 0
    for k, o in zip(NAMES, outs):
        assert np.array_equal(be.to_numpy(o).view(np.uint8), want[k].view(np.uint8)), k
    assert fw(0.0) != 0
    msg = lib.rrx_cxx_driver_error().decode()
    assert "rrx_raytracer_sw_phase" in msg and "dre" in msg, msg

    want = solve_bw(be, sc, d, sensor, n, phase=t)
    out = be.empty((sensor.npy, sensor.npx))
    numbers = sensor.numbers(be.np_dtype)

    def bw(dre):
        return lib.rrx_cxx_trace_rays_bw_phase(*scene, *optics, H(inc_dir), *sc.kn_grid, sensor.type, sensor.npx, sensor.npy, F(sensor.fov),
                                               H(numbers), ctypes.c_longlong(n), ctypes.c_ulonglong(sc.seed), be.RT_MAX_EVENTS, Pp(out),
                                               ctypes.byref(n_capped), ctypes.byref(n_clamped), *tab(dre), stream())

    assert bw(t.dre) == 0, lib.rrx_cxx_driver_error().decode()
    torch.cuda.synchronize()
    assert n_capped.value == 0 and n_clamped.value == 0
    assert np.array_equal(be.to_numpy(out).view(np.uint8), be.to_numpy(want["radiance"]).view(np.uint8))
    assert bw(-1.0) != 0
    msg = lib.rrx_cxx_driver_error().decode()
    assert "rrx_raytracer_bw_phase" in msg and "dre" in msg, msg
