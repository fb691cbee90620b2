"""GPU tests of the thermal tracer's cell sensors: 3-D longwave heating by emission reciprocity (rrx_heating3d_counts,
rrx_heating3d_counts_spectral, rrx_heating3d_render; csrc/rrx_raytracer_heating.hip). Scenes:
tests/heating_scenes.py; restatement: tests/raytracer_heating_ref.py. The tallies are integers added with integer atomics, so a run
that passes once passes always; the integer comparisons are exact, the bounds are derived, not measured:
  H0 cavity        every count is the integer 0;
  H1 slab          5 standard errors of 16 disjoint ray ranges about the extended-precision truth (heating_scenes.slab_truth);
                   test_raytracer_heating_ref.py holds that the ray budget puts the standard error below 2 % of the largest layer;
  H2 closure       5 times the root of the two estimators' summed variances, each from 16 ranges;
  ray for ray      one count per deposit plus 4 eps of the sum of |d|, the bound of test_gpu_raytracer_bw.py::test_ray_for_ray;
  uneven weights   half a count per deposit (the device and the restatement scale s0 by the same weight)."""
import ctypes
import math
import os

import numpy as np
import pytest

import heating_scenes as HS
import raytracer_heating_ref as H
import thermal_scenes as TS
from raytracer_dev import _be, _u64
from raytracer_thermal_dev import dev, k_null, ranges as sensor_ranges, render as sensor_render
from rte_rrtmgp_cpp_amd import camera as C
from rte_rrtmgp_cpp_amd import pipeline

pytestmark = pytest.mark.gpu
KEYS = ("counts", "n_capped", "n_clamped")
CHUNK = "RRX_RT_SPECTRAL_GPT_PER_LAUNCH"
NCELL = HS.NCELL


def numbers(be, c):
    """counts (ncell,) int64, n_capped and n_clamped (ints) of a counts dictionary on the device"""
    return dict(counts=be.to_numpy(c["counts"]).reshape(-1), n_capped=int(_u64(be, c["n_capped"])[0]), n_clamped=int(_u64(be, c["n_clamped"])[0]))


def k_null_all(be, sc, d):
    return be.rt_k_null_all(d["tau"], sc.nx, sc.ny, sc.dz, sc.kn_grid, sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"])


def heat(be, sc, d, g, ray0, nrays, kn=None, counts=None, max_events=None):
    """rrx_heating3d_counts"""
    kn = k_null(be, sc, d, g) if kn is None else kn
    return be.thermal_heating_counts(d["tau"], d["ssa"], g, sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["emis"], d["lay_src"], d["sfc_src"],
                                     float(sc.top_radiance[g]), sc.kn_grid, kn, sc.seed, ray0, nrays, top_at_1=sc.top_at_1,
                                     cloud=d["cloud"], band_lims=d["lims"], counts=counts, max_events=max_events)


def heat_spectral(be, sc, d, lists, ray0, nrays, kn=None, counts=None, max_events=None, top="own"):
    """rrx_heating3d_counts_spectral; lists = (ray_end, weight0)"""
    kn = k_null_all(be, sc, d) if kn is None else kn
    top = np.asarray(sc.top_radiance) if isinstance(top, str) else top
    return be.thermal_heating_counts_spectral(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["emis"], d["lay_src"], d["sfc_src"], top,
                                              lists[0], lists[1], sc.kn_grid, kn, sc.seed, ray0, nrays, d["lims"], top_at_1=sc.top_at_1,
                                              cloud=d["cloud"], counts=counts, max_events=max_events)


def heat_render(be, sc, d, m, max_events=None):
    """rrx_heating3d_render, flux_conv as (ncell,) on the host"""
    r = be.thermal_heating_render(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["emis"], d["lay_src"], d["sfc_src"], sc.kn_grid, m,
                                  sc.seed, d["lims"], top_at_1=sc.top_at_1, cloud=d["cloud"], max_events=max_events,
                                  top_radiance=np.asarray(sc.top_radiance))
    r["flux_conv"] = be.to_numpy(r["flux_conv"]).reshape(-1)
    return r


def heat_ranges(be, sc, d, n_ranges, rays_per_range):
    """the counts of n_ranges disjoint ray ranges of rays_per_range rays per cell each, summed over the g-points, (n_ranges, ncell);
    asserts that nothing was capped or clamped"""
    ncell = sc.ncol*sc.nz
    per = rays_per_range*ncell
    kn = [k_null(be, sc, d, g) for g in range(sc.tau.shape[0])]
    out = []
    for r in range(n_ranges):
        c = None
        for g in range(sc.tau.shape[0]):
            c = heat(be, sc, d, g, r*per, per, kn=kn[g], counts=c)
        c = numbers(be, c)
        assert c["n_capped"] == 0 and c["n_clamped"] == 0
        out.append(c["counts"])
    return np.stack(out)


# ---- H0: the cavity

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_h0_a_black_body_cavity_gives_the_integer_zero(dt, hip_f64, hip_f32):
    """Every source and top_radiance equal S_g, with cloud, gas scattering and sfc_emis < 1: every deposit is a difference of equal
    numbers, every count the integer 0, through each of the three entries."""
    be = _be(dt, hip_f64, hip_f32)
    sc = HS.cavity(be.np_dtype)
    d = dev(be, sc)
    assert d["ssa"] is not None and d["cloud"] is not None and float(sc.sfc_emis.max()) < 1
    m = np.array([40, 3, 1, 15, 6])
    ray_end, w0, _ = H.ray_list(sc, m)
    got = numbers(be, heat_spectral(be, sc, d, (ray_end, w0), 0, int(ray_end[-1])))
    assert not got["counts"].any() and got["n_capped"] == 0 and got["n_clamped"] == 0
    one = numbers(be, heat(be, sc, d, 0, 0, 8*NCELL))
    assert not one["counts"].any() and one["n_capped"] == 0
    r = heat_render(be, sc, d, m)
    assert not r["flux_conv"].any() and r["flux_conv"].shape == (NCELL,) and r["n_capped"] == 0 and r["n_clamped"] == 0


# ---- H1: the slab against truth

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_h1_the_slab_against_extended_precision_truth(dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc = HS.slab(be.np_dtype)
    d = dev(be, sc)
    assert d["ssa"] is None and d["cloud"] is None and sc.kn_grid == (sc.nx, sc.ny, sc.nz)
    parts = heat_ranges(be, sc, d, HS.RANGES, HS.SLAB_RAYS)
    truth = HS.slab_truth(sc).sum(axis=0)
    mean, se = TS.standard_error(parts, HS.SLAB_RAYS)
    mean, se = mean.reshape(sc.nz, sc.ncol), se.reshape(sc.nz, sc.ncol)
    dev_cell = np.abs(mean - truth[:, None])/se
    lay_mean, lay_se = TS.standard_error(parts.reshape(HS.RANGES, sc.nz, sc.ncol).sum(axis=2), HS.SLAB_RAYS*sc.ncol)
    dev_lay = np.abs(lay_mean - truth)/lay_se
    print(f"heating slab {dt}: layer means {np.round(lay_mean, 3)} against {np.round(truth, 3)} W m-2; worst deviation "
          f"{float(dev_cell.max()):.2f} standard errors per cell, {float(dev_lay.max()):.2f} of a layer mean (bound 5); largest standard "
          f"error of a cell {100*float(se.max()/np.abs(truth).max()):.2f} % of the largest layer value (bound 2 %)")
    assert np.all(se > 0) and se.max() < 0.02*np.abs(truth).max()
    assert np.all(dev_cell <= 5) and np.all(dev_lay <= 5)


# ---- H2: the energy closure in 3-D

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_h2_the_convergence_of_all_cells_is_the_net_flux_through_the_boundaries(dt, hip_f64, hip_f32):
    """general_lw: cloud, scattering, an emissivity per pixel. sum over the cells of flux_conv / ncol against (F_dn - F_up) at the top
    minus (F_dn - F_up) at the surface, the fluxes from rrx_thermal_render with the two flux sensors (one pixel per column)."""
    be = _be(dt, hip_f64, hip_f32)
    sc = HS.closure_scene(be.np_dtype)
    d = dev(be, sc)
    ngpt, R, total = sc.tau.shape[0], HS.CLOSURE_RAYS, HS.RANGES*HS.CLOSURE_RAYS
    r = heat_render(be, sc, d, np.full(ngpt, total))
    assert r["n_capped"] == 0 and r["n_clamped"] == 0
    conv = float(r["flux_conv"].astype(np.float64).sum())/sc.ncol
    conv_ranges = heat_ranges(be, sc, d, HS.RANGES, R).sum(axis=1)*2.0**-32/R/sc.ncol
    rad, rad_ranges = {}, {}
    for up in (True, False):
        sensor = C.flux_sensor(sc.nx, sc.ny, up=up)
        s = sensor_render(be, sc, d, sensor, total)
        assert s["n_capped"] == 0 and s["n_clamped"] == 0
        rad[up] = be.to_numpy(s["radiance"]).reshape(-1)
        rad_ranges[up] = sum(sensor_ranges(be, sc, d, sensor, g, HS.RANGES, R).astype(np.float64) for g in range(ngpt))*2.0**-32/R
    net = float(HS.boundary_net(sc, rad[True], rad[False]))
    net_ranges = HS.boundary_net(sc, rad_ranges[True], rad_ranges[False])
    se = math.hypot(conv_ranges.std(ddof=1), net_ranges.std(ddof=1))/math.sqrt(HS.RANGES)
    print(f"heating closure {dt}: convergence {conv:.4f}, boundary net {net:.4f} W m-2, difference {conv - net:+.4f} (bound {5*se:.4f}); "
          f"the ranges' means {conv_ranges.mean():.4f}, {net_ranges.mean():.4f}")
    assert se > 0 and abs(conv - net) <= 5*se


# ---- ray for ray

@pytest.mark.parametrize("top_at_1", [False, True])
def test_ray_for_ray_against_the_restatement(top_at_1, hip_f64):
    """3 rays per cell of every g-point on the general scene in fp64: a cell's count within one count per deposit plus 4 eps of the
    sum of |d| of the restatement's (the deposits are made of + - x / only; log, sin, cos and cbrt, which numpy and the device may
    round differently by an ulp, reach them through the weights' products alone)."""
    be = hip_f64
    sc = HS.general(np.float64, top_at_1)
    d = dev(be, sc)
    eps = np.finfo(np.float64).eps
    worst = 0
    for g in range(HS.NGPT):
        ref = H.trace_counts_heating(sc, g, 0, 3*NCELL)
        got = numbers(be, heat(be, sc, d, g, 0, 3*NCELL))
        assert got["n_capped"] == ref["n_capped"] == 0 and got["n_clamped"] == ref["n_clamped"] == 0
        off = np.abs(got["counts"] - ref["counts"])
        tol = ref["n_dep"] + 4*eps*ref["sum_abs"]*2.0**32
        worst = max(worst, int(off.max()))
        assert np.all(off <= tol), (g, int(off.max()))
        assert ref["counts"].any() == (g != HS.EMPTY)
    print(f"heating ray for ray top_at_1={top_at_1}: worst difference {worst} counts of 2^-32 W m-2")


# ---- integers

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_ranges_add_up_and_the_dealing_does_not_matter(dt, hip_f64, hip_f32, monkeypatch):
    """Uneven m_g with their weights, 5 088 rays (20 workgroups): the whole list equals three ranges, cut inside a g-point and on the
    boundary beside the empty range of the dark g-point; a second run; a run on one workgroup; and the per-g-point entry likewise."""
    be = _be(dt, hip_f64, hip_f32)
    sc = HS.general(be.np_dtype)
    d = dev(be, sc)
    m = np.array([24, 4, 0, 17, 8])
    ray_end, w0, _ = H.ray_list(sc, m)
    n = int(ray_end[-1])
    assert n > 4*256 and ray_end[2] == ray_end[3]
    kn = k_null_all(be, sc, d)
    whole = numbers(be, heat_spectral(be, sc, d, (ray_end, w0), 0, n, kn=kn))
    again = numbers(be, heat_spectral(be, sc, d, (ray_end, w0), 0, n, kn=kn))
    assert whole["n_capped"] == 0 and whole["counts"].all() and (whole["counts"] < 0).any() and (whole["counts"] > 0).any()
    for k in KEYS:
        assert np.array_equal(whole[k], again[k]), k
    for cuts in ((0, int(ray_end[1]) - 5, int(ray_end[2]), n), (0, int(ray_end[1]), int(ray_end[3]) + 7, n)):
        parts = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts = heat_spectral(be, sc, d, (ray_end, w0), a, b - a, kn=kn, counts=parts)
        parts = numbers(be, parts)
        for k in KEYS:
            assert np.array_equal(whole[k], parts[k]), (cuts, k)
    one = numbers(be, heat(be, sc, d, 3, 0, 17*NCELL))
    split = numbers(be, heat(be, sc, d, 3, 5*NCELL + 11, 12*NCELL - 11, counts=heat(be, sc, d, 3, 0, 5*NCELL + 11)))
    monkeypatch.setenv("RRX_RT_MAX_BLOCKS", "1")
    deep = numbers(be, heat_spectral(be, sc, d, (ray_end, w0), 0, n, kn=kn))
    one_deep = numbers(be, heat(be, sc, d, 3, 0, 17*NCELL))
    monkeypatch.delenv("RRX_RT_MAX_BLOCKS")
    for k in KEYS:
        assert np.array_equal(whole[k], deep[k]) and np.array_equal(one[k], split[k]) and np.array_equal(one[k], one_deep[k]), k
    # a NULL top_radiance is a top radiance of 0
    dark = numbers(be, heat_spectral(be, sc, d, (ray_end, w0), 0, n, kn=kn, top=None))
    zeros = numbers(be, heat_spectral(be, sc, d, (ray_end, w0), 0, n, kn=kn, top=np.zeros(HS.NGPT)))
    assert np.array_equal(dark["counts"], zeros["counts"]) and np.all(dark["counts"] <= whole["counts"]) and np.any(dark["counts"] < whole["counts"])
    # the binding refuses a list that does not ascend, a range beyond the list and a call without band_lims
    bad = ray_end.copy(); bad[2] = bad[1] - 1
    with pytest.raises(ValueError, match="must not descend"):
        heat_spectral(be, sc, d, (bad, w0), 0, 8, kn=kn)
    with pytest.raises(ValueError, match="beyond the list"):
        heat_spectral(be, sc, d, (ray_end, w0), n - 4, 8, kn=kn)
    with pytest.raises(ValueError, match="needs band_lims"):
        heat_spectral(be, sc, dict(d, lims=None, cloud=None), (ray_end, w0), 0, 8, kn=kn)


@pytest.mark.parametrize("variant", ["cloud", "clear", "null_ssa"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_with_unit_weights_the_spectral_entry_is_the_integer_sum_over_the_g_points(dt, variant, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc = HS.general(be.np_dtype, cloud=variant != "clear", gas_scatters=variant != "null_ssa")
    d = dev(be, sc)
    assert (d["ssa"] is None) == (variant == "null_ssa") and (d["cloud"] is None) == (variant == "clear")
    m = np.array([3, 3, 0, 3, 3])
    ray_end, _, _ = H.ray_list(sc, m)
    got = numbers(be, heat_spectral(be, sc, d, (ray_end, np.ones(HS.NGPT)), 0, int(ray_end[-1])))
    want = None
    for g in HS.ACTIVE:
        want = heat(be, sc, d, g, 0, 3*NCELL, counts=want)
    want = numbers(be, want)
    assert np.array_equal(got["counts"], want["counts"]) and want["counts"].any()
    assert got["n_capped"] == want["n_capped"] == 0 and got["n_clamped"] == want["n_clamped"] == 0


@pytest.mark.parametrize("variant", ["cloud", "null_ssa"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_result_does_not_depend_on_the_chunking_and_the_render_is_the_trace_entry_converted(dt, variant, hip_f64, hip_f32, monkeypatch):
    be = _be(dt, hip_f64, hip_f32)
    sc = HS.general(be.np_dtype, gas_scatters=variant != "null_ssa")
    d = dev(be, sc)
    m = np.array([9, 2, 0, 6, 7])
    monkeypatch.delenv(CHUNK, raising=False)
    whole = heat_render(be, sc, d, m)
    assert whole["n_capped"] == 0 and whole["n_clamped"] == 0 and whole["flux_conv"].all()
    for chunk in ("1", "2"):
        monkeypatch.setenv(CHUNK, chunk)
        got = heat_render(be, sc, d, m)
        assert np.array_equal(whole["flux_conv"].view(np.uint8), got["flux_conv"].view(np.uint8)), chunk
        assert got["n_capped"] == 0 and got["n_clamped"] == 0
    monkeypatch.delenv(CHUNK)
    # HipKernels.thermal_heating_render is the trace entry on the list of ray_list and one conversion with scale = U
    ray_end, w0, U = H.ray_list(sc, m)
    c = numbers(be, heat_spectral(be, sc, d, (ray_end, w0), 0, int(ray_end[-1])))
    by_hand = H.counts_to_flux(c["counts"], U, be.np_dtype)
    assert np.array_equal(by_hand.view(np.uint8), whole["flux_conv"].view(np.uint8))
    # no rays at all: zeroed outputs; a refused list
    none = heat_render(be, sc, d, np.zeros(HS.NGPT, dtype=np.int64))
    assert none["n_capped"] == 0 and not none["flux_conv"].any()
    with pytest.raises(RuntimeError, match="negative at g-point 3"):
        heat_render(be, sc, d, np.array([1, 1, 0, -1, 1]))


@pytest.mark.parametrize("top_at_1", [False, True])
def test_counts_with_uneven_weights_against_the_restatement(top_at_1, hip_f64):
    """Uneven m_g on the general scene: the device and the restatement scale the same s0 by the same weights and make the same
    deposits; where a transcendental of the transport rounds differently a deposit may differ in its last place, far below a count: a
    cell's count may differ by half a count per deposit of that cell, the number of which the restatement returns."""
    be = hip_f64
    sc = HS.general(np.float64, top_at_1)
    d = dev(be, sc)
    m = np.array([40, 3, 0, 15, 6])
    ray_end, w0, _ = H.ray_list(sc, m)
    assert len(set(w0[list(HS.ACTIVE)])) == 4 and w0[HS.EMPTY] == 0
    ref = H.trace_counts_spectral(sc, ray_end, w0, 0, int(ray_end[-1]))
    got = numbers(be, heat_spectral(be, sc, d, (ray_end, w0), 0, int(ray_end[-1])))
    assert ref["n_capped"] == 0 == got["n_capped"] and ref["n_clamped"] == 0 == got["n_clamped"]
    off = np.abs(got["counts"] - ref["counts"])
    print(f"heating spectral against the restatement top_at_1={top_at_1}: worst difference {int(off.max())} counts of 2^-32, "
          f"{int(ref['n_dep'].sum())} deposits, m = {list(m)}")
    assert ref["counts"].all() and np.all(2*off <= ref["n_dep"]), int(off.max())


# ---- the cap

def test_the_cap_is_counted_and_a_capped_ray_keeps_its_deposits(hip_f64):
    be = hip_f64
    sc = HS.general(np.float64)
    m = np.array([3, 1, 0, 2, 2])
    capped = heat_render(be, sc, dev(be, sc), m, max_events=2)
    ref = H.render(sc, m, max_events=2)
    assert 0 < capped["n_capped"] == ref["n_capped"] <= int(m.sum())*NCELL and capped["flux_conv"].any()
    # (half a count per deposit, U <= 1, and the conversion's rounding, which lies far below a count)
    assert np.all(np.abs(capped["flux_conv"] - ref["flux_conv"]) <= (ref["n_dep"] + 1)*2.0**-32)


# ---- the chain

def test_heating_lw_is_the_entry_on_the_chain_s_own_arrays(hip_f64):
    from rte_rrtmgp_cpp_amd import synthetic
    be = hip_f64
    nx, ny, nlay = 4, 4, 12
    kd = be.upload_kdist(synthetic.make_kdist("lw", ngpt=32, nbnd=2, npres=10, nflav=3, nminor_lower=5, nminor_upper=3))
    atm0 = synthetic.make_atmosphere(nx*ny, nlay, nbnd_lw=2, nbnd_sw=2, clouds=True)
    atm0.emis_sfc[:] = atm0.emis_sfc[:, :1]
    atm = pipeline.upload_atmosphere(be, atm0)
    lut = be.upload_lut(synthetic.make_cloud_lut(2, "lw"))
    dz = 70.e3/nlay
    top = np.linspace(0.0, 0.02, 32)
    args = (be, kd, atm, nx, ny, 400.0, 400.0, dz)
    kw = dict(cloud_lut=lut, kn_grid=(2, 2, 3), top_radiance=top)
    seed = HS.TSS.S.SEED

    _, col_gas, _ = pipeline.gas_state(be, kd, atm, None, interpolate=False)
    tau = be.gas_optics_lw_direct(kd, atm.p_lay, atm.t_lay, col_gas, be.empty((32, nlay, nx*ny)))
    src = be.planck_source_direct(kd, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, nlay if atm0.top_at_1 else 1, col_gas)
    cld = be.cloud_optics_2str(lut, atm.lwp, atm.iwp, atm.rel, atm.dei)
    emis = be.asarray(atm0.emis_sfc[:, 0].copy())

    def entry(m):
        return be.thermal_heating_render(tau, None, nx, ny, 400.0, 400.0, dz, emis, src["lay_src"], src["sfc_src"], (2, 2, 3), m, seed,
                                         kd.band_lims_gpt, top_at_1=atm0.top_at_1, cloud=cld, top_radiance=top)

    # allocation=None: every g-point gets rays_per_cell; heating_rate = g/cp flux_conv / |dp| formed on the host
    r = pipeline.heating_lw(*args, 2, seed, p_lev=atm.p_lev, **kw)
    want = entry(np.full(32, 2))
    got = be.to_numpy(r["flux_conv"])
    assert got.shape == (nlay, nx*ny) and r["n_capped"] == 0 and r["n_clamped"] == 0 and np.array_equal(r["rays_per_cell_gpt"], np.full(32, 2))
    assert np.array_equal(got.view(np.uint8), be.to_numpy(want["flux_conv"]).view(np.uint8)) and got.any()
    dp = np.abs(np.diff(be.to_numpy(atm.p_lev).astype(np.float64), axis=0))
    rate = be.to_numpy(r["heating_rate"]).astype(np.float64)
    assert rate.shape == got.shape and np.allclose(rate, 9.80665/1004.64*got/dp, rtol=4*np.finfo(np.float64).eps, atol=0)
    assert "heating_rate" not in pipeline.heating_lw(*args, 2, seed, **kw)
    # allocation="emission": rays_per_cell is the total, dealt by the power that the atmosphere emits
    P = 96
    e = pipeline.absorbed_emission(tau, src["lay_src"], kd.band_lims_gpt, cld)
    tau_abs = be.to_numpy(tau).astype(np.float64)
    lims = be.to_numpy(kd.band_lims_gpt)
    for b in range(2):
        tau_abs[lims[b, 0] - 1:lims[b, 1]] += (be.to_numpy(cld[0][b]).astype(np.float64)*(1.0 - be.to_numpy(cld[1][b]).astype(np.float64)))[None]
    assert np.allclose(e, (tau_abs*be.to_numpy(src["lay_src"]).astype(np.float64)).reshape(32, -1).sum(axis=1), rtol=1e-12)
    m = pipeline.spectral_allocation(e, P)
    assert int(m.sum()) == P and m.min() >= 1 and m.max() > m.min()
    r = pipeline.heating_lw(*args, P, seed, allocation="emission", **kw)
    assert np.array_equal(r["rays_per_cell_gpt"], m)
    assert np.array_equal(be.to_numpy(r["flux_conv"]).view(np.uint8), be.to_numpy(entry(m)["flux_conv"]).view(np.uint8))
    with pytest.raises(ValueError, match="cannot give 4 to each of 32"):
        pipeline.heating_lw(*args, P, seed, allocation="emission", min_per_gpt=4, **kw)
    with pytest.raises(ValueError, match="allocation is None or 'emission'"):
        pipeline.heating_lw(*args, P, seed, allocation="flux", **kw)
    with pytest.raises(ValueError, match="g-point 1 has no emission in the atmosphere"):
        pipeline.heating_allocation([1., 0., 2.], [1., 1., 1.], None, 8)
    with pytest.raises(ValueError, match="g-point 2 has no emission in the atmosphere"):
        pipeline.heating_allocation([1., 2., 0.], [1., 1., 0.], [0., 0., 0.5], 8)
    assert list(pipeline.heating_allocation([1., 0., 3.], [1., 0., 1.], None, 8)) == [2, 0, 6]


# ---- the C++ class

@pytest.mark.parametrize("variant", ["cloud", "null_ssa"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_cxx_class_gives_the_entry_bit_for_bit_and_throws(dt, variant, hip_f64, hip_f32):
    """Raytracer_thermal_gpu::trace_heating (through rrx_cxx_trace_heating, which wraps the caller's device arrays in Array_gpu views)
    against rrx_heating3d_render; a refusal of the entry arrives as an exception's message."""
    import torch
    be = _be(dt, hip_f64, hip_f32)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so" if dt == "f64" else "librte_rrtmgp_hip_sp.so"))
    lib.rrx_cxx_driver_error.restype = ctypes.c_char_p
    F = ctypes.c_double if dt == "f64" else ctypes.c_float
    sc = HS.general(be.np_dtype, cloud=variant == "cloud", gas_scatters=variant != "null_ssa")
    d = dev(be, sc)
    top = np.ascontiguousarray(sc.top_radiance, dtype=be.np_dtype)
    Hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    none = ctypes.c_void_p(0)
    P = lambda t: none if t is None else ctypes.c_void_p(t.data_ptr())
    flux_conv = be.empty((sc.nz, sc.ncol))
    n_capped, n_clamped = ctypes.c_ulonglong(99), ctypes.c_ulonglong(99)
    cloud = (none, none, none) if d["cloud"] is None else tuple(P(c) for c in d["cloud"])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(m, knx=sc.kn_grid[0]):
        m = np.ascontiguousarray(m, dtype=np.int64)
        return lib.rrx_cxx_trace_heating(sc.nx, sc.ny, sc.nz, HS.NGPT, HS.NBND, F(sc.dx), F(sc.dy), F(sc.dz), int(sc.top_at_1),
                                         P(d["tau"]), P(d["ssa"]), P(d["lims"]), *cloud, P(d["emis"]), P(d["lay_src"]), P(d["sfc_src"]), Hp(top),
                                         knx, sc.kn_grid[1], sc.kn_grid[2], Hp(m), ctypes.c_ulonglong(sc.seed), be.RT_MAX_EVENTS,
                                         P(flux_conv), ctypes.byref(n_capped), ctypes.byref(n_clamped), stream)

    m = np.array([5, 1, 0, 2, 2])
    want = heat_render(be, sc, d, m)
    assert call(m) == 0, lib.rrx_cxx_driver_error().decode()
    torch.cuda.synchronize()
    assert n_capped.value == 0 == want["n_capped"] and n_clamped.value == 0 == want["n_clamped"]
    got = be.to_numpy(flux_conv).reshape(-1)
    assert np.array_equal(got.view(np.uint8), want["flux_conv"].view(np.uint8)) and want["flux_conv"].all()
    assert call(np.array([1, -1, 0, 1, 1])) != 0
    msg = lib.rrx_cxx_driver_error().decode()
    assert "rrx_heating3d_render" in msg and "negative at g-point 1" in msg, msg
    assert call(m, knx=3) != 0
    assert "knx does not divide nx" in lib.rrx_cxx_driver_error().decode()
