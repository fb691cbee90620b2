"""GPU tests of thermal emission in the backward Monte Carlo ray tracer (csrc/rrx_raytracer_thermal.hip). Scenes and
sensors: tests/thermal_scenes.py (grids of 8x4x6 cells, two g-points, fixed seeds); the tallies are integers added with integer
atomics, so a run that passes once passes always. Bounds are derived, not measured:
  T1, T2, T3  five standard errors of 16 disjoint ray ranges (the estimate is a mean over independent rays); T1 adds, in quadrature,
              the reference's own standard error of the reflected term (thermal_scenes.schwarzschild_expected, the first of the two
              ways to treat that term: it is included, for every column);
  ray for ray one count per deposit plus 4 eps of the deposited sum, the bound of test_gpu_raytracer_bw.py::test_ray_for_ray (the
              deposits here are made of + - x / only; log, sin, cos and cbrt, which numpy and the device may round differently by an
              ulp, reach them through the weights' products alone);
  by band     nbnd eps of the sum.
test_raytracer_thermal_ref.py holds, on the CPU, that the ray counts used here put the restatement's standard error below 1 % of the
expected radiance, so that the statistical bounds are not vacuous."""
import ctypes
import math
import os

import numpy as np
import pytest

import raytracer_thermal_ref as T
import thermal_scenes as TS
from raytracer_thermal_dev import _be, _u64, dev, k_null, trace, render, clean, ranges
from rte_rrtmgp_cpp_amd import synthetic, pipeline, camera as C

pytestmark = pytest.mark.gpu
_EXPECTED, _PARTS = {}, {}


def expected_t1(g):
    if g not in _EXPECTED:
        _EXPECTED[g] = TS.schwarzschild_expected(TS.clear_columns(np.float64), g)
    return _EXPECTED[g]


def cavity_parts(be, dt, name, g):
    """the cavity's counts of RANGES ranges under one of its sensors, traced once for T2 and T3"""
    if (dt, name, g) not in _PARTS:
        sc = TS.cavity(be.np_dtype)
        _PARTS[dt, name, g] = ranges(be, sc, dev(be, sc), TS.cavity_sensors()[name], g, TS.RANGES, TS.CAVITY_RAYS//TS.RANGES)
    return _PARTS[dt, name, g]


# ---- T1: Schwarzschild's solution of clear columns under a nadir view

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_t1_schwarzschild(dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc = TS.clear_columns(be.np_dtype)
    d = dev(be, sc)
    assert d["ssa"] is None                     # the gas does not scatter: a NULL ssa
    sensor = C.orthographic(sc.nx, sc.ny)
    for g in range(2):
        want, se_want = expected_t1(g)
        got, se = TS.standard_error(ranges(be, sc, d, sensor, g, TS.RANGES, TS.T1_RAYS//TS.RANGES), TS.T1_RAYS//TS.RANGES)
        bound = 5.0*np.sqrt(se*se + se_want*se_want)
        print(f"thermal T1 {dt} g={g}: worst difference/bound {float(np.max(np.abs(got - want)/bound)):.2f}, radiance {want.min():.3f} .. "
              f"{want.max():.3f} W m-2 sr-1, standard error up to {float(np.max(se/want)):.4f} of it")
        assert np.all(se > 0) and np.all(se < 0.02*want)
        assert np.all(np.abs(got - want) <= bound)


# ---- T2: the black-body cavity

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", list(TS.cavity_sensors()))
def test_t2_cavity(name, dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    for g in range(2):
        got, se = TS.standard_error(cavity_parts(be, dt, name, g), TS.CAVITY_RAYS//TS.RANGES)
        print(f"thermal T2 {dt} {name} g={g}: radiance/S_g {float(got.min()/TS.S_G[g]):.4f} .. {float(got.max()/TS.S_G[g]):.4f}, standard "
              f"error up to {float(se.max()/TS.S_G[g]):.4f} S_g, worst difference {float(np.max(np.abs(got - TS.S_G[g])/se)):.2f} of it")
        # the bound is not vacuous: the restatement's standard error is below 0.01 S_g (held on the CPU); one estimated from 16 ranges
        # scatters by 1/sqrt(2 x 15) = 18 % of itself, and 0.02 S_g lies five of those above it
        assert np.all(se > 0) and np.all(se < 0.02*TS.S_G[g])
        assert np.all(np.abs(got - TS.S_G[g]) <= 5.0*se)


# ---- T3: the units, against the 1-D solver

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_t3_flux_against_the_1d_solver(dt, hip_f64, hip_f32):
    """rrx_lw_solver_noscat on the cavity's sources, lev_src = lay_src, sfc_emis = 1, no cloud, column by column: its upward flux at
    the top is pi S_g (one angle of weight 1: flux = pi w radiance). pi x the radiance of the flux sensor that faces down from the
    top of the cavity is that flux."""
    be = _be(dt, hip_f64, hip_f32)
    sc = TS.cavity_black(be.np_dtype)
    d = dev(be, sc)
    ngpt, nz, ncol = sc.tau.shape
    lev = np.concatenate([sc.lay_src, sc.lay_src[:, :1]], axis=1)
    secants = be.lw_secants_array(ncol, ngpt, 1, pipeline.MAX_GAUSS_PTS, be.asarray(pipeline.GAUSS_DS))
    weights = be.asarray(np.ascontiguousarray(pipeline.GAUSS_WTS[0, :1]))
    r = be.lw_solver_noscat(sc.top_at_1, secants, weights, d["tau"], d["lay_src"], be.asarray(lev), be.asarray(np.ones((ngpt, ncol), dtype=be.np_dtype)),
                            d["sfc_src"])
    up = be.to_numpy(r["flux_up"])[:, 0 if sc.top_at_1 else nz, :].astype(np.float64)
    for g in range(2):
        assert np.allclose(up[g], math.pi*TS.S_G[g], rtol=1e-5)
        got, se = TS.standard_error(cavity_parts(be, dt, "flux_down", g), TS.CAVITY_RAYS//TS.RANGES)
        print(f"thermal T3 {dt} g={g}: solver {up[g].mean():.4f} W m-2, sensor {math.pi*got.min():.4f} .. {math.pi*got.max():.4f}, worst "
              f"difference {float(np.max(np.abs(math.pi*got - up[g].mean())/(math.pi*se))):.2f} standard errors")
        assert np.all(np.abs(math.pi*got - up[g].mean()) <= 5.0*math.pi*se)


# ---- ray for ray against the numpy restatement

def ray_for_ray(be, sc, sensor, rpp, label):
    ref = T.render(sc, sensor, rpp)
    assert ref["n_capped"] == 0 and ref["n_clamped"] == 0
    r = render(be, sc, dev(be, sc), sensor, rpp)
    assert r["n_capped"] == 0 and r["n_clamped"] == 0
    got = be.to_numpy(r["radiance"]).reshape(-1)
    eps = np.finfo(np.float64).eps
    tol = np.sum(ref["n_dep"] * 2.0**-32 + 4*eps*ref["sum_d"], axis=0) / rpp
    err = np.abs(got - ref["radiance"])
    print(f"thermal ray for ray {label}: max difference {float(err.max()):.3e} W m-2 sr-1 (bound there {float(tol[np.argmax(err)]):.3e}), "
          f"worst difference/bound {float(np.max(err/tol)):.3f}, radiance {float(ref['radiance'].min()):.3f} .. "
          f"{float(ref['radiance'].max()):.3f}, {int(ref['deposits'].sum())} deposits in {int(ref['events'].sum())} events")
    assert np.all(ref["radiance"] > 0)
    assert np.all(err <= tol)


@pytest.mark.parametrize("kind", list(TS.sensors(6, 4)))
def test_ray_for_ray(kind, hip_f64):
    ray_for_ray(hip_f64, TS.general_lw(np.float64), TS.sensors(6, 4)[kind], 32, kind)


def test_ray_for_ray_from_above_the_top(hip_f64):
    """a camera above the domain top whose upper pixel rows look away from the medium: those rays end at once with top_radiance, the
    others are moved along the ray to the top"""
    cam = C.perspective(6, 4, (330., 250., 500.), yaw=0.6, pitch=-0.15, fov=math.radians(70.))
    sc = TS.general_lw(np.float64)
    away = T.trace_counts_thermal(sc, cam, 0, 0, 32*cam.npix)
    assert 0 < away["events"] and np.any(away["counts"] == 32*int(np.rint(1.5 * 2.0**32)))          # (pixels that see the top radiance alone)
    ray_for_ray(hip_f64, sc, cam, 32, "perspective from above")


def test_ray_for_ray_with_a_null_ssa_and_from_the_top_down(hip_f64):
    """clear_columns (NULL ssa, no cloud) under the flux sensor that faces down: the starts at the top, and the restatement's zeros
    for ssa against the device's NULL"""
    ray_for_ray(hip_f64, TS.clear_columns(np.float64), C.flux_sensor(6, 4, up=False), 32, "clear_columns flux_down")


# ---- integers

def test_counts_are_additive_and_reproducible(hip_f64):
    be = hip_f64
    sc = TS.general_lw(np.float64)
    d = dev(be, sc)
    sensor = TS.sensors(6, 4)["perspective"]
    n = 32*sensor.npix
    kn = k_null(be, sc, d, 1)
    whole = trace(be, sc, d, sensor, 1, 0, n, kn=kn)
    again = trace(be, sc, d, sensor, 1, 0, n, kn=kn)
    parts = trace(be, sc, d, sensor, 1, 0, n//3, kn=kn)
    parts = trace(be, sc, d, sensor, 1, n//3, n - n//3, kn=kn, counts=parts)
    for k in ("counts", "n_capped", "n_clamped"):
        assert np.array_equal(_u64(be, whole[k]), _u64(be, again[k])), k
        assert np.array_equal(_u64(be, whole[k]), _u64(be, parts[k])), k
    assert clean(be, whole).all()


def test_deep_ray_lists_on_few_threads_give_the_same_integers(hip_f64, monkeypatch):
    """With the launch capped at one workgroup the 768 rays are three per thread, taken inside the event loop."""
    be = hip_f64
    sc = TS.general_lw(np.float64)
    d = dev(be, sc)
    sensor = TS.sensors(6, 4)["fisheye"]
    n = 32*sensor.npix
    wide = trace(be, sc, d, sensor, 0, 5, n)
    monkeypatch.setenv("RRX_RT_MAX_BLOCKS", "1")
    deep = trace(be, sc, d, sensor, 0, 5, n)
    monkeypatch.delenv("RRX_RT_MAX_BLOCKS")
    for k in ("counts", "n_capped", "n_clamped"):
        assert np.array_equal(_u64(be, wide[k]), _u64(be, deep[k])), k
    assert clean(be, wide).any()


# ---- bits

def hand_loop(be, sc, d, sensor, rpp):
    """The loop of rrx_thermal_render made of the small entries: radiance by g-point, (ngpt, npix), and their sum in g-point order."""
    F = be.np_dtype.type
    total = be.zeros((sensor.npix,))
    per_g = []
    for g in range(sc.tau.shape[0]):
        c = trace(be, sc, d, sensor, g, 0, rpp*sensor.npix)
        clean(be, c)
        scale = float(F(1.)/F(rpp))
        be.rt_counts_to_flux(c["counts"], scale, total)
        per_g.append(be.to_numpy(be.rt_counts_to_flux(c["counts"], scale, be.zeros((sensor.npix,)))))
    return be.to_numpy(total), np.stack(per_g)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_loop_is_the_entries_and_the_bands_add_up(dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc = TS.general_lw(be.np_dtype)
    d = dev(be, sc)
    sensor = TS.sensors(6, 4)["orthographic"]
    rpp = 24
    total, per_g = hand_loop(be, sc, d, sensor, rpp)
    r = render(be, sc, d, sensor, rpp)
    assert r["radiance"].shape == (sensor.npy, sensor.npx) and r["n_capped"] == 0 and r["n_clamped"] == 0
    assert np.array_equal(total.view(np.uint8), be.to_numpy(r["radiance"]).reshape(-1).view(np.uint8))
    # by band: every g-point of these scenes is a band of its own
    b = render(be, sc, d, sensor, rpp, by_band=True)
    assert b["radiance"].shape == (2, sensor.npy, sensor.npx)
    rows = be.to_numpy(b["radiance"]).reshape(2, -1)
    assert np.array_equal(rows.view(np.uint8), per_g.view(np.uint8))
    assert np.all(np.abs(rows.astype(np.float64).sum(axis=0) - total) <= 2*np.finfo(be.np_dtype).eps*total)
    # a g-point of no band is dropped: in a scene without cloud, with band 0 holding g-point 1 alone, row 0 is g-point 1's
    clear = TS.clear_columns(be.np_dtype)
    dc = dev(be, clear)
    _, clear_g = hand_loop(be, clear, dc, sensor, rpp)
    one = render(be, clear, dc, sensor, rpp, by_band=True, lims=be.asarray(np.array([[2, 2], [9, 9]], dtype=np.int32)))
    got = be.to_numpy(one["radiance"]).reshape(2, -1)
    assert np.array_equal(got[0].view(np.uint8), clear_g[1].view(np.uint8)) and not got[1].any()
    with pytest.raises(ValueError, match="by_band"):
        render(be, clear, dc, sensor, rpp, by_band=True, lims=None)
    # without a top radiance less comes down
    dark = be.thermal_render(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["emis"], d["lay_src"], d["sfc_src"], sc.kn_grid, sensor, rpp,
                             sc.seed, top_at_1=sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"])
    assert np.all(be.to_numpy(dark["radiance"]).reshape(-1) <= total) and np.any(be.to_numpy(dark["radiance"]).reshape(-1) < total)


def test_the_cap_is_counted(hip_f64):
    be = hip_f64
    sc = TS.general_lw(np.float64)
    sensor = TS.sensors(6, 4)["orthographic"]
    capped = render(be, sc, dev(be, sc), sensor, 8, max_events=1)
    assert 0 < capped["n_capped"] == T.render(sc, sensor, 8, max_events=1)["n_capped"] <= 2*8*sensor.npix


# ---- the chain and the C++ class

def test_render_lw_is_the_entry_on_the_chain_s_own_arrays(hip_f64):
    """pipeline.render_lw with a cloud table and a coarse k_null grid: the clear LW gas optics, the Planck sources and the band cloud
    optics of the LW table, made by hand here, give rrx_thermal_render the same bits; channels are the band radiances through one
    matmul."""
    be = hip_f64
    nx, ny, nlay, rpp = 4, 4, 12, 8
    kd = be.upload_kdist(synthetic.make_kdist("lw", ngpt=32, nbnd=2, npres=10, nflav=3, nminor_lower=5, nminor_upper=3))
    atm0 = synthetic.make_atmosphere(nx*ny, nlay, nbnd_lw=2, nbnd_sw=2, clouds=True)
    atm0.emis_sfc[:] = atm0.emis_sfc[:, :1]
    atm = pipeline.upload_atmosphere(be, atm0)
    lut = be.upload_lut(synthetic.make_cloud_lut(2, "lw"))
    dz = 70.e3/nlay
    cam = C.perspective(5, 3, (800., 700., 20.e3), yaw=0.4, pitch=-1.0, fov=math.radians(50.))
    top = np.linspace(0.0, 0.02, 32)
    args = (be, kd, atm, nx, ny, 400.0, 400.0, dz, cam, rpp, TS.SEED)
    r = pipeline.render_lw(*args, cloud_lut=lut, kn_grid=(2, 2, 3), top_radiance=top)
    assert r["n_capped"] == 0 and r["n_clamped"] == 0 and r["radiance"].shape == (3, 5)

    _, col_gas, _ = pipeline.gas_state(be, kd, atm, None, interpolate=False)
    tau = be.gas_optics_lw_direct(kd, atm.p_lay, atm.t_lay, col_gas, be.empty((32, nlay, nx*ny)))
    src = be.planck_source_direct(kd, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, nlay if atm0.top_at_1 else 1, col_gas)
    cld = be.cloud_optics_2str(lut, atm.lwp, atm.iwp, atm.rel, atm.dei)
    emis = be.asarray(atm0.emis_sfc[:, 0].copy())
    scene = (tau, None, nx, ny, 400.0, 400.0, dz, emis, src["lay_src"], src["sfc_src"], (2, 2, 3), cam, rpp, TS.SEED)
    kw = dict(top_at_1=atm0.top_at_1, cloud=cld, band_lims=kd.band_lims_gpt, top_radiance=top)
    want = be.thermal_render(*scene, **kw)
    assert np.array_equal(be.to_numpy(r["radiance"]).view(np.uint8), be.to_numpy(want["radiance"]).view(np.uint8))
    assert float(r["radiance"].min()) > 0
    bands = pipeline.render_lw(*args, cloud_lut=lut, kn_grid=(2, 2, 3), top_radiance=top, channels="bands")
    want = be.thermal_render(*scene, **kw, by_band=True)
    assert bands["radiance"].shape == (2, 3, 5)
    assert np.array_equal(be.to_numpy(bands["radiance"]).view(np.uint8), be.to_numpy(want["radiance"]).view(np.uint8))
    M = np.array([[1.0, 1.0], [0.25, 0.0], [0.0, 2.0]])
    chan = be.to_numpy(pipeline.render_lw(*args, cloud_lut=lut, kn_grid=(2, 2, 3), top_radiance=top, channels=M)["radiance"])
    rows = be.to_numpy(want["radiance"]).astype(np.float64)
    assert chan.shape == (3, 3, 5) and np.allclose(chan, np.einsum("cb,bij->cij", M, rows), rtol=1e-13, atol=0)
    # a flux sensor: pi x radiance is the surface's downwelling irradiance
    flux = pipeline.render_lw(be, kd, atm, nx, ny, 400.0, 400.0, dz, C.flux_sensor(nx, ny, up=True), rpp, TS.SEED, cloud_lut=lut)
    down = math.pi*be.to_numpy(flux["radiance"])
    assert down.shape == (ny, nx) and down.min() > 0
    # the columns are the pixels, and one emissivity per pixel
    with pytest.raises(ValueError, match="nx ny"):
        pipeline.render_lw(be, kd, atm, nx, ny + 1, 400.0, 400.0, dz, cam, rpp, TS.SEED)
    with pytest.raises(ValueError, match="channels"):
        pipeline.render_lw(*args, channels="colour")
    atm0.emis_sfc[3, 1] *= 0.9
    with pytest.raises(ValueError, match="emissivity"):
        pipeline.render_lw(be, kd, pipeline.upload_atmosphere(be, atm0), nx, ny, 400.0, 400.0, dz, cam, rpp, TS.SEED)


@pytest.mark.parametrize("by_band", [0, 1])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_raytracer_thermal_gpu_class_gives_the_entry_bit_for_bit_and_throws(dt, by_band, hip_f64, hip_f32):
    """Raytracer_thermal_gpu::trace_rays_thermal (through rrx_cxx_trace_rays_thermal, which wraps the caller's device arrays in
    Array_gpu views) against rrx_thermal_render on general_lw; a refused argument comes back as an exception's message."""
    import torch
    be = _be(dt, hip_f64, hip_f32)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so" if dt == "f64" else "librte_rrtmgp_hip_sp.so"))
    lib.rrx_cxx_driver_error.restype = ctypes.c_char_p
    F = ctypes.c_double if dt == "f64" else ctypes.c_float
    sc = TS.general_lw(be.np_dtype)
    d = dev(be, sc)
    sensor = TS.sensors(6, 4)["perspective"]
    rpp = 16
    want = render(be, sc, d, sensor, rpp, by_band=bool(by_band))
    out = be.empty((2, sensor.npy, sensor.npx) if by_band else (sensor.npy, sensor.npx))
    top = np.ascontiguousarray(sc.top_radiance, dtype=be.np_dtype)
    numbers = sensor.numbers(be.np_dtype)
    n_capped, n_clamped = ctypes.c_ulonglong(99), ctypes.c_ulonglong(99)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(sensor_type):
        return lib.rrx_cxx_trace_rays_thermal(sc.nx, sc.ny, sc.nz, 2, 2, F(sc.dx), F(sc.dy), F(sc.dz), int(sc.top_at_1),
                                              P(d["tau"]), P(d["ssa"]), P(d["lims"]), *(P(c) for c in d["cloud"]), P(d["emis"]),
                                              P(d["lay_src"]), P(d["sfc_src"]), top.ctypes.data_as(ctypes.c_void_p), *sc.kn_grid, sensor_type,
                                              sensor.npx, sensor.npy, F(sensor.fov), numbers.ctypes.data_as(ctypes.c_void_p),
                                              ctypes.c_longlong(rpp), ctypes.c_ulonglong(sc.seed), be.RT_MAX_EVENTS, by_band, P(out),
                                              ctypes.byref(n_capped), ctypes.byref(n_clamped),
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert call(sensor.type) == 0, lib.rrx_cxx_driver_error().decode()
    torch.cuda.synchronize()
    assert n_capped.value == 0 and n_clamped.value == 0 and want["n_capped"] == 0
    assert np.array_equal(be.to_numpy(out).view(np.uint8), be.to_numpy(want["radiance"]).view(np.uint8))
    assert call(7) != 0
    msg = lib.rrx_cxx_driver_error().decode()
    assert "rrx_thermal_render" in msg and "sensor_type" in msg, msg
