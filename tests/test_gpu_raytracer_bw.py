"""GPU tests of the backward Monte Carlo ray tracer (csrc/rrx_raytracer_bw.hip). Scenes, sensors and comparisons:
tests/raytracer_bw_scenes.py (grids of 8x4x6 cells, two g-points, fixed seeds); the tallies are integers added with integer
atomics, so a run that passes once passes always. Bounds are derived, not measured: S1 the Bernoulli bound sqrt(p (1 - p)/N), S2
integers, S3 the forward tracer's derived bound combined with the standard error of 16 disjoint ray ranges, five sigma each; ray
for ray one count per deposit plus 4 eps of the deposited sum (two exp implementations within 1 ulp each; no decision depends on
exp).

Observed on an MI355X: see DESIGN.md 4.15."""
import ctypes
import math
import os

import numpy as np
import pytest

import raytracer_ref as R
import raytracer_bw_ref as B
import raytracer_scenes as FS
import raytracer_bw_scenes as S
from raytracer_dev import _be, _dev, _u64, k_null, backward, solve_bw
from rte_rrtmgp_cpp_amd import synthetic, pipeline, camera as C

pytestmark = pytest.mark.gpu
ONE = float(1 << 32)


def clean(be, c):
    """the counts as uint64 after asserting that nothing was capped or clamped"""
    assert int(_u64(be, c["n_capped"])[0]) == 0 and int(_u64(be, c["n_clamped"])[0]) == 0
    return _u64(be, c["counts"])


def hand_loop(be, sc, d, sensor, rpp):
    """The spectral loop of rrx_raytracer_bw made of the small entries: (radiance (npix,), per-g-point counts or None)."""
    F = be.np_dtype.type
    npix = sensor.npx*sensor.npy
    radiance = be.zeros((npix,))
    per_g = []
    for g in range(sc.tau.shape[0]):
        if not F(sc.inc_dir[g]) > 0:
            per_g.append(None)
            continue
        c = backward(be, sc, d, sensor, g, 0, rpp*npix)
        be.rt_counts_to_flux(c["counts"], float(F(sc.inc_dir[g]) / (F(sc.mu0)*F(rpp))), radiance)
        per_g.append(clean(be, c))
    return be.to_numpy(radiance), per_g


# ---- S1: the Bernoulli surface

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("view", ["nadir", "slant"])
def test_s1_bernoulli_surface(view, dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc = S.bernoulli(be.np_dtype)
    d = _dev(be, sc)
    sensor = S.bernoulli_sensors()[view]
    for g in range(2):
        counts = clean(be, backward(be, sc, d, sensor, g, 0, S.S1_RAYS*16))
        S.check_bernoulli(sc, sensor, g, counts, f"{dt} {view}")


# ---- S2: the shadow, in integers

@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("along", ["x", "y"])
def test_s2_shadow_in_integers(along, top_at_1, hip_f64):
    be = hip_f64
    sc = S.shadow(np.float64, along, top_at_1)
    dark, full = S.shadow_classes(sc)
    assert dark.sum() == 10 and full.sum() == sc.ncol - 14
    rays = 256
    counts = clean(be, backward(be, sc, _dev(be, sc), C.orthographic(sc.nx, sc.ny), 0, 0, rays*sc.ncol))
    assert np.all(counts[dark] == 0), counts[dark] / ONE
    assert rays*int(np.rint(0.5*sc.mu0/math.pi*ONE)) == S.shadow_full_count(sc, rays)
    assert np.all(counts[full] == S.shadow_full_count(sc, rays)), counts[full] / ONE
    assert np.all(counts[~dark & ~full] <= S.shadow_full_count(sc, rays))


# ---- S3: forward against backward

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_s3_forward_against_backward(dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc = S.general_direct(be.np_dtype)
    d = _dev(be, sc)
    per_range = (S.S3_RAYS//S.S3_RANGES)*sc.ncol
    worst = 0.0
    for g in range(2):
        kn = k_null(be, sc, d, g)
        fwd = be.rt_trace_counts(d["tau"], d["ssa"], g, sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, float(sc.inc_dir[g]),
                                 0.0, sc.kn_grid, kn, sc.seed, 0, S.S3_PHOTONS*sc.ncol, top_at_1=sc.top_at_1, cloud=d["cloud"],
                                 band_lims=d["lims"])
        assert int(_u64(be, fwd["n_capped"])[0]) == 0
        for name, sensor in S.flux_sensors(sc).items():
            parts = np.stack([clean(be, backward(be, sc, d, sensor, g, r*per_range, per_range, kn=kn)) for r in range(S.S3_RANGES)])
            worst = max(worst, S.compare_forward_backward(sc, g, name, _u64(be, fwd[name]), parts, dt))
    print(f"raytracer_bw S3 {dt}: worst {worst:.2f} combined sigma (bound 5)")


# ---- ray for ray against the numpy restatement

SENSORS = {"perspective": lambda: C.perspective(6, 4, (330., 250., 170.), yaw=0.6, pitch=-0.5, roll=0.2, fov=math.radians(70.)),
           "fisheye": lambda: C.fisheye(6, 4, (420., 130., 0.)),
           "orthographic": lambda: C.orthographic(6, 4, yaw=2.0, pitch=-1.0)}


@pytest.mark.parametrize("kind", list(SENSORS))
def test_ray_for_ray(kind, hip_f64):
    be = hip_f64
    sc = FS.general(np.float64)
    sensor = SENSORS[kind]()
    rpp = 32
    ref = B.raytracer_bw(sc, sensor, rpp)
    assert ref["n_capped"] == 0 and ref["n_clamped"] == 0
    r = solve_bw(be, sc, _dev(be, sc), sensor, rpp)
    assert r["n_capped"] == 0 and r["n_clamped"] == 0
    got = be.to_numpy(r["radiance"]).reshape(-1)
    eps = np.finfo(np.float64).eps
    scale = sc.inc_dir.astype(np.float64) / float(sc.mu0) / rpp
    tol = np.sum((ref["n_dep"] * 2.0**-32 + 4*eps*ref["sum_d"]) * scale[:, None], axis=0)
    err = np.abs(got - ref["radiance"])
    print(f"raytracer_bw ray for ray {kind}: max difference {float(err.max()):.3e} W m-2 sr-1 (bound there "
          f"{float(tol[np.argmax(err)]):.3e}), worst difference/bound {float(np.max(err/tol)):.3f}, radiance "
          f"{float(ref['radiance'].min()):.3f} .. {float(ref['radiance'].max()):.3f}, {int(ref['n_dep'].sum())} deposits")
    assert np.all(ref["radiance"] > 0)
    assert np.all(err <= tol)


# ---- counts

def test_counts_are_additive_reproducible_and_the_loop_is_the_entry(hip_f64):
    be = hip_f64
    sc = FS.general(np.float64)
    d = _dev(be, sc)
    sensor = SENSORS["perspective"]()
    n = 32*sensor.npix
    kn = k_null(be, sc, d, 1)
    whole = backward(be, sc, d, sensor, 1, 0, n, kn=kn)
    again = backward(be, sc, d, sensor, 1, 0, n, kn=kn)
    parts = backward(be, sc, d, sensor, 1, 0, n//3, kn=kn)
    parts = backward(be, sc, d, sensor, 1, n//3, n - n//3, kn=kn, counts=parts)
    for k in ("counts", "n_capped", "n_clamped"):
        assert np.array_equal(_u64(be, whole[k]), _u64(be, again[k])), k
        assert np.array_equal(_u64(be, whole[k]), _u64(be, parts[k])), k
    assert clean(be, whole).all()
    rpp = 32
    radiance, _ = hand_loop(be, sc, d, sensor, rpp)
    r = solve_bw(be, sc, d, sensor, rpp)
    assert r["radiance"].shape == (sensor.npy, sensor.npx)
    assert np.array_equal(radiance.view(np.uint8), be.to_numpy(r["radiance"]).reshape(-1).view(np.uint8))


def test_a_g_point_without_incident_flux_is_skipped_and_the_cap_is_counted(hip_f64):
    be = hip_f64
    sc = FS.general(np.float64)
    d = _dev(be, sc)
    sensor = SENSORS["orthographic"]()
    one = FS.general(np.float64)
    one.inc_dir = np.array([sc.inc_dir[0], 0.0])
    radiance, per_g = hand_loop(be, one, d, sensor, 8)
    assert per_g[1] is None and per_g[0].any()
    r = solve_bw(be, one, d, sensor, 8)
    assert np.array_equal(radiance.view(np.uint8), be.to_numpy(r["radiance"]).reshape(-1).view(np.uint8))
    # one event each: every ray that the first event does not end is dropped and counted, none loops
    capped = solve_bw(be, sc, d, sensor, 8, max_events=1)
    assert 0 < capped["n_capped"] == B.raytracer_bw(sc, sensor, 8, max_events=1)["n_capped"] <= 2*8*sensor.npix


def test_deep_ray_lists_on_few_threads_give_the_same_integers(hip_f64, monkeypatch):
    """With the launch capped at one workgroup the 768 rays are three per thread, taken inside the event loop, where a lane may
    also be walking to the sun; the counts are those of one ray per thread."""
    be = hip_f64
    sc = FS.general(np.float64)
    d = _dev(be, sc)
    sensor = SENSORS["fisheye"]()
    n = 32*sensor.npix
    wide = backward(be, sc, d, sensor, 0, 5, n)
    monkeypatch.setenv("RRX_RT_MAX_BLOCKS", "1")
    deep = backward(be, sc, d, sensor, 0, 5, n)
    monkeypatch.delenv("RRX_RT_MAX_BLOCKS")
    for k in ("counts", "n_capped", "n_clamped"):
        assert np.array_equal(_u64(be, wide[k]), _u64(be, deep[k])), k
    assert clean(be, wide).any()


# ---- the chain and the C++ class

def test_render_sw_is_the_entry_on_the_chain_s_own_arrays(hip_f64):
    """pipeline.render_sw with a cloud table and a coarse k_null grid: the clear gas optics, the band cloud optics without delta
    scaling and inc_dir = solar_source tsi_scaling mu0, made by hand here, give rrx_raytracer_bw the same bits."""
    be = hip_f64
    nx, ny, nlay, rpp = 4, 4, 12, 8
    kd = be.upload_kdist(synthetic.make_kdist("sw", ngpt=32, nbnd=2, npres=10, nflav=3, nminor_lower=5, nminor_upper=3))
    atm0 = synthetic.make_atmosphere(nx*ny, nlay, nbnd_lw=2, nbnd_sw=2, clouds=True)
    atm = pipeline.upload_atmosphere(be, atm0)
    lut = be.upload_lut(synthetic.make_cloud_lut(2, "sw"))
    dz = 70.e3/nlay
    cam = C.perspective(5, 3, (800., 700., 20.e3), yaw=0.4, pitch=-1.0, fov=math.radians(50.))
    r = pipeline.render_sw(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, cam, rpp, FS.SEED, cloud_lut=lut, kn_grid=(2, 2, 3))
    assert r["n_capped"] == 0 and r["n_clamped"] == 0 and r["radiance"].shape == (3, 5)

    _, col_gas, _ = pipeline.gas_state(be, kd, atm, None, interpolate=False)
    col_dry = be.get_col_dry(atm.vmr["h2o"], atm.p_lev)
    tau, ssa = be.empty((32, nlay, nx*ny)), be.empty((32, nlay, nx*ny))
    be.gas_optics_sw_direct(kd, atm.p_lay, atm.t_lay, col_gas, col_dry, tau, ssa, None)
    cld = be.cloud_optics_2str(lut, atm.lwp, atm.iwp, atm.rel, atm.dei)
    inc_dir = (be.to_numpy(kd.solar_source) * atm0.tsi_scaling[0]) * atm0.mu0[0]
    want = be.raytracer_bw(tau, ssa, nx, ny, 400.0, 400.0, dz, be.asarray(atm0.sfc_alb_dif[:, 0].copy()), float(atm0.mu0[0]), 1.1, inc_dir,
                           (2, 2, 3), cam, rpp, FS.SEED, top_at_1=atm0.top_at_1, cloud=cld, band_lims=kd.band_lims_gpt)
    assert np.array_equal(be.to_numpy(r["radiance"]).view(np.uint8), be.to_numpy(want["radiance"]).view(np.uint8))
    assert float(r["radiance"].min()) > 0
    # the sun is one for the domain, the columns are the pixels
    with pytest.raises(ValueError, match="nx ny"):
        pipeline.render_sw(be, kd, atm, nx, ny + 1, 400.0, 400.0, dz, 1.1, cam, rpp, FS.SEED)
    atm0.mu0[3] *= 0.9
    with pytest.raises(ValueError, match="mu0"):
        pipeline.render_sw(be, kd, pipeline.upload_atmosphere(be, atm0), nx, ny, 400.0, 400.0, dz, 1.1, cam, rpp, FS.SEED)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_raytracer_bw_gpu_class_gives_the_entry_bit_for_bit_and_throws(dt, hip_f64, hip_f32):
    """Raytracer_bw_gpu::trace_rays_bw (through rrx_cxx_trace_rays_bw, which wraps the caller's device arrays in Array_gpu views)
    against rrx_raytracer_bw on the general scene; a refused argument comes back as an exception's message."""
    import torch
    be = _be(dt, hip_f64, hip_f32)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so" if dt == "f64" else "librte_rrtmgp_hip_sp.so"))
    lib.rrx_cxx_driver_error.restype = ctypes.c_char_p
    F = ctypes.c_double if dt == "f64" else ctypes.c_float
    sc = FS.general(be.np_dtype)
    d = _dev(be, sc)
    sensor = SENSORS["perspective"]()
    rpp = 16
    want = solve_bw(be, sc, d, sensor, rpp)
    out = be.empty((sensor.npy, sensor.npx))
    inc_dir = np.ascontiguousarray(sc.inc_dir, dtype=be.np_dtype)
    numbers = sensor.numbers(be.np_dtype)
    n_capped, n_clamped = ctypes.c_ulonglong(99), ctypes.c_ulonglong(99)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(sensor_type):
        return lib.rrx_cxx_trace_rays_bw(sc.nx, sc.ny, sc.nz, 2, 2, F(sc.dx), F(sc.dy), F(sc.dz), int(sc.top_at_1),
                                         P(d["tau"]), P(d["ssa"]), P(d["lims"]), *(P(c) for c in d["cloud"]), P(d["alb"]), F(sc.mu0),
                                         F(sc.azimuth), inc_dir.ctypes.data_as(ctypes.c_void_p), *sc.kn_grid, sensor_type, sensor.npx,
                                         sensor.npy, F(sensor.fov), numbers.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(rpp),
                                         ctypes.c_ulonglong(sc.seed), be.RT_MAX_EVENTS, P(out), ctypes.byref(n_capped),
                                         ctypes.byref(n_clamped), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert call(sensor.type) == 0, lib.rrx_cxx_driver_error().decode()
    torch.cuda.synchronize()
    assert n_capped.value == 0 and n_clamped.value == 0 and want["n_capped"] == 0
    assert np.array_equal(be.to_numpy(out).view(np.uint8), be.to_numpy(want["radiance"]).view(np.uint8))
    assert call(7) != 0
    msg = lib.rrx_cxx_driver_error().decode()
    assert "rrx_raytracer_bw" in msg and "sensor_type" in msg, msg
