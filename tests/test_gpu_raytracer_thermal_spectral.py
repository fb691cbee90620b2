"""GPU tests of the thermal tracer with the rays of all g-points in one launch, counts by band and a channel matrix
(rrx_thermal_trace_counts_spectral, rrx_thermal_render_spectral; csrc/rrx_raytracer_thermal.hip). Scenes:
tests/thermal_spectral_scenes.py (4 x 4 x 6 cells, 5 g-points in 2 bands, one of them dark, sensors of 6 x 4 pixels); restatement:
tests/raytracer_thermal_spectral_ref.py. The tallies are integers added with integer atomics, so a run that passes once passes
always; the integer comparisons are exact, the bounds are derived (half a count per deposit where a weighted source rounds, five
sigma of thermal_spectral_scenes.schwarzschild_sigma, roundings of the precision for the channel sums), not measured."""
import ctypes
import math
import os

import numpy as np
import pytest

import raytracer_thermal_ref as T
import raytracer_thermal_spectral_ref as TSP
import thermal_spectral_scenes as TSS
from raytracer_dev import _be, _u64, numbers
from raytracer_thermal_dev import dev, k_null, trace, render
from rte_rrtmgp_cpp_amd import pipeline

pytestmark = pytest.mark.gpu
KEYS = ("counts", "n_capped", "n_clamped")
CHUNK = "RRX_RT_SPECTRAL_GPT_PER_LAUNCH"
NPIX = TSS.NPIX


def k_null_all(be, sc, d):
    return be.rt_k_null_all(d["tau"], sc.nx, sc.ny, sc.dz, sc.kn_grid, sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"])


def trace_spectral(be, sc, d, sensor, lists, ray0, nrays, kn=None, counts=None, max_events=None, top="own"):
    """rrx_thermal_trace_counts_spectral; lists = (ray_end, weight0)"""
    kn = k_null_all(be, sc, d) if kn is None else kn
    top = np.asarray(sc.top_radiance) if isinstance(top, str) else top
    return be.thermal_trace_counts_spectral(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["emis"], d["lay_src"], d["sfc_src"], top,
                                            lists[0], lists[1], sc.kn_grid, kn, sensor, sc.seed, ray0, nrays, d["lims"], top_at_1=sc.top_at_1,
                                            cloud=d["cloud"], counts=counts, max_events=max_events)


def render_spectral(be, sc, d, sensor, m, M, max_events=None):
    """rrx_thermal_render_spectral, the radiance as (nchan, npix) on the host"""
    r = be.thermal_render_spectral(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["emis"], d["lay_src"], d["sfc_src"], sc.kn_grid,
                                   sensor, m, sc.seed, d["lims"], M, top_at_1=sc.top_at_1, cloud=d["cloud"], max_events=max_events,
                                   top_radiance=np.asarray(sc.top_radiance))
    r["radiance"] = be.to_numpy(r["radiance"]).reshape(np.asarray(M).shape[0], -1)
    return r


# ---- 0: the set-up kernel

@pytest.mark.parametrize("cloud", [True, False])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_k_null_all_with_a_null_aerosol_is_k_null_slice_for_slice(dt, cloud, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc = TSS.general(be.np_dtype, cloud=cloud)
    d = dev(be, sc)
    every = be.to_numpy(k_null_all(be, sc, d))
    assert every.shape == (TSS.NGPT, *sc.kn_grid[::-1])
    for g in range(TSS.NGPT):
        one = be.to_numpy(k_null(be, sc, d, g))
        assert np.array_equal(every[g].view(np.uint8), one.view(np.uint8)) and one.all(), g


# ---- 1: the sum over the band's g-points

@pytest.mark.parametrize("kind", ["inside", "slant", "flux"])
@pytest.mark.parametrize("variant", ["cloud", "clear", "null_ssa"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_with_unit_weights_a_band_s_counts_are_the_integer_sum_over_its_g_points(dt, variant, kind, hip_f64, hip_f32):
    """m_g = 3 on the active g-points and arrays of ones for the weights: counts[b], n_capped and n_clamped are the integer sums over
    the band's g-points of rrx_thermal_trace_counts(g, 0, 3 npix)."""
    be = _be(dt, hip_f64, hip_f32)
    sc = TSS.general(be.np_dtype, cloud=variant != "clear", gas_scatters=variant != "null_ssa")
    sensor = TSS.sensors(sc)[kind]
    d = dev(be, sc)
    assert (d["ssa"] is None) == (variant == "null_ssa") and (d["cloud"] is None) == (variant == "clear")
    m = np.array([3, 3, 0, 3, 3])
    ray_end, _, _ = TSP.ray_list(sc, sensor, m)
    got = numbers(be, trace_spectral(be, sc, d, sensor, (ray_end, np.ones(TSS.NGPT)), 0, int(ray_end[-1])))
    assert got["counts"].shape == (TSS.NBND, NPIX)
    capped = clamped = 0
    for b, band in enumerate(TSS.BANDS):
        want = np.zeros(NPIX, dtype=np.uint64)
        for g in band:
            if m[g] > 0:
                c = numbers(be, trace(be, sc, d, sensor, g, 0, 3*NPIX))
                want = want + c["counts"]
                capped += int(c["n_capped"][0]); clamped += int(c["n_clamped"][0])
        assert np.array_equal(got["counts"][b], want) and want.any(), b
    assert int(got["n_capped"][0]) == capped == 0 and int(got["n_clamped"][0]) == clamped == 0


# ---- 2: ranges and dealing

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_ranges_add_up_and_the_dealing_does_not_matter(dt, hip_f64, hip_f32, monkeypatch):
    """Uneven m_g with their weights, 1 320 rays (6 workgroups): the whole list equals three ranges, cut inside a g-point and on the
    boundary beside the empty range of the dark g-point, and cut on a boundary and just behind the empty range; a second run; and a
    run on one workgroup."""
    be = _be(dt, hip_f64, hip_f32)
    sc = TSS.general(be.np_dtype)
    sensor = TSS.sensors(sc)["inside"]
    d = dev(be, sc)
    m = np.array([24, 4, 0, 19, 8])
    ray_end, w0, _ = TSP.ray_list(sc, sensor, m)
    n = int(ray_end[-1])
    assert n > 4*256 and ray_end[2] == ray_end[3]
    kn = k_null_all(be, sc, d)
    whole = numbers(be, trace_spectral(be, sc, d, sensor, (ray_end, w0), 0, n, kn=kn))
    again = numbers(be, trace_spectral(be, sc, d, sensor, (ray_end, w0), 0, n, kn=kn))
    assert int(whole["n_capped"][0]) == 0 and whole["counts"].any(axis=1).all()
    for k in KEYS:
        assert np.array_equal(whole[k], again[k]), k
    for cuts in ((0, int(ray_end[1]) - 5, int(ray_end[2]), n), (0, int(ray_end[1]), int(ray_end[3]) + 7, n)):
        parts = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts = trace_spectral(be, sc, d, sensor, (ray_end, w0), a, b - a, kn=kn, counts=parts)
        parts = numbers(be, parts)
        for k in KEYS:
            assert np.array_equal(whole[k], parts[k]), (cuts, k)
    monkeypatch.setenv("RRX_RT_MAX_BLOCKS", "1")
    deep = numbers(be, trace_spectral(be, sc, d, sensor, (ray_end, w0), 0, n, kn=kn))
    monkeypatch.delenv("RRX_RT_MAX_BLOCKS")
    for k in KEYS:
        assert np.array_equal(whole[k], deep[k]), k
    # a NULL top_radiance is a top radiance of 0
    dark = numbers(be, trace_spectral(be, sc, d, sensor, (ray_end, w0), 0, n, kn=kn, top=None))
    zeros = numbers(be, trace_spectral(be, sc, d, sensor, (ray_end, w0), 0, n, kn=kn, top=np.zeros(TSS.NGPT)))
    assert np.array_equal(dark["counts"], zeros["counts"]) and np.all(dark["counts"] <= whole["counts"]) and np.any(dark["counts"] < whole["counts"])
    # the binding refuses a list that does not ascend, a range beyond the list and a call without band_lims
    bad = ray_end.copy(); bad[2] = bad[1] - 1
    with pytest.raises(ValueError, match="must not descend"):
        trace_spectral(be, sc, d, sensor, (bad, w0), 0, 8, kn=kn)
    with pytest.raises(ValueError, match="beyond the list"):
        trace_spectral(be, sc, d, sensor, (ray_end, w0), n - 4, 8, kn=kn)
    with pytest.raises(ValueError, match="needs band_lims"):
        trace_spectral(be, sc, dict(d, lims=None, cloud=None), sensor, (ray_end, w0), 0, 8, kn=kn)


# ---- 3: chunking, and the binding against the entry made by hand

@pytest.mark.parametrize("variant", ["cloud", "null_ssa"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_result_does_not_depend_on_the_chunking(dt, variant, hip_f64, hip_f32, monkeypatch):
    be = _be(dt, hip_f64, hip_f32)
    sc = TSS.general(be.np_dtype, gas_scatters=variant != "null_ssa")
    sensor = TSS.sensors(sc)["slant"]
    d = dev(be, sc)
    m = pipeline.spectral_allocation(TSS.emission(sc), 24)
    M = np.eye(TSS.NBND)
    monkeypatch.delenv(CHUNK, raising=False)
    whole = render_spectral(be, sc, d, sensor, m, M)
    assert whole["n_capped"] == 0 and whole["n_clamped"] == 0 and whole["radiance"].any(axis=1).all()
    for chunk in ("1", "2"):
        monkeypatch.setenv(CHUNK, chunk)
        got = render_spectral(be, sc, d, sensor, m, M)
        assert np.array_equal(whole["radiance"].view(np.uint8), got["radiance"].view(np.uint8)), chunk
        assert got["n_capped"] == 0 and got["n_clamped"] == 0
    monkeypatch.delenv(CHUNK)
    # HipKernels.thermal_render_spectral is the trace entry on the list of ray_list and one conversion with scale = U
    ray_end, w0, U = TSP.ray_list(sc, sensor, m)
    c = trace_spectral(be, sc, d, sensor, (ray_end, w0), 0, int(ray_end[-1]))
    by_hand = be.to_numpy(be.camera_channels(c["counts"], M, float(U)))
    assert np.array_equal(by_hand.view(np.uint8), whole["radiance"].view(np.uint8))
    # no rays at all: zeroed outputs; a refused list
    none = render_spectral(be, sc, d, sensor, np.zeros(TSS.NGPT, dtype=np.int64), M)
    assert none["n_capped"] == 0 and not none["radiance"].any()
    with pytest.raises(RuntimeError, match="negative at g-point 3"):
        render_spectral(be, sc, d, sensor, np.array([1, 1, 0, -1, 1]), M)


# ---- 4: the weights against the restatement

@pytest.mark.parametrize("top_at_1", [False, True])
def test_counts_with_uneven_weights_against_the_restatement(top_at_1, hip_f64):
    """Uneven m_g on the general scene, the camera inside the domain. The device and the restatement scale the same sources by the
    same weights and make the same deposits; where a transcendental of the transport rounds differently the deposit may differ in its
    last place, which is far below a count: a pixel's count of a band may differ by half a count per deposit of that pixel and band,
    the number of which the restatement returns."""
    be = hip_f64
    sc = TSS.general(np.float64, top_at_1)
    sensor = TSS.sensors(sc)["inside"]
    d = dev(be, sc)
    m = np.array([40, 3, 0, 15, 6])
    ray_end, w0, _ = TSP.ray_list(sc, sensor, m)
    assert len(set(w0[list(TSS.ACTIVE)])) == 4 and w0[TSS.EMPTY] == 0
    ref = TSP.trace_counts(sc, sensor, ray_end, w0, 0, int(ray_end[-1]))
    got = numbers(be, trace_spectral(be, sc, d, sensor, (ray_end, w0), 0, int(ray_end[-1])))
    assert ref["n_capped"] == 0 == int(got["n_capped"][0]) and ref["n_clamped"] == 0 == int(got["n_clamped"][0])
    off = np.abs(got["counts"].astype(np.int64) - ref["counts"].astype(np.int64))
    print(f"thermal spectral against the restatement top_at_1={top_at_1}: worst difference {int(off.max())} counts of 2^-32, "
          f"{int(ref['n_dep'].sum())} deposits, m = {list(m)}")
    assert ref["counts"].any(axis=1).all()
    assert np.all(2*off <= ref["n_dep"]), int(off.max())


# ---- 5: unbiased

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_weighted_estimate_is_unbiased(dt, hip_f64, hip_f32):
    """Schwarzschild's sum under STAT_RAYS rays per pixel dealt by emission: the radiance of every pixel and band, and the image means,
    within 5 sigma of sum_g L_g, which does not depend on the dealing; sigma from schwarzschild_sigma. Every ray deposits exactly once,
    so that the deposits of a pixel and band are its rays. (test_raytracer_thermal_spectral_ref.py holds the restatement to the same
    bound with the same seed.)"""
    be = _be(dt, hip_f64, hip_f32)
    sc = TSS.schwarzschild(be.np_dtype)
    sensor = TSS.nadir()
    d = dev(be, sc)
    assert d["ssa"] is None and d["cloud"] is None
    m = pipeline.spectral_allocation(TSS.emission(sc), TSS.STAT_RAYS)
    got = render_spectral(be, sc, d, sensor, m, np.eye(TSS.NBND))
    assert got["n_capped"] == 0 and got["n_clamped"] == 0
    mean, sigma = TSS.schwarzschild_sigma(sc, m)
    rad = got["radiance"].astype(np.float64)
    dev_pix = np.abs(rad - mean[:, None]) / sigma[:, None]
    dev_mean = np.abs(rad.mean(axis=1) - mean) / (sigma/np.sqrt(NPIX))
    print(f"thermal spectral unbiased {dt}: m = {list(m)}, worst deviation {float(dev_pix.max()):.2f} sigma per pixel, "
          f"{float(dev_mean.max()):.2f} of the image mean (bound 5)")
    assert np.all(mean > 0) and np.all(dev_pix <= 5) and np.all(dev_mean <= 5), (float(dev_pix.max()), float(dev_mean.max()))


# ---- 6: channels

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_channel_matrix_against_the_restatement_s_channels(dt, hip_f64, hip_f32):
    """The device's counts through raytracer_bw_spectral_ref.channels, the sum in band order in the precision: the identity bit for
    bit (a product with 1 and sums with 0), any other matrix within nbnd roundings of the largest term (a product and a sum per band;
    the device may contract neither, the bound leaves room for the scale's rounding)."""
    be = _be(dt, hip_f64, hip_f32)
    eps = float(np.finfo(be.np_dtype).eps)
    sc = TSS.general(be.np_dtype)
    sensor = TSS.sensors(sc)["flux"]
    d = dev(be, sc)
    m = np.array([4, 1, 0, 2, 1])
    ray_end, w0, U = TSP.ray_list(sc, sensor, m)
    counts = _u64(be, trace_spectral(be, sc, d, sensor, (ray_end, w0), 0, int(ray_end[-1]))["counts"])
    bands = render_spectral(be, sc, d, sensor, m, np.eye(TSS.NBND))["radiance"]
    assert np.array_equal(bands, TSP.channels(counts, np.eye(TSS.NBND), U, be.np_dtype)) and np.all(bands > 0)
    M = np.array([[1.0, 1.0], [0.25, 0.75], [1.5, 0.0]])
    got = render_spectral(be, sc, d, sensor, m, M)["radiance"].astype(np.float64)
    want = TSP.channels(counts, M, U, be.np_dtype).astype(np.float64)
    largest = (np.abs(M)[:, :, None]*np.abs(bands.astype(np.float64))[None]).max(axis=1)
    off = np.abs(got - want) / (eps*largest)
    print(f"thermal spectral channels {dt}: worst difference from the restatement's channels {float(off.max()):.2f} eps of the largest term "
          f"(bound {2*TSS.NBND})")
    assert got.shape == (3, NPIX) and np.all(off <= 2*TSS.NBND)


# ---- 7: the loop against one launch

def test_one_launch_against_the_loop(hip_f64):
    """Equal m_g = 4 on every g-point and a row of ones against rrx_thermal_render with 4 rays per pixel: weight0 is exactly 1, so the
    two trace the same rays and tally the same integers; the loop converts per g-point with 1 / F(4) and adds in F, the one launch
    adds the integers by band and converts once with U = 1 / F(4): they differ only in where the conversion rounds, far below
    n_dep 2^-33 per pixel (the deposits of a pixel: the restatement's). In fp64 only: the bound lies below the spacing of fp32 numbers
    of the radiances' size, so fp32 cannot resolve it."""
    be = hip_f64
    sc = TSS.general(np.float64)
    sensor = TSS.sensors(sc)["slant"]
    d = dev(be, sc)
    m = np.full(TSS.NGPT, 4)
    ray_end, w0, U = TSP.ray_list(sc, sensor, m)
    assert np.array_equal(w0, np.ones(TSS.NGPT)) and U == 0.25
    n_dep = TSP.trace_counts(sc, sensor, ray_end, w0, 0, int(ray_end[-1]))["n_dep"].sum(axis=0)
    one = render_spectral(be, sc, d, sensor, m, np.ones((1, TSS.NBND)))
    many = render(be, sc, d, sensor, 4)
    assert one["n_capped"] == many["n_capped"] == 0 and one["n_clamped"] == many["n_clamped"] == 0
    loop = be.to_numpy(many["radiance"]).reshape(-1)
    err = np.abs(one["radiance"][0] - loop)
    tol = n_dep*2.0**-33
    print(f"thermal spectral one launch against the loop: worst difference {float(err.max()):.3e} W m-2 sr-1 (bound {float(tol.min()):.3e}), "
          f"{int(n_dep.sum())} deposits")
    assert loop.all() and np.all(err <= tol), float((err/tol).max())


# ---- 8: the cap

def test_the_cap_is_counted(hip_f64):
    be = hip_f64
    sc = TSS.general(np.float64)
    sensor = TSS.sensors(sc)["slant"]
    m = np.array([3, 1, 0, 2, 2])
    capped = render_spectral(be, sc, dev(be, sc), sensor, m, np.eye(TSS.NBND), max_events=1)
    assert 0 < capped["n_capped"] == TSP.render(sc, sensor, m, np.eye(TSS.NBND), max_events=1)["n_capped"] <= int(m.sum())*NPIX


# ---- 9: the chain

def test_render_lw_with_allocation_emission_is_the_entry_on_the_chain_s_own_arrays(hip_f64):
    from rte_rrtmgp_cpp_amd import camera as C, synthetic
    be = hip_f64
    nx, ny, nlay, P = 4, 4, 12, 96
    kd = be.upload_kdist(synthetic.make_kdist("lw", ngpt=32, nbnd=2, npres=10, nflav=3, nminor_lower=5, nminor_upper=3))
    atm0 = synthetic.make_atmosphere(nx*ny, nlay, nbnd_lw=2, nbnd_sw=2, clouds=True)
    atm0.emis_sfc[:] = atm0.emis_sfc[:, :1]
    atm = pipeline.upload_atmosphere(be, atm0)
    lut = be.upload_lut(synthetic.make_cloud_lut(2, "lw"))
    dz = 70.e3/nlay
    cam = C.perspective(5, 3, (800., 700., 20.e3), yaw=0.4, pitch=-1.0, fov=math.radians(50.))
    top = np.linspace(0.0, 0.02, 32)
    args = (be, kd, atm, nx, ny, 400.0, 400.0, dz, cam, P, TSS.S.SEED)
    kw = dict(cloud_lut=lut, kn_grid=(2, 2, 3), top_radiance=top, allocation="emission")
    M = np.array([[1.0, 1.0], [0.25, 0.0], [0.0, 2.0]])
    r = {key: pipeline.render_lw(*args, channels=ch, **kw) for key, ch in (("broad", None), ("bands", "bands"), ("M", M))}
    assert tuple(r["broad"]["radiance"].shape) == (3, 5) and tuple(r["bands"]["radiance"].shape) == (2, 3, 5)
    assert tuple(r["M"]["radiance"].shape) == (3, 3, 5) and all(v["n_capped"] == 0 and v["n_clamped"] == 0 for v in r.values())
    with pytest.raises(ValueError, match="channels is"):
        pipeline.render_lw(*args, channels=np.ones((2, 3)), **kw)
    with pytest.raises(ValueError, match="cannot give 4 to each of 32"):
        pipeline.render_lw(*args, min_per_gpt=4, **kw)
    with pytest.raises(ValueError, match="allocation is None or 'emission'"):
        pipeline.render_lw(*args, **dict(kw, allocation="flux"))

    _, col_gas, _ = pipeline.gas_state(be, kd, atm, None, interpolate=False)
    tau = be.gas_optics_lw_direct(kd, atm.p_lay, atm.t_lay, col_gas, be.empty((32, nlay, nx*ny)))
    src = be.planck_source_direct(kd, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, nlay if atm0.top_at_1 else 1, col_gas)
    cld = be.cloud_optics_2str(lut, atm.lwp, atm.iwp, atm.rel, atm.dei)
    emis = be.asarray(atm0.emis_sfc[:, 0].copy())
    m = pipeline.spectral_allocation(be.to_numpy(src["sfc_src"]).astype(np.float64).sum(axis=1), P)
    assert int(m.sum()) == P and m.min() >= 1 and m.max() > m.min()
    for key, matrix in (("broad", np.ones((1, 2))), ("bands", np.eye(2)), ("M", M)):
        want = be.thermal_render_spectral(tau, None, nx, ny, 400.0, 400.0, dz, emis, src["lay_src"], src["sfc_src"], (2, 2, 3), cam, m, TSS.S.SEED,
                                          kd.band_lims_gpt, matrix, top_at_1=atm0.top_at_1, cloud=cld, top_radiance=top)
        got, ref = be.to_numpy(r[key]["radiance"]), be.to_numpy(want["radiance"])
        assert np.array_equal(got.reshape(-1).view(np.uint8), ref.reshape(-1).view(np.uint8)) and (got > 0).all(), key
    # allocation=None is the loop of before
    a = pipeline.render_lw(*args[:-2], 2, TSS.S.SEED, cloud_lut=lut, kn_grid=(2, 2, 3), top_radiance=top)
    b = pipeline.render_lw(*args[:-2], 2, TSS.S.SEED, cloud_lut=lut, kn_grid=(2, 2, 3), top_radiance=top, allocation=None)
    want = be.thermal_render(tau, None, nx, ny, 400.0, 400.0, dz, emis, src["lay_src"], src["sfc_src"], (2, 2, 3), cam, 2, TSS.S.SEED,
                             top_at_1=atm0.top_at_1, cloud=cld, band_lims=kd.band_lims_gpt, top_radiance=top)
    assert np.array_equal(be.to_numpy(a["radiance"]), be.to_numpy(b["radiance"]))
    assert np.array_equal(be.to_numpy(a["radiance"]).view(np.uint8), be.to_numpy(want["radiance"]).view(np.uint8))


# ---- 10: the C++ class

@pytest.mark.parametrize("variant", ["cloud", "null_ssa"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_cxx_class_gives_the_entry_bit_for_bit_and_throws(dt, variant, hip_f64, hip_f32):
    """Raytracer_thermal_gpu::trace_rays_thermal_spectral (through rrx_cxx_trace_rays_thermal_spectral, which wraps the caller's device
    arrays in Array_gpu views) against rrx_thermal_render_spectral, with the caller's allocation and with
    Raytracer_gpu::spectral_allocation's over the emission; a refusal of the entry arrives as an exception's message."""
    import torch
    be = _be(dt, hip_f64, hip_f32)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so" if dt == "f64" else "librte_rrtmgp_hip_sp.so"))
    lib.rrx_cxx_driver_error.restype = ctypes.c_char_p
    F = ctypes.c_double if dt == "f64" else ctypes.c_float
    sc = TSS.general(be.np_dtype, cloud=variant == "cloud", gas_scatters=variant != "null_ssa")
    sensor = TSS.sensors(sc)["inside"]
    d = dev(be, sc)
    e = np.ascontiguousarray(TSS.emission(sc), dtype=be.np_dtype)
    top = np.ascontiguousarray(sc.top_radiance, dtype=be.np_dtype)
    M = np.ascontiguousarray([[0.25, 0.75], [1.0, 0.0], [1.0, 1.0]], dtype=be.np_dtype)
    numbers12 = sensor.numbers(be.np_dtype)
    H = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    none = ctypes.c_void_p(0)
    P = lambda t: none if t is None else ctypes.c_void_p(t.data_ptr())
    radiance = be.empty((M.shape[0], TSS.NPY, TSS.NPX))
    n_capped, n_clamped = ctypes.c_ulonglong(99), ctypes.c_ulonglong(99)
    cloud = (none, none, none) if d["cloud"] is None else tuple(P(c) for c in d["cloud"])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(m, total=-1, nchan=M.shape[0], sensor_type=sensor.type):
        m = np.ascontiguousarray(m, dtype=np.int64)
        return lib.rrx_cxx_trace_rays_thermal_spectral(sc.nx, sc.ny, sc.nz, TSS.NGPT, TSS.NBND, F(sc.dx), F(sc.dy), F(sc.dz), int(sc.top_at_1),
                                                       P(d["tau"]), P(d["ssa"]), P(d["lims"]), *cloud, P(d["emis"]), P(d["lay_src"]),
                                                       P(d["sfc_src"]), H(top), *sc.kn_grid, sensor_type, sensor.npx, sensor.npy, F(sensor.fov),
                                                       H(numbers12), H(m), ctypes.c_longlong(total), H(e), ctypes.c_ulonglong(sc.seed),
                                                       be.RT_MAX_EVENTS, nchan, H(M), P(radiance), ctypes.byref(n_capped),
                                                       ctypes.byref(n_clamped), stream)

    m = np.array([5, 1, 0, 2, 2])
    for given, total in ((m, -1), (np.zeros(TSS.NGPT, dtype=np.int64), 24)):
        dealt = given if total < 0 else pipeline.spectral_allocation(e, total)
        want = render_spectral(be, sc, d, sensor, dealt, M)
        assert call(given, total) == 0, lib.rrx_cxx_driver_error().decode()
        torch.cuda.synchronize()
        assert n_capped.value == 0 == want["n_capped"] and n_clamped.value == 0 == want["n_clamped"]
        got = be.to_numpy(radiance).reshape(-1, NPIX)
        assert np.array_equal(got.view(np.uint8), want["radiance"].view(np.uint8)) and want["radiance"].any(axis=1).all(), total
    assert call(np.array([1, -1, 0, 1, 1])) != 0
    msg = lib.rrx_cxx_driver_error().decode()
    assert "rrx_thermal_render_spectral" in msg and "negative at g-point 1" in msg, msg
    assert call(m, total=3) != 0
    assert "cannot give 1 to each of 4" in lib.rrx_cxx_driver_error().decode()
    assert call(m, nchan=0) != 0
    assert "nchan and nbnd must be >= 1" in lib.rrx_cxx_driver_error().decode()
    assert call(m, sensor_type=7) != 0
    assert "sensor_type" in lib.rrx_cxx_driver_error().decode()
