"""GPU tests of the backward tracer with the rays of all g-points in one launch, counts by band and a channel matrix
(rrx_camera_trace_counts_spectral, rrx_camera_channels, rrx_camera_render_spectral; csrc/rrx_raytracer_bw.hip). Scenes:
tests/raytracer_bw_spectral_scenes.py (4 x 4 x 6 cells, 5 g-points in 2 bands, one of them dark, sensors of 6 x 4 pixels);
restatement: tests/raytracer_bw_spectral_ref.py. The tallies are integers added with integer atomics, so a run that passes once
passes always; the integer comparisons are exact, the bounds are derived (half a count per deposit where a weight rounds, five sigma
of raytracer_bw_spectral_scenes.bernoulli_sigma, roundings of the precision for the channel sums), not measured."""
import ctypes
import os

import numpy as np
import pytest

import raytracer_phase_scenes as PS
import raytracer_bw_spectral_ref as BSP
import raytracer_bw_spectral_scenes as BSS
from raytracer_dev import _be, _u64, dev, device_table, numbers, k_null_all, backward_bg, backward_spectral, solve_bw_bg, render_spectral
from rte_rrtmgp_cpp_amd import pipeline

pytestmark = pytest.mark.gpu
BWK = ("counts", "n_capped", "n_clamped")
CHUNK = "RRX_RT_SPECTRAL_GPT_PER_LAUNCH"
NPIX = BSS.NPX*BSS.NPY


# ---- 1: the sum over the band's g-points

@pytest.mark.parametrize("kind", ["inside", "slant"])
@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("scene", ["general", "plain"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_with_unit_weights_a_band_s_counts_are_the_integer_sum_over_its_g_points(dt, scene, with_table, kind, hip_f64, hip_f32):
    """m_g = 3 on the active g-points and arrays of ones for the weights: counts[b], n_capped and n_clamped are the integer sums over
    the band's g-points of rrx_rt_bw_trace_counts_aer(g, 0, 3 npix). plain: nbg = 0 and NULL aerosol triples."""
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = getattr(BSS, scene)(be.np_dtype)
    sensor = BSS.sensors(sc)[kind]
    d, dbg = dev(be, sc, bg)
    phase = device_table(be, sc) if with_table else None
    m = np.array([3, 3, 0, 3, 3])
    ray_end, _, _ = BSP.ray_list(sc, sensor, m)
    got = numbers(be, backward_spectral(be, sc, d, dbg, sensor, (ray_end, np.ones(BSS.NGPT)), 0, int(ray_end[-1]), phase=phase))
    assert got["counts"].shape == (BSS.NBND, NPIX)
    capped = clamped = 0
    for b, band in enumerate(BSS.BANDS):
        want = np.zeros(NPIX, dtype=np.uint64)
        for g in band:
            if m[g] > 0:
                c = numbers(be, backward_bg(be, sc, d, dbg, sensor, g, 0, 3*NPIX, phase=phase, aer=True))
                want = want + c["counts"]
                capped += int(c["n_capped"][0]); clamped += int(c["n_clamped"][0])
        assert np.array_equal(got["counts"][b], want) and want.any(), b
    assert int(got["n_capped"][0]) == capped == 0 and int(got["n_clamped"][0]) == clamped == 0


# ---- 2: ranges and dealing

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_ranges_add_up_and_the_dealing_does_not_matter(dt, hip_f64, hip_f32, monkeypatch):
    """Uneven m_g with their weights, 1 320 rays (6 workgroups): the whole list equals three ranges, cut inside a g-point and on the
    boundary beside the empty range of the dark g-point, and cut on a boundary and just behind the empty range; and a run on one
    workgroup."""
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = BSS.general(be.np_dtype)
    sensor = BSS.sensors(sc)["inside"]
    d, dbg = dev(be, sc, bg)
    m = np.array([24, 4, 0, 19, 8])
    ray_end, w0, _ = BSP.ray_list(sc, sensor, m)
    n = int(ray_end[-1])
    assert n > 4*256 and ray_end[2] == ray_end[3]
    kn = k_null_all(be, sc, d)
    whole = numbers(be, backward_spectral(be, sc, d, dbg, sensor, (ray_end, w0), 0, n, kn=kn))
    assert int(whole["n_capped"][0]) == 0 and whole["counts"].any(axis=1).all()
    for cuts in ((0, int(ray_end[1]) - 5, int(ray_end[2]), n), (0, int(ray_end[1]), int(ray_end[3]) + 7, n)):
        parts = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts = backward_spectral(be, sc, d, dbg, sensor, (ray_end, w0), a, b - a, kn=kn, counts=parts)
        parts = numbers(be, parts)
        for k in BWK:
            assert np.array_equal(whole[k], parts[k]), (cuts, k)
    monkeypatch.setenv("RRX_RT_MAX_BLOCKS", "1")
    deep = numbers(be, backward_spectral(be, sc, d, dbg, sensor, (ray_end, w0), 0, n, kn=kn))
    monkeypatch.delenv("RRX_RT_MAX_BLOCKS")
    for k in BWK:
        assert np.array_equal(whole[k], deep[k]), k
    # the binding refuses a list that does not ascend and a range beyond the list
    bad = ray_end.copy(); bad[2] = bad[1] - 1
    with pytest.raises(ValueError, match="must not descend"):
        backward_spectral(be, sc, d, dbg, sensor, (bad, w0), 0, 8, kn=kn)
    with pytest.raises(ValueError, match="beyond the list"):
        backward_spectral(be, sc, d, dbg, sensor, (ray_end, w0), n - 4, 8, kn=kn)


# ---- 3: chunking

@pytest.mark.parametrize("scene", ["general", "plain"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_result_does_not_depend_on_the_chunking(dt, scene, hip_f64, hip_f32, monkeypatch):
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = getattr(BSS, scene)(be.np_dtype)
    sensor = BSS.sensors(sc)["slant"]
    d, dbg = dev(be, sc, bg)
    m = pipeline.spectral_allocation(sc.inc_dir.astype(np.float64), 24)
    M = np.eye(BSS.NBND)
    monkeypatch.delenv(CHUNK, raising=False)
    whole = render_spectral(be, sc, d, dbg, sensor, m, M)
    assert whole["n_capped"] == 0 and whole["n_clamped"] == 0 and whole["radiance"].any(axis=1).all()
    for chunk in ("1", "2"):
        monkeypatch.setenv(CHUNK, chunk)
        got = render_spectral(be, sc, d, dbg, sensor, m, M)
        assert np.array_equal(whole["radiance"].view(np.uint8), got["radiance"].view(np.uint8)), chunk
        assert got["n_capped"] == 0 and got["n_clamped"] == 0
    monkeypatch.delenv(CHUNK)
    # no rays at all: zeroed outputs; refused lists
    none = render_spectral(be, sc, d, dbg, sensor, np.zeros(BSS.NGPT, dtype=np.int64), M)
    assert none["n_capped"] == 0 and not none["radiance"].any()
    with pytest.raises(RuntimeError, match="no incident flux"):
        render_spectral(be, sc, d, dbg, sensor, np.array([1, 1, 1, 1, 1]), M)
    with pytest.raises(RuntimeError, match="negative at g-point 3"):
        render_spectral(be, sc, d, dbg, sensor, np.array([1, 1, 0, -1, 1]), M)


# ---- 4: the weights against the restatement

@pytest.mark.parametrize("top_at_1", [False, True])
def test_counts_with_uneven_weights_against_the_restatement(top_at_1, hip_f64):
    """The allocation's uneven m_g on the general scene with a table on the cloud, the camera inside the domain. The device and the
    restatement make the same deposits d and both tally llrint(d weight0 2^32): each deposit rounds once, so that a pixel's count of a
    band may differ by half a count per deposit of that pixel and band, the number of which the restatement returns."""
    import raytracer_phase_ref as P
    be = hip_f64
    sc, bg = BSS.general(np.float64, top_at_1)
    sensor = BSS.sensors(sc)["inside"]
    d, dbg = dev(be, sc, bg)
    m = pipeline.spectral_allocation(sc.inc_dir, 16)
    assert len(set(m[list(BSS.ACTIVE)])) > 2 and m[BSS.EMPTY] == 0
    table = P.build_tables(*PS.double_hg33(), np.float64, PS.RE0, PS.DRE)
    table.cld_re = PS.cell_radii(sc, np.float64)
    ray_end, w0, _ = BSP.ray_list(sc, sensor, m)
    ref = BSP.trace_counts(sc, bg, sensor, ray_end, w0, 0, int(ray_end[-1]), table=table)
    got = numbers(be, backward_spectral(be, sc, d, dbg, sensor, (ray_end, w0), 0, int(ray_end[-1]), phase=device_table(be, sc)))
    assert ref["n_capped"] == 0 == int(got["n_capped"][0]) and ref["n_clamped"] == 0 == int(got["n_clamped"][0])
    off = np.abs(got["counts"].astype(np.int64) - ref["counts"].astype(np.int64))
    print(f"raytracer_bw_spectral against the restatement top_at_1={top_at_1}: worst difference {int(off.max())} counts of 2^-32, "
          f"{int(ref['n_dep'].sum())} deposits, m = {list(m)}")
    assert ref["counts"].any(axis=1).all()
    assert np.all(2*off <= ref["n_dep"]), int(off.max())


# ---- 5: unbiased

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_weighted_estimate_is_unbiased(dt, hip_f64, hip_f32):
    """The Bernoulli surface under 256 rays per pixel dealt by flux: the radiance of every pixel and band, and the image means, within
    5 sigma of 1/mu0 sum_g inc_g c_g p_g, which does not depend on the dealing; sigma from bernoulli_sigma."""
    be = _be(dt, hip_f64, hip_f32)
    sc = BSS.bernoulli(be.np_dtype)
    sensor = BSS.sensors(sc)["nadir"]
    d, dbg = dev(be, sc, None)
    m = pipeline.spectral_allocation(sc.inc_dir.astype(np.float64), 256)
    _, w0, U = BSP.ray_list(sc, sensor, m)
    got = render_spectral(be, sc, d, dbg, sensor, m, np.eye(BSS.NBND))
    assert got["n_capped"] == 0 and got["n_clamped"] == 0
    mean, sigma = BSS.bernoulli_sigma(sc, m, w0, U)
    p, c = BSS.bernoulli_expected(sc)
    want = np.array([sum(BSS.INC[g]*c[g]*p[g] for g in band) for band in BSS.BANDS]) / float(sc.dtype.type(sc.mu0))
    assert np.allclose(mean, want, rtol=1e-5) and np.all(want > 0)          # (the weights carry the fluxes)
    rad = got["radiance"].astype(np.float64)
    dev_pix = np.abs(rad - want[:, None]) / sigma[:, None]
    dev_mean = np.abs(rad.mean(axis=1) - want) / (sigma/np.sqrt(NPIX))
    print(f"raytracer_bw_spectral unbiased {dt}: m = {list(m)}, worst deviation {max(float(dev_pix.max()), float(dev_mean.max())):.2f} "
          f"sigma (bound 5)")
    assert np.all(dev_pix <= 5) and np.all(dev_mean <= 5), (float(dev_pix.max()), float(dev_mean.max()))


# ---- 6: channels

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_channels(dt, hip_f64, hip_f32):
    """The identity gives the result by band bit for bit (one product with 1, sums with 0); a row of ones the in-order sum of the
    bands within one rounding per band; a two-row matrix M @ bands within nbnd roundings of the largest term (a product and a sum
    per band, each rounding once; the scale is applied to the sum here and to the terms there)."""
    be = _be(dt, hip_f64, hip_f32)
    eps = float(np.finfo(be.np_dtype).eps)
    sc, bg = BSS.general(be.np_dtype)
    sensor = BSS.sensors(sc)["flux"]
    d, dbg = dev(be, sc, bg)
    m = np.array([4, 1, 0, 2, 1])
    ray_end, w0, U = BSP.ray_list(sc, sensor, m)
    c = backward_spectral(be, sc, d, dbg, sensor, (ray_end, w0), 0, int(ray_end[-1]))
    F = np.dtype(be.np_dtype).type
    scale = float(F(U) / F(sc.mu0))          # (as the entry forms it, in the precision)
    x = (_u64(be, c["counts"]).astype(np.float64) * 2.0**-32).astype(F)
    bands = be.to_numpy(be.camera_channels(c["counts"], np.eye(BSS.NBND), scale))
    assert np.array_equal(bands, F(scale)*x) and np.all(bands > 0)
    by_entry = render_spectral(be, sc, d, dbg, sensor, m, np.eye(BSS.NBND))["radiance"]
    assert np.array_equal(by_entry.view(np.uint8), bands.view(np.uint8))
    ones = be.to_numpy(be.camera_channels(c["counts"], np.ones((1, BSS.NBND)), scale))[0]
    in_order = bands[0] + bands[1]
    off = np.abs(ones.astype(np.float64) - in_order) / (eps*np.abs(in_order))
    print(f"raytracer_bw_spectral channels {dt}: a row of ones differs from the in-order sum by at most {float(off.max()):.2f} eps (bound {BSS.NBND})")
    assert np.all(off <= BSS.NBND)
    M = np.array([[0.25, 0.75], [1.5, 0.0]])
    two = be.to_numpy(be.camera_channels(c["counts"], M, scale)).astype(np.float64)
    want = M @ bands.astype(np.float64)
    largest = (np.abs(M)[:, :, None]*np.abs(bands.astype(np.float64))[None]).max(axis=1)
    assert np.all(np.abs(two - want) <= 2*BSS.NBND*eps*largest)
    assert np.array_equal(two[1], (F(scale)*(F(1.5)*x[0])).astype(np.float64))


# ---- 7: the loop against one launch

def test_one_launch_against_the_loop(hip_f64):
    """Equal m_g = 4 and a row of ones against rrx_raytracer_bw_aer with 4 rays per pixel: the same rays and the same deposits d; the
    loop tallies llrint(d 2^32) and scales by inc_g / (mu0 m), the one launch tallies llrint(d weight0_g 2^32) and scales by U / mu0:
    they differ only in where the weight rounds, by half a count per deposit times U / mu0 (the deposits of a pixel: the
    restatement's)."""
    be = hip_f64
    sc, bg = BSS.general(np.float64)
    sensor = BSS.sensors(sc)["slant"]
    d, dbg = dev(be, sc, bg)
    m = np.where(np.array(BSS.INC) > 0, 4, 0)
    ray_end, w0, U = BSP.ray_list(sc, sensor, m)
    n_dep = BSP.trace_counts(sc, bg, sensor, ray_end, w0, 0, int(ray_end[-1]))["n_dep"].sum(axis=0)
    one = render_spectral(be, sc, d, dbg, sensor, m, np.ones((1, BSS.NBND)))
    many = solve_bw_bg(be, sc, d, dbg, sensor, 4, aer=True)
    many["radiance"] = be.to_numpy(many["radiance"]).reshape(-1)
    assert one["n_capped"] == many["n_capped"] == 0 and one["n_clamped"] == many["n_clamped"] == 0
    err = np.abs(one["radiance"][0] - many["radiance"])
    tol = 0.5*n_dep*2.0**-32*float(U)/sc.mu0
    print(f"raytracer_bw_spectral one launch against the loop: worst difference {float(err.max()):.3e} W m-2 sr-1 "
          f"(bound {float(tol.min()):.3e}), {int(n_dep.sum())} deposits")
    assert many["radiance"].any() and np.all(err <= tol), float((err/tol).max())


# ---- 8: the pipeline

@pytest.mark.parametrize("n_domain", [None, 4])
def test_the_chain_with_allocation_flux_is_the_entry_on_the_chain_s_own_arrays(n_domain, hip_f64):
    import math
    from rte_rrtmgp_cpp_amd import camera as C, synthetic
    be = hip_f64
    nx, ny, nlay, P, top_at_1, dz = 4, 3, 12, 48, True, 500.0
    nd = nlay if n_domain is None else n_domain
    kd = be.upload_kdist(synthetic.make_kdist("sw", ngpt=32, nbnd=2, npres=10, nflav=3, nminor_lower=5, nminor_upper=3))
    atm0 = synthetic.make_atmosphere(nx*ny, nlay, nbnd_lw=2, nbnd_sw=2, clouds=True, top_at_1=top_at_1, aerosols=True)
    atm = pipeline.upload_atmosphere(be, atm0)
    lut = be.upload_lut(synthetic.make_cloud_lut(2, "sw"))
    alut = be.upload_lut({k: (v.astype(be.np_dtype) if isinstance(v, np.ndarray) else v) for k, v in synthetic.make_aerosol_lut(2).items()})
    z_up = np.concatenate([np.arange(nd + 1)*dz, nd*dz + np.cumsum(np.linspace(700., 9000., nlay - nd))])
    split = {} if n_domain is None else dict(n_domain=nd, z_lev=z_up[::-1].copy())
    cam = C.perspective(4, 3, (800., 700., 1.5e3), yaw=0.4, pitch=-1.0, fov=math.radians(50.))
    args = (be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, cam, P, 77)
    kw = dict(cloud_lut=lut, kn_grid=(2, 1, 2), aerosol_lut=alut, allocation="flux", **split)
    M = np.array([[0.2, 0.9], [1.0, 0.0], [0.5, 0.5]])
    r = {key: pipeline.render_sw(*args, channels=ch, **kw) for key, ch in (("broad", None), ("bands", "bands"), ("M", M))}
    assert tuple(r["broad"]["radiance"].shape) == (3, 4) and tuple(r["bands"]["radiance"].shape) == (2, 3, 4)
    assert tuple(r["M"]["radiance"].shape) == (3, 3, 4) and all(v["n_capped"] == 0 for v in r.values())
    with pytest.raises(ValueError, match="channels is"):
        pipeline.render_sw(*args, channels=np.ones((2, 3)), **kw)
    with pytest.raises(ValueError, match="cannot give 2 to each of 32"):
        pipeline.render_sw(*args, min_per_gpt=2, **kw)

    _, col_gas, _ = pipeline.gas_state(be, kd, atm, None, interpolate=False)
    tau, ssa = be.empty((32, nlay, nx*ny)), be.empty((32, nlay, nx*ny))
    be.gas_optics_sw_direct(kd, atm.p_lay, atm.t_lay, col_gas, be.get_col_dry(atm.vmr["h2o"], atm.p_lev), tau, ssa, None)
    cld = be.cloud_optics_2str(lut, atm.lwp, atm.iwp, atm.rel, atm.dei)
    aer = tuple(be.aerosol_optics(alut, [atm.aermr["aermr%02d" % i] for i in range(1, 12)], atm.rh, atm.p_lev))
    inc_dir = (be.to_numpy(kd.solar_source) * atm0.tsi_scaling[0]) * atm0.mu0[0]
    grid, above = slice(nlay - nd, nlay), list(range(nlay - nd - 1, -1, -1))
    part = lambda t: t[:, grid, :].contiguous()
    dbg = None
    if n_domain is not None:
        col0 = lambda t: t[:, above, 0].contiguous()
        dbg = pipeline.Background(np.diff(z_up)[nd:].copy(), col0(tau), col0(ssa), tuple(col0(c) for c in cld), tuple(col0(c) for c in aer))
    m = pipeline.spectral_allocation(inc_dir, P)
    assert int(m.sum()) == P and m.min() >= 1 and m.max() > m.min()
    for key, matrix in (("broad", np.ones((1, 2))), ("bands", np.eye(2)), ("M", M)):
        want = be.camera_render_spectral(part(tau), part(ssa), nx, ny, 400.0, 400.0, dz, be.asarray(atm0.sfc_alb_dif[:, 0].copy()),
                                         float(atm0.mu0[0]), 1.1, inc_dir, (2, 1, 2), cam, m, 77, kd.band_lims_gpt, matrix, top_at_1=top_at_1,
                                         cloud=tuple(part(c) for c in cld), background=dbg, aerosol=tuple(part(c) for c in aer))
        got, ref = be.to_numpy(r[key]["radiance"]), be.to_numpy(want["radiance"])
        assert np.array_equal(got.reshape(-1).view(np.uint8), ref.reshape(-1).view(np.uint8)) and got.any(), key
    # allocation=None is the loop of before
    a = pipeline.render_sw(*args[:-2], 2, 77, cloud_lut=lut, kn_grid=(2, 1, 2), aerosol_lut=alut, **split)
    b = pipeline.render_sw(*args[:-2], 2, 77, cloud_lut=lut, kn_grid=(2, 1, 2), aerosol_lut=alut, allocation=None, **split)
    assert np.array_equal(be.to_numpy(a["radiance"]), be.to_numpy(b["radiance"]))


# ---- 9: the C++ class

@pytest.mark.parametrize("scene", ["general", "plain"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_cxx_class_gives_the_entry_bit_for_bit_and_throws(dt, scene, hip_f64, hip_f32):
    """Raytracer_bw_gpu::trace_rays_bw_spectral after set_phase_table, set_background and set_aerosol (through
    rrx_cxx_trace_rays_bw_spectral) against rrx_camera_render_spectral, with the caller's allocation and with
    Raytracer_gpu::spectral_allocation's; a refusal of the entry arrives as an exception's message."""
    import torch
    be = _be(dt, hip_f64, hip_f32)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so" if dt == "f64" else "librte_rrtmgp_hip_sp.so"))
    lib.rrx_cxx_driver_error.restype = ctypes.c_char_p
    F = ctypes.c_double if dt == "f64" else ctypes.c_float
    sc, bg = getattr(BSS, scene)(be.np_dtype)
    sensor = BSS.sensors(sc)["inside"]
    d, dbg = dev(be, sc, bg)
    nbg = 0 if bg is None else bg.nbg
    phase = device_table(be, sc)
    inc_dir = np.ascontiguousarray(sc.inc_dir, dtype=be.np_dtype)
    M = np.ascontiguousarray([[0.25, 0.75], [1.0, 0.0], [1.0, 1.0]], dtype=be.np_dtype)
    numbers12 = np.ascontiguousarray(np.concatenate([sensor.position, sensor.e_w, sensor.e_h, sensor.e_d]), dtype=be.np_dtype)
    H = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    none = ctypes.c_void_p(0)
    radiance = be.empty((M.shape[0], BSS.NPY, BSS.NPX))
    n_capped, n_clamped = ctypes.c_ulonglong(99), ctypes.c_ulonglong(99)
    table = (phase.mu.shape[0], phase.phase.shape[1], F(phase.re0), F(phase.dre), P(phase.mu), P(phase.phase), P(phase.cdf), P(phase.cld_re))
    medium = (0, none, none, none, none, none, none) if bg is None else (nbg, H(dbg.dz), P(dbg.tau), P(dbg.ssa), *(P(c) for c in dbg.cloud))
    grid = tuple(none if c is None else P(c) for c in d["aer"])
    aloft = (none, none, none) if bg is None else tuple(P(c) for c in dbg.aerosol)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(m, total=-1, aer=grid, nchan=M.shape[0]):
        m = np.ascontiguousarray(m, dtype=np.int64)
        return lib.rrx_cxx_trace_rays_bw_spectral(sc.nx, sc.ny, sc.nz, BSS.NGPT, BSS.NBND, F(sc.dx), F(sc.dy), F(sc.dz), int(sc.top_at_1),
                                                  P(d["tau"]), P(d["ssa"]), P(d["lims"]), *(P(c) for c in d["cloud"]), P(d["alb"]), F(sc.mu0),
                                                  F(sc.azimuth), H(inc_dir), *sc.kn_grid, sensor.type, sensor.npx, sensor.npy, F(sensor.fov),
                                                  H(numbers12), H(m), ctypes.c_longlong(total), ctypes.c_ulonglong(sc.seed), be.RT_MAX_EVENTS,
                                                  nchan, H(M), P(radiance), ctypes.byref(n_capped), ctypes.byref(n_clamped), *table, *medium,
                                                  *aer, *aloft, stream)

    m = np.array([5, 1, 0, 2, 2])
    for given, total in ((m, -1), (np.zeros(BSS.NGPT, dtype=np.int64), 24)):
        dealt = given if total < 0 else pipeline.spectral_allocation(inc_dir, total)
        want = render_spectral(be, sc, d, dbg, sensor, dealt, M, phase=phase)
        assert call(given, total) == 0, lib.rrx_cxx_driver_error().decode()
        torch.cuda.synchronize()
        assert n_capped.value == 0 == want["n_capped"] and n_clamped.value == 0 == want["n_clamped"]
        got = be.to_numpy(radiance).reshape(-1, NPIX)
        assert np.array_equal(got.view(np.uint8), want["radiance"].view(np.uint8)) and want["radiance"].any(axis=1).all(), total
    for bad, word in ((np.array([1, 1, 1, 1, 1]), "no incident flux"), (np.array([1, -1, 0, 1, 1]), "negative at g-point 1")):
        assert call(bad) != 0
        assert word in lib.rrx_cxx_driver_error().decode()
    assert call(m, total=3) != 0
    assert "cannot give 1 to each of 4" in lib.rrx_cxx_driver_error().decode()
    assert call(m, nchan=0) != 0
    assert "nchan and nbnd must be >= 1" in lib.rrx_cxx_driver_error().decode()
    if sc.aerosol is not None:
        assert call(m, aer=(grid[0], none, grid[2])) != 0
        assert "Raytracer_bw_gpu::set_aerosol" in lib.rrx_cxx_driver_error().decode()
