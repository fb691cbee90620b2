"""GPU tests of the forward Monte Carlo ray tracer (csrc/rrx_raytracer.hip). Scenes: tests/raytracer_scenes.py, grids
of 4x4x6 to 8x4x6 cells, two g-points with different incident flux, fixed seeds; the tallies are integers added with integer
atomics, so a run that passes once passes always. Statistical bound (derived, not measured): a tally whose per-photon
contribution lies in [0, 1] with mean p has a standard deviation of at most sqrt(p (1 - p) / N); five of these are allowed.
Every test asserts n_capped == 0.

Observed on an MI355X (worst |deviation| / sigma over all pixels and g-points, bound 5): see DESIGN.md 4.14."""
import numpy as np
import pytest

import raytracer_ref as R
import raytracer_scenes as S
from raytracer_dev import _be, _dev, _u64, forward, solve_fw
from rte_rrtmgp_cpp_amd import synthetic, pipeline

pytestmark = pytest.mark.gpu
ONE = float(1 << 32)
NAMES = R.COUNT_NAMES


def hand_loop(be, sc, d, ppp):
    """The spectral loop of rrx_raytracer_sw made of the three small entries: (broadband fluxes, per-g-point counts as uint64)."""
    F = be.np_dtype.type
    flux = {k: be.zeros((sc.ncol,)) for k in NAMES[:4]}
    flux.update({k: be.zeros((sc.nz, sc.ncol)) for k in NAMES[4:]})
    per_g = []
    for g in range(sc.tau.shape[0]):
        inc = F(sc.inc_dir[g]) + F(sc.inc_dif[g])
        if not inc > 0:
            per_g.append(None)
            continue
        c = forward(be, sc, d, g, 0, ppp*sc.ncol)
        scale = inc / F(ppp)
        for k in NAMES:
            be.rt_counts_to_flux(c[k], float(scale if k in NAMES[:4] else scale / F(sc.dz)), flux[k])
        per_g.append({k: _u64(be, v) for k, v in c.items()})
        assert int(per_g[-1]["n_capped"][0]) == 0
    return {k: be.to_numpy(v) for k, v in flux.items()}, per_g


def solve(be, sc, d, ppp):
    r = solve_fw(be, sc, d, ppp)
    assert r["n_capped"] == 0
    return r


def check_beer(sc, per_g, ppp, label):
    """every pixel's direct transmittance within 5 sigma of exp(-sum tau / mu0); prints the worst deviation in sigmas"""
    want = S.beer_expected(sc)
    worst = 0.0
    for g, c in enumerate(per_g):
        got = c["sfc_dn_dir"].astype(np.float64) / ONE / ppp
        sig = S.sigma(want[g], ppp)
        worst = max(worst, float(np.max(np.abs(got - want[g]) / sig)))
        assert np.all(np.abs(got - want[g]) <= 5*sig), (label, g)
        mean_sig = S.sigma(want[g].mean(), ppp*sc.ncol)
        worst_mean = abs(got.mean() - want[g].mean()) / mean_sig
        assert worst_mean <= 5, (label, g, worst_mean)
        assert not c["sfc_dn_dif"].any() and not c["tod_up"].any() and not c["sfc_up"].any()
    print(f"raytracer {label}: worst per-pixel deviation {worst:.2f} sigma (bound 5)")


# ---- A and G: Beer per pixel

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("kn_is_grid", [True, False])
def test_a_beer_per_pixel(kn_is_grid, dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc = S.beer(be.np_dtype, kn_is_grid)
    d = _dev(be, sc)
    ppp = 4096
    _, per_g = hand_loop(be, sc, d, ppp)
    check_beer(sc, per_g, ppp, f"A {dt} kn_is_grid={kn_is_grid}")
    if kn_is_grid and dt == "f64":
        # every weight is 0 or 1: nothing is lost, in integers and in the fluxes
        for c in per_g:
            assert int(c["abs_dir"].sum()) + int(c["sfc_dn_dir"].sum()) == ppp*sc.ncol*(1 << 32)
        r = solve(be, sc, d, ppp)
        incident = sc.ncol*float(np.sum(sc.inc_dir))
        total = float(np.sum(r["abs_dir"].astype(np.float64))*sc.dz + np.sum(r["sfc_dn_dir"].astype(np.float64)))
        assert abs(total - incident) <= 1e-12*incident
        assert np.all(r["tod_up"] == 0) and np.all(r["abs_dif"] == 0)


# ---- B and G: slant path and periodic wrap

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_b_slant_and_wrap(dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc = S.slant(be.np_dtype)
    ppp = 4096
    _, per_g = hand_loop(be, sc, _dev(be, sc), ppp)
    check_beer(sc, per_g, ppp, f"B {dt}")


# ---- C: the shadow is displaced along the direction of travel

@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("along", ["x", "y"])
def test_c_shadow_displacement(along, top_at_1, hip_f64):
    be = hip_f64
    sc = S.shadow(np.float64, along, top_at_1)
    lo, hi = R.pixel_path_range(sc, 0)
    lit, dark = hi == 0.0, lo > 40.0           # (a full chord through the block is tau = 70: 256 e^-40 photons are none)
    assert lit.sum() == sc.ncol - 8 and dark.sum() == 4
    ppp = 256
    c = forward(be, sc, _dev(be, sc), 0, 0, ppp*sc.ncol)
    direct = _u64(be, c["sfc_dn_dir"])
    assert int(_u64(be, c["n_capped"])[0]) == 0
    assert np.all(direct[lit] == ppp << 32), direct[lit] / ONE
    assert np.all(direct[dark] == 0), direct[dark] / ONE
    absorbed = _u64(be, c["abs_dir"])
    lay = sc.nz - 1 - 3 if top_at_1 else 3
    assert absorbed[lay].sum() == absorbed.sum() > 0
    assert int(absorbed.sum()) + int(direct.sum()) == ppp*sc.ncol << 32


# ---- D: conservative scattering

def test_d_conservative_scattering(hip_f64):
    be = hip_f64
    sc = S.conservative(np.float64)
    d = _dev(be, sc)
    ppp = 512
    _, per_g = hand_loop(be, sc, d, ppp)
    black = sc.sfc_albedo == 0
    for c in per_g:
        assert not c["abs_dir"].any() and not c["abs_dif"].any()
        for k in NAMES[:4]:
            assert np.all(c[k] % np.uint64(1 << 32) == 0), k          # all weights stay 0 or 1
        assert int(c["tod_up"].sum()) + int((c["sfc_dn_dir"] + c["sfc_dn_dif"])[black].sum()) == ppp*sc.ncol << 32
    r = solve(be, sc, d, ppp)
    assert np.all(r["abs_dir"] == 0) and np.all(r["abs_dif"] == 0)
    incident = sc.ncol*float(np.sum(sc.inc_dir) + np.sum(sc.inc_dif))
    total = float(np.sum(r["tod_up"]) + np.sum((r["sfc_dn_dir"] + r["sfc_dn_dif"])[black]))
    assert abs(total - incident) <= 1e-12*incident


# ---- E: photon for photon against the numpy restatement

@pytest.fixture(scope="module")
def general_reference():
    sc = S.general(np.float64)
    return sc, R.raytracer_sw(sc, 32)


def test_e_photon_for_photon(general_reference, hip_f64):
    be = hip_f64
    sc, ref = general_reference
    assert ref["n_capped"] == 0
    ppp = 32
    r = solve(be, sc, _dev(be, sc), ppp)
    inc = sc.inc_dir.astype(np.float64) + sc.inc_dif
    tol = float(np.sum(ref["events"] * 2.0**-33 / ppp * inc))         # each deposit rounds once
    for k in NAMES:
        t = tol if k in NAMES[:4] else tol / sc.dz
        err = float(np.max(np.abs(r[k] - ref[k])))
        print(f"raytracer E {k}: max difference {err:.3e} (bound {t:.3e}), max value {float(np.max(ref[k])):.3e}")
        assert ref[k].any(), k
        assert err <= t, k


# ---- F: counts

def test_f_counts_are_additive_reproducible_and_the_loop_is_the_entry(hip_f64):
    be = hip_f64
    sc = S.general(np.float64)
    d = _dev(be, sc)
    n = 32*sc.ncol
    kn = be.rt_k_null(d["tau"], 1, sc.nx, sc.ny, sc.dz, sc.kn_grid, sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"])
    assert np.array_equal(be.to_numpy(kn), R.k_null(sc, 1))
    whole = forward(be, sc, d, 1, 0, n, kn=kn)
    again = forward(be, sc, d, 1, 0, n, kn=kn)
    parts = forward(be, sc, d, 1, 0, n//3, kn=kn)
    parts = forward(be, sc, d, 1, n//3, n - n//3, kn=kn, counts=parts)
    for k in NAMES + ("n_capped",):
        assert np.array_equal(_u64(be, whole[k]), _u64(be, again[k])), k
        assert np.array_equal(_u64(be, whole[k]), _u64(be, parts[k])), k
    assert int(_u64(be, whole["n_capped"])[0]) == 0
    ppp = 32
    flux, _ = hand_loop(be, sc, d, ppp)
    r = solve(be, sc, d, ppp)
    for k in NAMES:
        assert np.array_equal(flux[k].view(np.uint8), r[k].view(np.uint8)), k


def test_a_g_point_without_incident_flux_is_skipped_and_the_cap_is_counted(hip_f64):
    be = hip_f64
    sc = S.general(np.float64)
    d = _dev(be, sc)
    one = S.general(np.float64)
    one.inc_dir = np.array([sc.inc_dir[0], 0.0]); one.inc_dif = np.array([sc.inc_dif[0], 0.0])
    flux, per_g = hand_loop(be, one, d, 8)
    assert per_g[1] is None
    r = solve(be, one, d, 8)
    for k in NAMES:
        assert np.array_equal(flux[k].view(np.uint8), r[k].view(np.uint8)), k
    capped = be.raytracer_sw(d["tau"], d["ssa"], sc.nx, sc.ny, sc.dx, sc.dy, sc.dz, d["alb"], sc.mu0, sc.azimuth, sc.inc_dir, sc.inc_dif,
                             sc.kn_grid, 8, sc.seed, top_at_1=sc.top_at_1, cloud=d["cloud"], band_lims=d["lims"], max_events=1)
    # one event each: every photon that the first event does not end is dropped and counted, none loops
    assert 0 < capped["n_capped"] == R.raytracer_sw(sc, 8, max_events=1)["n_capped"] <= 2*8*sc.ncol


# ---- H: the chain

def _uniform_atmosphere(ncol, nlay):
    atm = synthetic.make_atmosphere(ncol, nlay, nbnd_lw=2, nbnd_sw=2)
    for k, v in atm.__dict__.items():
        if isinstance(v, np.ndarray) and v.ndim >= 1:
            if v.shape[-1] == ncol:
                v[...] = v[..., :1]
            elif v.shape[0] == ncol:
                v[...] = v[:1]
    for v in atm.vmr.values():
        v[...] = v[..., :1]
    return atm


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_h_chain_direct_beam_matches_the_two_stream_solve(dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    nx, ny, nlay, ppp = 4, 4, 12, 1024
    ncol = nx*ny
    kd = be.upload_kdist(synthetic.make_kdist("sw", ngpt=32, nbnd=2, npres=10, nflav=3, nminor_lower=5, nminor_upper=3))
    atm0 = _uniform_atmosphere(ncol, nlay)
    atm = pipeline.upload_atmosphere(be, atm0)
    two = pipeline.solve_sw(be, kd, atm, keep=True)
    gdir = be.to_numpy(two["gpt_flux_dir"]).astype(np.float64)             # (ngpt, nlev, ncol); level 0 is the surface
    assert not atm0.top_at_1
    inc, p = gdir[:, -1, 0], gdir[:, 0, 0] / gdir[:, -1, 0]
    r = pipeline.raytrace_sw(be, kd, atm, nx, ny, 500.0, 500.0, 70.e3/nlay, 0.4, ppp, S.SEED, independent_column=True)
    assert r["n_capped"] == 0
    got = float(np.mean(be.to_numpy(r["sfc_dn_dir"]).astype(np.float64)))
    want = float(np.mean(be.to_numpy(two["flux_dn_dir"])[0].astype(np.float64)))
    sig = float(np.sqrt(np.sum(inc**2 * p*(1.0 - p)) / (ppp*ncol)))
    print(f"raytracer H {dt}: domain-mean direct flux {got:.4f} against {want:.4f} W m-2, {abs(got - want)/sig:.2f} sigma (bound 5)")
    assert abs(got - want) <= 5*sig
    # the sun is one for the domain
    atm0.mu0[3] *= 0.9
    with pytest.raises(ValueError, match="mu0"):
        pipeline.raytrace_sw(be, kd, pipeline.upload_atmosphere(be, atm0), nx, ny, 500.0, 500.0, 70.e3/nlay, 0.4, 8, S.SEED)
    with pytest.raises(ValueError, match="nx ny"):
        pipeline.raytrace_sw(be, kd, atm, nx, ny + 1, 500.0, 500.0, 70.e3/nlay, 0.4, 8, S.SEED)


# ---- the C++ class

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_raytracer_gpu_class_gives_the_entry_bit_for_bit_and_throws(dt, hip_f64, hip_f32):
    """Raytracer_gpu::trace_rays (through rrx_cxx_trace_rays, which wraps the caller's device arrays in Array_gpu views) against
    rrx_raytracer_sw on the general scene; a refused argument comes back as an exception's message."""
    import ctypes
    import os
    import torch
    be = _be(dt, hip_f64, hip_f32)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so" if dt == "f64" else "librte_rrtmgp_hip_sp.so"))
    lib.rrx_cxx_driver_error.restype = ctypes.c_char_p
    F = ctypes.c_double if dt == "f64" else ctypes.c_float
    sc = S.general(be.np_dtype)
    d = _dev(be, sc)
    ppp = 16
    want = solve(be, sc, d, ppp)
    outs = [be.empty((sc.ncol,)) for _ in range(4)] + [be.empty((sc.nz, sc.ncol)) for _ in range(2)]
    out6 = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in outs])
    inc_dir = np.ascontiguousarray(sc.inc_dir, dtype=be.np_dtype); inc_dif = np.ascontiguousarray(sc.inc_dif, dtype=be.np_dtype)
    n_capped = ctypes.c_ulonglong(99)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(mu0):
        return lib.rrx_cxx_trace_rays(sc.nx, sc.ny, sc.nz, 2, 2, F(sc.dx), F(sc.dy), F(sc.dz), int(sc.top_at_1), int(sc.independent_column),
                                      P(d["tau"]), P(d["ssa"]), P(d["lims"]), *(P(c) for c in d["cloud"]), P(d["alb"]), F(mu0), F(sc.azimuth),
                                      inc_dir.ctypes.data_as(ctypes.c_void_p), inc_dif.ctypes.data_as(ctypes.c_void_p), *sc.kn_grid,
                                      ctypes.c_longlong(ppp), ctypes.c_ulonglong(sc.seed), be.RT_MAX_EVENTS, out6, ctypes.byref(n_capped),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert call(sc.mu0) == 0, lib.rrx_cxx_driver_error().decode()
    torch.cuda.synchronize()
    assert n_capped.value == 0
    for k, t in zip(NAMES, outs):
        assert np.array_equal(be.to_numpy(t).view(np.uint8), want[k].view(np.uint8)), k
    assert call(0.0) != 0
    msg = lib.rrx_cxx_driver_error().decode()
    assert "rrx_raytracer_sw" in msg and "mu0" in msg, msg


def test_chain_with_clouds_is_the_entry_on_the_chain_s_own_arrays(hip_f64):
    """pipeline.raytrace_sw with a cloud table, 3-D mode, a coarse k_null grid: the clear gas optics, the band cloud optics without
    delta scaling and inc_dir = solar_source tsi_scaling mu0, made by hand here, give rrx_raytracer_sw the same bits."""
    be = hip_f64
    nx, ny, nlay, ppp = 4, 4, 12, 16
    kd = be.upload_kdist(synthetic.make_kdist("sw", ngpt=32, nbnd=2, npres=10, nflav=3, nminor_lower=5, nminor_upper=3))
    atm0 = synthetic.make_atmosphere(nx*ny, nlay, nbnd_lw=2, nbnd_sw=2, clouds=True)
    atm = pipeline.upload_atmosphere(be, atm0)
    lut = be.upload_lut(synthetic.make_cloud_lut(2, "sw"))
    dz = 70.e3/nlay
    r = pipeline.raytrace_sw(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, ppp, S.SEED, cloud_lut=lut, kn_grid=(2, 2, 3))
    assert r["n_capped"] == 0

    _, col_gas, _ = pipeline.gas_state(be, kd, atm, None, interpolate=False)
    col_dry = be.get_col_dry(atm.vmr["h2o"], atm.p_lev)
    tau, ssa = be.empty((32, nlay, nx*ny)), be.empty((32, nlay, nx*ny))
    be.gas_optics_sw_direct(kd, atm.p_lay, atm.t_lay, col_gas, col_dry, tau, ssa, None)
    cld = be.cloud_optics_2str(lut, atm.lwp, atm.iwp, atm.rel, atm.dei)
    assert float(cld[0].max()) > 0
    inc_dir = (be.to_numpy(kd.solar_source) * atm0.tsi_scaling[0]) * atm0.mu0[0]
    want = be.raytracer_sw(tau, ssa, nx, ny, 400.0, 400.0, dz, be.asarray(atm0.sfc_alb_dif[:, 0].copy()), float(atm0.mu0[0]), 1.1, inc_dir,
                           np.zeros_like(inc_dir), (2, 2, 3), ppp, S.SEED, top_at_1=atm0.top_at_1, cloud=cld, band_lims=kd.band_lims_gpt)
    for k in NAMES:
        assert np.array_equal(be.to_numpy(r[k]).view(np.uint8), be.to_numpy(want[k]).view(np.uint8)), k
    assert float(r["sfc_dn_dif"].max()) > 0 and float(r["tod_up"].max()) > 0 and float(r["abs_dif"].max()) > 0


def test_deep_photon_lists_on_few_threads_give_the_same_integers(hip_f64, monkeypatch):
    """A thread traces a list of photons (photon, photon + threads, ...) and takes the next one inside the event loop. With the
    launch capped at one workgroup the 1 024 photons are four per thread; the counts are those of one photon per thread."""
    be = hip_f64
    sc = S.general(np.float64)
    d = _dev(be, sc)
    n = 32*sc.ncol
    wide = forward(be, sc, d, 0, 7, n)
    monkeypatch.setenv("RRX_RT_MAX_BLOCKS", "1")
    deep = forward(be, sc, d, 0, 7, n)
    monkeypatch.delenv("RRX_RT_MAX_BLOCKS")
    for k in NAMES + ("n_capped",):
        assert np.array_equal(_u64(be, wide[k]), _u64(be, deep[k])), k
    assert _u64(be, wide["tod_up"]).any() and int(_u64(be, wide["n_capped"])[0]) == 0
