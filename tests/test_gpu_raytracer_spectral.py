"""GPU tests of the forward tracer with all g-points in one launch and photons dealt by flux (rrx_rt_k_null_all,
rrx_rt_bg_profile_all, rrx_rt_trace_counts_spectral, rrx_raytracer_sw_spectral; csrc/rrx_rt_common.h). Scenes:
tests/raytracer_spectral_scenes.py (5 g-points in 2 bands, one of them dark, 4 x 4 x 6 and 8 x 4 x 6 cells); restatement:
tests/raytracer_spectral_ref.py. The tallies are integers added with integer atomics, so a run that passes once passes always; the
integer comparisons are exact, the statistical bound is derived in raytracer_spectral_scenes.beer_sigma."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

import raytracer_ref as R
import raytracer_phase_scenes as PS
import raytracer_spectral_ref as SP
import raytracer_spectral_scenes as SS
from raytracer_dev import _be, NO_TRIPLE, dev, device_table, numbers, k_null, k_null_all, forward_bg, forward_spectral, solve_fw_spectral
from rte_rrtmgp_cpp_amd import pipeline

pytestmark = pytest.mark.gpu
FW, NEW = R.COUNT_NAMES, R.BG_COUNT_NAMES
ACTIVE = (0, 1, 3, 4)
CHUNK = "RRX_RT_SPECTRAL_GPT_PER_LAUNCH"


def keys_of(bg):
    return FW + (NEW if bg is not None else ())


# ---- 5: k_null and the profile of all g-points

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_k_null_all_and_bg_profile_all_are_the_per_g_point_entries_slice_by_slice(dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    for make in (SS.general, SS.wide, SS.plain):
        sc, bg = make(be.np_dtype)
        d, dbg = dev(be, sc, bg)
        kn = be.to_numpy(k_null_all(be, sc, d))
        assert kn.shape == (SS.NGPT,) + tuple(sc.kn_grid[::-1])
        for g in range(SS.NGPT):
            one = be.to_numpy(k_null(be, sc, d, g, aer=True))
            assert np.array_equal(kn[g].view(np.uint8), one.view(np.uint8)) and one.max() > 0, (make.__name__, g)
        if bg is not None:
            prof = be.to_numpy(be.rt_bg_profile_all(dbg, d["lims"]))
            assert prof.shape == (SS.NGPT, 7, bg.nbg + 1)
            for g in range(SS.NGPT):
                one = be.to_numpy(be.rt_bg_profile(dbg, g, d["lims"], aerosol=dbg.aerosol))
                assert np.array_equal(prof[g].view(np.uint8), one.view(np.uint8)) and one[0].any(), (make.__name__, g)
    # a background without cloud and aerosol: NULL triples
    sc, bg = SS.beer(be.np_dtype)
    d, dbg = dev(be, sc, bg)
    prof = be.to_numpy(be.rt_bg_profile_all(dbg))
    for g in range(SS.NGPT):
        assert np.array_equal(prof[g].view(np.uint8), be.to_numpy(be.rt_bg_profile(dbg, g, aerosol=NO_TRIPLE)).view(np.uint8))


def _same(be, a, b):
    """bit for bit; a, b: tensors, or numpy arrays of the backend's precision"""
    a, b = (x if isinstance(x, np.ndarray) else be.to_numpy(x) for x in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("grid", ["blocks", "cells"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_one_k_null_kernel_writes_what_the_three_wrote(dt, grid, top_at_1, hip_f64, hip_f32):
    """rrx_rt_k_null, _aer and _all launch one kernel: without aerosol the two-term k_ext, whichever entry, and
    slice g of _all is the per-g-point entry's; all of it the restatement's, bit for bit. blocks: 4 x 2 x 4 cells in blocks of
    2 x 2 x 2. cells: 8 x 8 x 5 with one block per cell, 320 blocks in two workgroups along x, where the slices must not overlap."""
    be = _be(dt, hip_f64, hip_f32)
    sc, _ = SS.setup(be.np_dtype, top_at_1) if grid == "blocks" else SS.setup(be.np_dtype, top_at_1, nx=8, ny=8, nz=5, kn=(8, 8, 5))
    d, _ = dev(be, sc, None)
    null = dict(d, aer=NO_TRIPLE)
    all_null, all_aer = k_null_all(be, sc, null), k_null_all(be, sc, d)
    assert tuple(all_aer.shape) == (3,) + tuple(sc.kn_grid[::-1])
    sc_no_aerosol = dataclasses.replace(sc, aerosol=None)
    for g in range(3):
        two_term = k_null(be, sc, d, g)
        assert _same(be, two_term, k_null(be, sc, null, g, aer=True)), g
        assert _same(be, two_term, all_null[g]) and _same(be, k_null(be, sc, d, g, aer=True), all_aer[g]), g
        assert _same(be, two_term, R.k_null(sc_no_aerosol, g)) and _same(be, all_aer[g], R.k_null(sc, g)), g
        assert not _same(be, two_term, all_aer[g])          # (the aerosol counts)
    if grid == "cells":
        for g in range(2):          # other inputs for slice g+1 leave slice g as it was
            tau = d["tau"].clone()
            tau[g + 1] *= 2
            changed = k_null_all(be, sc, dict(d, tau=tau))
            assert _same(be, changed[g], all_aer[g]) and not _same(be, changed[g + 1], all_aer[g + 1]), g


@pytest.mark.parametrize("nbg", [3, 1])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_one_profile_kernel_writes_what_the_three_wrote(dt, nbg, hip_f64, hip_f32):
    """rrx_rt_bg_profile, _aer and _all launch one kernel in two instantiations: the five rows are the first five of
    the seven, a NULL triple leaves zeros in the other two, slice g of _all is the per-g-point entry's, and all of it is the
    restatement's, bit for bit. (The profile is counted upward from the domain top: top_at_1 is not among its inputs.)"""
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = SS.setup(be.np_dtype, True, nbg=nbg)
    d, dbg = dev(be, sc, bg)
    every = be.rt_bg_profile_all(dbg, d["lims"])
    assert tuple(every.shape) == (3, 7, nbg + 1)
    for g in range(3):
        five, seven = be.to_numpy(be.rt_bg_profile(dbg, g, d["lims"])), be.to_numpy(be.rt_bg_profile(dbg, g, d["lims"], aerosol=NO_TRIPLE))
        assert _same(be, five, seven[:5].copy()) and not seven[5:].any(), g
        assert _same(be, every[g], be.rt_bg_profile(dbg, g, d["lims"], aerosol=dbg.aerosol)), g
        assert _same(be, five, np.ascontiguousarray(R.profile(sc, bg, g, aerosol=False))) and _same(be, every[g], R.profile(sc, bg, g)), g
        assert every[g][5].any()          # (the aerosol aloft counts)


# ---- 6: the sum over g-points

@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("scene", ["general", "plain"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_with_unit_weights_the_counts_are_the_integer_sum_over_g_points(dt, scene, with_table, hip_f64, hip_f32):
    """m_g = 8 on the active g-points and weight0 = 1: every tally and n_capped is the integer sum over g of
    rrx_rt_trace_counts_aer(g, 0, 8 ncol). plain: nbg = 0 and NULL aerosol triples."""
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = getattr(SS, scene)(be.np_dtype)
    d, dbg = dev(be, sc, bg)
    phase = device_table(be, sc) if with_table else None
    m = np.array([8, 8, 0, 8, 8])
    pe, w0, df, _ = SP.photon_list(sc, m)
    w0 = np.where(m > 0, 1.0, 0.0)
    got = numbers(be, forward_spectral(be, sc, d, dbg, (pe, w0, df), 0, int(pe[-1]), phase=phase))
    want = None
    for g in ACTIVE:
        c = numbers(be, forward_bg(be, sc, d, dbg, g, 0, 8*sc.ncol, phase=phase, aer=True))
        want = c if want is None else {k: want[k] + c[k] for k in c}
    assert int(got["n_capped"][0]) == 0
    for k in keys_of(bg) + ("n_capped",):
        assert np.array_equal(got[k], want[k]), k
    assert got["abs_dif"].any() and got["sfc_dn_dif"].any() and (bg is None or got["toa_up"].any())


# ---- 7: ranges and dealing

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_ranges_add_up_and_the_dealing_does_not_matter(dt, hip_f64, hip_f32, monkeypatch):
    """Uneven m_g with their weights on 32 columns (7 workgroups): the whole list equals three ranges, cut inside a g-point and on
    the boundary beside the empty range, and cut on a boundary and just behind the empty range; and a run on one workgroup."""
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = SS.wide(be.np_dtype)
    d, dbg = dev(be, sc, bg)
    m = np.array([24, 4, 0, 20, 8])
    pe, w0, df, _ = SP.photon_list(sc, m)
    n = int(pe[-1])
    assert n > 4*256 and pe[2] == pe[3]
    kn = k_null_all(be, sc, d)
    whole = numbers(be, forward_spectral(be, sc, d, dbg, (pe, w0, df), 0, n, kn=kn))
    assert int(whole["n_capped"][0]) == 0 and all(whole[k].any() for k in NEW)
    for cuts in ((0, int(pe[1]) - 5, int(pe[2]), n), (0, int(pe[1]), int(pe[3]) + 7, n)):
        parts = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts = forward_spectral(be, sc, d, dbg, (pe, w0, df), a, b - a, kn=kn, counts=parts)
        parts = numbers(be, parts)
        for k in FW + NEW + ("n_capped",):
            assert np.array_equal(whole[k], parts[k]), (cuts, k)
    monkeypatch.setenv("RRX_RT_MAX_BLOCKS", "1")
    deep = numbers(be, forward_spectral(be, sc, d, dbg, (pe, w0, df), 0, n, kn=kn))
    monkeypatch.delenv("RRX_RT_MAX_BLOCKS")
    for k in FW + NEW + ("n_capped",):
        assert np.array_equal(whole[k], deep[k]), k
    # the binding refuses a list that does not ascend and a range beyond the list
    bad = pe.copy(); bad[2] = bad[1] - 1
    with pytest.raises(ValueError, match="must not descend"):
        forward_spectral(be, sc, d, dbg, (bad, w0, df), 0, 8, kn=kn)
    with pytest.raises(ValueError, match="beyond the list"):
        forward_spectral(be, sc, d, dbg, (pe, w0, df), n - 4, 8, kn=kn)


# ---- 8: chunking

@pytest.mark.parametrize("scene", ["general", "plain"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_result_does_not_depend_on_the_chunking(dt, scene, hip_f64, hip_f32, monkeypatch):
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = getattr(SS, scene)(be.np_dtype)
    d, dbg = dev(be, sc, bg)
    m = pipeline.spectral_allocation(sc.inc_dir.astype(np.float64) + sc.inc_dif, 24)
    monkeypatch.delenv(CHUNK, raising=False)
    whole = solve_fw_spectral(be, sc, d, dbg, m)
    assert whole["n_capped"] == 0 and whole["abs_dif"].any()
    for chunk in ("1", "2"):
        monkeypatch.setenv(CHUNK, chunk)
        got = solve_fw_spectral(be, sc, d, dbg, m)
        for k in keys_of(bg):
            assert np.array_equal(whole[k].view(np.uint8), got[k].view(np.uint8)), (chunk, k)
        assert got["n_capped"] == 0
    monkeypatch.delenv(CHUNK)
    # no photons at all: zeroed outputs; a refused list
    none = solve_fw_spectral(be, sc, d, dbg, np.zeros(SS.NGPT, dtype=np.int64))
    assert none["n_capped"] == 0 and not any(none[k].any() for k in keys_of(bg))
    with pytest.raises(RuntimeError, match="no incident flux"):
        solve_fw_spectral(be, sc, d, dbg, np.array([1, 1, 1, 1, 1]))
    with pytest.raises(RuntimeError, match="negative at g-point 3"):
        solve_fw_spectral(be, sc, d, dbg, np.array([1, 1, 0, -1, 1]))


# ---- 9: the weights against the restatement

@pytest.mark.parametrize("top_at_1", [False, True])
def test_fluxes_with_uneven_weights_against_the_restatement(top_at_1, hip_f64):
    """The allocation's uneven m_g on the general scene with a table on the cloud. Allowed: events 2^-33 U max(weight0, 1) per
    flux, the form of the photon-for-photon test of test_gpu_raytracer.py: each deposit rounds once, to half a count of 2^-32 U
    (abs_* over dz, bg_abs_*[b] over dz_bg[b] ncol, as the conversion scales them)."""
    import raytracer_phase_ref as P
    be = hip_f64
    sc, bg = SS.general(np.float64, top_at_1)
    d, dbg = dev(be, sc, bg)
    m = pipeline.spectral_allocation(sc.inc_dir + sc.inc_dif, 32)
    assert len(set(m[list(ACTIVE)])) > 2 and m[SS.EMPTY] == 0
    table = P.build_tables(*PS.double_hg33(), np.float64, PS.RE0, PS.DRE)
    table.cld_re = PS.cell_radii(sc, np.float64)
    ref = SP.raytracer_sw(sc, bg, m, table=table)
    got = solve_fw_spectral(be, sc, d, dbg, m, phase=device_table(be, sc))
    assert ref["n_capped"] == 0 and got["n_capped"] == 0
    tol = ref["events"] * 2.0**-33 * float(ref["U"]) * max(float(ref["weight0"].max()), 1.0)
    for k in FW + NEW:
        scale = 1.0 if k in FW[:4] + NEW[:3] else (1.0/sc.dz if k in FW[4:] else 1.0/(bg.dz.astype(np.float64)*sc.ncol))
        err = np.abs(got[k].astype(np.float64) - ref[k])
        print(f"raytracer_spectral against the restatement top_at_1={top_at_1} {k}: worst difference {float(err.max()):.3e} "
              f"(bound {float(np.min(tol*scale)):.3e}), {ref['events']} events, m = {list(m)}")
        assert ref[k].any() or k == "sfc_dn_dir", k
        assert np.all(err <= tol*scale), (k, float(err.max()), tol)


# ---- 10: unbiased

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_weighted_estimate_is_unbiased(dt, hip_f64, hip_f32):
    """Independent columns of purely absorbing gas under 64 photons per pixel dealt by flux: sfc_dn_dir per pixel and its domain
    mean within 5 sigma of sum_g inc_g exp(-tau_g/mu0), sigma from raytracer_spectral_scenes.beer_sigma."""
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = SS.beer(be.np_dtype)
    d, dbg = dev(be, sc, bg)
    m = pipeline.spectral_allocation(sc.inc_dir.astype(np.float64) + sc.inc_dif, 64)
    _, w0, _, U = SP.photon_list(sc, m)
    got = solve_fw_spectral(be, sc, d, dbg, m)
    assert got["n_capped"] == 0
    mean, sigma = SS.beer_sigma(sc, bg, m, w0, U)
    want = (np.array(SS.INC)[:, None]*SS.beer_expected(sc, bg)).sum(axis=0)
    assert np.allclose(mean, want, rtol=1e-5)          # (the weights carry the fluxes: sum_g m_g U weight0_g p_g = sum_g inc_g p_g)
    dev_pix = np.abs(got["sfc_dn_dir"].astype(np.float64) - want) / sigma
    dev_mean = abs(float(got["sfc_dn_dir"].astype(np.float64).mean()) - float(want.mean())) / (float(np.sqrt(np.sum(sigma**2)))/sc.ncol)
    print(f"raytracer_spectral unbiased {dt}: m = {list(m)}, worst deviation {max(float(dev_pix.max()), dev_mean):.2f} sigma (bound 5)")
    assert np.all(dev_pix <= 5) and dev_mean <= 5, (float(dev_pix.max()), dev_mean)
    for k in ("sfc_dn_dif", "sfc_up", "toa_up", "tod_up", "abs_dif"):
        assert not got[k].any(), k


# ---- 11: the pipeline and the C++ class

@pytest.mark.parametrize("n_domain", [None, 4])
def test_the_chain_with_allocation_flux_is_the_entry_on_the_chain_s_own_arrays(n_domain, hip_f64):
    from rte_rrtmgp_cpp_amd import synthetic
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
    args = (be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, P, 77)
    r = pipeline.raytrace_sw(*args, cloud_lut=lut, kn_grid=(2, 1, 2), aerosol_lut=alut, allocation="flux", **split)
    assert r["n_capped"] == 0
    assert set(r) == set(FW + (NEW if n_domain is not None else ())) | {"n_capped"}
    with pytest.raises(ValueError, match="allocation"):
        pipeline.raytrace_sw(*args, allocation="equal")
    with pytest.raises(ValueError, match="cannot give 2 to each of 32"):
        pipeline.raytrace_sw(*args, allocation="flux", min_per_gpt=2)

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
    want = be.raytracer_sw_spectral(part(tau), part(ssa), nx, ny, 400.0, 400.0, dz, be.asarray(atm0.sfc_alb_dif[:, 0].copy()), float(atm0.mu0[0]),
                                    1.1, inc_dir, np.zeros_like(inc_dir), (2, 1, 2), m, 77, top_at_1=top_at_1, cloud=tuple(part(c) for c in cld),
                                    band_lims=kd.band_lims_gpt, background=dbg, aerosol=tuple(part(c) for c in aer))
    for k in FW + (NEW if n_domain is not None else ()):
        assert np.array_equal(be.to_numpy(r[k]).view(np.uint8), be.to_numpy(want[k]).view(np.uint8)) and be.to_numpy(r[k]).any(), k
    # allocation=None is the loop of before
    a = pipeline.raytrace_sw(*args[:-2], 2, 77, cloud_lut=lut, kn_grid=(2, 1, 2), aerosol_lut=alut, **split)
    b = pipeline.raytrace_sw(*args[:-2], 2, 77, cloud_lut=lut, kn_grid=(2, 1, 2), aerosol_lut=alut, allocation=None, **split)
    assert all(np.array_equal(be.to_numpy(a[k]), be.to_numpy(b[k])) for k in FW)


@pytest.mark.parametrize("scene", ["general", "plain"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_cxx_class_gives_the_entry_bit_for_bit_and_throws(dt, scene, hip_f64, hip_f32):
    """Raytracer_gpu::trace_rays_spectral after set_phase_table, set_background and set_aerosol (through rrx_cxx_trace_rays_spectral)
    against rrx_raytracer_sw_spectral, and Raytracer_gpu::spectral_allocation against pipeline.spectral_allocation."""
    import torch
    be = _be(dt, hip_f64, hip_f32)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so" if dt == "f64" else "librte_rrtmgp_hip_sp.so"))
    lib.rrx_cxx_driver_error.restype = ctypes.c_char_p
    F = ctypes.c_double if dt == "f64" else ctypes.c_float
    sc, bg = getattr(SS, scene)(be.np_dtype)
    d, dbg = dev(be, sc, bg)
    nbg = 0 if bg is None else bg.nbg
    phase = device_table(be, sc)
    inc_dir = np.ascontiguousarray(sc.inc_dir, dtype=be.np_dtype); inc_dif = np.ascontiguousarray(sc.inc_dif, dtype=be.np_dtype)
    H = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    none = ctypes.c_void_p(0)

    inc = (inc_dir + inc_dif).astype(be.np_dtype)
    m = np.zeros(SS.NGPT, dtype=np.int64)
    for total, floor in ((40, 1), (5, 1), (64, 3)):
        assert lib.rrx_cxx_spectral_allocation(SS.NGPT, H(inc), ctypes.c_longlong(total), ctypes.c_longlong(floor), H(m)) == 0
        assert np.array_equal(m, pipeline.spectral_allocation(inc, total, floor)), (total, floor, m)
    assert lib.rrx_cxx_spectral_allocation(SS.NGPT, H(inc), ctypes.c_longlong(3), ctypes.c_longlong(1), H(m)) != 0
    assert "cannot give 1 to each of 4" in lib.rrx_cxx_driver_error().decode()
    assert lib.rrx_cxx_spectral_allocation(SS.NGPT, H(inc), ctypes.c_longlong(40), ctypes.c_longlong(1), H(m)) == 0

    outs = [be.empty((sc.ncol,)) for _ in range(4)] + [be.empty((sc.nz, sc.ncol)) for _ in range(2)]
    news = [be.empty((sc.ncol,)) for _ in range(3)] + [be.empty((max(nbg, 1),)) for _ in range(2)]
    out6 = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in outs])
    out5 = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in news])
    n_capped = ctypes.c_ulonglong(99)
    table = (phase.mu.shape[0], phase.phase.shape[1], F(phase.re0), F(phase.dre), P(phase.mu), P(phase.phase), P(phase.cdf), P(phase.cld_re))
    medium = (0, none, none, none, none, none, none) if bg is None else (nbg, H(dbg.dz), P(dbg.tau), P(dbg.ssa), *(P(c) for c in dbg.cloud))
    grid = tuple(none if c is None else P(c) for c in d["aer"])
    aloft = (none, none, none) if bg is None else tuple(P(c) for c in dbg.aerosol)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(m, aer=grid):
        m = np.ascontiguousarray(m, dtype=np.int64)
        return lib.rrx_cxx_trace_rays_spectral(sc.nx, sc.ny, sc.nz, SS.NGPT, SS.NBND, F(sc.dx), F(sc.dy), F(sc.dz), int(sc.top_at_1),
                                               int(sc.independent_column), P(d["tau"]), P(d["ssa"]), P(d["lims"]), *(P(c) for c in d["cloud"]),
                                               P(d["alb"]), F(sc.mu0), F(sc.azimuth), H(inc_dir), H(inc_dif), *sc.kn_grid, H(m),
                                               ctypes.c_ulonglong(sc.seed), be.RT_MAX_EVENTS, out6, ctypes.byref(n_capped), out5, *table, *medium,
                                               *aer, *aloft, stream)

    want = solve_fw_spectral(be, sc, d, dbg, m, phase=phase)
    assert call(m) == 0, lib.rrx_cxx_driver_error().decode()
    torch.cuda.synchronize()
    assert n_capped.value == 0 and want["n_capped"] == 0
    for k, t in zip(keys_of(bg), outs + news):
        assert np.array_equal(be.to_numpy(t).view(np.uint8), want[k].view(np.uint8)) and (want[k].any() or k == "sfc_dn_dir"), k
    for bad, word in ((np.array([1, 1, 1, 1, 1]), "no incident flux"), (np.array([1, -1, 0, 1, 1]), "negative at g-point 1")):
        assert call(bad) != 0
        assert word in lib.rrx_cxx_driver_error().decode()
    if sc.aerosol is not None:
        assert call(m, aer=(grid[0], none, grid[2])) != 0
        assert "Raytracer_gpu::set_aerosol" in lib.rrx_cxx_driver_error().decode()
