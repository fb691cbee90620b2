"""GPU tests of the background atmosphere of the two ray tracers (rrx_rt_bg_profile and the rrx_*_bg entries; csrc/rrx_rt_common.h,
DESIGN 4.17). Scenes: tests/raytracer_bg_scenes.py (a 4 x 3 x 4 grid under 3 background layers of unequal thickness, one of them
empty; 2 g-points in 2 bands; fixed seeds); restatement: tests/raytracer_ref.py (bg=). The tallies are integers added with integer
atomics, so a run that passes once passes always. Bounds are derived, not measured: five sigma of sqrt(p (1 - p)/N) for the
closed forms, the forward bound combined with the standard error of 16 disjoint ray ranges for forward against backward, one count
per deposit (half a count per event, forward) plus 4 eps of the deposited sum ray for ray (two exp / log implementations within
1 ulp each; no decision depends on exp), and for the exact shadow one count per ray (the deposit is one exp of the device against
one of numpy: within 1 ulp of each other, and d 2^32 < 2^32 puts an ulp of d below one count).

Observed on an MI355X: see DESIGN.md 4.17."""
import ctypes
import math
import os

import numpy as np
import pytest

import raytracer_ref as R
import raytracer_bw_ref as B
import raytracer_bg_scenes as SB
import raytracer_bw_scenes as BS
import raytracer_scenes as S
import raytracer_phase_scenes as PS
from raytracer_dev import (_be, _dev, DevBackground, device_table, numbers, clean, forward, backward, solve_fw, solve_bw, forward_bg,
                           backward_bg, solve_fw_bg, solve_bw_bg)
from raytracer_bg_scenes import (check_absorbing, check_conservative, check_split, shadow_full_count, PPP_ABSORBING, PPP_CONSERVATIVE,
                                 PPP_SPLIT)
from rte_rrtmgp_cpp_amd import synthetic, pipeline

pytestmark = pytest.mark.gpu
ONE = float(1 << 32)
FW = R.COUNT_NAMES
NEW = R.BG_COUNT_NAMES


# ---- 3: the profile

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_bg_profile_against_numpy(dt, hip_f64, hip_f32):
    """The kernel and numpy make the same IEEE operations (+, x, / and min) in the same order, so the rows should agree to the bit;
    allowed are 2 ulp of the row's largest term: one for a product that a compiler may fuse into the sum after it, one for the
    quotient (or, in tau_above, for the sum) formed from it."""
    be = _be(dt, hip_f64, hip_f32)
    eps = np.finfo(be.np_dtype).eps
    for make in (SB.general, SB.conservative, SB.absorbing):
        sc, bg = make(be.np_dtype)
        dbg = DevBackground(be, bg)
        for g in range(2):
            got = be.to_numpy(be.rt_bg_profile(dbg, g, be.asarray(sc.band_lims)))
            want = R.profile(sc, bg, g, aerosol=False)
            assert got.shape == (5, bg.nbg + 1)
            for row in range(5):
                tol = 2*eps*float(np.max(np.abs(want[row])))
                err = float(np.max(np.abs(got[row].astype(np.float64) - want[row])))
                assert err <= tol, (make.__name__, g, row, err, tol)
            assert np.all(got[:4, bg.nbg] == 0) and got[4, bg.nbg] >= got[4, 0] >= got[4, bg.nbg - 1] == 0


# ---- 4: nbg = 0 is the medium without a background

@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_without_layers_the_bg_entries_give_the_integers_of_the_existing_entries(dt, with_table, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc = S.general(be.np_dtype)
    d = _dev(be, sc)
    phase = device_table(be, sc) if with_table else None
    n = 16*sc.ncol
    want, got = numbers(be, forward(be, sc, d, 1, 3, n, phase=phase)), numbers(be, forward_bg(be, sc, d, None, 1, 3, n, phase=phase))
    for k in FW + ("n_capped",):
        assert np.array_equal(want[k], got[k]), k
    assert want["tod_up"].any() and not any(got[k].any() for k in NEW)
    for name, sensor in (("perspective", B.Sensor(0, 5, 3, 0.0, (330., 250., 170.), (0.5, 0., 0.1), (0., 0.5, 0.), (0.3, 0.2, -0.9))),
                         ("orthographic", B.orthographic(5, 3, (0.3, -0.2, -0.9))), ("flux down", B.flux_sensor(5, 3, False)),
                         ("flux up", B.flux_sensor(5, 3, True))):
        want = numbers(be, backward(be, sc, d, sensor, 0, 2, 16*15, phase=phase))
        got = numbers(be, backward_bg(be, sc, d, None, sensor, 0, 2, 16*15, phase=phase))
        for k in ("counts", "n_capped", "n_clamped"):
            assert np.array_equal(want[k], got[k]), (name, k)
        assert want["counts"].any(), name
    if dt == "f64":
        a, b = solve_fw(be, sc, d, 8, phase=phase), solve_fw_bg(be, sc, d, None, 8, phase=phase)
        for k in FW:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        cam = B.orthographic(5, 3, (0.3, -0.2, -0.9))
        a, b = solve_bw(be, sc, d, cam, 8, phase=phase), solve_bw_bg(be, sc, d, None, cam, 8, phase=phase)
        assert np.array_equal(be.to_numpy(a["radiance"]).view(np.uint8), be.to_numpy(b["radiance"]).view(np.uint8))


# ---- 5: ray for ray against the restatement

@pytest.fixture(scope="module")
def general_reference():
    sc, bg = SB.general(np.float64)
    return sc, bg, R.raytracer_sw(sc, 32, bg=bg)


def test_photon_for_photon(general_reference, hip_f64):
    be = hip_f64
    sc, bg, ref = general_reference
    assert ref["n_capped"] == 0
    ppp = 32
    r = solve_fw_bg(be, sc, _dev(be, sc), DevBackground(be, bg), ppp)
    assert r["n_capped"] == 0
    inc = sc.inc_dir.astype(np.float64) + sc.inc_dif
    tol = float(np.sum(ref["events"] * 2.0**-33 / ppp * inc))         # each deposit rounds once
    for k in FW + NEW:
        t = tol if k in FW[:4] + NEW[:3] else (tol / sc.dz if k in FW[4:] else tol / float(np.min(bg.dz)) / sc.ncol)
        err = float(np.max(np.abs(r[k] - ref[k])))
        print(f"raytracer_bg photon for photon {k}: max difference {err:.3e} (bound {t:.3e}), max value {float(np.max(ref[k])):.3e}")
        assert ref[k].any(), k
        assert err <= t, k


@pytest.mark.parametrize("kind", ["inside", "aloft", "nadir"])
def test_ray_for_ray(kind, hip_f64):
    be = hip_f64
    sc, bg = SB.general(np.float64)
    sensor = SB.cameras(sc, bg)[kind]
    rpp = 32
    ref = B.raytracer_bw(sc, sensor, rpp, bg=bg)
    assert ref["n_capped"] == 0 and ref["n_clamped"] == 0
    r = solve_bw_bg(be, sc, _dev(be, sc), DevBackground(be, bg), sensor, rpp)
    assert r["n_capped"] == 0 and r["n_clamped"] == 0
    got = be.to_numpy(r["radiance"]).reshape(-1)
    eps = np.finfo(np.float64).eps
    scale = sc.inc_dir.astype(np.float64) / float(sc.mu0) / rpp
    tol = np.sum((ref["n_dep"] * 2.0**-32 + 4*eps*ref["sum_d"]) * scale[:, None], axis=0)
    err = np.abs(got - ref["radiance"])
    print(f"raytracer_bg ray for ray {kind}: max difference {float(err.max()):.3e} W m-2 sr-1 (bound there "
          f"{float(tol[np.argmax(err)]):.3e}), worst difference/bound {float(np.max(err/np.maximum(tol, 1e-300))):.3f}, radiance "
          f"{float(ref['radiance'].min()):.3f} .. {float(ref['radiance'].max()):.3f}, {int(ref['n_dep'].sum())} deposits")
    assert np.all(ref["radiance"] > 0)
    assert np.all(err <= tol)


# ---- 6: the exact shadow

@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("along", ["x", "y"])
def test_shadow_under_an_absorbing_background(along, top_at_1, hip_f64):
    be = hip_f64
    sc, bg = SB.shadow(np.float64, along, top_at_1)
    dark, full = BS.shadow_classes(sc)
    assert dark.sum() == 10 and full.sum() == sc.ncol - 14
    rays = 256
    cam = B.orthographic(sc.nx, sc.ny, (0., 0., -1.))                 # position.z = 0: it starts at the domain top
    counts = clean(be, backward_bg(be, sc, _dev(be, sc), DevBackground(be, bg), cam, 0, 0, rays*sc.ncol))
    want = shadow_full_count(sc, bg, 0, rays)
    assert 0 < want < BS.shadow_full_count(sc, rays)
    assert np.all(counts[dark] == 0), counts[dark] / ONE
    off = np.abs(counts[full].astype(np.int64) - want)
    print(f"raytracer_bg shadow {along} top_at_1={top_at_1}: lit pixels off by at most {int(off.max())} counts of {want} (bound {rays})")
    assert np.all(off <= rays)
    assert np.all(counts[~dark & ~full].astype(np.int64) <= want + rays)


# ---- 7: the closed forms on the device

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("independent_column", [False, True])
def test_absorbing_background_over_an_empty_grid_is_beer(independent_column, dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = SB.absorbing(be.np_dtype, independent_column)
    d, dbg = _dev(be, sc), DevBackground(be, bg)
    for g in range(2):
        c = numbers(be, forward_bg(be, sc, d, dbg, g, 0, PPP_ABSORBING*sc.ncol))
        c["n_capped"] = int(c["n_capped"][0])
        assert c["n_capped"] == 0
        check_absorbing(sc, bg, g, c, PPP_ABSORBING, f"{dt} ic={independent_column}")


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_conservative_scene_loses_nothing(dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = SB.conservative(be.np_dtype)
    d, dbg = _dev(be, sc), DevBackground(be, bg)
    for g in range(2):
        c = numbers(be, forward_bg(be, sc, d, dbg, g, 0, PPP_CONSERVATIVE*sc.ncol))
        c["n_capped"] = int(c["n_capped"][0])
        check_conservative(c, PPP_CONSERVATIVE*sc.ncol, f"{dt} g-point {g}")


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_a_column_split_into_grid_and_background_gives_the_same_fluxes(dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    (a, _), (b, bg) = SB.split(be.np_dtype)
    da, db, dbg = _dev(be, a), _dev(be, b), DevBackground(be, bg)
    for g in range(2):
        ca = numbers(be, forward(be, a, da, g, 0, PPP_SPLIT*a.ncol))
        cb = numbers(be, forward_bg(be, b, db, dbg, g, 0, PPP_SPLIT*b.ncol))
        assert int(ca["n_capped"][0]) == 0 and int(cb["n_capped"][0]) == 0
        check_split(ca, cb, PPP_SPLIT, a.ncol, g, dt)


# ---- 8: forward against backward

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_forward_against_backward(dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = SB.general_direct(be.np_dtype)
    d, dbg = _dev(be, sc), DevBackground(be, bg)
    per_range = (BS.S3_RAYS//BS.S3_RANGES)*sc.ncol
    worst = 0.0
    for g in range(2):
        fwd = numbers(be, forward_bg(be, sc, d, dbg, g, 0, BS.S3_PHOTONS*sc.ncol))
        assert int(fwd["n_capped"][0]) == 0
        for name, sensor in SB.flux_sensors(sc).items():
            ranges = np.stack([clean(be, backward_bg(be, sc, d, dbg, sensor, g, n*per_range, per_range)) for n in range(BS.S3_RANGES)])
            worst = max(worst, BS.compare_forward_backward(sc, g, name, fwd[name], ranges, f"bg {dt}"))
    print(f"raytracer_bg forward against backward {dt}: worst difference {worst:.2f} combined sigma (bound 5)")


# ---- 9: reproducibility and identity

def test_counts_are_additive_reproducible_and_the_loop_is_the_entry(hip_f64):
    be = hip_f64
    F = np.float64
    sc, bg = SB.general(np.float64)
    d, dbg = _dev(be, sc), DevBackground(be, bg)
    n = 32*sc.ncol
    whole, again = numbers(be, forward_bg(be, sc, d, dbg, 1, 0, n)), numbers(be, forward_bg(be, sc, d, dbg, 1, 0, n))
    parts = forward_bg(be, sc, d, dbg, 1, 0, n//3)
    parts = numbers(be, forward_bg(be, sc, d, dbg, 1, n//3, n - n//3, counts=parts))
    for k in FW + NEW + ("n_capped",):
        assert np.array_equal(whole[k], again[k]) and np.array_equal(whole[k], parts[k]), k
    assert int(whole["n_capped"][0]) == 0 and all(whole[k].any() for k in NEW)
    cam = SB.cameras(sc, bg)["aloft"]
    m = 32*12
    whole, again = numbers(be, backward_bg(be, sc, d, dbg, cam, 1, 0, m)), numbers(be, backward_bg(be, sc, d, dbg, cam, 1, 0, m))
    parts = backward_bg(be, sc, d, dbg, cam, 1, 0, m//3)
    parts = numbers(be, backward_bg(be, sc, d, dbg, cam, 1, m//3, m - m//3, counts=parts))
    for k in ("counts", "n_capped", "n_clamped"):
        assert np.array_equal(whole[k], again[k]) and np.array_equal(whole[k], parts[k]), k
    assert whole["counts"].all()

    # the hand loops: the profile, the trace and rrx_rt_counts_to_flux, g-point by g-point
    ppp = 16
    flux = {k: be.zeros((sc.ncol,)) for k in FW[:4] + NEW[:3]}
    flux.update({k: be.zeros((sc.nz, sc.ncol)) for k in FW[4:]})
    flux.update({k: be.zeros((bg.nbg,)) for k in NEW[3:]})
    radiance = be.zeros((12,))
    for g in range(2):
        inc = F(sc.inc_dir[g]) + F(sc.inc_dif[g])
        c = forward_bg(be, sc, d, dbg, g, 0, ppp*sc.ncol)
        scale = inc / F(ppp)
        for k in FW + NEW[:3]:
            be.rt_counts_to_flux(c[k], float(scale if k in FW[:4] + NEW[:3] else scale / F(sc.dz)), flux[k])
        for k in NEW[3:]:
            for b in range(bg.nbg):
                be.rt_counts_to_flux(c[k][b:b+1], float((scale / F(bg.dz[b])) / F(sc.ncol)), flux[k][b:b+1])
        cb = backward_bg(be, sc, d, dbg, cam, g, 0, ppp*12)
        be.rt_counts_to_flux(cb["counts"], float(F(sc.inc_dir[g]) / (F(sc.mu0)*F(ppp))), radiance)
    r = solve_fw_bg(be, sc, d, dbg, ppp)
    for k in FW + NEW:
        assert np.array_equal(be.to_numpy(flux[k]).view(np.uint8), r[k].view(np.uint8)), k
    rb = solve_bw_bg(be, sc, d, dbg, cam, ppp)
    assert np.array_equal(be.to_numpy(radiance).view(np.uint8), be.to_numpy(rb["radiance"]).reshape(-1).view(np.uint8))


def test_a_phase_table_applies_inside_the_grid_only(hip_f64):
    """With a table the grid's cloud scatters by it and the background's cloud by Henyey-Greenstein (the restatement takes table=
    for the grid alone): the counts differ from the Henyey-Greenstein run, are reproducible, and are the restatement's."""
    be = hip_f64
    sc, bg = SB.general(np.float64)
    d, dbg = _dev(be, sc), DevBackground(be, bg)
    phase = device_table(be, sc)
    n = 16*sc.ncol
    hg, tab = numbers(be, forward_bg(be, sc, d, dbg, 1, 0, n)), numbers(be, forward_bg(be, sc, d, dbg, 1, 0, n, phase=phase))
    again = numbers(be, forward_bg(be, sc, d, dbg, 1, 0, n, phase=phase))
    assert int(tab["n_capped"][0]) == 0
    assert any(not np.array_equal(hg[k], tab[k]) for k in FW + NEW)
    for k in FW + NEW:
        assert np.array_equal(tab[k], again[k]), k
    import raytracer_phase_ref as P
    ref_table = P.build_tables(*PS.double_hg33(), np.float64, PS.RE0, PS.DRE)
    ref_table.cld_re = PS.cell_radii(sc, np.float64)
    ref = R.trace_counts(sc, 1, 0, n, table=ref_table, bg=bg)
    assert ref["n_capped"] == 0
    for k in FW + NEW:          # each deposit rounds once: half a count per event
        off = np.abs(tab[k].reshape(-1).astype(np.int64) - ref[k].reshape(-1).astype(np.int64))
        assert int(off.max()) <= ref["events"]//2 + 1, (k, int(off.max()))
    cam = SB.cameras(sc, bg)["nadir"]
    a, b = clean(be, backward_bg(be, sc, d, dbg, cam, 1, 0, 16*12)), clean(be, backward_bg(be, sc, d, dbg, cam, 1, 0, 16*12, phase=phase))
    assert a.all() and b.all() and not np.array_equal(a, b)


@pytest.mark.parametrize("top_at_1", [False, True])
def test_the_chain_with_n_domain_is_the_entry_on_the_chain_s_own_arrays(top_at_1, hip_f64):
    """pipeline.raytrace_sw / render_sw with n_domain: the lowest n_domain layers as the grid and the layers above, from column 0
    and counted upward, as the background, made by hand here, give the _bg entries the same bits."""
    from rte_rrtmgp_cpp_amd import camera as C
    be = hip_f64
    nx, ny, nlay, nd, ppp = 4, 3, 12, 4, 8
    kd = be.upload_kdist(synthetic.make_kdist("sw", ngpt=32, nbnd=2, npres=10, nflav=3, nminor_lower=5, nminor_upper=3))
    atm0 = synthetic.make_atmosphere(nx*ny, nlay, nbnd_lw=2, nbnd_sw=2, clouds=True, top_at_1=top_at_1)
    atm = pipeline.upload_atmosphere(be, atm0)
    lut = be.upload_lut(synthetic.make_cloud_lut(2, "sw"))
    dz = 500.0
    z_up = np.concatenate([np.arange(nd + 1)*dz, nd*dz + np.cumsum(np.linspace(700., 9000., nlay - nd))])
    z_lev = z_up[::-1].copy() if top_at_1 else z_up
    r = pipeline.raytrace_sw(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, ppp, S.SEED, cloud_lut=lut, kn_grid=(2, 1, 2), n_domain=nd, z_lev=z_lev)
    assert r["n_capped"] == 0
    cam = C.perspective(4, 3, (800., 700., 5.e3), yaw=0.4, pitch=-1.0, fov=math.radians(50.))
    rb = pipeline.render_sw(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, cam, ppp, S.SEED, cloud_lut=lut, kn_grid=(2, 1, 2), n_domain=nd, z_lev=z_lev)
    assert rb["n_capped"] == 0 and rb["n_clamped"] == 0

    _, col_gas, _ = pipeline.gas_state(be, kd, atm, None, interpolate=False)
    col_dry = be.get_col_dry(atm.vmr["h2o"], atm.p_lev)
    tau, ssa = be.empty((32, nlay, nx*ny)), be.empty((32, nlay, nx*ny))
    be.gas_optics_sw_direct(kd, atm.p_lay, atm.t_lay, col_gas, col_dry, tau, ssa, None)
    cld = be.cloud_optics_2str(lut, atm.lwp, atm.iwp, atm.rel, atm.dei)
    grid = slice(nlay - nd, nlay) if top_at_1 else slice(0, nd)
    above = list(range(nlay - nd - 1, -1, -1)) if top_at_1 else list(range(nd, nlay))

    class Bg:
        pass
    dbg = Bg()
    dbg.dz = np.diff(z_up)[nd:].copy()
    dbg.tau, dbg.ssa = tau[:, above, 0].contiguous(), ssa[:, above, 0].contiguous()
    dbg.cloud = tuple(c[:, above, 0].contiguous() for c in cld)
    part = lambda t: t[:, grid, :].contiguous()
    inc_dir = (be.to_numpy(kd.solar_source) * atm0.tsi_scaling[0]) * atm0.mu0[0]
    alb = be.asarray(atm0.sfc_alb_dif[:, 0].copy())
    cloud = tuple(part(c) for c in cld)
    want = be.raytracer_sw_bg(part(tau), part(ssa), nx, ny, 400.0, 400.0, dz, alb, float(atm0.mu0[0]), 1.1, inc_dir, np.zeros_like(inc_dir),
                              (2, 1, 2), ppp, S.SEED, top_at_1=top_at_1, cloud=cloud, band_lims=kd.band_lims_gpt, background=dbg)
    for k in FW + NEW:
        assert np.array_equal(be.to_numpy(r[k]).view(np.uint8), be.to_numpy(want[k]).view(np.uint8)), k
        assert float(want[k].max()) > 0 or k == "sfc_dn_dir", k
    wb = be.raytracer_bw_bg(part(tau), part(ssa), nx, ny, 400.0, 400.0, dz, alb, float(atm0.mu0[0]), 1.1, inc_dir, (2, 1, 2), cam, ppp, S.SEED,
                            top_at_1=top_at_1, cloud=cloud, band_lims=kd.band_lims_gpt, background=dbg)
    assert np.array_equal(be.to_numpy(rb["radiance"]).view(np.uint8), be.to_numpy(wb["radiance"]).view(np.uint8))
    assert float(rb["radiance"].min()) > 0
    with pytest.raises(ValueError, match="n_domain"):
        pipeline.raytrace_sw(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, ppp, S.SEED, n_domain=nlay, z_lev=z_lev)
    with pytest.raises(ValueError, match="z_lev"):
        pipeline.render_sw(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, cam, ppp, S.SEED, n_domain=nd)


@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_cxx_classes_with_a_background_give_the_entries_bit_for_bit_and_throw(dt, top_at_1, hip_f64, hip_f32):
    """Raytracer_gpu / Raytracer_bw_gpu after set_background (through rrx_cxx_trace_rays_bg / rrx_cxx_trace_rays_bw_bg) against
    rrx_raytracer_sw_bg / rrx_raytracer_bw_bg; a refused argument comes back as an exception's message."""
    import torch
    be = _be(dt, hip_f64, hip_f32)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so" if dt == "f64" else "librte_rrtmgp_hip_sp.so"))
    lib.rrx_cxx_driver_error.restype = ctypes.c_char_p
    F = ctypes.c_double if dt == "f64" else ctypes.c_float
    sc, bg = SB.general(be.np_dtype, top_at_1)
    d, dbg = _dev(be, sc), DevBackground(be, bg)
    ppp = 16
    want = solve_fw_bg(be, sc, d, dbg, ppp)
    outs = [be.empty((sc.ncol,)) for _ in range(4)] + [be.empty((sc.nz, sc.ncol)) for _ in range(2)]
    news = [be.empty((sc.ncol,)) for _ in range(3)] + [be.empty((bg.nbg,)) for _ in range(2)]
    out6 = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in outs])
    out5 = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in news])
    inc_dir = np.ascontiguousarray(sc.inc_dir, dtype=be.np_dtype); inc_dif = np.ascontiguousarray(sc.inc_dif, dtype=be.np_dtype)
    n_capped, n_clamped = ctypes.c_ulonglong(99), ctypes.c_ulonglong(99)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    H = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    none = ctypes.c_void_p(0)
    table = (0, 0, F(0.), F(0.), none, none, none, none)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def medium(dz):
        return (bg.nbg, H(dz), P(dbg.tau), P(dbg.ssa), *(P(c) for c in dbg.cloud))

    def call(dz):
        return lib.rrx_cxx_trace_rays_bg(sc.nx, sc.ny, sc.nz, 2, 2, F(sc.dx), F(sc.dy), F(sc.dz), int(sc.top_at_1), int(sc.independent_column),
                                         P(d["tau"]), P(d["ssa"]), P(d["lims"]), *(P(c) for c in d["cloud"]), P(d["alb"]), F(sc.mu0), F(sc.azimuth),
                                         H(inc_dir), H(inc_dif), *sc.kn_grid, ctypes.c_longlong(ppp), ctypes.c_ulonglong(sc.seed), be.RT_MAX_EVENTS,
                                         out6, ctypes.byref(n_capped), out5, *table, *medium(dz), stream)

    assert call(dbg.dz) == 0, lib.rrx_cxx_driver_error().decode()
    torch.cuda.synchronize()
    assert n_capped.value == 0 and want["n_capped"] == 0
    for k, t in zip(FW + NEW, outs + news):
        assert np.array_equal(be.to_numpy(t).view(np.uint8), want[k].view(np.uint8)), k
    bad = dbg.dz.copy(); bad[1] = 0.
    assert call(bad) != 0
    msg = lib.rrx_cxx_driver_error().decode()
    assert "rrx_raytracer_sw_bg" in msg and "dz_bg" in msg, msg

    cam = SB.cameras(sc, bg)["aloft"]
    wantb = solve_bw_bg(be, sc, d, dbg, cam, ppp)
    out = be.empty((cam.npy, cam.npx))
    nums = np.concatenate([np.asarray(v, dtype=np.float64) for v in (cam.position, cam.e_w, cam.e_h, cam.e_d)]).astype(be.np_dtype)

    def callb(dz):
        return lib.rrx_cxx_trace_rays_bw_bg(sc.nx, sc.ny, sc.nz, 2, 2, F(sc.dx), F(sc.dy), F(sc.dz), int(sc.top_at_1),
                                            P(d["tau"]), P(d["ssa"]), P(d["lims"]), *(P(c) for c in d["cloud"]), P(d["alb"]), F(sc.mu0),
                                            F(sc.azimuth), H(inc_dir), *sc.kn_grid, cam.type, cam.npx, cam.npy, F(cam.fov), H(nums),
                                            ctypes.c_longlong(ppp), ctypes.c_ulonglong(sc.seed), be.RT_MAX_EVENTS, P(out), ctypes.byref(n_capped),
                                            ctypes.byref(n_clamped), *table, *medium(dz), stream)

    assert callb(dbg.dz) == 0, lib.rrx_cxx_driver_error().decode()
    torch.cuda.synchronize()
    assert n_capped.value == 0 and n_clamped.value == 0 and wantb["n_capped"] == 0
    assert np.array_equal(be.to_numpy(out).view(np.uint8), be.to_numpy(wantb["radiance"]).view(np.uint8))
    assert callb(bad) != 0
    msg = lib.rrx_cxx_driver_error().decode()
    assert "rrx_raytracer_bw_bg" in msg and "dz_bg" in msg, msg
