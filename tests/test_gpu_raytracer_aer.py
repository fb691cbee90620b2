"""GPU tests of aerosol as a third scattering species of the two ray tracers (rrx_rt_k_null_aer, rrx_rt_bg_profile_aer and the
rrx_*_aer entries; csrc/rrx_rt_common.h). Scenes: tests/raytracer_aer_scenes.py (the 4 x 3 x 4 grid under 3
background layers of raytracer_bg_scenes; 2 g-points in 2 bands; fixed seeds); restatement: tests/raytracer_ref.py (Scene.aerosol, Background.aerosol). The tallies
are integers added with integer atomics, so a run that passes once passes always. Bounds are derived, not measured, and are those
of test_gpu_raytracer_bg.py: five sigma of sqrt(p (1 - p)/N) for the closed forms, the forward bound combined with the standard
error of 16 disjoint ray ranges for forward against backward, 2 ulp of a row's largest term for the profile. Against the
restatement every count is equal, photon for photon and ray for ray."""
import math

import numpy as np
import pytest

import raytracer_ref as R
import raytracer_bw_ref as B
import raytracer_bg_scenes as SB
import raytracer_bw_scenes as BS
import raytracer_scenes as S
import raytracer_phase_scenes as PS
import raytracer_aer_scenes as SA
from raytracer_dev import (_be, NO_TRIPLE, DevBackground, dev, device_table, numbers, clean, k_null, forward_bg, backward_bg, solve_fw_bg,
                           solve_bw_bg)

pytestmark = pytest.mark.gpu
ONE = float(1 << 32)
FW = R.COUNT_NAMES
NEW = R.BG_COUNT_NAMES
BWK = ("counts", "n_capped", "n_clamped")


# ---- 1: the profile and k_null

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_profile_and_k_null_against_numpy(dt, hip_f64, hip_f32):
    """The kernels and numpy make the same IEEE operations in the same order; allowed are 2 ulp of the row's largest term, as in
    the profile test of test_gpu_raytracer_bg.py."""
    be = _be(dt, hip_f64, hip_f32)
    eps = np.finfo(be.np_dtype).eps
    for make in (SA.general, SA.conservative, SA.beer):
        sc, bg = make(be.np_dtype)
        d, dbg = dev(be, sc, bg)
        for g in range(2):
            got = be.to_numpy(be.rt_bg_profile(dbg, g, d["lims"], aerosol=dbg.aerosol))
            want = R.profile(sc, bg, g)
            assert got.shape == (7, bg.nbg + 1)
            for row in range(7):
                tol = 2*eps*float(np.max(np.abs(want[row])))
                err = float(np.max(np.abs(got[row].astype(np.float64) - want[row])))
                assert err <= tol, (make.__name__, g, row, err, tol)
            assert np.all(got[:4, bg.nbg] == 0) and np.all(got[5:, bg.nbg] == 0) and got[4, bg.nbg] >= got[4, 0] >= got[4, bg.nbg - 1] == 0
            assert got[5].any() == (make is not SA.beer)          # (an aerosol that only absorbs has k_sca_aer = 0)
            got, want = be.to_numpy(k_null(be, sc, d, g, aer=True)), R.k_null(sc, g)
            assert got.shape == want.shape
            assert float(np.max(np.abs(got.astype(np.float64) - want))) <= 2*eps*float(want.max()), (make.__name__, g)
    # a NULL triple writes zeros into the two new rows and the five rows of rrx_rt_bg_profile
    sc, bg = SB.general(be.np_dtype)
    dbg = DevBackground(be, bg)
    five, seven = be.to_numpy(be.rt_bg_profile(dbg, 1, be.asarray(sc.band_lims))), be.to_numpy(be.rt_bg_profile(dbg, 1, be.asarray(sc.band_lims), aerosol=NO_TRIPLE))
    assert np.array_equal(five, seven[:5]) and not seven[5:].any()


# ---- 2: no aerosol is today

@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_without_aerosol_the_aer_entries_give_the_integers_of_the_bg_entries(dt, with_table, with_bg, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc0, bg0 = SB.general(be.np_dtype)
    bg0 = bg0 if with_bg else None
    grid, aloft = SA.zeros(be.np_dtype)
    grid, aloft = (grid[0], grid[1] + 0.9, grid[2] + 0.7), (aloft[0], aloft[1] + 0.9, aloft[2] + 0.7)          # tau_a = 0 with ssa_a, g_a that are not
    cam = SB.cameras(sc0, SB.general(be.np_dtype)[1])
    sensors = ("inside", "nadir") + (("aloft",) if with_bg else ())
    d0, dbg0 = dev(be, sc0, bg0)
    phase = device_table(be, sc0) if with_table else None
    n, m = 16*sc0.ncol, 16*12
    want = numbers(be, forward_bg(be, sc0, d0, dbg0, 1, 3, n, phase=phase, aer=False))
    want_bw = {s: numbers(be, backward_bg(be, sc0, d0, dbg0, cam[s], 1, 2, m, phase=phase, aer=False)) for s in sensors}
    assert want["abs_dif"].any() and all(w["counts"].any() for w in want_bw.values())
    for how, in_grid, in_bg in (("NULL", None, None), ("zeros", grid, aloft)):
        sc, bg = SB.general(be.np_dtype)
        sc.aerosol, bg.aerosol = in_grid, in_bg
        d, dbg = dev(be, sc, bg if with_bg else None)
        got = numbers(be, forward_bg(be, sc, d, dbg, 1, 3, n, phase=phase, aer=True))
        for k in FW + NEW + ("n_capped",):
            assert np.array_equal(want[k], got[k]), (how, k)
        for s in sensors:
            got = numbers(be, backward_bg(be, sc, d, dbg, cam[s], 1, 2, m, phase=phase, aer=True))
            for k in BWK:
                assert np.array_equal(want_bw[s][k], got[k]), (how, s, k)
        a, b = solve_fw_bg(be, sc0, d0, dbg0, 8, phase=phase, aer=False), solve_fw_bg(be, sc, d, dbg, 8, phase=phase, aer=True)
        for k in FW + NEW:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (how, k)
        a, b = solve_bw_bg(be, sc0, d0, dbg0, cam["nadir"], 8, phase=phase, aer=False), solve_bw_bg(be, sc, d, dbg, cam["nadir"], 8, phase=phase, aer=True)
        assert np.array_equal(be.to_numpy(a["radiance"]).view(np.uint8), be.to_numpy(b["radiance"]).view(np.uint8)), how


# ---- 3: swap

@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_swap_cloud_and_aerosol(dt, top_at_1, hip_f64, hip_f32):
    """T as cloud and no aerosol (A) against no cloud and T as aerosol (B), grid and background: every tally and n_capped agree
    integer for integer. The formulas of DESIGN 4.18 make this exact; a difference means the species draw or the parentheses."""
    be = _be(dt, hip_f64, hip_f32)
    (sa, ba), (sb, bb) = SA.swap(be.np_dtype, top_at_1)
    (da, dba), (db, dbb) = dev(be, sa, ba), dev(be, sb, bb)
    n = 32*sa.ncol
    for g in range(2):
        ca, cb = numbers(be, forward_bg(be, sa, da, dba, g, 0, n, aer=True)), numbers(be, forward_bg(be, sb, db, dbb, g, 0, n, aer=True))
        for k in FW + NEW + ("n_capped",):
            assert np.array_equal(ca[k], cb[k]), (g, k)
        assert ca["abs_dif"].any() and ca["toa_up"].any()
        for name, cam in SB.cameras(sa, ba).items():
            ra, rb = numbers(be, backward_bg(be, sa, da, dba, cam, g, 0, 32*12, aer=True)), numbers(be, backward_bg(be, sb, db, dbb, cam, g, 0, 32*12, aer=True))
            for k in BWK:
                assert np.array_equal(ra[k], rb[k]), (g, name, k)
            assert ra["counts"].any()


# ---- 4: photon for photon and ray for ray

def _ref_table(sc):
    import raytracer_phase_ref as P
    t = P.build_tables(*PS.double_hg33(), np.float64, PS.RE0, PS.DRE)
    t.cld_re = PS.cell_radii(sc, np.float64)
    return t


@pytest.mark.parametrize("top_at_1", [False, True])
def test_photon_for_photon(top_at_1, hip_f64):
    """the general scene with a table on the cloud and aerosol in the grid and the background: every count of every tally is the
    restatement's. (The numbers that are tallied are products and quotients; log, exp, sin, cos, cbrt and sqrt of the device and of
    numpy enter only through directions and free paths, and on this scene they decide no cell and change no rounded count.)"""
    be = hip_f64
    sc, bg = SA.general(np.float64, top_at_1)
    d, dbg = dev(be, sc, bg)
    n = 32*sc.ncol
    for g in range(2):
        ref = R.trace_counts(sc, g, 0, n, table=_ref_table(sc), bg=bg)
        got = numbers(be, forward_bg(be, sc, d, dbg, g, 0, n, phase=device_table(be, sc), aer=True))
        assert ref["n_capped"] == 0 and int(got["n_capped"][0]) == 0
        for k in FW + NEW:
            off = np.abs(got[k].reshape(-1).astype(np.int64) - ref[k].reshape(-1).astype(np.int64))
            print(f"raytracer_aer photon for photon top_at_1={top_at_1} g-point {g} {k}: worst difference {int(off.max())} counts of 2^-32, "
                  f"{ref['events']} events")
            assert ref[k].any() or k == "sfc_dn_dir", k
            assert np.array_equal(got[k].reshape(-1), ref[k].reshape(-1)), (g, k, int(off.max()))


@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("kind", ["inside", "aloft", "nadir"])
def test_ray_for_ray(kind, top_at_1, hip_f64):
    be = hip_f64
    sc, bg = SA.general(np.float64, top_at_1)
    sensor = SB.cameras(sc, bg)[kind]
    d, dbg = dev(be, sc, bg)
    n = 32*12
    for g in range(2):
        ref = B.trace_counts_bw(sc, sensor, g, 0, n, table=_ref_table(sc), bg=bg)
        assert ref["n_capped"] == 0 and ref["n_clamped"] == 0
        got = clean(be, backward_bg(be, sc, d, dbg, sensor, g, 0, n, phase=device_table(be, sc), aer=True))
        off = np.abs(got.astype(np.int64) - ref["counts"].astype(np.int64))
        print(f"raytracer_aer ray for ray {kind} top_at_1={top_at_1} g-point {g}: worst difference {int(off.max())} counts of 2^-32, "
              f"{int(ref['n_dep'].sum())} deposits")
        assert np.all(ref["counts"] > 0)
        assert np.array_equal(got, ref["counts"]), (g, int(off.max()))


# ---- 5: Beer

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("independent_column", [False, True])
def test_a_purely_absorbing_aerosol_is_beer(independent_column, dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = SA.beer(be.np_dtype, independent_column)
    d, dbg = dev(be, sc, bg)
    for g in range(2):
        c = numbers(be, forward_bg(be, sc, d, dbg, g, 0, SA.PPP_BEER*sc.ncol, aer=True))
        assert int(c["n_capped"][0]) == 0
        SA.check_beer(sc, bg, g, c, SA.PPP_BEER, f"{dt} ic={independent_column}")


# ---- 6: forward against backward

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_forward_against_backward(dt, hip_f64, hip_f32):
    be = _be(dt, hip_f64, hip_f32)
    sc, bg = SA.general_direct(be.np_dtype)
    d, dbg = dev(be, sc, bg)
    per_range = (BS.S3_RAYS//BS.S3_RANGES)*sc.ncol
    worst = 0.0
    for g in range(2):
        fwd = numbers(be, forward_bg(be, sc, d, dbg, g, 0, BS.S3_PHOTONS*sc.ncol, max_events=SA.MAX_EVENTS, aer=True))
        assert int(fwd["n_capped"][0]) == 0
        for name, sensor in SB.flux_sensors(sc).items():
            ranges = np.stack([clean(be, backward_bg(be, sc, d, dbg, sensor, g, n*per_range, per_range, max_events=SA.MAX_EVENTS, aer=True))
                               for n in range(BS.S3_RANGES)])
            worst = max(worst, BS.compare_forward_backward(sc, g, name, fwd[name], ranges, f"aer {dt}"))
    print(f"raytracer_aer forward against backward {dt}: worst difference {worst:.2f} combined sigma (bound 5)")


# ---- 7: the table is the cloud's alone

def test_the_table_is_the_cloud_s_alone(hip_f64):
    """aerosol is the only scatterer (the gas and the cloud absorb): a sharply peaked phase table changes nothing"""
    be = hip_f64
    sc, bg = SA.aerosol_only(np.float64)
    d, dbg = dev(be, sc, bg)
    mu = np.cos(np.linspace(np.pi, 0., 257))
    peaked = np.broadcast_to(np.exp(40.*(mu - 1.)) + 1.e-6, (2, 3, mu.size)).copy()
    phase = device_table(be, sc, (mu, peaked))
    n = 32*sc.ncol
    hg, tab = numbers(be, forward_bg(be, sc, d, dbg, 1, 0, n, aer=True)), numbers(be, forward_bg(be, sc, d, dbg, 1, 0, n, phase=phase, aer=True))
    for k in FW + NEW + ("n_capped",):
        assert np.array_equal(hg[k], tab[k]), k
    assert hg["sfc_dn_dif"].any() and hg["toa_up"].any()
    for name, cam in SB.cameras(sc, bg).items():
        a, b = numbers(be, backward_bg(be, sc, d, dbg, cam, 1, 0, 32*12, aer=True)), numbers(be, backward_bg(be, sc, d, dbg, cam, 1, 0, 32*12, phase=phase, aer=True))
        for k in BWK:
            assert np.array_equal(a[k], b[k]), (name, k)
        assert a["counts"].any()
    # the same table on a scene whose cloud scatters does change the counts
    sc, bg = SA.general(np.float64)
    d, dbg = dev(be, sc, bg)
    hg, tab = numbers(be, forward_bg(be, sc, d, dbg, 1, 0, n, aer=True)), numbers(be, forward_bg(be, sc, d, dbg, 1, 0, n, phase=device_table(be, sc, (mu, peaked)), aer=True))
    assert any(not np.array_equal(hg[k], tab[k]) for k in FW + NEW)


# ---- 8: additivity, reproducibility, and the loops

@pytest.mark.parametrize("with_table", [False, True])
def test_counts_are_additive_reproducible_and_the_loops_are_the_entries(with_table, hip_f64):
    be = hip_f64
    F = np.float64
    sc, bg = SA.general(np.float64)
    d, dbg = dev(be, sc, bg)
    phase = device_table(be, sc) if with_table else None
    n = 32*sc.ncol
    whole, again = numbers(be, forward_bg(be, sc, d, dbg, 1, 0, n, phase=phase, aer=True)), numbers(be, forward_bg(be, sc, d, dbg, 1, 0, n, phase=phase, aer=True))
    parts = forward_bg(be, sc, d, dbg, 1, 0, n//3, phase=phase, aer=True)
    parts = numbers(be, forward_bg(be, sc, d, dbg, 1, n//3, n - n//3, phase=phase, counts=parts, aer=True))
    for k in FW + NEW + ("n_capped",):
        assert np.array_equal(whole[k], again[k]) and np.array_equal(whole[k], parts[k]), k
    assert int(whole["n_capped"][0]) == 0 and all(whole[k].any() for k in NEW)
    cam = SB.cameras(sc, bg)["aloft"]
    m = 32*12
    whole, again = numbers(be, backward_bg(be, sc, d, dbg, cam, 1, 0, m, phase=phase, aer=True)), numbers(be, backward_bg(be, sc, d, dbg, cam, 1, 0, m, phase=phase, aer=True))
    parts = backward_bg(be, sc, d, dbg, cam, 1, 0, m//3, phase=phase, aer=True)
    parts = numbers(be, backward_bg(be, sc, d, dbg, cam, 1, m//3, m - m//3, phase=phase, counts=parts, aer=True))
    for k in BWK:
        assert np.array_equal(whole[k], again[k]) and np.array_equal(whole[k], parts[k]), k
    assert whole["counts"].all()

    # the hand loops: k_null, the profile, the trace and rrx_rt_counts_to_flux, g-point by g-point
    ppp = 16
    flux = {k: be.zeros((sc.ncol,)) for k in FW[:4] + NEW[:3]}
    flux.update({k: be.zeros((sc.nz, sc.ncol)) for k in FW[4:]})
    flux.update({k: be.zeros((bg.nbg,)) for k in NEW[3:]})
    radiance = be.zeros((12,))
    for g in range(2):
        inc = F(sc.inc_dir[g]) + F(sc.inc_dif[g])
        c = forward_bg(be, sc, d, dbg, g, 0, ppp*sc.ncol, phase=phase, aer=True)
        scale = inc / F(ppp)
        for k in FW + NEW[:3]:
            be.rt_counts_to_flux(c[k], float(scale if k in FW[:4] + NEW[:3] else scale / F(sc.dz)), flux[k])
        for k in NEW[3:]:
            for b in range(bg.nbg):
                be.rt_counts_to_flux(c[k][b:b+1], float((scale / F(bg.dz[b])) / F(sc.ncol)), flux[k][b:b+1])
        cb = backward_bg(be, sc, d, dbg, cam, g, 0, ppp*12, phase=phase, aer=True)
        be.rt_counts_to_flux(cb["counts"], float(F(sc.inc_dir[g]) / (F(sc.mu0)*F(ppp))), radiance)
    r = solve_fw_bg(be, sc, d, dbg, ppp, phase=phase, aer=True)
    for k in FW + NEW:
        assert np.array_equal(be.to_numpy(flux[k]).view(np.uint8), r[k].view(np.uint8)), k
    rb = solve_bw_bg(be, sc, d, dbg, cam, ppp, phase=phase, aer=True)
    assert np.array_equal(be.to_numpy(radiance).view(np.uint8), be.to_numpy(rb["radiance"]).reshape(-1).view(np.uint8))
    # and they are not the loops without aerosol
    plain = solve_fw_bg(be, sc, d, dbg, ppp, phase=phase, aer=False)
    assert any(not np.array_equal(plain[k], r[k]) for k in FW + NEW)


# ---- 9: the chain

def _chain(be, nx, ny, nlay, top_at_1, clouds, uniform=False):
    """a synthetic SW k-distribution, an atmosphere with CAMS-like aerosol (every column the first one when uniform), and the LUTs"""
    import dataclasses
    from rte_rrtmgp_cpp_amd import synthetic, pipeline
    kd = be.upload_kdist(synthetic.make_kdist("sw", ngpt=32, nbnd=2, npres=10, nflav=3, nminor_lower=5, nminor_upper=3))
    atm0 = synthetic.make_atmosphere(nx*ny, nlay, nbnd_lw=2, nbnd_sw=2, clouds=clouds, top_at_1=top_at_1, aerosols=True)
    if uniform:
        same = lambda a: np.ascontiguousarray(np.repeat(a[..., :1], nx*ny, axis=-1)) if isinstance(a, np.ndarray) and a.ndim >= 1 and a.shape[-1] == nx*ny else a
        changes = {f.name: same(getattr(atm0, f.name)) for f in dataclasses.fields(atm0) if isinstance(getattr(atm0, f.name), np.ndarray)}
        changes["vmr"] = {k: same(v) for k, v in atm0.vmr.items()}
        changes["aermr"] = {k: same(v) for k, v in atm0.aermr.items()}
        atm0 = dataclasses.replace(atm0, **changes)
    atm = pipeline.upload_atmosphere(be, atm0)
    lut = be.upload_lut(synthetic.make_cloud_lut(2, "sw")) if clouds else None
    alut = be.upload_lut({k: (v.astype(be.np_dtype) if isinstance(v, np.ndarray) else v) for k, v in synthetic.make_aerosol_lut(2).items()})
    return kd, atm0, atm, lut, alut


def _chain_arrays(be, kd, atm0, atm, lut, alut, nlay, ncol):
    """the chain's own arrays: the clear gas optics, the band cloud and aerosol triples, inc_dir and the albedo"""
    from rte_rrtmgp_cpp_amd import pipeline
    _, col_gas, _ = pipeline.gas_state(be, kd, atm, None, interpolate=False)
    col_dry = be.get_col_dry(atm.vmr["h2o"], atm.p_lev)
    tau, ssa = be.empty((32, nlay, ncol)), be.empty((32, nlay, ncol))
    be.gas_optics_sw_direct(kd, atm.p_lay, atm.t_lay, col_gas, col_dry, tau, ssa, None)
    cld = be.cloud_optics_2str(lut, atm.lwp, atm.iwp, atm.rel, atm.dei) if lut is not None else None
    aer = tuple(be.aerosol_optics(alut, [atm.aermr["aermr%02d" % i] for i in range(1, 12)], atm.rh, atm.p_lev))
    inc_dir = (be.to_numpy(kd.solar_source) * atm0.tsi_scaling[0]) * atm0.mu0[0]
    return tau, ssa, cld, aer, inc_dir, be.asarray(atm0.sfc_alb_dif[:, 0].copy())


@pytest.mark.parametrize("n_domain", [None, 4])
@pytest.mark.parametrize("top_at_1", [False, True])
def test_the_chain_with_an_aerosol_lut_is_the_entry_on_the_chain_s_own_arrays(top_at_1, n_domain, hip_f64):
    from rte_rrtmgp_cpp_amd import pipeline, camera as C
    be = hip_f64
    nx, ny, nlay, ppp = 4, 3, 12, 8
    nd = nlay if n_domain is None else n_domain
    kd, atm0, atm, lut, alut = _chain(be, nx, ny, nlay, top_at_1, True)
    dz = 500.0
    z_up = np.concatenate([np.arange(nd + 1)*dz, nd*dz + np.cumsum(np.linspace(700., 9000., nlay - nd))])
    z_lev = z_up[::-1].copy() if top_at_1 else z_up
    split = {} if n_domain is None else dict(n_domain=nd, z_lev=z_lev)
    r = pipeline.raytrace_sw(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, ppp, S.SEED, cloud_lut=lut, kn_grid=(2, 1, 2), aerosol_lut=alut, **split)
    plain = pipeline.raytrace_sw(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, ppp, S.SEED, cloud_lut=lut, kn_grid=(2, 1, 2), **split)
    assert r["n_capped"] == 0
    cam = C.perspective(4, 3, (800., 700., 1.5e3), yaw=0.4, pitch=-1.0, fov=math.radians(50.))
    rb = pipeline.render_sw(be, kd, atm, nx, ny, 400.0, 400.0, dz, 1.1, cam, ppp, S.SEED, cloud_lut=lut, kn_grid=(2, 1, 2), aerosol_lut=alut, **split)
    assert rb["n_capped"] == 0 and rb["n_clamped"] == 0

    tau, ssa, cld, aer, inc_dir, alb = _chain_arrays(be, kd, atm0, atm, lut, alut, nlay, nx*ny)
    grid = slice(nlay - nd, nlay) if top_at_1 else slice(0, nd)
    above = list(range(nlay - nd - 1, -1, -1)) if top_at_1 else list(range(nd, nlay))
    part = lambda t: t[:, grid, :].contiguous()
    dbg = None
    if n_domain is not None:
        class Bg:
            pass
        dbg = Bg()
        dbg.dz = np.diff(z_up)[nd:].copy()
        dbg.tau, dbg.ssa = tau[:, above, 0].contiguous(), ssa[:, above, 0].contiguous()
        dbg.cloud = tuple(c[:, above, 0].contiguous() for c in cld)
        dbg.aerosol = tuple(c[:, above, 0].contiguous() for c in aer)
    cloud, aerosol = tuple(part(c) for c in cld), tuple(part(c) for c in aer)
    assert float(aerosol[0].max()) > 0
    want = be.raytracer_sw_bg(part(tau), part(ssa), nx, ny, 400.0, 400.0, dz, alb, float(atm0.mu0[0]), 1.1, inc_dir, np.zeros_like(inc_dir),
                              (2, 1, 2), ppp, S.SEED, top_at_1=top_at_1, cloud=cloud, band_lims=kd.band_lims_gpt, background=dbg, aerosol=aerosol)
    keys = FW + (NEW if n_domain is not None else ())
    assert set(r) == set(keys) | {"n_capped"}
    for k in keys:
        assert np.array_equal(be.to_numpy(r[k]).view(np.uint8), be.to_numpy(want[k]).view(np.uint8)), k
    assert any(not np.array_equal(be.to_numpy(r[k]), be.to_numpy(plain[k])) for k in keys)
    wb = be.raytracer_bw_bg(part(tau), part(ssa), nx, ny, 400.0, 400.0, dz, alb, float(atm0.mu0[0]), 1.1, inc_dir, (2, 1, 2), cam, ppp, S.SEED,
                            top_at_1=top_at_1, cloud=cloud, band_lims=kd.band_lims_gpt, background=dbg, aerosol=aerosol)
    assert np.array_equal(be.to_numpy(rb["radiance"]).view(np.uint8), be.to_numpy(wb["radiance"]).view(np.uint8))
    assert float(rb["radiance"].min()) > 0


def test_the_chain_s_direct_beam_under_haze_is_beer(hip_f64):
    """A horizontally uniform clear atmosphere under independent_column: the domain-mean sfc_dn_dir is
    sum_g inc_dir[g] exp(-(tau + tau_a)[g]/mu0) from the chain's arrays, within five sigma (a per-photon contribution in [0, 1] with
    mean p_g: sigma^2 = sum_g inc_dir[g]^2 p_g (1 - p_g)/N); without aerosol_lut the mean differs by more than that bound."""
    from rte_rrtmgp_cpp_amd import pipeline
    be = hip_f64
    nx, ny, nlay, ppp = 4, 3, 10, 1024          # (nlay is not ncol: an (nlay,) aerosol profile is told from an (ncol,) field)
    kd, atm0, atm, _, alut = _chain(be, nx, ny, nlay, False, False, uniform=True)
    args = (be, kd, atm, nx, ny, 400.0, 400.0, 500.0, 1.1, ppp, S.SEED)
    hazy = pipeline.raytrace_sw(*args, kn_grid=(2, 1, 2), independent_column=True, aerosol_lut=alut)
    clear = pipeline.raytrace_sw(*args, kn_grid=(2, 1, 2), independent_column=True)
    assert hazy["n_capped"] == 0 and clear["n_capped"] == 0
    tau, _, _, aer, inc_dir, _ = _chain_arrays(be, kd, atm0, atm, None, alut, nlay, nx*ny)
    band = R.band_of_gpt(be.to_numpy(kd.band_lims_gpt), 32)
    t_gas = be.to_numpy(tau).astype(np.float64)[:, :, 0].sum(axis=1)
    t_aer = be.to_numpy(aer[0]).astype(np.float64)[:, :, 0].sum(axis=1)[band]
    mu0, n = float(atm0.mu0[0]), ppp*nx*ny
    p = np.exp(-(t_gas + t_aer)/mu0)
    want, bound = float(np.sum(inc_dir*p)), 5*math.sqrt(float(np.sum(inc_dir**2 * p*(1 - p)/n)))
    got, without = float(be.to_numpy(hazy["sfc_dn_dir"]).mean()), float(be.to_numpy(clear["sfc_dn_dir"]).mean())
    print(f"raytracer_aer chain beer: sfc_dn_dir {got:.3f} against {want:.3f} W m-2 (bound {bound:.3f}); without aerosol_lut {without:.3f}; "
          f"aerosol optical depth {float(t_aer.min()):.3f} .. {float(t_aer.max()):.3f}")
    assert abs(got - want) <= bound
    assert abs(without - got) > bound


# ---- 10: the C++ classes

@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_cxx_classes_with_aerosol_give_the_entries_bit_for_bit_and_throw(dt, top_at_1, hip_f64, hip_f32):
    """Raytracer_gpu / Raytracer_bw_gpu after set_background and set_aerosol (through rrx_cxx_trace_rays_aer / rrx_cxx_trace_rays_bw_aer)
    against rrx_raytracer_sw_aer / rrx_raytracer_bw_aer; a refused combination comes back as an exception's message."""
    import ctypes
    import os
    import torch
    be = _be(dt, hip_f64, hip_f32)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so" if dt == "f64" else "librte_rrtmgp_hip_sp.so"))
    lib.rrx_cxx_driver_error.restype = ctypes.c_char_p
    F = ctypes.c_double if dt == "f64" else ctypes.c_float
    sc, bg = SA.general(be.np_dtype, top_at_1)
    d, dbg = dev(be, sc, bg)
    ppp = 16
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
    with_bg = (bg.nbg, H(dbg.dz), P(dbg.tau), P(dbg.ssa), *(P(c) for c in dbg.cloud))
    no_bg = (0, none, none, none, none, none, none)
    grid, aloft = tuple(P(c) for c in d["aer"]), tuple(P(c) for c in dbg.aerosol)

    def call(medium, aer, bg_aer):
        return lib.rrx_cxx_trace_rays_aer(sc.nx, sc.ny, sc.nz, 2, 2, F(sc.dx), F(sc.dy), F(sc.dz), int(sc.top_at_1), int(sc.independent_column),
                                          P(d["tau"]), P(d["ssa"]), P(d["lims"]), *(P(c) for c in d["cloud"]), P(d["alb"]), F(sc.mu0), F(sc.azimuth),
                                          H(inc_dir), H(inc_dif), *sc.kn_grid, ctypes.c_longlong(ppp), ctypes.c_ulonglong(sc.seed), be.RT_MAX_EVENTS,
                                          out6, ctypes.byref(n_capped), out5, *table, *medium, *aer, *bg_aer, stream)

    want = solve_fw_bg(be, sc, d, dbg, ppp, aer=True)
    assert call(with_bg, grid, aloft) == 0, lib.rrx_cxx_driver_error().decode()
    torch.cuda.synchronize()
    assert n_capped.value == 0 and want["n_capped"] == 0
    for k, t in zip(FW + NEW, outs + news):
        assert np.array_equal(be.to_numpy(t).view(np.uint8), want[k].view(np.uint8)), k
    # the grid's aerosol alone, without a background
    want = solve_fw_bg(be, sc, d, None, ppp, aer=True)
    assert call(no_bg, grid, (none, none, none)) == 0, lib.rrx_cxx_driver_error().decode()
    torch.cuda.synchronize()
    for k, t in zip(FW, outs):
        assert np.array_equal(be.to_numpy(t).view(np.uint8), want[k].view(np.uint8)), k
    for medium, aer, bg_aer, word in ((no_bg, grid, aloft, "needs a background"), (with_bg, (grid[0], none, grid[2]), aloft, "all empty or all"),
                                      (with_bg, grid, (aloft[0], aloft[1], none), "all empty or all")):
        assert call(medium, aer, bg_aer) != 0
        msg = lib.rrx_cxx_driver_error().decode()
        assert "Raytracer_gpu::set_aerosol" in msg and word in msg, msg

    cam = SB.cameras(sc, bg)["aloft"]
    wantb = solve_bw_bg(be, sc, d, dbg, cam, ppp, aer=True)
    out = be.empty((cam.npy, cam.npx))
    nums = np.concatenate([np.asarray(v, dtype=np.float64) for v in (cam.position, cam.e_w, cam.e_h, cam.e_d)]).astype(be.np_dtype)

    def callb(medium, aer, bg_aer):
        return lib.rrx_cxx_trace_rays_bw_aer(sc.nx, sc.ny, sc.nz, 2, 2, F(sc.dx), F(sc.dy), F(sc.dz), int(sc.top_at_1),
                                             P(d["tau"]), P(d["ssa"]), P(d["lims"]), *(P(c) for c in d["cloud"]), P(d["alb"]), F(sc.mu0),
                                             F(sc.azimuth), H(inc_dir), *sc.kn_grid, cam.type, cam.npx, cam.npy, F(cam.fov), H(nums),
                                             ctypes.c_longlong(ppp), ctypes.c_ulonglong(sc.seed), be.RT_MAX_EVENTS, P(out), ctypes.byref(n_capped),
                                             ctypes.byref(n_clamped), *table, *medium, *aer, *bg_aer, stream)

    assert callb(with_bg, grid, aloft) == 0, lib.rrx_cxx_driver_error().decode()
    torch.cuda.synchronize()
    assert n_capped.value == 0 and n_clamped.value == 0 and wantb["n_capped"] == 0
    assert np.array_equal(be.to_numpy(out).view(np.uint8), be.to_numpy(wantb["radiance"]).view(np.uint8))
    assert callb(no_bg, grid, aloft) != 0
    msg = lib.rrx_cxx_driver_error().decode()
    assert "Raytracer_bw_gpu::set_aerosol" in msg and "needs a background" in msg, msg
