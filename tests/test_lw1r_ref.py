"""Checks of tests/lw1r_ref.py, the numpy reference of the rescaled LW no-scattering solver (no GPU)."""
import math

import numpy as np
import pytest

import lw1r_ref as R
import lw2s_ref


def arr(x, dtype=np.float64):
    """a scalar or list as a (ngpt, n, ncol) = (1, n, 1) array"""
    return np.asarray(x, dtype=dtype).reshape(1, -1, 1)


def random_problem(rng, ngpt, nlay, ncol, nmus=1):
    tau = 10.0**rng.uniform(-9, 1.5, (ngpt, nlay, ncol))
    ssa = rng.uniform(0, 0.99, (ngpt, nlay, ncol)); g = rng.uniform(-0.3, 0.9, (ngpt, nlay, ncol))
    lay = rng.uniform(5, 40, (ngpt, nlay, ncol)); lev = rng.uniform(5, 40, (ngpt, nlay + 1, ncol))
    emis = rng.uniform(0.5, 1.0, (ngpt, ncol)); ssrc = rng.uniform(5, 40, (ngpt, ncol)); inc = rng.uniform(0, 30, (ngpt, ncol))
    sec = rng.uniform(1.2, 2.2, (nmus, ngpt, ncol)); w = rng.uniform(0.2, 0.6, nmus)
    return sec, w, tau, ssa, g, lay, lev, emis, ssrc, inc


@pytest.mark.parametrize("top_at_1", [True, False])
def test_ssa_zero_is_the_no_scattering_solve(top_at_1, oracle_f64):
    """(a) ssa = 0 against the CPU oracle's rte_lw_solver_noscat, per g-point: the same arithmetic, 1e-13 relative"""
    rng = np.random.default_rng(41)
    sec, w, tau, ssa, g, lay, lev, emis, ssrc, inc = random_problem(rng, 8, 12, 7)
    want = oracle_f64.lw_solver_noscat(top_at_1, sec, w, tau, lay, lev, emis, ssrc, inc_flux=inc)
    up, dn = R.solve(sec, w, tau, np.zeros_like(tau), g, lay, lev, emis, ssrc, inc, top_at_1)
    e_up = np.max(np.abs(up - want["flux_up"]) / np.abs(want["flux_up"]))
    e_dn = np.max(np.abs(dn - want["flux_dn"]) / np.abs(want["flux_dn"]))
    print(f"ssa = 0 against the oracle: up {e_up:.2e}, dn {e_dn:.2e}")
    assert e_up <= 1e-13 and e_dn <= 1e-13


def test_flipped_inputs_give_flipped_outputs_bit_for_bit():
    """(b) both orientations give the same numbers on flipped arrays"""
    rng = np.random.default_rng(42)
    sec, w, tau, ssa, g, lay, lev, emis, ssrc, inc = random_problem(rng, 4, 15, 5, nmus=2)
    jac = rng.uniform(0.1, 0.5, emis.shape)
    a = R.solve(sec, w, tau, ssa, g, lay, lev, emis, ssrc, inc, True, sfc_src_jac=jac)
    f = lambda x: np.ascontiguousarray(x[:, ::-1])
    b = R.solve(sec, w, f(tau), f(ssa), f(g), f(lay), f(lev), emis, ssrc, inc, False, sfc_src_jac=jac)
    for x, y in zip(a, b):
        assert np.array_equal(x, y[:, ::-1])


@pytest.mark.parametrize("top_at_1", [True, False])
def test_isothermal_closure(top_at_1):
    """(c) every source B and the top radiance B: every radiance is B at 1e-14 relative, for any ssa, g and emissivity -- the bracket
    of each adjustment vanishes identically"""
    rng = np.random.default_rng(43)
    ngpt, nlay, ncol = 6, 40, 5
    sec, w, tau, ssa, g, _, _, emis, _, _ = random_problem(rng, ngpt, nlay, ncol)
    w = np.array([1.0])
    b = rng.uniform(5, 40, (ngpt, 1, ncol))
    lay = np.broadcast_to(b, (ngpt, nlay, ncol)).copy(); lev = np.broadcast_to(b, (ngpt, nlay + 1, ncol)).copy()
    up, dn = R.solve(sec, w, tau, ssa, g, lay, lev, emis, b[:, 0], np.pi * b[:, 0], top_at_1)
    want = np.pi * lev
    e = max(np.max(np.abs(up - want) / want), np.max(np.abs(dn - want) / want))
    print(f"isothermal closure: {e:.2e}")
    assert e <= 1e-14


CASES = {"ice": (0.3, 0.6, 0.9), "liq": (2.0, 0.5, 0.85), "thin": (0.05, 0.7, 0.8)}


@pytest.mark.parametrize("gas_tau", [0.002, 0.05])
@pytest.mark.parametrize("cloud", sorted(CASES))
def test_rescaling_halves_the_absorption_only_error(cloud, gas_tau):
    """(d) one column of 40 layers, 200-295 K, black-body level sources, emissivity 0.98, a cloud in layers 15-21: against the
    two-stream solve with scattering (lw2s_ref.solve) the rescaled error is at most half the error of an absorption-only solve
    (tau (1 - ssa)), for both fluxes. The reference alone gives ratios of 0.09 ... 0.18."""
    nlay = 40
    tc, wc, gc = CASES[cloud]
    t_lev = np.linspace(200., 295., nlay + 1)
    b_lev = 5.670374419e-8 * t_lev**4 / np.pi
    lev = b_lev.reshape(1, nlay + 1, 1); lay = (0.5 * (b_lev[1:] + b_lev[:-1])).reshape(1, nlay, 1)
    tau = np.full((1, nlay, 1), gas_tau); ssa = np.zeros_like(tau); g = np.zeros_like(tau)
    tau[0, 15:22] += tc; ssa[0, 15:22] = tc * wc / tau[0, 15:22]; g[0, 15:22] = gc
    emis = np.full((1, 1), 0.98); ssrc = b_lev[-1].reshape(1, 1)
    sec = np.full((1, 1, 1), 1.66); w = np.array([1.0])
    ref_up, ref_dn = lw2s_ref.solve(tau, ssa, g, lev, emis, ssrc)
    err = lambda got: tuple(float(np.max(np.abs(a - b))) for a, b in zip(got, (ref_up, ref_dn)))
    e_abs = err(R.solve(sec, w, tau * (1 - ssa), ssa, g, lay, lev, emis, ssrc, rescale=False))
    e_res = err(R.solve(sec, w, tau, ssa, g, lay, lev, emis, ssrc))
    print(f"{cloud} {gas_tau}: absorption only {e_abs[0]:.2f}, {e_abs[1]:.2f}; rescaled {e_res[0]:.2f}, {e_res[1]:.2f} W m-2")
    assert e_res[0] <= 0.5 * e_abs[0] and e_res[1] <= 0.5 * e_abs[1]


def test_one_layer_by_hand():
    """(e) one layer, every intermediate worked out with math.* from the formulas of DESIGN 4.11"""
    tau, ssa, g, D, wt = 0.7, 0.6, 0.4, 1.5, 0.8
    top, mid, bot, emis, ssrc, inc, sjac = 10.0, 12.5, 14.0, 0.9, 15.0, 2.0, 0.25
    wb = ssa * (1 - g) / 2; st = 1 - ssa + wb; cn = 0.4 * wb / st
    tl = tau * D * st; tr = math.exp(-tl); an = 1 - tr * tr
    fact = (1 - tr) / tl - tr
    sdn = (1 - tr) * bot + 2 * fact * (mid - bot)
    sup = (1 - tr) * top + 2 * fact * (mid - top)
    dn0 = inc / math.pi
    dn1 = tr * dn0 + sdn
    up1 = dn1 * (1 - emis) + emis * ssrc
    up0 = tr * up1 + sup + cn * (an * dn0 - tr * sdn - sup)
    dn1 = tr * dn0 + sdn + cn * (an * up1 - tr * sup - sdn)
    s = math.pi * wt
    for top_at_1 in (True, False):
        lev = arr([top, bot] if top_at_1 else [bot, top])
        up, dn, jac = R.solve(np.full((1, 1, 1), D), np.array([wt]), arr(tau), arr(ssa), arr(g), arr(mid), lev, np.full((1, 1), emis),
                              np.full((1, 1), ssrc), np.full((1, 1), inc), top_at_1, sfc_src_jac=np.full((1, 1), sjac))
        i0, i1 = (0, 1) if top_at_1 else (1, 0)
        assert up[0, i0, 0] == pytest.approx(s * up0, rel=1e-14) and dn[0, i0, 0] == pytest.approx(s * dn0, rel=1e-14)
        assert up[0, i1, 0] == pytest.approx(s * up1, rel=1e-14) and dn[0, i1, 0] == pytest.approx(s * dn1, rel=1e-14)
        assert jac[0, i1, 0] == pytest.approx(s * emis * sjac, rel=1e-14) and jac[0, i0, 0] == pytest.approx(s * tr * emis * sjac, rel=1e-14)



def test_float32_thick_branch_just_above_the_threshold_loses_four_digits():
    """Why single g-points of the float32 reference need a wider bound than their sums (tests/test_gpu_lw_rescaled.py): the thick
    branch of the source factor, (1 - tr)/tl - tr, just above tau_thres = eps^(1/4) = 0.019 in float32. tr carries up to eps (its rounding
    and the exponential's last bit), the division by tl makes that eps/tl, and fact itself is about tl/2: a relative error of up to
    2 eps/tl^2 = 6.9e-4 of the part of the layer's source that fact multiplies."""
    thres = float(np.sqrt(np.sqrt(np.finfo(np.float32).eps)))
    tl64 = (thres * np.linspace(1.001, 2., 4000)).reshape(1, -1, 1)
    out = {}
    for dt in (np.float32, np.float64):
        tl = tl64.astype(dt)
        z = np.zeros_like(tl)
        _, sdn, sup, _ = R.layers(tl, z, z, dt(1), z + dt(30), z, z)           # level sources 0: the sources are 2 fact lay_source
        out[dt] = sup.astype(np.float64)
    rel = float(np.max(np.abs(out[np.float32] - out[np.float64]) / out[np.float64]))
    print(f"float32 source factor just above tau_thres: {rel:.2e} of its value")
    assert 2e-5 < rel < 2 * np.finfo(np.float32).eps / thres**2
