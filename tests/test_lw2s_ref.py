"""Hand-written cases for tests/lw2s_ref.py, the numpy reference of the LW two-stream solver with scattering (no GPU)."""
import math

import numpy as np
import pytest

import lw2s_ref as R


def arr(x, dtype=np.float64):
    """a scalar or list as a (ngpt, n, ncol) = (1, n, 1) array"""
    return np.asarray(x, dtype=dtype).reshape(1, -1, 1)


def test_one_layer_by_hand():
    """One layer, every intermediate worked out with math.* from the formulas of DESIGN 4.10"""
    tau, ssa, g, top, bot, emis, ssrc, inc = 0.7, 0.6, 0.4, 10.0, 14.0, 0.9, 15.0, 2.0
    g1 = 1.66 * (1 - 0.5 * ssa * (1 + g)); g2 = 1.66 * 0.5 * ssa * (1 - g)
    k = math.sqrt((g1 - g2) * (g1 + g2))
    e1 = math.exp(-tau * k); e2 = e1 * e1
    rt = 1 / (k * (1 + e2) + g1 * (1 - e2))
    r = rt * g2 * (1 - e2); t = rt * 2 * k * e1
    z = (bot - top) / (tau * (g1 + g2))
    su = math.pi * ((z + top) - r * (-z + top) - t * (z + bot))
    sd = math.pi * ((-z + bot) - r * (z + bot) - t * (-z + top))
    a_sfc = 1 - emis; s_sfc = math.pi * emis * ssrc
    den = 1 / (1 - r * a_sfc)
    src0 = su + t * den * (s_sfc + a_sfc * sd)
    alb0 = r + t * t * a_sfc * den
    up0 = inc * alb0 + src0
    dn1 = (t * inc + r * s_sfc + sd) * den
    up1 = dn1 * a_sfc + s_sfc

    rd, td, gs = R.two_stream(arr(tau), arr(ssa), arr(g))
    assert rd.item() == pytest.approx(r, rel=1e-14) and td.item() == pytest.approx(t, rel=1e-14)
    s_up, s_dn = R.sources(arr(tau), gs, rd, td, arr(top), arr(bot))
    assert s_up.item() == pytest.approx(su, rel=1e-13) and s_dn.item() == pytest.approx(sd, rel=1e-13)
    for top_at_1 in (True, False):
        lev = arr([top, bot] if top_at_1 else [bot, top])
        up, dn = R.solve(arr(tau), arr(ssa), arr(g), lev, np.full((1, 1), emis), np.full((1, 1), ssrc), np.full((1, 1), inc), top_at_1)
        i0, i1 = (0, 1) if top_at_1 else (1, 0)
        assert up[0, i0, 0] == pytest.approx(up0, rel=1e-13) and dn[0, i0, 0] == inc
        assert up[0, i1, 0] == pytest.approx(up1, rel=1e-13) and dn[0, i1, 0] == pytest.approx(dn1, rel=1e-13)
    # energy: what goes in (inc + both sources' share) is consistent with a reflecting / transmitting slab, 0 <= r, t and r + t <= 1
    assert 0 < r < 1 and 0 < t < 1 and r + t < 1


def test_thin_layer_switch():
    """tau = 1e-8 has no sources, the next double above it has the full expression"""
    rd, td, gs = R.two_stream(arr([1e-8, np.nextafter(1e-8, 1)]), arr([0.5, 0.5]), arr([0.2, 0.2]))
    s_up, s_dn = R.sources(arr([1e-8, np.nextafter(1e-8, 1)]), gs, rd, td, arr([10., 10.]), arr([12., 12.]))
    assert s_up[0, 0, 0] == 0 and s_dn[0, 0, 0] == 0
    assert s_up[0, 1, 0] != 0 and s_dn[0, 1, 0] != 0
    # the layer emits about pi * D * (1 - ssa) * tau * B on either side: a loose physical bracket, the cancellation leaves few digits
    assert abs(s_up[0, 1, 0]) < 1e-5 and abs(s_dn[0, 1, 0]) < 1e-5


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_no_scattering_limit(dtype):
    tau = arr([0., 1e-3, 0.3, 5., 40.], dtype)
    rd, td, _ = R.two_stream(tau, np.zeros_like(tau), np.zeros_like(tau))
    assert rd.dtype == dtype and np.all(rd == 0)
    # Tdif = RT 2 k e1 with RT = 1/(2 k) to a few roundings; the rounded argument tau*k of the exponential adds |tau k| eps
    want = np.exp(-1.66 * tau.astype(np.float64))
    assert np.all(np.abs(td - want) <= np.finfo(dtype).eps * (4 + 2 * 1.66 * tau) * want)


@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("with_cloud", [True, False])
def test_isothermal_closure(top_at_1, with_cloud):
    """B_lev, sfc_src and inc_flux/pi equal per g-point: flux_up = flux_dn = pi * sum of the sources at every level"""
    rng = np.random.default_rng(3)
    ngpt, nlay, ncol = 6, 17, 5
    gb = np.array([1, 1, 2, 2, 2, 3], dtype=np.int32)
    tau = 10.0**rng.uniform(-4, 1.5, (ngpt, nlay, ncol)); tau[0, 3] = 0; tau[1, 5] = 1e-9
    cld = (rng.uniform(0, 4, (3, nlay, ncol)), rng.uniform(0, 0.999999, (3, nlay, ncol)), rng.uniform(-0.3, 0.9, (3, nlay, ncol))) if with_cloud else None
    b = rng.uniform(5, 40, ngpt)
    pfrac = np.ones((ngpt, nlay, ncol)); blev = np.empty((3, nlay + 1, ncol))
    # one source value per g-point needs pfrac to carry it: B_lev = 1, pfrac = b
    pfrac *= b[:, None, None]; blev[:] = 1.0
    emis = rng.uniform(0.5, 1.0, (ngpt, ncol)); ssrc = np.repeat(b[:, None], ncol, 1)
    up, dn = R.solve_fractions(tau, pfrac, blev, gb, cld, emis, ssrc, np.pi * ssrc, top_at_1)
    want = np.pi * b.sum()
    np.testing.assert_allclose(up, want, rtol=1e-9); np.testing.assert_allclose(dn, want, rtol=1e-9)


def test_combine_is_the_increment_arithmetic():
    tau = arr([0.5, 0.0, 2.0]); gb = np.array([1], dtype=np.int32)
    cld = (arr([1.5, 0.0, 0.0]).reshape(1, 3, 1), arr([0.8, 0.5, 0.5]).reshape(1, 3, 1), arr([0.7, 0.3, 0.3]).reshape(1, 3, 1))
    t, w, g = R.combine(tau, cld, gb)
    assert t[0, :, 0].tolist() == [2.0, 0.0, 2.0]
    assert w[0, 0, 0] == pytest.approx(1.5 * 0.8 / 2.0) and w[0, 1, 0] == 0 and w[0, 2, 0] == 0
    assert g[0, 0, 0] == pytest.approx(0.7) and g[0, 1, 0] == 0 and g[0, 2, 0] == 0


def test_sources_as_written_cancel_and_the_regrouped_form_does_not():
    """The stated source formulas in float64 against the same formulas in extended precision, at tau = 1e-4 with level sources that
    differ by their own size: the as-written form is off by about 1e-8 of a thin layer's source (the per-g-point bound of the GPU tests is the
    reference's error), the regrouped form the kernels use by a few eps"""
    L = np.longdouble
    if np.finfo(L).eps > 1e-18:
        pytest.skip("no extended precision on this platform")
    rng = np.random.default_rng(0)
    n = 4000
    tau = np.full(n, 1e-4) * rng.uniform(1., 2., n); ssa = rng.uniform(0., 0.9, n); g = rng.uniform(-0.3, 0.9, n)
    top = rng.uniform(5., 40., n); bot = rng.uniform(5., 40., n)

    def written(tau, ssa, g, top, bot):
        r, t, gs = R.two_stream(tau, ssa, g)
        return R.sources(tau, gs, r, t, top, bot)

    def regrouped(tau, ssa, g, top, bot):
        g1 = R.D * (1 - 0.5 * ssa * (1 + g)); g2 = R.D * 0.5 * ssa * (1 - g)
        k = np.sqrt(np.maximum((g1 - g2) * (g1 + g2), R.K2_MIN)); x = tau * k
        e1 = np.exp(-x); u = -np.expm1(-x); m = u * (1 + e1); kp = k * (1 + e1 * e1)
        rt = 1 / (kp + g1 * m); rdif = rt * g2 * m; omt = rt * (k * u * u + g1 * m)
        itg = 1 / (tau * (g1 + g2))
        c = rt * ((k * u * u * itg - g1 * m) + (m * (g1 + g2) * itg - kp))
        dc = (bot - top) * c
        return np.pi * (dc + (bot * omt - rdif * top)), np.pi * ((top * omt - rdif * bot) - dc)

    exact = written(*(a.astype(L) for a in (tau, ssa, g, top, bot)))
    scale = np.pi * R.D * tau * np.maximum(top, bot)          # the size of a thin layer's source (a source itself may pass through 0)
    rel = lambda got: max(float(np.max(np.abs(got[i].astype(L) - exact[i]) / scale)) for i in range(2))
    e_written, e_regrouped = rel(written(tau, ssa, g, top, bot)), rel(regrouped(tau, ssa, g, top, bot))
    print(f"sources at tau = 1e-4: as written {e_written:.2e}, regrouped {e_regrouped:.2e}")
    # as written: eps Z / (D tau B) = eps / (D (gamma1 + gamma2) tau^2), about 1e-9 ... 1e-8 here; regrouped: a few eps / (D tau), 1e-11
    assert 1e-9 < e_written < 1e-6
    assert e_regrouped < 1e-10 and e_regrouped < e_written / 100
