"""CPU tests of the phase-table restatement (tests/raytracer_phase_ref.py) and of the package's table helpers
(rte_rrtmgp_cpp_amd/phase_tables.py): what the builder makes of a Henyey-Greenstein table, the round trip of the sampler against
the longdouble inverse, from_angles and the reader of the reference's Mie file layout on a file written here."""
import numpy as np
import pytest

import raytracer_phase_ref as P
import raytracer_phase_scenes as PS
from rte_rrtmgp_cpp_amd import phase_tables, rrxio


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_builder_normalises_hg_and_reproduces_its_analytic_cdf(dtype):
    mu, raw = PS.hg1800(0.85)
    t = P.build_tables(mu, raw, dtype)
    eps = np.finfo(dtype).eps
    m = t.mu.astype(np.float64)
    for b in range(PS.NBND):
        for i in range(3):
            p, c = t.phase[b, i].astype(np.float64), t.cdf[b, i].astype(np.float64)
            # the stored table integrates to one by the trapezoid rule: its numbers are rounded to dtype, relative eps/2 each (eps/2
            # of the integral at the most), and the builder's total is a sequential sum of 1 799 terms in double
            assert abs(0.5*np.sum(0.5*(p[1:] + p[:-1])*np.diff(m)) - 1.0) <= eps + 1800*np.finfo(np.float64).eps
            assert c[0] == 0.0 and c[-1] == 1.0 and np.all(np.diff(c) >= 0)
            # the trapezoid rule against the analytic CDF C of HG on these nodes. The rule's own error up to node i is at most
            # rule_i = 1/2 sum h^3/12 max|P''| (P'' of HG from the closed form; it grows with mu, so the maximum of an interval is
            # at its right node). The builder divides by the rule's total 1 + e_n: cdf_i - C_i = (e_i - C_i e_n)/(1 + e_n), so
            # |cdf_i - C_i| <= (rule_i + C_i rule_n)/(1 - rule_n); 64 eps for the rounding of the nodes, the table and the sums
            g = 0.85
            p2 = 15.0*g*g*(1 - g*g) / (1 + g*g - 2*g*m)**3.5
            rule = 0.5*np.cumsum(np.diff(m)**3/12.0*p2[1:])
            exact = P.hg_cdf(m[1:], g)
            err = np.abs(c[1:] - exact)
            bound = (rule + exact*rule[-1])/(1.0 - rule[-1]) + 64*eps
            assert np.all(err <= bound), float(np.max(err/bound))
    # the normalisation of the raw table does not matter: the three radii hold the same table to rounding
    # (raw differs by one rounding to dtype per node, the sums by at most 1 800 roundings in double, the result by one to dtype)
    tol = 2*eps + 1800*np.finfo(np.float64).eps
    assert np.allclose(t.phase[0, 0], t.phase[0, 2], rtol=tol, atol=0)
    assert np.allclose(t.cdf[0, 0], t.cdf[0, 2], rtol=0, atol=tol)


def test_builder_on_the_isotropic_tables_is_exact():
    for nodes in (2, 5):
        for dtype in (np.float64, np.float32):
            mu, raw = PS.isotropic(nodes, 3)
            t = P.build_tables(mu, raw, dtype)
            assert np.all(t.phase == 1.0)
            assert np.array_equal(t.cdf[0, 0], (t.mu.astype(np.float64) + 1.0)/2.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_table_with_a_zero_interval(dtype):
    """P = 0 on [-1/2, 0] and at the node +1/2: a flat piece of the CDF, zero denominators at its ends; the sampler never returns a
    cosine inside the empty interval and stays monotone"""
    mu = np.array([-1., -0.5, 0., 0.5, 1.])
    raw = np.array([[[2., 0., 0., 0., 4.]]])
    t = P.build_tables(mu, raw, dtype)
    assert np.array_equal(t.cdf[0, 0], np.array([0., 1./3., 1./3., 1./3., 1.], dtype=np.float64).astype(dtype))
    F = np.dtype(dtype).type
    third = t.cdf[0, 0, 1]
    u = np.sort(np.concatenate([np.linspace(0.0005, 0.9995, 2000).astype(dtype), [np.nextafter(third, F(0.)), third, np.nextafter(third, F(1.))]]))
    cos, iv = P.sample(t, 0, np.zeros_like(u), u, with_interval=True)
    assert np.all(np.isfinite(cos)) and np.all(np.diff(cos) >= 0)
    assert not np.any((cos > -0.5) & (cos < 0.5))
    assert np.all(cos[u < third] <= -0.5) and np.all(cos[u >= third] >= 0.5) and cos[u == third][0] == 0.5
    assert np.all(P.evaluate(t, 0, np.zeros(3, dtype=dtype), np.array([-0.25, 0., 0.5], dtype=dtype)) == 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("which", ["double_hg33", "hg1800"])
def test_round_trip_against_longdouble(which, dtype):
    """C(sample(u)) = u with C evaluated in longdouble on the stored table. One rounding of u - C_i (|u - C_i| <= 1) and of the
    blend of C_i, each eps/2, carried through the inverse, and the rounding of the result to dtype, eps/2 |cos| <= eps/2 times the
    density P <= P_max there: |C(cos) - u| <= (2 + P_max) eps, P_max the table's largest value; 4 more eps for the remaining
    operations of the inverse (s, the square root, the division), which act on t = cos - mu_i only."""
    mu, raw = getattr(PS, which)()
    t = P.build_tables(mu, raw, dtype, PS.RE0, PS.DRE)
    eps = float(np.finfo(dtype).eps)
    for b in range(PS.NBND):
        u, re = PS.probe_pairs(t, b, dtype)
        cos, iv = P.sample(t, b, re, u, with_interval=True)
        assert np.all(cos >= t.mu[iv]) and np.all(cos <= t.mu[iv+1])
        back = P.cdf_ld(t, b, re, cos)
        p_max = float(t.phase[b].max())
        err = np.abs(back - u.astype(P.LD)).astype(np.float64)
        print(f"phase round trip {which} {np.dtype(dtype).name} band {b}: max |C(sample(u)) - u| = {err.max():.3e} "
              f"= {err.max()/eps:.2f} eps (bound {(6 + p_max):.1f} eps, P_max = {p_max:.1f})")
        assert np.all(err <= (6 + p_max)*eps)
        # per radius the sampler is monotone in u
        for r in range(PS.probe_re(dtype).size):
            n = u.size // PS.probe_re(dtype).size
            assert np.all(np.diff(cos[r*n:(r+1)*n]) >= 0)


def test_index_clamps_and_maps_nan_to_the_first_table():
    t = P.build_tables(*PS.double_hg33(), np.float32, PS.RE0, PS.DRE)
    ire, jre, f = P.index(t, PS.probe_re(np.float32))
    assert ire.tolist() == [0, 1, 1, 0, 1, 0, 1, 1, 0] and np.array_equal(jre, ire + 1)
    assert f.tolist()[:5] == [0., 0., 1., 0., 1.] and f[-1] == 0 and f[5] == np.float32(0.25) and f[6] == np.float32(0.5)


def test_equal_tables_blend_to_themselves_and_evaluation_is_the_sampled_density():
    mu, raw = PS.double_hg33()
    raw[:, 1] = raw[:, 0]; raw[:, 2] = raw[:, 0]
    t3 = P.build_tables(mu, raw, np.float64, PS.RE0, PS.DRE)
    t1 = P.build_tables(mu, raw[:, :1], np.float64, PS.RE0, PS.DRE)
    u, re = PS.probe_pairs(t3, 1, np.float64)
    assert np.array_equal(P.sample(t3, 1, re, u), P.sample(t1, 1, re, u))
    cs = np.linspace(-1, 1, re.size)
    assert np.array_equal(P.evaluate(t3, 1, re, cs), P.evaluate(t1, 1, re, cs))
    # dC/dmu = P/2: a centred difference of the longdouble CDF inside an interval against the evaluator
    t = P.build_tables(*PS.double_hg33(), np.float64, PS.RE0, PS.DRE)
    mid = 0.5*(t.mu[1:] + t.mu[:-1]); h = 0.25*np.diff(t.mu)
    rr = np.full(mid.size, 8.5)
    slope = (P.cdf_ld(t, 0, rr, mid + h) - P.cdf_ld(t, 0, rr, mid - h)) / (2*h.astype(P.LD))
    assert np.allclose(np.asarray(2*slope, dtype=np.float64), P.evaluate(t, 0, rr, mid), rtol=1e-12, atol=0)


def test_forward_restatement_with_an_isotropic_table_is_the_hg_restatement_with_g_zero():
    import raytracer_ref as R
    sc = PS.general_g(np.float64, 0.0)
    t = P.build_tables(*PS.isotropic(5, 3), np.float64, PS.RE0, PS.DRE)
    t.cld_re = PS.cell_radii_with_nan(sc, np.float64)
    a, b = R.trace_counts(sc, 1, 3, 400), R.trace_counts(sc, 1, 3, 400, table=t)
    for k in R.COUNT_NAMES + ("n_capped", "events"):
        assert np.array_equal(a[k], b[k]), k
    assert a["abs_dif"].any()


def test_backward_restatement_with_an_isotropic_table_is_the_hg_restatement_with_g_zero():
    import raytracer_bw_ref as B
    sc = PS.general_g(np.float64, 0.0)
    t = P.build_tables(*PS.isotropic(2, 1), np.float64, PS.RE0, PS.DRE)
    t.cld_re = PS.cell_radii_with_nan(sc, np.float64)
    sensor = B.flux_sensor(sc.nx, sc.ny, True)
    a, b = B.trace_counts_bw(sc, sensor, 0, 0, 320), B.trace_counts_bw(sc, sensor, 0, 0, 320, table=t)
    for k in ("counts", "n_dep", "n_capped", "n_clamped", "events", "walk_cells"):
        assert np.array_equal(a[k], b[k]), k
    assert a["counts"].any()


def test_helpers_of_the_package_are_those_of_the_restatement():
    mu = phase_tables.nodes(33, 2.5)
    assert np.array_equal(mu, P.nodes(33, 2.5)) and mu[0] == -1 and mu[-1] == 1 and np.all(np.diff(mu) > 0)
    assert np.array_equal(phase_tables.henyey_greenstein(mu, 0.7), P.hg(mu, 0.7))
    assert np.array_equal(phase_tables.double_hg(mu, 0.8, -0.4, 0.9), P.double_hg(mu, 0.8, -0.4, 0.9))


def test_from_angles_reverses_an_ascending_angle_table():
    angle = np.array([0., 0.5, 2., 10., 60., 90., 150., 180.])
    phase = np.arange(2*3*8, dtype=np.float64).reshape(2, 3, 8)
    mu, raw = phase_tables.from_angles(angle, phase)
    assert mu[0] == -1 and mu[-1] == 1 and np.all(np.diff(mu) > 0)
    assert np.allclose(mu, np.cos(np.deg2rad(angle))[::-1], rtol=0, atol=1e-16)
    assert np.array_equal(raw, phase[..., ::-1]) and raw.flags.c_contiguous
    mu_r, _ = phase_tables.from_angles(np.deg2rad(angle), phase, degrees=False)
    assert np.allclose(mu_r, mu, rtol=0, atol=1e-15)
    for bad in (angle[::-1], angle[1:], angle[:-1], np.r_[angle[:3], angle[2:]]):
        with pytest.raises(ValueError, match="from_angles"):
            phase_tables.from_angles(bad, phase[..., :bad.size])


def test_reader_of_the_reference_mie_layout(tmp_path):
    angle = np.array([0., 1., 5., 30., 90., 180.])
    phase = np.random.default_rng(3).uniform(0.1, 9., (2, 4, 6))
    path = str(tmp_path / "mie.rrxb")
    rrxio.write(path, {"band": 2, "r_eff": 4, "n_ang": 6}, {"phase": (phase, ["band", "r_eff", "n_ang"]), "phase_angle": (angle, ["n_ang"])})
    mu, raw, re0, dre = phase_tables.read_mie(path)
    assert (re0, dre) == (2.5, 1.0) and raw.shape == (2, 4, 6)
    assert np.array_equal(raw, phase[..., ::-1]) and mu[0] == -1 and mu[-1] == 1
    t = P.build_tables(mu, raw, np.float64, re0, dre)
    assert np.all(t.cdf[..., -1] == 1) and np.all(np.diff(t.cdf, axis=-1) > 0)
    rrxio.write(path, {"band": 2, "r_eff": 4, "n_ang": 6}, {"phase": (phase, ["band", "r_eff", "n_ang"])})
    with pytest.raises(ValueError, match="phase_angle"):
        phase_tables.read_mie(path)
    rrxio.write(path, {"band": 2, "r_eff": 4, "n_ang": 6}, {"phase": (phase.transpose(1, 0, 2), ["r_eff", "band", "n_ang"]), "phase_angle": (angle, ["n_ang"])})
    with pytest.raises(ValueError, match="band, r_eff, n_ang"):
        phase_tables.read_mie(path)
