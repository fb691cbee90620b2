"""CPU tests of the allocation of photons to g-points (pipeline.spectral_allocation) and of the numpy restatement of the forward
tracer with all g-points in one launch (tests/raytracer_spectral_ref.py), on the scenes that the GPU tests reuse
(tests/raytracer_spectral_scenes.py)."""
import numpy as np
import pytest

import raytracer_ref as R
import raytracer_bw_ref as B
import raytracer_phase_ref as P
import raytracer_spectral_ref as SP
import raytracer_bw_spectral_ref as BSP
import raytracer_spectral_scenes as SS
from rte_rrtmgp_cpp_amd import pipeline, synthetic

COUNTS = R.ALL_COUNTS + ("n_capped", "events")


# ---- 1: the allocation

def test_allocation_sums_to_P_honours_the_floor_and_leaves_dark_g_points_out():
    inc = np.array(SS.INC)
    for P, floor in ((64, 1), (4, 1), (5, 1), (1000, 3), (64, 0), (12, 3)):
        m = pipeline.spectral_allocation(inc, P, floor)
        assert m.dtype == np.int64 and int(m.sum()) == P, (P, floor, m)
        assert np.all(m[inc > 0] >= floor) and m[SS.EMPTY] == 0, (P, floor, m)
    assert list(pipeline.spectral_allocation(inc, 4, 1)) == [1, 1, 0, 1, 1]
    assert not pipeline.spectral_allocation(np.zeros(3), 0).any()


def test_allocation_is_proportional_within_one_photon_where_the_floor_does_not_bind():
    rng = np.random.default_rng(7)
    for P in (64, 257, 10000):
        inc = rng.uniform(0.5, 50.0, 12)
        inc[5] = 0.0
        # without a floor nothing binds: every g-point is within one photon of P x its share
        m = pipeline.spectral_allocation(inc, P, 0)
        assert np.all(np.abs(m - P*inc/inc.sum()) < 1.0), (P, m)
    # with a floor: the g-points it binds hold exactly the floor, the others share what is left, each within one photon
    inc = np.array([1000., 1., 500., 0., 2., 250.])
    m = pipeline.spectral_allocation(inc, 100, 2)
    bound = (inc > 0) & (100*inc/inc.sum() < 2)
    assert list(np.nonzero(bound)[0]) == [1, 4] and np.all(m[bound] == 2) and m[3] == 0
    free = (inc > 0) & ~bound
    rest = 100 - int(m[bound].sum())
    assert np.all(np.abs(m[free] - rest*inc[free]/inc[free].sum()) < 1.0), m


def test_allocation_ties_go_to_the_lower_g_and_it_raises_below_the_floor():
    assert list(pipeline.spectral_allocation([1., 1., 1., 0.], 4)) == [2, 1, 1, 0]
    assert list(pipeline.spectral_allocation([1., 1., 1., 0.], 5)) == [2, 2, 1, 0]
    assert list(pipeline.spectral_allocation([0., 3., 3.], 3, 0)) == [0, 2, 1]
    assert list(pipeline.spectral_allocation([2., 2.], 5, 2)) == [3, 2]
    with pytest.raises(ValueError, match="cannot give 1 to each of 4"):
        pipeline.spectral_allocation(SS.INC, 3)
    with pytest.raises(ValueError, match="cannot give 2 to each of 4"):
        pipeline.spectral_allocation(SS.INC, 7, 2)
    with pytest.raises(ValueError):
        pipeline.spectral_allocation([0., 0.], 4)
    with pytest.raises(ValueError):
        pipeline.spectral_allocation([1., -1.], 4)


def test_photon_list_of_the_pipeline_is_the_restatement_s():
    for dt in (np.float64, np.float32):
        sc, _ = SS.general(dt)
        m = pipeline.spectral_allocation(sc.inc_dir.astype(np.float64) + sc.inc_dif, 40)
        a, b = pipeline.spectral_photon_list(sc.inc_dir, sc.inc_dif, m, sc.ncol, dt), SP.photon_list(sc, m)
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y)) and np.asarray(x).dtype == np.asarray(y).dtype
        pe, w0, df, U = a
        assert pe[0] == 0 and pe[SS.EMPTY] == pe[SS.EMPTY + 1] and w0[SS.EMPTY] == 0
        # sum_g m_g weight0_g U = S up to rounding: the weights carry the fluxes
        assert abs(float(np.sum(m*w0.astype(np.float64))*float(U)) - float(np.sum(SS.INC))) < 1e-5*float(np.sum(SS.INC))
    equal = pipeline.spectral_photon_list([3., 3., 0., 3.], [1., 1., 0., 1.], [8, 8, 0, 8], 16, np.float32)
    assert np.all(equal[1][[0, 1, 3]] == 1.0) and np.all(equal[2][[0, 1, 3]] == 0.25)
    with pytest.raises(ValueError, match="no incident flux"):
        pipeline.spectral_photon_list([3., 0.], [0., 0.], [1, 1], 16, np.float64)


# ---- 2: the restatement

def test_search_steps_over_empty_ranges():
    pe = np.array([0, 4, 4, 4, 9, 9, 12])
    assert [SP.gpt_of_photon(pe, p) for p in range(13)] == [0]*4 + [3]*5 + [5]*3 + [6]
    assert SP.ranges_by_gpt(pe, 2, 9) == [(0, 2, 2), (3, 0, 5), (5, 0, 2)]
    assert SP.ranges_by_gpt(pe, 4, 0) == [] and SP.ranges_by_gpt(pe, 10, 10) == [(5, 1, 2)]


@pytest.mark.parametrize("with_bg", [True, False])
def test_with_unit_weights_the_counts_are_the_integer_sum_over_g_points(with_bg):
    sc, bg = SS.general(np.float64) if with_bg else SS.plain(np.float64)
    m = np.array([2, 2, 0, 2, 2])
    pe = np.concatenate([[0], np.cumsum(m*sc.ncol)])
    got = SP.trace_counts(sc, bg, pe, np.ones(5), 0, int(pe[-1]))
    want = None
    for g in (0, 1, 3, 4):
        c = R.trace_counts(sc, g, 0, 2*sc.ncol, bg=bg)
        want = c if want is None else {k: want[k] + c[k] for k in COUNTS}
    for k in COUNTS:
        assert np.array_equal(got[k], want[k]), k
    assert got["n_capped"] == 0 and got["abs_dif"].any() and got["sfc_dn_dif"].any()
    assert got["toa_up"].any() == with_bg


def test_ranges_add_up_exactly_inside_a_g_point_and_on_a_boundary():
    sc, bg = SS.general(np.float64)
    m = np.array([3, 1, 0, 2, 1])
    pe, w0, _, _ = SP.photon_list(sc, m)
    n = int(pe[-1])
    whole = SP.trace_counts(sc, bg, pe, w0, 0, n)
    for cuts in ((0, int(pe[1]) - 5, n), (0, int(pe[1]), n), (0, int(pe[2]), int(pe[3]) + 7, n)):
        parts = [SP.trace_counts(sc, bg, pe, w0, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
        for k in COUNTS:
            assert np.array_equal(sum(p[k] for p in parts[1:]) + parts[0][k], whole[k]), (cuts, k)
    assert whole["n_capped"] == 0
    # the weights change the deposits alone: with w0 = 2 on g-point 0 every deposit doubles before it is rounded (a photon leaves
    # through TOA at most once, so toa_up differs from twice itself by at most one count per photon) and the paths are the same
    one = SP.trace_counts(sc, bg, pe, np.ones(5), 0, int(pe[1]))
    two = SP.trace_counts(sc, bg, pe, np.array([2., 1., 1., 1., 1.]), 0, int(pe[1]))
    off = np.abs(two["toa_up"].astype(np.int64) - 2*one["toa_up"].astype(np.int64))
    assert one["toa_up"].any() and int(off.max()) <= int(pe[1]) and np.all(two["toa_up"] >= one["toa_up"])
    assert two["events"] == one["events"]


def test_the_restatement_binds_nothing_while_it_runs():
    """The weight, the background, the aerosol and the table are arguments of the event loops: after a forward and a backward
    spectral call, and after a call that raises part-way (its second g-point has no weight), every attribute of every restatement
    module is bound to the object it was bound to before."""
    import raytracer_bw_spectral_scenes as BSS
    modules = (R, B, P, SP, BSP)
    before = [dict(vars(mod)) for mod in modules]
    sc, bg = SS.general(np.float64)
    sensor = BSS.sensors(sc)["inside"]
    m = np.array([1, 1, 0, 1, 1])
    pe, w0, _, _ = SP.photon_list(sc, m)
    assert SP.trace_counts(sc, bg, pe, w0, 0, int(pe[-1]))["abs_dif"].any()
    re, rw0, _ = BSP.ray_list(sc, sensor, m)
    assert BSP.trace_counts(sc, bg, sensor, re, rw0, 0, int(re[-1]))["counts"].any()
    with pytest.raises(IndexError):
        SP.trace_counts(sc, bg, pe, w0[:1], 0, int(pe[-1]))
    with pytest.raises(IndexError):
        BSP.trace_counts(sc, bg, sensor, re, rw0[:1], 0, int(re[-1]))
    for mod, was in zip(modules, before):
        now = vars(mod)
        assert set(now) == set(was), mod.__name__
        for k, v in was.items():
            assert now[k] is v, (mod.__name__, k)


# ---- 4: what the allocation is for

def test_variance_ratio_of_the_synthetic_shortwave_set():
    """ngpt sum inc^2 / (sum inc)^2: the broadband variance of the equal split over that of the split in proportion to the flux, at an
    equal per-photon spread in every g-point (DESIGN 4.19 records the number). At least 1 by Cauchy-Schwarz."""
    kd = synthetic.make_kdist("sw", ngpt=224, nbnd=14)
    inc = np.asarray(kd.solar_source, dtype=np.float64)
    ratio = inc.size*float(np.sum(inc*inc)) / float(np.sum(inc))**2
    print(f"raytracer_spectral variance ratio of the synthetic 224-g-point shortwave set: {ratio:.3f} "
          f"(inc spans {inc.min():.3e} .. {inc.max():.3e})")
    assert ratio >= 1.0
