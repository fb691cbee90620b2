"""CPU tests of the numpy restatement of aerosol as a third scattering species (tests/raytracer_aer_ref.py) on the
scenes and seeds that the GPU tests reuse (tests/raytracer_aer_scenes.py). Statistical bound (derived, not measured): a tally whose
per-photon contribution lies in [0, 1] with mean p has a standard deviation of at most sqrt(p (1 - p) / N); five are allowed."""
import numpy as np
import pytest

import raytracer_ref as R
import raytracer_bw_ref as B
import raytracer_bg_ref as BG
import raytracer_bg_scenes as SB
import raytracer_bw_scenes as BS
import raytracer_aer_ref as A
import raytracer_aer_scenes as SA

FW = R.COUNT_NAMES + BG.BG_COUNT_NAMES
BW = ("counts", "n_dep", "n_capped", "n_clamped", "events", "walk_cells")


@pytest.mark.parametrize("how", ["none", "zeros"])
def test_without_aerosol_the_restatement_is_the_one_without(how):
    """no aerosol, and aerosol triples of zeros (with g_a and ssa_a that are not zero), give the existing restatements' integers"""
    sc0, bg0 = SB.general(np.float64)
    grid, aloft = (None, None) if how == "none" else SA.zeros(np.float64)
    if how == "zeros":
        grid, aloft = (grid[0], grid[1] + 0.9, grid[2] + 0.7), (aloft[0], aloft[1] + 0.9, aloft[2] + 0.7)
    sc, bg = SA.with_aerosol(sc0, bg0, grid, aloft)
    cam = SB.cameras(sc0, bg0)
    for b0, b in ((bg0, bg), (None, None)):
        want, got = BG.trace_counts(sc0, b0, 1, 5, 16*sc.ncol), A.trace_counts(sc, b, 1, 5, 16*sc.ncol)
        for k in FW + ("n_capped", "events"):
            assert np.array_equal(want[k], got[k]), k
        assert want["abs_dif"].any()
        for name in ("inside", "nadir") + (("aloft",) if b is not None else ()):
            want, got = BG.trace_counts_bw(sc0, b0, cam[name], 1, 3, 8*12), A.trace_counts_bw(sc, b, cam[name], 1, 3, 8*12)
            for k in BW:
                assert np.array_equal(want[k], got[k]), (name, k)
            assert want["counts"].any()
    want, got = R.trace_counts(sc0, 1, 5, 16*sc.ncol), A.trace_counts(sc, None, 1, 5, 16*sc.ncol)
    for k in R.COUNT_NAMES + ("n_capped", "events"):
        assert np.array_equal(want[k], got[k]), k
    want, got = B.trace_counts(sc0, cam["inside"], 0, 3, 8*12), A.trace_counts_bw(sc, None, cam["inside"], 0, 3, 8*12)
    for k in BW:
        assert np.array_equal(want[k], got[k]), k
    # the steps of the existing restatements are back in place
    assert R.Grid is not A.AerGrid and BG.Medium is not A.AerMedium and R.collide is not A.collide


def test_the_restatement_leaves_the_existing_ones_alone_when_it_raises():
    sc, bg = SA.general(np.float64)
    with pytest.raises(ValueError):
        A.trace_counts_bw(sc, bg, SB.cameras(sc, bg)["inside"], 0, 0, 7, ranges=2)
    assert R.Grid is not A.AerGrid and R.collision_outcome is not A.collision_outcome and BG.collide_bg is not A.collide_bg


def test_k_null_and_profile_hold_the_aerosol():
    sc, bg = SA.general(np.float64)
    for g in range(2):
        kn = A.k_null(sc, g)
        plain = R.k_null(sc, g)
        assert kn.shape == plain.shape and np.all(kn >= plain) and (np.any(kn > plain) == (g == 1))
        prof, plain = A.profile(sc, bg, g), BG.profile(sc, bg, g)
        assert prof.shape == (7, bg.nbg + 1) and np.all(prof[5:, bg.nbg] == 0)
        assert np.array_equal(prof[2:4], plain[2:4]) and np.all(prof[0] >= plain[0]) and prof[0, 0] > plain[0, 0]
        assert prof[5, 0] > 0 and prof[5, 1] == 0 and prof[6, 0] in (0.7, 0.65)
        assert prof[4, bg.nbg] > plain[4, bg.nbg] and prof[4, 0] == plain[4, 0]


@pytest.mark.parametrize("top_at_1", [False, True])
def test_swap_cloud_and_aerosol(top_at_1):
    """T as cloud (A) and T as aerosol (B) give the same integers: the formulas with their parentheses make it exact"""
    (sa, ba), (sb, bb) = SA.swap(np.float64, top_at_1)
    ca, cb = A.trace_counts(sa, ba, 1, 0, 16*sa.ncol), A.trace_counts(sb, bb, 1, 0, 16*sb.ncol)
    for k in FW + ("n_capped", "events"):
        assert np.array_equal(ca[k], cb[k]), k
    assert ca["abs_dif"].any() and ca["toa_up"].any()
    for name, cam in SB.cameras(sa, ba).items():
        ra, rb = A.trace_counts_bw(sa, ba, cam, 1, 0, 8*12), A.trace_counts_bw(sb, bb, cam, 1, 0, 8*12)
        for k in BW:
            assert np.array_equal(ra[k], rb[k]), (name, k)
        assert ra["counts"].any()


@pytest.mark.parametrize("independent_column", [False, True])
def test_a_purely_absorbing_aerosol_is_beer(independent_column):
    sc, bg = SA.beer(np.float64, independent_column)
    for g in range(2):
        c = A.trace_counts(sc, bg, g, 0, SA.PPP_BEER*sc.ncol)
        assert c["n_capped"] == 0
        SA.check_beer(sc, bg, g, c, SA.PPP_BEER, f"numpy ic={independent_column}")


def test_conservative_scene_loses_nothing():
    sc, bg = SA.conservative(np.float64)
    for g in range(2):
        c = A.trace_counts(sc, bg, g, 0, SB.PPP_CONSERVATIVE*sc.ncol)
        SB.check_conservative(c, SB.PPP_CONSERVATIVE*sc.ncol, f"numpy g-point {g}")


def test_the_general_scene_has_every_kind_of_cell():
    sc, bg = SA.general(np.float64)
    ta, tc, t = sc.aerosol[0][1], sc.cloud[0][1], sc.tau[1]
    share = float((ta > 0).mean())
    assert 0.35 <= share <= 0.65 and not sc.aerosol[0][0].any()
    assert np.any((ta > 0) & (tc == 0) & (t == 0)) and np.any((ta > 0) & (tc > 0) & (t > 0))
    assert bg.aerosol[0][:, 0].all()


def test_forward_against_backward_conditions_hold_on_the_restatement():
    """The GPU test of forward against backward takes n_capped == 0 and n_clamped == 0 as conditions; max_events = SA.MAX_EVENTS and
    the general direct scene meet them on the restatement alone, with the longest history far below the cap."""
    sc, bg = SA.general_direct(np.float64)
    for g in range(2):
        c = A.trace_counts(sc, bg, g, 0, 256*sc.ncol, max_events=SA.MAX_EVENTS)
        assert c["n_capped"] == 0
        for name, sensor in SB.flux_sensors(sc).items():
            r = A.trace_counts_bw(sc, bg, sensor, g, 0, 64*sc.ncol, max_events=SA.MAX_EVENTS)
            assert r["n_capped"] == 0 and r["n_clamped"] == 0 and r["counts"].any(), name
