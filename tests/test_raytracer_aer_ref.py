"""CPU tests of the numpy restatement of aerosol as a third scattering species (Scene.aerosol and Background.aerosol of
tests/raytracer_ref.py) on the
scenes and seeds that the GPU tests reuse (tests/raytracer_aer_scenes.py). Statistical bound (derived, not measured): a tally whose
per-photon contribution lies in [0, 1] with mean p has a standard deviation of at most sqrt(p (1 - p) / N); five are allowed."""
import dataclasses

import numpy as np
import pytest

import raytracer_ref as R
import raytracer_bw_ref as B
import raytracer_bg_scenes as SB
import raytracer_aer_scenes as SA
from raytracer_pinned import pinned

FW = R.ALL_COUNTS
BW = ("counts", "n_dep", "n_capped", "n_clamped", "events", "walk_cells")


@pytest.mark.parametrize("how", ["none", "zeros"])
def test_without_aerosol_the_restatement_is_the_one_without(how):
    """No aerosol, and aerosol triples of zeros (with g_a and ssa_a that are not zero), give the integers of the tracers without
    aerosol. zeros: against aerosol None, two different inputs of the one loop. none: the loop is the one that draws among three
    species, and what the loops without aerosol gave is recorded (raytracer_pinned.py: the cases `via` raytracer_ref,
    raytracer_bw_ref and raytracer_bg_ref); pinned() checks that the loop still gives it, with and without a background."""
    if how == "none":
        for name in ("plain", "plain_table", "bg", "bg_f32", "bg_top0", "bg_none", "bg_table"):
            fw, bw = pinned("fw_" + name), pinned("bw_" + name)
            assert fw["abs_dif"].any() and bw["counts"].any() and fw["aerosol_scatterings"] == 0 == bw["aerosol_scatterings"], name
        for d, keys in (("fw", FW + ("n_capped", "events")), ("bw", BW)):
            for k in keys:
                assert np.array_equal(pinned(d + "_bg")[k], pinned(d + "_aer_none")[k]), (d, k)
        return
    sc0, bg0 = SB.general(np.float64)
    sc, bg = SB.general(np.float64)
    grid, aloft = SA.zeros(np.float64)
    sc.aerosol, bg.aerosol = (grid[0], grid[1] + 0.9, grid[2] + 0.7), (aloft[0], aloft[1] + 0.9, aloft[2] + 0.7)
    cam = SB.cameras(sc0, bg0)
    for b0, b in ((bg0, bg), (None, None)):
        want, got = R.trace_counts(sc0, 1, 5, 16*sc.ncol, bg=b0), R.trace_counts(sc, 1, 5, 16*sc.ncol, bg=b)
        for k in FW + ("n_capped", "events"):
            assert np.array_equal(want[k], got[k]), k
        assert want["abs_dif"].any()
        for name in ("inside", "nadir") + (("aloft",) if b is not None else ()):
            want, got = B.trace_counts_bw(sc0, cam[name], 1, 3, 8*12, bg=b0), B.trace_counts_bw(sc, cam[name], 1, 3, 8*12, bg=b)
            for k in BW:
                assert np.array_equal(want[k], got[k]), (name, k)
            assert want["counts"].any()


def test_the_restatement_leaves_the_existing_ones_alone_when_it_raises():
    """a call that raises leaves the next one what it was (nothing is bound while a call runs: test_raytracer_spectral_ref.py)"""
    sc, bg = SA.general(np.float64)
    cam = SB.cameras(sc, bg)["inside"]
    before = B.trace_counts_bw(sc, cam, 0, 0, 8, bg=bg)
    with pytest.raises(ValueError):
        B.trace_counts_bw(sc, cam, 0, 0, 7, ranges=2, bg=bg)
    after = B.trace_counts_bw(sc, cam, 0, 0, 8, bg=bg)
    for k in BW:
        assert np.array_equal(before[k], after[k]), k


def test_k_null_and_profile_hold_the_aerosol():
    sc, bg = SA.general(np.float64)
    for g in range(2):
        kn = R.k_null(sc, g)
        plain = R.k_null(dataclasses.replace(sc, aerosol=None), g)
        assert kn.shape == plain.shape and np.all(kn >= plain) and (np.any(kn > plain) == (g == 1))
        prof, plain = R.profile(sc, bg, g), R.profile(sc, bg, g, aerosol=False)
        assert prof.shape == (7, bg.nbg + 1) and plain.shape == (5, bg.nbg + 1) and np.all(prof[5:, bg.nbg] == 0)
        assert np.array_equal(prof[2:4], plain[2:4]) and np.all(prof[0] >= plain[0]) and prof[0, 0] > plain[0, 0]
        assert prof[5, 0] > 0 and prof[5, 1] == 0 and prof[6, 0] in (0.7, 0.65)
        assert prof[4, bg.nbg] > plain[4, bg.nbg] and prof[4, 0] == plain[4, 0]


@pytest.mark.parametrize("top_at_1", [False, True])
def test_swap_cloud_and_aerosol(top_at_1):
    """T as cloud (A) and T as aerosol (B) give the same integers: the formulas with their parentheses make it exact"""
    (sa, ba), (sb, bb) = SA.swap(np.float64, top_at_1)
    ca, cb = R.trace_counts(sa, 1, 0, 16*sa.ncol, bg=ba), R.trace_counts(sb, 1, 0, 16*sb.ncol, bg=bb)
    for k in FW + ("n_capped", "events"):
        assert np.array_equal(ca[k], cb[k]), k
    assert ca["abs_dif"].any() and ca["toa_up"].any()
    for name, cam in SB.cameras(sa, ba).items():
        ra, rb = B.trace_counts_bw(sa, cam, 1, 0, 8*12, bg=ba), B.trace_counts_bw(sb, cam, 1, 0, 8*12, bg=bb)
        for k in BW:
            assert np.array_equal(ra[k], rb[k]), (name, k)
        assert ra["counts"].any()


@pytest.mark.parametrize("independent_column", [False, True])
def test_a_purely_absorbing_aerosol_is_beer(independent_column):
    sc, bg = SA.beer(np.float64, independent_column)
    for g in range(2):
        c = R.trace_counts(sc, g, 0, SA.PPP_BEER*sc.ncol, bg=bg)
        assert c["n_capped"] == 0
        SA.check_beer(sc, bg, g, c, SA.PPP_BEER, f"numpy ic={independent_column}")


def test_conservative_scene_loses_nothing():
    sc, bg = SA.conservative(np.float64)
    for g in range(2):
        c = R.trace_counts(sc, g, 0, SB.PPP_CONSERVATIVE*sc.ncol, bg=bg)
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
        c = R.trace_counts(sc, g, 0, 256*sc.ncol, max_events=SA.MAX_EVENTS, bg=bg)
        assert c["n_capped"] == 0
        for name, sensor in SB.flux_sensors(sc).items():
            r = B.trace_counts_bw(sc, sensor, g, 0, 64*sc.ncol, max_events=SA.MAX_EVENTS, bg=bg)
            assert r["n_capped"] == 0 and r["n_clamped"] == 0 and r["counts"].any(), name
