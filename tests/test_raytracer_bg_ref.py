"""CPU tests of the numpy restatement of the ray tracers with a background atmosphere (bg= of tests/raytracer_ref.py)
against closed forms, on the scenes and seeds that the GPU tests reuse (tests/raytracer_bg_scenes.py). Statistical bound (derived,
not measured): a tally whose per-photon contribution lies in [0, 1] with mean p has a standard deviation of at most
sqrt(p (1 - p) / N); five of these are allowed."""
import numpy as np
import pytest

import raytracer_ref as R
import raytracer_bw_ref as B
import raytracer_bg_scenes as SB
from raytracer_pinned import pinned

from raytracer_bg_scenes import (ONE, PPP_ABSORBING, PPP_SPLIT, PPP_CONSERVATIVE, check_absorbing, check_conservative, check_split,
                                 shadow_full_count)


@pytest.mark.parametrize("independent_column", [False, True])
def test_absorbing_background_over_an_empty_grid_is_beer(independent_column):
    sc, bg = SB.absorbing(np.float64, independent_column)
    for g in range(2):
        c = R.trace_counts(sc, g, 0, PPP_ABSORBING*sc.ncol, bg=bg)
        assert c["n_capped"] == 0
        check_absorbing(sc, bg, g, c, PPP_ABSORBING, f"numpy ic={independent_column}")


def test_conservative_scene_loses_nothing():
    sc, bg = SB.conservative(np.float64)
    for g in range(2):
        check_conservative(R.trace_counts(sc, g, 0, PPP_CONSERVATIVE*sc.ncol, bg=bg), PPP_CONSERVATIVE*sc.ncol, f"numpy g-point {g}")


def test_a_column_split_into_grid_and_background_gives_the_same_fluxes():
    (a, _), (b, bg) = SB.split(np.float64)
    for g in range(2):
        ca = R.trace_counts(a, g, 0, PPP_SPLIT*a.ncol)
        cb = R.trace_counts(b, g, 0, PPP_SPLIT*b.ncol, bg=bg)
        assert ca["n_capped"] == 0 and cb["n_capped"] == 0
        check_split(ca, cb, PPP_SPLIT, a.ncol, g, "numpy")


def test_without_a_background_the_restatement_is_the_one_without():
    """The tracer without a background is the original one, bit for bit. The original event loops had no notion of a background;
    what they gave is recorded (raytracer_pinned.py: the cases `via` raytracer_ref and raytracer_bw_ref), and the loop
    that deals lanes to the grid and to the background gives it with bg=None, in both precisions, as it gave it when it was a
    module of its own (`via` raytracer_bg_ref)."""
    for name in ("plain", "plain_f32", "plain_top0", "plain_table", "bg_none", "bg_none_f32"):
        fw, bw = pinned("fw_" + name), pinned("bw_" + name)
        assert fw["abs_dif"].any() and bw["counts"].any(), name
        # nothing is tallied above the domain top, and there is no layer to absorb
        assert not (fw["toa_up"].any() or fw["tod_dn_dir"].any() or fw["tod_dn_dif"].any()) and fw["bg_abs_dir"].size == 0, name
    for k in R.COUNT_NAMES + ("n_capped", "events"):
        assert np.array_equal(pinned("fw_plain")[k], pinned("fw_bg_none")[k]), k
    for k in ("counts", "n_dep", "n_capped", "n_clamped", "events", "walk_cells"):
        assert np.array_equal(pinned("bw_plain")[k], pinned("bw_bg_none")[k]), k


def test_counts_are_additive_over_ranges_with_a_background():
    sc, bg = SB.general(np.float64)
    n = 16*sc.ncol
    whole = R.trace_counts(sc, 1, 0, n, bg=bg)
    a, b = R.trace_counts(sc, 1, 0, n//3, bg=bg), R.trace_counts(sc, 1, n//3, n - n//3, bg=bg)
    assert whole["n_capped"] == 0
    for k in R.ALL_COUNTS:
        assert np.array_equal(whole[k], a[k] + b[k]), k
        assert whole[k].any() or k == "sfc_dn_dir", k          # (of 16 photons per pixel none comes down the whole way unscattered)
    cam = SB.cameras(sc, bg)["aloft"]
    whole = B.trace_counts_bw(sc, cam, 1, 0, 16*12, bg=bg)
    a, b = B.trace_counts_bw(sc, cam, 1, 0, 5*12, bg=bg), B.trace_counts_bw(sc, cam, 1, 5*12, 11*12, bg=bg)
    assert np.array_equal(whole["counts"], a["counts"] + b["counts"]) and whole["counts"].any()
    assert whole["n_capped"] == 0 and whole["n_clamped"] == 0


def test_backward_shadow_under_an_absorbing_background_is_exact():
    """S2 of raytracer_bw_scenes under the absorbing background: a fully lit pixel deposits rays x llrint(0.5 mu0/pi T 2^32) with
    T = exp(-(0 + tau_bg/mu0)), the one exp that the restatement forms; shadowed pixels count 0. The camera (position.z = 0) starts
    at the domain top, so its own rays do not cross the background."""
    import raytracer_bw_scenes as BS
    sc, bg = SB.shadow(np.float64, "x", False)
    dark, full = BS.shadow_classes(sc)
    rays = 8
    cam = B.orthographic(sc.nx, sc.ny, (0., 0., -1.))
    c = B.trace_counts_bw(sc, cam, 0, 0, rays*sc.ncol, bg=bg)
    assert c["n_capped"] == 0 and c["n_clamped"] == 0
    want = shadow_full_count(sc, bg, 0, rays)
    assert want < BS.shadow_full_count(sc, rays)
    assert np.all(c["counts"][dark] == 0)
    assert np.all(c["counts"][full] == np.uint64(want)), c["counts"][full] / float(ONE)
    assert np.all(c["counts"][~dark & ~full] <= np.uint64(want))
