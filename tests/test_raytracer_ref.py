"""CPU tests of the numpy restatement of the ray tracer (tests/raytracer_ref.py): Beer's law per pixel, exact conservation in the
analog scenes (every weight 0 or 1: integer identities), the slant-path geometry and the displaced shadow, additivity over photon
ranges. The statistical bound is derived (raytracer_scenes.sigma), five standard deviations, on fixed seeds."""
import numpy as np
import pytest

import raytracer_ref as R
import raytracer_scenes as S

ONE = 1 << 32
PPP = 512


def _counts(scene, ppp=PPP):
    out = [R.trace_counts(scene, g, 0, ppp*scene.ncol) for g in range(scene.tau.shape[0])]
    for c in out:
        assert c["n_capped"] == 0
    return out


@pytest.mark.parametrize("kn_is_grid", [True, False])
def test_beer_per_pixel(kn_is_grid):
    scene = S.beer(np.float64, kn_is_grid)
    want = S.beer_expected(scene)
    for g, c in enumerate(_counts(scene)):
        got = c["sfc_dn_dir"].astype(np.float64) / ONE / PPP
        assert np.all(np.abs(got - want[g]) <= 5*S.sigma(want[g], PPP)), (g, np.max(np.abs(got - want[g]) / S.sigma(want[g], PPP)))
        assert not c["sfc_dn_dif"].any() and not c["sfc_up"].any() and not c["tod_up"].any() and not c["abs_dif"].any()
        if kn_is_grid:          # k_null = k_ext in every cell: f_no_abs = 0, every weight is 0 or 1, the books balance in integers
            assert int(c["abs_dir"].sum()) + int(c["sfc_dn_dir"].sum()) == PPP*scene.ncol*ONE
            assert np.all(c["abs_dir"] % ONE == 0) and np.all(c["sfc_dn_dir"] % ONE == 0)


def test_top_at_1_only_reverses_the_layer_index():
    a = S.beer(np.float64, True, top_at_1=True)
    b = S.beer(np.float64, True, top_at_1=False)
    b.tau = np.ascontiguousarray(a.tau[:, ::-1]); b.ssa = np.ascontiguousarray(a.ssa[:, ::-1])
    ca, cb = R.trace_counts(a, 0, 0, 64*a.ncol), R.trace_counts(b, 0, 0, 64*b.ncol)
    assert np.array_equal(ca["sfc_dn_dir"], cb["sfc_dn_dir"]) and np.array_equal(ca["abs_dir"], cb["abs_dir"][::-1])


def test_slant_path_and_wrap():
    scene = S.slant(np.float64)
    want = S.beer_expected(scene)
    for g, c in enumerate(_counts(scene)):
        got = c["sfc_dn_dir"].astype(np.float64) / ONE / PPP
        assert np.all(np.abs(got - want[g]) <= 5*S.sigma(want[g], PPP))
        assert abs(got.mean() - want[g].mean()) <= 5*S.sigma(want[g].mean(), PPP*scene.ncol)
        assert not c["tod_up"].any() and not c["sfc_dn_dif"].any()


@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("along", ["x", "y"])
def test_shadow_is_displaced_along_the_direction_of_travel(along, top_at_1):
    scene = S.shadow(np.float64, along, top_at_1)
    lo, hi = R.pixel_path_range(scene, 0)
    lit, dark = hi == 0.0, lo > 40.0
    # the block's layer is k = 3 upward and tan(theta) = dx/dz: the shadow lies 3 cells further along the direction of travel
    n = scene.nx if along == "x" else scene.ny
    behind = [(m + 3) % n for m in (2, 3)]
    for pix in np.nonzero(dark)[0]:
        assert ((pix % scene.nx) if along == "x" else (pix // scene.nx)) in behind
    assert dark.sum() == 4 and lit.sum() == scene.ncol - 8
    c = R.trace_counts(scene, 0, 0, 64*scene.ncol)
    assert c["n_capped"] == 0
    assert np.all(c["sfc_dn_dir"][lit] == 64*ONE) and np.all(c["sfc_dn_dir"][dark] == 0)
    lay = scene.nz - 1 - 3 if top_at_1 else 3
    assert c["abs_dir"][lay].sum() == c["abs_dir"].sum() > 0


def test_conservative_scattering_loses_nothing():
    scene = S.conservative(np.float64)
    black = scene.sfc_albedo == 0
    for c in _counts(scene, 128):
        assert not c["abs_dir"].any() and not c["abs_dif"].any()
        for k in R.COUNT_NAMES[:4]:
            assert np.all(c[k] % ONE == 0), k
        assert int(c["tod_up"].sum()) + int((c["sfc_dn_dir"] + c["sfc_dn_dif"])[black].sum()) == 128*scene.ncol*ONE
        assert np.array_equal(c["sfc_up"][~black], (c["sfc_dn_dir"] + c["sfc_dn_dif"])[~black]) and not c["sfc_up"][black].any()


def test_counts_are_additive_over_photon_ranges():
    scene = S.general(np.float64)
    n = 16*scene.ncol
    whole = R.trace_counts(scene, 1, 0, n)
    a, b = R.trace_counts(scene, 1, 0, n//3), R.trace_counts(scene, 1, n//3, n - n//3)
    for k in R.COUNT_NAMES:
        assert np.array_equal(whole[k], a[k] + b[k]), k
    assert whole["events"] == a["events"] + b["events"] and whole["n_capped"] == 0
    # (expected-value absorption with roulette conserves energy in the mean only: no integer identity here; every tally is in use)
    assert whole["sfc_dn_dif"].any() and whole["abs_dif"].any() and whole["tod_up"].any()


def test_k_null_is_the_block_maximum():
    scene = S.general(np.float64)
    kn = R.k_null(scene, 0)
    assert kn.shape == (3, 2, 2)
    k_ext = ((scene.tau[0] + scene.cloud[0][0]) / scene.dz).reshape(6, 4, 8)[::-1]
    assert kn[1, 0, 1] == k_ext[2:4, 0:2, 4:8].max() and kn.max() == k_ext.max()


def test_float32_runs_the_same_algorithm():
    scene = S.beer(np.float32, False)
    want = S.beer_expected(scene)
    c = R.trace_counts(scene, 0, 0, 256*scene.ncol)
    got = c["sfc_dn_dir"].astype(np.float64) / ONE / 256
    assert c["n_capped"] == 0 and np.all(np.abs(got - want[0]) <= 5*S.sigma(want[0], 256))
