"""CPU tests of the restatement of the backward tracer with the rays of all g-points in one launch (raytracer_bw_spectral_ref.py,
DESIGN 4.21): with unit weights the counts of a band are the integer sum of raytracer_bw_ref.trace_counts_bw over its g-points,
ranges of the list add up, the clamp follows the weight, and the channel matrix is a sum in band order."""
import numpy as np
import pytest

import raytracer_bw_ref as B
import raytracer_bw_spectral_ref as BSP
import raytracer_bw_spectral_scenes as BSS


def _unit(m):
    return np.where(np.asarray(m) > 0, 1.0, 0.0)


@pytest.mark.parametrize("scene", ["general", "plain"])
def test_unit_weights_give_the_integer_sum_over_the_band_s_g_points(scene):
    sc, bg = getattr(BSS, scene)(np.float64)
    sensor = BSS.sensors(sc)["inside"]
    m = np.array([2, 1, 0, 3, 1])
    ray_end, _, _ = BSP.ray_list(sc, sensor, m)
    npix = BSS.NPX*BSS.NPY
    assert ray_end[BSS.EMPTY] == ray_end[BSS.EMPTY + 1] and ray_end[-1] == m.sum()*npix
    got = BSP.trace_counts(sc, bg, sensor, ray_end, _unit(m), 0, int(ray_end[-1]))
    for b, band in enumerate(BSS.BANDS):
        want = np.zeros(npix, dtype=np.uint64)
        for g in band:
            if m[g] > 0:
                want = want + B.trace_counts_bw(sc, sensor, g, 0, int(m[g])*npix, bg=bg)["counts"]
        assert np.array_equal(got["counts"][b], want) and want.any(), b
    assert got["n_capped"] == 0 and got["n_clamped"] == 0


def test_ranges_of_the_list_add_up():
    sc, bg = BSS.general(np.float64)
    sensor = BSS.sensors(sc)["slant"]
    m = np.array([2, 1, 0, 2, 1])
    ray_end, w0, _ = BSP.ray_list(sc, sensor, m)
    n = int(ray_end[-1])
    whole = BSP.trace_counts(sc, bg, sensor, ray_end, w0, 0, n)
    # cut inside a g-point, and on the boundary beside the empty range of the dark g-point
    cuts = (0, int(ray_end[1]) - 5, int(ray_end[BSS.EMPTY]), n)
    parts = [BSP.trace_counts(sc, bg, sensor, ray_end, w0, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(whole["counts"], sum(p["counts"] for p in parts)) and whole["counts"].all()
    assert np.array_equal(whole["n_dep"], sum(p["n_dep"] for p in parts))
    assert whole["events"] == sum(p["events"] for p in parts)


def test_the_weights_carry_the_fluxes_and_the_clamp_follows_the_weight():
    sc, bg = BSS.plain(np.float64)
    sensor = BSS.sensors(sc)["nadir"]
    m = np.array([5, 1, 0, 2, 1])
    ray_end, w0, U = BSP.ray_list(sc, sensor, m)
    assert np.allclose(m*w0*U, sc.inc_dir) and w0[BSS.EMPTY] == 0
    n = int(ray_end[1])
    plain = BSP.trace_counts(sc, bg, sensor, ray_end, _unit(m), 0, n)
    # a weight of 2^40 lifts every deposit above 2^-20 over the clamp of 2^20: it then counts 2^52 exactly
    big = BSP.trace_counts(sc, bg, sensor, ray_end, np.full(BSS.NGPT, 2.0**40), 0, n)
    assert plain["n_clamped"] == 0 and 0 < big["n_clamped"] <= big["n_dep"].sum()
    assert np.all(big["counts"][0] <= big["n_dep"][0].astype(np.uint64) << np.uint64(52))
    assert not big["counts"][1].any()


def test_channels_sum_in_band_order():
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 1 << 40, (3, 7)).astype(np.uint64)
    x = counts.astype(np.float64) * 2.0**-32
    ident = BSP.channels(counts, np.eye(3), 1.5, np.float64)
    assert np.array_equal(ident, 1.5*x)
    M = np.array([[1., 1., 1.], [0.25, 0., 2.]])
    got = BSP.channels(counts, M, 1.5, np.float64)
    assert np.array_equal(got[0], 1.5*((x[0] + x[1]) + x[2])) and np.array_equal(got[1], 1.5*((0.25*x[0] + 0.*x[1]) + 2.*x[2]))
    assert BSP.channels(counts, M, 1.5, np.float32).dtype == np.float32


def test_render_is_one_conversion_of_the_summed_counts():
    sc, bg = BSS.plain(np.float64)
    sensor = BSS.sensors(sc)["flux"]
    m = np.array([2, 1, 0, 1, 1])
    r = BSP.render(sc, bg, sensor, m, np.eye(2))
    assert r["radiance"].shape == (2, BSS.NPX*BSS.NPY) and np.all(r["radiance"] > 0)
    scale = float(r["U"]) / sc.mu0
    assert np.allclose(r["radiance"], scale*r["counts"].astype(np.float64)*2.0**-32, rtol=1e-15)
