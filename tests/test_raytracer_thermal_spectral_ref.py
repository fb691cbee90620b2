"""CPU tests of the restatement of the thermal tracer with the rays of all g-points in one launch (raytracer_thermal_spectral_ref.py,
DESIGN 4.24): with unit weights the counts of a band are the integer sum of raytracer_thermal_ref.trace_counts_thermal over its
g-points, ranges of the list add up, the clamp follows the weight, equal m_g give weights of exactly 1, the chain refuses what would
bias the result, and the statistical scene's restatement stays inside the derived bound that the GPU test holds the device to."""
import numpy as np
import pytest

import raytracer_thermal_ref as T
import raytracer_thermal_spectral_ref as TSP
import thermal_spectral_scenes as TSS
from rte_rrtmgp_cpp_amd import pipeline


def _unit(m):
    return np.where(np.asarray(m) > 0, 1.0, 0.0)


@pytest.mark.parametrize("cloud", [True, False])
def test_unit_weights_give_the_integer_sum_over_the_band_s_g_points(cloud):
    sc = TSS.general(np.float64, cloud=cloud)
    sensor = TSS.sensors(sc)["inside"]
    m = np.array([2, 1, 0, 3, 1])
    ray_end, _, _ = TSP.ray_list(sc, sensor, m)
    assert ray_end[TSS.EMPTY] == ray_end[TSS.EMPTY + 1] and ray_end[-1] == m.sum()*TSS.NPIX
    got = TSP.trace_counts(sc, sensor, ray_end, _unit(m), 0, int(ray_end[-1]))
    for b, band in enumerate(TSS.BANDS):
        want = np.zeros(TSS.NPIX, dtype=np.uint64)
        for g in band:
            if m[g] > 0:
                want = want + T.trace_counts_thermal(sc, sensor, g, 0, int(m[g])*TSS.NPIX)["counts"]
        assert np.array_equal(got["counts"][b], want) and want.any(), b
    assert got["n_capped"] == 0 and got["n_clamped"] == 0


def test_ranges_of_the_list_add_up():
    sc = TSS.general(np.float64, top_at_1=False)
    sensor = TSS.sensors(sc)["slant"]
    m = np.array([2, 1, 0, 2, 1])
    ray_end, w0, _ = TSP.ray_list(sc, sensor, m)
    n = int(ray_end[-1])
    whole = TSP.trace_counts(sc, sensor, ray_end, w0, 0, n)
    # cut inside a g-point, and on the boundary beside the empty range of the dark g-point
    cuts = (0, int(ray_end[1]) - 5, int(ray_end[TSS.EMPTY]), n)
    parts = [TSP.trace_counts(sc, sensor, ray_end, w0, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(whole["counts"], sum(p["counts"] for p in parts)) and whole["counts"].all()
    assert np.array_equal(whole["n_dep"], sum(p["n_dep"] for p in parts))
    assert whole["events"] == sum(p["events"] for p in parts)


def test_the_clamp_follows_the_weight():
    sc = TSS.general(np.float64, gas_scatters=False)
    sensor = TSS.sensors(sc)["flux"]
    m = np.array([5, 1, 0, 2, 1])
    ray_end, w0, U = TSP.ray_list(sc, sensor, m)
    assert np.allclose(m*w0*U, _unit(m)) and w0[TSS.EMPTY] == 0
    n = int(ray_end[1])
    plain = TSP.trace_counts(sc, sensor, ray_end, _unit(m), 0, n)
    # a weight of 2^40 lifts every source above 2^-20 over the clamp of 2^20: such a deposit then counts 2^52 exactly
    big = TSP.trace_counts(sc, sensor, ray_end, np.full(TSS.NGPT, 2.0**40), 0, n)
    assert plain["n_clamped"] == 0 and 0 < big["n_clamped"] <= big["n_dep"].sum()
    assert np.all(big["counts"][0] <= big["n_dep"][0].astype(np.uint64) << np.uint64(52))
    assert not big["counts"][1].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_equal_rays_give_weights_of_exactly_one(dtype):
    sc = TSS.general(dtype)
    sensor = TSS.sensors(sc)["inside"]
    for rays in (1, 3, 7, 1000):
        m = np.where(np.asarray(TSS.S_G) > 0, rays, 0)
        ray_end, w0, U = TSP.ray_list(sc, sensor, m)
        assert np.array_equal(w0, _unit(m).astype(dtype)) and w0.dtype == np.dtype(dtype), rays
        assert U == np.dtype(dtype).type(1.)/np.dtype(dtype).type(rays)
        # the scaled scene is then the scene, bit for bit
        scaled = TSP.scaled_scene(sc, w0)
        keep = list(TSS.ACTIVE)
        assert np.array_equal(scaled.lay_src[keep], sc.lay_src[keep]) and np.array_equal(scaled.sfc_src[keep], sc.sfc_src[keep])
    everywhere = np.full(TSS.NGPT, 5)
    assert np.array_equal(TSP.ray_list(sc, sensor, everywhere)[1], np.ones(TSS.NGPT, dtype=dtype))


def test_render_is_one_conversion_of_the_summed_counts():
    sc = TSS.general(np.float64, cloud=False)
    sensor = TSS.sensors(sc)["flux"]
    m = np.array([2, 1, 0, 1, 1])
    r = TSP.render(sc, sensor, m, np.eye(2))
    assert r["radiance"].shape == (2, TSS.NPIX) and np.all(r["radiance"] > 0)
    assert np.allclose(r["radiance"], float(r["U"])*r["counts"].astype(np.float64)*2.0**-32, rtol=1e-15)


def test_render_lw_refuses_what_would_bias_the_result():
    sc = TSS.general(np.float64)
    e = TSS.emission(sc)
    lay_max = sc.lay_src.reshape(TSS.NGPT, -1).max(axis=1)
    m = pipeline.emission_allocation(e, lay_max, sc.top_radiance, 64)
    assert int(m.sum()) == 64 and m[TSS.EMPTY] == 0 and all(m[g] >= 1 for g in TSS.ACTIVE) and m[0] > m[3] > m[4] > m[1]
    assert np.array_equal(m, pipeline.spectral_allocation(e, 64)) and np.array_equal(m, pipeline.emission_allocation(e, lay_max, None, 64))
    glowing = lay_max.copy(); glowing[TSS.EMPTY] = 1e-3
    with pytest.raises(ValueError, match="g-point 2 has no surface emission"):
        pipeline.emission_allocation(e, glowing, None, 64)
    top = np.zeros(TSS.NGPT); top[TSS.EMPTY] = 0.5
    with pytest.raises(ValueError, match="g-point 2 has no surface emission"):
        pipeline.emission_allocation(e, lay_max, top, 64)
    with pytest.raises(ValueError, match="per g-point"):
        pipeline.emission_allocation(e, lay_max[:-1], None, 64)
    with pytest.raises(ValueError, match="cannot give 1 to each of 4"):
        pipeline.emission_allocation(e, lay_max, None, 3)
    with pytest.raises(ValueError, match="allocation is None or 'emission'"):
        pipeline.render_lw(None, None, None, 4, 4, 1., 1., 1., None, 8, 0, allocation="flux")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_statistical_scene_s_restatement_stays_inside_the_derived_bound(dtype):
    """What test_gpu_raytracer_thermal_spectral.py asks of the device, asked of the restatement with the same seed: every pixel's
    radiance by band within 5 sigma of Schwarzschild's sum, sigma from schwarzschild_sigma; and every ray deposits exactly once."""
    sc = TSS.schwarzschild(dtype)
    sensor = TSS.nadir()
    m = pipeline.spectral_allocation(TSS.emission(sc), TSS.STAT_RAYS)
    assert m[TSS.EMPTY] == 0 and len(set(m[list(TSS.ACTIVE)])) == 4
    r = TSP.render(sc, sensor, m, np.eye(TSS.NBND))
    assert r["n_capped"] == 0 and r["n_clamped"] == 0
    per_band = np.array([sum(m[g] for g in band) for band in TSS.BANDS])
    assert np.array_equal(r["n_dep"], np.repeat(per_band[:, None], TSS.NPIX, axis=1))
    mean, sigma = TSS.schwarzschild_sigma(sc, m)
    L, _ = TSS.schwarzschild_expected(sc)
    assert np.all(mean > 0) and np.all(sigma > 0) and np.all(sigma < 0.2*mean) and L[TSS.EMPTY] == 0
    rad = r["radiance"].astype(np.float64)
    dev_pix = np.abs(rad - mean[:, None]) / sigma[:, None]
    dev_mean = np.abs(rad.mean(axis=1) - mean) / (sigma/np.sqrt(TSS.NPIX))
    print(f"thermal spectral restatement {np.dtype(dtype).name}: m = {list(m)}, worst deviation {float(dev_pix.max()):.2f} sigma per pixel, "
          f"{float(dev_mean.max()):.2f} of the image mean (bound 5)")
    assert np.all(dev_pix <= 5) and np.all(dev_mean <= 5)
