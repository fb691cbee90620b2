"""CPU tests of the restatement of the thermal tracer's cell sensors (raytracer_heating_ref.py): a black-body cavity
gives all-zero counts, ranges add up, with unit weights the spectral form is the integer sum over the g-points, the slab stays inside
five standard errors of the extended-precision truth (the bound that test_gpu_raytracer_heating.py holds the device to) and its ray
budget keeps the standard error below 2 % of the largest layer value, and a digest record (tests/golden/heating_ref_digests.json)
holds the restatement, and the steps of raytracer_ref that it imports, through later refactors."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import heating_scenes as HS
import raytracer_heating_ref as H
import thermal_scenes as TS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heating_ref_digests.json")
NCELL = HS.NCELL


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_cavity_gives_all_zero_counts(dtype):
    sc = HS.cavity(dtype)
    assert sc.cloud is not None and np.any(sc.ssa > 0) and np.all(sc.sfc_emis < 1)
    m = np.array([3, 2, 1, 2, 2])
    r = H.render(sc, m)
    assert not r["counts"].any() and not r["flux_conv"].any() and r["n_dep"].sum() == 0
    assert r["deposits"] > 10*NCELL and r["events"] > r["deposits"] and r["n_capped"] == 0 and r["n_clamped"] == 0


def test_the_start_is_the_ray_s_own_cell_and_the_stream_is_its_own():
    """a cell whose s0 is 0 ends its ray at once; another g-point and another tracer's counter word give other numbers"""
    sc = HS.general(np.float64, top_at_1=False)
    B0, s0 = H.reference(sc, 1)
    assert B0.shape == s0.shape == (NCELL,) and np.all(s0 > 0)
    whole = H.trace_counts_heating(sc, 1, 0, 2*NCELL)
    assert whole["counts"].shape == (NCELL,) and whole["counts"].dtype == np.int64 and (whole["counts"] < 0).any() and (whole["counts"] > 0).any()
    # cells that absorb nothing: tau (1 - ssa) = 0 with ssa = 1 and no cloud
    clear = HS.general(np.float64, top_at_1=False, cloud=False)
    clear.medium.ssa = np.ones_like(clear.medium.ssa)
    dead = H.trace_counts_heating(clear, 1, 0, 2*NCELL)
    assert dead["events"] == 0 and dead["deposits"] == 0 and not dead["counts"].any()
    assert not np.array_equal(H.trace_counts_heating(sc, 0, 0, 2*NCELL)["counts"], whole["counts"])


def test_ranges_add_up_and_the_cap_is_counted():
    sc = HS.general(np.float64)
    n = 4*NCELL
    whole = H.trace_counts_heating(sc, 3, 0, n)
    # disjoint ranges, cut inside a pass over the cells
    cuts = (0, NCELL + 7, 3*NCELL - 1, n)
    parts = [H.trace_counts_heating(sc, 3, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    for k in ("counts", "n_dep"):
        assert np.array_equal(sum(p[k] for p in parts), whole[k]), k
    assert sum(p["events"] for p in parts) == whole["events"] and whole["n_capped"] == 0 and whole["counts"].any()
    split = H.trace_counts_heating(sc, 3, 0, n, ranges=4)
    assert np.array_equal(split["counts"].sum(axis=0), whole["counts"])
    assert np.array_equal(split["counts"][1], H.trace_counts_heating(sc, 3, NCELL, NCELL)["counts"])
    # a ray that the cap drops keeps what it has deposited
    capped = H.trace_counts_heating(sc, 3, 0, n, max_events=2)
    assert 0 < capped["n_capped"] <= n and capped["events"] <= 2*n and capped["counts"].any()


@pytest.mark.parametrize("cloud", [True, False])
def test_unit_weights_give_the_integer_sum_over_the_g_points(cloud):
    sc = HS.general(np.float64, cloud=cloud)
    m = np.array([2, 1, 0, 3, 1])
    ray_end, _, _ = H.ray_list(sc, m)
    assert ray_end[HS.EMPTY] == ray_end[HS.EMPTY + 1] and ray_end[-1] == m.sum()*NCELL
    got = H.trace_counts_spectral(sc, ray_end, np.ones(HS.NGPT), 0, int(ray_end[-1]))
    want = sum(H.trace_counts_heating(sc, g, 0, int(m[g])*NCELL)["counts"] for g in range(HS.NGPT) if m[g] > 0)
    assert np.array_equal(got["counts"], want) and want.any()
    # ranges of the list add up, cut inside a g-point and beside the empty range
    w0 = H.ray_list(sc, m)[1]
    whole = H.trace_counts_spectral(sc, ray_end, w0, 0, int(ray_end[-1]))
    cuts = (0, int(ray_end[1]) - 5, int(ray_end[HS.EMPTY]), int(ray_end[-1]))
    parts = [H.trace_counts_spectral(sc, ray_end, w0, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(whole["counts"], sum(p["counts"] for p in parts))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_render_is_one_conversion_of_the_summed_counts(dtype):
    sc = HS.general(dtype, cloud=False)
    m = np.array([2, 1, 0, 1, 1])
    r = H.render(sc, m)
    assert r["flux_conv"].shape == (NCELL,) and r["flux_conv"].dtype == np.dtype(dtype)
    assert np.allclose(r["flux_conv"], float(r["U"])*r["counts"].astype(np.float64)*2.0**-32, rtol=4*np.finfo(dtype).eps)
    equal = H.ray_list(sc, np.full(HS.NGPT, 7))
    assert np.array_equal(equal[1], np.ones(HS.NGPT, dtype=dtype)) and equal[2] == np.dtype(dtype).type(1.)/np.dtype(dtype).type(7.)


# ---- H1: the slab against truth

def slab_ray_variance(sc, samples=1 << 16, seed=77):
    """Plain numpy, no restatement: (mean, variance) (ngpt, nz) of the one deposit of a ray of the slab. The ray starts at a uniform
    height of its layer with mu = 1 - 2u and ends where its free path -log u, in vertical optical depth |mu| times it, runs out: in a
    layer (it deposits (B_l - B0) s0: the gas only absorbs and k_null = k_ext), at the black surface or through the top."""
    rng = np.random.default_rng(seed)
    tau = sc.tau.astype(np.float64)[:, :, 0]
    B = sc.lay_src.astype(np.float64)[:, :, 0]
    ngpt, nz = tau.shape
    mean, var = np.zeros((ngpt, nz)), np.zeros((ngpt, nz))
    for g in range(ngpt):
        edges = np.concatenate([[0.0], np.cumsum(tau[g])])          # the vertical optical depth of the levels, from the surface
        for k in range(nz):
            t0 = edges[k] + rng.uniform(size=samples)*tau[g, k]
            mu = 1.0 - 2.0*rng.uniform(size=samples)
            t1 = t0 + mu*(-np.log(rng.uniform(size=samples)))
            lay = np.clip(np.searchsorted(edges, t1, side="right") - 1, 0, nz - 1)
            S = np.where(t1 <= 0.0, float(sc.sfc_src[g, 0]), np.where(t1 >= edges[-1], float(sc.top_radiance[g]), B[g, lay]))
            d = (S - B[g, k])*(4.0*math.pi*tau[g, k])
            mean[g, k], var[g, k] = d.mean(), d.var()
    return mean, var


def test_the_slab_s_truth_and_its_ray_budget():
    """256 and 512 nodes agree; the plain Monte Carlo of the estimator agrees with the truth; and SLAB_RAYS rays per cell, g-point and
    range hold the standard error of a cell below 2 % of the largest layer value"""
    sc = HS.slab(np.float64)
    tau = sc.tau[:, :, 0]
    assert tau.min() == 0.01 and tau.max() == 3.0 and sc.cloud is None and np.all(sc.sfc_emis == 1) and np.all(sc.top_radiance[list(HS.ACTIVE)] > 0)
    truth = HS.slab_truth(sc)
    assert np.max(np.abs(truth - HS.slab_truth(sc, 512))) <= 1e-13*np.abs(truth).max()
    assert not truth[HS.EMPTY].any() and np.all(np.ptp(sc.lay_src[0, :, 0]) > 0)
    samples = 1 << 16
    mean, var = slab_ray_variance(sc, samples)
    dev = np.abs(mean - truth)/np.sqrt(np.maximum(var, 1e-300)/samples)
    assert np.all(dev[list(HS.ACTIVE)] <= 5), float(dev.max())
    broadband = truth.sum(axis=0)
    se = np.sqrt(var.sum(axis=0)/(HS.RANGES*HS.SLAB_RAYS))
    print(f"heating slab: layer values {np.round(broadband, 3)} W m-2, predicted standard error of a cell {np.round(se, 3)}: "
          f"{100*float(se.max()/np.abs(broadband).max()):.2f} % of the largest")
    assert se.max() < 0.02*np.abs(broadband).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_slab_s_restatement_stays_inside_five_standard_errors(dtype):
    """What test_gpu_raytracer_heating.py asks of the device with SLAB_RAYS rays, asked of the restatement with 64 per cell, g-point
    and range: every cell, and every layer mean, within 5 standard errors (of 16 disjoint ranges) of the truth; every ray deposits once"""
    sc = HS.slab(dtype)
    R = 64
    parts = np.zeros((HS.RANGES, NCELL), dtype=np.int64)
    for g in range(HS.NGPT):
        c = H.trace_counts_heating(sc, g, 0, HS.RANGES*R*NCELL, ranges=HS.RANGES)
        assert c["n_capped"] == 0 and c["n_clamped"] == 0 and c["deposits"] == HS.RANGES*R*NCELL
        parts += c["counts"]
    truth = HS.slab_truth(sc).sum(axis=0)
    mean, se = TS.standard_error(parts, R)
    dev_cell = np.abs(mean.reshape(sc.nz, sc.ncol) - truth[:, None]) / se.reshape(sc.nz, sc.ncol)
    lay_mean, lay_se = TS.standard_error(parts.reshape(HS.RANGES, sc.nz, sc.ncol).sum(axis=2), R*sc.ncol)
    dev_lay = np.abs(lay_mean - truth)/lay_se
    print(f"heating slab restatement {np.dtype(dtype).name}: worst deviation {float(dev_cell.max()):.2f} standard errors per cell, "
          f"{float(dev_lay.max()):.2f} of a layer mean (bound 5)")
    assert np.all(se > 0) and np.all(dev_cell <= 5) and np.all(dev_lay <= 5)


def test_the_restatement_closes_the_energy_budget_in_3d():
    """H2 of test_gpu_raytracer_heating.py on the restatement with 16 rays per cell, pixel, g-point and range: the flux convergence
    summed over the cells against the net flux through the boundaries from the thermal tracer's two flux sensors"""
    import raytracer_thermal_ref as T
    from rte_rrtmgp_cpp_amd import camera as C
    sc = HS.closure_scene(np.float64)
    R, ncell = 16, sc.ncol*sc.nz
    parts = np.zeros((HS.RANGES, ncell), dtype=np.int64)
    rad = {True: np.zeros((HS.RANGES, sc.ncol)), False: np.zeros((HS.RANGES, sc.ncol))}
    for g in range(sc.tau.shape[0]):
        c = H.trace_counts_heating(sc, g, 0, HS.RANGES*R*ncell, ranges=HS.RANGES)
        assert c["n_capped"] == 0 and c["n_clamped"] == 0
        parts += c["counts"]
        for up in rad:
            t = T.trace_counts_thermal(sc, C.flux_sensor(sc.nx, sc.ny, up=up), g, 0, HS.RANGES*R*sc.ncol, ranges=HS.RANGES)
            rad[up] += t["counts"].astype(np.float64)*2.0**-32/R
    conv = parts.sum(axis=1)*2.0**-32/R/sc.ncol
    net = HS.boundary_net(sc, rad[True], rad[False])
    se = math.hypot(conv.std(ddof=1), net.std(ddof=1))/math.sqrt(HS.RANGES)
    print(f"heating closure restatement: convergence {conv.mean():.3f}, boundary net {net.mean():.3f} W m-2, 5 standard errors {5*se:.3f}")
    assert abs(conv.mean() - net.mean()) <= 5*se


def digests():
    """counts digests of three scenes, every g-point: 8 rays per cell"""
    scenes = {"general": HS.general, "general upward": lambda dt: HS.general(dt, top_at_1=False, gas_scatters=False), "slab": HS.slab}
    out = {}
    for name, scene in scenes.items():
        for dt in (np.float64, np.float32):
            sc = scene(dt)
            r = [H.trace_counts_heating(sc, g, 0, 8*NCELL) for g in range(HS.NGPT)]
            out[f"{name} {np.dtype(dt).name}"] = dict(
                counts=hashlib.sha256(np.stack([c["counts"] for c in r]).astype("<i8").tobytes()).hexdigest(),
                events=[int(c["events"]) for c in r], deposits=[int(c["deposits"]) for c in r])
    return out


def test_digests_are_the_recorded_ones():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert digests() == want


if __name__ == "__main__":          # writes the record
    with open(GOLDEN, "w") as f:
        json.dump(digests(), f, indent=1, sort_keys=True)
        f.write("\n")
