"""CPU tests of the numpy restatement of the thermal ray tracer (tests/raytracer_thermal_ref.py), which the GPU tests
compare the kernel with ray for ray: the two physics statements that the estimator has to meet (Schwarzschild's solution of a clear
column, the black-body cavity), additivity over ray ranges, the cap, and a record of counts digests (tests/golden/
thermal_ref_digests.json) that holds the restatement, and the steps of raytracer_ref that it imports, through later refactors.

Bounds: 5 standard errors of 16 disjoint ray ranges (the estimate is a mean of independent rays; fixed seeds, so a run that passes
once passes always), plus for the Schwarzschild case the reference's own standard error of the reflected term."""
import hashlib
import json
import os

import numpy as np
import pytest

import raytracer_thermal_ref as T
import thermal_scenes as TS
from rte_rrtmgp_cpp_amd import camera as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thermal_ref_digests.json")


@pytest.mark.parametrize("g", [0, 1])
def test_t1_schwarzschild_with_the_reflected_term(g):
    sc = TS.clear_columns(np.float64)
    sensor = C.orthographic(sc.nx, sc.ny)
    want, se_want = TS.schwarzschild_expected(sc, g)
    r = T.trace_counts_thermal(sc, sensor, g, 0, TS.T1_RAYS*sensor.npix, ranges=TS.RANGES)
    assert r["n_capped"] == 0 and r["n_clamped"] == 0 and r["cloud_scatterings"] == 0
    got, se = TS.standard_error(r["counts"], TS.T1_RAYS//TS.RANGES)
    bound = 5.0*np.sqrt(se*se + se_want*se_want)
    print(f"thermal ref T1 g={g}: worst difference/bound {float(np.max(np.abs(got - want)/bound)):.2f}, radiance {want.min():.3f} .. "
          f"{want.max():.3f}, standard error up to {float(np.max(se/want)):.4f} of it, the reference's up to {float(np.max(se_want/want)):.1e}")
    assert np.all(se < 0.02*want) and np.all(se_want < 0.1*se)          # the bound is not vacuous, and it is the tracer's own
    assert np.all(np.abs(got - want) <= bound)


@pytest.mark.parametrize("name", list(TS.cavity_sensors()))
def test_t2_cavity_and_the_ray_count_of_the_gpu_test(name):
    """every pixel of every sensor sees S_g, and CAVITY_RAYS rays per pixel put the standard error below 1 % of it"""
    sc = TS.cavity(np.float64)
    sensor = TS.cavity_sensors()[name]
    for g in range(2):
        r = T.trace_counts_thermal(sc, sensor, g, 0, TS.CAVITY_RAYS*sensor.npix, ranges=TS.RANGES)
        assert r["n_capped"] == 0 and r["n_clamped"] == 0 and r["cloud_scatterings"] > 0
        got, se = TS.standard_error(r["counts"], TS.CAVITY_RAYS//TS.RANGES)
        print(f"thermal ref T2 {name} g={g}: radiance/S_g {float(got.min()/TS.S_G[g]):.4f} .. {float(got.max()/TS.S_G[g]):.4f}, standard error "
              f"up to {float(se.max()/TS.S_G[g]):.4f} S_g, worst difference {float(np.max(np.abs(got - TS.S_G[g])/se)):.2f} of it, "
              f"{r['events']/(TS.CAVITY_RAYS*sensor.npix):.1f} events per ray")
        assert np.all(se > 0) and np.all(se < 0.01*TS.S_G[g])
        assert np.all(np.abs(got - TS.S_G[g]) <= 5.0*se)


def test_counts_are_additive_over_ranges_and_the_cap_is_counted():
    sc = TS.general_lw(np.float64)
    sensor = TS.sensors(6, 4)["perspective"]
    n = 32*sensor.npix
    whole = T.trace_counts_thermal(sc, sensor, 1, 0, n)
    split = T.trace_counts_thermal(sc, sensor, 1, 0, n, ranges=4)
    parts = [T.trace_counts_thermal(sc, sensor, 1, q*(n//4), n//4) for q in range(4)]
    for k in ("counts", "n_dep"):
        assert np.array_equal(split[k].sum(axis=0, dtype=whole[k].dtype), whole[k]), k
        assert all(np.array_equal(split[k][q], parts[q][k]) for q in range(4)), k
    assert sum(p["events"] for p in parts) == whole["events"] and whole["n_capped"] == 0 and whole["counts"].all()
    capped = T.trace_counts_thermal(sc, sensor, 1, 0, n, max_events=1)
    assert 0 < capped["n_capped"] <= n and capped["events"] <= n
    # another g-point, another stream
    assert not np.array_equal(T.trace_counts_thermal(sc, sensor, 0, 0, n)["counts"], whole["counts"])


def digests():
    """counts digests of three scene / sensor pairs, both g-points: 32 rays per pixel"""
    pairs = {"general_lw perspective": (TS.general_lw, TS.sensors(6, 4)["perspective"]),
             "cavity fisheye": (TS.cavity, TS.sensors(6, 4)["fisheye"]),
             "clear_columns flux_down": (TS.clear_columns, C.flux_sensor(6, 4, up=False))}
    out = {}
    for name, (scene, sensor) in pairs.items():
        for dt in (np.float64, np.float32):
            sc = scene(dt)
            r = [T.trace_counts_thermal(sc, sensor, g, 0, 32*sensor.npix) for g in range(2)]
            out[f"{name} {np.dtype(dt).name}"] = dict(
                counts=hashlib.sha256(np.stack([c["counts"] for c in r]).astype("<u8").tobytes()).hexdigest(),
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
