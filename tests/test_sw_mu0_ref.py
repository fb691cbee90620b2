"""CPU tests of the mu0-by-layer feature's reference and argument checks: the NumPy spherical-geometry correction of tests/sw_mu0_ref.py
has the properties of the formula, and pipeline.ResidentSolver refuses mu0_lay= / altitude= / ref_altitude= that do not fit, before it
touches a device."""
import types

import numpy as np
import pytest

import sw_mu0_ref
from rte_rrtmgp_cpp_amd import pipeline, sharding


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_equals_ref_mu_at_the_reference_altitude(dtype):
    rng = np.random.default_rng(3)
    ref_mu = rng.uniform(0.01, 1.0, 50).astype(dtype)
    ref_alt = rng.uniform(0., 3000., 50).astype(dtype)
    mu = sw_mu0_ref.spherical_mu0(ref_mu, np.repeat(ref_alt[None, :], 4, axis=0), ref_alt)
    assert mu.dtype == dtype and mu.shape == (4, 50)
    # 1 - (1 - m^2) and the square root each round once: a few ulp of 1 on m^2, i.e. eps / m^2 relative on m
    eps = np.finfo(dtype).eps
    assert np.all(np.abs(mu - ref_mu[None, :]) <= 2*eps / ref_mu[None, :])
    mu0 = sw_mu0_ref.spherical_mu0(ref_mu, np.zeros((4, 50), dtype=dtype))          # ref_alt = None is altitude 0
    assert np.array_equal(mu0, sw_mu0_ref.spherical_mu0(ref_mu, np.zeros((4, 50), dtype=dtype), np.zeros(50, dtype=dtype)))


def test_reference_rises_strictly_with_altitude():
    ref_mu = np.array([1e-3, 0.05, 0.3, 0.7, 0.99])
    alt = np.repeat(np.linspace(0., 80e3, 41)[:, None], ref_mu.size, axis=1)
    mu = sw_mu0_ref.spherical_mu0(ref_mu, alt)
    assert np.all(np.diff(mu, axis=0) > 0)
    assert np.all(mu <= 1.0) and np.all(mu[0] > 0)
    # the horizon: at 80 km a sun on the horizon at the ground stands sqrt(1 - (R/(R+z))^2) ~ 0.157 high
    assert abs(sw_mu0_ref.spherical_mu0(np.array([1e-12]), np.array([[80e3]]))[0, 0] - np.sqrt(1 - (6.37123e6/(6.37123e6 + 80e3))**2)) < 1e-9


def test_reference_overhead_sun_stays_overhead_and_dark_columns_pass_through():
    alt = np.repeat(np.linspace(0., 60e3, 7)[:, None], 4, axis=1)
    ref_mu = np.array([1.0, 0.0, -0.2, -1.0])
    mu = sw_mu0_ref.spherical_mu0(ref_mu, alt, np.zeros(4))
    assert np.all(mu[:, 0] == 1.0)
    assert np.array_equal(mu[:, 1:], np.broadcast_to(ref_mu[None, 1:], (7, 3)))
    # below the reference altitude the radicand may turn negative: clamped, not NaN
    low = sw_mu0_ref.spherical_mu0(np.array([1e-4]), np.array([[0.]]), np.array([5000.]))
    assert low[0, 0] == 0.0


def _atm(nlay=5, ncol=8):
    return types.SimpleNamespace(nlay=nlay, ncol=ncol)


def test_resident_solver_refuses_arguments_that_do_not_fit():
    atm = _atm()
    ok2, ok1 = np.full((5, 8), 100.), np.zeros(8)
    mk = lambda **kw: pipeline.ResidentSolver(None, None, None, atm, **kw)
    with pytest.raises(ValueError, match="give one"):
        mk(mu0_lay=np.full((5, 8), 0.5), altitude=ok2)
    with pytest.raises(ValueError, match="ref_altitude without altitude"):
        mk(ref_altitude=ok1)
    with pytest.raises(ValueError, match="ref_altitude without altitude"):
        mk(mu0_lay=np.full((5, 8), 0.5), ref_altitude=ok1)
    for bad in (np.zeros((8, 5)), np.zeros((5, 7)), np.zeros(8), np.zeros((1, 5, 8))):
        with pytest.raises(ValueError, match="mu0_lay .* is not"):
            mk(mu0_lay=bad + 0.5)
        with pytest.raises(ValueError, match="altitude .* is not"):
            mk(altitude=bad + 100.)
    for bad in (np.zeros(7), np.zeros((1, 8)), np.zeros((5, 8))):
        with pytest.raises(ValueError, match="ref_altitude .* is not"):
            mk(altitude=ok2, ref_altitude=bad)
    below = ok2.copy(); below[3, 2] = -1.0
    with pytest.raises(ValueError, match="below"):
        mk(altitude=below)
    ref = ok1 + 50.; ref[6] = 100.5
    with pytest.raises(ValueError, match="below"):
        mk(altitude=ok2, ref_altitude=ref)


def test_the_fields_travel_with_the_columns():
    for k, axis in (("mu0_lay", -1), ("altitude", -1), ("ref_altitude", 0)):
        assert pipeline.ResidentSolver._COLUMN_FIELDS[k] == axis and k in pipeline.ResidentSolver._SW_FIELDS
    alt = np.arange(3*10, dtype=np.float64).reshape(3, 10); ref = np.arange(10, dtype=np.float64)
    parts = [sharding.shard_sw_geometry(r, 3, altitude=alt, ref_altitude=ref) for r in range(3)]
    assert all(set(p) == {"altitude", "ref_altitude"} for p in parts)
    assert np.array_equal(np.concatenate([p["altitude"] for p in parts], axis=1), alt)
    assert np.array_equal(np.concatenate([p["ref_altitude"] for p in parts]), ref)
    assert [p["altitude"].shape[1] for p in parts] == [e - s for s, e in (sharding.column_range(r, 3, 10) for r in range(3))]
    assert set(sharding.shard_sw_geometry(1, 3, mu0_lay=alt)) == {"mu0_lay"} and sharding.shard_sw_geometry(0, 2) == {}
