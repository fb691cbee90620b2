"""CPU tests of the numpy restatement of the backward ray tracer (tests/raytracer_bw_ref.py) on the scenes of
raytracer_bw_scenes.py: S1 the Bernoulli surface, S2 the shadow in integers, S3 forward against backward, additivity over ray
ranges, the sensors' geometry and the camera helper. Bounds are derived (raytracer_bw_scenes), five standard deviations, fixed seeds."""
import math

import numpy as np
import pytest

import raytracer_ref as R
import raytracer_bw_ref as B
import raytracer_bw_scenes as S


@pytest.mark.parametrize("view", ["nadir", "slant"])
def test_s1_bernoulli_surface(view):
    sc = S.bernoulli(np.float64)
    sensor = S.bernoulli_sensors()[view]
    for g in range(2):
        c = B.trace_counts_bw(sc, sensor, g, 0, S.S1_RAYS*16)
        assert c["n_capped"] == 0 and c["n_clamped"] == 0
        S.check_bernoulli(sc, sensor, g, c["counts"], f"ref {view}")
        # every deposit is the same number: the count is a multiple of it up to one unit per deposit
        _, dep = S.bernoulli_expected(sc, sensor, g)
        assert np.all(np.abs(c["counts"].astype(np.float64) - c["n_dep"]*dep*S.ONE) <= c["n_dep"]*(1.0 + 1e-9*dep*S.ONE))


def test_s1_float32_runs_the_same_algorithm():
    sc = S.bernoulli(np.float32)
    sensor = S.bernoulli_sensors()["slant"]
    c = B.trace_counts_bw(sc, sensor, 0, 0, S.S1_RAYS*16)
    assert c["n_capped"] == 0
    S.check_bernoulli(sc, sensor, 0, c["counts"], "ref f32 slant")


@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("along", ["x", "y"])
def test_s2_shadow_in_integers(along, top_at_1):
    sc = S.shadow(np.float64, along, top_at_1)
    dark, full = S.shadow_classes(sc)
    assert dark.sum() == 6 + 4 and full.sum() == sc.ncol - 6 - 8
    rays = 16
    c = B.trace_counts_bw(sc, B.orthographic(sc.nx, sc.ny, (0., 0., -1.)), 0, 0, rays*sc.ncol)
    assert c["n_capped"] == 0 and c["n_clamped"] == 0
    assert np.all(c["counts"][dark] == 0), c["counts"][dark]
    assert np.all(c["counts"][full] == S.shadow_full_count(sc, rays)), c["counts"][full] / S.ONE
    edge = ~dark & ~full
    assert np.all(c["counts"][edge] <= S.shadow_full_count(sc, rays))


@pytest.fixture(scope="module")
def forward_general():
    sc = S.general_direct(np.float64)
    return sc, [R.trace_counts(sc, g, 0, S.S3_PHOTONS*sc.ncol) for g in range(2)]


@pytest.mark.parametrize("name", ["sfc_dn_dif", "tod_up"])
def test_s3_forward_against_backward(name, forward_general):
    sc, fwd = forward_general
    sensor = S.flux_sensors(sc)[name]
    per_range = (S.S3_RAYS//S.S3_RANGES)*sc.ncol
    worst = 0.0
    for g in range(2):
        assert fwd[g]["n_capped"] == 0
        c = B.trace_counts_bw(sc, sensor, g, 0, S.S3_RANGES*per_range, ranges=S.S3_RANGES)
        assert c["n_capped"] == 0 and c["n_clamped"] == 0
        if g == 0:          # a range tallied apart is the range traced alone
            assert np.array_equal(B.trace_counts_bw(sc, sensor, g, 3*per_range, per_range)["counts"], c["counts"][3])
        worst = max(worst, S.compare_forward_backward(sc, g, name, fwd[g][name], c["counts"], "ref"))
    print(f"raytracer_bw S3 ref {name}: worst {worst:.2f} combined sigma")


def test_counts_are_additive_over_ray_ranges_and_the_cap_is_counted():
    sc = S.general_direct(np.float64)
    sensor = B.Sensor(0, 6, 4, 0.0, (330., 250., 170.), (0.5, 0., 0.), (0., 0.4, 0.1), (0.2, 0.3, -0.9))
    n = 16*24
    whole = B.trace_counts_bw(sc, sensor, 1, 0, n)
    a, b = B.trace_counts_bw(sc, sensor, 1, 0, n//3), B.trace_counts_bw(sc, sensor, 1, n//3, n - n//3)
    assert np.array_equal(whole["counts"], a["counts"] + b["counts"]) and np.array_equal(whole["n_dep"], a["n_dep"] + b["n_dep"])
    assert whole["events"] == a["events"] + b["events"] and whole["walk_cells"] == a["walk_cells"] + b["walk_cells"]
    assert whole["counts"].all() and whole["n_capped"] == 0 and whole["n_clamped"] == 0
    # the walk to the sun is bounded by construction
    assert whole["walk_cells"] <= whole["n_dep"].sum()*B.max_walk(sc)
    capped = B.trace_counts_bw(sc, sensor, 1, 0, n, max_events=1)
    assert 0 < capped["n_capped"] <= n


def test_a_sensor_that_looks_away_from_the_domain_sees_nothing():
    sc = S.general_direct(np.float64)
    z_top = sc.nz*sc.dz
    up = B.Sensor(0, 2, 2, 0.0, (100., 100., z_top + 50.), (0.1, 0., 0.), (0., 0.1, 0.), (0., 0., 1.))
    c = B.trace_counts_bw(sc, up, 0, 0, 64)
    assert not c["counts"].any() and c["events"] == 0 and c["n_capped"] == 0
    # from above the top, looking down: moved along the ray to the top, the same counts as the orthographic nadir view's geometry allows
    down = B.Sensor(0, 2, 2, 0.0, (100., 100., z_top + 50.), (0.1, 0., 0.), (0., 0.1, 0.), (0., 0., -1.))
    assert B.trace_counts_bw(sc, down, 0, 0, 64)["counts"].any()


def test_camera_helper_builds_orthonormal_axes_from_the_geometry():
    from rte_rrtmgp_cpp_amd import camera as C
    for yaw, pitch, roll in ((0., 0., 0.), (0.7, -0.4, 0.3), (2.5, 1.1, -1.2), (-1.0, -0.5*math.pi, 0.)):
        r, u, d = C.view_axes(yaw, pitch, roll)
        m = np.stack([r, u, d])
        assert np.allclose(m @ m.T, np.eye(3), atol=1e-14)
        assert np.allclose(np.cross(r, u), -d, atol=1e-14)          # right x up = towards the viewer
    r, u, d = C.view_axes(0., 0.)
    assert np.allclose(d, (1, 0, 0)) and np.allclose(r, (0, -1, 0)) and np.allclose(u, (0, 0, 1))
    assert np.allclose(C.view_axes(0.5*math.pi, 0.)[2], (0, 1, 0), atol=1e-15)
    assert np.allclose(C.view_axes(0.3, -0.5*math.pi)[2], (0, 0, -1), atol=1e-15)
    cam = C.perspective(8, 4, (1., 2., 3.), 0.3, -0.2, fov=math.radians(90.))
    assert cam.type == 0 and cam.npix == 32 and cam.numbers().shape == (12,)
    assert math.isclose(np.linalg.norm(cam.e_w), 1.0) and math.isclose(np.linalg.norm(cam.e_h), 0.5)       # tan(45 deg), aspect 2
    assert C.orthographic(4, 4).e_d == (0., 0., -1.) or np.allclose(C.orthographic(4, 4).e_d, (0, 0, -1), atol=1e-15)
    assert C.flux_sensor(2, 2, up=False).e_d[2] == -1.0 and C.fisheye(2, 2, (0, 0, 0)).fov == math.pi
    with pytest.raises(ValueError):
        C.orthographic(4, 4, pitch=0.2)
