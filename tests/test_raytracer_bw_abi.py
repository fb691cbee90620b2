"""CPU tests of the backward ray tracer entries (rrx_rt_bw_trace_counts, rrx_raytracer_bw): declared in both precisions with the
stream last and exported, their argument checks answer without a GPU and name the argument, and the host libraries export
Raytracer_bw_gpu::trace_rays_bw and rrx_cxx_trace_rays_bw."""
import os
import re
import subprocess

import numpy as np
import pytest

import abi

ROOT = abi.ROOT
HOSTLIBS = [os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", n) for n in ("librte_rrtmgp_hip.so", "librte_rrtmgp_hip_sp.so")]
ENTRIES = ("rrx_rt_bw_trace_counts", "rrx_raytracer_bw")


def test_header_declares_the_entries_in_both_precisions_with_the_stream_last():
    for name in ENTRIES:
        assert abi.declares(name), name
        for sfx, F in zip(abi.SFXS, ("double", "float")):
            params = abi.params(name, sfx)
            assert params[-1] == ("void*", "stream"), name
            for piece in (("int", "sensor_type"), ("int", "npx"), ("int", "npy"), (F, "fov"), (f"const {F}*", "sensor"),
                          ("unsigned long long", "seed"), ("int", "max_events"), ("unsigned long long*", "n_capped"),
                          ("unsigned long long*", "n_clamped")):
                assert piece in params, (name, piece)
    for sfx, F in zip(abi.SFXS, ("double", "float")):
        params = abi.params("rrx_rt_bw_trace_counts", sfx)
        for piece in ((f"const {F}*", "k_null"), ("long long", "ray0"), ("long long", "nrays"), ("unsigned long long*", "counts")):
            assert piece in params, piece


def test_library_exports_the_entries():
    lib = abi.lib()
    for name in ENTRIES:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx


SCENE = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, igpt=1, top_at_1=0, dx=100., dy=100., dz=50., mu0=0.5, azimuth=0.3, knx=1, kny=2, knz=1,
             sensor_type=0, npx=3, npy=2, fov=1.0, seed=7, ray0=0, nrays=12, rays_per_pixel=2, max_events=100)
SENSOR = (50., 60., 20., 0.5, 0., 0., 0., 0.5, 0., 0., 0., -1.)


def _call(lib, entry, sfx, null=(), sensor_numbers=SENSOR, **over):
    """The entry on memory that the device never touches (the checks come before any HIP call); the sensor's 12 numbers and inc_dir
    of rrx_raytracer_bw are host arrays. Returns the status."""
    F = np.float64 if sfx == "_f64" else np.float32
    scene = dict(SCENE, sensor=np.array(sensor_numbers, dtype=F), inc_dir=np.array([1., 2.], dtype=F))
    scene = {k: v for k, v in scene.items() if k in abi.names(entry)}
    return abi.call(lib, entry, sfx, null=null, **{**scene, **over})[0]


NEEDED = {"rrx_rt_bw_trace_counts": ("tau", "ssa", "sfc_albedo", "k_null", "sensor", "counts", "n_capped", "n_clamped"),
          "rrx_raytracer_bw": ("tau", "ssa", "sfc_albedo", "inc_dir", "sensor", "radiance", "n_capped", "n_clamped")}
EXTENTS = {"rrx_rt_bw_trace_counts": ("nx", "ny", "nz", "ngpt", "npx", "npy", "nrays"),
           "rrx_raytracer_bw": ("nx", "ny", "nz", "ngpt", "npx", "npy", "rays_per_pixel")}


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_null_that_is_needed_is_refused_without_a_gpu(entry, sfx):
    lib = abi.lib()
    for name in NEEDED[entry]:
        assert _call(lib, entry, sfx, null=(name,)) != 0, name
        msg = abi.last_error(lib)
        assert entry + sfx in msg and name + " is NULL" in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_extents_return_zero_without_a_launch_and_negative_ones_are_refused(entry, sfx):
    lib = abi.lib()
    for d in EXTENTS[entry]:
        assert _call(lib, entry, sfx, **{d: 0}) == 0, d
        assert _call(lib, entry, sfx, null=("tau", "counts", "radiance"), **{d: 0}) == 0, d
        assert _call(lib, entry, sfx, **{d: -1}) != 0, d
        msg = abi.last_error(lib)
        assert entry + sfx in msg and d + " is negative" in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_scene_and_sensor_checks_name_the_argument(entry, sfx):
    lib = abi.lib()
    look = (50., 60., 20., 0.5, 0., 0., 0., 0.5, 0.)
    for over, word in (({"mu0": 0.}, "mu0"), ({"mu0": -0.2}, "mu0"), ({"dz": 0.}, "dz"), ({"knx": 3}, "knx"), ({"knz": 0}, "knz"),
                       ({"null": ("cld_ssa",)}, "cld_tau, cld_ssa, cld_g"), ({"null": ("band_lims_gpt",)}, "band_lims_gpt"),
                       ({"max_events": 0}, "max_events"),
                       ({"sensor_type": 4}, "sensor_type"), ({"sensor_type": -1}, "sensor_type"),
                       ({"sensor_numbers": look + (0., 0., 0.)}, "e_d"),
                       ({"sensor_numbers": (50., 60., -1.) + look[3:] + (0., 0., -1.)}, "position"),
                       ({"sensor_numbers": look + (0., float("nan"), -1.)}, "not finite"),
                       ({"sensor_type": 1, "fov": 0.}, "fov"), ({"sensor_type": 1, "fov": 7.}, "fov"),
                       ({"sensor_type": 2, "sensor_numbers": look + (0., 0., 1.)}, "e_d"),
                       ({"sensor_type": 2, "sensor_numbers": look + (0., 0., -2.)}, "e_d"),
                       ({"sensor_type": 3, "sensor_numbers": look + (1., 0., 0.)}, "e_d.z")):
        assert _call(lib, entry, sfx, **over) != 0, over
        msg = abi.last_error(lib)
        assert entry + sfx in msg and word in msg, msg
    # a clear sky: the whole triple NULL is accepted as far as the argument checks go (no rays: no launch)
    none = {"nrays": 0} if entry == "rrx_rt_bw_trace_counts" else {"rays_per_pixel": 0}
    assert _call(lib, entry, sfx, null=("cld_tau", "cld_ssa", "cld_g", "band_lims_gpt"), **none) == 0
    if entry == "rrx_rt_bw_trace_counts":
        assert _call(lib, entry, sfx, igpt=2) != 0 and "igpt" in abi.last_error(lib)
        assert _call(lib, entry, sfx, ray0=-1) != 0 and "ray0" in abi.last_error(lib)
    else:
        F = np.float64 if sfx == "_f64" else np.float32
        assert _call(lib, entry, sfx, inc_dir=np.array([1., -2.], dtype=F)) != 0 and "inc_dir" in abi.last_error(lib)


def test_host_libraries_export_the_backward_raytracer_class():
    text = open(os.path.join(ROOT, "include", "Raytracer_bw.h")).read()
    assert "class Raytracer_bw_gpu" in text and "trace_rays_bw(" in text
    assert "rrx_cxx_trace_rays_bw(" in open(os.path.join(ROOT, "include_test", "rrx_cxx_driver.h")).read()
    for hostlib in HOSTLIBS:
        if not os.path.exists(hostlib):
            pytest.fail(f"{hostlib} not built: run __graft_entry__.build()")
        syms = subprocess.run(["nm", "-DC", "--defined-only", hostlib], capture_output=True, text=True).stdout
        assert "Raytracer_bw_gpu::trace_rays_bw(" in syms and "rrx_cxx_trace_rays_bw" in syms, hostlib
