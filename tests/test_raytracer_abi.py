"""CPU tests of the ray tracer entries (rrx_rt_k_null, rrx_rt_trace_counts, rrx_rt_counts_to_flux, rrx_raytracer_sw): declared in
both precisions with the stream last and exported, their argument checks answer without a GPU, and the host library exports
Raytracer_gpu::trace_rays."""
import os
import re
import subprocess

import numpy as np
import pytest

import abi

ROOT = abi.ROOT
HOSTLIBS = [os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", n) for n in ("librte_rrtmgp_hip.so", "librte_rrtmgp_hip_sp.so")]
ENTRIES = ("rrx_rt_k_null", "rrx_rt_trace_counts", "rrx_rt_counts_to_flux", "rrx_raytracer_sw")


def test_header_declares_the_entries_in_both_precisions_with_the_stream_last():
    text = abi.header_text()
    for name in ENTRIES:
        assert abi.declares(name), name
        for sfx in abi.SFXS:
            assert abi.params(name, sfx)[-1] == ("void*", "stream"), name
    for sfx in abi.SFXS:
        params = abi.params("rrx_rt_trace_counts", sfx)
        for piece in (("unsigned long long", "seed"), ("long long", "photon0"), ("long long", "nphotons"), ("int", "max_events"),
                      ("unsigned long long*", "n_capped")):
            assert piece in params, piece
    assert "RRX_DECLARE(double, _f64)" in text and "RRX_DECLARE(float, _f32)" in text


def test_library_exports_the_entries():
    lib = abi.lib()
    for name in ENTRIES:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx


SCENE = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, igpt=1, top_at_1=0, independent_column=0, dx=100., dy=100., dz=50., mu0=0.5, azimuth=0.3,
             inc_dir=1., inc_dif=0., knx=1, kny=2, knz=1, seed=7, photon0=0, nphotons=8, photons_per_pixel=2, max_events=100, n=8, scale=1.)


def _call(lib, entry, sfx, null=(), **over):
    """The entry on host memory that is never touched (the checks come before any HIP call); inc_dir / inc_dif of rrx_raytracer_sw
    are host arrays of ngpt numbers. Returns the status."""
    scene = dict(SCENE)
    if entry == "rrx_raytracer_sw":
        F = np.float64 if sfx == "_f64" else np.float32
        scene.update(inc_dir=np.array([1., 2.], dtype=F), inc_dif=np.zeros(2, dtype=F))
    scene = {k: v for k, v in scene.items() if k in abi.names(entry)}
    return abi.call(lib, entry, sfx, null=null, **{**scene, **over})[0]


OUTS = ("sfc_dn_dir", "sfc_dn_dif", "sfc_up", "tod_up", "abs_dir", "abs_dif", "n_capped")
NEEDED = {"rrx_rt_k_null": ("tau", "k_null"),
          "rrx_rt_trace_counts": ("tau", "ssa", "sfc_albedo", "k_null") + OUTS,
          "rrx_rt_counts_to_flux": ("counts", "out"),
          "rrx_raytracer_sw": ("tau", "ssa", "sfc_albedo", "inc_dir", "inc_dif") + OUTS}
EXTENTS = {"rrx_rt_k_null": ("nx", "ny", "nz", "ngpt"),
           "rrx_rt_trace_counts": ("nx", "ny", "nz", "ngpt", "nphotons"),
           "rrx_rt_counts_to_flux": ("n",),
           "rrx_raytracer_sw": ("nx", "ny", "nz", "ngpt", "photons_per_pixel")}


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
        assert _call(lib, entry, sfx, null=("tau", "counts", "sfc_up"), **{d: 0}) == 0, d
        assert _call(lib, entry, sfx, **{d: -1}) != 0, d
        msg = abi.last_error(lib)
        assert entry + sfx in msg and d + " is negative" in msg, msg


@pytest.mark.parametrize("sfx", ["_f64", "_f32"])
@pytest.mark.parametrize("entry", ["rrx_rt_trace_counts", "rrx_raytracer_sw"])
def test_scene_checks_name_the_argument(entry, sfx):
    lib = abi.lib()
    for over, word in (({"mu0": 0.}, "mu0"), ({"mu0": -0.2}, "mu0"), ({"dz": 0.}, "dz"), ({"knx": 3}, "knx"), ({"knz": 0}, "knz"),
                       ({"null": ("cld_ssa",)}, "cld_tau, cld_ssa, cld_g"), ({"null": ("band_lims_gpt",)}, "band_lims_gpt"),
                       ({"max_events": 0}, "max_events")):
        assert _call(lib, entry, sfx, **over) != 0, over
        msg = abi.last_error(lib)
        assert entry + sfx in msg and word in msg, msg
    # a clear sky: the whole triple NULL is accepted as far as the argument checks go (nphotons = 0: no launch)
    none = {"nphotons": 0} if entry == "rrx_rt_trace_counts" else {"photons_per_pixel": 0}
    assert _call(lib, entry, sfx, null=("cld_tau", "cld_ssa", "cld_g", "band_lims_gpt"), **none) == 0
    if entry == "rrx_rt_trace_counts":
        assert _call(lib, entry, sfx, igpt=2) != 0 and "igpt" in abi.last_error(lib)
        assert _call(lib, entry, sfx, inc_dir=0.) != 0 and "inc_dir" in abi.last_error(lib)


def test_host_libraries_export_the_raytracer_class():
    text = open(os.path.join(ROOT, "include", "Raytracer.h")).read()
    assert "class Raytracer_gpu" in text and "trace_rays(" in text
    for hostlib in HOSTLIBS:
        if not os.path.exists(hostlib):
            pytest.fail(f"{hostlib} not built: run __graft_entry__.build()")
        syms = subprocess.run(["nm", "-DC", "--defined-only", hostlib], capture_output=True, text=True).stdout
        assert "Raytracer_gpu::trace_rays(" in syms, hostlib
