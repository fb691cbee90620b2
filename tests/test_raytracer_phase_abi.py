"""CPU tests of the phase-table entries (rrx_rt_phase_tables / _sample / _eval and the four rrx_*_phase twins of the tracer
entries): declared in both precisions with the stream last and exported; the twins' argument lists are those of the existing
entries followed by the table; every refusal answers without a GPU and names the argument; zero extents return 0."""
import numpy as np
import pytest

import abi

TWINS = {"rrx_rt_trace_counts_phase": "rrx_rt_trace_counts", "rrx_raytracer_sw_phase": "rrx_raytracer_sw",
         "rrx_rt_bw_trace_counts_phase": "rrx_rt_bw_trace_counts", "rrx_raytracer_bw_phase": "rrx_raytracer_bw"}
ARRAYS = ("rrx_rt_phase_sample", "rrx_rt_phase_eval")
TABLE = ("mu", "phase", "cdf", "cld_re")
SCENE = dict(nx=2, ny=2, nz=2, ngpt=2, nbnd=1, igpt=1, top_at_1=0, independent_column=0, dx=100., dy=100., dz=50., mu0=0.5, azimuth=0.3,
             knx=1, kny=2, knz=1, sensor_type=0, npx=3, npy=2, fov=1.0, seed=7, ray0=0, nrays=12, rays_per_pixel=2, photon0=0, nphotons=8,
             photons_per_pixel=2, max_events=100, nmu=5, nre=3, re0=4.0, dre=3.0)
SENSOR = (50., 60., 20., 0.5, 0., 0., 0., 0.5, 0., 0., 0., -1.)
EXTENTS = {"rrx_rt_trace_counts_phase": ("nx", "ny", "nz", "ngpt", "nphotons"),
           "rrx_raytracer_sw_phase": ("nx", "ny", "nz", "ngpt", "photons_per_pixel"),
           "rrx_rt_bw_trace_counts_phase": ("nx", "ny", "nz", "ngpt", "npx", "npy", "nrays"),
           "rrx_raytracer_bw_phase": ("nx", "ny", "nz", "ngpt", "npx", "npy", "rays_per_pixel")}


def _call(lib, entry, sfx, null=(), **over):
    """The entry on memory that the device never touches (the checks come before any HIP call). Returns the status."""
    F = np.float64 if sfx == "_f64" else np.float32
    scene = dict(SCENE, sensor=np.array(SENSOR, dtype=F))
    if entry.startswith("rrx_raytracer"):
        scene.update(inc_dir=np.array([1., 2.], dtype=F), inc_dif=np.array([0., 0.], dtype=F))
    scene = {k: v for k, v in scene.items() if k in abi.names(entry)}
    return abi.call(lib, entry, sfx, null=null, **{**scene, **over})[0]


def test_header_declares_the_entries_and_the_twins_extend_the_existing_lists():
    for name in list(TWINS) + list(ARRAYS) + ["rrx_rt_phase_tables"]:
        assert abi.declares(name), name
    for sfx, F in zip(abi.SFXS, ("double", "float")):
        tail = (("int", "nmu"), ("int", "nre"), (F, "re0"), (F, "dre"), (f"const {F}*", "mu"), (f"const {F}*", "phase"),
                (f"const {F}*", "cdf"), (f"const {F}*", "cld_re"), ("void*", "stream"))
        for twin, base in TWINS.items():
            assert abi.params(twin, sfx) == abi.params(base, sfx)[:-1] + tail, twin
        assert abi.params("rrx_rt_phase_tables", sfx) == (("int", "nmu"), ("int", "nre"), ("int", "nbnd"), (f"const {F}*", "mu"),
                                                          (f"const {F}*", "phase_raw"), (f"{F}*", "phase"), (f"{F}*", "cdf"), ("void*", "stream"))
        head = (("long long", "n"), ("int", "nmu"), ("int", "nre"), ("int", "nbnd"), ("int", "ibnd"), (F, "re0"), (F, "dre"),
                (f"const {F}*", "mu"), (f"const {F}*", "phase"), (f"const {F}*", "cdf"))
        assert abi.params("rrx_rt_phase_sample", sfx) == head + ((f"const {F}*", "u"), (f"const {F}*", "re"), (f"{F}*", "cos_out"), ("void*", "stream"))
        assert abi.params("rrx_rt_phase_eval", sfx) == head + ((f"const {F}*", "cs"), (f"const {F}*", "re"), (f"{F}*", "p_out"), ("void*", "stream"))


def test_library_exports_the_entries():
    lib = abi.lib()
    for name in list(TWINS) + list(ARRAYS) + ["rrx_rt_phase_tables"]:
        for sfx in abi.SFXS:
            assert lib.has(name + sfx), name + sfx


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", list(TWINS))
def test_the_twins_refuse_a_bad_table_without_a_gpu(entry, sfx):
    lib = abi.lib()
    for over, word in (({"null": ("cdf",)}, "mu, phase, cdf, cld_re must be all NULL or all given"),
                       ({"null": ("mu", "phase", "cdf")}, "all NULL or all given"),
                       ({"null": ("cld_re",)}, "all NULL or all given"),
                       ({"null": ("cld_tau", "cld_ssa", "cld_g", "band_lims_gpt")}, "a phase table needs the cloud triple"),
                       ({"nmu": 1}, "nmu must be >= 2"), ({"nmu": -3}, "nmu must be >= 2"), ({"nmu": 4097}, "nmu must be <= 4096"),
                       ({"nre": 0}, "nre must be >= 1"), ({"nre": -1}, "nre must be >= 1"),
                       ({"dre": 0.}, "dre must be > 0"), ({"dre": -1.}, "dre must be > 0"), ({"dre": float("nan")}, "dre must be > 0"),
                       # what the existing entries refuse is still refused
                       ({"mu0": 0.}, "mu0"), ({"knx": 3}, "knx"), ({"null": ("cld_ssa",)}, "cld_tau, cld_ssa, cld_g"),
                       ({"null": ("tau",)}, "tau is NULL"), ({"max_events": 0}, "max_events")):
        assert _call(lib, entry, sfx, **over) != 0, over
        msg = abi.last_error(lib)
        assert msg.startswith(entry + sfx) and word in msg, msg
    # one radius needs no dre; the largest table is accepted as far as the checks go (no photons or rays: no launch)
    none = {d: 0 for d in EXTENTS[entry][-1:]}
    assert _call(lib, entry, sfx, nre=1, dre=0., **none) == 0
    assert _call(lib, entry, sfx, nmu=4096, **none) == 0
    assert _call(lib, entry, sfx, nmu=2, **none) == 0


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", list(TWINS))
def test_the_twins_without_a_table_take_the_checks_of_the_existing_entries(entry, sfx):
    lib = abi.lib()
    none = {d: 0 for d in EXTENTS[entry][-1:]}
    # all four pointers NULL: nmu, nre, re0, dre are not read
    assert _call(lib, entry, sfx, null=TABLE, nmu=0, nre=0, dre=0., **none) == 0
    assert _call(lib, entry, sfx, null=TABLE + ("cld_tau", "cld_ssa", "cld_g", "band_lims_gpt"), **none) == 0
    assert _call(lib, entry, sfx, null=TABLE, mu0=1.5) != 0 and "mu0" in abi.last_error(lib)
    for d in EXTENTS[entry]:
        for null in ((), TABLE):
            assert _call(lib, entry, sfx, null=null, **{d: 0}) == 0, d
            assert _call(lib, entry, sfx, null=null, **{d: -1}) != 0, d
            msg = abi.last_error(lib)
            assert entry + sfx in msg and d + " is negative" in msg, msg


@pytest.mark.parametrize("sfx", abi.SFXS)
def test_phase_tables_checks(sfx):
    lib = abi.lib()
    entry = "rrx_rt_phase_tables"
    ok = dict(nmu=5, nre=3, nbnd=2)
    assert abi.call(lib, entry, sfx, **dict(ok, nbnd=0))[0] == 0
    assert abi.call(lib, entry, sfx, null=("mu", "phase_raw", "phase", "cdf"), **dict(ok, nbnd=0))[0] == 0
    for over, word in (({"nbnd": -1}, "nbnd is negative"), ({"nmu": -1}, "nmu is negative"), ({"nre": -2}, "nre is negative"),
                       ({"nmu": 1}, "nmu must be >= 2"), ({"nmu": 0}, "nmu must be >= 2"), ({"nmu": 4097}, "nmu must be <= 4096"),
                       ({"nre": 0}, "nre must be >= 1")):
        status, msg = abi.call(lib, entry, sfx, **dict(ok, **over))
        assert status != 0 and msg.startswith(entry + sfx) and word in msg, msg
    for name in ("mu", "phase_raw", "phase", "cdf"):
        status, msg = abi.call(lib, entry, sfx, null=(name,), **ok)
        assert status != 0 and name + " is NULL" in msg, msg


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ARRAYS)
def test_array_entries_checks(entry, sfx):
    lib = abi.lib()
    ok = dict(n=7, nmu=5, nre=3, nbnd=2, ibnd=1, re0=4.0, dre=3.0)
    assert abi.call(lib, entry, sfx, **dict(ok, n=0))[0] == 0
    assert abi.call(lib, entry, sfx, null=abi.pointers(entry), **dict(ok, n=0))[0] == 0
    for over, word in (({"n": -1}, "n is negative"), ({"nmu": 1}, "nmu must be >= 2"), ({"nmu": 4097}, "nmu must be <= 4096"),
                       ({"nre": 0}, "nre must be >= 1"), ({"dre": 0.}, "dre must be > 0"), ({"nbnd": 0}, "nbnd must be >= 1"),
                       ({"ibnd": 2}, "ibnd is outside"), ({"ibnd": -1}, "ibnd is outside")):
        status, msg = abi.call(lib, entry, sfx, **dict(ok, **over))
        assert status != 0 and msg.startswith(entry + sfx) and word in msg, msg
    for name in abi.pointers(entry):
        status, msg = abi.call(lib, entry, sfx, null=(name,), **ok)
        assert status != 0 and name + " is NULL" in msg, msg
    assert abi.call(lib, entry, sfx, **dict(ok, n=0, nre=1, dre=0.))[0] == 0


def test_host_libraries_export_the_phase_table_setters():
    import os
    import subprocess
    for header, cls in (("Raytracer.h", "Raytracer_gpu"), ("Raytracer_bw.h", "Raytracer_bw_gpu")):
        text = open(os.path.join(abi.ROOT, "include", header)).read()
        assert "set_phase_table(" in text and "clear_phase_table(" in text, header
    driver = open(os.path.join(abi.ROOT, "include_test", "rrx_cxx_driver.h")).read()
    assert "rrx_cxx_trace_rays_phase(" in driver and "rrx_cxx_trace_rays_bw_phase(" in driver
    for name in ("librte_rrtmgp_hip.so", "librte_rrtmgp_hip_sp.so"):
        hostlib = os.path.join(abi.ROOT, "rte-rrtmgp-cpp_amd", "lib", name)
        if not os.path.exists(hostlib):
            pytest.fail(f"{hostlib} not built: run __graft_entry__.build()")
        syms = subprocess.run(["nm", "-DC", "--defined-only", hostlib], capture_output=True, text=True).stdout
        for sym in ("Raytracer_gpu::set_phase_table(", "Raytracer_bw_gpu::set_phase_table(",
                    "rrx_cxx_trace_rays_phase", "rrx_cxx_trace_rays_bw_phase"):
            assert sym in syms, (name, sym)
