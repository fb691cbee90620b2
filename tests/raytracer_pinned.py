"""The recorded results of the numpy restatement of the ray tracers (raytracer_ref.py, raytracer_bw_ref.py and the two spectral
modules), for test_raytracer_ref_pinned.py and the tests that compare with them. tests/golden/raytracer_ref_digests.json holds one
blake2b digest per case of what the restatement returned before its plain, background, aerosol and spectral forms became calls of
one forward and one backward event loop (seven modules then, each form through its own: the case's `via`); run() recomputes a case
with the restatement as it is. The digest covers what the call returned then; a call may return more today (the tallies above the
domain top and the scattering tallies, whatever the form).

A case is built from the scene builders: raytracer_aer_scenes.general for the g-point forms, raytracer_spectral_scenes.general on
4 x 3 x 4 cells for the spectral ones, then `aerosol` (both, grid, aloft, none, or triples of zeros with ssa_a = 0.9 and g_a = 0.7),
`bg`, `independent_column`, `band_lims` and `table` (double_hg33 of raytracer_phase_scenes with cell_radii). The file's `defaults`
hold for what a case does not name; `sensors` are the sensors by name; `keysets[case.keys]` names what the digest covers, in
order."""
import functools
import hashlib
import json
import os

import numpy as np

import raytracer_ref as R
import raytracer_bw_ref as B
import raytracer_spectral_ref as SP
import raytracer_bw_spectral_ref as BSP
import raytracer_phase_ref as P
import raytracer_phase_scenes as PS
import raytracer_aer_scenes as SA
import raytracer_spectral_scenes as SS

with open(os.path.join(os.path.dirname(__file__), "golden", "raytracer_ref_digests.json")) as f:
    PINNED = json.load(f)
CASES = [dict(PINNED["defaults"], **c) for c in PINNED["cases"]]
DT = {"f64": np.float64, "f32": np.float32}


def digest(res, keys):
    h = hashlib.blake2b(digest_size=16)
    for k in keys:
        v = res[k]
        h.update(k.encode())
        if isinstance(v, (int, np.integer)):
            h.update(b"int" + str(int(v)).encode())
        else:
            a = np.ascontiguousarray(v)
            h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def build(case):
    """(scene, background or None, table or None)"""
    dt = DT[case["dtype"]]
    if case["kind"] in ("fw", "bw", "sw", "bw_solve"):
        sc, bg = SA.general(dt, case["top_at_1"])
    else:
        sc, bg = SS.general(dt, case["top_at_1"], nx=4, ny=3, nz=4, kn=(2, 1, 2))
    how = case["aerosol"]
    if how == "zeros":
        nb = sc.cloud[0].shape[0]
        z, zb = np.zeros((nb, sc.nz, sc.ncol), dtype=dt), np.zeros((nb, bg.nbg), dtype=dt)
        sc.aerosol, bg.aerosol = (z, z + dt(0.9), z + dt(0.7)), (zb, zb + dt(0.9), zb + dt(0.7))
    if how in ("none", "aloft"):
        sc.aerosol = None
    if how in ("none", "grid"):
        bg.aerosol = None
    if not case["bg"]:
        bg = None
    sc.independent_column = case["independent_column"]
    if case["band_lims"] is not None:
        sc.band_lims = np.array(case["band_lims"], dtype=np.int32)
    table = None
    if case["table"]:
        table = P.build_tables(*PS.double_hg33(), dt, PS.RE0, PS.DRE)
        table.cld_re = PS.cell_radii(sc, dt)
    return sc, bg, table


def listed(case, lister, *args):
    """(the list's ends, the weights: the list's own, or the case's)"""
    end, w0 = lister(*args)[:2]
    if case["weights"] != "list":
        w0 = np.asarray(case["weights"], dtype=w0.dtype)
    n = int(end[-1]) - case["first"] if case["n"] == "rest" else case["n"]
    return end, w0, n


def run(case):
    sc, bg, table = build(case)
    kind, me = case["kind"], case["max_events"]
    sensor = B.Sensor(**PINNED["sensors"][case["sensor"]])
    if kind == "fw":
        return R.trace_counts(sc, case["igpt"], case["first"], case["n"], me, table, bg)
    if kind == "bw":
        return B.trace_counts_bw(sc, sensor, case["igpt"], case["first"], case["n"], me, case["ranges"], table, bg)
    if kind == "sw":
        return R.raytracer_sw(sc, case["per_pixel"], me, bg)
    if kind == "bw_solve":
        return B.raytracer_bw(sc, sensor, case["per_pixel"], me, bg)
    if kind == "spectral_fw":
        end, w0, n = listed(case, SP.photon_list, sc, case["m"])
        return SP.trace_counts(sc, bg, end, w0, case["first"], n, me, table)
    if kind == "spectral_sw":
        return SP.raytracer_sw(sc, bg, case["m"], me, table)
    if kind == "spectral_bw":
        end, w0, n = listed(case, BSP.ray_list, sc, sensor, case["m"])
        return BSP.trace_counts(sc, bg, sensor, end, w0, case["first"], n, me, table)
    assert kind == "render", kind
    return BSP.render(sc, bg, sensor, case["m"], np.array(case["M"]), me, table)


@functools.lru_cache(maxsize=None)
def pinned(name):
    """what the restatement gives for the recorded case `name`, after the check that it is what was recorded (computed once; the
    callers leave it unchanged)"""
    case = next(c for c in CASES if c["name"] == name)
    res = run(case)
    assert digest(res, PINNED["keysets"][case["keys"]]) == case["digest"], name
    return res
