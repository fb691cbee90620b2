#!/usr/bin/env python3
"""Digests of the integers that the backward and the thermal ray tracers' trace entries write, on the smallest scene that reaches every
branch of a ray's start: a 4 x 4 x 4 grid of 100 x 100 x 50 m cells with k_null blocks of 2 x 2 x 2 cells, 2 g-points in 1 band, cloud
in some cells, 4 x 3 pixels, 64 rays per pixel. Entries: rrx_rt_bw_trace_counts, _phase, _bg, _aer (the last two with 2 background
layers of 300 and 500 m, so that a start may lie in a layer), rrx_camera_trace_counts_spectral (the same background),
rrx_thermal_trace_counts and rrx_thermal_trace_counts_spectral. Sensors, in both precisions: perspective inside the grid, between the
domain top and the background's top looking down, above both looking down (moved to the top) and looking up (ends at once), fisheye with
fov = 2 pi, orthographic from the domain top and from aloft, flux sensor facing up, facing down, and facing down from aloft.

One JSON line per case with the sha256 of counts, n_capped and n_clamped, printed and appended to --out. Two builds that write the same
lines traced the same rays to the same integers.

  python tools/rt_sensor_digests.py [--lib PATH] [--label NAME] [--out profiles/rt_sensor_refactor_digests.jsonl]
--lib: a librrx_hip.so of another build in place of the tree's own; --label goes into every line as "build" and is the one field in
which the lines of two builds may differ."""
import argparse
import hashlib
import json
import math
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NX, NY, NZ, NGPT, KN = 4, 4, 4, 2, (2, 2, 2)
DX, DY, DZ, DZ_BG = 100.0, 100.0, 50.0, (300.0, 500.0)
NPX, NPY, RPP, SEED, MU0, AZIMUTH = 4, 3, 64, 2024, 0.6, 0.7


def sensors(C):
    inside, aloft, above = (150., 170., 120.), (150., 170., 600.), (150., 170., 1500.)
    ortho, down = C.orthographic(NPX, NPY, yaw=0.4, pitch=-1.2), C.flux_sensor(NPX, NPY, up=False)
    lifted = lambda cam: C.Camera(cam.type, cam.npx, cam.npy, cam.fov, (0., 0., 600.), cam.e_w, cam.e_h, cam.e_d)
    return {"perspective_inside": C.perspective(NPX, NPY, inside, yaw=0.8, pitch=-0.5),
            "perspective_aloft_down": C.perspective(NPX, NPY, aloft, yaw=0.8, pitch=-1.0),
            "perspective_above_down": C.perspective(NPX, NPY, above, yaw=0.8, pitch=-1.0),
            "perspective_above_up": C.perspective(NPX, NPY, above, yaw=0.8, pitch=0.9),
            "fisheye_2pi": C.fisheye(NPX, NPY, inside, fov=2.*math.pi),
            "orthographic": ortho, "orthographic_aloft": lifted(ortho),
            "flux_up": C.flux_sensor(NPX, NPY, up=True), "flux_down": down, "flux_down_aloft": lifted(down)}


def scene(be):
    """the medium on the device: gas, a cloud in some cells, an aerosol, a background of two layers, the thermal sources"""
    rng = np.random.default_rng(5)
    ncol, A = NX*NY, be.asarray
    u = lambda lo, hi, *shape: rng.uniform(lo, hi, shape)
    cld_tau = np.where(u(0., 1., 1, NZ, ncol) < 0.4, u(0.5, 4., 1, NZ, ncol), 0.)
    s = SimpleNamespace(tau=A(u(0.01, 0.2, NGPT, NZ, ncol)), ssa=A(u(0.3, 0.99, NGPT, NZ, ncol)), lims=A(np.array([[1, NGPT]], dtype=np.int32)),
                        cloud=tuple(A(a) for a in (cld_tau, u(0.9, 1., 1, NZ, ncol), u(0.7, 0.9, 1, NZ, ncol))),
                        aerosol=tuple(A(a) for a in (u(0., 0.1, 1, NZ, ncol), u(0.8, 1., 1, NZ, ncol), u(0.5, 0.8, 1, NZ, ncol))),
                        albedo=A(u(0.05, 0.5, ncol)), emis=A(u(0.8, 1., ncol)), lay_src=A(u(50., 90., NGPT, NZ, ncol)),
                        sfc_src=A(u(90., 120., NGPT, ncol)), top=np.array([3., 5.]), cld_re=A(u(5., 15., NZ, ncol)))
    s.background = SimpleNamespace(dz=np.array(DZ_BG), tau=A(u(0.02, 0.2, NGPT, 2)), ssa=A(u(0.5, 0.99, NGPT, 2)),
                                   cloud=tuple(A(a) for a in (u(0., 0.5, 1, 2), u(0.9, 1., 1, 2), u(0.7, 0.9, 1, 2))), aerosol=None)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_sensor_refactor_digests.jsonl"))
    args = ap.parse_args()

    import rte_rrtmgp_cpp_amd as R
    from rte_rrtmgp_cpp_amd import camera as C, hip_kernels, phase_tables
    if args.lib is not None:
        hip_kernels.LIB_PATH = os.path.abspath(args.lib)

    nrays, lines = RPP*NPX*NPY, []
    ray_end, ones = np.array([0, nrays, 2*nrays], dtype=np.int64), np.ones(NGPT)
    for dt in ("f64", "f32"):
        be = R.HipKernels(np.float64 if dt == "f64" else np.float32, "cuda:0")
        s = scene(be)
        mu = phase_tables.nodes(33)
        table = phase_tables.build(be, mu, np.stack([phase_tables.double_hg(mu, 0.85, -0.3, 0.9), phase_tables.henyey_greenstein(mu, 0.8)])[None],
                                   re0=5., dre=10.).with_radius(s.cld_re)
        grid = dict(top_at_1=False, cloud=s.cloud, band_lims=s.lims)
        kn = lambda **kw: be.rt_k_null(s.tau, 1, NX, NY, DZ, KN, False, cloud=s.cloud, band_lims=s.lims, **kw)
        kn_all = lambda **kw: be.rt_k_null_all(s.tau, NX, NY, DZ, KN, False, cloud=s.cloud, band_lims=s.lims, **kw)
        solar = (NX, NY, DX, DY, DZ, s.albedo, MU0, AZIMUTH)
        thermal = (NX, NY, DX, DY, DZ, s.emis, s.lay_src, s.sfc_src)
        for name, cam in sensors(C).items():
            put = lambda k_null: (KN, k_null, cam, SEED, 0)          # kn_grid ... ray0
            cases = {
                "rt_bw_trace_counts": lambda: be.rt_bw_trace_counts(s.tau, s.ssa, 1, *solar, *put(kn()), nrays, **grid),
                "rt_bw_trace_counts_phase": lambda: be.rt_bw_trace_counts(s.tau, s.ssa, 1, *solar, *put(kn()), nrays, phase=table, **grid),
                "rt_bw_trace_counts_bg": lambda: be.rt_bw_trace_counts_bg(s.tau, s.ssa, 1, *solar, *put(kn()), nrays, background=s.background, **grid),
                "rt_bw_trace_counts_aer": lambda: be.rt_bw_trace_counts_bg(s.tau, s.ssa, 1, *solar, *put(kn(aerosol=s.aerosol)), nrays,
                                                                           background=s.background, aerosol=s.aerosol, **grid),
                "camera_trace_counts_spectral": lambda: be.camera_trace_counts_spectral(
                    s.tau, s.ssa, *solar, ray_end, ones, *put(kn_all(aerosol=s.aerosol)), 2*nrays, s.lims, cloud=s.cloud, phase=table,
                    background=s.background, aerosol=s.aerosol),
                "thermal_trace_counts": lambda: be.thermal_trace_counts(s.tau, s.ssa, 1, *thermal, float(s.top[1]), *put(kn()), nrays, **grid),
                "thermal_trace_counts_spectral": lambda: be.thermal_trace_counts_spectral(
                    s.tau, s.ssa, *thermal, s.top, ray_end, ones, *put(kn_all()), 2*nrays, s.lims, cloud=s.cloud),
            }
            for entry, run in cases.items():
                counts = run()
                line = dict(build=args.label, entry=entry, dtype=dt, sensor=name)
                for k in ("counts", "n_capped", "n_clamped"):
                    line[k] = hashlib.sha256(counts[k].cpu().numpy().tobytes()).hexdigest()
                line["sum_counts"] = int(counts["counts"].cpu().numpy().astype(np.uint64).sum(dtype=np.uint64))
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
