#!/usr/bin/env python3
"""The thermal ray tracer's cell sensors (rrx_heating3d_render) in rays per second, in one process on one GPU, on
the broken-cloud field of tools/raytracer_bench.py (cells of 100 x 100 x 50 m, 32 layers, k_null blocks of 8 x 8 x 4 cells) with the
longwave sources of tools/raytracer_thermal_bench.py, as tools/raytracer_thermal_spectral_bench.py sets them up: --nx x --ny columns,
--ngpt g-points, --rays-per-cell rays per cell and g-point. The yardstick runs on the same field in the same process:
rrx_thermal_render_spectral under the perspective camera of that tool with --nx x --ny pixels and --rays-per-pixel rays per pixel and
g-point, a row of ones for its channel matrix.

Forms, each in fp64 and fp32:
  heating   rrx_heating3d_render with equal m_g
  camera    rrx_thermal_render_spectral with equal m_g (the yardstick)
Device events around --steps calls after --warmup, --rounds times; the two forms alternate round by round; the median is reported
and the rounds are kept. --restatement adds the events and deposits per ray of tests/raytracer_heating_ref.py on the --cut x --cut
corner of the field, g-point 0, float64 (no GPU). One JSON line each, printed and appended to --out (default
profiles/raytracer_heating_bench.txt). A record, not a target: no threshold is set here.

One precision per process, each under a time limit of its own, and nothing starts after a step that failed:

  timeout -k 10 300 python tools/raytracer_heating_bench.py --dtype f64 &&
  timeout -k 10 300 python tools/raytracer_heating_bench.py --dtype f32 &&
  timeout -k 10 300 python tools/raytracer_heating_bench.py --dtype none --restatement
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DX, DY, DZ, SEED, NZ = 100.0, 100.0, 50.0, 11, 32


def restatement(tau, ssa, cloud, lims, albedo, nx, cut, rays_per_cell):
    """events and deposits per ray on the cut x cut corner of the field, g-point 0, float64"""
    import raytracer_ref as R
    import raytracer_heating_ref as H
    import raytracer_thermal_ref as T
    from raytracer_thermal_bench import sources
    col = (np.arange(cut)[None, :] + nx*np.arange(cut)[:, None]).reshape(-1)
    take = lambda a: np.ascontiguousarray(a[..., col])
    lay, sfc, emis = sources(tau, albedo)
    ngpt = tau.shape[0]
    medium = R.Scene(nx=cut, ny=cut, nz=NZ, dx=DX, dy=DY, dz=DZ, tau=take(tau), ssa=take(ssa), sfc_albedo=take(albedo), mu0=1.0, azimuth=0.0,
                     inc_dir=np.zeros(ngpt), inc_dif=np.zeros(ngpt), kn_grid=(max(cut//8, 1), max(cut//8, 1), NZ//4),
                     cloud=tuple(take(c) for c in cloud), band_lims=lims.reshape(-1, 2), top_at_1=False, seed=SEED)
    sc = T.ThermalScene(medium, take(lay), take(sfc), take(emis), np.zeros(ngpt))
    nrays = rays_per_cell*cut*cut*NZ
    c = H.trace_counts_heating(sc, 0, 0, nrays)
    return dict(tool="raytracer_heating_bench", record="restatement", cut=cut, nz=NZ, gpt=0, rays=nrays, events_per_ray=round(c["events"]/nrays, 3),
                deposits_per_ray=round(c["deposits"]/nrays, 3), nonzero_deposits_per_ray=round(int(c["n_dep"].sum())/nrays, 3),
                n_capped=c["n_capped"], n_clamped=c["n_clamped"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=256)
    ap.add_argument("--ny", type=int, default=256)
    ap.add_argument("--ngpt", type=int, default=16)
    ap.add_argument("--rays-per-cell", type=int, default=1)
    ap.add_argument("--rays-per-pixel", type=int, default=4)
    ap.add_argument("--dtype", default="both", choices=["both", "f64", "f32", "none"])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--cut", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raytracer_heating_bench.txt"))
    args = ap.parse_args()

    from raytracer_bench import broken_cloud_field
    from raytracer_thermal_bench import sources

    nx, ny, ngpt = args.nx, args.ny, args.ngpt
    kn_grid = (nx//8, ny//8, NZ//4)
    tau, ssa, cloud, lims, albedo = broken_cloud_field(nx, ny, NZ, ngpt)
    lines = []
    if args.dtype != "none":
        import torch
        import rte_rrtmgp_cpp_amd as R
        from rte_rrtmgp_cpp_amd import camera as C
        lay, sfc, emis = sources(tau, albedo)
        cam = C.perspective(nx, ny, (0.5*nx*DX, 0.5*ny*DY, 0.9*NZ*DZ), yaw=0.8, pitch=-0.5, fov=math.radians(60.))
        m_cell = np.full(ngpt, args.rays_per_cell, dtype=np.int64)
        m_pix = np.full(ngpt, args.rays_per_pixel, dtype=np.int64)
        ones = np.ones((1, int(lims.shape[0])))
        for dt in (("f64", "f32") if args.dtype == "both" else (args.dtype,)):
            be = R.HipKernels(np.float64 if dt == "f64" else np.float32, "cuda:0")
            A = be.asarray
            d_cloud, d_lims = tuple(A(c) for c in cloud), A(lims)
            scene = (A(tau), A(ssa), nx, ny, DX, DY, DZ, A(emis), A(lay), A(sfc), kn_grid)
            runs = {"heating": lambda: be.thermal_heating_render(*scene, m_cell, SEED, d_lims, cloud=d_cloud),
                    "camera": lambda: be.thermal_render_spectral(*scene, cam, m_pix, SEED, d_lims, ones, cloud=d_cloud)}
            rays = {"heating": args.rays_per_cell*nx*ny*NZ*ngpt, "camera": args.rays_per_pixel*nx*ny*ngpt}
            times, result = {k: [] for k in runs}, {}
            for _ in range(args.rounds):
                for form, run in runs.items():
                    for _ in range(args.warmup):
                        run()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.steps):
                        result[form] = run()
                    e1.record()
                    torch.cuda.synchronize()
                    times[form].append(e0.elapsed_time(e1) / args.steps)
            for form in runs:
                r = result[form]
                ms = float(np.median(times[form]))
                out = dict(tool="raytracer_heating_bench", dtype=dt, form=form, ms=round(ms, 3), rounds_ms=[round(t, 3) for t in times[form]],
                           rays=rays[form], rays_per_s=round(rays[form] / (ms*1e-3)), n_capped=r["n_capped"], n_clamped=r["n_clamped"],
                           nx=nx, ny=ny, nz=NZ, ngpt=ngpt, kn_grid=list(kn_grid), steps=args.steps, warmup=args.warmup, rounds=args.rounds,
                           device=torch.cuda.get_device_name(0))
                if form == "heating":
                    f = r["flux_conv"].double()
                    out.update(rays_per_cell_per_gpt=args.rays_per_cell, mean_flux_conv=round(float(f.mean().item()), 6),
                               min_layer_mean=round(float(f.mean(dim=1).min().item()), 6), max_layer_mean=round(float(f.mean(dim=1).max().item()), 6))
                else:
                    out.update(rays_per_pixel_per_gpt=args.rays_per_pixel, npx=nx, npy=ny,
                               mean_radiance=round(float(r["radiance"].double().mean().item()), 6))
                print(json.dumps(out), flush=True)
                lines.append(json.dumps(out))
            del d_cloud, scene, runs, result
            torch.cuda.empty_cache()
    if args.restatement:
        lines.append(json.dumps(restatement(tau, ssa, cloud, lims, albedo, nx, args.cut, args.rays_per_cell)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
