#!/usr/bin/env python3
"""The backward ray tracer's spectral loop against the rays of all g-points in one launch (rrx_raytracer_bw_aer against
rrx_camera_render_spectral), in one process on one GPU, on the broken-cloud field of tools/raytracer_bench.py (cells of
100 x 100 x 50 m, 32 layers, k_null blocks of 8 x 8 x 4 cells, albedo 0.2, mu0 = 0.6, equal incident flux in every g-point) under the
perspective camera of tools/raytracer_bw_bench.py, at equal TOTAL rays: the one-launch form gets m_g = rays per pixel of the loop in
every g-point and a row of ones for its channel matrix, so its weights are 1 and it traces the very rays of the loop.

Two budgets: `small`, a preview: 64 x 64 pixels over 64 x 64 columns, --ngpt-small g-points (224, the size of the shortwave set), 1
ray per pixel and g-point (4 096 rays per launch of the loop), and `large`, 256 x 256 pixels over 256 x 256 columns, --ngpt-large
g-points (16), 4 rays.
Forms, each in fp64 and fp32:
  loop      rrx_raytracer_bw_aer with NULL aerosol triples and no background: the host loop over g-points
  spectral  rrx_camera_render_spectral with equal m_g and a row of ones
Device events around --steps calls after --warmup, --rounds times; the two forms alternate round by round, so that a drift of the
clocks meets both; the median is reported and the rounds are kept: the loop's own spread is the margin of the comparison. One JSON
line each, printed and appended to --out (default profiles/raytracer_bw_spectral_bench.txt). A record, not a target.

  python tools/raytracer_bw_spectral_bench.py
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

DX, DY, DZ, MU0, AZIMUTH, SEED, NZ = 100.0, 100.0, 50.0, 0.6, 0.5, 11, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngpt-small", type=int, default=224)
    ap.add_argument("--ngpt-large", type=int, default=16)
    ap.add_argument("--budgets", default="small,large")
    ap.add_argument("--dtype", default="both", choices=["both", "f64", "f32"])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raytracer_bw_spectral_bench.txt"))
    args = ap.parse_args()

    import torch
    import rte_rrtmgp_cpp_amd as R
    from rte_rrtmgp_cpp_amd import camera as C
    from raytracer_bench import broken_cloud_field

    budgets = {"small": (64, 64, args.ngpt_small, 1), "large": (256, 256, args.ngpt_large, 4)}
    lines = []
    for name in args.budgets.split(","):
        nx, ny, ngpt, rpp = budgets[name]
        kn_grid = (nx//8, ny//8, NZ//4)
        tau, ssa, cloud, lims, albedo = broken_cloud_field(nx, ny, NZ, ngpt)
        cam = C.perspective(nx, ny, (0.5*nx*DX, 0.5*ny*DY, 0.9*NZ*DZ), yaw=0.8, pitch=-0.5, fov=math.radians(60.))
        inc_dir, m = np.full(ngpt, 100.0), np.full(ngpt, rpp, dtype=np.int64)
        ones = np.ones((1, int(lims.shape[0])))
        for dt in (("f64", "f32") if args.dtype == "both" else (args.dtype,)):
            be = R.HipKernels(np.float64 if dt == "f64" else np.float32, "cuda:0")
            A = be.asarray
            d_tau, d_ssa, d_cloud, d_lims, d_alb = A(tau), A(ssa), tuple(A(c) for c in cloud), A(lims), A(albedo)
            scene = (d_tau, d_ssa, nx, ny, DX, DY, DZ, d_alb, MU0, AZIMUTH, inc_dir, kn_grid, cam)
            runs = {"loop": lambda: be.raytracer_bw_bg(*scene, rpp, SEED, aerosol=(None, None, None), cloud=d_cloud, band_lims=d_lims),
                    "spectral": lambda: be.camera_render_spectral(*scene, m, SEED, d_lims, ones, cloud=d_cloud)}
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
            rays = rpp*nx*ny*ngpt
            for form in runs:
                r = result[form]
                ms = float(np.median(times[form]))
                out = dict(tool="raytracer_bw_spectral_bench", budget=name, dtype=dt, form=form, ms=round(ms, 3),
                           rounds_ms=[round(t, 3) for t in times[form]], rays=rays, rays_per_s=round(rays / (ms*1e-3)),
                           n_capped=r["n_capped"], n_clamped=r["n_clamped"], nx=nx, ny=ny, nz=NZ, npx=nx, npy=ny, ngpt=ngpt,
                           rays_per_pixel_per_gpt=rpp, kn_grid=list(kn_grid), mean_radiance=round(float(r["radiance"].double().mean().item()), 6),
                           gpt_per_launch_env=os.environ.get("RRX_RT_SPECTRAL_GPT_PER_LAUNCH"), steps=args.steps, warmup=args.warmup,
                           rounds=args.rounds, device=torch.cuda.get_device_name(0))
                if form == "spectral":
                    out["speedup_over_loop"] = round(float(np.median(times["loop"])) / ms, 3)
                print(json.dumps(out), flush=True)
                lines.append(json.dumps(out))
            del d_tau, d_ssa, d_cloud, scene, runs, result
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
