#!/usr/bin/env python3
"""The thermal ray tracer's loop over g-points against the rays of all g-points in one launch (rrx_thermal_render against
rrx_thermal_render_spectral), in one process on one GPU, on the broken-cloud field of tools/raytracer_bench.py (cells of
100 x 100 x 50 m, 32 layers, k_null blocks of 8 x 8 x 4 cells) with the longwave sources of tools/raytracer_thermal_bench.py (sfc_emis =
1 - the field's albedo, a layer source that falls with height, a warmer surface, nothing coming down through the top) under the
perspective camera of tools/raytracer_bw_bench.py, at equal TOTAL rays: the one-launch form gets m_g = rays per pixel of the loop in
every g-point and a row of ones for its channel matrix, so its weights are exactly 1 and it traces the very rays of the loop.

Two budgets: `small`, a preview: 64 x 64 pixels over 64 x 64 columns, --ngpt-small g-points (224), 1 ray per pixel and g-point (4 096
rays per launch of the loop), and `large`, 256 x 256 pixels over 256 x 256 columns, --ngpt-large g-points (16), 4 rays.
Forms, each in fp64 and fp32:
  loop      rrx_thermal_render: the host loop over g-points
  spectral  rrx_thermal_render_spectral with equal m_g and a row of ones
Device events around --steps calls after --warmup, --rounds times; the two forms alternate round by round, so that a drift of the
clocks meets both; the median is reported and the rounds are kept: the loop's own spread is the margin of the comparison. One JSON
line each, printed and appended to --out (default profiles/raytracer_thermal_spectral_bench.txt). A record, not a target.

One budget and one precision per process, each under a time limit of its own, and nothing starts after a step that failed:

  timeout -k 10 300 python tools/raytracer_thermal_spectral_bench.py --budgets small --dtype f64 &&
  timeout -k 10 300 python tools/raytracer_thermal_spectral_bench.py --budgets small --dtype f32 &&
  timeout -k 10 300 python tools/raytracer_thermal_spectral_bench.py --budgets large --dtype f64 &&
  timeout -k 10 300 python tools/raytracer_thermal_spectral_bench.py --budgets large --dtype f32 &&
  timeout -k 10 300 python tools/raytracer_thermal_spectral_bench.py --budgets none --variance-ratio

--variance-ratio: ngpt sum e^2 / (sum e)^2 of the synthetic 256-g-point longwave set (synthetic.make_kdist("lw") on
synthetic.make_atmosphere), e_g the sum over the columns of the chain's own sfc_src[g]: the broadband variance of the equal split over
that of the split in proportion to the emission, at an equal per-ray spread in every g-point (DESIGN 4.19 records 1.090 for the
shortwave set).
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

DX, DY, DZ, SEED, NZ = 100.0, 100.0, 50.0, 11, 32


def variance_ratio(R, torch):
    from rte_rrtmgp_cpp_amd import pipeline, synthetic
    be = R.HipKernels(np.float64, "cuda:0")
    kd = be.upload_kdist(synthetic.make_kdist("lw"))
    atm = pipeline.upload_atmosphere(be, synthetic.make_atmosphere(64))
    _, col_gas, _ = pipeline.gas_state(be, kd, atm, None, interpolate=False)
    src = be.planck_source_direct(kd, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, pipeline._sfc_lay(atm), col_gas)
    e = be.to_numpy(src["sfc_src"]).astype(np.float64).sum(axis=1)
    ratio = e.size*float(np.sum(e*e)) / float(np.sum(e))**2
    return dict(tool="raytracer_thermal_spectral_bench", record="variance_ratio", set="synthetic.make_kdist('lw')", ngpt=int(e.size),
                ncol=64, variance_ratio=round(ratio, 3), e_min=float(e.min()), e_max=float(e.max()), spread=round(float(e.max()/e.min()), 1),
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngpt-small", type=int, default=224)
    ap.add_argument("--ngpt-large", type=int, default=16)
    ap.add_argument("--budgets", default="small,large", help="small, large, both with a comma, or none")
    ap.add_argument("--dtype", default="both", choices=["both", "f64", "f32"])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variance-ratio", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raytracer_thermal_spectral_bench.txt"))
    args = ap.parse_args()

    import torch
    import rte_rrtmgp_cpp_amd as R
    from rte_rrtmgp_cpp_amd import camera as C
    from raytracer_bench import broken_cloud_field
    from raytracer_thermal_bench import sources

    budgets = {"small": (64, 64, args.ngpt_small, 1), "large": (256, 256, args.ngpt_large, 4)}
    lines = []
    for name in ([] if args.budgets == "none" else args.budgets.split(",")):
        nx, ny, ngpt, rpp = budgets[name]
        kn_grid = (nx//8, ny//8, NZ//4)
        tau, ssa, cloud, lims, albedo = broken_cloud_field(nx, ny, NZ, ngpt)
        lay, sfc, emis = sources(tau, albedo)
        cam = C.perspective(nx, ny, (0.5*nx*DX, 0.5*ny*DY, 0.9*NZ*DZ), yaw=0.8, pitch=-0.5, fov=math.radians(60.))
        m = np.full(ngpt, rpp, dtype=np.int64)
        ones = np.ones((1, int(lims.shape[0])))
        for dt in (("f64", "f32") if args.dtype == "both" else (args.dtype,)):
            be = R.HipKernels(np.float64 if dt == "f64" else np.float32, "cuda:0")
            A = be.asarray
            d_cloud, d_lims = tuple(A(c) for c in cloud), A(lims)
            scene = (A(tau), A(ssa), nx, ny, DX, DY, DZ, A(emis), A(lay), A(sfc), kn_grid, cam)
            runs = {"loop": lambda: be.thermal_render(*scene, rpp, SEED, cloud=d_cloud, band_lims=d_lims),
                    "spectral": lambda: be.thermal_render_spectral(*scene, m, SEED, d_lims, ones, cloud=d_cloud)}
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
                out = dict(tool="raytracer_thermal_spectral_bench", budget=name, dtype=dt, form=form, ms=round(ms, 3),
                           rounds_ms=[round(t, 3) for t in times[form]], rays=rays, rays_per_s=round(rays / (ms*1e-3)),
                           n_capped=r["n_capped"], n_clamped=r["n_clamped"], nx=nx, ny=ny, nz=NZ, npx=nx, npy=ny, ngpt=ngpt,
                           rays_per_pixel_per_gpt=rpp, kn_grid=list(kn_grid), mean_radiance=round(float(r["radiance"].double().mean().item()), 6),
                           gpt_per_launch_env=os.environ.get("RRX_RT_SPECTRAL_GPT_PER_LAUNCH"), steps=args.steps, warmup=args.warmup,
                           rounds=args.rounds, device=torch.cuda.get_device_name(0))
                if form == "spectral":
                    out["speedup_over_loop"] = round(float(np.median(times["loop"])) / ms, 3)
                print(json.dumps(out), flush=True)
                lines.append(json.dumps(out))
            del d_cloud, scene, runs, result
            torch.cuda.empty_cache()
    if args.variance_ratio:
        lines.append(json.dumps(variance_ratio(R, torch)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
