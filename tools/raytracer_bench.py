#!/usr/bin/env python3
"""Throughput of the forward Monte Carlo ray tracer (rrx_raytracer_sw), in one process on one GPU.

A synthetic broken-cloud field: nx x ny x nz cells of 100 x 100 x 50 m, a thin scattering gas in every cell, and liquid-like cloud
(tau = 2 per cell, ssa = 0.999, g = 0.85) in the cells of layers nz/4 .. nz/2 where a smoothed random field exceeds its 60th
percentile (cloud cover about 40 %, in clumps of a few cells); albedo 0.2, mu0 = 0.6, --ngpt g-points with equal incident flux,
k_null blocks of 8 x 8 x 4 cells. Timed with device events around --steps calls after --warmup, --rounds times; the median is
reported as photons per second, for fp64 and fp32, in 3-D and in independent-column mode. One JSON line per configuration, printed and
appended to --out (default profiles/raytracer_bench.txt). A record, not a target.

  python tools/raytracer_bench.py
  python tools/raytracer_bench.py --nx 256 --ny 256 --photons-per-pixel 128
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def broken_cloud_field(nx, ny, nz, ngpt, seed=7):
    """(tau, ssa) (ngpt, nz, ncol), the cloud triple (1, nz, ncol), band limits, albedo (ncol,); layer 0 is the lowest"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((ny, nx))
    for _ in range(4):                                   # periodic smoothing: clumps of a few cells
        f = (f + np.roll(f, 1, 0) + np.roll(f, -1, 0) + np.roll(f, 1, 1) + np.roll(f, -1, 1)) / 5.0
    cloudy = (f > np.percentile(f, 60.0)).reshape(-1)
    ncol = nx*ny
    tau = np.full((ngpt, nz, ncol), 0.01) * (1.0 + 0.5*np.arange(ngpt))[:, None, None]
    ssa = np.full((ngpt, nz, ncol), 0.6)
    ct = np.zeros((1, nz, ncol))
    ct[0, nz//4:nz//2, :] = np.where(cloudy, 2.0, 0.0)[None, :]
    cloud = (ct, np.full_like(ct, 0.999), np.full_like(ct, 0.85))
    return tau, ssa, cloud, np.array([[1, ngpt]], dtype=np.int32), np.full(ncol, 0.2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=128)
    ap.add_argument("--ny", type=int, default=128)
    ap.add_argument("--nz", type=int, default=32)
    ap.add_argument("--ngpt", type=int, default=4)
    ap.add_argument("--photons-per-pixel", type=int, default=64)
    ap.add_argument("--dtype", default="both", choices=["both", "f64", "f32"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raytracer_bench.txt"))
    args = ap.parse_args()

    import torch
    import rte_rrtmgp_cpp_amd as R

    nx, ny, nz, ngpt, ppp = args.nx, args.ny, args.nz, args.ngpt, args.photons_per_pixel
    kn_grid = (max(nx//8, 1), max(ny//8, 1), max(nz//4, 1))
    tau, ssa, cloud, lims, albedo = broken_cloud_field(nx, ny, nz, ngpt)
    inc_dir, inc_dif = np.full(ngpt, 100.0), np.zeros(ngpt)
    lines = []
    for dt in (("f64", "f32") if args.dtype == "both" else (args.dtype,)):
        be = R.HipKernels(np.float64 if dt == "f64" else np.float32, "cuda:0")
        A = be.asarray
        d_tau, d_ssa, d_cloud, d_lims, d_alb = A(tau), A(ssa), tuple(A(c) for c in cloud), A(lims), A(albedo)
        for ic in (False, True):
            state = {}

            def run():
                state["r"] = be.raytracer_sw(d_tau, d_ssa, nx, ny, 100.0, 100.0, 50.0, d_alb, 0.6, 0.5, inc_dir, inc_dif, kn_grid, ppp, 11,
                                             independent_column=ic, cloud=d_cloud, band_lims=d_lims)

            times = []
            for _ in range(args.rounds):
                for _ in range(args.warmup):
                    run()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    run()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) / args.steps)
            ms = float(np.median(times))
            r = state["r"]
            photons = ppp*nx*ny*ngpt
            inc = float(np.sum(inc_dir))
            mean = lambda k: float(r[k].double().mean().item())
            out = dict(tool="raytracer_bench", dtype=dt, mode="independent_column" if ic else "3d", ms=round(ms, 3),
                       rounds_ms=[round(t, 3) for t in times], photons=photons, photons_per_s=round(photons / (ms*1e-3)),
                       n_capped=r["n_capped"], max_blocks_env=os.environ.get("RRX_RT_MAX_BLOCKS"), nx=nx, ny=ny, nz=nz, ngpt=ngpt,
                       photons_per_pixel=ppp, kn_grid=list(kn_grid),
                       mean_sfc_dn_over_inc=round((mean("sfc_dn_dir") + mean("sfc_dn_dif")) / inc, 5),
                       mean_tod_up_over_inc=round(mean("tod_up") / inc, 5), steps=args.steps, warmup=args.warmup, rounds=args.rounds,
                       device=torch.cuda.get_device_name(0))
            print(json.dumps(out), flush=True)
            lines.append(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
