#!/usr/bin/env python3
"""Throughput of both ray tracers with a background atmosphere (rrx_raytracer_sw_bg, rrx_raytracer_bw_bg), in one
process on one GPU, on the broken-cloud field of tools/raytracer_bench.py (128 x 128 x 32 cells of 100 x 100 x 50 m, k_null blocks of
8 x 8 x 4 cells, albedo 0.2, mu0 = 0.6, 4 g-points with equal incident flux).

The background: --nbg clear layers (default 8) above the 1.6 km grid, thickening upward from 0.5 km to 6 km, with the scattering
gas of the grid thinning upward (tau 0.02 .. 0.003 per layer and g-point step, ssa 0.6). For the forward tracer (3-D mode) and the
backward tracer's two sensors of tools/raytracer_bw_bench.py, each in fp64 and fp32, one line with the background and one without
from the same session: the existing entry, and the _bg entry with nbg = 0 (the BG kernel on the medium without layers). Device
events around --steps calls after --warmup, --rounds times; the median is reported. One JSON line each, printed and appended to
--out (default profiles/raytracer_bg_bench.txt). A record, not a target.

  python tools/raytracer_bg_bench.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DX, DY, DZ, MU0, AZIMUTH, SEED = 100.0, 100.0, 50.0, 0.6, 0.5, 11


class Background:
    def __init__(self, be, nbg, ngpt):
        self.dz = np.linspace(500.0, 6000.0, nbg).astype(be.np_dtype)
        tau = np.linspace(0.02, 0.003, nbg)[None, :] * (1.0 + 0.5*np.arange(ngpt))[:, None]
        self.tau, self.ssa, self.cloud = be.asarray(tau), be.asarray(np.full((ngpt, nbg), 0.6)), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=128)
    ap.add_argument("--ny", type=int, default=128)
    ap.add_argument("--nz", type=int, default=32)
    ap.add_argument("--ngpt", type=int, default=4)
    ap.add_argument("--nbg", type=int, default=8)
    ap.add_argument("--npx", type=int, default=256)
    ap.add_argument("--npy", type=int, default=256)
    ap.add_argument("--rays-per-pixel", type=int, default=16)
    ap.add_argument("--photons-per-pixel", type=int, default=64)
    ap.add_argument("--dtype", default="both", choices=["both", "f64", "f32"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raytracer_bg_bench.txt"))
    args = ap.parse_args()

    import torch
    import rte_rrtmgp_cpp_amd as R
    from rte_rrtmgp_cpp_amd import camera as C
    from raytracer_bench import broken_cloud_field
    from raytracer_bw_bench import cameras

    nx, ny, nz, ngpt, rpp, ppp = args.nx, args.ny, args.nz, args.ngpt, args.rays_per_pixel, args.photons_per_pixel
    kn_grid = (max(nx//8, 1), max(ny//8, 1), max(nz//4, 1))
    tau, ssa, cloud, lims, albedo = broken_cloud_field(nx, ny, nz, ngpt)
    inc_dir = np.full(ngpt, 100.0)
    lines = []

    def timed(run):
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
        return float(np.median(times)), [round(t, 3) for t in times]

    def emit(out):
        out.update(nx=nx, ny=ny, nz=nz, ngpt=ngpt, kn_grid=list(kn_grid), steps=args.steps, warmup=args.warmup, rounds=args.rounds,
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))

    for dt in (("f64", "f32") if args.dtype == "both" else (args.dtype,)):
        be = R.HipKernels(np.float64 if dt == "f64" else np.float32, "cuda:0")
        A = be.asarray
        d_tau, d_ssa, d_cloud, d_lims, d_alb = A(tau), A(ssa), tuple(A(c) for c in cloud), A(lims), A(albedo)
        bg = Background(be, args.nbg, ngpt)
        scene = (d_tau, d_ssa, nx, ny, DX, DY, DZ, d_alb, MU0, AZIMUTH, inc_dir)
        common = dict(cloud=d_cloud, band_lims=d_lims)
        forms = (("existing entry", None), ("bg entry, nbg = 0", 0), (f"bg entry, nbg = {args.nbg}", args.nbg))

        for form, nbg in forms:
            state = {}

            def run():
                if nbg is None:
                    state["r"] = be.raytracer_sw(*scene, np.zeros(ngpt), kn_grid, ppp, SEED, **common)
                else:
                    state["r"] = be.raytracer_sw_bg(*scene, np.zeros(ngpt), kn_grid, ppp, SEED, background=bg if nbg else None, **common)

            ms, rounds_ms = timed(run)
            r = state["r"]
            photons = ppp*nx*ny*ngpt
            inc = float(np.sum(inc_dir))
            mean = lambda k: float(r[k].double().mean().item())
            out = dict(tool="raytracer_bg_bench", tracer="forward 3d", dtype=dt, form=form, ms=round(ms, 3), rounds_ms=rounds_ms, photons=photons,
                       photons_per_s=round(photons / (ms*1e-3)), n_capped=r["n_capped"], photons_per_pixel=ppp,
                       mean_sfc_dn_over_inc=round((mean("sfc_dn_dir") + mean("sfc_dn_dif")) / inc, 5),
                       mean_tod_up_over_inc=round(mean("tod_up") / inc, 5))
            if nbg:
                out.update(mean_toa_up_over_inc=round(mean("toa_up") / inc, 5),
                           mean_tod_dn_over_inc=round((mean("tod_dn_dir") + mean("tod_dn_dif")) / inc, 5))
            emit(out)

        for name, cam in cameras(C, nx, ny, nz, args.npx, args.npy).items():
            for form, nbg in forms:
                state = {}

                def run():
                    if nbg is None:
                        state["r"] = be.raytracer_bw(*scene, kn_grid, cam, rpp, SEED, **common)
                    else:
                        state["r"] = be.raytracer_bw_bg(*scene, kn_grid, cam, rpp, SEED, background=bg if nbg else None, **common)

                ms, rounds_ms = timed(run)
                r = state["r"]
                rays = rpp*cam.npix*ngpt
                emit(dict(tool="raytracer_bg_bench", tracer="backward", sensor=name, dtype=dt, form=form, ms=round(ms, 3), rounds_ms=rounds_ms,
                          rays=rays, rays_per_s=round(rays / (ms*1e-3)), n_capped=r["n_capped"], n_clamped=r["n_clamped"], npx=cam.npx,
                          npy=cam.npy, rays_per_pixel=rpp, mean_radiance=round(float(r["radiance"].double().mean().item()), 4)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
