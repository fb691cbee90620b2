#!/usr/bin/env python3
"""Throughput of the backward Monte Carlo ray tracer (rrx_raytracer_bw), in one process on one GPU, on the
broken-cloud field of tools/raytracer_bench.py (128 x 128 x 32 cells of 100 x 100 x 50 m, k_null blocks of 8 x 8 x 4 cells, albedo
0.2, mu0 = 0.6, 4 g-points with equal incident flux).

Two sensors of 256 x 256 pixels: a perspective camera above the cloud layer in the middle of the domain, looking forward and down,
and the nadir orthographic view from the top. fp64 and fp32, device events around --steps calls after --warmup, --rounds times; the
median is reported as rays per second and ms per call. Beside them, from the same session, the forward tracer's photons per second
on the same field (3-D mode, the configuration of tools/raytracer_bench.py), and, counted by the numpy restatement
(tests/raytracer_bw_ref.py) on the 32 x 32 cut of the field with cameras of 32 x 32 pixels, the events and the sun-walk cells per
ray: the two kinds of pass through the kernel's one loop. One JSON line each, printed and appended to --out (default
profiles/raytracer_bw_bench.txt). A record, not a target.

  python tools/raytracer_bw_bench.py
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

DX, DY, DZ, MU0, AZIMUTH, SEED = 100.0, 100.0, 50.0, 0.6, 0.5, 11


def cameras(C, nx, ny, nz, npx, npy):
    return {"perspective": C.perspective(npx, npy, (0.5*nx*DX, 0.5*ny*DY, 0.9*nz*DZ), yaw=0.8, pitch=-0.5, fov=math.radians(60.)),
            "orthographic": C.orthographic(npx, npy)}


def restatement_counts(C, tau, ssa, cloud, lims, albedo, nx, ny, nz, cut, rays_per_pixel):
    """events and sun-walk cells per ray on the cut x cut corner of the field, g-point 0, float64"""
    import raytracer_ref as R
    import raytracer_bw_ref as B
    col = (np.arange(cut)[None, :] + nx*np.arange(cut)[:, None]).reshape(-1)
    take = lambda a: np.ascontiguousarray(a[..., col])
    sc = R.Scene(nx=cut, ny=cut, nz=nz, dx=DX, dy=DY, dz=DZ, tau=take(tau), ssa=take(ssa), sfc_albedo=take(albedo), mu0=MU0, azimuth=AZIMUTH,
                 inc_dir=np.full(tau.shape[0], 100.0), inc_dif=np.zeros(tau.shape[0]), kn_grid=(max(cut//8, 1), max(cut//8, 1), max(nz//4, 1)),
                 cloud=tuple(take(c) for c in cloud), band_lims=lims.reshape(-1, 2), top_at_1=False, seed=SEED)
    out = {}
    for name, cam in cameras(C, cut, cut, nz, cut, cut).items():
        nrays = rays_per_pixel*cam.npix
        c = B.trace_counts_bw(sc, cam, 0, 0, nrays)
        out[name] = dict(rays=nrays, events_per_ray=round(c["events"]/nrays, 3), walk_cells_per_ray=round(c["walk_cells"]/nrays, 3),
                         deposits_per_ray=round(int(c["n_dep"].sum())/nrays, 3), n_capped=c["n_capped"], walk_bound=B.max_walk(sc))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=128)
    ap.add_argument("--ny", type=int, default=128)
    ap.add_argument("--nz", type=int, default=32)
    ap.add_argument("--ngpt", type=int, default=4)
    ap.add_argument("--npx", type=int, default=256)
    ap.add_argument("--npy", type=int, default=256)
    ap.add_argument("--rays-per-pixel", type=int, default=16)
    ap.add_argument("--photons-per-pixel", type=int, default=64, help="of the forward tracer's line")
    ap.add_argument("--cut", type=int, default=32, help="side of the corner the restatement counts on (0: skip)")
    ap.add_argument("--dtype", default="both", choices=["both", "f64", "f32"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raytracer_bw_bench.txt"))
    args = ap.parse_args()

    import torch
    import rte_rrtmgp_cpp_amd as R
    from rte_rrtmgp_cpp_amd import camera as C
    from raytracer_bench import broken_cloud_field

    nx, ny, nz, ngpt, rpp = args.nx, args.ny, args.nz, args.ngpt, args.rays_per_pixel
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
                   max_blocks_env=os.environ.get("RRX_RT_MAX_BLOCKS"), device=torch.cuda.get_device_name(0))
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))

    for dt in (("f64", "f32") if args.dtype == "both" else (args.dtype,)):
        be = R.HipKernels(np.float64 if dt == "f64" else np.float32, "cuda:0")
        A = be.asarray
        d_tau, d_ssa, d_cloud, d_lims, d_alb = A(tau), A(ssa), tuple(A(c) for c in cloud), A(lims), A(albedo)
        for name, cam in cameras(C, nx, ny, nz, args.npx, args.npy).items():
            state = {}

            def run():
                state["r"] = be.raytracer_bw(d_tau, d_ssa, nx, ny, DX, DY, DZ, d_alb, MU0, AZIMUTH, inc_dir, kn_grid, cam, rpp, SEED,
                                             cloud=d_cloud, band_lims=d_lims)

            ms, rounds_ms = timed(run)
            r = state["r"]
            rays = rpp*cam.npix*ngpt
            emit(dict(tool="raytracer_bw_bench", dtype=dt, sensor=name, ms=round(ms, 3), rounds_ms=rounds_ms, rays=rays,
                      rays_per_s=round(rays / (ms*1e-3)), n_capped=r["n_capped"], n_clamped=r["n_clamped"], npx=cam.npx, npy=cam.npy,
                      rays_per_pixel=rpp, mean_radiance=round(float(r["radiance"].double().mean().item()), 4),
                      max_radiance=round(float(r["radiance"].double().max().item()), 4)))
        state = {}

        def run_forward():
            state["r"] = be.raytracer_sw(d_tau, d_ssa, nx, ny, DX, DY, DZ, d_alb, MU0, AZIMUTH, inc_dir, np.zeros(ngpt), kn_grid,
                                         args.photons_per_pixel, SEED, cloud=d_cloud, band_lims=d_lims)

        ms, rounds_ms = timed(run_forward)
        photons = args.photons_per_pixel*nx*ny*ngpt
        emit(dict(tool="raytracer_bw_bench", dtype=dt, sensor="(forward tracer, 3d, same session)", ms=round(ms, 3), rounds_ms=rounds_ms,
                  photons=photons, photons_per_s=round(photons / (ms*1e-3)), n_capped=state["r"]["n_capped"],
                  photons_per_pixel=args.photons_per_pixel))
    if args.cut > 0:
        counts = restatement_counts(C, tau, ssa, cloud, lims, albedo, nx, ny, nz, args.cut, 4)
        emit(dict(tool="raytracer_bw_bench", restatement_on_cut=args.cut, cameras_of_pixels=[args.cut, args.cut], g_point=0, **counts))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
