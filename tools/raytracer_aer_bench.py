#!/usr/bin/env python3
"""Throughput of both ray tracers with aerosol as a third scattering species (rrx_raytracer_sw_aer, rrx_raytracer_bw_aer, DESIGN
4.18), in one process on one GPU, on the scenes of tools/raytracer_bg_bench.py: the broken-cloud field of tools/raytracer_bench.py
(128 x 128 x 32 cells of 100 x 100 x 50 m, k_null blocks of 8 x 8 x 4 cells, albedo 0.2, mu0 = 0.6, 4 g-points with equal incident
flux) under its 8 clear background layers.

Forms, for the forward tracer (3-D mode) and the backward tracer's two sensors of tools/raytracer_bw_bench.py, each in fp64 and fp32:
  plain the entries without a background (rrx_raytracer_sw, rrx_raytracer_bw): the instantiations without BG, for an A/B of those
  bg    the _bg entry: no aerosol, the BG instantiations
  null  the _aer entry with every aerosol pointer NULL: the same instantiations (the figure must lie within the spread of `bg`)
  haze  the _aer entry with a haze: aerosol optical depth 0.3 per g-point over the lowest 16 layers of every column (tau_a 0.3/16 per
        cell, ssa_a 0.92, g_a 0.7) and 0.05 in the lowest background layer
--library names another build of librrx_hip.so (the parent commit's, say) for an A/B on the same box: only `plain` and `bg` can run there.
Device events around --steps calls after --warmup, --rounds times; the median is reported, the rounds are kept. One JSON line each,
printed and appended to --out (default profiles/raytracer_aer_bench.txt). A record, not a target.

  python tools/raytracer_aer_bench.py
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
    ap.add_argument("--forms", default="bg,null,haze")
    ap.add_argument("--library", default=None)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raytracer_aer_bench.txt"))
    args = ap.parse_args()

    import torch
    import rte_rrtmgp_cpp_amd as R
    from rte_rrtmgp_cpp_amd import camera as C, hip_kernels
    from raytracer_bench import broken_cloud_field
    from raytracer_bw_bench import cameras
    from raytracer_bg_bench import Background

    forms = args.forms.split(",")
    if args.library is not None:
        if not set(forms) <= {"plain", "bg"}:
            sys.exit("--library: another build has only the plain and bg forms (--forms plain,bg)")
        hip_kernels.LIB_PATH = os.path.abspath(args.library)

    nx, ny, nz, ngpt, rpp, ppp = args.nx, args.ny, args.nz, args.ngpt, args.rays_per_pixel, args.photons_per_pixel
    kn_grid = (max(nx//8, 1), max(ny//8, 1), max(nz//4, 1))
    tau, ssa, cloud, lims, albedo = broken_cloud_field(nx, ny, nz, ngpt)
    nbnd = int(np.asarray(lims).shape[0])
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
        out.update(nx=nx, ny=ny, nz=nz, ngpt=ngpt, nbg=args.nbg, kn_grid=list(kn_grid), steps=args.steps, warmup=args.warmup, rounds=args.rounds,
                   library=args.label, device=torch.cuda.get_device_name(0))
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))

    for dt in (("f64", "f32") if args.dtype == "both" else (args.dtype,)):
        be = R.HipKernels(np.float64 if dt == "f64" else np.float32, "cuda:0")
        A = be.asarray
        d_tau, d_ssa, d_cloud, d_lims, d_alb = A(tau), A(ssa), tuple(A(c) for c in cloud), A(lims), A(albedo)
        bg = Background(be, args.nbg, ngpt)
        # the haze: the lowest half of the grid (tau, ssa are (ngpt, nz, ncol); the field's layer 0 is the lowest), one layer aloft
        low = max(nz//2, 1)
        at = np.zeros((nbnd, nz, nx*ny)); at[:, :low] = 0.3/low
        haze = tuple(A(a) for a in (at, np.full_like(at, 0.92), np.full_like(at, 0.7)))
        bt = np.zeros((nbnd, args.nbg)); bt[:, 0] = 0.05
        hazy_bg = Background(be, args.nbg, ngpt)
        hazy_bg.aerosol = tuple(A(a) for a in (bt, np.full_like(bt, 0.92), np.full_like(bt, 0.7)))
        scene = (d_tau, d_ssa, nx, ny, DX, DY, DZ, d_alb, MU0, AZIMUTH, inc_dir)
        common = dict(cloud=d_cloud, band_lims=d_lims)
        extra = {"bg": dict(background=bg), "null": dict(background=bg, aerosol=(None, None, None)), "haze": dict(background=hazy_bg, aerosol=haze)}

        for form in forms:
            state = {}

            def run():
                if form == "plain":
                    state["r"] = be.raytracer_sw(*scene, np.zeros(ngpt), kn_grid, ppp, SEED, **common)
                else:
                    state["r"] = be.raytracer_sw_bg(*scene, np.zeros(ngpt), kn_grid, ppp, SEED, **common, **extra[form])

            ms, rounds_ms = timed(run)
            r = state["r"]
            photons = ppp*nx*ny*ngpt
            inc = float(np.sum(inc_dir))
            mean = lambda k: float(r[k].double().mean().item())
            emit(dict(tool="raytracer_aer_bench", tracer="forward 3d", dtype=dt, form=form, ms=round(ms, 3), rounds_ms=rounds_ms, photons=photons,
                      photons_per_s=round(photons / (ms*1e-3)), n_capped=r["n_capped"], photons_per_pixel=ppp,
                      mean_sfc_dn_over_inc=round((mean("sfc_dn_dir") + mean("sfc_dn_dif")) / inc, 5),
                      mean_toa_up_over_inc=round(mean("tod_up" if form == "plain" else "toa_up") / inc, 5)))

        for name, cam in cameras(C, nx, ny, nz, args.npx, args.npy).items():
            for form in forms:
                state = {}

                def run():
                    if form == "plain":
                        state["r"] = be.raytracer_bw(*scene, kn_grid, cam, rpp, SEED, **common)
                    else:
                        state["r"] = be.raytracer_bw_bg(*scene, kn_grid, cam, rpp, SEED, **common, **extra[form])

                ms, rounds_ms = timed(run)
                r = state["r"]
                rays = rpp*cam.npix*ngpt
                emit(dict(tool="raytracer_aer_bench", tracer="backward", sensor=name, dtype=dt, form=form, ms=round(ms, 3), rounds_ms=rounds_ms,
                          rays=rays, rays_per_s=round(rays / (ms*1e-3)), n_capped=r["n_capped"], n_clamped=r["n_clamped"], npx=cam.npx,
                          npy=cam.npy, rays_per_pixel=rpp, mean_radiance=round(float(r["radiance"].double().mean().item()), 4)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
