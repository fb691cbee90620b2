#!/usr/bin/env python3
"""Throughput of the two ray tracers with a tabulated cloud phase function (rrx_raytracer_sw_phase, rrx_raytracer_bw_phase; DESIGN
4.16) beside the Henyey-Greenstein entries, in one process on one GPU, on the broken-cloud field of tools/raytracer_bench.py and
the two cameras of tools/raytracer_bw_bench.py (128 x 128 x 32 cells, 256 x 256 pixels, 4 g-points).

The table: 1 800 nodes (phase_tables.nodes, spacing shrinking towards +1) x 20 radii 2.5 + 1 i, HG(0.85) at every radius, so that
the tabulated runs estimate what the Henyey-Greenstein runs estimate (the means are printed); the cells' radius is a smooth field
across the whole grid, so that neighbouring lanes read different tables. fp64 and fp32, device events around --steps calls after
--warmup, --rounds times, the median. Counted by the numpy restatements (tests/raytracer_ref.py, raytracer_bw_ref.py) on the
32 x 32 cut of the field, g-point 0: the cloud scatterings per photon / ray, from which the extra time per tabulated cloud
scattering follows (an aggregate over the whole machine, not a latency). --lib times the Henyey-Greenstein entries of another build
of librrx_hip.so (the parent commit's) in the same way. One JSON line each, printed and appended to --out. A record, not a target.

  python tools/raytracer_phase_bench.py
  python tools/raytracer_phase_bench.py --lib /path/to/parent/librrx_hip.so --label parent
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NMU, NRE, RE0, DRE, G = 1800, 20, 2.5, 1.0, 0.85


def radius_field(nx, ny, nz):
    """(nz, ncol): 2 .. 23 micron, smooth in x and y, rising with height: below, across and above the grid"""
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny))
    base = 12.5 + 8.0*np.sin(2*np.pi*ix/nx)*np.cos(2*np.pi*iy/ny)
    return np.ascontiguousarray(base.reshape(1, -1) + np.linspace(-2.5, 2.5, nz)[:, None])


def scatterings_on_cut(C, tau, ssa, cloud, lims, albedo, re, nx, nz, cut, table_np):
    import raytracer_ref as R
    import raytracer_bw_ref as B
    from raytracer_bw_bench import cameras, DX, DY, DZ, MU0, AZIMUTH, SEED
    col = (np.arange(cut)[None, :] + nx*np.arange(cut)[:, None]).reshape(-1)
    take = lambda a: np.ascontiguousarray(a[..., col])
    sc = R.Scene(nx=cut, ny=cut, nz=nz, dx=DX, dy=DY, dz=DZ, tau=take(tau), ssa=take(ssa), sfc_albedo=take(albedo), mu0=MU0, azimuth=AZIMUTH,
                 inc_dir=np.full(tau.shape[0], 100.0), inc_dif=np.zeros(tau.shape[0]), kn_grid=(max(cut//8, 1), max(cut//8, 1), max(nz//4, 1)),
                 cloud=tuple(take(c) for c in cloud), band_lims=lims.reshape(-1, 2), top_at_1=False, seed=SEED)
    table_np.cld_re = take(re)
    n = 4*cut*cut
    f = R.trace_counts(sc, 0, 0, n, table=table_np)
    out = {"forward": dict(photons=n, events_per_photon=round(f["events"]/n, 3), cloud_scatterings_per_photon=round(f["cloud_scatterings"]/n, 3))}
    for name, cam in cameras(C, cut, cut, nz, cut, cut).items():
        b = B.trace_counts_bw(sc, cam, 0, 0, 4*cam.npix, table=table_np)
        out[name] = dict(rays=4*cam.npix, events_per_ray=round(b["events"]/(4*cam.npix), 3),
                         cloud_scatterings_per_ray=round(b["cloud_scatterings"]/(4*cam.npix), 3))
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
    ap.add_argument("--photons-per-pixel", type=int, default=64)
    ap.add_argument("--cut", type=int, default=32, help="side of the corner the restatement counts on (0: skip)")
    ap.add_argument("--dtype", default="both", choices=["both", "f64", "f32"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of librrx_hip.so: only its Henyey-Greenstein entries are timed")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raytracer_phase_bench.txt"))
    args = ap.parse_args()

    import torch
    import rte_rrtmgp_cpp_amd as R
    from rte_rrtmgp_cpp_amd import camera as C, phase_tables, hip_kernels
    from raytracer_bench import broken_cloud_field
    from raytracer_bw_bench import cameras, DX, DY, DZ, MU0, AZIMUTH, SEED
    if args.lib is not None:
        hip_kernels.LIB_PATH = os.path.abspath(args.lib)

    nx, ny, nz, ngpt = args.nx, args.ny, args.nz, args.ngpt
    kn_grid = (max(nx//8, 1), max(ny//8, 1), max(nz//4, 1))
    tau, ssa, cloud, lims, albedo = broken_cloud_field(nx, ny, nz, ngpt)
    re = radius_field(nx, ny, nz)
    mu = phase_tables.nodes(NMU)
    raw = np.broadcast_to(phase_tables.henyey_greenstein(mu, G), (1, NRE, NMU)).copy()
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
        out = dict(tool="raytracer_phase_bench", build=args.label, **out)
        out.update(nx=nx, ny=ny, nz=nz, ngpt=ngpt, steps=args.steps, warmup=args.warmup, rounds=args.rounds, device=torch.cuda.get_device_name(0))
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))

    for dt in (("f64", "f32") if args.dtype == "both" else (args.dtype,)):
        be = R.HipKernels(np.float64 if dt == "f64" else np.float32, "cuda:0")
        A = be.asarray
        d_tau, d_ssa, d_cloud, d_lims, d_alb = A(tau), A(ssa), tuple(A(c) for c in cloud), A(lims), A(albedo)
        forms = [("hg", None)]
        if args.lib is None:
            forms.append((f"table {NMU} x {NRE}", phase_tables.build(be, mu, raw, RE0, DRE).with_radius(A(re))))
        for form, phase in forms:
            kw = dict(phase=phase) if phase is not None else {}
            state = {}

            def run_forward():
                state["r"] = be.raytracer_sw(d_tau, d_ssa, nx, ny, DX, DY, DZ, d_alb, MU0, AZIMUTH, inc_dir, np.zeros(ngpt), kn_grid,
                                             args.photons_per_pixel, SEED, cloud=d_cloud, band_lims=d_lims, **kw)

            ms, rounds_ms = timed(run_forward)
            r = state["r"]
            photons = args.photons_per_pixel*nx*ny*ngpt
            mean = lambda k: float(r[k].double().mean().item())
            emit(dict(dtype=dt, tracer="forward 3d", phase=form, ms=round(ms, 3), rounds_ms=rounds_ms, photons=photons,
                      photons_per_s=round(photons/(ms*1e-3)), n_capped=r["n_capped"],
                      mean_sfc_dn_over_inc=round((mean("sfc_dn_dir") + mean("sfc_dn_dif"))/float(inc_dir.sum()), 5),
                      mean_tod_up_over_inc=round(mean("tod_up")/float(inc_dir.sum()), 5)))
            for name, cam in cameras(C, nx, ny, nz, args.npx, args.npy).items():
                def run():
                    state["r"] = be.raytracer_bw(d_tau, d_ssa, nx, ny, DX, DY, DZ, d_alb, MU0, AZIMUTH, inc_dir, kn_grid, cam,
                                                 args.rays_per_pixel, SEED, cloud=d_cloud, band_lims=d_lims, **kw)

                ms, rounds_ms = timed(run)
                r = state["r"]
                rays = args.rays_per_pixel*cam.npix*ngpt
                emit(dict(dtype=dt, tracer="backward " + name, phase=form, ms=round(ms, 3), rounds_ms=rounds_ms, rays=rays,
                          rays_per_s=round(rays/(ms*1e-3)), n_capped=r["n_capped"], n_clamped=r["n_clamped"],
                          mean_radiance=round(float(r["radiance"].double().mean().item()), 4)))
    if args.cut > 0 and args.lib is None:
        import raytracer_phase_ref as P
        counts = scatterings_on_cut(C, tau, ssa, cloud, lims, albedo, re, nx, nz, args.cut, P.build_tables(mu, raw, np.float64, RE0, DRE))
        emit(dict(restatement_on_cut=args.cut, g_point=0, **counts))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
