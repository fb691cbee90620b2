#!/usr/bin/env python3
"""Cost of the LW quadrature angles, in one process on one GPU (bench.py's synthetic workload).

Solver stage: the LW solver on the inputs of one ResidentSolver step (tau, Planck fractions, band Planck functions, sfc_src of the
product chain), timed with device events around --steps launches after --warmup, for nmus = 1..4 angles in two modes:

  fused      rrx_lw_solver_noscat_fractions_angles: one kernel, each g-point read once and solved nmus times
  general    the only route for nmus > 1 before: lay_source / lev_source materialised (rrx_planck_sources_from_fractions), the general
             solver with do_broadband (one pass of the per-g-point kernel per angle, then rrx_sum_broadband twice)

Step: ResidentSolver(do_broadband=True) steps with 1 and 3 angles, timed as bench.py times them (wall clock between two
synchronisations). The modes take turns (--rounds times, each mode's median is reported). One JSON line per mode: ms, the ratio
general / fused of the same angle count (vs_general) and fused(nmus) / (nmus * fused(1)) (vs_one_angle).

  python tools/lw_angles_bench.py                               # C4 fp64 clear sky: 16 384 columns x 140 layers x 256 g-points
  python tools/lw_angles_bench.py --dtype f32
  python tools/lw_angles_bench.py --ncol 2048
  python tools/lw_angles_bench.py --dtype f32 --ncol 32768 --allsky
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=128*128)
    ap.add_argument("--nlay", type=int, default=140)
    ap.add_argument("--ngpt", type=int, default=256)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--allsky", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="solver stage only")
    args = ap.parse_args()

    import torch
    import rte_rrtmgp_cpp_amd as R
    from rte_rrtmgp_cpp_amd import synthetic, pipeline
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)      # (its atmosphere, not its main())

    np_dtype = np.float64 if args.dtype == "f64" else np.float32
    be = R.HipKernels(np_dtype, "cuda:0")
    nbnd = args.ngpt // 16
    kd_lw = be.upload_kdist(synthetic.make_kdist("lw", ngpt=args.ngpt, nbnd=nbnd))
    kd_sw = be.upload_kdist(synthetic.make_kdist("sw", ngpt=args.ngpt, nbnd=nbnd))
    a = argparse.Namespace(ncol=args.ncol, nlay=args.nlay, scaling="weak", top_at_1=False, allsky=args.allsky, col_spread=0.0)
    _, atm0 = bench.local_atmosphere(a, nbnd, 0, 1)
    atm = pipeline.upload_atmosphere(be, atm0.astype(np_dtype))
    luts = None
    if args.allsky:
        cast = lambda lut: be.upload_lut({k: (v.astype(np_dtype) if isinstance(v, np.ndarray) else v) for k, v in lut.items()})
        luts = (cast(synthetic.make_cloud_lut(nbnd, "lw")), cast(synthetic.make_cloud_lut(nbnd, "sw")))

    # the solver's inputs: those of one product step
    sv = {n: pipeline.ResidentSolver(be, kd_lw, kd_sw, atm, do_broadband=True, cloud_luts=luts, n_gauss_angles=n) for n in (1, 3)}
    sv[1].step()
    torch.cuda.synchronize()
    buf, ncol, nlay, ngpt = sv[1].lw, sv[1].secants.shape[2], args.nlay, args.ngpt
    top, emis = atm.top_at_1, sv[1].sfc_emis_gpt
    up, dn = be.empty((nlay+1, ncol)), be.empty((nlay+1, ncol))
    lay, lev = be.empty((ngpt, nlay, ncol)), be.empty((ngpt, nlay+1, ncol))
    gauss_Ds = be.asarray(pipeline.GAUSS_DS)
    sec = {n: be.lw_secants_array(ncol, ngpt, n, pipeline.MAX_GAUSS_PTS, gauss_Ds) for n in (1, 2, 3, 4)}
    wts = {n: be.asarray(np.ascontiguousarray(pipeline.GAUSS_WTS[n-1, :n])) for n in (1, 2, 3, 4)}

    def fused(n):
        return lambda: be.lw_solver_noscat_fractions_angles(top, kd_lw, sec[n], wts[n], buf["tau"], buf, emis, flux_up=up, flux_dn=dn)

    def general(n):
        def run():
            be.planck_sources_from_fractions(kd_lw, buf, lay, lev)
            be.lw_solver_noscat(top, sec[n], wts[n], buf["tau"], lay, lev, emis, buf["sfc_src"], do_broadband=True)
        return run

    def timed_device(fn):
        for _ in range(args.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    def timed_wall(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    modes = [("solver", m, n, f(n), timed_device) for n in (1, 2, 3, 4) for m, f in (("fused", fused), ("general", general))]
    if not args.no_step:
        modes += [("step", "broadband", n, sv[n].step, timed_wall) for n in (1, 3)]
    times = {(s, m, n): [] for s, m, n, _, _ in modes}
    for _ in range(args.rounds):
        for s, m, n, fn, timer in modes:
            times[(s, m, n)].append(timer(fn))
    med = {k: float(np.median(v)) for k, v in times.items()}
    for s, m, n, _, _ in modes:
        ms = med[(s, m, n)]
        out = {"stage": s, "mode": m, "nmus": n, "ms": round(ms, 3), "rounds_ms": [round(t, 3) for t in times[(s, m, n)]]}
        if s == "solver" and m == "fused":
            out["vs_general"] = round(med[(s, "general", n)] / ms, 3)
            out["vs_one_angle"] = round(ms / (n * med[(s, "fused", 1)]), 3)
        if s == "step":
            out["vs_one_angle_step"] = round(ms / med[(s, m, 1)], 3)
        out.update(dtype=args.dtype, ncol=args.ncol, nlay=args.nlay, ngpt=args.ngpt, allsky=args.allsky, steps=args.steps,
                   warmup=args.warmup, device=torch.cuda.get_device_name(0))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
