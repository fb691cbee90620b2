#!/usr/bin/env python3
"""Cost of the surface-temperature Jacobian of the LW upward flux, in one process on one GPU (bench.py's synthetic workload).

Solver stage: the LW solver on the inputs of one ResidentSolver step (tau, Planck fractions, band Planck functions, sfc_src and
sfc_src_jac of the product chain), timed with device events around --steps launches after --warmup, in three modes:

  fluxes     rrx_lw_solver_noscat_fractions: the broadband fluxes alone (the stage of bench.py's step)
  jacobian   rrx_lw_solver_noscat_fractions_jac: the same fluxes plus flux_up_jac from one solve
  general    the only route before: lay_source / lev_source materialised (rrx_planck_sources_from_fractions), the general solver with
             do_broadband and do_jacobians (per-g-point Jacobian), then rrx_sum_broadband of the Jacobian

Step: ResidentSolver(do_broadband=True) steps with and without jacobian=True, timed as bench.py times them (wall clock between two
synchronisations). The modes take turns (--rounds times, each mode's median is reported). One JSON line per mode.

  python tools/jacobian_bench.py                                # C4 fp64 clear sky: 16 384 columns x 140 layers x 256 g-points
  python tools/jacobian_bench.py --dtype f32
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
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
    a = argparse.Namespace(ncol=args.ncol, nlay=args.nlay, scaling="weak", top_at_1=False, allsky=False, col_spread=0.0)
    _, atm0 = bench.local_atmosphere(a, nbnd, 0, 1)
    atm = pipeline.upload_atmosphere(be, atm0.astype(np_dtype))

    # the solver's inputs: those of one product step
    sv = pipeline.ResidentSolver(be, kd_lw, kd_sw, atm, do_broadband=True, jacobian=True)
    sv.step()
    torch.cuda.synchronize()
    buf, ncol, nlay, ngpt = sv.lw, sv.secants.shape[2], args.nlay, args.ngpt
    top = atm.top_at_1
    up, dn, jac = be.empty((nlay+1, ncol)), be.empty((nlay+1, ncol)), be.empty((nlay+1, ncol))

    def fluxes():
        be.lw_solver_noscat_fractions(top, kd_lw, sv.secants, sv.weights, buf["tau"], buf, sv.sfc_emis_gpt, flux_up=up, flux_dn=dn)

    def jacobian():
        be.lw_solver_noscat_fractions_jac(top, kd_lw, sv.secants, sv.weights, buf["tau"], buf, sv.sfc_emis_gpt, flux_up=up, flux_dn=dn,
                                          flux_up_jac=jac)

    lay, lev = be.empty((ngpt, nlay, ncol)), be.empty((ngpt, nlay+1, ncol))

    def general():
        be.planck_sources_from_fractions(kd_lw, buf, lay, lev)
        r = be.lw_solver_noscat(top, sv.secants, sv.weights, buf["tau"], lay, lev, sv.sfc_emis_gpt, buf["sfc_src"], do_broadband=True,
                                do_jacobians=True, sfc_src_jac=buf["sfc_src_jac"])
        be.sum_broadband(r["flux_up_jac"], out=jac)

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

    step_plain = pipeline.ResidentSolver(be, kd_lw, kd_sw, atm, do_broadband=True).step
    step_jac = sv.step
    modes = [("solver", "fluxes", fluxes, timed_device), ("solver", "jacobian", jacobian, timed_device),
             ("solver", "general", general, timed_device),
             ("step", "broadband", step_plain, timed_wall), ("step", "jacobian", step_jac, timed_wall)]
    times = {(s, m): [] for s, m, _, _ in modes}
    for _ in range(args.rounds):
        for s, m, fn, timer in modes:
            times[(s, m)].append(timer(fn))
    ref = {s: float(np.median(times[(s, m)])) for s, m in (("solver", "fluxes"), ("step", "broadband"))}
    for s, m, _, _ in modes:
        ms = float(np.median(times[(s, m)]))
        out = {"stage": s, "mode": m, "ms": round(ms, 3), "rounds_ms": [round(t, 3) for t in times[(s, m)]],
               "vs_plain": round(ms / ref[s], 3), "dtype": args.dtype, "ncol": args.ncol, "nlay": args.nlay, "ngpt": args.ngpt,
               "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
