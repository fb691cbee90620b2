#!/usr/bin/env python3
"""Cost of by-band fluxes, in one process on one GPU: ResidentSolver steps (LW+SW, bench.py's synthetic workload) timed the way bench.py
times them -- W warm-up steps, then K steps between two torch.cuda.synchronize() calls, wall clock -- in three modes:

  broadband   ResidentSolver(do_broadband=True): the headline step (fused solvers, seven broadband arrays)
  byband      ResidentSolver(do_broadband=True, byband=True): the fused solvers' by-band form (band sums, band net, broadband arrays)
  per-gpoint  ResidentSolver(do_broadband=False) + sum_byband / net_byband_full of its per-g-point fluxes: the by-band cost before

The modes take turns (--rounds times, each mode's median is reported) so that a drift of the box shows in all of them alike. One JSON
line per mode.

  python tools/byband_bench.py                                  # C4 fp64 clear sky: 16 384 columns x 140 layers x 256 g-points
  python tools/byband_bench.py --ncol 2048
  python tools/byband_bench.py --dtype f32 --allsky --ncol 32768
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
    ap.add_argument("--nbnd", type=int, default=0, help="bands of the synthetic k-distributions (default ngpt/16, as bench.py)")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--allsky", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default="broadband,byband,per-gpoint")
    args = ap.parse_args()

    import torch
    import rte_rrtmgp_cpp_amd as R
    from rte_rrtmgp_cpp_amd import synthetic, pipeline
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)      # (its atmosphere, not its main())

    np_dtype = np.float64 if args.dtype == "f64" else np.float32
    be = R.HipKernels(np_dtype, "cuda:0")
    nbnd = args.nbnd if args.nbnd else args.ngpt // 16
    kd_lw = be.upload_kdist(synthetic.make_kdist("lw", ngpt=args.ngpt, nbnd=nbnd))
    kd_sw = be.upload_kdist(synthetic.make_kdist("sw", ngpt=args.ngpt, nbnd=nbnd))
    luts = None
    if args.allsky:
        cast = lambda lut: be.upload_lut({k: (v.astype(np_dtype) if isinstance(v, np.ndarray) else v) for k, v in lut.items()})
        luts = (cast(synthetic.make_cloud_lut(nbnd, "lw")), cast(synthetic.make_cloud_lut(nbnd, "sw")))
    a = argparse.Namespace(ncol=args.ncol, nlay=args.nlay, scaling="weak", top_at_1=False, allsky=args.allsky, col_spread=0.0)
    _, atm0 = bench.local_atmosphere(a, nbnd, 0, 1)
    atm = pipeline.upload_atmosphere(be, atm0.astype(np_dtype))

    def make(mode):
        if mode == "broadband":
            s = pipeline.ResidentSolver(be, kd_lw, kd_sw, atm, do_broadband=True, cloud_luts=luts)
            return s.step
        if mode == "byband":
            s = pipeline.ResidentSolver(be, kd_lw, kd_sw, atm, do_broadband=True, cloud_luts=luts, byband=True)
            return s.step
        s = pipeline.ResidentSolver(be, kd_lw, kd_sw, atm, do_broadband=False, cloud_luts=luts)
        bl, bs = kd_lw.band_lims_gpt, kd_sw.band_lims_gpt

        def step():
            F = s.step()
            s.bnd = (be.sum_byband(s.lw["gpt_up"], bl), be.sum_byband(s.lw["gpt_dn"], bl), be.net_byband_full(s.lw["gpt_dn"], s.lw["gpt_up"], bl),
                     be.sum_byband(s.sw["gpt_up"], bs), be.sum_byband(s.sw["gpt_dn"], bs), be.sum_byband(s.sw["gpt_dir"], bs),
                     be.net_byband_full(s.sw["gpt_dn"], s.sw["gpt_up"], bs))
            return F
        return step

    modes = [m for m in args.modes.split(",") if m]
    times = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            step = make(m)
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            times[m].append((time.perf_counter() - t0) / args.steps * 1e3)
            del step
            torch.cuda.empty_cache()
    ref = float(np.median(times["broadband"])) if "broadband" in times else None
    for m in modes:
        ms = float(np.median(times[m]))
        out = {"mode": m, "ms_per_step": round(ms, 3), "rounds_ms": [round(t, 3) for t in times[m]],
               "vs_broadband": round(ms / ref, 3) if ref else None, "dtype": args.dtype, "sky": "all-sky" if args.allsky else "clear-sky",
               "ncol": args.ncol, "nlay": args.nlay, "ngpt": args.ngpt, "nbnd": nbnd, "steps": args.steps, "warmup": args.warmup,
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
