#!/usr/bin/env python3
"""Cost of sunlit-only SW, in one process on one GPU: ResidentSolver steps (LW+SW, bench.py's synthetic workload) timed the way bench.py
times them -- W warm-up steps, then K steps between two torch.cuda.synchronize() calls, wall clock:

  off        ResidentSolver(sunlit=False) on the all-sunlit atmosphere: the headline step
  on@F       ResidentSolver(sunlit=True) with a fraction F of the columns sunlit; the dark ones are picked at random (not in a block),
             half at mu0 = 0, half below the horizon

Each mode also runs a few steps with stage events: the SW stage is sw_gas_optics + sw_solver + sw_reduce (gather of the sunlit
columns' inputs, gas optics, solver, zero-filling scatter). host_wait_ms is the host time spent in the one wait of a sunlit step
(for the column count), per step. The modes take turns (--rounds times, medians reported). One JSON line per mode.

  python tools/sunlit_bench.py                                  # C4 fp64 clear sky: 16 384 columns x 140 layers x 256 g-points
  python tools/sunlit_bench.py --dtype f32 --allsky --ncol 32768
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
    ap.add_argument("--fractions", default="1.0,0.75,0.5,0.25")
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
    luts = None
    if args.allsky:
        cast = lambda lut: be.upload_lut({k: (v.astype(np_dtype) if isinstance(v, np.ndarray) else v) for k, v in lut.items()})
        luts = (cast(synthetic.make_cloud_lut(nbnd, "lw")), cast(synthetic.make_cloud_lut(nbnd, "sw")))
    a = argparse.Namespace(ncol=args.ncol, nlay=args.nlay, scaling="weak", top_at_1=False, allsky=args.allsky, col_spread=0.0)
    _, atm0 = bench.local_atmosphere(a, nbnd, 0, 1)
    atm0 = atm0.astype(np_dtype)
    rng = np.random.default_rng(2026)
    fracs = [float(f) for f in args.fractions.split(",") if f]

    def atmosphere(frac):
        mu0 = atm0.mu0.copy()
        dark = rng.permutation(args.ncol)[:int(round((1.0 - frac) * args.ncol))]
        mu0[dark[:dark.size // 2]] = 0.0
        mu0[dark[dark.size // 2:]] = -0.5
        atm0.mu0, keep = np.ascontiguousarray(mu0), atm0.mu0
        try:
            return pipeline.upload_atmosphere(be, atm0)
        finally:
            atm0.mu0 = keep

    atms = {"off": pipeline.upload_atmosphere(be, atm0)}
    atms.update({"on@%g" % f: atmosphere(f) for f in fracs})
    modes = list(atms)
    times = {m: [] for m in modes}
    stages = {m: [] for m in modes}
    waits = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            s = pipeline.ResidentSolver(be, kd_lw, kd_sw, atms[m], do_broadband=True, cloud_luts=luts, sunlit=(m != "off"))
            for _ in range(args.warmup):
                s.step()
            torch.cuda.synchronize()
            if s.sunlit:
                s.sun_wait_ms = 0.0
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
            torch.cuda.synchronize()
            times[m].append((time.perf_counter() - t0) / args.steps * 1e3)
            if s.sunlit:
                waits[m].append(s.sun_wait_ms / args.steps)
            s.enable_stage_events(3)
            for _ in range(3):
                s.step()
            torch.cuda.synchronize()
            st = s.stage_ms()
            stages[m].append(st)
            del s
            torch.cuda.empty_cache()
    ref = float(np.median(times["off"]))
    sw_ref = None
    for m in modes:
        ms = float(np.median(times[m]))
        st = {k: round(float(np.median([r[k] for r in stages[m]])), 3) for k in stages[m][0]}
        sw = round(st["sw_gas_optics"] + st["sw_solver"] + st["sw_reduce"], 3)
        if m == "off":
            sw_ref = sw
        out = {"mode": m, "sunlit_fraction": 1.0 if m == "off" else float(m.split("@")[1]), "ms_per_step": round(ms, 3),
               "vs_off": round(ms / ref, 3), "sw_stage_ms": sw, "sw_vs_off": round(sw / sw_ref, 3), "stages_ms": st,
               "host_wait_ms": round(float(np.median(waits[m])), 4) if waits[m] else None,
               "rounds_ms": [round(t, 3) for t in times[m]], "dtype": args.dtype, "sky": "all-sky" if args.allsky else "clear-sky",
               "ncol": args.ncol, "nlay": args.nlay, "ngpt": args.ngpt, "steps": args.steps, "warmup": args.warmup,
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
