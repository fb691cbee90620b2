#!/usr/bin/env python3
"""Cost of McICA cloud sampling, in one process on one GPU: ResidentSolver steps (LW+SW, bench.py's synthetic all-sky workload) timed
the way bench.py times them -- W warm-up steps, then K steps between two torch.cuda.synchronize() calls, wall clock:

  allsky       today's route: the band cloud properties added inside the fused all-sky gas optics, every cloud overcast
  mcica@S      ResidentSolver(cloud_fraction=...): clear gas optics, then rrx_mcica_increment_*; a share S of the layers of every
               column is cloudy (one contiguous block per column, at a random height) with cloud fraction --fraction, the rest clear

Each mode also runs a few steps with stage events: the gas-optics stages hold the cloud optics, the gas optics and the sampling
kernel. The modes take turns (--rounds times, medians reported). One JSON line per mode.

  python tools/mcica_bench.py                                   # C5's per-GPU shape: fp32 all-sky, 32 768 columns x 140 x 256
  python tools/mcica_bench.py --overlap exp_ran
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
    ap.add_argument("--ncol", type=int, default=32768)
    ap.add_argument("--nlay", type=int, default=140)
    ap.add_argument("--ngpt", type=int, default=256)
    ap.add_argument("--dtype", default="f32", choices=["f64", "f32"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shares", default="0.1,0.3,1.0")
    ap.add_argument("--fraction", type=float, default=0.5)
    ap.add_argument("--overlap", default="max_ran", choices=["max_ran", "exp_ran"])
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
    cast = lambda lut: be.upload_lut({k: (v.astype(np_dtype) if isinstance(v, np.ndarray) else v) for k, v in lut.items()})
    luts = (cast(synthetic.make_cloud_lut(nbnd, "lw")), cast(synthetic.make_cloud_lut(nbnd, "sw")))
    a = argparse.Namespace(ncol=args.ncol, nlay=args.nlay, scaling="weak", top_at_1=False, allsky=True, col_spread=0.0)
    _, atm0 = bench.local_atmosphere(a, nbnd, 0, 1)
    atm = pipeline.upload_atmosphere(be, atm0.astype(np_dtype))
    rng = np.random.default_rng(2026)

    def cloud_fraction(share):
        n = int(round(share * args.nlay))
        start = rng.integers(0, args.nlay - n + 1, args.ncol)
        lay = np.arange(args.nlay)[:, None]
        return be.asarray(np.where((lay >= start[None, :]) & (lay < start[None, :] + n), args.fraction, 0.0).astype(np_dtype))

    fields = {"allsky": None}
    fields.update({"mcica@%g" % s: cloud_fraction(s) for s in (float(f) for f in args.shares.split(",") if f)})
    alpha = be.asarray(np.full((args.nlay-1, args.ncol), 0.7, dtype=np_dtype)) if args.overlap == "exp_ran" else None
    modes = list(fields)
    times = {m: [] for m in modes}
    stages = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            kw = {} if fields[m] is None else dict(cloud_fraction=fields[m], cloud_overlap=args.overlap, overlap_param=alpha, mcica_seed=1)
            s = pipeline.ResidentSolver(be, kd_lw, kd_sw, atm, do_broadband=True, cloud_luts=luts, **kw)
            for _ in range(args.warmup):
                s.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.mcica_seed += 1                 # (a host advances the seed between calls)
                s.step()
            torch.cuda.synchronize()
            times[m].append((time.perf_counter() - t0) / args.steps * 1e3)
            s.enable_stage_events(3)
            for _ in range(3):
                s.step()
            torch.cuda.synchronize()
            stages[m].append(s.stage_ms())
            del s
            torch.cuda.empty_cache()
    ref = float(np.median(times["allsky"]))
    for m in modes:
        ms = float(np.median(times[m]))
        st = {k: round(float(np.median([r[k] for r in stages[m]])), 3) for k in stages[m][0]}
        f = fields[m]
        out = {"mode": m, "cloudy_layer_share": None if f is None else round(float((f > 0).float().mean().item()), 4),
               "cloud_fraction": None if f is None else args.fraction, "overlap": None if f is None else args.overlap,
               "ms_per_step": round(ms, 3), "vs_allsky": round(ms / ref, 3),
               "gas_optics_ms": round(st["lw_gas_optics"] + st["sw_gas_optics"], 3), "stages_ms": st,
               "rounds_ms": [round(t, 3) for t in times[m]], "dtype": args.dtype, "ncol": args.ncol, "nlay": args.nlay, "ngpt": args.ngpt,
               "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
