#!/usr/bin/env python3
"""Cost of a cosine of the solar zenith angle per layer in the SW solver, in one process on one GPU. One ResidentSolver step of
bench.py's synthetic workload fills the SW optical properties; the broadband solve on them is then timed three ways with device
events (W warm-up calls, then K calls between two events), the modes taking turns (--rounds times, medians reported):

  fused_1d          rrx_sw_solver_2stream, do_broadband: the fused one-kernel form with mu0(ncol)
  fused_mu0lay      rrx_sw_solver_2stream_mu0lay, do_broadband: the fused form with mu0_lay(ncol, nlay)
  pergpt_mu0lay     the same entry under SW variant 7: the per-g-point by-layer kernel into a workspace and the three g-point sums

mu0_lay comes from rrx_zenith_angle_spherical_correction on altitudes made from the pressures (scale height 7.5 km); its cost
is reported too. One JSON line per mode; vs_fused_1d is the figure to quote.

  python tools/sw_mu0lay_bench.py                                       # the bench shape: fp64 clear sky, 16 384 x 140 x 224
  python tools/sw_mu0lay_bench.py --dtype f32 --allsky --ncol 32768 --ngpt 256
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=16384)
    ap.add_argument("--nlay", type=int, default=140)
    ap.add_argument("--ngpt", type=int, default=224)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--allsky", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import torch
    import rte_rrtmgp_cpp_amd as R
    from rte_rrtmgp_cpp_amd import synthetic, pipeline
    from rte_rrtmgp_cpp_amd._ffi import BoolArg
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
    atm = pipeline.upload_atmosphere(be, atm0)
    sv = pipeline.ResidentSolver(be, kd_lw, kd_sw, atm, do_broadband=True, cloud_luts=luts, sort_columns="0")
    assert sv.perm is None, "the bench shapes are multiples of 16 columns"
    sv.step()
    tau, ssa = sv.sw["tau"], sv.sw["ssa"]
    g = None if sv.g_zero else sv.sw["g"]
    toa = be.toa_source(args.ncol, kd_sw.solar_source, atm.tsi_scaling)
    alt = be.asarray((7500.*np.log(atm0.p_lev.max(axis=0)[None, :].astype(np.float64) / atm0.p_lay)).astype(np_dtype))
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    mu0_lay = be.empty((args.nlay, args.ncol))
    corr_ms = timed(lambda: be.zenith_angle_spherical_correction(atm.mu0, alt, out=mu0_lay))
    out = {k: be.empty((args.nlay+1, args.ncol)) for k in ("flux_up", "flux_dn", "flux_dir")}
    top = BoolArg(atm.top_at_1)

    def one_d():
        be._c("sw_solver_2stream", args.ncol, args.nlay, args.ngpt, top, tau, ssa, g, atm.mu0, sv.alb_dir, sv.alb_dif, toa,
              None, None, None, BoolArg(False), None, BoolArg(True), out["flux_up"], out["flux_dn"], out["flux_dir"])

    def by_layer():
        be.sw_solver_2stream_mu0lay(atm.top_at_1, tau, ssa, g, mu0_lay, sv.alb_dir, sv.alb_dif, toa, do_broadband=True, out=out)

    def per_gpt():
        be.set_variant(sw=7)
        try:
            by_layer()
        finally:
            be.set_variant(sw=0)

    modes = {"fused_1d": one_d, "fused_mu0lay": by_layer, "pergpt_mu0lay": per_gpt}
    times = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m, fn in modes.items():
            times[m].append(timed(fn))
    ref = float(np.median(times["fused_1d"]))
    for m in modes:
        ms = float(np.median(times[m]))
        print(json.dumps({"mode": m, "ms_per_solve": round(ms, 3), "vs_fused_1d": round(ms / ref, 3), "rounds_ms": [round(t, 3) for t in times[m]],
                          "correction_ms": round(corr_ms, 4), "dtype": args.dtype, "allsky": args.allsky, "g_array": g is not None,
                          "ncol": args.ncol, "nlay": args.nlay, "ngpt": args.ngpt, "steps": args.steps, "warmup": args.warmup,
                          "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
