#!/usr/bin/env python3
"""Cost of the rescaled LW no-scattering solver, in one process on one GPU (bench.py's synthetic workload).

The LW solver stage on the inputs of one ResidentSolver step (tau, Planck fractions, band Planck functions, sfc_src of the product
chain; with --allsky the LW band cloud tau / ssa / g of rrx_cloud_optics_2str), timed with device events around --steps launches
after --warmup, in four configurations that take turns (--rounds times; each one's median is reported):

  noscat         (a) rrx_lw_solver_noscat_fractions, the existing solve (with --allsky: on the all-sky absorption optical depth); it
                 runs twice per round (noscat, noscat_again): the spread of (a) against itself is the noise floor of the comparison
  materialised   (b) gas tau copied, ssa = g = 0, rrx_inc_2stream_by_2stream_bybnd (with clouds), rrx_planck_sources_from_fractions,
                 then rrx_lw_solver_noscat_rescaled with do_broadband
  fused          (c) rrx_lw_solver_noscat_fractions_rescaled
  twostream      (d) rrx_lw_solver_2stream_fractions, the fused two-stream solve with scattering

One JSON line per configuration: ms, the rounds, and for fused the ratios c_over_a, c_over_b and c_over_d, the margin b - c and the
spread of (a).

  python tools/lw1r_bench.py                               # C4 fp64: 16 384 columns x 140 layers x 256 g-points
  python tools/lw1r_bench.py --dtype f32
  python tools/lw1r_bench.py --ncol 2048
  python tools/lw1r_bench.py --dtype f32 --ncol 32768 --allsky
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
    ap.add_argument("--ncol", type=int, default=128*128)
    ap.add_argument("--nlay", type=int, default=140)
    ap.add_argument("--ngpt", type=int, default=256)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--allsky", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
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
    kd_lw = be.upload_kdist(synthetic.make_kdist("lw", ngpt=args.ngpt, nbnd=nbnd).astype(np_dtype))
    kd_sw = be.upload_kdist(synthetic.make_kdist("sw", ngpt=args.ngpt, nbnd=nbnd).astype(np_dtype))
    a = argparse.Namespace(ncol=args.ncol, nlay=args.nlay, scaling="weak", top_at_1=False, allsky=args.allsky, col_spread=0.0)
    _, atm0 = bench.local_atmosphere(a, nbnd, 0, 1)
    atm = pipeline.upload_atmosphere(be, atm0.astype(np_dtype))
    luts = None
    if args.allsky:
        cast = lambda lut: be.upload_lut({k: (v.astype(np_dtype) if isinstance(v, np.ndarray) else v) for k, v in lut.items()})
        luts = (cast(synthetic.make_cloud_lut(nbnd, "lw")), cast(synthetic.make_cloud_lut(nbnd, "sw")))

    # the solvers' inputs: those of one product step (the no-scattering one with the cloud absorption in tau, the other clear)
    sv = pipeline.ResidentSolver(be, kd_lw, kd_sw, atm, do_broadband=True, cloud_luts=luts)
    sc = pipeline.ResidentSolver(be, kd_lw, kd_sw, atm, do_broadband=True, cloud_luts=luts, lw_scattering=True)
    sv.step(); sc.step()
    cld = be.cloud_optics_2str(luts[0], atm.lwp, atm.iwp, atm.rel, atm.dei) if luts is not None else None
    torch.cuda.synchronize()
    nlay, ngpt = args.nlay, args.ngpt
    ncol = sc.lw["tau"].shape[2]
    top = atm.top_at_1
    up, dn = be.empty((nlay+1, ncol)), be.empty((nlay+1, ncol))
    m_tau, m_ssa, m_g = be.empty((ngpt, nlay, ncol)), be.empty((ngpt, nlay, ncol)), be.empty((ngpt, nlay, ncol))
    m_lay, m_lev = be.empty((ngpt, nlay, ncol)), be.empty((ngpt, nlay+1, ncol))

    def noscat():
        be.lw_solver_noscat_fractions(top, kd_lw, sv.secants, sv.weights, sv.lw["tau"], sv.lw, sv.sfc_emis_gpt, flux_up=up, flux_dn=dn)

    def materialised():
        m_tau.copy_(sc.lw["tau"]); m_ssa.zero_(); m_g.zero_()
        if cld is not None:
            be.inc_2stream_by_2stream_bybnd(m_tau, m_ssa, m_g, *cld, kd_lw.band_lims_gpt)
        be.planck_sources_from_fractions(kd_lw, sc.lw, lay_src=m_lay, lev_src=m_lev)
        be._c("lw_solver_noscat_rescaled", ncol, nlay, ngpt, BoolArg(top), 1, sv.secants, sv.weights, m_tau, m_ssa, m_g, m_lay, m_lev,
              sc.sfc_emis_gpt, sc.lw["sfc_src"], None, None, None, BoolArg(True), up, dn, BoolArg(False), None, None)

    def fused():
        be.lw_solver_noscat_fractions_rescaled(top, kd_lw, sv.secants, sv.weights, sc.lw["tau"], sc.lw, sc.sfc_emis_gpt, cloud=cld,
                                               flux_up=up, flux_dn=dn)

    def twostream():
        be.lw_solver_2stream_fractions(top, kd_lw, sc.lw["tau"], sc.lw, sc.sfc_emis_gpt, cloud=cld, flux_up=up, flux_dn=dn)

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

    modes = [("noscat", noscat), ("materialised", materialised), ("fused", fused), ("twostream", twostream), ("noscat_again", noscat)]
    times = {m: [] for m, _ in modes}
    for _ in range(args.rounds):
        for m, fn in modes:
            times[m].append(timed_device(fn))
    med = {m: float(np.median(v)) for m, v in times.items()}
    both = times["noscat"] + times["noscat_again"]
    spread = max(both) - min(both)
    for m, _ in modes:
        out = {"stage": "solver", "mode": m, "ms": round(med[m], 4), "rounds_ms": [round(t, 4) for t in times[m]]}
        if m == "fused":
            out.update(c_over_a=round(med[m] / med["noscat"], 4), c_over_b=round(med[m] / med["materialised"], 4),
                       c_over_d=round(med[m] / med["twostream"], 4), cheaper_than_twostream=bool(med[m] < med["twostream"]),
                       b_minus_c_ms=round(med["materialised"] - med[m], 4), noscat_spread_ms=round(spread, 4),
                       faster_than_materialised_by_more_than_the_spread=bool(med["materialised"] - med[m] > spread))
        out.update(dtype=args.dtype, ncol=args.ncol, nlay=args.nlay, ngpt=args.ngpt, allsky=args.allsky, steps=args.steps,
                   warmup=args.warmup, rounds=args.rounds, device=torch.cuda.get_device_name(0))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
