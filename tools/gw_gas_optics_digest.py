#!/usr/bin/env python3
"""Digests of the raw gas-optics arrays of the bench's synthetic problem (LW fractions form: tau, pfrac, B_lay, B_lev, sfc_src,
sfc_src_jac; SW form: tau, ssa, and g with --allsky), one JSON line. Two builds that print the same line computed the same bits: the arrays themselves
are gigabytes at C4, the digests are compared instead.

  python tools/gw_gas_optics_digest.py [--ncol 16384] [--nlay 140] [--ngpt 256] [--nbnd 0] [--dtype f64] [--col-spread 0.0]
                                      [--allsky] [--window 0|1]
--allsky passes by-band cloud properties through the entries' by_band= arguments (the all-sky kernel forms); --window 0 switches the
windowed kernel off (rrx_set_gas_window), so that the gather kernels compute everything."""
import argparse, hashlib, json, os, sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rte_rrtmgp_cpp_amd as R
from rte_rrtmgp_cpp_amd import synthetic, pipeline

ap = argparse.ArgumentParser()
ap.add_argument("--ncol", type=int, default=16384)
ap.add_argument("--nlay", type=int, default=140)
ap.add_argument("--ngpt", type=int, default=256)
ap.add_argument("--nbnd", type=int, default=0)
ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
ap.add_argument("--col-spread", type=float, default=0.0)
ap.add_argument("--allsky", action="store_true")
ap.add_argument("--window", type=int, default=1, choices=[0, 1])
a = ap.parse_args()
nbnd = a.nbnd or a.ngpt // 16
dt = np.float64 if a.dtype == "f64" else np.float32
be = R.HipKernels(dt, "cuda:0")
atm0 = synthetic.make_atmosphere(a.ncol, a.nlay, nbnd_lw=nbnd, nbnd_sw=nbnd, seed=1234)
if a.col_spread > 0:
    import bench                                         # (the benchmark's own way of making the columns differ)
    atm0 = bench.spread_columns(atm0, a.col_spread, 0, a.ncol, a.ncol)
atm = pipeline.upload_atmosphere(be, atm0.astype(dt))
out = {"ncol": a.ncol, "nlay": a.nlay, "ngpt": a.ngpt, "nbnd": nbnd, "dtype": a.dtype, "col_spread": a.col_spread,
       "allsky": a.allsky, "window": a.window}
be.lib.call("rrx_set_gas_window", a.window)
cld = None
if a.allsky:                                             # by-band cloud optical depth, single-scattering albedo, asymmetry
    rng = np.random.default_rng(4321)
    cld = [be.asarray(rng.uniform(lo, hi, (nbnd, a.nlay, a.ncol)).astype(dt)) for lo, hi in ((0.0, 2.0), (0.5, 1.0), (0.0, 0.9))]


def digest(t):
    h = hashlib.blake2b(digest_size=16)
    flat = t.reshape(-1)
    for s in range(0, flat.numel(), 1 << 26):           # (pieces: the host copy of a whole C4 array is 4.7 GB)
        h.update(flat[s:s + (1 << 26)].cpu().numpy().tobytes())
    return h.hexdigest()


shape = (a.ngpt, a.nlay, a.ncol)
kd = be.upload_kdist(synthetic.make_kdist("lw", ngpt=a.ngpt, nbnd=nbnd).astype(dt))
col_dry, col_gas, _ = pipeline.gas_state(be, kd, atm, interpolate=False)
tau = be.empty(shape)
fr = be.gas_optics_lw_fractions(kd, atm.p_lay, atm.t_lay, atm.t_lev, atm.t_sfc, pipeline._sfc_lay(atm), col_gas, tau,
                                by_band=cld[0] if a.allsky else None)
out["lw_tau"] = digest(tau)
for k, v in fr.items():
    if hasattr(v, "data_ptr"):
        out["lw_" + k] = digest(v)
del tau, fr
kd = be.upload_kdist(synthetic.make_kdist("sw", ngpt=a.ngpt, nbnd=nbnd).astype(dt))
col_dry, col_gas, _ = pipeline.gas_state(be, kd, atm, interpolate=False)
tau, ssa, g = be.empty(shape), be.empty(shape), (be.empty(shape) if a.allsky else None)
be.gas_optics_sw_direct(kd, atm.p_lay, atm.t_lay, col_gas, col_dry, tau, ssa, g, by_band=cld)
out["sw_tau"], out["sw_ssa"] = digest(tau), digest(ssa)
if a.allsky:
    out["sw_g"] = digest(g)
print(json.dumps(out), flush=True)
