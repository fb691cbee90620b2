"""Host time of the argument assembly of one HipKernels.raytracer_sw_bg call (no GPU): the binding on CPU tensors with _c stubbed,
so that what is timed is the Python between the caller and the library: the gathered scene (raytracer_args.RtScene), the checks,
the output tensors and the argument tuple. Compares the hip_kernels.py of this tree with another one given by --other (a file
holding an older hip_kernels.py; it is loaded into this tree's package), alternately, --repeats times --calls calls each, and
prints the medians with the other's min-max range, in the style of tools/ffi_call_overhead.py.

  python tools/rt_binding_overhead.py --other /path/to/older/hip_kernels.py
"""
import argparse
import importlib.util
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rte_rrtmgp_cpp_amd as R          # noqa: E402


def recorder(module):
    class Stub(module.HipKernels):
        def __init__(self):
            self.np_dtype, self.sfx, self.tdtype, self.device, self.stream = np.dtype(np.float64), "_f64", torch.float64, torch.device("cpu"), None
            self.calls = 0

        def _c(self, name, *args):
            self.calls += 1
            return 0
    return Stub()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("rte_rrtmgp_cpp_amd._other_hip_kernels", a.other)
    other = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(other)
    sides = {"other": recorder(other), "this": recorder(R.hip_kernels)}

    nx, ny, nz, ngpt, nbnd, nbg = 4, 3, 4, 2, 2, 3
    t = lambda *shape: torch.ones(shape, dtype=torch.float64)
    triple = lambda *shape: (t(*shape), t(*shape), t(*shape))
    background = SimpleNamespace(dz=np.array([300.0, 1250.0, 4100.0]), tau=t(ngpt, nbg), ssa=t(ngpt, nbg), cloud=triple(nbnd, nbg), aerosol=triple(nbnd, nbg))
    args = (t(ngpt, nz, nx*ny), t(ngpt, nz, nx*ny), nx, ny, 100.0, 100.0, 50.0, t(nx*ny), 0.6, 0.5, np.ones(ngpt), np.zeros(ngpt), (2, 1, 2), 4, 11)
    kw = dict(cloud=triple(nbnd, nz, nx*ny), band_lims=torch.tensor([[1, 1], [2, 2]], dtype=torch.int32), background=background,
              aerosol=triple(nbnd, nz, nx*ny))
    us = {k: [] for k in sides}
    for be in sides.values():
        assert set(be.raytracer_sw_bg(*args, **kw)) == set(be.RT_COUNTS + be.RT_BG_COUNTS + ("n_capped",)) and be.calls == 1
    for _ in range(a.repeats):
        for k, be in sides.items():
            call = be.raytracer_sw_bg
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call(*args, **kw)
            us[k].append((time.perf_counter() - t0) / a.calls * 1e6)
    print(f"raytracer_sw_bg (rrx_raytracer_sw_aer, 56 arguments) on a {nx} x {ny} x {nz} grid with {nbg} background layers, CPU tensors, _c stubbed, "
          f"{a.repeats} x {a.calls} calls each, alternating; microseconds per call")
    for k, v in us.items():
        print(f"{k:6s} median {statistics.median(v):7.2f}  min {min(v):7.2f}  max {max(v):7.2f}  runs " + " ".join(f"{x:.2f}" for x in v))
    verdict = "not above" if statistics.median(us["this"]) <= max(us["other"]) else "ABOVE"
    print(f"this tree's median is {verdict} the other's range")


if __name__ == "__main__":
    main()
