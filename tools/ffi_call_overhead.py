"""Host time per Lib.call of one zero-extent call of a long entry (no GPU): rrx_gas_optics_lw_fractions_allsky_f64 with numpy buffers
and ncol = 0, which the entry answers with "empty problem" (status 1) before any HIP call, the same work on both sides. Compares
the _ffi.py of this tree (signatures from include/rrx_hip.h) with another one given by --other (a file holding an older _ffi.py),
alternately, --repeats times --calls calls each, and prints the medians with the other's min-max range.

  python tools/ffi_call_overhead.py --other /path/to/older/_ffi.py [--tensors] [--entry rrx_sum_broadband_f64]
"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENTRY = "rrx_gas_optics_lw_fractions_allsky_f64"


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def arguments(new, entry, tensors):
    """The entry's argument list from its declaration: ncol = 0, live host buffers (numpy arrays, or torch CPU tensors)"""
    dtypes = {"double": np.float64, "int": np.int32, "RrxBool": np.int8}
    args = []
    for ctype, name in new.read_signatures()[entry].params:
        base = ctype.replace("const", "").replace("*", "").strip()
        if name == "stream":
            args.append(None)
        elif "*" in ctype:
            args.append(np.zeros(4, dtype=dtypes[base]))
            if tensors:
                import torch
                args[-1] = torch.from_numpy(args[-1])
        elif base == "double":
            args.append(1.0)
        else:
            args.append(0 if name == "ncol" else 2)
    return args


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100000)
    ap.add_argument("--entry", default=ENTRY, help="an _f64 entry without RrxBool scalars that answers ncol = 0 before any HIP call")
    ap.add_argument("--tensors", action="store_true", help="torch CPU tensors instead of numpy arrays")
    a = ap.parse_args()
    pkg = os.path.join(ROOT, "rte-rrtmgp-cpp_amd")
    lib_path = os.path.join(pkg, "lib", "librrx_hip.so")
    new, old = load(os.path.join(pkg, "_ffi.py"), "ffi_new"), load(a.other, "ffi_other")
    args = arguments(new, a.entry, a.tensors)
    libs = {"other": old.Lib(lib_path, np.float64), "this": new.Lib(lib_path, np.float64, header=new.HEADER_PATH)}
    us = {k: [] for k in libs}
    for lib in libs.values():
        lib.call(a.entry, *args)
    if a.entry == ENTRY:
        assert libs["this"].call(ENTRY, *args) == 1 and b"empty problem" in libs["this"].call("rrx_last_error")
    for _ in range(a.repeats):
        for k, lib in libs.items():
            call = lib.call
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call(a.entry, *args)
            us[k].append((time.perf_counter() - t0) / a.calls * 1e6)
    print(f"{a.entry}, {len(args)} arguments, ncol = 0, {'torch CPU tensors' if a.tensors else 'numpy arrays'}, {a.repeats} x {a.calls} calls each, "
          "alternating; microseconds per Lib.call")
    for k, v in us.items():
        print(f"{k:6s} median {statistics.median(v):7.3f}  min {min(v):7.3f}  max {max(v):7.3f}  runs " + " ".join(f"{x:.3f}" for x in v))
    verdict = "not above" if statistics.median(us["this"]) <= max(us["other"]) else "ABOVE"
    print(f"this tree's median is {verdict} the other's range")


if __name__ == "__main__":
    main()
