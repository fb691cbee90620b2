"""What the GPU tests of the C++ host layer share: the stand-alone driver (test_rte_rrtmgp_gpu) run in-process through
rrx_host_main of librte_rrtmgp_hip.so."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTLIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librte_rrtmgp_hip.so")


def run_driver(workdir, *flags, env=None):
    """rrx_host_main with `flags` in workdir, where the driver reads its input and writes rte_rrtmgp_output.nc: the command-line
    driver's behaviour and exit status. env: environment variables for this run only; the process's own come back after it."""
    lib = ctypes.CDLL(HOSTLIB)
    argv = [b"test_rte_rrtmgp_gpu"] + [f.encode() for f in flags]
    old, saved = os.getcwd(), {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        os.chdir(workdir)
        return lib.rrx_host_main(len(argv), (ctypes.c_char_p * len(argv))(*argv))
    finally:
        os.chdir(old)
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
