"""bench.py --dump-outputs without a GPU: what output_arrays makes of a step's packed fluxes (names, precision, size bound, the
fixed column sample), and the options of a plain run."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _packed(ncol, nlev=141, dtype=np.float64):
    f = np.arange(7 * nlev * ncol, dtype=np.float64).reshape(7, nlev, ncol)
    return f.astype(dtype)


def test_small_outputs_are_written_whole(tmp_path):
    F = _packed(300, dtype=np.float32)
    bench.dump_outputs(str(tmp_path), F)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in bench.FLUX_NAMES)
    for i, n in enumerate(bench.FLUX_NAMES):
        a = np.load(tmp_path / (n + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, F[i]), n


def test_large_outputs_are_a_fixed_column_sample_within_the_budget(tmp_path):
    F = _packed(16384)                                  # the default workload: 129 MB of fp64 fluxes
    bench.dump_outputs(str(tmp_path), F)
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert total <= bench.DUMP_BYTES and total > bench.DUMP_BYTES // 2
    a = bench.output_arrays(F)
    b = bench.output_arrays(F.copy())
    cols = (a["lw_flux_up"][0] - F[0, 0, 0]).astype(np.int64)      # row 0 of flux 0 holds the column index
    assert np.all(np.diff(cols) > 0) and cols[-1] < 16384
    for i, n in enumerate(bench.FLUX_NAMES):
        assert a[n].dtype == np.float64 and np.array_equal(a[n], b[n]) and np.array_equal(a[n], F[i][:, cols]), n
        assert np.array_equal(np.load(tmp_path / (n + ".npy")), a[n]), n


def test_plain_run_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dry-run"], capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode != 0 and "--steps" in bad.stderr
