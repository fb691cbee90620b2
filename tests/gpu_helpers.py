"""What the direct GPU kernel tests share (tests/test_gpu_support_kernels.py, tests/test_gpu_optics_kernels.py): the precision fixture,
outputs allocated with a guard tail, and the comparison of bit patterns."""
import ctypes

import numpy as np
import pytest
import torch

GUARD = -7
ULL = ctypes.c_ulonglong


@pytest.fixture(params=["f64", "f32"])
def be(request, hip_f64, hip_f32):
    return hip_f64 if request.param == "f64" else hip_f32


def guarded(be, shape, dtype=None):
    """(buf, out): out is a contiguous tensor of `shape` at the head of buf, which is twice as long (at least two words); all of
    buf holds GUARD"""
    n = int(np.prod(shape, dtype=np.int64))
    buf = torch.full((max(2*n, 2),), GUARD, dtype=dtype or be.tdtype, device=be.device)
    return buf, buf[:n].view(tuple(shape))


def guarded_copy(be, a):
    """a numpy array on the device, with a guard tail (for arrays a kernel updates in place)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf, out = guarded(be, a.shape, t.dtype)
    out.copy_(t)
    return buf, out


def tail_untouched(buf, out):
    return bool((buf[out.numel():] == GUARD).all().item())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    """equal shapes, types and bit patterns (tells -0.0 from 0.0, which == does not)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def dev(be, a):
    """numpy -> device, the dtype kept as it is"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(be.device)


def int_array(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])
