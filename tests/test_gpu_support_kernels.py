"""GPU tests of the layer around the solvers and the gas optics, one entry point of include/rrx_hip.h at a time: the column-ordering
kernels (csrc/rrx_columns.hip: sort, identity, spread, gathers, scatter) and the glue kernels (csrc/rrx_misc.hip: subsets, fills,
gas columns, heating rate, by-band sums, by-band increments, band -> g-point expansion).

Every reference is plain numpy (tests/support_ref.py, itself checked by tests/test_support_ref.py). Whatever only moves data, adds
or multiplies once is compared bit for bit. Every output is allocated with a tail of guard words as long as itself, filled with -7,
which must come back untouched. An entry's empty problem (an extent of 0) is followed by a valid call that must succeed and be
right: no launch error may be left behind."""
import ctypes
import types

import numpy as np
import pytest
import torch

import cases
import support_ref as ref
from gpu_helpers import GUARD, ULL, be, dev, guarded, guarded_copy, int_array, same_bits, tail_untouched      # noqa: F401 (be: a fixture)
from rte_rrtmgp_cpp_amd import synthetic, pipeline

pytestmark = pytest.mark.gpu


# ==== column order (csrc/rrx_columns.hip) ======================================================================================
SORT_NCOL = [1, 2, 255, 256, 257, 4097, 70000]      # (70 000: beyond the sizes rocprim sorts within one workgroup or a few)
PADS = [0, 1, 15]
KEY_KINDS = ["uniform", "ties", "signed", "sorted", "reversed"]


def sort_keys(kind, ncol, rng, dtype):
    """No NaN, no zero of either sign: there a radix order and numpy's differ by definition. Rounded to the key type BEFORE the
    reference is taken (fp32 rounding makes ties of its own among 70 000 pressures)."""
    p = rng.uniform(5.0e4, 1.1e5, ncol)
    if kind == "ties":
        p = 9.0e4 + 1.0e3*rng.integers(0, 8, ncol)
    elif kind == "signed":
        p = rng.uniform(-1.0e3, 1.0e3, ncol)
        p[p == 0.] = 1.
    elif kind == "sorted":
        p = np.sort(p)
    elif kind == "reversed":
        p = np.sort(p)[::-1]
    return np.ascontiguousarray(p.astype(dtype))


@pytest.mark.parametrize("ncol", SORT_NCOL)
def test_sort_columns_is_the_stable_ascending_order(ncol, be):
    """perm[:ncol] is numpy's stable argsort of the key, the npad entries behind it repeat perm[ncol-1], the key is not modified."""
    rng = np.random.default_rng(ncol)
    for kind in KEY_KINDS:
        key_np = sort_keys(kind, ncol, rng, be.np_dtype)
        want = ref.sort_perm(key_np, 0)
        for npad in PADS:
            key = dev(be, key_np)
            buf, perm = guarded(be, (ncol + npad,), torch.int32)
            be._c("sort_columns", ncol, key, npad, perm)
            got = perm.cpu().numpy()
            assert np.array_equal(got[:ncol], want), (kind, npad)
            assert (got[ncol:] == got[ncol-1]).all(), (kind, npad)
            assert np.array_equal(got, ref.sort_perm(key_np, npad)), (kind, npad)
            assert same_bits(key.cpu().numpy(), key_np), (kind, npad)
            assert tail_untouched(buf, perm), (kind, npad)


def test_sort_and_identity_refuse_empty_problems(be):
    key = dev(be, sort_keys("uniform", 8, np.random.default_rng(0), be.np_dtype))
    buf, perm = guarded(be, (8,), torch.int32)
    for ncol, npad in ((0, 0), (0, 3), (8, -1)):
        with pytest.raises(RuntimeError, match="empty problem"):
            be._c("sort_columns", ncol, key, npad, perm)
        with pytest.raises(RuntimeError, match="empty problem"):
            be.lib.call("rrx_identity_columns", ncol, npad, perm, be._st())
    assert (buf == GUARD).all()
    be._c("sort_columns", 8, key, 0, perm)                             # a valid call straight afterwards
    assert np.array_equal(perm.cpu().numpy(), ref.sort_perm(key.cpu().numpy(), 0))
    be.lib.call("rrx_identity_columns", 5, 3, perm, be._st())
    assert np.array_equal(perm.cpu().numpy(), ref.identity_perm(5, 3)) and tail_untouched(buf, perm)


@pytest.mark.parametrize("ncol", SORT_NCOL)
def test_identity_columns(ncol, hip_f64):
    be = hip_f64
    for npad in PADS:
        buf, perm = guarded(be, (ncol + npad,), torch.int32)
        be.lib.call("rrx_identity_columns", ncol, npad, perm, be._st())
        assert np.array_equal(perm.cpu().numpy(), ref.identity_perm(ncol, npad)), npad
        assert tail_untouched(buf, perm), npad


THRESHOLD = 0.2
QUIET, LOUD = 0.25*THRESHOLD, 2.5*THRESHOLD            # (max - min)/mean of a run, far on either side of the threshold


def spread_case(block, full_ratios, tail, tail_ratio, rng, dtype, threshold=THRESHOLD):
    """Keys of len(full_ratios) full runs of `block` columns with the given (max - min)/mean each, and a partial run of `tail`
    columns behind them. Rounded to the key type; every full run is then at least 1 % of the threshold away from it (far above
    the rounding of an fp32 sum of <= 1 000 terms, 6e-5), so the float64 rule of support_ref decides alone. Returns (keys, flag)."""
    runs = [ref.spread_run(block, r, rng.uniform(6.0e4, 1.05e5), rng) for r in full_ratios]
    if tail:
        runs.append(ref.spread_run(tail, tail_ratio, 9.0e4, rng))
    key = np.ascontiguousarray(np.concatenate(runs).astype(dtype))
    ratios = ref.run_ratios(key, block)
    assert len(ratios) == len(full_ratios) and (np.abs(ratios - threshold) >= 0.01*threshold).all(), ratios
    return key, ref.column_spread(key, block, threshold)


def spread_flag(be, key_np, block, flag, threshold=THRESHOLD):
    be._c("column_spread", len(key_np), dev(be, key_np), block, float(threshold), flag)
    return int(flag.cpu().numpy()[0])


@pytest.mark.parametrize("block", [16, 256, 300, 1000])
def test_column_spread_follows_the_rule_on_full_runs(block, be):
    """block 16: fewer columns than lanes in the workgroup; 256: exactly the workgroup; 300, 1 000: the strided load loop. The
    offending run first, last full, and only in the partial tail (ignored); no partial tail; fewer columns than one run; and a
    run 3 % on either side of the threshold."""
    rng = np.random.default_rng(block)
    buf, flag = guarded(be, (1,), torch.int32)
    half = block // 2
    table = [   # (ratios of the full runs, columns of the partial run, its ratio, expected flag)
        ([QUIET, QUIET, QUIET], 0, 0., 0),
        ([LOUD, QUIET, QUIET], 0, 0., 1),
        ([QUIET, QUIET, LOUD], 0, 0., 1),
        ([QUIET, QUIET, QUIET], half, QUIET, 0),
        ([LOUD, QUIET, QUIET], half, QUIET, 1),
        ([QUIET, QUIET, LOUD], half, QUIET, 1),
        ([QUIET, QUIET, QUIET], half, 2*LOUD, 0),                      # offending columns in the partial tail only
        ([QUIET], 1, 0., 0),
        ([], block - 1, 2*LOUD, 0),                                    # fewer columns than one run
        ([QUIET, 0.97*THRESHOLD], 0, 0., 0),
        ([QUIET, 1.03*THRESHOLD], half, QUIET, 1),
    ]
    for full, tail, tail_ratio, expect in table:
        key, want = spread_case(block, full, tail, tail_ratio, rng, be.np_dtype)
        assert want == expect, (full, tail)
        assert spread_flag(be, key, block, flag) == want, (full, tail, tail_ratio)
        assert tail_untouched(buf, flag)


def test_column_spread_rewrites_its_flag(be):
    """Flagged input, then quiet input on the same flag buffer: the second call must bring the flag back to 0 (and a first call on
    a buffer that holds neither 0 nor 1 must leave 0 or 1)."""
    rng = np.random.default_rng(3)
    buf, flag = guarded(be, (1,), torch.int32)
    loud, _ = spread_case(256, [QUIET, LOUD], 100, QUIET, rng, be.np_dtype)
    quiet, _ = spread_case(256, [QUIET, QUIET], 100, QUIET, rng, be.np_dtype)
    assert spread_flag(be, quiet, 256, flag) == 0                      # over the guard word
    assert spread_flag(be, loud, 256, flag) == 1
    assert spread_flag(be, quiet, 256, flag) == 0
    assert tail_untouched(buf, flag)
    for ncol, block in ((0, 256), (600, 0)):
        with pytest.raises(RuntimeError, match="empty problem"):
            be._c("column_spread", ncol, dev(be, quiet), block, THRESHOLD, flag)
    assert spread_flag(be, loud, 256, flag) == 1                       # a valid call straight afterwards


@pytest.mark.parametrize("spread", [0.0, 0.35])
@pytest.mark.parametrize("ncol", [273, 600])
def test_column_spread_is_the_auto_decision_of_the_resident_solver(ncol, spread, be):
    """block 256, threshold 0.2 on the surface pressures -- the call of the C++ driver (Radiation_solver.cpp) -- gives the
    sort_columns that pipeline.ResidentSolver(sort_columns="auto") decides in Python on the same atmosphere."""
    kw = dict(ngpt=32, nbnd=2, npres=10, nflav=3, nminor_lower=5, nminor_upper=3)
    kl, ks = be.upload_kdist(synthetic.make_kdist("lw", **kw)), be.upload_kdist(synthetic.make_kdist("sw", **kw))
    atm0 = synthetic.make_atmosphere(ncol, 12, nbnd_lw=2, nbnd_sw=2, seed=ncol)
    f = np.random.default_rng(ncol + 1).uniform(1. - spread, 1. + spread, ncol)
    atm0.p_lay = np.ascontiguousarray(atm0.p_lay * f); atm0.p_lev = np.ascontiguousarray(atm0.p_lev * f)
    atm = pipeline.upload_atmosphere(be, atm0)
    solver = pipeline.ResidentSolver(be, kl, ks, atm, do_broadband=True, sort_columns="auto")
    p_sfc = atm.p_lev[-1 if atm.top_at_1 else 0].contiguous()
    ratios = ref.run_ratios(p_sfc.cpu().numpy(), 256)
    assert (np.abs(ratios - THRESHOLD) >= 0.01*THRESHOLD).all(), ratios
    buf, flag = guarded(be, (1,), torch.int32)
    be._c("column_spread", ncol, p_sfc, 256, THRESHOLD, flag)
    got = int(flag.cpu().numpy()[0])
    assert got == int(spread > 0.)
    assert got == int(solver.sort_columns)
    assert tail_untouched(buf, flag)


# (nout, nrest): 65 537 = one column more than the 256 x 256 threads of the x grid; 4 097 = one row more than the y grid's cap
GATHER_SHAPES = [(1, 1), (255, 3), (257, 40), (65537, 2), (3, 4097)]


def gather_perms(nout, rng):
    """(ncol_in, perm, npad) with nout != ncol_in: a padded order (a permutation of ncol_in columns, then npad repeats of its last
    entry) and a subset (nout of ncol_in = nout + 2 columns, the form of the sunlit-column list; npad = None)"""
    out = []
    if nout > 1:
        npad = min(15, nout - 1)
        order = rng.permutation(nout - npad).astype(np.int32)
        out.append((nout - npad, np.concatenate([order, np.full(npad, order[-1], dtype=np.int32)]), npad))
    out.append((nout + 2, rng.permutation(nout + 2)[:nout].astype(np.int32), None))
    return out


@pytest.mark.parametrize("nout,nrest", GATHER_SHAPES)
def test_gather_cols_and_scatter_cols(nout, nrest, be):
    rng = np.random.default_rng(nout + nrest)
    for ncol_in, perm_np, npad in gather_perms(nout, rng):
        a = rng.standard_normal((nrest, ncol_in)).astype(be.np_dtype)
        perm = dev(be, perm_np)
        buf, out = guarded(be, (nrest, nout))
        be._c("gather_cols", nout, ULL(nrest), perm, ncol_in, dev(be, a), out)
        assert same_bits(out.cpu().numpy(), ref.gather_cols(a, perm_np)), (ncol_in, npad)
        assert tail_untouched(buf, out)
        if npad is not None:           # the way back: scatter of the first ncol columns returns the input on every column
            buf2, back = guarded(be, (nrest, ncol_in))
            be._c("scatter_cols", ncol_in, ULL(nrest), perm, nout, out, ncol_in, back)
            assert same_bits(back.cpu().numpy(), a)
            assert tail_untouched(buf2, back)
        else:                           # scatter of a subset: the columns not named keep what they held
            src = rng.standard_normal((nrest, nout)).astype(be.np_dtype)
            n = max(nout - 1, 1)
            buf2, dst = guarded(be, (nrest, ncol_in))
            dst0 = dst.cpu().numpy().copy()
            be._c("scatter_cols", n, ULL(nrest), perm, nout, dev(be, src), ncol_in, dst)
            assert same_bits(dst.cpu().numpy(), ref.scatter_cols(src, perm_np, n, dst0))
            assert tail_untouched(buf2, dst)


@pytest.mark.parametrize("n1", [1, 4, 17])
@pytest.mark.parametrize("nout", [1, 3, 17, 255, 257, 65537])
def test_gather_lastdim(nout, n1, be):
    """(n1, ncol) arrays, e.g. emis_sfc(nbnd, ncol); 17 x 17 is the square case on which a transposed source index stays in bounds"""
    rng = np.random.default_rng(100*n1 + nout)
    for ncol_in, perm_np, npad in gather_perms(nout, rng):
        a = rng.standard_normal((ncol_in, n1)).astype(be.np_dtype)
        buf, out = guarded(be, (nout, n1))
        be._c("gather_lastdim", n1, nout, dev(be, perm_np), dev(be, a), out)
        assert same_bits(out.cpu().numpy(), ref.gather_lastdim(a, perm_np)), (ncol_in, npad)
        assert tail_untouched(buf, out)


def test_gathers_and_scatter_do_nothing_on_empty_problems(be):
    rng = np.random.default_rng(5)
    a = rng.standard_normal((3, 5)).astype(be.np_dtype)
    perm_np = np.array([4, 0, 2, 2], dtype=np.int32)
    perm, src = dev(be, perm_np), dev(be, a)
    buf, out = guarded(be, (3, 4))
    for nout, nrest in ((0, 3), (4, 0), (0, 0)):
        assert be._c("gather_cols", nout, ULL(nrest), perm, 5, src, out) == 0
        assert be._c("scatter_cols", nout, ULL(nrest), perm, 5, src, 4, out) == 0
    for n1, nout in ((0, 4), (3, 0)):
        assert be._c("gather_lastdim", n1, nout, perm, src, out) == 0
    assert (buf == GUARD).all()
    be._c("gather_cols", 4, ULL(3), perm, 5, src, out)                 # valid calls straight afterwards
    assert same_bits(out.cpu().numpy(), ref.gather_cols(a, perm_np))
    buf, out = guarded(be, (4, 5))
    be._c("gather_lastdim", 5, 4, dev(be, np.array([2, 0, 1, 1], dtype=np.int32)), src, out)
    assert same_bits(out.cpu().numpy(), ref.gather_lastdim(a, np.array([2, 0, 1, 1])))
    assert tail_untouched(buf, out)


# ==== glue (csrc/rrx_misc.hip) =================================================================================================
def subset_nd_call(be, a, starts, sub_dims, elem_bytes=None):
    """rrx_subset_nd on numpy array `a` (axes = the ABI's dimensions reversed). The source is uploaded into a buffer long enough
    that a kernel which treated a broadcast dimension like a sliced one would still read inside it. Returns (got, want)."""
    want, strides, spread = ref.subset_nd(a, starts, sub_dims)
    reach = 1 + sum((s + n - 1)*st for s, n, st in zip(starts, sub_dims, strides))
    src = torch.zeros((max(a.size, reach),), dtype=torch.from_numpy(a).dtype, device=be.device)
    src[:a.size] = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1).to(be.device)
    buf, out = guarded(be, want.shape, src.dtype)
    nd = len(sub_dims)
    be.lib.call("rrx_subset_nd", out, src, a.dtype.itemsize if elem_bytes is None else elem_bytes, nd, int_array(sub_dims),
                (ctypes.c_longlong * nd)(*strides), int_array(starts), int_array(spread), be._st())
    assert tail_untouched(buf, out)
    return out.cpu().numpy(), want


SUBSET_ND_CASES = {     # dims, starts, sub_dims in the ABI's order (first = fastest); a dimension of extent 1 is broadcast
    "1d-interior": ([37], [5], [20]),
    "1d-whole": ([37], [0], [37]),
    "1d-one-element": ([37], [36], [1]),
    "1d-broadcast": ([1], [0], [9]),
    "3d-slices-extent-1-block": ([7, 5, 6], [2, 1, 3], [4, 1, 2]),
    "3d-whole": ([7, 5, 6], [0, 0, 0], [7, 5, 6]),
    "3d-broadcast-first": ([1, 6, 3], [0, 2, 1], [5, 3, 2]),
    "3d-broadcast-middle": ([5, 1, 4], [1, 0, 0], [3, 3, 4]),
    "3d-broadcast-last": ([4, 3, 1], [0, 1, 0], [4, 2, 3]),
    "3d-several-workgroups": ([300, 7, 1], [20, 1, 0], [257, 5, 3]),
    "7d-broadcast-middle": ([3, 2, 1, 4, 2, 3, 2], [1, 0, 0, 2, 1, 0, 1], [2, 2, 5, 2, 1, 3, 1]),
    "7d-broadcast-first-and-last": ([1, 2, 3, 2, 2, 2, 1], [0, 1, 1, 0, 0, 1, 0], [4, 1, 2, 2, 2, 1, 3]),
}


@pytest.mark.parametrize("dtype", [np.int8, np.int32, np.float64], ids=["1-byte", "4-byte", "8-byte"])
@pytest.mark.parametrize("case", sorted(SUBSET_ND_CASES))
def test_subset_nd(case, dtype, hip_f64):
    dims, starts, sub_dims = SUBSET_ND_CASES[case]
    rng = np.random.default_rng(len(case))
    a = rng.integers(-100, 100, size=tuple(dims[::-1])).astype(dtype)
    if dtype == np.float64:
        a = a + rng.uniform(0., 1., a.shape)
    got, want = subset_nd_call(hip_f64, a, starts, sub_dims)
    assert same_bits(got, want)


def test_subset_nd_refusals_and_empty_block(hip_f64):
    be = hip_f64
    a = np.arange(24, dtype=np.int32)
    src = dev(be, a)
    buf, out = guarded(be, (24,), torch.int32)

    def call(elem_bytes, ndim, sub):
        n = max(ndim, 1)
        return be.lib.call("rrx_subset_nd", out, src, elem_bytes, ndim, int_array(sub), (ctypes.c_longlong * n)(*([1]*n)),
                           int_array([0]*n), int_array([0]*n), be._st())
    for ndim in (0, 8):
        with pytest.raises(RuntimeError, match="ndim"):
            call(4, ndim, [1]*max(ndim, 1))
    for eb in (2, 0, 16):
        with pytest.raises(RuntimeError, match="element size"):
            call(eb, 1, [24])
    assert call(4, 1, [0]) == 0                                        # an empty block: nothing written
    assert (buf == GUARD).all()
    got, want = subset_nd_call(be, a.reshape(2, 3, 4), [1, 0, 1], [2, 3, 1])        # a valid call straight afterwards
    assert same_bits(got, want)


COL_RANGES = [(1, 7), (39, 7), (12, 20), (1, 45), (45, 1)]             # (col_s 1-based, ncol_sub) of 45: first, last, interior, whole


@pytest.mark.parametrize("col_s,ncol_sub", COL_RANGES)
def test_subset_cols_and_subset_lastdim(col_s, ncol_sub, be):
    rng = np.random.default_rng(col_s)
    ncol, nrest = 45, 3*21
    a = rng.standard_normal((nrest, ncol)).astype(be.np_dtype)
    buf, out = guarded(be, (nrest, ncol_sub))
    be._c("subset_cols", ncol, nrest, col_s, ncol_sub, dev(be, a), out)
    assert same_bits(out.cpu().numpy(), np.ascontiguousarray(a[:, col_s-1:col_s-1+ncol_sub]))
    assert tail_untouched(buf, out)
    assert same_bits(be.subset_cols(dev(be, a), col_s, ncol_sub).cpu().numpy(), out.cpu().numpy())
    n1 = 16
    b = rng.standard_normal((ncol, n1)).astype(be.np_dtype)
    buf, out = guarded(be, (ncol_sub, n1))
    be._c("subset_lastdim", n1, ncol, col_s, ncol_sub, dev(be, b), out)
    assert same_bits(out.cpu().numpy(), np.ascontiguousarray(b[col_s-1:col_s-1+ncol_sub]))
    assert tail_untouched(buf, out)


def test_subset_ranges_outside_the_array_and_empty_ranges(be):
    rng = np.random.default_rng(2)
    ncol, nrest = 45, 6
    a = rng.standard_normal((nrest, ncol)).astype(be.np_dtype)
    src = dev(be, a)
    buf, out = guarded(be, (nrest, ncol))
    for col_s, ncol_sub in ((40, 7), (46, 1), (0, 3), (1, 46)):        # (40, 7) ends one column past the end
        with pytest.raises(RuntimeError, match="column range outside the full array"):
            be._c("subset_cols", ncol, nrest, col_s, ncol_sub, src, out)
        with pytest.raises(RuntimeError, match="column range outside the full array"):
            be._c("subset_lastdim", nrest, ncol, col_s, ncol_sub, src, out)
    assert be._c("subset_cols", ncol, nrest, 3, 0, src, out) == 0
    assert be._c("subset_cols", ncol, 0, 3, 5, src, out) == 0
    assert be._c("subset_lastdim", nrest, ncol, 3, 0, src, out) == 0
    assert be._c("subset_lastdim", 0, ncol, 3, 5, src, out) == 0
    assert (buf == GUARD).all()
    buf, out = guarded(be, (nrest, 5))
    be._c("subset_cols", ncol, nrest, 3, 5, src, out)                  # valid calls straight afterwards
    assert same_bits(out.cpu().numpy(), np.ascontiguousarray(a[:, 2:7])) and tail_untouched(buf, out)
    b = a.reshape(ncol, nrest)
    buf, out = guarded(be, (5, nrest))
    be._c("subset_lastdim", nrest, ncol, 3, 5, src, out)
    assert same_bits(out.cpu().numpy(), np.ascontiguousarray(b[2:7])) and tail_untouched(buf, out)


@pytest.mark.parametrize("narr", [1, 2, 3, 4])
def test_get_from_subset(narr, be):
    """the subset lands in the first, the last and an interior position; the other columns keep their values"""
    rng = np.random.default_rng(narr)
    ncol, nlay, nbnd, ncol_in = 45, 21, 3, 7
    for col_s in (1, ncol - ncol_in + 1, 12):
        fulls0 = [rng.standard_normal((nbnd, nlay, ncol)).astype(be.np_dtype) for _ in range(narr)]
        subs0 = [rng.standard_normal((nbnd, nlay, ncol_in)).astype(be.np_dtype) for _ in range(narr)]
        fulls = [guarded_copy(be, f) for f in fulls0]
        be.get_from_subset(ncol, nlay, nbnd, ncol_in, col_s, [f for _, f in fulls], [dev(be, s) for s in subs0])
        for (buf, f), want in zip(fulls, ref.get_from_subset(fulls0, subs0, col_s)):
            assert same_bits(f.cpu().numpy(), want), col_s
            assert tail_untouched(buf, f), col_s


def test_get_from_subset_refusals_and_empty_problems(be):
    rng = np.random.default_rng(7)
    ncol, nlay, ncol_in = 45, 5, 7
    full0 = rng.standard_normal((nlay, ncol)).astype(be.np_dtype)
    sub0 = rng.standard_normal((nlay, ncol_in)).astype(be.np_dtype)
    buf, full = guarded_copy(be, full0)
    sub = dev(be, sub0)
    PA = ctypes.c_void_p * 4
    pf, ps = PA(full.data_ptr(), 0, 0, 0), PA(sub.data_ptr(), 0, 0, 0)
    for narr in (0, 5):
        with pytest.raises(RuntimeError, match="narr"):
            be._c("get_from_subset", ncol, nlay, 1, ncol_in, 1, narr, pf, ps)
    for col_s in (0, ncol - ncol_in + 2):                              # the second ends one column past the end
        with pytest.raises(RuntimeError, match="column range outside the full array"):
            be._c("get_from_subset", ncol, nlay, 1, ncol_in, col_s, 1, pf, ps)
    assert be._c("get_from_subset", ncol, nlay, 1, 0, 4, 1, pf, ps) == 0
    assert be._c("get_from_subset", ncol, 0, 1, ncol_in, 4, 1, pf, ps) == 0
    assert be._c("get_from_subset", ncol, nlay, 0, ncol_in, 4, 1, pf, ps) == 0
    assert same_bits(full.cpu().numpy(), full0) and tail_untouched(buf, full)
    be.get_from_subset(ncol, nlay, 1, ncol_in, 4, [full], [sub])      # a valid call straight afterwards
    assert same_bits(full.cpu().numpy(), ref.get_from_subset([full0], [sub0], 4)[0]) and tail_untouched(buf, full)


@pytest.mark.parametrize("n", [1, 255, 1048577])                       # 1 048 577 = one more than the grid's 4 096 x 256 threads
def test_fill(n, be):
    for value in (1.5, float.fromhex("-0x1.5555555555555p-3")):
        value = float(be.np_dtype.type(value))                         # (representable in the array's type: the call rounds nothing)
        buf, out = guarded(be, (n,))
        be._c("fill", ULL(n), value, out)
        assert same_bits(out.cpu().numpy(), np.full(n, value, dtype=be.np_dtype))
        assert tail_untouched(buf, out)


def test_fill_of_nothing(be):
    buf, out = guarded(be, (4,))
    assert be._c("fill", ULL(0), 3.0, out) == 0
    assert (buf == GUARD).all()
    be._c("fill", ULL(4), -0.0, out)                                   # a valid call straight afterwards
    assert same_bits(out.cpu().numpy(), np.full(4, -0.0, dtype=be.np_dtype)) and tail_untouched(buf, out)


def gas_sources(ngas, nlay, ncol, rng, dtype):
    """ngas concentrations, scalar / (1, nlay) profile / (ncol, nlay) field in turn: numpy arrays (1, 1), (nlay, 1), (nlay, ncol)"""
    shapes = [(1, 1), (nlay, 1), (nlay, ncol)]
    return [rng.uniform(1e-9, 1e-2, shapes[i % 3]).astype(dtype) for i in range(ngas)]


def abi_dims(v):
    return v.shape[1], v.shape[0]


@pytest.mark.parametrize("ngas", [0, 1, 3, 32])
def test_fill_gases_all_and_the_per_gas_loop(ngas, be):
    """col_gas = vmr * col_dry, one multiplication: bit for bit, from the one-launch entry and from the per-gas entry (which also
    keeps the broadcast vmr)"""
    rng = np.random.default_rng(ngas)
    ncol, nlay = 45, 7
    col_dry_np = rng.uniform(1e20, 1e24, (nlay, ncol)).astype(be.np_dtype)
    vm = gas_sources(ngas, nlay, ncol, rng, be.np_dtype)
    want = ref.fill_gases(col_dry_np, vm)
    col_dry, vt = dev(be, col_dry_np), [dev(be, v) for v in vm]
    buf, col_gas = guarded(be, (ngas + 1, nlay, ncol))
    be._c("fill_gases_all", ncol, nlay, ngas, (ctypes.c_void_p * ngas)(*[v.data_ptr() for v in vt]),
          int_array([abi_dims(v)[0] for v in vm]), int_array([abi_dims(v)[1] for v in vm]), col_gas, col_dry)
    assert same_bits(col_gas.cpu().numpy(), want)
    assert tail_untouched(buf, col_gas)
    buf2, col_gas2 = guarded(be, (ngas + 1, nlay, ncol))
    bufv, vmr = guarded(be, (ngas, nlay, ncol))
    be._c("fill_gases", ncol, nlay, ncol, nlay, ngas, 0, vmr, col_dry, col_gas2, col_dry)
    for i, (v, t) in enumerate(zip(vm, vt), start=1):
        be._c("fill_gases", ncol, nlay, *abi_dims(v), ngas, i, vmr, t, col_gas2, col_dry)
    assert same_bits(col_gas2.cpu().numpy(), want)
    assert same_bits(vmr.cpu().numpy(), np.ascontiguousarray(np.stack([np.broadcast_to(v, (nlay, ncol)) for v in vm]))
                     if ngas else np.zeros((0, nlay, ncol), dtype=be.np_dtype))
    assert tail_untouched(buf2, col_gas2) and tail_untouched(bufv, vmr)


def test_fill_gases_refusals_and_empty_problems(be):
    rng = np.random.default_rng(1)
    ncol, nlay = 9, 4
    col_dry_np = rng.uniform(1e20, 1e24, (nlay, ncol)).astype(be.np_dtype)
    col_dry = dev(be, col_dry_np)
    vm = gas_sources(33, nlay, ncol, rng, be.np_dtype)
    vt = [dev(be, v) for v in vm]
    ptrs = (ctypes.c_void_p * 33)(*[v.data_ptr() for v in vt])
    d1, d2 = int_array([abi_dims(v)[0] for v in vm]), int_array([abi_dims(v)[1] for v in vm])
    buf, col_gas = guarded(be, (34, nlay, ncol))
    for ngas in (33, -1):
        with pytest.raises(RuntimeError, match="more gases"):
            be._c("fill_gases_all", ncol, nlay, ngas, ptrs, d1, d2, col_gas, col_dry)
    assert be._c("fill_gases_all", 0, nlay, 3, ptrs, d1, d2, col_gas, col_dry) == 0
    assert be._c("fill_gases_all", ncol, 0, 3, ptrs, d1, d2, col_gas, col_dry) == 0
    assert be._c("fill_gases", 0, nlay, 1, 1, 3, 1, col_gas, vt[0], col_gas, col_dry) == 0
    assert (buf == GUARD).all()
    be._c("fill_gases_all", ncol, nlay, 3, ptrs, d1, d2, col_gas, col_dry)        # a valid call straight afterwards
    assert same_bits(col_gas.cpu().numpy()[:4], ref.fill_gases(col_dry_np, vm[:3]))


@pytest.mark.parametrize("ngas", [3, 33])
def test_hip_kernels_fill_gases_takes_profiles_of_one_dimension(ngas, be):
    """HipKernels.fill_gases: up to 32 gases in one launch, more through the per-gas entry (no k-distribution of the suite has that
    many); a profile may come as (nlay,) -- it used to be read as a scalar, element 0 for every layer -- or as (nlay, 1); a scalar
    as any one-element tensor; other shapes are refused by name."""
    rng = np.random.default_rng(ngas)
    ncol, nlay = 45, 7
    col_dry_np = rng.uniform(1e20, 1e24, (nlay, ncol)).astype(be.np_dtype)
    vm = gas_sources(ngas, nlay, ncol, rng, be.np_dtype)
    names = [f"gas{i}" for i in range(ngas)]
    kd = types.SimpleNamespace(ngas=ngas, gas_names=names)
    given = {}
    for i, (name, v) in enumerate(zip(names, vm)):
        if v.shape == (1, 1):
            given[name] = dev(be, v.reshape(1) if i % 2 else v)
        elif v.shape == (nlay, 1):
            given[name] = dev(be, v.reshape(nlay) if i % 2 else v)
        else:
            given[name] = dev(be, v)
    assert any(t.dim() == 1 and t.numel() == nlay for t in given.values())
    got = be.fill_gases(kd, given, dev(be, col_dry_np))
    assert same_bits(got.cpu().numpy(), ref.fill_gases(col_dry_np, vm))
    for bad in ((nlay + 1,), (ncol,), (ncol, nlay), (nlay, ncol, 1)):
        given[names[1]] = torch.zeros(bad, dtype=be.tdtype, device=be.device)
        with pytest.raises(ValueError, match=names[1]):
            be.fill_gases(kd, given, dev(be, col_dry_np))


@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
@pytest.mark.parametrize("ncol,nlay", [(1, 1), (65, 3), (300, 40)])
def test_heating_rate(ncol, nlay, top_at_1, be, capsys):
    """Against -(g/cp)*(F[k+1]-F[k])/(p[k+1]-p[k]) in np.longdouble from the rounded inputs, relative and elementwise. Bound: 8
    machine epsilons of the result type -- the kernel is four rounded operations on exact inputs (two differences, a product, a
    quotient), each allowed 2 ulp to cover an fp32 division that is not correctly rounded; each error is relative to that
    operation's own result, so the cancellation in the flux difference does not enter."""
    rng = np.random.default_rng(1000*ncol + nlay + top_at_1)
    g_over_cp = float(be.np_dtype.type(9.80665/1004.64))
    dp = rng.uniform(50., 5000., (nlay, ncol))
    plev = 100. + np.concatenate([np.zeros((1, ncol)), np.cumsum(dp, axis=0)])         # pressure grows with the index: top first
    if not top_at_1:
        plev = plev[::-1]
    plev = np.ascontiguousarray(plev.astype(be.np_dtype))
    flux = rng.uniform(-300., 300., (nlay + 1, ncol)).astype(be.np_dtype)
    buf, hr = guarded(be, (nlay, ncol))
    be._c("heating_rate", ncol, nlay, g_over_cp, dev(be, flux), dev(be, plev), hr)
    want = ref.heating_rate(flux, plev, g_over_cp)
    assert (want != 0).all()
    got = hr.cpu().numpy()
    err = float(np.max(np.abs(got.astype(np.longdouble) - want) / np.abs(want)) / np.finfo(be.np_dtype).eps)
    with capsys.disabled():
        print(f"\n  heating_rate {be.sfx} ncol={ncol} nlay={nlay} top_at_1={top_at_1}: worst error {err:.3f} eps", end="")
    assert err <= 8.0                  # observed on an MI355X: at most 1.53 eps in fp64 and 1.25 eps in fp32 ((300, 40), top0 / top1)
    assert tail_untouched(buf, hr)
    assert same_bits(be.heating_rate(dev(be, flux), dev(be, plev), g_over_cp).cpu().numpy(), got)       # the wrapper: same call



def test_heating_rate_of_nothing(be):
    buf, hr = guarded(be, (3, 5))
    flux = dev(be, np.arange(20, dtype=be.np_dtype).reshape(4, 5)**2)
    plev = dev(be, (1000. - 100.*np.arange(20, dtype=be.np_dtype)).reshape(4, 5))
    assert be._c("heating_rate", 0, 3, 0.5, flux, plev, hr) == 0
    assert be._c("heating_rate", 5, 0, 0.5, flux, plev, hr) == 0
    assert (buf == GUARD).all()
    be._c("heating_rate", 5, 3, 0.5, flux, plev, hr)                   # a valid call straight afterwards
    want = ref.heating_rate(flux.cpu().numpy(), plev.cpu().numpy(), 0.5)
    assert np.max(np.abs(hr.cpu().numpy() - want) / np.abs(want)) <= 8*np.finfo(be.np_dtype).eps


# ---- by band ---------------------------------------------------------------------------------------------------------------------
BAND_LAYOUTS = {"uneven": [1, 3, 8, 16, 40], "one-per-gpoint": [1]*24, "one-band": [48], "empty-inside": [8, 0, 16, 8],
                "empty-at-ends": [0, 16, 16, 0]}
LAYOUT_IDS = list(BAND_LAYOUTS)


def spectral_fluxes(sizes, nlev, ncol, rng, dtype):
    """(ngpt, nlev, ncol) values of either sign; column 0 is -0.0 at every g-point (a sum started from zero would give +0.0)"""
    a = rng.uniform(-9., 9., (sum(sizes), nlev, ncol)).astype(dtype)
    a[:, :, 0] = -0.0
    return a


@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_sum_byband_and_net_byband_full(layout, be):
    """numpy sums in g-point order, bit for bit (additions and one subtraction per g-point only); empty bands are exact zeros,
    also where the band's first g-point lies behind the last one (empty-at-ends)"""
    sizes = BAND_LAYOUTS[layout]
    rng = np.random.default_rng(len(sizes))
    nlev, ncol = 7, 45
    lims_np = ref.band_layout(sizes)
    dn, up = (spectral_fluxes(sizes, nlev, ncol, rng, be.np_dtype) for _ in range(2))
    lims = dev(be, lims_np)
    ngpt, nbnd = sum(sizes), len(sizes)
    buf, out = guarded(be, (nbnd, nlev, ncol))
    be._c("sum_byband", ncol, nlev, ngpt, nbnd, lims, dev(be, dn), out)
    got = out.cpu().numpy()
    assert same_bits(got, ref.sum_byband(dn, lims_np))
    assert tail_untouched(buf, out)
    buf, out = guarded(be, (nbnd, nlev, ncol))
    be._c("net_byband_full", ncol, nlev, ngpt, nbnd, lims, dev(be, dn), dev(be, up), out)
    net = out.cpu().numpy()
    assert same_bits(net, ref.net_byband(dn, up, lims_np))
    assert tail_untouched(buf, out)
    for ib, n in enumerate(sizes):
        if n == 0:
            assert same_bits(got[ib], np.zeros((nlev, ncol), dtype=be.np_dtype)), ib
            assert same_bits(net[ib], np.zeros((nlev, ncol), dtype=be.np_dtype)), ib
        else:
            assert np.signbit(got[ib][:, 0]).all(), ib                 # -0.0 + -0.0 + ...: the sum does not start from +0.0
    assert same_bits(be.sum_byband(dev(be, dn), lims).cpu().numpy(), got)                  # the wrappers: the same calls
    assert same_bits(be.net_byband_full(dev(be, dn), dev(be, up), lims).cpu().numpy(), net)


@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_increments_by_band(layout, be):
    """tau(gpt) += tau(band of gpt): bit for bit. The two-stream form: tau bit for bit; ssa and g against the kernel's expressions
    in np.longdouble at 5 machine epsilons -- all terms are non-negative here (g >= 0), so rounding errors add and are never
    amplified; the worst path holds 6 rounded operations (numerator: two products and a sum, denominator: a product and a sum,
    the quotient), each within half an epsilon when correctly rounded (a fused multiply-add only removes one), the fp32 quotient
    allowed 2: 4.5 in all. The g-points of no band keep their bits."""
    sizes = BAND_LAYOUTS[layout]
    rng = np.random.default_rng(10 + len(sizes))
    nlay, ncol = 7, 45
    ngpt_in, nbnd = sum(sizes), len(sizes)
    lims_np = ref.band_layout(sizes)
    if layout == "one-band":           # g-points in front of and behind the one band belong to no band
        lims_np = lims_np + 5
    ngpt = int(lims_np.max()) + (4 if layout == "one-band" else 0)
    ngpt = max(ngpt, ngpt_in)
    lims = dev(be, lims_np)
    shp, bshp = (ngpt, nlay, ncol), (nbnd, nlay, ncol)
    t1 = 10.0**rng.uniform(-4, 1.5, shp); w1 = rng.uniform(0., 1., shp); g1 = rng.uniform(0., .9, shp)
    t2 = 10.0**rng.uniform(-4, 1.5, bshp); w2 = rng.uniform(0., 1., bshp); g2 = rng.uniform(0., .9, bshp)
    t1, w1, g1, t2, w2, g2 = (x.astype(be.np_dtype) for x in (t1, w1, g1, t2, w2, g2))
    in_band = ref.gpoint_band(lims_np, ngpt) >= 0
    if layout == "one-band":
        assert not in_band[:5].any() and not in_band[-4:].any() and in_band.sum() == 48
    # one scalar
    buf, tau = guarded_copy(be, t1)
    be._c("inc_1scalar_by_1scalar_bybnd", ncol, nlay, ngpt, tau, dev(be, t2), nbnd, lims)
    assert same_bits(tau.cpu().numpy(), ref.inc_1scalar_bybnd(t1, t2, lims_np))
    assert same_bits(tau.cpu().numpy()[~in_band], t1[~in_band])
    assert tail_untouched(buf, tau)
    # two-stream
    (bt, T), (bw, W), (bg, G) = (guarded_copy(be, x) for x in (t1, w1, g1))
    be._c("inc_2stream_by_2stream_bybnd", ncol, nlay, ngpt, T, W, G, dev(be, t2), dev(be, w2), dev(be, g2), nbnd, lims)
    Tr, Wr, Gr = ref.inc_2stream_bybnd(t1, w1, g1, t2, w2, g2, lims_np, 3*np.finfo(be.np_dtype).tiny)
    assert same_bits(T.cpu().numpy(), Tr)
    eps = np.finfo(be.np_dtype).eps
    for name, got, want, orig in (("ssa", W.cpu().numpy(), Wr, w1), ("g", G.cpu().numpy(), Gr, g1)):
        assert same_bits(got[~in_band], orig[~in_band]), name
        if in_band.any():
            err = np.max(np.abs(got[in_band].astype(np.longdouble) - want[in_band]) / np.abs(want[in_band]))
            assert err <= 5*eps, (name, float(err/eps))
    assert tail_untouched(bt, T) and tail_untouched(bw, W) and tail_untouched(bg, G)


@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_expand_and_transpose(layout, be):
    """(nbnd, ncol) -> (ncol, ngpt): 300 columns (two workgroups); the g-points of no band (empty bands own none) are not written"""
    sizes = BAND_LAYOUTS[layout]
    rng = np.random.default_rng(20 + len(sizes))
    ncol, nbnd = 300, len(sizes)
    lims_np = ref.band_layout(sizes)
    if layout == "one-band":
        lims_np = lims_np + 5
    ngpt = int(lims_np.max()) + 4
    arr = rng.standard_normal((ncol, nbnd)).astype(be.np_dtype)
    buf, out = guarded(be, (ngpt, ncol))
    before = out.cpu().numpy().copy()
    be._c("expand_and_transpose", ncol, nbnd, dev(be, lims_np), dev(be, arr), out)
    got = out.cpu().numpy()
    assert same_bits(got, ref.expand_and_transpose(arr, lims_np, ngpt, before))
    assert (got[ref.gpoint_band(lims_np, ngpt) < 0] == GUARD).all()
    assert tail_untouched(buf, out)


def test_byband_entries_do_nothing_on_empty_problems(be):
    rng = np.random.default_rng(4)
    sizes = [2, 0, 3]
    lims_np = ref.band_layout(sizes)
    lims = dev(be, lims_np)
    nlev, ncol, ngpt, nbnd = 3, 5, 5, 3
    a = spectral_fluxes(sizes, nlev, ncol, rng, be.np_dtype)
    b = rng.standard_normal((nbnd, nlev, ncol)).astype(be.np_dtype)
    src, bnd = dev(be, a), dev(be, b)
    buf, out = guarded(be, (ngpt, nlev, ncol))
    for nc, nl, nb in ((0, nlev, nbnd), (ncol, 0, nbnd), (ncol, nlev, 0)):
        assert be._c("sum_byband", nc, nl, ngpt, nb, lims, src, out) == 0
        assert be._c("net_byband_full", nc, nl, ngpt, nb, lims, src, src, out) == 0
        assert be._c("inc_1scalar_by_1scalar_bybnd", nc, nl, ngpt, out, bnd, nb, lims) == 0
        assert be._c("inc_2stream_by_2stream_bybnd", nc, nl, ngpt, out, out, out, bnd, bnd, bnd, nb, lims) == 0
        if nc == 0 or nb == 0:
            assert be._c("expand_and_transpose", nc, nb, lims, bnd, out) == 0
    assert be._c("inc_1scalar_by_1scalar_bybnd", ncol, nlev, 0, out, bnd, nbnd, lims) == 0
    assert (buf == GUARD).all()
    buf, out = guarded(be, (nbnd, nlev, ncol))
    be._c("sum_byband", ncol, nlev, ngpt, nbnd, lims, src, out)        # valid calls straight afterwards
    assert same_bits(out.cpu().numpy(), ref.sum_byband(a, lims_np)) and tail_untouched(buf, out)
    buf, tau = guarded_copy(be, a)
    be._c("inc_1scalar_by_1scalar_bybnd", ncol, nlev, ngpt, tau, bnd, nbnd, lims)
    assert same_bits(tau.cpu().numpy(), ref.inc_1scalar_bybnd(a, b, lims_np)) and tail_untouched(buf, tau)
    buf, out = guarded(be, (ngpt, ncol))
    arr = rng.standard_normal((ncol, nbnd)).astype(be.np_dtype)
    be._c("expand_and_transpose", ncol, nbnd, lims, dev(be, arr), out)
    assert same_bits(out.cpu().numpy(), ref.expand_and_transpose(arr, lims_np, ngpt, np.full((ngpt, ncol), GUARD, dtype=be.np_dtype)))


@pytest.mark.parametrize("layout", ["empty-inside", "empty-at-ends"])
def test_sum_byband_is_the_fused_sw_solvers_band_sum(layout, hip_f64):
    """include/rrx_hip.h on the fused by-band solvers: "a band with hi < lo is empty (zeros) ... as rrx_sum_byband". The per-g-point
    SW solver + rrx_sum_byband against bnd_flux_* of rrx_sw_solver_2stream_byband on layouts with empty bands: 1e-11, the
    tolerance of tests/test_gpu_byband.py for this pair (the two solver kernels differ in the last bits); empty bands exact zeros
    on both sides."""
    be = hip_f64
    sizes = BAND_LAYOUTS[layout]
    rng = np.random.default_rng(len(layout))
    ngpt, nlay, ncol = sum(sizes), 60, 45
    shp = (ngpt, nlay, ncol)
    up = be.asarray
    tau, ssa, g = up(10.0**rng.uniform(-4, 1.5, shp)), up(rng.uniform(0., 1., shp)), up(rng.uniform(-0.3, 0.9, shp))
    mu0 = up(rng.uniform(0.05, 1.0, ncol))
    adir, adif, inc = (up(rng.uniform(0., hi, (ngpt, ncol))) for hi in (0.6, 0.6, 5.))
    lims_np = ref.band_layout(sizes)
    lims = dev(be, lims_np)
    fused = be.sw_solver_2stream_byband(False, tau, ssa, g, mu0, adir, adif, inc, lims)
    per_gpt = be.sw_solver_2stream(False, tau, ssa, g, mu0, adir, adif, inc)
    for k in ("up", "dn", "dir"):
        want = be.sum_byband(per_gpt["flux_" + k], lims).cpu().numpy()
        got = fused["bnd_flux_" + k].cpu().numpy()
        assert same_bits(want, ref.sum_byband(per_gpt["flux_" + k].cpu().numpy(), lims_np)), k
        assert cases.rel_err(got, want) <= 1e-11, k
        for ib, n in enumerate(sizes):
            if n == 0:
                assert not want[ib].any() and not got[ib].any(), (k, ib)


# ==== the binding itself (rte-rrtmgp-cpp_amd/_ffi.py) =============================================================================
def test_binding_refuses_a_tensor_of_the_other_precision(be):
    """HipKernels calls go through the declarations of include/rrx_hip.h: gauss_Ds in the other precision is a TypeError that names
    the parameter, raised before the library is entered; with the right tensors the entry gives secants[imu, g, c] =
    gauss_Ds[n_quad-1, imu] as ever (rte_solver_kernels_launchers.cu:48-58)."""
    ncol, ngpt, n_quad = 4, 8, 1
    other = torch.float32 if be.tdtype == torch.float64 else torch.float64
    Ds = np.ascontiguousarray(pipeline.GAUSS_DS.astype(be.np_dtype))
    buf, out = guarded(be, (n_quad, ngpt, ncol))
    with pytest.raises(TypeError, match="gauss_Ds"):
        be.lw_secants_array(ncol, ngpt, n_quad, pipeline.MAX_GAUSS_PTS, dev(be, Ds).to(other), out=out)
    assert bool((buf == GUARD).all().item())                                                   # nothing ran
    with pytest.raises(TypeError, match="secants"):
        be.lw_secants_array(ncol, ngpt, n_quad, pipeline.MAX_GAUSS_PTS, dev(be, Ds), out=out.to(other))
    got = be.lw_secants_array(ncol, ngpt, n_quad, pipeline.MAX_GAUSS_PTS, dev(be, Ds), out=out)
    want = np.empty((n_quad, ngpt, ncol), dtype=be.np_dtype)
    want[:] = Ds.reshape(pipeline.MAX_GAUSS_PTS, pipeline.MAX_GAUSS_PTS)[n_quad-1, :n_quad, None, None]
    assert same_bits(got.cpu().numpy(), want) and tail_untouched(buf, out)
    assert same_bits(be.lw_secants_array(ncol, ngpt, n_quad, pipeline.MAX_GAUSS_PTS, dev(be, Ds)).cpu().numpy(), want)
