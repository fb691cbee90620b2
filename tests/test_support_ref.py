"""CPU tests of tests/support_ref.py, the numpy references of tests/test_gpu_support_kernels.py, on cases small enough to check by
eye: a wrong reference must not be able to make a wrong kernel pass."""
import numpy as np

import support_ref as ref


def test_subset_nd_2x3x2_with_a_broadcast_dimension():
    """ABI array a(2, 1, 2) (first index fastest: elements 0 1 | 2 3), block = rows 2..2 of dimension 1, the singleton dimension 2
    broadcast to 3, both entries of dimension 3 -> out(1, 3, 2)."""
    a = np.array([[[0, 1]], [[2, 3]]], dtype=np.int32)              # numpy axes (d3, d2, d1) = (2, 1, 2)
    out, strides, spread = ref.subset_nd(a, starts=[1, 0, 0], sub_dims=[1, 3, 2])
    assert strides == [1, 2, 2] and spread == [0, 1, 0]
    assert out.shape == (2, 3, 1)
    assert out.tolist() == [[[1], [1], [1]], [[3], [3], [3]]]
    # the whole 2 x 3 x 2 block of a(2, 1, 2): every element of the middle dimension repeats the 2 x 2 plane
    out, _, _ = ref.subset_nd(a, starts=[0, 0, 0], sub_dims=[2, 3, 2])
    assert out.tolist() == [[[0, 1], [0, 1], [0, 1]], [[2, 3], [2, 3], [2, 3]]]
    # no broadcast: plain slicing with non-zero starts
    b = np.arange(24).reshape(2, 3, 4)                                # ABI b(4, 3, 2)
    out, strides, spread = ref.subset_nd(b, starts=[1, 2, 0], sub_dims=[2, 1, 2])
    assert strides == [1, 4, 12] and spread == [0, 0, 0]
    assert out.tolist() == [[[9, 10]], [[21, 22]]]


def test_sort_of_five_columns_with_a_tie_and_padding():
    key = np.array([3., 1., 2., 1., 5.])
    assert ref.sort_perm(key, 0).tolist() == [1, 3, 2, 0, 4]         # the tie 1., 1. keeps its order (stable)
    assert ref.sort_perm(key, 3).tolist() == [1, 3, 2, 0, 4, 4, 4, 4]
    assert ref.sort_perm(np.array([2., -1., 1.]), 1).tolist() == [1, 2, 0, 0]
    assert ref.identity_perm(3, 2).tolist() == [0, 1, 2, 2, 2]
    assert ref.sort_perm(key, 0).dtype == np.int32 and ref.identity_perm(3, 2).dtype == np.int32


def test_column_spread_on_each_side_of_the_threshold():
    # runs of 4: [10 10 10 10] spans 0; [9 10 11 10] spans 2/10 = 0.2; [8 10 12 10] spans 4/10 = 0.4
    quiet, edge, wide = [10., 10., 10., 10.], [9., 10., 11., 10.], [8., 10., 12., 10.]
    assert ref.run_ratios(np.array(quiet + edge + wide), 4).tolist() == [0., 0.2, 0.4]
    assert ref.column_spread(np.array(quiet + wide), 4, 0.3) == 1
    assert ref.column_spread(np.array(wide + quiet), 4, 0.3) == 1
    assert ref.column_spread(np.array(quiet + edge), 4, 0.3) == 0
    assert ref.column_spread(np.array(edge), 4, 0.2) == 0              # strictly greater than threshold*mean
    assert ref.column_spread(np.array(edge), 4, 0.19) == 1
    assert ref.column_spread(np.array(quiet + wide[:3]), 4, 0.3) == 0  # a trailing partial run is ignored
    assert ref.column_spread(np.array(wide[:3]), 4, 0.3) == 0          # fewer columns than one run
    rng = np.random.default_rng(1)
    for n, ratio in ((16, 0.05), (256, 0.194), (300, 0.206), (1000, 0.5)):
        run = ref.spread_run(n, ratio, 9.0e4, rng)
        assert abs(ref.run_ratios(run, n)[0] - ratio) <= 1e-12*ratio


def test_band_sums_with_an_empty_band():
    lims = ref.band_layout([2, 0, 1])
    assert lims.tolist() == [[1, 2], [3, 2], [3, 3]]
    assert ref.band_layout([0, 2, 0]).tolist() == [[1, 0], [1, 2], [3, 2]]
    assert ref.gpoint_band(lims, 3).tolist() == [0, 0, 2]
    assert ref.gpoint_band(np.array([[2, 2]]), 3).tolist() == [-1, 0, -1]
    gpt = np.array([[1., -0.0], [2., -0.0], [4., -0.0]])               # (ngpt = 3, 2 cells)
    s = ref.sum_byband(gpt, lims)
    assert s.tolist() == [[3., 0.], [0., 0.], [4., 0.]]
    assert np.signbit(s[0, 1]) and np.signbit(s[2, 1])                  # -0.0 + -0.0 and a lone -0.0 stay -0.0
    assert not np.signbit(s[1]).any()                                   # the empty band is +0.0
    up = np.array([[0.5, 1.], [0.5, 1.], [0.5, 1.]])
    assert ref.net_byband(gpt, up, lims).tolist() == [[2., -2.], [0., 0.], [3.5, -1.]]


def test_gathers_scatter_and_the_small_references():
    a = np.array([[10, 11, 12], [20, 21, 22]])                         # (nrest = 2, ncol = 3)
    perm = np.array([2, 0, 1, 1])
    g = ref.gather_cols(a, perm)
    assert g.tolist() == [[12, 10, 11, 11], [22, 20, 21, 21]]
    assert ref.scatter_cols(g, perm, 3, np.zeros_like(a)).tolist() == a.tolist()
    assert ref.scatter_cols(g, perm, 1, np.full_like(a, -7)).tolist() == [[-7, -7, 12], [-7, -7, 22]]
    assert ref.gather_lastdim(a.T.copy(), perm).tolist() == [[12, 22], [10, 20], [11, 21], [11, 21]]
    full = [np.zeros((2, 4))]
    assert ref.get_from_subset(full, [np.ones((2, 2))], 2)[0].tolist() == [[0, 1, 1, 0], [0, 1, 1, 0]]
    cd = np.array([[1., 2.], [3., 4.]])                                 # (nlay = 2, ncol = 2)
    cg = ref.fill_gases(cd, [np.array([[2.]]), np.array([[1.], [10.]]), np.array([[1., 0.], [0., 1.]])])
    assert cg.tolist() == [[[1., 2.], [3., 4.]], [[2., 4.], [6., 8.]], [[1., 2.], [30., 40.]], [[1., 0.], [0., 4.]]]
    lims = np.array([[1, 2], [4, 4]], dtype=np.int32)
    e = ref.expand_and_transpose(np.array([[1., 2.], [3., 4.]]), lims, 4, np.full((4, 2), -7.))
    assert e.tolist() == [[1., 3.], [1., 3.], [-7., -7.], [2., 4.]]
    t = ref.inc_1scalar_bybnd(np.ones((4, 1)), np.array([[0.5], [0.25]]), lims)
    assert t.tolist() == [[1.5], [1.5], [1.], [1.25]]
    # heating rate: F = 10 -> 4 over p = 1000 -> 900: -(g/cp) * (-6)/(-100) = -0.06 g/cp
    hr = ref.heating_rate(np.array([[10.], [4.]]), np.array([[1000.], [900.]]), 0.5)
    assert hr.shape == (1, 1) and abs(float(hr[0, 0]) + 0.03) < 1e-15
