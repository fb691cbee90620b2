"""CPU tests of the numpy restatement of the McICA cloud sampling (tests/mcica_ref.py): the generator's known answers, the overlap
rules by construction and the statistics of the sampled cloud cover. The GPU tests compare the kernels with this restatement."""
import numpy as np
import pytest

import mcica_ref as M

SEED = 0x0123456789abcdef
NCOL, NLAY, NGPT = 70, 11, 16


def profile():
    f = np.zeros((NLAY,))
    f[2], f[3], f[4], f[7], f[10] = 0.3, 0.6, 0.45, 0.5, 1.0
    return f


def field(dtype=np.float64):
    return np.ascontiguousarray(np.broadcast_to(profile()[:, None], (NLAY, NCOL))).astype(dtype)


KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,)*4, (0xffffffff,)*2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    assert " ".join("%08x" % int(x) for x in M.philox4x32_10(ctr, key)) == want


def test_philox_is_elementwise():
    ctr = [np.array([c[i] for c, _, _ in KNOWN]) for i in range(4)]
    key = [np.array([k[i] for _, k, _ in KNOWN]) for i in range(2)]
    out = M.philox4x32_10(ctr, key)
    for j, (_, _, want) in enumerate(KNOWN):
        assert " ".join("%08x" % int(w[j]) for w in out) == want


def test_uniform_is_inside_the_unit_interval_and_the_same_in_both_precisions():
    x = np.concatenate([np.array([0, 1, 511, 512, 0x7fffffff, 0x80000000, 0xfffffe00, 0xffffffff], dtype=np.uint32),
                        np.random.default_rng(1).integers(0, 2**32, 4096, dtype=np.uint64).astype(np.uint32)])
    u32, u64 = M.uniform(x, np.float32), M.uniform(x, np.float64)
    assert u32.dtype == np.float32 and u64.dtype == np.float64
    assert np.all(u32 > 0) and np.all(u32 < 1) and np.all(u64 > 0) and np.all(u64 < 1)
    assert np.array_equal(u32.astype(np.float64), u64)
    assert u64.min() == 2.0**-24 and u64.max() == 1 - 2.0**-24


def test_draws_use_one_word_per_layer_and_the_column_identity():
    u = M.draws(SEED, 1, 0, [7, 3], 2, 6, np.float64)
    w = M.philox4x32_10((3, 1, 1, 2), (SEED & 0xffffffff, SEED >> 32))           # column 3, g-point 1, layers 4..7, domain 1, draw u
    assert u[1, 5, 1] == M.uniform(w[1], np.float64)
    v = M.draws(SEED, 1, 1, [7, 3], 2, 6, np.float64)
    w = M.philox4x32_10((7, 0, 0, 3), (SEED & 0xffffffff, SEED >> 32))
    assert v[0, 2, 0] == M.uniform(w[2], np.float64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_alpha_one_is_maximum_random(dtype):
    cf = field(dtype)
    ids = np.arange(NCOL)
    a = M.cloud_mask(cf, None, SEED, 0, ids, NGPT)
    b = M.cloud_mask(cf, np.ones((NLAY-1, NCOL), dtype=dtype), SEED, 0, ids, NGPT)
    assert np.array_equal(a, b)


def test_maximum_overlap_inside_a_block_nests_the_masks():
    m = M.cloud_mask(field(), None, SEED, 0, np.arange(NCOL), NGPT).astype(bool)
    assert np.all(m[:, 3] | ~m[:, 2])          # 0.3 inside 0.6
    assert np.all(m[:, 3] | ~m[:, 4])          # 0.45 inside 0.6
    assert np.all(m[:, 4] | ~m[:, 2])          # the rank is kept through the whole block: 0.3 inside 0.45


@pytest.mark.parametrize("alpha", [None, 0.7, 0.0])
def test_overcast_is_all_cloudy_and_clear_is_none(alpha):
    al = None if alpha is None else np.full((NLAY-1, NCOL), alpha)
    ids = np.arange(NCOL)
    assert np.all(M.cloud_mask(np.ones((NLAY, NCOL)), al, SEED, 0, ids, NGPT) == 1)
    assert np.all(M.cloud_mask(np.zeros((NLAY, NCOL)), al, SEED, 0, ids, NGPT) == 0)
    m = M.cloud_mask(field(), al, SEED, 1, ids, NGPT)
    assert np.all(m[:, 10] == 1) and np.all(m[:, [0, 1, 5, 6, 8, 9]] == 0)


@pytest.mark.parametrize("domain", [0, 1])
@pytest.mark.parametrize("alpha", [None, 0.7, 0.0])
def test_cloud_cover_statistics(alpha, domain):
    """Every layer's cloudy share within 4 sigma of its fraction, sigma^2 = f (1 - f) / 1120; layers 2 and 3 both cloudy within 4 sigma
    of alpha 0.3 + (1 - alpha) 0.18 (alpha = None: 1). The two-draw form keeps the marginal exact; this restatement stays within 1.9."""
    n = NCOL * NGPT
    assert n == 1120
    al = None if alpha is None else np.full((NLAY-1, NCOL), alpha)
    m = M.cloud_mask(field(), al, SEED, domain, np.arange(NCOL), NGPT).astype(bool)
    for ilay, f in enumerate(profile()):
        sigma = np.sqrt(f * (1 - f) / n)
        share = m[:, ilay].mean()
        print(f"alpha {alpha} domain {domain} layer {ilay}: share {share:.4f} of {f}, {abs(share - f) / max(sigma, 1e-300):.2f} sigma")
        assert abs(share - f) <= 4 * sigma
    a = 1.0 if alpha is None else alpha
    p = a * 0.3 + (1 - a) * 0.18
    sigma = np.sqrt(p * (1 - p) / n)
    both = (m[:, 2] & m[:, 3]).mean()
    print(f"alpha {alpha} domain {domain} layers 2 and 3: share {both:.4f} of {p:.4f}, {abs(both - p) / sigma:.2f} sigma")
    assert abs(both - p) <= 4 * sigma


def test_sampled_increments_touch_only_cloudy_cells_inside_a_band():
    rng = np.random.default_rng(3)
    ngpt, nlay, ncol = 8, 5, 6
    lims = np.array([[1, 3], [5, 4], [5, 7]])               # an empty band; g-points 4 and 8 belong to none
    cf = rng.uniform(0, 1, (nlay, ncol)) * (rng.uniform(0, 1, (nlay, ncol)) > 0.4)
    mask = M.cloud_mask(cf, None, 5, 0, np.arange(ncol), ngpt)
    tau, ssa, g = (rng.uniform(0.1, 1, (ngpt, nlay, ncol)) for _ in range(3))
    ct, cw, cg = (rng.uniform(0.1, 1, (3, nlay, ncol)) for _ in range(3))
    hit = M.sampled_mask(mask, lims)
    assert not hit[[3, 7]].any() and hit.any() and (~hit[:3]).any()
    t1 = M.increment_1scalar(tau, ct, mask, lims)
    assert np.array_equal(t1[~hit], tau[~hit])
    assert np.array_equal(t1[:3][hit[:3]], (tau[:3] + ct[0][None])[hit[:3]])
    t2, w2, g2 = M.increment_2stream(tau, ssa, g, ct, cw, cg, mask, lims)
    assert np.array_equal(t2, t1)
    for new, old in ((w2, ssa), (g2, g)):
        assert np.array_equal(new[~hit], old[~hit]) and np.all(new[hit] != old[hit])
    want_w = (tau*ssa + ct[2][None]*cw[2][None]) / (tau + ct[2][None])
    assert np.array_equal(w2[4:7][hit[4:7]], want_w[4:7][hit[4:7]])
