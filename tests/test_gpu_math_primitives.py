"""GPU tests of the solvers' hand-written math primitives (csrc/rrx_common.h: exp_neg in its polynomial, LDS-table and fp32 forms,
fast_rcp, sqrt_pos, sqrt_nonneg) evaluated ON THE DEVICE through rrx_math_selftest, against np.longdouble, in ulps. Their comments
quote accuracies that were measured on the host (a host model of the same arithmetic, against the C library); the solvers' accuracy
rests on them.

Error: |got - truth| over the ulp of the truth's binade in the run's dtype, never smaller than the smallest denormal (so a denormal
result is measured in units of the smallest denormal). Bound, per primitive: the figure its comment documents against the C library
plus 1 ulp, the C library's own documented bound against truth:
    exp_neg, polynomial form (fp64)   1.0 + 1 = 2.0 ulp
    exp_neg, LDS-table form (fp64)    1.3 + 1 = 2.3 ulp
    exp_neg (fp32)                    1 (v_exp_f32) + 1 = 2 ulp; a result below FLT_MIN may be flushed to 0 instead
    fast_rcp                          1 + 1 = 2 ulp
    sqrt_pos, sqrt_nonneg             1 + 1 = 2 ulp; sqrt_nonneg(0) is an exact 0 and a denormal argument gives a finite value
Arguments: a fixed grid of edges plus seeded draws, about 1e5 per primitive, inside the domain each comment states.

Measured on an MI355X (this file's prints; the figures beside the primitives in csrc/rrx_common.h are these):
    exp_neg, polynomial form (fp64)   1.02 ulp (at x = -294.92); denormal results within 0.75 of the smallest denormal
    exp_neg, LDS-table form (fp64)    1.27 ulp (at x = -3.50); denormal results within 1.08
    exp_neg (fp32)                    1.21 ulp (at x = -24.78); every result below FLT_MIN is 0
    fast_rcp                          0.50 ulp in both precisions (correctly rounded on the sample)
    sqrt_pos, sqrt_nonneg             0.50 ulp fp64, 0.90 ulp fp32; sqrt_nonneg has sqrt_pos's bits, sqrt_nonneg(0) = +0, the smallest normal
                                      is exact, a denormal gives 7.5e-167 (fp64) / 0 (fp32)
Every primitive is inside its documented figure. One CLAIM was wrong: the table form's comment promised that "an absurd argument still
ends in 0"; on the device exp_neg(-1e300, table) returns inf (beyond |x| = 1e77 the reduced argument, which is rounding residue by
then, overflows the polynomial). No solver argument is anywhere near, so the comment was corrected (0 down to about -1e60, asserted
here at -1e60) and the primitive left alone.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L = np.longdouble
N_DRAWS = 60000
LN2 = L(np.log(2.0)) + L(2.3190468138462996e-17)             # ln 2 to longdouble: the double and its tail
BOUND = {("exp_neg", "f64"): 2.0, ("exp_neg_table", "f64"): 2.3, ("exp_neg", "f32"): 2.0, ("exp_neg_table", "f32"): 2.0,
         "fast_rcp": 2.0, "sqrt_pos": 2.0, "sqrt_nonneg": 2.0}


def _be(dt, hip_f64, hip_f32):
    return (hip_f64, np.float64) if dt == "f64" else (hip_f32, np.float32)


def ulps(got, truth, F):
    """|got - truth| in ulps of F at truth (longdouble), the ulp never below F's smallest denormal"""
    fi = np.finfo(F)
    _, e = np.frexp(np.abs(truth))                             # |truth| = m 2^e, m in [0.5, 1): its binade starts at 2^(e - 1)
    ulp = np.ldexp(L(1), np.maximum(e - 1, fi.minexp) - fi.nmant)
    return (np.abs(got.astype(L) - truth) / ulp).astype(np.float64)


def run(be, primitive, x):
    return be.to_numpy(be.math_selftest(primitive, be.asarray(x)))


def exp_arguments(F):
    """x <= 0: zeros, tiny arguments, both sides of every reduction boundary -(k + 1/2) ln2 and -(k + 1/2) ln2/64 for small k, the
    range where the result is denormal and then 0, and seeded draws over the solver's range (log-uniform and uniform)"""
    rng = np.random.default_rng(11)
    fi = np.finfo(F)
    ln2 = float(LN2)
    under = -float(fi.minexp) * ln2                            # exp(-under) = the smallest normal
    zero_at = -float(fi.minexp - fi.nmant - 1) * ln2           # below exp(-zero_at) even the smallest denormal rounds to 0
    edges = [0.0, -0.0, -float(fi.tiny), -1e-300 if F == np.float64 else -1e-38, -1e-8]
    k = np.arange(0, 48)
    bnd = np.concatenate([-(k + 0.5) * ln2, -(np.arange(0, 400) + 0.5) * ln2 / 64]).astype(F)
    sides = [bnd]
    up, dn = bnd, bnd
    for _ in range(3):                                         # three neighbours on either side of each boundary
        up, dn = np.nextafter(up, F(0)), np.nextafter(dn, F(-np.inf))
        sides += [up, dn]
    denormal = np.linspace(-under * 0.985, -zero_at * 1.002, 20000)      # fp64: -698 ... -746.6; fp32: -86 ... -104.1
    draws = np.concatenate([-10.0**rng.uniform(-8, np.log10(under), N_DRAWS // 2), -rng.uniform(0, under, N_DRAWS // 2)])
    return np.concatenate([np.array(edges), *sides, denormal, draws]).astype(F)


@pytest.mark.parametrize("form", ["exp_neg", "exp_neg_table"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_exp_neg(dt, form, hip_f64, hip_f32):
    be, F = _be(dt, hip_f64, hip_f32)
    fi = np.finfo(F)
    x = exp_arguments(F)
    got = run(be, form, x)
    truth = np.exp(x.astype(L))
    e = ulps(got, truth, F)
    normal = truth >= L(fi.tiny)
    flushed = (got == 0) & ~normal
    ok = np.where(flushed & (dt == "f32"), 0.0, e)             # fp32: a result below FLT_MIN is 0 or within the bound
    worst_n, worst_d = float(e[normal].max()), float(ok[~normal].max())
    print(f"MATH {form} {dt} n={x.size}: normal results {worst_n:.3f} ulp (at x = {x[normal][e[normal].argmax()]!r}), "
          f"results below the smallest normal {worst_d:.3f} (units of the smallest denormal; {int(flushed.sum())} of {int((~normal).sum())} are 0), "
          f"bound {BOUND[(form, dt)]}")
    # far beyond the underflow, inside the domain each comment states: the result is an exact 0. The polynomial form: x > -1.4e9 (n
    # must fit an int); the table form: down to about -1e60; fp32 forms x log2(e) first, which must stay finite
    far = {("exp_neg", "f64"): [-1e3, -1e9], ("exp_neg_table", "f64"): [-1e3, -1e9, -1e60]}.get((form, dt), [-1e3, -1e9, -1e30])
    got_far = run(be, form, np.array(far, dtype=F))
    print(f"MATH {form} {dt} far arguments {far}: {got_far.tolist()}")
    if (form, dt) == ("exp_neg_table", "f64"):                 # outside that domain, reported only (see the docstring)
        print(f"MATH {form} {dt} at -1e300: {run(be, form, np.array([-1e300]))[0]!r}")
    assert np.isfinite(got).all()
    assert got[0] == 1 and got[1] == 1                         # x = 0 and -0.0
    assert worst_n <= BOUND[(form, dt)] and worst_d <= BOUND[(form, dt)]
    assert np.all(got_far == 0), got_far
    if dt == "f32":
        assert np.array_equal(got, run(be, "exp_neg" if form == "exp_neg_table" else "exp_neg_table", x))      # one fp32 form


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_fast_rcp(dt, hip_f64, hip_f32):
    """the solver's domain [1e-5, 1e3] (the comment excludes 0, inf and denormals): log-uniform draws, powers of two and their neighbours"""
    be, F = _be(dt, hip_f64, hip_f32)
    rng = np.random.default_rng(12)
    p2 = (2.0**np.arange(-16, 10)).astype(F)
    x = np.concatenate([np.array([1e-5, 1e3, 1.0, 3.0, 1 / 3], dtype=F), p2, np.nextafter(p2, F(0)), np.nextafter(p2, F(np.inf)),
                        (10.0**rng.uniform(-5, 3, 100000)).astype(F)])
    x = x[(x >= F(1e-5)) & (x <= F(1e3))]
    got = run(be, "fast_rcp", x)
    e = ulps(got, L(1) / x.astype(L), F)
    print(f"MATH fast_rcp {dt} n={x.size}: {e.max():.3f} ulp (at x = {x[e.argmax()]!r}), bound {BOUND['fast_rcp']}")
    assert e.max() <= BOUND["fast_rcp"]


def sqrt_arguments(F, rng):
    sq = (np.arange(1, 5, dtype=np.float64)**2).astype(F)
    return np.concatenate([np.array([1e-12, 16.0, 1.0, 2.0, 0.5], dtype=F), sq, np.nextafter(sq, F(0)), np.nextafter(sq, F(np.inf)),
                           (10.0**rng.uniform(-12, np.log10(16.0), 70000)).astype(F), rng.uniform(1e-12, 16.0, 30000).astype(F)])


@pytest.mark.parametrize("primitive", ["sqrt_pos", "sqrt_nonneg"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_sqrt(dt, primitive, hip_f64, hip_f32):
    """[1e-12, 16], the range of k^2 and of products of Planck fractions; sqrt_nonneg also at 0 (an exact 0), at the smallest normal and
    at a denormal (finite)"""
    be, F = _be(dt, hip_f64, hip_f32)
    x = sqrt_arguments(F, np.random.default_rng(13))
    got = run(be, primitive, x)
    e = ulps(got, np.sqrt(x.astype(L)), F)
    print(f"MATH {primitive} {dt} n={x.size}: {e.max():.3f} ulp (at x = {x[e.argmax()]!r}), bound {BOUND[primitive]}")
    assert e.max() <= BOUND[primitive]
    if primitive == "sqrt_nonneg":
        assert np.array_equal(got, run(be, "sqrt_pos", x))                               # a normal argument gives sqrt_pos's bits
        fi = np.finfo(F)
        edge = np.array([0.0, fi.tiny, fi.smallest_subnormal * 1000], dtype=F)
        g = run(be, "sqrt_nonneg", edge)
        e_tiny = float(ulps(g[1:2], np.sqrt(edge[1:2].astype(L)), F)[0])
        print(f"MATH sqrt_nonneg {dt} edges: sqrt(0) = {g[0]!r}, the smallest normal {e_tiny:.3f} ulp, a denormal -> {g[2]!r}")
        assert g[0] == 0 and not np.signbit(g[0])
        assert e_tiny <= BOUND[primitive]
        assert np.isfinite(g[2]) and g[2] >= 0


def test_bad_arguments_are_refused(hip_f64):
    be = hip_f64
    x = be.asarray(np.array([-1.0, -2.0]))
    y = be.empty((2,)).fill_(-7.0)
    with pytest.raises(ValueError):
        be.math_selftest("exp", x)
    for which, n, a, b in ((5, 2, x, y), (-1, 2, x, y), (0, -1, x, y), (0, 2, None, y), (0, 2, x, None)):
        with pytest.raises(RuntimeError, match="rrx_math_selftest"):
            be._c("math_selftest", which, n, a, b)
    be._c("math_selftest", 0, 0, None, None)                   # nothing to do
    assert bool((y == -7.0).all())
