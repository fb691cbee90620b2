"""GPU tests of the kernels between gas optics and the solvers, one entry point of include/rrx_hip.h at a time (csrc/rrx_misc.hip):
cloud optics in its three forms, aerosol optics, the full g-point increments, delta scaling, the broadband sum and net, col_dry and
the TOA source kernels.

Every reference is plain numpy (tests/optics_ref.py, itself checked by tests/test_optics_ref.py against the goldens of the
reference's CPU classes and by hand). Whatever only moves data, adds, subtracts or multiplies once is compared bit for bit, and so
is every edge whose result is exact. The rest is bounded from the reference alone: with e_ref the largest relative error of the
working-precision evaluation (the kernel's expressions in the arrays' dtype, every operation rounded once) against the np.longdouble
truth over the case, every kernel element lies within (2*e_ref + 2*eps)*|truth|, elements whose truth is 0 are exactly 0, and
e_ref <= 16 eps is asserted so that the bound cannot hide anything (optics_ref.kernel_bound has the reasons for the 2 and the 2).
Each tolerance test prints the kernel's worst error beside e_ref (profiles/optics_kernels_errors.txt keeps a run's lines).

Shapes: the element-wise kernels and the cloud and aerosol kernels run on a 1-D grid of 256 threads and at most 4 096 workgroups:
1, 255 and 257 elements (cells), a mixed shape (3, 7, 45) and one case just above 1 048 576, where the grid-stride loop takes its
second turn; the TOA kernels on at most 64 workgroups x ngpt: 1, 255, 257 and 16 385 columns. Every output and every array updated
in place carries a guard tail that must come back untouched, and an empty problem is followed by a valid call that must be right."""
import ctypes

import numpy as np
import pytest

import cases
import optics_ref as ref
from gpu_helpers import GUARD, be, dev, guarded, guarded_copy, same_bits, tail_untouched      # noqa: F401 (be: a fixture)
from rte_rrtmgp_cpp_amd import synthetic

pytestmark = pytest.mark.gpu

LD = np.longdouble
BIG = 1048577                                                          # one more than the grid's 4 096 x 256 threads
SHAPES = [(1, 1, 1), (1, 1, 255), (1, 1, 257), (3, 7, 45), (1, 1, BIG)]                # (ngpt or nbnd, nlay, ncol)
SHAPE_IDS = ["1", "255", "257", "3x7x45", "1048577"]


def check_bound(capsys, be, what, names, got, work, truth, scales=None):
    """the module's bound, output by output; got: kernel arrays (numpy), work / truth: the two evaluations of optics_ref"""
    lines, failures = [], []
    for name, k, w, t in zip(names, got, work, truth):
        scale = None if scales is None else scales.get(name)
        e_ref, ref_zeros = ref.rel_errors(np.asarray(w, dtype=k.dtype), t, scale)
        e_k, zeros_exact = ref.rel_errors(k, t, scale)
        lines.append(f"  optics-error {be.sfx[1:]} {what} {name}: kernel {e_k:.2f} eps, e_ref {e_ref:.2f} eps")
        if not (ref_zeros and e_ref <= ref.E_REF_CAP):
            failures.append(f"{name}: the reference itself is outside the cap: e_ref {e_ref:.2f} eps")
        if not zeros_exact:
            failures.append(f"{name}: an element whose truth is 0 is not exactly 0")
        if not e_k <= ref.kernel_bound(e_ref):
            failures.append(f"{name}: kernel {e_k:.2f} eps > 2*{e_ref:.2f} + 2")
    with capsys.disabled():
        print("\n" + "\n".join(lines), end="")
    assert not failures, (what, failures)


def within_bound(got, work, truth):
    """the module's bound for one output, for the valid calls that follow refused and empty ones"""
    e_ref, _ = ref.rel_errors(np.asarray(work, dtype=got.dtype), truth)
    e_k, zeros_exact = ref.rel_errors(got, truth)
    return zeros_exact and e_ref <= ref.E_REF_CAP and e_k <= ref.kernel_bound(e_ref)


def inplace(be, arrays):
    """guarded device copies of numpy arrays: ([buf...], [tensor...])"""
    pairs = [guarded_copy(be, a) for a in arrays]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def tails_untouched(bufs, outs):
    return all(tail_untouched(b, o) for b, o in zip(bufs, outs))


# ==== increments and delta scaling ================================================================================================
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_increment_1scalar(shape, be):
    rng = np.random.default_rng(shape[2])
    t1, t2 = (rng.uniform(-9., 9., shape).astype(be.np_dtype) for _ in range(2))
    ngpt, nlay, ncol = shape
    buf, tau = guarded_copy(be, t1)
    be._c("increment_1scalar_by_1scalar", ncol, nlay, ngpt, tau, dev(be, t2))
    assert same_bits(tau.cpu().numpy(), ref.increment_1scalar(t1, t2))
    assert tail_untouched(buf, tau)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_increment_2stream(shape, be, capsys):
    """tau bit for bit (one addition); ssa and g within the module's bound on tau = 10**U(-4, 1.5), ssa in [0, 1], g in [0, 0.9]"""
    rng = np.random.default_rng(10 + shape[2])
    a = ref.two_stream_inputs(shape, rng, be.np_dtype) + ref.two_stream_inputs(shape, rng, be.np_dtype)
    ngpt, nlay, ncol = shape
    bufs, (T, W, G) = inplace(be, a[:3])
    be._c("increment_2stream_by_2stream", ncol, nlay, ngpt, T, W, G, *(dev(be, x) for x in a[3:]))
    got = [x.cpu().numpy() for x in (T, W, G)]
    work, truth = ref.increment_2stream(*a, be.np_dtype.type), ref.increment_2stream(*a, LD)
    assert same_bits(got[0], work[0])
    check_bound(capsys, be, f"increment_2stream {shape}", ("tau", "ssa", "g"), got, work, truth)
    assert tails_untouched(bufs, (T, W, G))


def test_increment_2stream_exact_edges(be):
    """Both tau 0: tau = ssa = g = 0. Both ssa 0: g = 0 (and ssa = 0). tau2 = 0: tau unchanged (and with equal ssa, g the pair is
    unchanged where the arithmetic is exact). Denormal tau below the floor 3*tiny: the quotients are taken by the floor, not by the
    tau -- the working-precision restatement gives the bits."""
    dt = be.np_dtype
    tiny = np.finfo(dt).tiny
    a = lambda *v: np.array(v, dtype=dt)
    den = dt.type(tiny)/dt.type(4.)                                    # a denormal
    t1 = a(0., 2., 2., tiny, den, 0.);       w1 = a(.5, 0., .5, 1., .5, .75);  g1 = a(.5, .5, .5, .5, .5, .25)
    t2 = a(0., 1., 0., tiny, den, den);      w2 = a(.5, 0., .5, 1., .5, .5);   g2 = a(.5, .5, .5, .5, .25, .5)
    bufs, (T, W, G) = inplace(be, (t1, w1, g1))
    be._c("increment_2stream_by_2stream", 6, 1, 1, T, W, G, dev(be, t2), dev(be, w2), dev(be, g2))
    got = [x.cpu().numpy() for x in (T, W, G)]
    for k, w in zip(got, ref.increment_2stream(t1, w1, g1, t2, w2, g2, dt.type)):
        assert same_bits(k, w)
    assert got[0][:3].tolist() == [0., 3., 2.] and got[1][:3].tolist() == [0., 0., .5] and got[2][:3].tolist() == [0., 0., .5]
    # by the floor: (2 tiny)/(3 tiny), (tiny/4)/(3 tiny) and (tiny/8)/(3 tiny); by the tau they would be 1, 1/2 and 1/2
    assert np.allclose(got[1][3:].astype(np.float64), [2/3, 1/12, 1/24], rtol=1e-6, atol=0.)
    assert tails_untouched(bufs, (T, W, G))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_delta_scale(shape, be, capsys):
    rng = np.random.default_rng(20 + shape[2])
    a = ref.two_stream_inputs(shape, rng, be.np_dtype)
    ngpt, nlay, ncol = shape
    bufs, (T, W, G) = inplace(be, a)
    be._c("delta_scale_2str_k", ncol, nlay, ngpt, T, W, G)
    got = [x.cpu().numpy() for x in (T, W, G)]
    check_bound(capsys, be, f"delta_scale {shape}", ("tau", "ssa", "g"), got, ref.delta_scale(*a, be.np_dtype.type), ref.delta_scale(*a, LD))
    assert tails_untouched(bufs, (T, W, G))


def test_delta_scale_exact_edges(be):
    """g = 0: the identity on all three arrays. g = 1: g' = 0. g = 1, ssa = 1: tau' = 0 and ssa' = 0. ssa = 0: tau unchanged and
    ssa' = 0."""
    dt = be.np_dtype
    a = lambda *v: np.array(v, dtype=dt)
    t, w, g = a(2.3, 1e-4, 2., 2., 31.7), a(.7, 1., .5, 1., 0.), a(0., 0., 1., 1., .6)
    bufs, (T, W, G) = inplace(be, (t, w, g))
    be._c("delta_scale_2str_k", 5, 1, 1, T, W, G)
    T, W, G = (x.cpu().numpy() for x in (T, W, G))
    assert same_bits(T[:2], t[:2]) and same_bits(W[:2], w[:2]) and same_bits(G[:2], g[:2])
    assert same_bits(G[2:4], a(0., 0.)) and same_bits(T[3:4], a(0.)) and same_bits(W[3:4], a(0.))
    assert same_bits(T[4:], t[4:]) and same_bits(W[4:], a(0.))
    for k, r in zip((T, W, G), ref.delta_scale(t, w, g, dt.type)):
        assert same_bits(k, r)


# ==== broadband sum and net, col_dry ==============================================================================================
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 1, 255), (3, 1, 257), (3, 7, 45), (2, 1, BIG)], ids=SHAPE_IDS)
def test_sum_broadband_and_net(shape, be):
    """sums in ascending g-point order from +0.0, bit for bit: column 0 is -0.0 at every g-point and sums to +0.0 (sum_byband gives
    -0.0 there); the net is one subtraction"""
    rng = np.random.default_rng(30 + shape[2])
    ngpt, nlev, ncol = shape
    gpt = rng.uniform(-9., 9., shape).astype(be.np_dtype)
    gpt[:, :, 0] = -0.0
    buf, out = guarded(be, (nlev, ncol))
    be._c("sum_broadband", ncol, nlev, ngpt, dev(be, gpt), out)
    got = out.cpu().numpy()
    assert same_bits(got, ref.sum_broadband(gpt))
    assert not np.signbit(got[:, 0]).any() and tail_untouched(buf, out)
    dn, up = gpt[0], rng.uniform(-9., 9., (nlev, ncol)).astype(be.np_dtype)
    buf, out = guarded(be, (nlev, ncol))
    be._c("net_broadband_precalc", ncol, nlev, dev(be, dn), dev(be, up), out)
    assert same_bits(out.cpu().numpy(), ref.net_broadband(dn, up)) and tail_untouched(buf, out)


@pytest.mark.parametrize("nlay,ncol,top_at_1", [(nl, nc, top) for nl, nc in ((1, 1), (1, 255), (1, 257), (7, 45)) for top in (False, True)]
                         + [(1, BIG, False)])                          # (one large case per kernel)
def test_col_dry(nlay, ncol, top_at_1, be, capsys):
    h, plev = ref.col_dry_inputs(nlay, ncol, top_at_1, np.random.default_rng(40 + ncol), be.np_dtype)
    buf, out = guarded(be, (nlay, ncol))
    be._c("get_col_dry", ncol, nlay, dev(be, h), dev(be, plev), out)
    check_bound(capsys, be, f"col_dry ({nlay}, {ncol}) top_at_1={top_at_1}", ("col_dry",), [out.cpu().numpy()],
                [ref.col_dry(h, plev, be.np_dtype.type)], [ref.col_dry(h, plev, LD)])
    assert tail_untouched(buf, out)


# ==== TOA source ==================================================================================================================
@pytest.mark.parametrize("ngpt", [1, 3])
@pytest.mark.parametrize("ncol", [1, 255, 257, 16385])                 # 16 385: one more than the grid's 64 x 256 columns
def test_toa_source_kernels(ncol, ngpt, be):
    """bit for bit: spread_col copies, scaling_to_subset and toa_source multiply once; toa_source without a scaling is spread_col"""
    rng = np.random.default_rng(50 + ncol + ngpt)
    src = rng.uniform(.1, 9., ngpt).astype(be.np_dtype)
    fac = rng.uniform(.9, 1.1, ncol).astype(be.np_dtype)
    buf, out = guarded(be, (ngpt, ncol))
    be._c("spread_col", ncol, ngpt, out, dev(be, src))
    spread = out.cpu().numpy()
    assert same_bits(spread, ref.spread_col(src, ncol)) and tail_untouched(buf, out)
    be._c("scaling_to_subset", ncol, ngpt, out, dev(be, fac))
    scaled = out.cpu().numpy()
    assert same_bits(scaled, ref.scaling_to_subset(spread, fac)) and tail_untouched(buf, out)
    buf, out = guarded(be, (ngpt, ncol))
    be._c("toa_source", ncol, ngpt, out, dev(be, src), dev(be, fac))
    assert same_bits(out.cpu().numpy(), ref.toa_source(src, fac, ncol)) and same_bits(out.cpu().numpy(), scaled)
    assert tail_untouched(buf, out)
    buf, out = guarded(be, (ngpt, ncol))
    be._c("toa_source", ncol, ngpt, out, dev(be, src), None)
    assert same_bits(out.cpu().numpy(), spread) and tail_untouched(buf, out)


# ==== cloud optics ================================================================================================================
def cloud_call(be, entry, lut, ldev, nbnd, arrays, nout):
    """rrx_cloud_optics_<entry> on device arrays (clwp, ciwp, reliq, deice) into guarded outputs: ([buf...], [out...])"""
    nlay, ncol = arrays[0].shape
    pairs = [guarded(be, (nbnd, nlay, ncol)) for _ in range(nout)]
    be._c("cloud_optics_" + entry, ncol, nlay, nbnd, lut["nsize_liq"], lut["nsize_ice"],
          lut["radliq_lwr"], lut["radliq_upr"], lut["diamice_lwr"], lut["diamice_upr"],
          *(ldev[k] for k in ("lut_extliq", "lut_ssaliq", "lut_asyliq", "lut_extice", "lut_ssaice", "lut_asyice")),
          *arrays, *(p[1] for p in pairs))
    return [p[0] for p in pairs], [p[1] for p in pairs]


def cloud_three_forms(be, lut, nbnd, arrays_np):
    """the three entries on one set of inputs: (2str triple, 1scl tau, delta triple) as numpy; guard tails checked; the one-pass delta
    form must be the two-pass form (2str, then delta_scale_2str_k in place) bit for bit"""
    ldev = be.upload_lut({k: (np.asarray(v).astype(be.np_dtype) if isinstance(v, np.ndarray) else v) for k, v in lut.items()})
    arrays = [dev(be, a) for a in arrays_np]
    nlay, ncol = arrays_np[0].shape
    b2, two = cloud_call(be, "2str", lut, ldev, nbnd, arrays, 3)
    b1, one = cloud_call(be, "1scl", lut, ldev, nbnd, arrays, 1)
    bd, delta = cloud_call(be, "2str_delta", lut, ldev, nbnd, arrays, 3)
    out = [x.cpu().numpy() for x in two], one[0].cpu().numpy(), [x.cpu().numpy() for x in delta]
    assert tails_untouched(b2, two) and tails_untouched(b1, one) and tails_untouched(bd, delta)
    be._c("delta_scale_2str_k", ncol, nlay, nbnd, *two)
    for a, b in zip(two, out[2]):
        assert same_bits(a.cpu().numpy(), b)
    assert tails_untouched(b2, two)
    return out


@pytest.mark.parametrize("shape,kind", [(s, k) for s in SHAPES[:4] for k in ("lw", "sw")] + [((2, 1, BIG), "lw")])       # (one large case)
def test_cloud_optics(shape, kind, be, capsys):
    """All three forms within the module's bound; rrx_cloud_optics_2str_delta against rrx_cloud_optics_2str followed by
    rrx_delta_scale_2str_k bit for bit. Sizes uniform over the table and (from 255 cells on) every node of both phases, both ends,
    0.5 and 2.5 steps below and above the table; water paths 10**U(-3, 2.5), about 30 % of the cells cloud-free per phase.

    The 1-scalar tau (tau_l - tau_l*ssa_l) + (tau_i - tau_i*ssa_i) on the SW table is a difference of nearly equal terms (ssa about
    0.97): relative to the result the working-precision evaluation itself is 57 to 60 epsilons from the truth, far above the cap that
    keeps the bound honest, so there its error is measured relative to the extinction tau_l + tau_i, which the rounding errors of the
    two terms scale with; on the LW table (ssa about 0.5) relative to the result as everywhere else."""
    nbnd, nlay, ncol = shape
    lut = synthetic.make_cloud_lut(nbnd, kind)
    arrays = ref.cloud_inputs(lut, nlay, ncol, np.random.default_rng(60 + ncol), be.np_dtype)
    two, one, delta = cloud_three_forms(be, lut, nbnd, arrays)
    w2, w1, wd = ref.cloud_optics(lut, *arrays, be.np_dtype.type)
    t2, t1, td = ref.cloud_optics(lut, *arrays, LD)
    names = ("tau", "ssa", "g", "tau_1scl", "tau_delta", "ssa_delta", "g_delta")
    check_bound(capsys, be, f"cloud {kind} {(nbnd, nlay, ncol)}", names, two + [one] + delta, w2 + (w1,) + wd, t2 + (t1,) + td,
                scales={"tau_1scl": t2[0]} if kind == "sw" else None)


def test_cloud_optics_exact_edges(be):
    """optics_ref.hand_cloud_case, where every value is a short binary fraction: the node, both ends, 2.5 steps below (the clamp) and
    above the table, liquid only, ice only and both phases -- tau bit for bit against the restatement, and ssa, g wherever the
    quotient is exact. The cells with water path 0 or -1 give exact +0.0 in every output of all three forms, whatever their sizes
    hold (NaN, -1e30)."""
    dt = be.np_dtype
    lut, *arrays = ref.hand_cloud_case(dt)
    two, one, delta = cloud_three_forms(be, lut, 1, arrays)
    w2, w1, wd = ref.cloud_optics(lut, *arrays, dt.type)
    assert same_bits(two[0], w2[0]) and same_bits(one, w1)
    assert two[0][0, 0].tolist() == [4., 8., 3., 18., .5, 0., .5, 4.5]
    assert two[1][0, 0, :7].tolist() == [.25, .5, .75, 1.125, 2., 0., .5] and two[2][0, 0].tolist() == [.5, .5, .25, .5, -.375, 0., .5, .5]
    assert abs(float(two[1][0, 0, 7]) - 1.25/4.5) <= 2*np.finfo(dt).eps
    zero = np.zeros(1, dtype=dt)
    for a in two + [one] + delta:
        assert same_bits(a[0, 0, 5:6], zero)
    # a whole field of cloud-free cells with garbage sizes, more than one workgroup
    n = 300
    clear = [np.where(np.arange(n) % 2, 0., -1.).astype(dt).reshape(1, n), np.zeros((1, n), dtype=dt),
             np.where(np.arange(n) % 3, np.nan, -1e30).astype(dt).reshape(1, n), np.full((1, n), np.nan, dtype=dt)]
    lut3 = synthetic.make_cloud_lut(3, "sw")
    two, one, delta = cloud_three_forms(be, lut3, 3, clear)
    for a in two + [one] + delta:
        assert same_bits(a, np.zeros((3, 1, n), dtype=dt))


# ==== aerosol optics ==============================================================================================================
def aerosol_call(be, lut, aermr_np, rh, plev):
    """rrx_aerosol_optics on numpy inputs into guarded outputs: (tau, ssa, g) as numpy, guard tails checked"""
    ldev = be.upload_lut(lut)
    nlay, ncol = rh.shape
    nphobic, nbnd = lut["mext_phobic"].shape
    nphilic, nhum = lut["mext_philic"].shape[:2]
    aermr = [dev(be, m) for m in aermr_np]
    ptrs = (ctypes.c_void_p * 11)(*[m.data_ptr() for m in aermr])
    per_col = (ctypes.c_int * 11)(*[1 if m.dim() == 2 else 0 for m in aermr])
    pairs = [guarded(be, (nbnd, nlay, ncol)) for _ in range(3)]
    be._c("aerosol_optics", ncol, nlay, nbnd, nhum, nphobic, nphilic, ptrs, per_col, dev(be, rh), dev(be, plev), ldev["rh_upper"],
          *(ldev[k] for k in ("mext_phobic", "ssa_phobic", "g_phobic", "mext_philic", "ssa_philic", "g_philic")), *(p[1] for p in pairs))
    assert all(tail_untouched(b, o) for b, o in pairs)
    return [o.cpu().numpy() for _, o in pairs]


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 255), (1, 1, 257), (3, 7, 45), (2, 4097, 257)], ids=SHAPE_IDS)
def test_aerosol_optics_shapes(shape, be, capsys):
    """synthetic tables, mixing ratios mixed (fields and profiles); the large case has 4 097 layers of 257 columns, so that the
    profiles' index i / ncol is exercised beyond the first turn of the grid-stride loop"""
    nbnd, nlay, ncol = shape
    lut = {k: v.astype(be.np_dtype) for k, v in synthetic.make_aerosol_lut(nbnd).items()}
    aermr, rh, plev = ref.aerosol_inputs(lut, nlay, ncol, bool(ncol % 2), "mixed", np.random.default_rng(70 + ncol), be.np_dtype)
    got = aerosol_call(be, lut, aermr, rh, plev)
    check_bound(capsys, be, f"aerosol synthetic {shape} mixed", ("tau", "ssa", "g"), got,
                ref.aerosol_optics(lut, aermr, rh, plev, be.np_dtype.type), ref.aerosol_optics(lut, aermr, rh, plev, LD))


@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
@pytest.mark.parametrize("table", ["synthetic", "real"])
def test_aerosol_optics_tables_orders_and_humidities(table, top_at_1, be, capsys, tmp_path):
    """the synthetic tables and the real CAMS ones, both column orders, mixing ratios all fields, all profiles and mixed; the humidity
    holds every class bound, 0 and 1.05 -- above the last bound, where the kernel uses the last class (the reference reads past the
    table)"""
    lut = cases.real_aerosol_lut(tmp_path) if table == "real" else synthetic.make_aerosol_lut(5)
    lut = {k: np.ascontiguousarray(v.astype(be.np_dtype)) for k, v in lut.items()}
    for kinds in ("fields", "profiles", "mixed"):
        aermr, rh, plev = ref.aerosol_inputs(lut, 7, 45, top_at_1, kinds, np.random.default_rng(80 + len(kinds)), be.np_dtype)
        assert (rh[0, :len(lut["rh_upper"])] == lut["rh_upper"]).all() and rh.max() > lut["rh_upper"][-1] and rh.min() == 0.
        got = aerosol_call(be, lut, aermr, rh, plev)
        check_bound(capsys, be, f"aerosol {table} (7, 45) top_at_1={top_at_1} {kinds}", ("tau", "ssa", "g"), got,
                    ref.aerosol_optics(lut, aermr, rh, plev, be.np_dtype.type), ref.aerosol_optics(lut, aermr, rh, plev, LD))


def test_aerosol_optics_exact_edges(be, capsys):
    """a cell with all eleven mixing ratios 0 gives tau = ssa = g = +0.0 (the others are not disturbed); tables with one humidity
    class"""
    dt = be.np_dtype
    lut = {k: v.astype(dt) for k, v in synthetic.make_aerosol_lut(3, nhum=1).items()}
    assert lut["mext_philic"].shape[1] == 1
    aermr, rh, plev = ref.aerosol_inputs(lut, 7, 45, False, "fields", np.random.default_rng(90), dt)
    for m in aermr:
        m[2, 5] = 0.; m[6, 44] = 0.
    got = aerosol_call(be, lut, aermr, rh, plev)
    for a in got:
        assert same_bits(a[:, 2, 5], np.zeros(3, dtype=dt)) and same_bits(a[:, 6, 44], np.zeros(3, dtype=dt))
    check_bound(capsys, be, "aerosol nhum=1 (7, 45)", ("tau", "ssa", "g"), got,
                ref.aerosol_optics(lut, aermr, rh, plev, dt.type), ref.aerosol_optics(lut, aermr, rh, plev, LD))


# ==== refusals and empty problems =================================================================================================
ZEROS3 = [(0, 2, 3), (5, 0, 3), (5, 2, 0), (0, 0, 0)]
NEGATIVES3 = [(-1, 2, 3), (5, -2, 3), (5, 2, -3), (-5, -2, 3), (0, 2, -3)]      # a positive product of extents; a negative beside a 0


def test_elementwise_entries_refuse_negative_extents_and_skip_empty_problems(be):
    """increment_1scalar, increment_2stream, delta_scale: an extent of 0 returns 0 and touches nothing, a negative extent is refused
    by name before any launch; a valid call straight afterwards is right"""
    dt = be.np_dtype
    shape = (3, 2, 5)
    rng = np.random.default_rng(100)
    a = ref.two_stream_inputs(shape, rng, dt) + ref.two_stream_inputs(shape, rng, dt)
    bufs, (T, W, G) = inplace(be, a[:3])
    t2, w2, g2 = (dev(be, x) for x in a[3:])
    calls = {"increment_1scalar_by_1scalar": lambda nc, nl, ng: be._c("increment_1scalar_by_1scalar", nc, nl, ng, T, t2),
             "increment_2stream_by_2stream": lambda nc, nl, ng: be._c("increment_2stream_by_2stream", nc, nl, ng, T, W, G, t2, w2, g2),
             "delta_scale_2str_k": lambda nc, nl, ng: be._c("delta_scale_2str_k", nc, nl, ng, T, W, G)}
    for name, call in calls.items():
        for ext in ZEROS3:
            assert call(*ext) == 0, (name, ext)
        for ext in NEGATIVES3:
            with pytest.raises(RuntimeError, match=f"rrx_{name}: negative extent"):
                call(*ext)
    for x, x0 in zip((T, W, G), a[:3]):
        assert same_bits(x.cpu().numpy(), x0)
    assert tails_untouched(bufs, (T, W, G))
    calls["increment_1scalar_by_1scalar"](5, 2, 3)                     # valid calls straight afterwards
    assert same_bits(T.cpu().numpy(), ref.increment_1scalar(a[0], a[3]))
    calls["delta_scale_2str_k"](5, 2, 3)
    summed = ref.increment_1scalar(a[0], a[3])
    for x, w, t in zip((T, W, G), ref.delta_scale(summed, a[1], a[2], dt.type), ref.delta_scale(summed, a[1], a[2], LD)):
        assert within_bound(x.cpu().numpy(), w, t)
    assert tails_untouched(bufs, (T, W, G))


def test_flux_and_col_dry_entries_refuse_negative_extents_and_skip_empty_problems(be):
    """sum_broadband, net_broadband_precalc, get_col_dry; sum_broadband with no g-points and a non-empty (ncol, nlev) is no empty
    problem: it writes zeros"""
    dt = be.np_dtype
    rng = np.random.default_rng(101)
    gpt = rng.uniform(-9., 9., (3, 4, 5)).astype(dt)
    h, plev = ref.col_dry_inputs(3, 5, False, rng, dt)
    src, hd, pd = dev(be, gpt), dev(be, h), dev(be, plev)
    buf, out = guarded(be, (4, 5))
    for nc, nl in ((0, 4), (5, 0), (0, 0)):
        for ng in (3, 0):
            assert be._c("sum_broadband", nc, nl, ng, src, out) == 0
        assert be._c("net_broadband_precalc", nc, nl, src, src, out) == 0
        assert be._c("get_col_dry", nc, nl, hd, pd, out) == 0
    for nc, nl, ng in ((-5, 4, 3), (5, -4, 3), (5, 4, -3), (-5, -4, 3), (0, 4, -3)):
        with pytest.raises(RuntimeError, match="rrx_sum_broadband: negative extent"):
            be._c("sum_broadband", nc, nl, ng, src, out)
    for nc, nl in ((-5, 4), (5, -4), (-5, -4)):
        with pytest.raises(RuntimeError, match="rrx_net_broadband_precalc: negative extent"):
            be._c("net_broadband_precalc", nc, nl, src, src, out)
        with pytest.raises(RuntimeError, match="rrx_get_col_dry: negative extent"):
            be._c("get_col_dry", nc, nl, hd, pd, out)
    assert (buf == GUARD).all()
    assert be._c("sum_broadband", 5, 4, 0, src, out) == 0              # no g-points: zeros
    assert same_bits(out.cpu().numpy(), np.zeros((4, 5), dtype=dt)) and tail_untouched(buf, out)
    be._c("sum_broadband", 5, 4, 3, src, out)                          # valid calls straight afterwards
    assert same_bits(out.cpu().numpy(), ref.sum_broadband(gpt)) and tail_untouched(buf, out)
    be._c("net_broadband_precalc", 5, 4, dev(be, gpt[0]), dev(be, gpt[1]), out)
    assert same_bits(out.cpu().numpy(), ref.net_broadband(gpt[0], gpt[1])) and tail_untouched(buf, out)
    buf, out = guarded(be, (3, 5))
    be._c("get_col_dry", 5, 3, hd, pd, out)
    assert within_bound(out.cpu().numpy(), ref.col_dry(h, plev, dt.type), ref.col_dry(h, plev, LD)) and tail_untouched(buf, out)


def test_toa_entries_refuse_negative_extents_and_skip_empty_problems(be):
    """spread_col and scaling_to_subset return 0 on an empty problem; toa_source keeps its refusal of one"""
    dt = be.np_dtype
    src, fac = np.array([1.5, 2.5, 3.5], dtype=dt), np.array([.5, 2., 4., 8.], dtype=dt)
    s, f = dev(be, src), dev(be, fac)
    buf, out = guarded(be, (3, 4))
    for nc, ng in ((0, 3), (4, 0), (0, 0)):
        assert be._c("spread_col", nc, ng, out, s) == 0
        assert be._c("scaling_to_subset", nc, ng, out, f) == 0
        with pytest.raises(RuntimeError, match="rrx_toa_source: empty problem"):
            be._c("toa_source", nc, ng, out, s, f)
    for nc, ng in ((-4, 3), (4, -3), (-4, -3)):
        with pytest.raises(RuntimeError, match="rrx_spread_col: negative extent"):
            be._c("spread_col", nc, ng, out, s)
        with pytest.raises(RuntimeError, match="rrx_scaling_to_subset: negative extent"):
            be._c("scaling_to_subset", nc, ng, out, f)
        with pytest.raises(RuntimeError, match="rrx_toa_source: empty problem"):
            be._c("toa_source", nc, ng, out, s, f)
    assert (buf == GUARD).all()
    be._c("spread_col", 4, 3, out, s)                                  # valid calls straight afterwards
    be._c("scaling_to_subset", 4, 3, out, f)
    assert same_bits(out.cpu().numpy(), ref.toa_source(src, fac, 4)) and tail_untouched(buf, out)
    buf, out = guarded(be, (3, 4))
    be._c("toa_source", 4, 3, out, s, f)
    assert same_bits(out.cpu().numpy(), ref.toa_source(src, fac, 4)) and tail_untouched(buf, out)


def test_cloud_entries_refuse_negative_extents_short_tables_and_skip_empty_problems(be):
    """ncol, nlay or nbnd = 0: returns 0, nothing touched; a negative extent and a size table of one entry (no interval; the step
    would divide by zero) are refused by name before any launch"""
    dt = be.np_dtype
    nbnd, nlay, ncol = 3, 2, 5
    lut = synthetic.make_cloud_lut(nbnd, "lw")
    ldev = be.upload_lut({k: (v.astype(dt) if isinstance(v, np.ndarray) else v) for k, v in lut.items()})
    arrays_np = ref.cloud_inputs(lut, nlay, ncol, np.random.default_rng(102), dt)
    arrays = [dev(be, a) for a in arrays_np]
    pairs = [guarded(be, (nbnd, nlay, ncol)) for _ in range(3)]
    outs = [p[1] for p in pairs]
    tabs = [ldev[k] for k in ("lut_extliq", "lut_ssaliq", "lut_asyliq", "lut_extice", "lut_ssaice", "lut_asyice")]

    def call(entry, nc, nl, nb, nsl=lut["nsize_liq"], nsi=lut["nsize_ice"]):
        return be._c("cloud_optics_" + entry, nc, nl, nb, nsl, nsi, lut["radliq_lwr"], lut["radliq_upr"], lut["diamice_lwr"],
                     lut["diamice_upr"], *tabs, *arrays, *(outs[:1] if entry == "1scl" else outs))
    for entry in ("2str", "2str_delta", "1scl"):
        for ext in ZEROS3:
            assert call(entry, *ext) == 0, (entry, ext)
        for ext in NEGATIVES3:
            with pytest.raises(RuntimeError, match=f"rrx_cloud_optics_{entry}: negative extent"):
                call(entry, *ext)
        for nsl, nsi in ((1, lut["nsize_ice"]), (lut["nsize_liq"], 1), (0, 0), (lut["nsize_liq"], -3)):
            with pytest.raises(RuntimeError, match=f"rrx_cloud_optics_{entry}: cloud size tables need at least 2 entries"):
                call(entry, ncol, nlay, nbnd, nsl, nsi)
    assert all(bool((b == GUARD).all().item()) for b, _ in pairs)
    call("2str", ncol, nlay, nbnd)                                     # a valid call straight afterwards
    for (b, o), w, t in zip(pairs, ref.cloud_optics(lut, *arrays_np, dt.type)[0], ref.cloud_optics(lut, *arrays_np, LD)[0]):
        assert within_bound(o.cpu().numpy(), w, t) and tail_untouched(b, o)


def test_aerosol_entry_refuses_negative_extents_and_skips_empty_problems(be):
    dt = be.np_dtype
    nbnd, nlay, ncol = 3, 2, 5
    lut = {k: v.astype(dt) for k, v in synthetic.make_aerosol_lut(nbnd).items()}
    ldev = be.upload_lut(lut)
    aermr_np, rh, plev = ref.aerosol_inputs(lut, nlay, ncol, False, "mixed", np.random.default_rng(103), dt)
    aermr = [dev(be, m) for m in aermr_np]
    ptrs = (ctypes.c_void_p * 11)(*[m.data_ptr() for m in aermr])
    per_col = (ctypes.c_int * 11)(*[1 if m.dim() == 2 else 0 for m in aermr])
    pairs = [guarded(be, (nbnd, nlay, ncol)) for _ in range(3)]
    rhd, pd = dev(be, rh), dev(be, plev)
    tabs = [ldev[k] for k in ("mext_phobic", "ssa_phobic", "g_phobic", "mext_philic", "ssa_philic", "g_philic")]

    def call(nc, nl, nb):
        return be._c("aerosol_optics", nc, nl, nb, 12, 14, 7, ptrs, per_col, rhd, pd, ldev["rh_upper"], *tabs, *(p[1] for p in pairs))
    for ext in ZEROS3:
        assert call(*ext) == 0, ext
    for ext in NEGATIVES3:
        with pytest.raises(RuntimeError, match="rrx_aerosol_optics: negative extent"):
            call(*ext)
    assert all(bool((b == GUARD).all().item()) for b, _ in pairs)
    call(ncol, nlay, nbnd)                                             # a valid call straight afterwards
    for (b, o), w, t in zip(pairs, ref.aerosol_optics(lut, aermr_np, rh, plev, dt.type), ref.aerosol_optics(lut, aermr_np, rh, plev, LD)):
        assert within_bound(o.cpu().numpy(), w, t) and tail_untouched(b, o)
