"""GPU tests of every LW no-scattering entry against longdouble truth (tests/lw_ref.py), regime by regime.

Every other comparison of these entries (rrx_lw_solver_noscat, _fractions, _fractions_jac, _fractions_byband, _fractions_angles,
_fractions_optimal) is with the CPU oracle or between two of them, in the same precision and in cases.rel_err's norm (error over the
array's largest value; 1e-10 fp64, 3e-5 fp32), which hides every optically thin contribution. Here each (g-point, column) profile is
compared with a solve in np.longdouble that evaluates the source factor exactly, and falls into one regime (lw_ref.GPOINT_REGIMES: tau D
of every layer below the switch tau_thres = eps^(1/4) with dark or lit levels, across it, just above it, moderate, opaque up to the
underflow of exp, cases.tall_inputs' optical depths with layers of tau = 0, the same with hot layers). Norm: lw_ref.profile_error, per
quantity (flux_up, flux_dn, flux_up_jac separately) the largest error over the levels over the profile's largest truth value, in
units of the dtype's eps.

Bound. Per regime and quantity, kernel <= 8 x max(E_regime, 32 eps) (lw_ref.bound_eps). E_regime is the CPU oracle's own worst error
against the same truth in the same regime, shape, orientation, dtype, angle set and quantity, computed here from the oracle's
per-g-point fluxes; for the summed forms (broadband, by band) those are added in g-point order in the run's dtype first, the truth in
longdouble, and a column takes the regime of lw_ref.column_regimes. Margin and floor are those of tests/test_gpu_sw_truth.py, for its
reasons: exp_neg is documented at <= 1.3 ulp against libm's 1, fast_rcp replaces the division, the scans re-associate the recurrences.
Nothing in a bound comes from a kernel. The optimal-angle secants are formed in longdouble and rounded to the run's dtype, so that
truth, oracle and kernel solve with the same D; what the entry returns through secants_out is compared with that rounding separately,
within (nlay + 8) eps as in tests/test_gpu_lw_optimal_angles.py.

Inputs: lw_ref.inputs, ten g-points in four uneven bands, one regime each; sfc_emis == 1 in every third column; no incident flux in three
g-points. Shapes: lw_ref.SHAPES, the smallest that reach each tiling of lw_fused_broadband, launch_scan and the serial kernel; both
orientations on the two smallest of each dtype. Every fused form runs with the automatic g-point split (two ranges at these sizes) and
once more in one range. tests/test_lw_ref.py holds the truth to closed forms, asserts the conditions on the inputs, records the
oracle's per-regime table (CPU) and shows with a numpy model in place of a kernel that this bound rejects exp off by 2^-40 / 2^-18 and a
series one term short.

Measured on an MI355X (this file's prints), worst over the shapes, orientations, quantities, angle sets and both g-point splits; "oracle"
is the oracle's error on the profile set where the kernel's is largest, "ratio" the largest kernel / oracle among the lines where the
kernel is beyond the 32-eps floor. The kernel figures were measured on the GPU; the oracle's (E_regime, and the table of
tests/test_lw_ref.py) and the numpy model's on a CPU.
  per g-point (rrx_lw_solver_noscat)
    regime       fp64 kernel   oracle    ratio     fp32 kernel   oracle   ratio
    opaque       1.2 eps       0.80      -         1.3 eps       1.3      -
    moderate     6.6           2.9       -         5.2           4.3      -
    thin_dark    4.2e2         4.2e2     1.01      5.8           6.2      -
    plain        3.7e3         3.7e3     1.00      44            43       1.02
    thin         1.3e4         1.3e4     1.00      1.6e2         88       3.64
    hot_layer    1.4e4         1.4e4     1.00      1.5e2         1.6e2    1.03
    just_thick   4.7e5         4.7e5     1.00      44            45       1.09
    seam         6.6e6         6.6e6     1.00      3.4e2         3.4e2    1.44
  sums of the fused forms and of the general route (fractions, _jac, _byband, _angles, _optimal, do_broadband on sources; fp32 variant 15)
    all g-points (seam)      3.5e3 eps (oracle 3.5e3, ratio 1.06)        17 eps (oracle 18)
    band 1 (thin_dark)       4.0e2 (4.0e2, 1.00)                         5.4 (5.5)
    bands 2, 3 (seam)        1.9e5 (1.9e5, 1.00)                         1.1e2 (1.1e2, 1.30)
    band 4 (hot_layer)       3.4e3 (3.4e3, 1.02)                         22 (22)
  The largest share of a bound that any kernel figure takes is 0.13 in fp64 (i.e. the oracle's own error: 1/8) and 0.42 in fp32 (thin,
  per g-point, three angles at (12, 15): flux_dn 106 eps where the oracle has 29, under the floor). No profile is outside the bound, so no model term was added.
  secants_out of the optimal-angle entry: at most 0.62 eps from the rounded longdouble fit (bound nlay + 8 eps).
In fp64 the kernels reproduce the oracle's error to three digits in every ill-conditioned regime: what is measured there is the
formula's cancellation on these inputs, which both evaluate alike, and the LDS-table exp_neg, fast_rcp and the re-associated scans add
nothing visible to it. Where the formula is well-conditioned (opaque, moderate) the kernels sit at 1 ... 7 eps.
"""
import numpy as np
import pytest
import types

import lw_ref
from lw_ref import CASES, IDS, NBND, NGPT, QUANTITIES, Report, as_dict

pytestmark = pytest.mark.gpu


def _be(dt, hip_f64, hip_f32):
    return hip_f64 if dt == "f64" else hip_f32


class Dev:
    """the inputs of one shape on the device"""
    def __init__(self, be, dt, shape):
        self.be, self.dt, self.shape = be, dt, shape
        I = lw_ref.inputs(dt, *shape)
        up = lambda a: be.asarray(np.array(a))                           # (a copy: the shared inputs are read-only)
        self.tau, self.lay, self.lev, self.emis, self.ssrc, self.sjac, self.inc = (up(I[k]) for k in ("tau", "lay", "lev", "emis", "ssrc", "sjac", "inc"))
        self.fr = dict(pfrac=up(I["pfrac"]), blay=up(I["blay"]), blev=up(I["blev"]), sfc_src=self.ssrc, sfc_src_jac=self.sjac)
        self.kd = types.SimpleNamespace(gpoint_bands=up(I["gb"]), band_lims_gpt=up(I["band_lims"]))
        self.fit = up(np.ascontiguousarray(I["fit"].T))                  # the C ABI's layout: (2, nbnd), first index fastest

    def angles(self, angles):
        sec, w = lw_ref.angles_of(self.dt, *self.shape, angles)
        return self.be.asarray(np.array(sec)), self.be.asarray(np.array(w))

    def numpy(self, r):
        return {k: self.be.to_numpy(v) for k, v in r.items()}


def _splits(be):
    return lw_ref.splits(be)


def _check_summed(rep, what, dt, shape, top_at_1, angles, with_inc, got, gpts=None, from_fractions=True):
    """got: dict of (nlev, ncol) sums over the g-points gpts (default: all)"""
    gpts = np.arange(NGPT) if gpts is None else gpts
    for q in got:
        assert got[q].shape == (shape[1] + 1, shape[0]), (q, got[q].shape)
    rep.check(what, got, as_dict(lw_ref.oracle(dt, *shape, top_at_1, angles, with_inc), gpts, True),
              as_dict(lw_ref.truth(dt, *shape, top_at_1, angles, with_inc, from_fractions), gpts),
              lw_ref.column_regimes(lw_ref.regimes(dt, *shape)[gpts]))


# ---- the per-g-point entry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_per_gpoint_entry(dt, shape, top_at_1, hip_f64, hip_f32, oracle_built):
    """rrx_lw_solver_noscat on sources, per-g-point fluxes: one and three angles, with and without the Jacobian, with and without
    incident flux"""
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = Report(dt)
    reg = lw_ref.regimes(dt, *shape)
    for angles in ("1", "3"):
        sec, w = d.angles(angles)
        for with_inc in (True, False):
            orc, truth = as_dict(lw_ref.oracle(dt, *shape, top_at_1, angles, with_inc)), as_dict(lw_ref.truth(dt, *shape, top_at_1, angles, with_inc, False))
            for jac in (False, True):
                r = be.lw_solver_noscat(top_at_1, sec, w, d.tau, d.lay, d.lev, d.emis, d.ssrc, inc_flux=d.inc if with_inc else None,
                                        do_jacobians=jac, sfc_src_jac=d.sjac if jac else None)
                got = d.numpy(r)
                assert set(got) == set(QUANTITIES[:3 if jac else 2])
                rep.check(f"per-g-point {shape} top_at_1={top_at_1} angles={angles} inc={with_inc} jac={jac}", got, orc, truth, reg)
    rep.done()


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_per_gpoint_entry_in_broadband_mode(dt, shape, top_at_1, hip_f64, hip_f32, oracle_built):
    """rrx_lw_solver_noscat(do_broadband) on sources: the fused LITE = false form where a tiling takes the shape, the general kernel
    and a g-point sum where none does ((9, 200) fp32)"""
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = Report(dt)
    sec, w = d.angles("1")
    for label, ctx in _splits(be):
        with ctx:
            for with_inc in (True, False):
                r = be.lw_solver_noscat(top_at_1, sec, w, d.tau, d.lay, d.lev, d.emis, d.ssrc, inc_flux=d.inc if with_inc else None, do_broadband=True)
                _check_summed(rep, f"broadband on sources {shape} top_at_1={top_at_1} inc={with_inc}, {label}", dt, shape, top_at_1, "1", with_inc,
                              d.numpy(r), from_fractions=False)
    rep.done()


# ---- the Planck-lite entries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_fractions_entry(dt, shape, top_at_1, hip_f64, hip_f32, oracle_built):
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = Report(dt)
    sec, w = d.angles("1")
    for label, ctx in _splits(be):
        with ctx:
            for with_inc in (True, False):
                r = be.lw_solver_noscat_fractions(top_at_1, d.kd, sec, w, d.tau, d.fr, d.emis, inc_flux=d.inc if with_inc else None)
                _check_summed(rep, f"fractions {shape} top_at_1={top_at_1} inc={with_inc}, {label}", dt, shape, top_at_1, "1", with_inc, d.numpy(r))
    rep.done()


@pytest.mark.parametrize("shape,top_at_1", [c[1:] for c in CASES if c[0] == "f32"], ids=[i for c, i in zip(CASES, IDS) if c[0] == "f32"])
def test_fractions_entry_fp32_one_column_per_lane(shape, top_at_1, hip_f32, oracle_built):
    """rrx_set_lw_variant(15): the one-column form ahead of the others (it declines the shapes beyond 143 layers)"""
    be, dt = hip_f32, "f32"
    d = Dev(be, dt, shape)
    rep = Report(dt)
    sec, w = d.angles("1")
    be.set_variant(lw=15)
    try:
        r = be.lw_solver_noscat_fractions(top_at_1, d.kd, sec, w, d.tau, d.fr, d.emis, inc_flux=d.inc)
        _check_summed(rep, f"fractions, variant 15 {shape} top_at_1={top_at_1}", dt, shape, top_at_1, "1", True, d.numpy(r))
    finally:
        be.set_variant(lw=0)
    rep.done()


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_fractions_jac_entry(dt, shape, top_at_1, hip_f64, hip_f32, oracle_built):
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = Report(dt)
    sec, w = d.angles("1")
    for label, ctx in _splits(be):
        with ctx:
            r = be.lw_solver_noscat_fractions_jac(top_at_1, d.kd, sec, w, d.tau, d.fr, d.emis, inc_flux=d.inc)
            got = d.numpy(r)
            assert set(got) == set(QUANTITIES)
            _check_summed(rep, f"fractions_jac {shape} top_at_1={top_at_1}, {label}", dt, shape, top_at_1, "1", True, got)
    rep.done()


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_fractions_byband_entry(dt, shape, top_at_1, hip_f64, hip_f32, oracle_built):
    """each band's sums against the truth of its g-points (band 1 is thin_dark alone), and the broadband arrays"""
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = Report(dt)
    sec, w = d.angles("1")
    for label, ctx in _splits(be):
        with ctx:
            got = d.numpy(be.lw_solver_noscat_fractions_byband(top_at_1, d.kd, sec, w, d.tau, d.fr, d.emis, inc_flux=d.inc))
            what = f"by band {shape} top_at_1={top_at_1}, {label}"
            assert got["bnd_flux_up"].shape == (NBND, shape[1] + 1, shape[0])
            for ib in range(NBND):
                _check_summed(rep, f"{what}, band {ib + 1}", dt, shape, top_at_1, "1", True,
                              dict(flux_up=got["bnd_flux_up"][ib], flux_dn=got["bnd_flux_dn"][ib]), lw_ref.band_gpoints(ib))
            _check_summed(rep, f"{what}, broadband", dt, shape, top_at_1, "1", True, dict(flux_up=got["flux_up"], flux_dn=got["flux_dn"]))
            assert np.array_equal(got["bnd_flux_net"], got["bnd_flux_dn"] - got["bnd_flux_up"])
    rep.done()


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_fractions_angles_entry(dt, shape, top_at_1, hip_f64, hip_f32, oracle_built):
    """three angles whose secants differ by g-point and column, fluxes and Jacobian"""
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = Report(dt)
    sec, w = d.angles("3")
    for label, ctx in _splits(be):
        with ctx:
            r = be.lw_solver_noscat_fractions_angles(top_at_1, d.kd, sec, w, d.tau, d.fr, d.emis, inc_flux=d.inc, jacobian=True)
            _check_summed(rep, f"fractions_angles {shape} top_at_1={top_at_1}, {label}", dt, shape, top_at_1, "3", True, d.numpy(r))
    rep.done()


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_fractions_optimal_entry(dt, shape, top_at_1, hip_f64, hip_f32, oracle_built):
    """the secants formed in the kernel: secants_out against the longdouble fit rounded to the run's dtype within (nlay + 8) eps, the
    fluxes and the Jacobian against the truth solved with that rounding"""
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = Report(dt)
    _, w = d.angles("opt")
    want_sec = lw_ref.angles_of(dt, *shape, "opt")[0][0].astype(np.float64)
    sec_bound = (shape[1] + 8) * rep.eps
    failures = []
    for label, ctx in _splits(be):
        with ctx:
            r = be.lw_solver_noscat_fractions_optimal(top_at_1, d.kd, w, d.tau, d.fr, d.emis, fit=d.fit, inc_flux=d.inc, jacobian=True, keep_secants=True)
            got = d.numpy(r)
            e_sec = float(np.max(np.abs(got.pop("secants").astype(np.float64) - want_sec) / want_sec))
            print(f"LWTRUTH fractions_optimal {shape} top_at_1={top_at_1}, {label} secants {dt}: kernel {e_sec / rep.eps:.4g} eps, bound {sec_bound / rep.eps:.4g} eps")
            if not e_sec <= sec_bound:
                failures.append(f"secants_out, {label}: {e_sec / rep.eps:.4g} eps > {sec_bound / rep.eps:.4g} eps")
            _check_summed(rep, f"fractions_optimal {shape} top_at_1={top_at_1}, {label}", dt, shape, top_at_1, "opt", True, got)
    assert not failures, "\n".join(failures)
    rep.done()
