"""GPU tests of the two rescaled LW entries (rrx_lw_solver_noscat_rescaled, rrx_lw_solver_noscat_fractions_rescaled;
csrc/rrx_solver_lw1r.hip) against the longdouble truth of tests/lw1r_truth.py, regime by regime.

Every other comparison of these entries (tests/test_gpu_lw_rescaled.py) is with tests/lw1r_ref.py in the same precision and in
cases.rel_err's norm, which hides every optically thin contribution; its fp32 per-g-point tolerance, 3.8e-4, is the reference's own
cancellation just above the source factor's switch. Here each (g-point, column) profile is compared with a solve in np.longdouble that
evaluates the source factor exactly (lw_ref.source_factor) and falls into one regime (lw1r_truth.GPOINT_REGIMES: an interval of tau D st
that holds for every secant of the tests, and a scattering class). Norm: lw_ref.profile_error per quantity (flux_up, flux_dn,
flux_up_jac), in eps of the dtype.

Bound. Per regime and quantity, kernel <= 8 x max(E_regime, 32 eps) (lw_ref.bound_eps; margin and floor are lw_ref's, for its reasons).
E_regime is the worst error against the same truth of lw1r_truth.solve_model, which is tests/lw1r_ref.solve (asserted bit for bit on the
CPU), in the same regime, shape, orientation, dtype, angle set, entry and quantity. For the sums the model is added in g-point order in
the run's dtype, the truth in longdouble, and a column takes the regime of lw1r_truth.column_regimes. Nothing in a bound comes from a
kernel; seed, ranges and lists are chosen in lw1r_truth.py from the inputs and the model alone. All outputs must be finite. No cell is
unresolved: the largest bound is 1.0e-8 of a flux in fp64 and 5.7e-4 in fp32 (tests/test_lw1r_truth.py, from the model alone).

Inputs: lw1r_truth.inputs, 15 g-points in ten uneven bands, one regime per band; sfc_emis == 1 in every third column; four g-points
without incident flux. Shapes: lw1r_truth.SHAPES, the smallest layer counts that reach each tiling of lw1r_fused (written beside the
list) and 600 layers, which no tiling takes; both orientations on the two smallest of each dtype. The general entry runs per g-point with
one and with three angles (secants drawn per g-point and column from [1.6, 1.7]), with and without the Jacobian, with and without
incident flux; with do_broadband, and the fused entry, under the automatic g-point split and once more in one range. The fused entry also
runs on the thin_dark band alone, on the seam band alone (ill-conditioned) and on the moderate band alone (well-conditioned), and with null
cloud arrays, which must give the bits of all-zero arrays.

Measured on an MI355X (this file's prints), worst over the shapes, orientations, quantities, angle sets, runs with and without incident
flux and both g-point splits; "model" is the model's error on the profile set where the kernel's is largest. The kernel figures were
measured on the GPU; the model's (E_regime, and the table of tests/test_lw1r_truth.py) on a CPU. eps of the dtype.
  per g-point (rrx_lw_solver_noscat_rescaled)
    regime              fp64 kernel   model     fp32 kernel   model
    moderate            4.3           4.0       5.7           7.2
    thin_dark           4.3e2         4.3e2     6.8           7.7
    opaque              1.5           1.1       1.4           1.4
    moderate_cloud      3.5           2.7       3.9           6.0
    conservative        2.2e3         2.2e3     18            27
    wide                4.3e3         4.3e3     28            37
    thin_lit            9.2e3         9.7e3     1.0e2         96
    near_conservative   2.9           2.1       2.9           4.6
    just_thick          6.5e5         6.5e5     48            87
    seam                1.9e6         1.9e6     1.8e2         3.0e2
  sums
    general entry with do_broadband, all g-points (seam)   fp64 1.5e3 (model 1.5e3)     fp32 3.9 (5.1)
    fused, all g-points (seam)                             fp64 1.5e3 (1.5e3)           fp32 4.1 (5.5)
    fused, thin_dark band alone                            fp64 3.8e2 (3.8e2)           fp32 5.5 (8.9)
    fused, seam band alone                                 fp64 8.7e5 (8.7e5)           fp32 1.7e2 (2.8e2)
    fused, moderate band alone                             fp64 4.6 (2.5)               fp32 2.8 (6.0)
    fused, null cloud arrays                               fp64 1.1e3 (1.1e3)           fp32 5.6 (5.8); the bits of all-zero arrays in every case
  The largest share of a bound that any kernel figure takes is 0.15 (thin_lit, per g-point, both dtypes); in the ill-conditioned regimes
  of fp64 it is 0.13, i.e. the model's own error (1/8). No profile is outside its bound and no kernel changed.
In fp64 the kernels reproduce the model's error to two digits in every ill-conditioned regime (seam, just_thick, thin_lit, wide,
conservative, thin_dark): what is measured there is the cancellation of the source factor on these inputs, which kernel and model
evaluate alike, and the three lane scans, fast_rcp and the LDS-table exp add nothing visible to it. (The largest kernel figures are
smaller than the largest entries of the CPU table, which also covers the profiles where the kernel is not at its worst.)
"""
import numpy as np
import pytest
import types

import lw_ref
import lw1r_truth as T
from lw1r_truth import CASES, IDS, NGPT, QUANTITIES, as_dict

pytestmark = pytest.mark.gpu
ALONE = (0, 2, 4)              # the bands that the fused entry also solves alone: thin_dark, seam, moderate


def _be(dt, hip_f64, hip_f32):
    return hip_f64 if dt == "f64" else hip_f32


class Dev:
    """the inputs of one shape on the device; gpts: only these g-points, as a problem of one band (ib)"""
    def __init__(self, be, dt, shape, gpts=None, ib=None):
        self.be, self.dt, self.shape = be, dt, shape
        I = T.inputs(dt, *shape)
        self.up = up = lambda a: be.asarray(np.ascontiguousarray(np.array(a)))     # (a copy: the shared inputs are read-only)
        self.g_sel = g = slice(None) if gpts is None else gpts
        b = slice(None) if ib is None else slice(ib, ib + 1)
        self.tau, self.ssa, self.g, self.lay, self.lev = (up(I[k][g]) for k in ("tau", "ssa", "g", "lay", "lev"))
        self.emis, self.ssrc, self.sjac, self.inc = (up(I[k][g]) for k in ("emis", "ssrc", "sjac", "inc"))
        self.tau_g = up(I["tau_g"][g])
        self.fr = dict(pfrac=up(I["pfrac"][g]), blay=up(I["blay"][b]), blev=up(I["blev"][b]), sfc_src=self.ssrc)
        self.cloud = tuple(up(I[k][b]) for k in ("tau_c", "ssa_c", "g_c"))
        self.zero_cloud = tuple(up(np.zeros_like(I[k][b])) for k in ("tau_c", "ssa_c", "g_c"))
        if gpts is None:
            gb, lims = I["gb"], I["band_lims"]
        else:
            gb, lims = np.ones(len(gpts), dtype=np.int32), np.array([[1, len(gpts)]], dtype=np.int32)
        self.kd = types.SimpleNamespace(gpoint_bands=up(gb), band_lims_gpt=up(lims))

    def angles(self, angles):
        sec, w = T.angles_of(self.dt, *self.shape, angles)
        return self.up(sec[:, self.g_sel]), self.up(w)

    def numpy(self, r):
        return {k: self.be.to_numpy(v) for k, v in r.items()}


def _check_summed(rep, what, dt, shape, top_at_1, entry, angles, with_inc, got, gpts=None):
    gpts = np.arange(NGPT) if gpts is None else gpts
    for q in got:
        assert got[q].shape == (shape[1] + 1, shape[0]), (q, got[q].shape)
    rep.check(what, got, as_dict(T.model(dt, *shape, top_at_1, entry, angles, with_inc), gpts, True),
              as_dict(T.truth(dt, *shape, top_at_1, entry, angles, with_inc), gpts), T.column_regimes(T.regimes(dt, *shape)[gpts]))


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_general_entry_per_gpoint(dt, shape, top_at_1, hip_f64, hip_f32):
    """rrx_lw_solver_noscat_rescaled, per-g-point fluxes: one and three angles, with and without the Jacobian, with and without
    incident flux; every profile against its own regime"""
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = T.report(dt)
    reg = T.regimes(dt, *shape)
    for angles in ("1", "3"):
        sec, w = d.angles(angles)
        for with_inc in (True, False):
            mod, truth = as_dict(T.model(dt, *shape, top_at_1, "general", angles, with_inc)), as_dict(T.truth(dt, *shape, top_at_1, "general", angles, with_inc))
            for jac in (False, True):
                r = be.lw_solver_noscat_rescaled(top_at_1, sec, w, d.tau, d.ssa, d.g, d.lay, d.lev, d.emis, d.ssrc, inc_flux=d.inc if with_inc else None,
                                                 do_jacobians=jac, sfc_src_jac=d.sjac if jac else None)
                got = d.numpy(r)
                assert set(got) == set(QUANTITIES[:3 if jac else 2])
                rep.check(f"general per-g-point {shape} top_at_1={top_at_1} angles={angles} inc={with_inc} jac={jac}", got, mod, truth, reg)
    rep.done()


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_general_entry_in_broadband_mode(dt, shape, top_at_1, hip_f64, hip_f32):
    """rrx_lw_solver_noscat_rescaled(do_broadband), one and three angles: the sums over all g-points, under both g-point splits"""
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = T.report(dt)
    for label, ctx in lw_ref.splits(be):
        with ctx:
            for angles in ("1", "3"):
                sec, w = d.angles(angles)
                for with_inc in (True, False):
                    r = be.lw_solver_noscat_rescaled(top_at_1, sec, w, d.tau, d.ssa, d.g, d.lay, d.lev, d.emis, d.ssrc, inc_flux=d.inc if with_inc else None,
                                                     do_broadband=True)
                    _check_summed(rep, f"general broadband {shape} top_at_1={top_at_1} angles={angles} inc={with_inc}, {label}", dt, shape, top_at_1,
                                  "general", angles, with_inc, d.numpy(r))
    rep.done()


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_fractions_entry(dt, shape, top_at_1, hip_f64, hip_f32):
    """rrx_lw_solver_noscat_fractions_rescaled (one angle): all g-points with and without incident flux, the bands of ALONE each alone,
    null cloud arrays (the bits of all-zero arrays, and the truth of pure gas absorption); under both g-point splits"""
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = T.report(dt)

    def run(dev, cloud, with_inc):
        sec, w = dev.angles("1")
        return dev.numpy(be.lw_solver_noscat_fractions_rescaled(top_at_1, dev.kd, sec, w, dev.tau_g, dev.fr, dev.emis, cloud=cloud,
                                                                inc_flux=dev.inc if with_inc else None))
    for label, ctx in lw_ref.splits(be):
        with ctx:
            what = f"fractions {shape} top_at_1={top_at_1}, {label}"
            for with_inc in (True, False):
                _check_summed(rep, f"{what} inc={with_inc}", dt, shape, top_at_1, "fused", "1", with_inc, run(d, d.cloud, with_inc))
            for ib in ALONE:
                gpts = T.band_gpoints(ib)
                sub = Dev(be, dt, shape, gpts, ib)
                _check_summed(rep, f"{what} band {ib + 1} alone", dt, shape, top_at_1, "fused", "1", True, run(sub, sub.cloud, True), gpts)
            null, zero = run(d, None, True), run(d, d.zero_cloud, True)
            for q in null:
                assert np.array_equal(null[q], zero[q]), f"{what}: null cloud arrays and all-zero arrays differ in {q}"
            _check_summed(rep, f"{what} null cloud", dt, shape, top_at_1, "null", "1", True, null)
    rep.done()
