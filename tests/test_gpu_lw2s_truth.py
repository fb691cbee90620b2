"""GPU tests of the two LW two-stream entries (rrx_lw_solver_2stream, rrx_lw_solver_2stream_fractions; csrc/rrx_solver_lw2s.hip) against
the longdouble truth of tests/lw2s_truth.py, regime by regime.

Every other comparison of these entries (tests/test_gpu_lw_2stream.py) is with tests/lw2s_ref.py, the as-written formulas in the same
precision, in cases.rel_err's norm; that reference is 2e6 ... 8e10 eps from truth on every thin g-point (tests/test_lw2s_truth.py), hence
tolerances of 2.1e-8 (fp64) and 9.1e-2 (fp32) per g-point. Here each (g-point, column) profile is compared with a solve in np.longdouble
that evaluates the same function without its cancellations, and falls into one regime (lw2s_truth.GPOINT_REGIMES, regime_ranges). Norm:
lw_ref.profile_error per quantity (flux_up, flux_dn), in eps of the dtype.

Bound. Per regime and quantity, kernel <= 8 x max(E_regime, 32 eps) (lw_ref.bound_eps; margin and floor are lw_ref's, for its reasons).
E_regime is the worst error against the same truth of lw2s_truth's regrouped model -- the formulas of the kernel file's header in the run's
dtype with numpy, the C library's exp, true division and sequential recurrences -- in the same regime, shape, orientation, dtype, entry
and quantity. For the sums (do_broadband, the fused entry) the model is added in g-point order in the run's dtype, the truth in longdouble,
and a column takes the regime of lw2s_truth.column_regimes. Nothing in a bound comes from a kernel; seed, ranges and lists are chosen in
lw2s_truth.py from the inputs and the models alone, and each says so where it stands. All outputs must be finite.

UNRESOLVED CELLS. A cell whose bound exceeds 1e-2 of the profile's largest flux tests nothing. tests/test_lw2s_truth.py computes that list
from the model alone and asserts that it is flux_dn of thin_dark and thin_unlit in fp32 and nothing else: the regrouped formula's remaining
absolute error of a few eps in c, times (lev_bot - lev_top)/(tau G lev), is of order one where tau is 1e-7 and flux_dn is layer emission
alone. Those two cells are printed and bounded like the others here, but they say nothing about the kernel. In fp64 the list is empty
(largest bound 3.2e-11).

Inputs: lw2s_truth.inputs, 15 g-points in nine uneven bands, one regime per band; sfc_emis == 1 in every third column; four g-points
without incident flux, one of them without surface emission. Shapes: lw2s_truth.SHAPES, the smallest layer counts that reach each tiling
of lw2s_fused (written beside the list) and 600 layers, which no tiling takes (materialised route, serial kernel); both orientations on
the two smallest of each dtype. The fused entry and the general entry with do_broadband run under the automatic g-point split and once more
in one range (lw_ref.splits). The fused entry also runs on the thin_dark band alone and on the conservative band alone (ill-conditioned)
and on the moderate band alone (well-conditioned), so that none hides behind the others in the whole-array sum, and with null cloud
arrays, which must give the bits of all-zero arrays.

Measured on an MI355X (this file's prints), worst over the shapes, orientations, quantities, runs with and without incident flux and both
g-point splits; "model" is the regrouped model's error on the profile set where the kernel's is largest. The kernel figures were measured
on the GPU; the model's (E_regime, and the tables of tests/test_lw2s_truth.py) on a CPU. eps of the dtype.
  per g-point (rrx_lw_solver_2stream)
    regime              fp64 kernel   model     fp32 kernel   model
    opaque              2.1           1.9       2.3           2.3
    moderate            2.6           2.5       3.5           3.2
    moderate_cloud      3.6           3.6       3.5           3.3
    wide                8.1           3.0       5.3           3.1
    switch              99            1.1e2     97            1.2e2
    near_conservative   63            59        78            58
    thin_lit            1.8e2         1.6e2     1.1e2         1.0e2
    conservative        5.1e3         3.3e3     2.4e2         2.2e2
    thin_unlit          6.1e3         7.4e3     6.1e3         4.4e3      (fp32 flux_dn: unresolved)
    thin_dark           2.6e4         1.8e4     2.1e4         3.2e4      (fp32 flux_dn: unresolved)
    The largest share of a bound is 0.32 in fp64 (conservative) and 0.24 in fp32 (thin_dark): every profile is inside.
  sums
    rrx_lw_solver_2stream(do_broadband), all g-points     fp64 2.6e2 (model 6.5e2)      fp32 38 (model 53)
    fused, all g-points                                   fp64 3.3e2 (model 2.3e2)      fp32 39 (model 54)
    fused, thin_dark band alone                           fp64 2.6e4 (1.8e4)            fp32 2.1e4 (3.2e4)
    fused, moderate band alone                            fp64 2.3 (1.6)                fp32 2.5 (2.0)
    fused, conservative band alone                        fp64 5.1e3 (3.3e3)            fp32 2.3e2 (3.5e2)
    fused, null cloud arrays                              fp64 8.7 (16)                 fp32 13 (23); the bits of all-zero arrays in every case
THE FINDING, AND ITS FIX. On its first run this file put the fused fp64 kernel outside the bound in the conservative regime (ssa = 1
exactly, tau in (1e-4, 10^1.5), three layers of 0) from 140 layers on, alone and therefore in the sum of all g-points; the serial kernel,
the materialised route, fp32 (conservative range (1e-4, 1)) and null cloud arrays were inside. The conservative band alone, flux_dn
(flux_up alike), eps of fp64, before and after the change of the kernel:
    layers          15     40      80      140      180      200      300      400      500      600 (materialised route, serial kernel)
    kernel before   11     2.0e2   1.9e3   1.07e4   1.24e4   1.19e4   3.84e4   8.82e4   1.02e5   5.1e3
    kernel now      9.8    74      2.8e2   5.1e2    3.7e2    7.3e2    1.3e3    3.2e3    2.3e3    5.1e3
    model           24     51      2.7e2   5.1e2    6.9e2    7.3e2    8.5e2    2.3e3    3.0e3    3.3e3
    bound           256    4.1e2   2.1e3   4.1e3    5.5e3    5.9e3    6.8e3    1.8e4    2.4e4    2.6e4
Cause: the fused kernel scanned the albedo as a normalised Moebius composite per lane, and the normalisation of two composed sub-stacks,
1 + m10 p01 = 1 - R R', cancels as both reflectances approach 1 (a conservative stack of optical depth T reflects 1 - O(1/T)); the
sequential recurrence's 1 - Rdif a never does. A numpy restatement of the scan on the float64 Rdif, Tdif of these inputs left the albedo at
the lanes' chunk boundaries 1.2e2 / 2.1e2 / 6.7e2 eps off at 80 / 140 / 500 layers where the sequential recurrence is 3 / 5 / 8 eps off;
the same scan on the co-albedo 1 - a, whose map has non-negative coefficients only, 11 / 10 / 22 eps. (The CPU model with the kernel's
ssa = tau_c ssa_c x rcp(tau) in place of the division did not move: that candidate was ruled out.) The kernel now scans the co-albedo, with
the layer's absorptance 1 - Rdif - Tdif = RT (k u^2 + (gamma1 - gamma2) m) formed without the subtraction (csrc/rrx_solver_lw2s.hip);
every other figure of this header is unchanged by it to the digits shown.
"""
import numpy as np
import pytest
import types

import lw_ref
import lw2s_truth as T
from lw2s_truth import CASES, IDS, NGPT, as_dict

pytestmark = pytest.mark.gpu
ALONE = (0, 3, 6)              # the bands that the fused entry also solves alone: thin_dark, moderate, conservative


def _be(dt, hip_f64, hip_f32):
    return hip_f64 if dt == "f64" else hip_f32


class Dev:
    """the inputs of one shape on the device; gpts: only these g-points, as a problem of one band (ib)"""
    def __init__(self, be, dt, shape, gpts=None, ib=None):
        self.be = be
        I = T.inputs(dt, *shape)
        up = lambda a: be.asarray(np.ascontiguousarray(np.array(a)))             # (a copy: the shared inputs are read-only)
        g = slice(None) if gpts is None else gpts
        b = slice(None) if ib is None else slice(ib, ib + 1)
        self.tau, self.ssa, self.g, self.lev = (up(I[k][g]) for k in ("tau", "ssa", "g", "lev"))
        self.emis, self.ssrc, self.inc = (up(I[k][g]) for k in ("emis", "ssrc", "inc"))
        self.tau_g = up(I["tau_g"][g])
        self.fr = dict(pfrac=up(I["pfrac"][g]), blev=up(I["blev"][b]), sfc_src=self.ssrc)
        self.cloud = tuple(up(I[k][b]) for k in ("tau_c", "ssa_c", "g_c"))
        self.zero_cloud = tuple(up(np.zeros_like(I[k][b])) for k in ("tau_c", "ssa_c", "g_c"))
        if gpts is None:
            gb, lims = I["gb"], I["band_lims"]
        else:
            gb, lims = np.ones(len(gpts), dtype=np.int32), np.array([[1, len(gpts)]], dtype=np.int32)
        self.kd = types.SimpleNamespace(gpoint_bands=up(gb), band_lims_gpt=up(lims))

    def numpy(self, r):
        return {k: self.be.to_numpy(v) for k, v in r.items()}


def _check_summed(rep, what, dt, shape, top_at_1, entry, with_inc, got, gpts=None):
    """got: dict of (nlev, ncol) sums over the g-points gpts (default: all)"""
    gpts = np.arange(NGPT) if gpts is None else gpts
    for q in got:
        assert got[q].shape == (shape[1] + 1, shape[0]), (q, got[q].shape)
    rep.check(what, got, as_dict(T.model(dt, *shape, top_at_1, entry, with_inc), gpts, True), as_dict(T.truth(dt, *shape, top_at_1, entry, with_inc), gpts),
              T.column_regimes(T.regimes(dt, *shape, with_inc)[gpts]))


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_general_entry_per_gpoint(dt, shape, top_at_1, hip_f64, hip_f32):
    """rrx_lw_solver_2stream, per-g-point fluxes, with and without incident flux: every profile against its own regime"""
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = T.report(dt)
    for with_inc in (True, False):
        got = d.numpy(be.lw_solver_2stream(top_at_1, d.tau, d.ssa, d.g, d.lev, d.emis, d.ssrc, inc_flux=d.inc if with_inc else None))
        assert set(got) == set(T.QUANTITIES)
        rep.check(f"general per-g-point {shape} top_at_1={top_at_1} inc={with_inc}", got, as_dict(T.model(dt, *shape, top_at_1, "general", with_inc)),
                  as_dict(T.truth(dt, *shape, top_at_1, "general", with_inc)), T.regimes(dt, *shape, with_inc))
    rep.done()


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_general_entry_in_broadband_mode(dt, shape, top_at_1, hip_f64, hip_f32):
    """rrx_lw_solver_2stream(do_broadband): the sums over all g-points, under both g-point splits"""
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = T.report(dt)
    for label, ctx in lw_ref.splits(be):
        with ctx:
            for with_inc in (True, False):
                r = be.lw_solver_2stream(top_at_1, d.tau, d.ssa, d.g, d.lev, d.emis, d.ssrc, inc_flux=d.inc if with_inc else None, do_broadband=True)
                _check_summed(rep, f"general broadband {shape} top_at_1={top_at_1} inc={with_inc}, {label}", dt, shape, top_at_1, "general", with_inc, d.numpy(r))
    rep.done()


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_fractions_entry(dt, shape, top_at_1, hip_f64, hip_f32):
    """rrx_lw_solver_2stream_fractions: all g-points with and without incident flux, the bands of ALONE each alone, null
    cloud arrays (the bits of all-zero arrays, and the truth of pure gas absorption); under both g-point splits.
    The conservative band alone is what found the cancelling normalisation of the albedo scan (this file's header)."""
    be = _be(dt, hip_f64, hip_f32)
    d = Dev(be, dt, shape)
    rep = T.report(dt)
    run = lambda dev, cloud, with_inc: dev.numpy(be.lw_solver_2stream_fractions(top_at_1, dev.kd, dev.tau_g, dev.fr, dev.emis, cloud=cloud,
                                                                                inc_flux=dev.inc if with_inc else None))
    for label, ctx in lw_ref.splits(be):
        with ctx:
            what = f"fractions {shape} top_at_1={top_at_1}, {label}"
            for with_inc in (True, False):
                _check_summed(rep, f"{what} inc={with_inc}", dt, shape, top_at_1, "fused", with_inc, run(d, d.cloud, with_inc))
            for ib in ALONE:
                gpts = T.band_gpoints(ib)
                sub = Dev(be, dt, shape, gpts, ib)
                _check_summed(rep, f"{what} band {ib + 1} alone", dt, shape, top_at_1, "fused", True, run(sub, sub.cloud, True), gpts)
            null, zero = run(d, None, True), run(d, d.zero_cloud, True)
            for q in T.QUANTITIES:
                assert np.array_equal(null[q], zero[q]), f"{what}: null cloud arrays and all-zero arrays differ in {q}"
            _check_summed(rep, f"{what} null cloud", dt, shape, top_at_1, "null", True, null)
    rep.done()
