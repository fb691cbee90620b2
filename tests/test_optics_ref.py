"""CPU tests of tests/optics_ref.py, the numpy references of tests/test_gpu_optics_kernels.py: against the goldens of the reference's
unmodified CPU classes (cloud and aerosol optics) and of its kernel text (increments, delta scaling), at the tolerances
tests/test_oracle_golden.py grants the oracle on the same files; on cases small enough to check by hand; and the size of e_ref, the
working-precision evaluation's own error, on the inputs of the GPU tolerance tests. A wrong reference must not be able to make a
wrong kernel pass."""
import os

import numpy as np
import pytest

import cases
import optics_ref as ref
from rte_rrtmgp_cpp_amd import synthetic

LD = np.longdouble


def golden_close(name, got, want):
    """the oracle's tolerance on the goldens (tests/test_oracle_golden.py, cases.Checker): 1e-13 / 2e-6 with the floors 1e-6 / 1e-2"""
    f64 = want.dtype == np.float64
    e = cases.rel_err(np.asarray(got, dtype=np.float64), want, 1e-6 if f64 else 1e-2)
    assert e <= (1e-13 if f64 else 2e-6), (name, e)


# ==== against the goldens =========================================================================================================
@pytest.mark.parametrize("path", cases.golden_files("cloud_"), ids=os.path.basename)
def test_cloud_optics_matches_reference_cpu_class(path):
    G = np.load(path)
    lut = synthetic.make_cloud_lut(int(G["lut_nbnd"]), str(G["lut_kind"]))
    assert cases.optics_lut_digest(lut) == str(G["lut_digest"])
    dt = G["clwp"].dtype
    for ctype in (LD, dt.type):
        two, one, _ = ref.cloud_optics(lut, G["clwp"], G["ciwp"], G["reliq"], G["deice"], ctype)
        for name, got in zip(("tau_2str", "ssa_2str", "g_2str"), two):
            golden_close(name, got, G[name])
        if ctype is LD and str(G["lut_kind"]) == "sw":
            # On the SW table the 1-scalar tau is a difference of nearly equal terms (ssa about 0.97): the fp32 golden itself, rounded
            # operation by operation, lies 57 to 60 epsilons (7e-6) from the truth relative to the result. The truth is therefore
            # held to the same tolerance relative to the extinction; the working-precision evaluation, which rounds as the
            # reference's class does, to the plain one.
            f64 = dt == np.float64
            scale = np.abs(G["tau_2str"]) + (1e-6 if f64 else 1e-2)*np.max(G["tau_2str"])
            err = float(np.max(np.abs(one - G["tau_1scl"].astype(LD)) / scale))
            assert err <= (1e-13 if f64 else 2e-6), err
        else:
            golden_close("tau_1scl", one, G["tau_1scl"])


@pytest.mark.parametrize("path", cases.golden_files("aerosol_"), ids=os.path.basename)
def test_aerosol_optics_matches_reference_cpu_class(path, tmp_path):
    G = np.load(path)
    lut = cases.real_aerosol_lut(tmp_path) if str(G["table"]) == "real" else synthetic.make_aerosol_lut(5)
    assert cases.optics_lut_digest(lut) == str(G["lut_digest"])
    dt = G["rh"].dtype
    lut = {k: v.astype(dt) for k, v in lut.items()}
    aermr = [G["aermr%02d" % i] for i in range(1, 12)]
    for ctype in (LD, dt.type):
        got = ref.aerosol_optics(lut, aermr, G["rh"], G["p_lev"], ctype)
        for name, a in zip(("tau", "ssa", "g"), got):
            golden_close(name, a, G[name])
    # and the vectorised evaluation that pins the oracle: the same expressions in the same order, so the same bits
    want = cases.aerosol_optics_numpy(lut, aermr, G["rh"], G["p_lev"])
    for a, b in zip(ref.aerosol_optics(lut, aermr, G["rh"], G["p_lev"], dt.type), want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("path", cases.golden_files("random_"), ids=os.path.basename)
def test_increments_and_delta_scale_match_reference_kernel_text(path):
    G = np.load(path)
    dt = G["lw_tau"].dtype
    t1, w1, g1 = G["lw_tau"], G["sw_ssa"], G["sw_g"]
    for ctype in (LD, dt.type):
        for name, got in zip(("tau", "ssa", "g"), ref.increment_2stream(t1, w1, g1, G["op_t2"], G["op_w2"], G["op_g2"], ctype)):
            golden_close("op_inc2_" + name, got, G["op_inc2_" + name])
        for name, got in zip(("tau", "ssa", "g"), ref.delta_scale(t1, w1, g1, ctype)):
            golden_close("op_ds_" + name, got, G["op_ds_" + name])
    golden_close("op_inc1_tau", ref.increment_1scalar(t1, G["op_t2"]), G["op_inc1_tau"])


# ==== by hand =====================================================================================================================
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cloud_optics_by_hand(dtype):
    """ref.hand_cloud_case: liquid water path 2 in every cloudy cell. Radius 4: on the middle node. 2 and 6: the ends of the table
    (at the upper end the index stays nsize-1 and the weight is 1). -3: 2.5 steps below, index clamped to 1, weight -2.5: ext =
    4 - 2.5*(2 - 4) = 9. 11: 2.5 steps above, index 2, weight 3.5: ext = 2 + 3.5*(1.5 - 2) = 0.25. Then a cloud-free cell with
    garbage sizes, an ice-only cell and a cell with both phases."""
    lut, clwp, ciwp, reliq, deice = ref.hand_cloud_case(dtype)
    index, x = ref.size_table_position(reliq, 2., 6., 3, clwp > 0)
    assert index.tolist() == [[2, 1, 2, 1, 2, 1, 1, 2]] and x.tolist() == [[1., 0., 2., -2.5, 4.5, 0., 0., 1.]]
    for ctype in (LD, dtype):
        (tau, ssa, g), one, (td, wd, gd) = ref.cloud_optics(lut, clwp, ciwp, reliq, deice, ctype)
        assert tau.shape == (1, 1, 8) and tau.dtype == np.dtype(ctype)
        # liquid only: tau = 2*ext, ssa and g straight from the tables
        assert tau[0, 0, :5].tolist() == [4., 8., 3., 18., .5]
        assert ssa[0, 0, :5].tolist() == [.25, .5, .75, 1.125, 2.]
        assert g[0, 0, :5].tolist() == [.5, .5, .25, .5, -.375]
        assert one[0, 0, :5].tolist() == [3., 4., .75, -2.25, -.5]                      # tau - tau*ssa
        # cloud-free, whatever the sizes hold: exact zeros in every form
        for a in (tau, ssa, g, one, td, wd, gd):
            assert a[0, 0, 5] == 0 and not np.signbit(a[0, 0, 5])
        # ice only (path 1 on the node 20): ext .5; both: tau = 4 + .5, tau*ssa = 1 + .25, tau*ssa*g = .5 + .125
        assert (tau[0, 0, 6], ssa[0, 0, 6], g[0, 0, 6], one[0, 0, 6]) == (.5, .5, .5, .25)
        assert tau[0, 0, 7] == 4.5 and g[0, 0, 7] == .5 and one[0, 0, 7] == 3.25
        assert abs(ssa[0, 0, 7] - LD(1.25)/LD(4.5)) <= np.finfo(dtype).eps
        # delta scaling of the node cell: f = 1/4, w*f = 1/16: tau 4*15/16, ssa (3/16)/(15/16), g (1/4)/(3/4)
        assert td[0, 0, 0] == 3.75 and abs(wd[0, 0, 0] - LD(.2)) <= np.finfo(dtype).eps and abs(gd[0, 0, 0] - LD(1)/3) <= np.finfo(dtype).eps
        # ... and it is delta_scale of the two-stream triple
        if ctype is dtype:
            for a, b in zip((td, wd, gd), ref.delta_scale(tau, ssa, g, dtype)):
                assert np.array_equal(a, b)


def test_humidity_classes_and_aerosol_optics_by_hand():
    """bounds .3 .6 1: humidity on a bound belongs to the class below it, 0 to the first class, 1.05 (above every bound) to the last.
    One species (aermr01 = SS1, hydrophilic column 0) with mixing ratio 1 over a layer of dp = 9.81: tau is the table entry of the
    cell's class."""
    rh_upper = np.array([.3, .6, 1.])
    rh = np.array([[0., .3, .31, .6, 1., 1.05]])
    assert ref.humidity_class(rh_upper, rh).tolist() == [[0, 0, 1, 1, 2, 2]]
    assert ref.humidity_class(rh_upper[:1], rh).tolist() == [[0]*6]
    lut = dict(rh_upper=rh_upper, mext_phobic=np.ones((11, 1)), ssa_phobic=np.full((11, 1), .5), g_phobic=np.full((11, 1), .25),
               mext_philic=np.ones((5, 3, 1)), ssa_philic=np.full((5, 3, 1), .5), g_philic=np.full((5, 3, 1), .25))
    lut["mext_philic"][0, :, 0] = [1., 2., 4.]
    plev = np.array([[9.81]*6, [0.]*6])
    aermr = [np.zeros((1, 6)) for _ in range(11)]
    aermr[0] = np.ones(1)                                               # a profile
    for ctype in (LD, np.float64):
        tau, ssa, g = ref.aerosol_optics(lut, aermr, rh, plev, ctype)
        assert tau[0, 0].tolist() == [1., 1., 2., 2., 4., 4.] and (ssa == .5).all() and (g == .25).all()
        # the reversed column order gives the same (|dp|)
        tau, _, _ = ref.aerosol_optics(lut, aermr, rh, plev[::-1], ctype)
        assert tau[0, 0].tolist() == [1., 1., 2., 2., 4., 4.]
    # hydrophobic dust (aermr05 -> column 7) is looked up without the class; all eleven mixing ratios 0: exact zeros
    lut["mext_phobic"][7, 0] = 8.
    aermr[0] = np.zeros(1); aermr[4] = np.full((1, 6), .5)
    tau, ssa, g = ref.aerosol_optics(lut, aermr, rh, plev, np.float64)
    assert (tau == 4.).all() and (ssa == .5).all() and (g == .25).all()
    aermr[4] = np.zeros((1, 6))
    for a in ref.aerosol_optics(lut, aermr, rh, plev, np.float64):
        assert not a.any() and not np.signbit(a).any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_increments_delta_scale_and_sums_by_hand(dtype):
    a = lambda *v: np.array(v, dtype=dtype)
    tiny = np.finfo(dtype).tiny
    # tau 1 (ssa .5, g .5) + tau 3 (ssa .5, g .25): tau 4, scattering .5 + 1.5 = 2, ssa .5, g (.25 + .375)/2
    t, w, g = ref.increment_2stream(a(1.), a(.5), a(.5), a(3.), a(.5), a(.25), dtype)
    assert (t[0], w[0], g[0]) == (4., .5, .3125)
    # both tau 0: zeros; both ssa 0: g = 0; tau2 = 0: tau unchanged; tau below the floor 3*tiny: divided by the floor, not by tau
    t, w, g = ref.increment_2stream(a(0., 2., 2., tiny), a(.5, 0., .5, 1.), a(.5, .5, .5, .5), a(0., 1., 0., tiny), a(.5, 0., .5, 1.),
                                    a(.5, .5, .5, .5), dtype)
    assert t.tolist() == [0., 3., 2., float(2*tiny)] and w.tolist()[:3] == [0., 0., .5] and g.tolist()[:3] == [0., 0., .5]
    assert w[3] == dtype(2*tiny) / ref.floor_of(dtype) and abs(float(w[3]) - 2/3) < 1e-6
    # delta scaling: g = 0 is the identity; g = 1: g' = 0; g = 1, ssa = 1: tau' = ssa' = 0; ssa = 0: tau unchanged, ssa' = 0
    t, w, g = ref.delta_scale(a(2., 2., 2., 2.), a(.75, .5, 1., 0.), a(0., 1., 1., .5), dtype)
    assert t.tolist() == [2., 1., 0., 2.] and w.tolist() == [.75, 0., 0., 0.] and g.tolist()[:3] == [0., 0., 0.]
    # g = .5, ssa = .5: f = 1/4, wf = 1/8: tau*7/8, ssa (3/8)/(7/8), g (1/4)/(3/4)
    t, w, g = ref.delta_scale(a(8.), a(.5), a(.5), np.longdouble)
    assert t[0] == 7. and abs(w[0] - LD(3)/7) < 1e-18 and abs(g[0] - LD(1)/3) < 1e-18
    # sums: -0.0 columns sum to +0.0 (the sum starts from +0.0); no g-points: zeros
    gpt = np.array([[[1., -0.]], [[2., -0.]], [[4., -0.]]], dtype=dtype)
    s = ref.sum_broadband(gpt)
    assert s.tolist() == [[7., 0.]] and not np.signbit(s).any() and s.dtype == dtype
    assert ref.sum_broadband(gpt[:0]).tolist() == [[0., 0.]]
    assert ref.net_broadband(a(5., 1.), a(2., 3.)).tolist() == [3., -2.]
    assert ref.increment_1scalar(a(1., 2.), a(.5, -2.)).tolist() == [1.5, 0.]
    src, fac = a(1., 2., 3.), a(.5, 2.)
    assert ref.spread_col(src, 2).tolist() == [[1., 1.], [2., 2.], [3., 3.]]
    assert ref.scaling_to_subset(ref.spread_col(src, 2), fac).tolist() == [[.5, 2.], [1., 4.], [1.5, 6.]]
    assert np.array_equal(ref.toa_source(src, fac, 2), ref.scaling_to_subset(ref.spread_col(src, 2), fac))
    assert np.array_equal(ref.toa_source(src, None, 2), ref.spread_col(src, 2))


def test_col_dry_by_hand():
    """dry air (h = 0) over dp = 9.80665 Pa: 10*dp*N_A/(1000*m_dry*100*g0) = N_A/(1e4*m_dry) molecules per cm2; either column order"""
    plev = np.array([[1000.], [1000. - 9.80665]])
    want = LD(6.02214076e23) / (LD(1e4) * LD(0.028964))
    for p in (plev, plev[::-1]):
        got = ref.col_dry(np.zeros((1, 1)), p, LD)
        assert abs(got[0, 0] - want) <= 1e-12*want                     # (dp itself is rounded: 1000 - 9.80665 is not exact)
    # water vapour: the mean molar mass goes down and the dry share is 1/(1 + h)
    h = 0.04
    m_air = (LD(0.028964) + LD(0.018016)*LD(h)) / (1 + LD(h))
    got = ref.col_dry(np.full((1, 1), h), plev, LD)
    assert abs(got[0, 0] - want*LD(0.028964)/m_air/(1 + LD(h))) <= 1e-12*want


# ==== e_ref on the inputs of the GPU tolerance tests ==============================================================================
def e_ref_table(work, truth, names, scales=None):
    out = {}
    for i, name in enumerate(names):
        e, zeros_exact = ref.rel_errors(work[i], truth[i], None if scales is None else scales.get(name))
        assert zeros_exact, name
        out[name] = e
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_working_precision_error_stays_within_the_cap(dtype, capsys):
    """e_ref <= 16 epsilons for every output the GPU tolerance tests bound by it, on their inputs (4 000 random cells plus nodes
    and out-of-table sizes for the clouds). The 1-scalar cloud tau on the SW table is a difference of nearly equal terms (ssa about
    0.97): relative to the result its e_ref is far above the cap, relative to the extinction it is inside."""
    dt = np.dtype(dtype)
    lines = []
    for kind in ("lw", "sw"):
        lut = synthetic.make_cloud_lut(3, kind)
        args = ref.cloud_inputs(lut, 1, 4048, np.random.default_rng(1), dt)
        assert (args[0] == 0).mean() > 0.2 and (args[1] == 0).mean() > 0.2
        tw, ow, dw = ref.cloud_optics(lut, *args, dt.type)
        tt, ot, dtr = ref.cloud_optics(lut, *args, LD)
        e = e_ref_table(tw + dw, tt + dtr, ("tau", "ssa", "g", "tau_delta", "ssa_delta", "g_delta"))
        e["tau_1scl"], _ = ref.rel_errors(ow, ot, tt[0] if kind == "sw" else None)
        if kind == "sw":
            assert ref.rel_errors(ow, ot)[0] > ref.E_REF_CAP                          # why the extinction is the scale there
        lines.append((f"cloud {kind}", e))
    for table, lut in (("synthetic", synthetic.make_aerosol_lut(3)), ("nhum1", synthetic.make_aerosol_lut(2, nhum=1))):
        lut = {k: v.astype(dt) for k, v in lut.items()}
        for top_at_1 in (False, True):
            aermr, rh, plev = ref.aerosol_inputs(lut, 40, 100, top_at_1, "mixed", np.random.default_rng(2), dt)
            e = e_ref_table(ref.aerosol_optics(lut, aermr, rh, plev, dt.type), ref.aerosol_optics(lut, aermr, rh, plev, LD), ("tau", "ssa", "g"))
            lines.append((f"aerosol {table} top_at_1={top_at_1}", e))
    a = ref.two_stream_inputs((3, 7, 190), np.random.default_rng(3), dt) + ref.two_stream_inputs((3, 7, 190), np.random.default_rng(4), dt)
    lines.append(("increment_2stream", e_ref_table(ref.increment_2stream(*a, dt.type), ref.increment_2stream(*a, LD), ("tau", "ssa", "g"))))
    lines.append(("delta_scale", e_ref_table(ref.delta_scale(*a[:3], dt.type), ref.delta_scale(*a[:3], LD), ("tau", "ssa", "g"))))
    for top_at_1 in (False, True):
        h, p = ref.col_dry_inputs(40, 100, top_at_1, np.random.default_rng(5), dt)
        e, _ = ref.rel_errors(ref.col_dry(h, p, dt.type), ref.col_dry(h, p, LD))
        lines.append((f"col_dry top_at_1={top_at_1}", {"col_dry": e}))
    with capsys.disabled():
        for what, e in lines:
            print(f"\n  e_ref {dt.name} {what}: " + ", ".join(f"{k} {v:.2f}" for k, v in e.items()), end="")
    for what, e in lines:
        for k, v in e.items():
            assert v <= ref.E_REF_CAP, (what, k, v)
