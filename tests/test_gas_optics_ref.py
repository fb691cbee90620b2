"""The NumPy reference of the gas optics (tests/gas_optics_ref.py) against the CPU oracle, in fp64 and fp32, on a regular
k-distribution, on irregular ones (tests/gas_cases.py: unequal bands, contributor intervals of every kind) and on atmospheres
that leave the tables. Integer outputs are equal; floating outputs agree to the rounding floor of the arithmetic, which the
long-double reference measures here (e_oracle, e_oracle32) and gas_cases.E_ORACLE / E_ORACLE32 record: the tolerances of the GPU
tests (tests/test_gpu_gas_optics_edges.py) are set from those records."""
import numpy as np
import pytest

import cases
import gas_cases as gc
import gas_optics_ref as ref

NCOL, NLAY = 193, 30        # the shape of the fp32 GPU cases; the fp64 bound does not depend on the measured floor (8 e_oracle < 1e-12)
CASES = [("regular", "whole")] + [("irregular", v) for v in gc.VARIANTS] + [("edges", "whole")]
IDS = [f if f != "irregular" else f + "-" + v for f, v in CASES]


def as_int(a):
    return np.asarray(a).astype(np.int64)


@pytest.mark.parametrize("kind", ["lw", "sw"])
@pytest.mark.parametrize("family,variant", CASES, ids=IDS)
def test_reference_matches_oracle_fp64(family, variant, kind, oracle_f64):
    kd, atm, col_dry, col_gas, _ = gc.family_case(oracle_f64, family, kind, NCOL, NLAY, variant=variant)
    r64 = gc.reference_outputs(kd, atm, col_dry, col_gas, np.float64)
    rld = gc.reference_outputs(kd, atm, col_dry, col_gas, np.longdouble)
    o = gc.shaped_route(oracle_f64, kd, atm, col_dry, col_gas)
    for k in gc.INT_KEYS:
        assert np.array_equal(as_int(o["it_" + k]), as_int(r64["it_" + k])), k
        assert np.array_equal(as_int(o["it_" + k]), as_int(rld["it_" + k])), k + " (long double)"
    keys = tuple("it_" + s for s in gc.STATE_KEYS) + gc.float_keys(kind)
    e_oracle = {k: cases.rel_err(o[k], rld[k].astype(np.float64)) for k in keys}
    print(f"e_oracle {family} {variant} {kind}:", {k: f"{v:.1e}" for k, v in e_oracle.items()})
    for k in keys:
        assert e_oracle[k] <= gc.E_ORACLE[family][gc.group_of(k)], f"{k}: e_oracle {e_oracle[k]:.2e} above its record"
        e = cases.rel_err(r64[k], o[k])
        assert e <= gc.tol64(family, k), f"{k}: {e:.2e}"
    # the inputs are well defined for the reference arithmetic: finite everywhere, optical depths not negative, sources positive
    for k in gc.float_keys(kind):
        assert np.isfinite(r64[k]).all(), k
    assert (r64["tau"] >= 0).all()
    if kind == "lw":
        assert min(r64[k].min() for k in ("lay_src", "lev_src", "sfc_src", "pfrac", "blay", "blev")) > 0
    else:
        assert r64["tau_ray"].min() > 0 and r64["ssa"].min() >= 0 and r64["ssa"].max() <= 1


@pytest.mark.parametrize("kind", ["lw", "sw"])
@pytest.mark.parametrize("family", ["regular", "irregular", "edges"])
def test_reference_matches_oracle_fp32(family, kind, oracle_f64, oracle_f32):
    """The fp32 oracle against the fp64 reference on the same float32 inputs: e_oracle32. Integer indices are equal wherever the
    cell is 1e-4 of a spacing clear of the nodes (and everywhere on them)."""
    kd, atm, col_dry, col_gas, clear = gc.family_case(oracle_f64, family, kind, NCOL, NLAY, np.float32)
    r = gc.reference_outputs(kd.astype(np.float32), atm, col_dry, col_gas, np.float64, work=np.float32)
    o = gc.shaped_route(oracle_f32, kd, atm, col_dry, col_gas)
    assert clear.mean() > 0.95
    for k in gc.INT_KEYS:
        a, b = as_int(o["it_" + k]), as_int(r["it_" + k])
        assert not ((a != b) & (clear if a.ndim == 2 else clear[None, :, :, None])).any(), k
    keys = tuple("it_" + s for s in gc.STATE_KEYS) + gc.float_keys(kind)
    e32 = {k: cases.rel_err(o[k], r[k], floor=1e-2) for k in keys}
    print(f"e_oracle32 {family} {kind}:", {k: f"{v:.1e}" for k, v in e32.items()})
    for k in keys:
        assert e32[k] <= gc.E_ORACLE32[family][gc.group_of(k)], f"{k}: e_oracle32 {e32[k]:.2e} above its record"


def test_irregular_kdist_has_what_it_is_for():
    for kind in ("lw", "sw"):
        runs = {v: gc.chunk_runs(gc.irregular_kdist(kind, variant=v)) for v in gc.VARIANTS}
        kd = gc.irregular_kdist(kind, variant="whole")
        ncmax = (kd.ngpt + gc.GCH - 1) // gc.GCH + kd.nbnd
        assert kd.ngpt == 77 and kd.ngpt % 16 != 0 and 1 in gc.SIZES and max(gc.SIZES) > 16
        assert all(runs[v] <= ncmax for v in ("fits", "whole", "span", "many")) and runs["cuts"] > ncmax, (runs, ncmax)
        assert runs["fits"] > (kd.ngpt + 15) // 16 + 2, "band-aligned chunks, not the regular cut"
        for sfx in ("lower", "upper"):
            lims = getattr(kd, "minor_limits_gpt_" + sfx)
            n = lims[:, 1] - lims[:, 0] + 1
            bands = kd.gpoint_bands[lims[:, 1] - 1] - kd.gpoint_bands[lims[:, 0] - 1]
            assert (n == 1).any() and (bands == 1).any() and (bands == 0).any()
        assert (kd.minor_limits_gpt_upper[:, 1] - kd.minor_limits_gpt_upper[:, 0] + 1 == kd.ngpt).any()       # the whole spectrum
        assert kd.minor_limits_gpt_lower.shape != kd.minor_limits_gpt_upper.shape
        if kind == "lw":
            for ib in range(kd.nbnd):
                s = kd.planck_frac[kd.band_lims_gpt[ib, 0] - 1: kd.band_lims_gpt[ib, 1]].sum(axis=0)
                assert np.allclose(s, 1.0, rtol=0, atol=1e-14)
        same_twice = kd.flavor[:, 0] == kd.flavor[:, 1]
        assert same_twice[kd.gpoint_flavor - 1].any()
        many = gc.irregular_kdist(kind, variant="many")
        lims = many.minor_limits_gpt_lower
        assert max(int(((lims[:, 0] <= g + 1) & (lims[:, 1] >= g + 1)).sum()) for g in range(many.ngpt)) == 13


def test_edge_atmosphere_leaves_the_tables(oracle_f64):
    kd, atm, col_dry, col_gas, _ = gc.family_case(oracle_f64, "edges", "lw", 70, 30)
    pos = ref.positions(kd, atm.p_lay, atm.t_lay, col_gas)
    it = ref.interpolation(kd, atm.p_lay, atm.t_lay, col_gas)
    fpress = pos["press"] - it["jpress"]
    ftemp = pos["temp"] - it["jtemp"]
    assert fpress.min() < -0.5 and fpress.max() > 1.3, "pressures beyond both ends of press_ref"
    assert fpress.min() > -2 and fpress.max() < 3 and ftemp.min() > -2 and ftemp.max() < 3, "within two spacings"
    assert ftemp.min() < -0.5 and ftemp.max() > 1.3, "temperatures beyond both ends of temp_ref"
    assert (gc.node_distance(pos["temp"]) == 0).sum() >= 10, "cells exactly on a temperature node"
    end = kd.temp_ref_min + (kd.nPlanckTemp - 1) * kd.totplnk_delta
    ts = atm.t_sfc
    assert ((ts < end) & (ts + 1 > end)).any() and (ts > end).any() and (ts < kd.temp_ref_min).any() and (atm.t_lev > end).any()
    eta = pos["eta"] / (kd.neta - 1)
    assert (eta == 0).any() and (eta == 1).any() and (it["col_mix"] == 0).any()
    o3 = atm.vmr["o3"][-1]
    sw = o3[1:][o3[:-1] > 0] / o3[:-1][o3[:-1] > 0]
    assert sw.max() > 1e2 and 0 < sw[sw > 0].min() < 1e-2, "a key species swings between neighbouring columns"


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_by_band_combination_matches_oracle(dtype, oracle_f64):
    kd = gc.irregular_kdist("sw")
    rng = np.random.default_rng(3)
    shp, bshp = (kd.ngpt, 5, 9), (kd.nbnd, 5, 9)
    tau, ssa, g = 10.0 ** rng.uniform(-6, 1, shp), rng.uniform(0, 1, shp), np.zeros(shp)
    ct, cw, cg = np.where(rng.random(bshp) < 0.4, 0.0, 10.0 ** rng.uniform(-3, 1, bshp)), rng.uniform(0, 1, bshp), rng.uniform(0, 0.9, bshp)
    t1 = tau.copy(); oracle_f64.inc_1scalar_by_1scalar_bybnd(t1, ct, kd.band_lims_gpt)
    assert cases.rel_err(ref.add_by_band_1scalar(kd, tau, ct, dtype).astype(np.float64), t1) <= 1e-15
    t2, w2, g2 = tau.copy(), ssa.copy(), g.copy()
    oracle_f64.inc_2stream_by_2stream_bybnd(t2, w2, g2, ct, cw, cg, kd.band_lims_gpt)
    for a, b in zip(ref.add_by_band_2stream(kd, tau, ssa, g, ct, cw, cg, dtype), (t2, w2, g2)):
        assert cases.rel_err(a.astype(np.float64), b) <= 1e-14
