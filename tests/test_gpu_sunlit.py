"""GPU tests of sunlit-only SW: the column list (rrx_sunlit_columns) against numpy, the zero-filling scatter, and
pipeline.ResidentSolver(sunlit=True) / the C++ solvers (set_sunlit_columns, --sunlit-columns) on atmospheres with night columns:
exact zeros in the dark, the plain solve of the day-only sub-atmosphere and the CPU oracle in the light, LW untouched."""

import numpy as np
import pytest

import cases
from rte_rrtmgp_cpp_amd import synthetic, pipeline

pytestmark = pytest.mark.gpu
KW = dict(ngpt=48, nbnd=4, npres=16, nflav=4, nminor_lower=7, nminor_upper=4)
SW_ROWS = slice(3, 7)


# ---- the column list and the scatter ----------------------------------------------------------------------------------------------
def _mu0_cases(ncol, rng):
    mixed = rng.uniform(-1.0, 1.0, ncol)
    for n, val in ((ncol // 5, 0.0), (ncol // 10, -0.0), (min(7, ncol), 1e-30), (min(3, ncol // 2), np.nan)):
        mixed[rng.choice(ncol, n, replace=False)] = val
    single = np.zeros(ncol); single[ncol // 3] = 0.25
    return {"all_day": rng.uniform(0.01, 1.0, ncol), "all_night": -rng.uniform(0.0, 1.0, ncol), "single": single, "mixed": mixed}


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ncol", [1, 200, 16385])
@pytest.mark.parametrize("with_order", [False, True])
@pytest.mark.parametrize("pad_to", [1, 16])
def test_sunlit_columns_matches_numpy(dt, ncol, with_order, pad_to, hip_f64, hip_f32):
    be = hip_f64 if dt == "f64" else hip_f32
    rng = np.random.default_rng(ncol + 7*pad_to + with_order)
    order = rng.permutation(ncol).astype(np.int32) if with_order else None
    for name, mu0 in _mu0_cases(ncol, rng).items():
        mu0 = mu0.astype(be.np_dtype)
        o = np.arange(ncol) if order is None else order
        want = o[np.flatnonzero(mu0[o] > 0)]
        perm, count = be.sunlit_columns(be.asarray(mu0), None if order is None else be.asarray(order), pad_to)
        n = int(be.to_numpy(count)[0])
        p = be.to_numpy(perm)
        assert n == want.size, (name, n, want.size)
        assert np.array_equal(p[:n], want), name
        n_out = -(-n // pad_to) * pad_to
        assert np.all(p[n:n_out] == (want[-1] if n else 0)), name


@pytest.mark.parametrize("layout", ["col_n2", "col_nlev_nbnd", "packed7", "packed_bnd"])
def test_scatter_cols_fill(layout, hip_f64):
    """Zeros in every column not listed, the listed ones scattered: (col, n2), (col, nlev, nbnd) and ResidentSolver's packed
    (k, nlev, col) / (k, nbnd, nlev, col) buffers -- all column-fastest in memory."""
    be = hip_f64
    ncol = 301
    lead = {"col_n2": (9,), "col_nlev_nbnd": (3, 9), "packed7": (4, 9), "packed_bnd": (4, 3, 9)}[layout]
    rng = np.random.default_rng(3)
    keep = np.sort(rng.choice(ncol, 170, replace=False)).astype(np.int32)
    n_out = 176
    perm = np.concatenate([keep, np.full(n_out - keep.size, keep[-1], np.int32)])
    src = rng.uniform(1.0, 2.0, lead + (n_out,))
    dst = be.asarray(np.full(lead + (ncol,), np.nan))
    be.scatter_cols_fill(keep.size, be.asarray(perm), be.asarray(src), dst)
    want = np.zeros(lead + (ncol,))
    want[..., keep] = src[..., :keep.size]
    got = be.to_numpy(dst)
    assert np.array_equal(got, want)
    assert not np.signbit(got).any()
    be.scatter_cols_fill(0, be.asarray(perm), be.asarray(src[..., :0].copy()), dst)
    assert np.array_equal(be.to_numpy(dst), np.zeros_like(want))


# ---- ResidentSolver ------------------------------------------------------------------------------------------------------------------
def _night(atm0, frac, seed):
    """about `frac` of the columns at random in the dark: half of them at mu0 = 0 (one in four at -0.0), half below the horizon"""
    rng = np.random.default_rng(seed)
    ncol = atm0.ncol
    mu0 = rng.uniform(0.1, 1.0, ncol)
    dark = rng.choice(ncol, int(round(frac * ncol)), replace=False)
    h = dark.size // 2
    mu0[dark[:h]] = 0.0
    mu0[dark[:h:4]] = -0.0
    mu0[dark[h:]] = -rng.uniform(0.0, 1.0, dark.size - h)
    atm0.mu0 = np.ascontiguousarray(mu0.astype(atm0.p_lay.dtype))
    return atm0


def _subset(atm0, idx):
    """the numpy atmosphere of columns idx"""
    out = {}
    for k, v in atm0.__dict__.items():
        if k == "ncol":
            out[k] = int(idx.size)
        elif k in pipeline.ResidentSolver._COLUMN_FIELDS and v is not None:
            out[k] = np.ascontiguousarray(np.take(v, idx, axis=v.ndim - 1 if pipeline.ResidentSolver._COLUMN_FIELDS[k] < 0 else 0))
        elif isinstance(v, dict):
            out[k] = {n: (np.ascontiguousarray(a[:, idx]) if a.ndim == 2 else a) for n, a in v.items()}
        else:
            out[k] = v
    return synthetic.Atmosphere(**out)


def _case(be, ncol, nlay, clouds=False, spread=False, frac=0.4, seed=11):
    atm0 = synthetic.make_atmosphere(ncol, nlay, nbnd_lw=KW["nbnd"], nbnd_sw=KW["nbnd"], seed=seed, clouds=clouds)
    if spread:                           # surface pressures far apart: sorting has work to do
        f = np.random.default_rng(seed + 1).uniform(0.65, 1.35, ncol)
        atm0.p_lay = np.ascontiguousarray(atm0.p_lay * f); atm0.p_lev = np.ascontiguousarray(atm0.p_lev * f)
    atm0 = _night(atm0.astype(be.np_dtype), frac, seed + 2)
    kl0, ks0 = synthetic.make_kdist("lw", **KW), synthetic.make_kdist("sw", **KW)
    luts0 = (synthetic.make_cloud_lut(KW["nbnd"], "lw"), synthetic.make_cloud_lut(KW["nbnd"], "sw")) if clouds else None
    return atm0, kl0, ks0, luts0


def _solve(be, atm0, kl0, ks0, luts0, **kw):
    luts = tuple(be.upload_lut(l) for l in luts0) if luts0 is not None else None
    sv = pipeline.ResidentSolver(be, be.upload_kdist(kl0), be.upload_kdist(ks0), pipeline.upload_atmosphere(be, atm0),
                                 do_broadband=True, cloud_luts=luts, **kw)
    F = be.to_numpy(sv.step()).copy()
    B = {k: be.to_numpy(v).copy() for k, v in sv.bnd_fluxes.items()} if sv.bnd_fluxes is not None else None
    return sv, F, B


VARIANTS = {
    "f64":         dict(dt="f64"),
    "f64_overlap": dict(dt="f64", overlap=True),
    "byband":      dict(dt="f64", byband=True),
    "allsky":      dict(dt="f64", clouds=True),
    "f32":         dict(dt="f32"),
    "sorted":      dict(dt="f64", spread=True, sort="1"),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_resident_solver_sunlit_mixed(variant, hip_f64, hip_f32, monkeypatch):
    """1 000 columns (padded to 1 008), 40 % of them dark: SW exactly zero there, the day columns as the plain solve of the day-only
    sub-atmosphere, LW bit for bit as sunlit=False."""
    v = VARIANTS[variant]
    be = hip_f64 if v["dt"] == "f64" else hip_f32
    monkeypatch.setenv("RRX_PAD_COLUMNS", "1")
    ncol, nlay = 1000, 40
    atm0, kl0, ks0, luts0 = _case(be, ncol, nlay, clouds=v.get("clouds", False), spread=v.get("spread", False))
    kw = dict(byband=v.get("byband", False), overlap=v.get("overlap", False), sort_columns=v.get("sort", "0"))
    _, ref, ref_b = _solve(be, atm0, kl0, ks0, luts0, **kw)
    sv, got, got_b = _solve(be, atm0, kl0, ks0, luts0, sunlit=True, **kw)
    assert sv.npad == 8 and sv.sort_columns == (kw["sort_columns"] == "1")
    day = np.flatnonzero(atm0.mu0 > 0)
    night = np.flatnonzero(~(atm0.mu0 > 0))
    assert 350 <= night.size <= 450
    assert np.array_equal(got[:3], ref[:3]), "LW must not change"
    assert np.all(got[SW_ROWS][..., night] == 0.0) and not np.signbit(got[SW_ROWS][..., night]).any()
    assert np.isfinite(got).all()
    _, sub, sub_b = _solve(be, _subset(atm0, day), kl0, ks0, luts0, byband=kw["byband"], sort_columns="0")
    tol, floor = (1e-12, 1e-6) if v["dt"] == "f64" else (1e-4, 1e-2)
    assert cases.rel_err(got[SW_ROWS][..., day], sub[SW_ROWS], floor=floor) <= tol
    if kw["byband"]:
        assert set(got_b) == set(ref_b)
        for k in got_b:
            if k.startswith("lw"):
                assert np.array_equal(got_b[k], ref_b[k]), k
            else:
                assert np.all(got_b[k][..., night] == 0.0), k
                assert cases.rel_err(got_b[k][..., day], sub_b[k], floor=floor) <= tol, k


def test_resident_solver_sunlit_day_columns_match_oracle(hip_f64, oracle_f64):
    """The day columns of a mixed 300-column atmosphere against the CPU oracle's SW solve of those columns (1e-7, the SW tolerance of
    the parity tests)."""
    be, orc = hip_f64, oracle_f64
    atm0, kl0, ks0, _ = _case(be, 300, 30, seed=21)
    _, got, _ = _solve(be, atm0, kl0, ks0, None, sunlit=True)
    day = np.flatnonzero(atm0.mu0 > 0)
    o = pipeline.solve_sw(orc, orc.upload_kdist(ks0), pipeline.upload_atmosphere(orc, _subset(atm0, day)))
    for i, k in zip(range(3, 7), ("flux_up", "flux_dn", "flux_dn_dir", "flux_net")):
        assert cases.rel_err(got[i][:, day], orc.to_numpy(o[k])) <= 1e-7, k


@pytest.mark.parametrize("sort", ["0", "1"])
def test_resident_solver_all_sunlit_is_bit_identical(sort, hip_f64, monkeypatch):
    be = hip_f64
    monkeypatch.setenv("RRX_PAD_COLUMNS", "1")
    atm0, kl0, ks0, _ = _case(be, 1000, 40, spread=True, frac=0.0)
    assert (atm0.mu0 > 0).all()
    _, ref, _ = _solve(be, atm0, kl0, ks0, None, sort_columns=sort)
    sv, got, _ = _solve(be, atm0, kl0, ks0, None, sunlit=True, sort_columns=sort)
    assert np.array_equal(got, ref)
    assert np.array_equal(be.to_numpy(sv.step()), ref), "a second step must reproduce the first"


def test_resident_solver_all_dark_gives_zero_sw(hip_f64):
    be = hip_f64
    atm0, kl0, ks0, _ = _case(be, 200, 30, frac=1.0)
    _, ref, _ = _solve(be, atm0, kl0, ks0, None, byband=True)
    sv, got, _ = _solve(be, atm0, kl0, ks0, None, sunlit=True, byband=True)
    assert np.array_equal(got[:3], ref[:3])
    assert np.all(got[SW_ROWS] == 0.0)
    for k, b in sv.bnd_fluxes.items():
        if k.startswith("sw"):
            assert np.all(be.to_numpy(b) == 0.0), k


# ---- C++ solvers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clouds", [False, True], ids=["clear", "allsky"])
def test_cxx_driver_sunlit_columns_matches_pipeline(clouds, hip_f64):
    """set_sunlit_columns(true) with a column block of 1 000 on 2 500 columns with a pressure spread (sorted and padded on the device)
    against ResidentSolver(sunlit=True): zeros in the dark, the solve of the plain path elsewhere."""
    from rte_rrtmgp_cpp_amd import cxx_driver
    be = hip_f64
    atm0, kl0, ks0, luts0 = _case(be, 2500, 30, clouds=clouds, spread=True, seed=31)
    _, ref, _ = _solve(be, atm0, kl0, ks0, luts0, sunlit=True)
    drv = cxx_driver.CxxDriver(be, kl0, ks0, pipeline.upload_atmosphere(be, atm0), luts0, column_block=1000, sunlit=True)
    try:
        got = be.to_numpy(drv.step()).copy()
    finally:
        drv.close()
    night = np.flatnonzero(~(atm0.mu0 > 0))
    assert np.all(got[SW_ROWS][..., night] == 0.0) and np.isfinite(got).all()
    assert cases.rel_err(got[:3], ref[:3]) <= 1e-11 and cases.rel_err(got[3:], ref[3:]) <= 1e-7


def test_rfmip_style_night_sites_match_oracle_on_sunlit_sites(hip_f64, oracle_f64):
    """RFMIP's mu0 = max(0, cos(sza)) (night sites at exactly 0) through the C++ solvers with --sunlit-columns: finite fluxes, zero
    SW at night, the oracle on the sunlit sites."""
    from rte_rrtmgp_cpp_amd import cxx_driver
    be, orc = hip_f64, oracle_f64
    ncol = 100
    atm0, kl0, ks0, _ = _case(be, ncol, 30, seed=41)
    sza = np.random.default_rng(42).uniform(0.0, 180.0, ncol)
    atm0.mu0 = np.ascontiguousarray(np.maximum(0.0, np.cos(np.deg2rad(sza))))
    drv = cxx_driver.CxxDriver(be, kl0, ks0, pipeline.upload_atmosphere(be, atm0), None, sunlit=True)
    try:
        got = be.to_numpy(drv.step()).copy()
    finally:
        drv.close()
    assert np.isfinite(got).all()
    day = np.flatnonzero(atm0.mu0 > 0)
    assert 0 < day.size < ncol
    night = np.setdiff1d(np.arange(ncol), day)
    assert np.all(got[SW_ROWS][..., night] == 0.0)
    o = pipeline.solve_sw(orc, orc.upload_kdist(ks0), pipeline.upload_atmosphere(orc, _subset(atm0, day)))
    for i, k in zip(range(3, 7), ("flux_up", "flux_dn", "flux_dn_dir", "flux_net")):
        assert cases.rel_err(got[i][:, day], orc.to_numpy(o[k])) <= 1e-7, k
