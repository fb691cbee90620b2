"""GPU tests of the McICA cloud sampling (csrc/rrx_mcica.hip): the three entries against the numpy restatement
(tests/mcica_ref.py) bit for bit, the column identities through permutations and splits, pipeline.ResidentSolver(cloud_fraction=...)
against today's all-sky route where the fractions are 0 or 1, the bracketing of a half-cloudy solve, the refused pairs, and the C++
classes and driver against ResidentSolver."""
import os

import numpy as np
import pytest

import cases
from host_driver import run_driver
import mcica_ref as M
from rte_rrtmgp_cpp_amd import synthetic, synthetic_files, rrxio, pipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789abcdef

# (ncol, nlay, ngpt, band limits): more than one row of 64 lanes with an incomplete last one, an incomplete last group of four
# layers and a one-g-point band; the smallest problem; an empty band
GRIDS = {"70x11x16": (70, 11, 16, [[1, 5], [6, 6], [7, 16]]),
         "1x1x1": (1, 1, 1, [[1, 1]]),
         "16x9x8_empty_band": (16, 9, 8, [[1, 3], [4, 3], [4, 8]])}
PROFILES = ("blocks", "ends", "clear", "overcast", "random")


def cloud_fraction(profile, ncol, nlay, dtype):
    f = np.zeros((nlay, ncol))
    if profile == "blocks":            # 0.3 / 0.6 / 0.45 in layers 2-4, 0.5 in layer 7, 1 in layer 10 (those the grid has)
        for ilay, v in ((2, 0.3), (3, 0.6), (4, 0.45), (7, 0.5), (10, 1.0)):
            if ilay < nlay:
                f[ilay] = v
        if nlay == 1:
            f[0] = 0.5
    elif profile == "ends":            # cloud in the first and in the last array layer
        f[0] = 0.4; f[-1] = 0.7
    elif profile == "overcast":
        f[:] = 1.0
    elif profile == "random":          # every column its own profile, clear layers among them
        rng = np.random.default_rng(17)
        f = rng.uniform(0.0, 1.0, (nlay, ncol)) * (rng.uniform(0.0, 1.0, (nlay, ncol)) > 0.35)
    return np.ascontiguousarray(f.astype(dtype))


def overlap_parameter(ncol, nlay, dtype):
    rng = np.random.default_rng(23)
    a = rng.uniform(0.0, 1.0, (max(nlay-1, 0), ncol))
    a[rng.uniform(0.0, 1.0, a.shape) < 0.1] = 0.0
    a[rng.uniform(0.0, 1.0, a.shape) < 0.1] = 1.0
    return np.ascontiguousarray(a.astype(dtype))


def column_ids(mode, ncol):
    """(col_id array or None, col_id0, the identities)"""
    if mode == "col_id0":
        return None, 5, np.arange(ncol) + 5
    ids = (np.random.default_rng(29).permutation(4*ncol)[:ncol] + 3).astype(np.int32)
    return ids, 0, ids


def optical_inputs(ncol, nlay, ngpt, nbnd, dtype, seed=31):
    rng = np.random.default_rng(seed)
    g3 = lambda lo, hi, n: np.ascontiguousarray(rng.uniform(lo, hi, (n, nlay, ncol)).astype(dtype))
    return dict(tau=g3(0.01, 3.0, ngpt), ssa=g3(0.0, 1.0, ngpt), g=g3(-0.2, 0.9, ngpt),
                ctau=g3(0.0, 20.0, nbnd), cssa=g3(0.0, 1.0, nbnd), cg=g3(0.0, 0.95, nbnd))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("ids", ["col_id", "col_id0"])
@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_entries_match_the_numpy_restatement(grid, profile, dt, overlap, ids, hip_f64, hip_f32):
    be = hip_f64 if dt == "f64" else hip_f32
    ncol, nlay, ngpt, lims = GRIDS[grid]
    lims = np.array(lims, dtype=np.int32)
    cf = cloud_fraction(profile, ncol, nlay, be.np_dtype)
    al = overlap_parameter(ncol, nlay, be.np_dtype) if overlap == "exp_ran" else None
    cid, cid0, idents = column_ids(ids, ncol)
    x = optical_inputs(ncol, nlay, ngpt, lims.shape[0], be.np_dtype)
    A = be.asarray
    kw = dict(alpha=None if al is None else A(al), col_id=None if cid is None else A(cid), col_id0=cid0)
    d_lims, d_cf = A(lims), A(cf)
    for domain in (0, 1):
        want = M.cloud_mask(cf, al, SEED, domain, idents, ngpt)
        if profile == "clear":
            assert not want.any()
        if profile == "overcast":
            assert want.all()
        hit = M.sampled_mask(want, lims)

        # the mask alone
        got = be.mcica_cloud_mask(ngpt, d_cf, seed=SEED, domain=domain, **kw)
        assert np.array_equal(be.to_numpy(got), want), "rrx_mcica_cloud_mask"

        # one scalar: cloudy cells tau + cld_tau, every other cell the input, bit for bit
        tau = A(x["tau"].copy())
        mask = be.mcica_increment_1scalar(tau, A(x["ctau"]), d_lims, d_cf, seed=SEED, domain=domain, mask=True, **kw)
        assert np.array_equal(be.to_numpy(mask), want), "rrx_mcica_increment_1scalar mask"
        t1 = be.to_numpy(tau)
        assert same_bits(t1, M.increment_1scalar(x["tau"], x["ctau"], want, lims))
        assert same_bits(t1[~hit], x["tau"][~hit])
        tau_nomask = A(x["tau"].copy())
        assert be.mcica_increment_1scalar(tau_nomask, A(x["ctau"]), d_lims, d_cf, seed=SEED, domain=domain, **kw) is None
        assert same_bits(be.to_numpy(tau_nomask), t1), "mask_out = NULL must not change the increment"

        # two-stream: cloudy cells as rrx_increment_2stream_by_2stream on g-point cloud arrays built in numpy, the others the input
        t, w, g = A(x["tau"].copy()), A(x["ssa"].copy()), A(x["g"].copy())
        mask = be.mcica_increment_2stream(t, w, g, A(x["ctau"]), A(x["cssa"]), A(x["cg"]), d_lims, d_cf, seed=SEED, domain=domain,
                                          mask=True, **kw)
        assert np.array_equal(be.to_numpy(mask), want), "rrx_mcica_increment_2stream mask"
        rt, rw, rg = A(x["tau"].copy()), A(x["ssa"].copy()), A(x["g"].copy())
        be.increment_2stream_by_2stream(rt, rw, rg, *(A(M.expand_bands(x[k], lims, ngpt)) for k in ("ctau", "cssa", "cg")))
        for name, got_a, ref_a, inp in (("tau", t, rt, x["tau"]), ("ssa", w, rw, x["ssa"]), ("g", g, rg, x["g"])):
            got_a, ref_a = be.to_numpy(got_a), be.to_numpy(ref_a)
            assert same_bits(got_a[hit], ref_a[hit]), name
            assert same_bits(got_a[~hit], inp[~hit]), name


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
def test_column_identity_survives_permutation_and_splitting(overlap, dt, hip_f64, hip_f32):
    be = hip_f64 if dt == "f64" else hip_f32
    ncol, nlay, ngpt, lims = GRIDS["70x11x16"]
    lims = np.array(lims, dtype=np.int32)
    A, N = be.asarray, be.to_numpy
    cf = cloud_fraction("random", ncol, nlay, be.np_dtype)
    al = overlap_parameter(ncol, nlay, be.np_dtype) if overlap == "exp_ran" else None
    x = optical_inputs(ncol, nlay, ngpt, 3, be.np_dtype)
    C = lambda a, idx: np.ascontiguousarray(a[..., idx])

    def run(idx, col_id, col_id0):
        """the sampled two-stream increment and mask of the columns idx, in that order"""
        t, w, g = (A(C(x[k], idx)) for k in ("tau", "ssa", "g"))
        m = be.mcica_increment_2stream(t, w, g, *(A(C(x[k], idx)) for k in ("ctau", "cssa", "cg")), A(lims), A(C(cf, idx)),
                                       alpha=None if al is None else A(C(al, idx)), seed=SEED, domain=1,
                                       col_id=None if col_id is None else A(col_id.astype(np.int32)), col_id0=col_id0, mask=True)
        t1 = A(C(x["tau"], idx))
        be.mcica_increment_1scalar(t1, A(C(x["ctau"], idx)), A(lims), A(C(cf, idx)), alpha=None if al is None else A(C(al, idx)),
                                   seed=SEED, domain=1, col_id=None if col_id is None else A(col_id.astype(np.int32)), col_id0=col_id0)
        return [N(a) for a in (t, w, g, m, t1)]

    every = np.arange(ncol)
    ref = run(every, None, 5)
    assert ref[3].any() and not ref[3].all()
    perm = np.random.default_rng(5).permutation(ncol)
    got = run(perm, perm + 5, 0)
    for a, b in zip(got, ref):
        back = np.empty_like(a); back[..., perm] = a
        assert same_bits(back, b)
    lo, hi = run(every[:33], None, 5), run(every[33:], None, 5 + 33)
    for a, b, c in zip(lo, hi, ref):
        assert same_bits(np.concatenate([a, b], axis=-1), c)


# ---- ResidentSolver --------------------------------------------------------------------------------------------------------------------
KW = dict(ngpt=48, nbnd=4, npres=16, nflav=4, nminor_lower=7, nminor_upper=4)
NCOL, NLAY = 17, 30


@pytest.fixture(scope="module")
def chain_case():
    """A small all-sky case with pressures far apart (sorting has work to do) and cloud fractions of 0 or 1: lwp = iwp = 0 wherever
    the fraction is 0. frac_half: fraction 0.5 wherever there is cloud."""
    atm = synthetic.make_atmosphere(NCOL, NLAY, nbnd_lw=KW["nbnd"], nbnd_sw=KW["nbnd"], seed=11, clouds=True)
    f = np.random.default_rng(12).uniform(0.65, 1.35, NCOL)
    atm.p_lay = np.ascontiguousarray(atm.p_lay * f); atm.p_lev = np.ascontiguousarray(atm.p_lev * f)
    cloudy = (atm.lwp + atm.iwp) > 0
    keep = cloudy & (np.random.default_rng(13).uniform(0.0, 1.0, cloudy.shape) < 0.7)
    assert keep.any() and (cloudy & ~keep).any()
    for k in ("lwp", "iwp", "rel", "dei"):
        setattr(atm, k, np.ascontiguousarray(np.where(keep, getattr(atm, k), 0.0)))
    frac01 = np.ascontiguousarray(keep.astype(np.float64))
    # (a fraction of 1 in some cells without condensate as well: they add a cloud of zero optical depth, as the all-sky route does)
    frac01[(np.random.default_rng(14).uniform(0.0, 1.0, keep.shape) < 0.1) & ~cloudy] = 1.0
    return dict(atm=atm, kl=synthetic.make_kdist("lw", **KW), ks=synthetic.make_kdist("sw", **KW),
                luts=(synthetic.make_cloud_lut(KW["nbnd"], "lw"), synthetic.make_cloud_lut(KW["nbnd"], "sw")),
                frac01=frac01, frac_half=np.ascontiguousarray(0.5 * keep))


def solver(be, case, clouds=True, frac=None, **kw):
    luts = tuple(be.upload_lut(l) for l in case["luts"]) if clouds else None
    if frac is not None:
        kw["cloud_fraction"] = be.asarray(np.ascontiguousarray(frac.astype(be.np_dtype)))
    kw.setdefault("sort_columns", "0")
    return pipeline.ResidentSolver(be, be.upload_kdist(case["kl"]), be.upload_kdist(case["ks"]),
                                   pipeline.upload_atmosphere(be, case["atm"].astype(be.np_dtype)), do_broadband=True, cloud_luts=luts, **kw)


def solve(be, case, **kw):
    return be.to_numpy(solver(be, case, **kw).step()).copy()


def lw_sw_err(got, ref, floor=1e-6):
    return cases.rel_err(got[:3], ref[:3], floor=floor), cases.rel_err(got[3:], ref[3:], floor=floor)


def test_chain_fractions_of_0_or_1_match_the_allsky_route_f64(chain_case, hip_f64, monkeypatch):
    """Fractions in {0, 1}: the sampled chain against today's all-sky chain. LW to 1e-11 (routes of the same arithmetic), SW to 1e-7
    (the SW bound: the all-sky route increments clear cells by zero, which moves ssa and g by an ulp; the sampled one leaves them)."""
    be = hip_f64
    monkeypatch.setenv("RRX_PAD_COLUMNS", "1")
    ref = solve(be, chain_case)
    got = solve(be, chain_case, frac=chain_case["frac01"], mcica_seed=SEED)
    e_lw, e_sw = lw_sw_err(got, ref)
    print(f"fp64 sampled vs all-sky: LW {e_lw:.2e} SW {e_sw:.2e}")
    assert e_lw <= 1e-11 and e_sw <= 1e-7
    # exponential-random overlap, another seed and an offset draw the same mask from fractions of 0 or 1
    al = be.asarray(np.full((NLAY-1, NCOL), 0.5))
    got2 = solve(be, chain_case, frac=chain_case["frac01"], cloud_overlap="exp_ran", overlap_param=al, mcica_seed=3, mcica_col_offset=1000)
    assert np.array_equal(got2, got)
    # sorted (forced) and padded to 32 columns against the caller's order
    sv = solver(be, chain_case, frac=chain_case["frac01"], mcica_seed=SEED, sort_columns="1")
    assert sv.sort_columns and sv.npad == 15 and not np.array_equal(be.to_numpy(sv.perm[:NCOL]), np.arange(NCOL))
    e_lw, e_sw = lw_sw_err(be.to_numpy(sv.step()), got)
    print(f"fp64 sampled, sorted and padded vs unsorted: LW {e_lw:.2e} SW {e_sw:.2e}")
    assert e_lw <= 1e-11 and e_sw <= 1e-7


# fp32, sampled against all-sky, fractions in {0, 1} (cases.rel_err with the fp32 floor of 1e-2): twice the largest error observed on
# the MI355X (DESIGN 8's rule). Observed: LW 0.0 -- the same bits, tau + 0 is exact and the fused all-sky gas optics adds the band
# cloud with the increment's arithmetic -- and SW 4.699e-06 (the all-sky route's increment by zero moves ssa and g by an ulp in the
# clear cells, the sampled route leaves them), unsorted and sorted-and-padded alike.
F32_LW_BOUND = 0.0
F32_SW_BOUND = 9.4e-6


def test_chain_fractions_of_0_or_1_match_the_allsky_route_f32(chain_case, hip_f32, monkeypatch):
    be = hip_f32
    monkeypatch.setenv("RRX_PAD_COLUMNS", "1")
    ref = solve(be, chain_case)
    got = solve(be, chain_case, frac=chain_case["frac01"], mcica_seed=SEED)
    e_lw, e_sw = lw_sw_err(got, ref, floor=1e-2)
    print(f"fp32 sampled vs all-sky: LW {e_lw:.3e} SW {e_sw:.3e}")
    got_s = solve(be, chain_case, frac=chain_case["frac01"], mcica_seed=SEED, sort_columns="1")
    s_lw, s_sw = lw_sw_err(got_s, ref, floor=1e-2)
    print(f"fp32 sampled, sorted and padded vs all-sky: LW {s_lw:.3e} SW {s_sw:.3e}")
    assert max(e_lw, s_lw) <= F32_LW_BOUND and max(e_sw, s_sw) <= F32_SW_BOUND


@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
def test_chain_fractional_cloud_keeps_its_subcolumns_when_sorted_and_padded(overlap, chain_case, hip_f64, monkeypatch):
    """Fraction 0.5: the sub-columns are drawn by column identity, so the sorted and padded step solves the same sub-columns as the
    step in the caller's order (the bounds of routes of the same arithmetic), and another seed or offset solves other ones."""
    be = hip_f64
    monkeypatch.setenv("RRX_PAD_COLUMNS", "1")
    kw = dict(frac=chain_case["frac_half"], mcica_seed=SEED, mcica_col_offset=40)
    if overlap == "exp_ran":
        kw.update(cloud_overlap="exp_ran", overlap_param=be.asarray(overlap_parameter(NCOL, NLAY, np.float64)))
    plain = solve(be, chain_case, **kw)
    sv = solver(be, chain_case, sort_columns="1", **kw)
    assert sv.npad == 15
    e_lw, e_sw = lw_sw_err(be.to_numpy(sv.step()), plain)
    assert e_lw <= 1e-11 and e_sw <= 1e-7
    assert np.array_equal(be.to_numpy(sv.step()), be.to_numpy(sv.step()).copy()), "the same seed draws the same mask"
    first = be.to_numpy(sv.step()).copy()
    sv.mcica_seed += 1                           # a host advances the seed between calls
    assert not np.array_equal(be.to_numpy(sv.step()), first)
    assert not np.array_equal(solve(be, chain_case, **dict(kw, mcica_col_offset=41)), plain)


def test_chain_works_with_byband_jacobian_and_angles(chain_case, hip_f64):
    """byband, jacobian, n_gauss_angles and optimal_angles only read the g-point tau: with fractions of 0 or 1 they give what they give
    on the all-sky route."""
    be = hip_f64
    frac = chain_case["frac01"]
    for kw in (dict(byband=True), dict(jacobian=True), dict(n_gauss_angles=3), dict(jacobian=True, n_gauss_angles=2)):
        e_lw, e_sw = lw_sw_err(solve(be, chain_case, frac=frac, **kw), solve(be, chain_case, **kw))
        assert e_lw <= 1e-11 and e_sw <= 1e-7, kw
    a, b = solver(be, chain_case, frac=frac, byband=True), solver(be, chain_case, byband=True)
    a.step(); b.step()
    for k in a.bnd_fluxes:
        assert cases.rel_err(be.to_numpy(a.bnd_fluxes[k]), be.to_numpy(b.bnd_fluxes[k])) <= (1e-11 if k.startswith("lw") else 1e-7), k
    a, b = solver(be, chain_case, frac=frac, jacobian=True), solver(be, chain_case, jacobian=True)
    a.step(); b.step()
    assert cases.rel_err(be.to_numpy(a.lw_flux_up_jac), be.to_numpy(b.lw_flux_up_jac)) <= 1e-11


def test_half_cloudy_surface_flux_lies_between_clear_and_overcast(chain_case, hip_f64):
    be = hip_f64
    overcast = solve(be, chain_case)
    clear = solve(be, chain_case, frac=np.zeros((NLAY, NCOL)))
    assert cases.rel_err(clear[:3], solve(be, chain_case, clouds=False)[:3]) <= 1e-11        # (fraction 0 is the clear-sky solve)
    half = solve(be, chain_case, frac=chain_case["frac_half"], mcica_seed=SEED)
    isfc = 0                                      # (surface first)
    lo, mid, hi = clear[1][isfc], half[1][isfc], overcast[1][isfc]
    slack = 1e-11 * np.abs(hi)
    assert np.all(lo <= hi + slack)
    assert np.all(mid >= lo - slack) and np.all(mid <= hi + slack)
    cloudy_cols = chain_case["frac_half"].any(axis=0)
    assert np.all(mid[cloudy_cols] > lo[cloudy_cols]) and np.all(mid[cloudy_cols] < hi[cloudy_cols])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_resident_solver_refuses_the_pairs_it_cannot_serve(chain_case, hip_f64):
    be = hip_f64
    frac = chain_case["frac01"]
    for kw in (dict(lw_scattering=True), dict(lw_rescaling=True), dict(sunlit=True)):
        with pytest.raises(ValueError, match="cloud_fraction"):
            solver(be, chain_case, frac=frac, **kw)
    with pytest.raises(ValueError, match="cloud_luts"):
        solver(be, chain_case, clouds=False, frac=frac)
    with pytest.raises(ValueError, match="overlap_param"):
        solver(be, chain_case, frac=frac, cloud_overlap="exp_ran")
    with pytest.raises(ValueError, match="overlap_param"):
        solver(be, chain_case, frac=frac, overlap_param=be.asarray(np.ones((NLAY-1, NCOL))))
    with pytest.raises(ValueError, match="cloud_overlap"):
        solver(be, chain_case, frac=frac, cloud_overlap="random")
    with pytest.raises(ValueError, match="cloud_fraction"):
        solver(be, chain_case, frac=frac[:-1])


@pytest.mark.parametrize("pair", ["lw_scattering", "lw_rescaling", "sunlit"])
def test_cxx_solvers_refuse_the_same_pairs(pair, chain_case, hip_f64):
    from rte_rrtmgp_cpp_amd import cxx_driver
    be = hip_f64
    drv = cxx_driver.CxxDriver(be, chain_case["kl"], chain_case["ks"], pipeline.upload_atmosphere(be, chain_case["atm"]), chain_case["luts"],
                               cloud_fraction=be.asarray(chain_case["frac01"]), **{pair: True})
    try:
        with pytest.raises(RuntimeError, match="cloud sampling"):
            drv.step()
    finally:
        drv.close()


# ---- C++ classes and driver ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
def test_cxx_classes_match_resident_solver(overlap, hip_f64):
    """set_cloud_sampling on 300 columns with a pressure spread in column blocks of 128, sorted and padded on the device, against
    ResidentSolver in the caller's order: the column identities follow the blocks and the sort."""
    from rte_rrtmgp_cpp_amd import cxx_driver
    be = hip_f64
    ncol, nlay = 300, 20
    atm = synthetic.make_atmosphere(ncol, nlay, nbnd_lw=KW["nbnd"], nbnd_sw=KW["nbnd"], seed=31, clouds=True)
    f = np.random.default_rng(32).uniform(0.65, 1.35, ncol)
    atm.p_lay = np.ascontiguousarray(atm.p_lay * f); atm.p_lev = np.ascontiguousarray(atm.p_lev * f)
    case = dict(atm=atm, kl=synthetic.make_kdist("lw", **KW), ks=synthetic.make_kdist("sw", **KW),
                luts=(synthetic.make_cloud_lut(KW["nbnd"], "lw"), synthetic.make_cloud_lut(KW["nbnd"], "sw")))
    frac = np.random.default_rng(33).uniform(0.0, 1.0, (nlay, ncol)) * ((atm.lwp + atm.iwp) > 0)
    kw = dict(mcica_seed=SEED, mcica_col_offset=7)
    if overlap == "exp_ran":
        kw.update(cloud_overlap="exp_ran", overlap_param=be.asarray(overlap_parameter(ncol, nlay, np.float64)))
    ref = solve(be, case, frac=frac, **kw)
    assert not np.array_equal(ref, solve(be, case, frac=frac, **dict(kw, mcica_seed=SEED + 1)))
    drv = cxx_driver.CxxDriver(be, case["kl"], case["ks"], pipeline.upload_atmosphere(be, atm), case["luts"], column_block=128, sort_mode=1,
                               cloud_fraction=be.asarray(frac), **kw)
    try:
        got = be.to_numpy(drv.step()).copy()
        drv.mcica_seed = SEED + 1
        other = be.to_numpy(drv.step()).copy()
    finally:
        drv.close()
    e_lw, e_sw = lw_sw_err(got, ref)
    assert e_lw <= 1e-11 and e_sw <= 1e-7
    assert not np.array_equal(other, got)


def read_output(d):
    _, v = rrxio.read(os.path.join(d, "rte_rrtmgp_output.nc"))
    return {k: a[0].squeeze(axis=-2) if a[0].ndim >= 3 else a[0] for k, a in v.items()}


@pytest.fixture(scope="module")
def driver_case(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rrx_mcica"))
    kw = dict(ngpt=48, nbnd=3, npres=12, nflav=4, nminor_lower=7, nminor_upper=4)
    ncol, nlay = 45, 24
    atm = synthetic.make_atmosphere(ncol, nlay, nbnd_lw=3, nbnd_sw=3, clouds=True, seed=5)
    case = dict(dir=d, atm=atm, kl=synthetic.make_kdist("lw", **kw), ks=synthetic.make_kdist("sw", **kw),
                luts=(synthetic.make_cloud_lut(3, "lw"), synthetic.make_cloud_lut(3, "sw")))
    case["frac"] = np.random.default_rng(6).uniform(0.0, 1.0, (nlay, ncol)) * ((atm.lwp + atm.iwp) > 0)
    case["alpha"] = overlap_parameter(ncol, nlay, np.float64)
    return case


def test_driver_with_cloud_fraction_matches_resident_solver(driver_case, hip_f64):
    be, c = hip_f64, driver_case
    keys = ("lw_flux_up", "lw_flux_dn", "lw_flux_net", "sw_flux_up", "sw_flux_dn", "sw_flux_dn_dir", "sw_flux_net")
    synthetic_files.write_case(c["dir"], c["atm"], c["kl"], c["ks"], *c["luts"], cloud_frac=c["frac"], overlap_param=c["alpha"])
    for flags, kw in ((["--mcica-seed", "12345"], dict(mcica_seed=12345)),
                      (["--cloud-overlap", "exp-ran", "--mcica-seed=0x0123456789abcdef"],
                       dict(mcica_seed=SEED, cloud_overlap="exp_ran", overlap_param=be.asarray(c["alpha"])))):
        # 45 columns in blocks of 16 (padded to 48 on the device)
        assert run_driver(c["dir"], "--cloud-optics", "--cloud-fraction", *flags, env={"RRX_COL_BLOCK": "16"}) == 0
        out = read_output(c["dir"])
        ref = solve(be, c, frac=c["frac"], **kw)
        for i, k in enumerate(keys):
            assert cases.rel_err(out[k], ref[i]) <= (1e-11 if k.startswith("lw") else 1e-7), (flags, k)


def test_driver_refuses_bad_cloud_sampling_options(driver_case):
    c = driver_case
    synthetic_files.write_case(c["dir"], c["atm"], c["kl"], c["ks"], *c["luts"], cloud_frac=c["frac"])
    for flags in (["--cloud-fraction"],                                                     # no cloud optics
                  ["--cloud-optics", "--cloud-fraction", "--lw-scattering"],
                  ["--cloud-optics", "--cloud-fraction", "--lw-rescaling"],
                  ["--cloud-optics", "--cloud-fraction", "--sunlit-columns"],
                  ["--cloud-optics", "--cloud-fraction", "--cloud-overlap", "exp-ran"],      # no overlap_param in the file
                  ["--cloud-optics", "--cloud-fraction", "--cloud-overlap", "random"],
                  ["--cloud-optics", "--cloud-fraction", "--mcica-seed", "-1"],
                  ["--cloud-optics", "--cloud-fraction", "--mcica-seed"]):
        assert run_driver(c["dir"], *flags) == 1, flags
    synthetic_files.write_case(c["dir"], c["atm"], c["kl"], c["ks"], *c["luts"])                 # no cloud_frac in the file
    assert run_driver(c["dir"], "--cloud-optics", "--cloud-fraction") == 1
