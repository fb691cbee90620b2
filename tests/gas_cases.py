"""Inputs the gas optics does not get from synthetic.make_kdist / make_atmosphere alone: k-distributions with unequal bands and
minor-contributor intervals of every kind (irregular_kdist), and atmospheres that leave the tables, sit on their nodes and lose
their key species (edge_atmosphere). Both start from the synthetic products and reshape them; the random draws of those stay as
they are. Shared by tests/test_gas_optics_ref.py (CPU) and tests/test_gpu_gas_optics_edges.py."""
import copy

import numpy as np

import gas_optics_ref as ref
from rte_rrtmgp_cpp_amd import synthetic

GCH = 16                                   # g-points per chunk of the windowed gas optics at most
SIZES = [4, 16, 7, 1, 20, 16, 13]          # 77 g-points: a 1-g-point band, bands above 16 g-points, ngpt no multiple of 16
VARIANTS = ("fits", "whole", "span", "many", "cuts")
# flavors (1-based rows of synthetic's flavor table: 1 (h2o,co2) 2 (h2o,o3) 3 (co2,o3) 4 (h2o,n2o) 5 (h2o,ch4) 6 (co2,n2o) 7 (co2,co2)
# 8 (h2o,h2o) 9 (o3,o3) 10 (o2,o2)) of the bands in the lower and the upper regime: neighbours that share a flavor, neighbours
# that do not, and pairs that hold the same gas twice
FLAV_LOWER = [1, 7, 2, 2, 3, 3, 9]
FLAV_UPPER = [4, 8, 8, 5, 5, 6, 10]


def irregular_kdist(kind, sizes=SIZES, variant="fits", npres=20, seed=1234):
    """A k-distribution with bands of `sizes` g-points. The rows of kmajor, planck_frac, krayl and solar_source are those of the
    first sizes[b] g-points of band b of a make_kdist product with equal bands (planck_frac renormalised per band); flavors per
    band from FLAV_LOWER / FLAV_UPPER (cycled); contributor lists that differ between the regimes, with intervals inside a band,
    of one g-point, over two bands, overlapping, and all eight combinations of density scaling, complement and scaling gas;
    kminor_start out of interval order.
    variant: "fits"  every chunk has the staged form of the windowed kernel in both regimes (intervals span bands of one flavor)
             "whole" + an interval over the whole spectrum in the upper list (flavor of g-point 1 for all of it)
             "span"  + an interval over two bands of different flavors in the lower list
             "many"  + contributors on band 2 of the lower list until it has 13 (more than a chunk may list)
             "cuts"  + one-g-point intervals in the lower list until the runs outnumber the chunks the tables have room for"""
    assert variant in VARIANTS and len(sizes) >= 6 and sizes[1] >= 9 and sizes[4] >= 6 and sizes[5] >= 2
    nbnd, gpb = len(sizes), max(GCH, max(sizes))
    base = synthetic.make_kdist(kind, ngpt=nbnd * gpb, nbnd=nbnd, npres=npres, nflav=10, nminor_lower=12, nminor_upper=9, seed=seed)
    rows = np.concatenate([b * gpb + np.arange(s) for b, s in enumerate(sizes)])
    ngpt = int(rows.size)
    e = np.cumsum(sizes); b = e - np.asarray(sizes)                       # 0-based first g-point and end of every band
    kd = copy.deepcopy(base)
    kd.ngpt = ngpt
    kd.kmajor = np.ascontiguousarray(base.kmajor[rows])
    kd.band_lims_gpt = np.stack([b + 1, e], axis=1).astype(np.int32)
    kd.gpoint_bands = np.repeat(1 + np.arange(nbnd), sizes).astype(np.int32)
    fl = np.stack([np.resize(FLAV_LOWER, nbnd), np.resize(FLAV_UPPER, nbnd)], axis=1)
    kd.gpoint_flavor = np.ascontiguousarray(np.repeat(fl, sizes, axis=0).astype(np.int32))
    if kind == "lw":
        pf = base.planck_frac[rows]
        for ib in range(nbnd):
            pf[b[ib]:e[ib]] /= pf[b[ib]:e[ib]].sum(axis=0, keepdims=True)
        kd.planck_frac = np.ascontiguousarray(pf)
    else:
        kd.krayl = np.ascontiguousarray(base.krayl[:, rows])
        kd.solar_source = np.ascontiguousarray(base.solar_source[rows] * (base.solar_source.sum() / base.solar_source[rows].sum()))

    # (first g-point 0-based, end, gas, scales with density, by complement, scaling gas)
    lower = [(b[1], e[1], 4, 1, 1, 2),                 # a whole band
             (b[1] + 2, b[1] + 8, 5, 1, 0, 6),         # inside it, overlapping the one before
             (b[3], b[3] + 1, 6, 1, 1, 0),             # one g-point
             (b[2], e[3], 7, 0, 0, 0),                 # two bands (of one flavor in this regime)
             (b[4] + 2, e[4], 3, 0, 1, 3),             # from inside a band to its end
             (b[5], e[5], 1, 0, 0, 5),
             (b[0], e[0], 4, 0, 1, 0),
             (b[-1], e[-1], 2, 1, 0, 0)]
    upper = [(b[4], e[4], 5, 1, 0, 1),
             (b[5], b[5] + 1, 4, 1, 1, 7),             # one g-point at the start of a band
             (b[1], e[2], 6, 0, 0, 0),                 # two bands (of one flavor in this regime)
             (b[1] + 2, b[1] + 8, 2, 1, 0, 0)]
    if variant == "whole":
        upper.append((0, ngpt, 7, 1, 1, 4))
    if variant == "span":
        lower.append((b[1], e[2], 6, 1, 0, 3))         # lower flavors of bands 1 and 2 differ
    if variant == "many":
        lower += [(b[1], e[1], 1 + i % 7, i % 2, (i // 2) % 2, (3 * i) % 8) for i in range(13 - 2)]
    if variant == "cuts":
        lower += [(b[4] + i, b[4] + i + 1, 1 + i % 7, 1, 0, 0) for i in (0, 1, 3)] + [(b[5] + 4, b[5] + 6, 3, 0, 0, 0)]
    for sfx, items, src in (("lower", lower, base.kminor_lower), ("upper", upper, base.kminor_upper)):
        n = len(items)
        lens = np.array([hi - lo for lo, hi, *_ in items])
        order = np.random.default_rng(seed + n).permutation(n)          # where each interval's rows sit in kminor: not in interval order
        start = np.zeros(n, np.int64)
        start[order] = np.concatenate([[0], np.cumsum(lens[order])[:-1]])
        if n > 2:
            assert (np.diff(start) < 0).any(), "kminor_start must be out of interval order"
        nk = int(lens.sum())
        setattr(kd, "kminor_" + sfx, np.ascontiguousarray(src[(7 * np.arange(nk) + 3) % src.shape[0]]))
        setattr(kd, "minor_limits_gpt_" + sfx, np.array([[lo + 1, hi] for lo, hi, *_ in items], dtype=np.int32))
        setattr(kd, "kminor_start_" + sfx, (start + 1).astype(np.int32))
        setattr(kd, "idx_minor_" + sfx, np.array([x[2] for x in items], dtype=np.int32))
        setattr(kd, "minor_scales_with_density_" + sfx, np.array([x[3] for x in items], dtype=np.int8))
        setattr(kd, "scale_by_complement_" + sfx, np.array([x[4] for x in items], dtype=np.int8))
        setattr(kd, "idx_minor_scaling_" + sfx, np.array([x[5] for x in items], dtype=np.int32))
    combos = {(int(x[3]), int(x[4]), int(x[5] > 0)) for x in lower + upper}
    assert len(combos) == 8, "all eight combinations of density scaling, complement and scaling gas"
    return kd


def chunk_runs(kd):
    """How many chunks the cut rules of the windowed gas optics make of this k-distribution before the bound on their number:
    runs between flavor changes and contributor limits, cut every GCH g-points."""
    gf = kd.gpoint_flavor
    cuts = {g for g in range(1, kd.ngpt) if (gf[g] != gf[g - 1]).any()}
    for sfx in ("lower", "upper"):
        lims = np.asarray(getattr(kd, "minor_limits_gpt_" + sfx)).reshape(-1, 2)
        cuts |= {int(x) for x in np.concatenate([lims[:, 0] - 1, lims[:, 1]]) if 0 < x < kd.ngpt}
    n, s = 0, 0
    for p in sorted(cuts) + [kd.ngpt]:
        n += -(-(p - s) // GCH); s = p
    return n


def node_distance(x):
    """Distance of table coordinates to the nearest node, in spacings."""
    return np.abs(x - np.rint(x))


def assert_clear_of_nodes(kd, play, tlay, col_gas, work=np.float64):
    """The conditions under which the regime flag and the integer indices can be compared exactly: every cell is away from the
    tropopause pressure (1e-6 in ln p; 1e-3 for a float32 build), and -- fp64 -- at least 1e-9 of a spacing away from every
    temperature, pressure and eta node unless it sits on one exactly (deliberately: a temperature set to a node, a zero key species,
    a flavor that holds one gas twice). Returns the cells (nlay, ncol) that are 1e-4 of a spacing clear of every node they are not
    exactly on: where single precision finds the same indices."""
    f32 = np.dtype(work) == np.float32
    pos = ref.positions(kd, play, tlay, col_gas, np.longdouble, work)
    assert float(np.abs(pos["trop"]).min()) >= (1e-3 if f32 else 1e-6), "a cell sits on the tropopause pressure"
    clear = np.ones(pos["temp"].shape, bool)
    for k in ("temp", "press", "eta"):
        d = node_distance(pos[k])
        near = (d > 0) & (d < 1e-9)
        assert f32 or not near.any(), f"{int(near.sum())} cells within 1e-9 of a {k} node"
        ok = (d == 0) | (d >= 1e-4)
        clear &= ok if k != "eta" else ok.all(axis=(0, 3))
    if f32:
        # eta = 1 is the other discontinuity of the arithmetic (its index is clamped, its fraction is not): a cell that single
        # precision rounds onto it moves by percents, so a float32 case keeps clear of it unless it sits on it exactly
        d = (kd.neta - 1) - pos["eta"]
        assert not ((d > 0) & (d < 1e-4)).any(), "a cell rounds to eta = 1 in single precision"
    return clear


def with_ozone_floor(atm0, floor=1e-9):
    """A copy whose ozone is at least `floor`: for float32 cases, whose eta must not round to 1 (assert_clear_of_nodes)."""
    atm = copy.deepcopy(atm0)
    atm.vmr["o3"] = np.maximum(atm.vmr["o3"], floor)
    return atm


def edge_case(orc64, kd, atm0, dtype=np.float64, **kw):
    """edge_atmosphere in precision `dtype` with its gas columns, checked by assert_clear_of_nodes: (atmosphere, col_dry, col_gas,
    cells clear of the nodes)."""
    atm = edge_atmosphere(atm0, kd, **kw).astype(dtype)
    col_dry, col_gas = gas_columns(orc64, kd, atm, dtype)
    return atm, col_dry, col_gas, assert_clear_of_nodes(kd, atm.p_lay, atm.t_lay, col_gas, dtype)


# what edge_atmosphere does to the columns of a group
PATTERNS = ("p_high", "p_low", "t_low", "t_high", "t_node", "no_second", "no_first", "no_both", "no_h2o", "swing", "tsfc_end", "tsfc_beyond",
            "tsfc_below", "plain")


def edge_atmosphere(atm0, kd, block=1, patterns=PATTERNS, seed=5):
    """A copy of a make_atmosphere product whose columns, in groups of `block` neighbours, take the patterns in turn:
    p_high / p_low   pressures above the first / below the last reference pressure (less than two spacings)
    t_low / t_high   temperatures below temp_ref[0] / above temp_ref[-1] (less than two spacings; t_sfc and t_lev go along,
                     so the Planck table is left at both ends too)
    t_node           every third layer exactly on a temperature node
    no_second / no_first / no_both / no_h2o   o3 / co2 / both / h2o zero: eta = 1, eta = 0 and the col_mix fall-back, depending on the flavor
    swing            o3 and co2 times 1e-3 .. 1e3 from one column to the next
    tsfc_end / tsfc_beyond / tsfc_below   t_sfc within 1 K of the end of the Planck table, beyond it, below its start
    plain            untouched
    (edge_case adds the gas columns and asserts the distance to the nodes.)"""
    atm = copy.deepcopy(atm0)
    rng = np.random.default_rng(seed)
    nlay, ncol = atm.p_lay.shape
    prl = np.asarray(kd.press_ref_log, np.float64)
    dlnp = abs(float(kd.press_ref_log_delta))
    swing = 10.0 ** np.stack([rng.uniform(-3, 3, ncol), rng.uniform(-3, 1, ncol)])      # (co2 x 10 at most: see the ozone floor below)
    for c in range(ncol):
        pat = patterns[(c // block) % len(patterns)]
        jit = 1.0 + 0.003 * ((c % block) / max(block, 1))               # neighbours of a group are alike, not equal
        if pat in ("p_high", "p_low"):
            if pat == "p_high":
                f = np.exp(prl[0] + 1.1 * dlnp) / atm.p_lay[:, c].max()
            else:
                f = max(np.exp(prl[-1] - 0.6 * dlnp), 0.7) / atm.p_lay[:, c].min()
            atm.p_lay[:, c] *= f * jit; atm.p_lev[:, c] *= f * jit
        elif pat in ("t_low", "t_high"):
            if pat == "t_low":
                off = (kd.temp_ref[0] - 1.15 * kd.temp_ref_delta) - atm.t_lay[:, c].min()
            else:
                off = (kd.temp_ref[-1] + 0.45 * kd.temp_ref_delta) - atm.t_lay[:, c].max()
            off += 0.4 * (jit - 1.0) / 0.003
            atm.t_lay[:, c] += off; atm.t_lev[:, c] += off; atm.t_sfc[c] += off
        elif pat == "t_node":
            near = kd.temp_ref[np.argmin(np.abs(atm.t_lay[::3, c][:, None] - kd.temp_ref[None, :]), axis=1)]
            atm.t_lay[::3, c] = near
        elif pat in ("no_second", "no_first", "no_both", "no_h2o"):
            for name in {"no_second": ("o3",), "no_first": ("co2",), "no_both": ("o3", "co2"), "no_h2o": ("h2o",)}[pat]:
                atm.vmr[name][:, c] = 0.0
        elif pat == "swing":
            # (not below the smallest ozone of the plain columns: eta stays 1e-9 of a spacing away from its last node)
            atm.vmr["o3"][:, c] = np.maximum(atm.vmr["o3"][:, c] * swing[0, c], atm0.vmr["o3"].min())
            atm.vmr["co2"][:, c] *= swing[1, c]
        elif pat == "tsfc_end":
            atm.t_sfc[c] = kd.temp_ref[-1] - 0.4 - 0.3 * (jit - 1.0) / 0.003
        elif pat == "tsfc_beyond":
            atm.t_sfc[c] = kd.temp_ref[-1] + 1.3 + 2.0 * (jit - 1.0) / 0.003
        elif pat == "tsfc_below":
            atm.t_sfc[c] = kd.temp_ref[0] - 0.7 - 2.0 * (jit - 1.0) / 0.003
    return atm


def gas_columns(orc64, kd, atm, dtype=np.float64):
    """col_dry and col_gas of an atmosphere from the fp64 oracle, cast to `dtype`: every backend of a test is fed the same arrays,
    so that the table coordinates checked by assert_clear_of_nodes are those every backend sees."""
    col_dry = orc64.get_col_dry(np.ascontiguousarray(atm.vmr["h2o"], dtype=np.float64), np.ascontiguousarray(atm.p_lev, dtype=np.float64))
    col_gas = orc64.fill_gases(kd, {n: np.asarray(v, dtype=np.float64) for n, v in atm.vmr.items()}, col_dry)
    return np.ascontiguousarray(col_dry.astype(dtype)), np.ascontiguousarray(col_gas.astype(dtype))


INT_KEYS = ("jtemp", "jpress", "tropo", "jeta")
STATE_KEYS = ("col_mix", "fminor", "fmajor")


def reference_outputs(kd, atm, col_dry, col_gas, dtype=np.float64, work=np.float64):
    """Everything the gas optics of one k-distribution computes, from gas_optics_ref: the interpolation state, LW tau and the
    Planck outputs, or SW tau_abs, tau_ray, tau, ssa, g."""
    it = ref.interpolation(kd, atm.p_lay, atm.t_lay, col_gas, dtype, work)
    out = {"it_" + k: v for k, v in it.items()}
    tau = ref.tau_absorption(kd, it, atm.p_lay, atm.t_lay, col_gas, dtype)
    if kd.kind == "lw":
        out["tau"] = tau
        out.update(ref.planck_source(kd, it, atm.t_lay, atm.t_lev, atm.t_sfc, atm.nlay if atm.top_at_1 else 1, dtype))
    else:
        out["tau_abs"] = tau
        out["tau_ray"] = ref.tau_rayleigh(kd, it, col_dry, col_gas, dtype)
        out["tau"], out["ssa"], out["g"] = ref.combine(tau, out["tau_ray"], dtype, work)
    return out


def shaped_route(be, kd0, atm0, col_dry0, col_gas0):
    """The same outputs from a backend's reference-shaped entry points (the oracle, or the HIP kernels behind rrx_interpolation,
    rrx_compute_tau_absorption, rrx_compute_tau_rayleigh, rrx_combine_abs_and_rayleigh, rrx_compute_planck_source), as numpy arrays."""
    N = be.to_numpy
    kd = be.upload_kdist(kd0)
    up = be.asarray
    play, tlay, col_dry, col_gas = up(atm0.p_lay), up(atm0.t_lay), up(col_dry0), up(col_gas0)
    it = be.interpolation(kd, play, tlay, col_gas)
    out = {"it_" + k: N(v) for k, v in it.items()}
    tau = be.zeros((kd0.ngpt, atm0.nlay, atm0.ncol))
    be.compute_tau_absorption(kd, it, play, tlay, col_gas, tau)
    if kd0.kind == "lw":
        out["tau"] = N(tau)
        src = be.compute_planck_source(kd, it, tlay, up(atm0.t_lev), up(atm0.t_sfc), atm0.nlay if atm0.top_at_1 else 1)
        out.update({k: N(v) for k, v in src.items()})
    else:
        out["tau_abs"] = N(tau)
        tr = be.compute_tau_rayleigh(kd, it, col_dry, col_gas)
        out["tau_ray"] = N(tr)
        out["tau"], out["ssa"], out["g"] = (N(x) for x in be.combine_abs_and_rayleigh(tau, tr))
    return out


def float_keys(kind):
    return ("tau", "lay_src", "lev_src", "sfc_src", "sfc_src_jac") if kind == "lw" else ("tau_abs", "tau_ray", "tau", "ssa")


def spread_atmosphere(ncol, nlay, nbnd, seed=7, top_at_1=False, clouds=False):
    """make_atmosphere with the columns +-35 % apart in pressure and +-12 K in temperature: both regimes and several table cells
    in every wavefront."""
    atm = synthetic.make_atmosphere(ncol, nlay, nbnd_lw=nbnd, nbnd_sw=nbnd, seed=seed, top_at_1=top_at_1, clouds=clouds)
    rng = np.random.default_rng(seed + 1)
    scale = rng.uniform(0.65, 1.35, ncol)
    atm.p_lay = np.ascontiguousarray(atm.p_lay * scale[None, :]); atm.p_lev = np.ascontiguousarray(atm.p_lev * scale[None, :])
    dT = rng.uniform(-12, 12, ncol)
    atm.t_lay = np.ascontiguousarray(atm.t_lay + dT[None, :]); atm.t_lev = np.ascontiguousarray(atm.t_lev + dT[None, :])
    return atm


# Rounding floors of the reference arithmetic per case family, measured by tests/test_gas_optics_ref.py (which asserts that they
# still hold): E_ORACLE = rel_err(fp64 oracle, long-double reference), E_ORACLE32 = rel_err(fp32 oracle, fp64 reference on the same
# float32 inputs, floor 1e-2), the largest over LW and SW, rounded up. "optics": tau, ssa, sources, Planck outputs, col_mix;
# "jac": sfc_src_jac (a difference of two neighbouring Planck values); "weights": fminor, fmajor (fmod(eta (neta-1), 1) leaves an
# absolute error of a few 1e-16 -- a few 1e-7 in single precision -- in weights near zero that are compared relative to 1e-6 --
# 1e-2 -- of the largest).
E_ORACLE = {"regular": dict(optics=1.0e-15, jac=2e-14, weights=1.2e-9),
            "irregular": dict(optics=1.0e-15, jac=3e-14, weights=1.2e-9),
            "edges": dict(optics=1.5e-15, jac=3e-14, weights=1.2e-9)}
E_ORACLE32 = {"regular": dict(optics=5e-7, jac=9e-6, weights=1.2e-4),
              "irregular": dict(optics=4e-7, jac=1.6e-5, weights=1.2e-4),
              "edges": dict(optics=6e-7, jac=1.6e-5, weights=1.2e-4)}
TOL_WINDOW = 1e-12                          # what the project holds its windowed kernel to (tests/test_gas_window_tables.py)


def group_of(key):
    return "jac" if key == "sfc_src_jac" else "weights" if key in ("it_fminor", "it_fmajor", "fminor", "fmajor") else "optics"


def tol64(family, key):
    """fp64 outputs against the reference: the windowed kernel's bound, or 8 x the oracle's own rounding floor if that is larger."""
    return max(TOL_WINDOW, 8 * E_ORACLE[family][group_of(key)])


def tol32(family, key):
    return 4 * E_ORACLE32[family][group_of(key)]


def family_case(orc64, family, kind, ncol, nlay, dtype=np.float64, variant="whole", top_at_1=False, block=1, patterns=PATTERNS, npres=20,
                spread=True, z_top=70.e3):
    """(k-distribution, atmosphere, col_dry, col_gas, cells clear of the nodes) of a case family, in precision `dtype`:
    "regular"   make_kdist with four 16-g-point bands, columns +-35 % / +-12 K apart
    "irregular" irregular_kdist(variant) on the same kind of columns (spread=False: on make_atmosphere's columns, which are alike)
    "edges"     irregular_kdist(variant) on edge_atmosphere(block, patterns)"""
    f32 = np.dtype(dtype) == np.float32
    if family == "regular":
        kd = synthetic.make_kdist(kind, ngpt=64, nbnd=4, npres=npres, nflav=4, nminor_lower=9, nminor_upper=5)
    else:
        kd = irregular_kdist(kind, variant=variant, npres=npres)
    if family == "edges":
        atm0 = synthetic.make_atmosphere(ncol, nlay, nbnd_lw=kd.nbnd, nbnd_sw=kd.nbnd, seed=11, top_at_1=top_at_1)
        atm, col_dry, col_gas, clear = edge_case(orc64, kd, with_ozone_floor(atm0) if f32 else atm0, dtype, block=block, patterns=patterns)
    else:
        atm0 = spread_atmosphere(ncol, nlay, kd.nbnd, top_at_1=top_at_1) if spread else \
            synthetic.make_atmosphere(ncol, nlay, nbnd_lw=kd.nbnd, nbnd_sw=kd.nbnd, seed=7, top_at_1=top_at_1, z_top=z_top)
        atm = (with_ozone_floor(atm0) if f32 else atm0).astype(dtype)
        col_dry, col_gas = gas_columns(orc64, kd, atm, dtype)
        clear = assert_clear_of_nodes(kd, atm.p_lay, atm.t_lay, col_gas, dtype)
    return kd, atm, col_dry, col_gas, clear


def census_atmosphere(reason, kd, ncol, nlay, wide=256, z_top=70.e3):
    """A make_atmosphere product (columns alike: the windowed kernel takes them all) in which the first `wide` columns -- one
    workgroup of the windowed gas optics per layer, or per four layers -- cannot share a box of table nodes, for one reason:
    0  temperatures 48 K apart (more than three temp_ref_delta) at equal pressure
    1  pressures a factor 2.1 apart (more than exp(3 press_ref_log_delta) at npres = 59), inside the table
    2  every column 3 % to one side of the tropopause pressure at one layer, alternately (all columns: that layer alone straddles)
    4  ozone and n2o (key species of the lower and of the upper regime) times 1e-3 .. 1e3 from one column to the next, at equal
       temperature and pressure
    The columns behind `wide` stay as they were."""
    atm = synthetic.make_atmosphere(ncol, nlay, nbnd_lw=kd.nbnd, nbnd_sw=kd.nbnd, seed=13, z_top=z_top)
    n = min(wide, ncol)
    if reason == 0:
        off = np.linspace(-24.0, 24.0, n)
        atm.t_lay[:, :n] += off; atm.t_lev[:, :n] += off
    elif reason == 1:
        f = np.geomspace(0.5, 1.05, n)
        atm.p_lay[:, :n] *= f; atm.p_lev[:, :n] *= f
    elif reason == 2:
        l = int(np.argmin(np.abs(np.log(atm.p_lay[:, 0]) - kd.press_ref_trop_log)))
        f = np.exp(kd.press_ref_trop_log) / atm.p_lay[l, 0] * np.where(np.arange(ncol) % 2 == 0, 0.97, 1.03)
        atm.p_lay *= f; atm.p_lev *= f
    elif reason == 4:
        rng = np.random.default_rng(17)
        # (ozone not below its smallest value as it was: eta stays 1e-9 of a spacing away from its last node)
        atm.vmr["o3"][:, :n] = np.maximum(atm.vmr["o3"][:, :n] * 10.0 ** rng.uniform(-3, 3, n), atm.vmr["o3"].min())
        atm.vmr["n2o"][:, :n] *= 10.0 ** rng.uniform(-3, 3, n)
    else:
        raise ValueError(reason)
    return atm
