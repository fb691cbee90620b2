"""The longdouble two-stream + adding solver of tests/sw2s_ref.py, pinned with the CPU oracle alone: how far the fp64 and fp32 oracle sit
from it class by class, the conditions on the inputs that tests/test_gpu_sw_truth.py relies on, and closed forms.

Norm: sw2s_ref.profile_error, one number per (g-point, column) profile -- the largest |oracle - truth| over the levels of flux_up and
flux_dn over the profile's largest flux_dn -- in units of the dtype's eps. Classes: sw2s_ref.classes.

The record that is asserted (first measurement, cases.tall_inputs(4242, 24, nlay, 12), nlay 16 / 60 / 140; the oracle must stay below
8 x these at every shape of this file):

    class          fp64 oracle vs truth     fp32 oracle vs truth
    conservative   4.0e5 eps                44 eps
    resonant       115 eps                  120 eps
    plain          21 eps                   25 eps

Re-measured at the shapes and the seed of the GPU tests (sw2s_ref.SHAPES, SEED = 4243; worst of the orientations that run; CPU only,
nothing here ran on a GPU); n = profiles per class of the 12 x ncol, share of the plain class in brackets:

    fp64 (ncol, nlay)   conservative      resonant          plain
    (11, 15)            5.4e5 eps, n 11   40 eps,  n 2      27 eps, n 119 (0.90)
    (11, 40)            3.3e5 eps, n 11   43 eps,  n 21     24 eps, n 100 (0.76)
    (19, 140)           4.5e5 eps, n 19   103 eps, n 77     45 eps, n 132 (0.58)
    (9, 200)            2.5e5 eps, n 9    63 eps,  n 32     20 eps, n 67  (0.62)
    (9, 300)            4.0e5 eps, n 9    107 eps, n 42     8 eps,  n 57  (0.53)
    fp32
    (11, 15)            39 eps            37 eps            15 eps        (0.90)
    (19, 140)           43 eps            173 eps           24 eps        (0.58)
    (9, 190)            31 eps            16 eps            13 eps        (0.48)
    flux_dir (sw2s_ref.beam_error), every class and shape: at most 2.4 eps in both precisions.

With the cosines drawn per layer (mu0_lay, the by-layer entries) the same inputs give, worst over the shapes: fp64 conservative 7.0e5,
resonant 765, plain 37 eps; fp32 60 / 217 / 40 eps.

What the record does not say. The resonant class has a heavy tail in the REFERENCE: over seeds 4242 ... 4249 at these shapes, 3 of 40
fp64 draws hold a profile beyond 8 x 115 eps (1.9e3, 2.0e3, 3.8e3 eps; the profile's own min |1 - (k mu0)^2| is 4e-4 ... 7e-3 there, so
the 1e-2 threshold is not what lets them through), and the plain class reaches 112 eps once (the record says 21). That is why the GPU
test measures the oracle's own error E_class on ITS inputs instead of quoting this table, and why the seed is fixed where the oracle is
inside the record (sw2s_ref.SEED).

Conditions (asserted below for every shape the GPU tests use). With mu0 per column: conservative share <= 10 %, plain share >= 40 %,
the plain class >= 20 profiles everywhere, the resonant class >= 20 profiles from 40 layers on ((11, 15) has 2: there the 32-eps floor of
the GPU test carries the bound). The conservative class is one g-point, so it has ncol profiles, 9 ... 19: it is bounded by a constant
(CONS64), not through a sample. With the cosines drawn per layer every column can meet a resonance, so the plain share falls with the
number of layers: 0.83 / 0.70 / 0.55 at 15 / 40 / 140 layers, then 0.37 at 190 and 200 and 0.24 at 300 (26 profiles). There the 40 % cannot
hold and is not asserted; the count of 20 is."""
import numpy as np
import pytest

import sw2s_ref
from sw2s_ref import SHAPES, BOTH_ORIENTATIONS, CLASSES

L = np.longdouble
RECORD = {"f64": dict(conservative=4.0e5, resonant=115., plain=21.), "f32": dict(conservative=44., resonant=120., plain=25.)}
CASES = [(dt, s, top) for dt in ("f64", "f32") for i, s in enumerate(SHAPES[dt]) for top in ((False, True) if i < BOTH_ORIENTATIONS else (False,))]
IDS = [f"{dt}-{s[0]}x{s[1]}-top{int(t)}" for dt, s, t in CASES]


def oracle_errors(orc, dt, shape, top_at_1, by_layer=False):
    """(profile errors, beam errors) of the oracle against truth, (ngpt, ncol) each, in eps of the run's dtype"""
    I = sw2s_ref.inputs(dt, *shape)
    up, dn, beam = sw2s_ref.truth(dt, *shape, top_at_1, by_layer)
    r = orc.sw_solver_2stream(top_at_1, I["tau"], I["ssa"], I["g"], I["mu0_lay"] if by_layer else I["mu0"], I["adir"], I["adif"], I["inc"])
    eps = np.finfo(sw2s_ref.np_dtype(dt)).eps
    return sw2s_ref.profile_error(r["flux_up"], r["flux_dn"], up, dn) / eps, sw2s_ref.beam_error(r["flux_dir"], beam) / eps


@pytest.mark.parametrize("dt,shape,top_at_1", CASES, ids=IDS)
def test_oracle_stays_inside_the_recorded_table(dt, shape, top_at_1, oracle_f64, oracle_f32):
    orc = oracle_f64 if dt == "f64" else oracle_f32
    cls = sw2s_ref.input_classes(dt, *shape)
    e, eb = oracle_errors(orc, dt, shape, top_at_1)
    worst = {c: float(e[cls == c].max()) for c in CLASSES if (cls == c).any()}
    print(f"oracle vs truth {dt} {shape} top_at_1={top_at_1}: " + ", ".join(f"{c} {w:.3g} eps (n {int((cls == c).sum())})" for c, w in worst.items())
          + f"; flux_dir {eb.max():.3g} eps")
    for c, w in worst.items():
        assert w <= 8 * RECORD[dt][c], (c, w)
    assert eb.max() <= 8, eb.max()                   # a product of exponentials: nothing ill-conditioned (4e-16 = 2 eps recorded)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_oracle_with_cosines_by_layer_is_as_close(dt, oracle_f64, oracle_f32):
    """The by-layer semantics of the truth against the oracle's: the same table; a cosine taken from the wrong layer or
    the wrong end for the top level is an error of order one"""
    orc = oracle_f64 if dt == "f64" else oracle_f32
    for i, shape in enumerate(SHAPES[dt][:3]):
        cls = sw2s_ref.input_classes(dt, *shape, True)
        for top_at_1 in (False, True) if i < BOTH_ORIENTATIONS else (False,):
            e, eb = oracle_errors(orc, dt, shape, top_at_1, True)
            for c in CLASSES:
                if (cls == c).any():
                    print(f"oracle vs truth, by layer, {dt} {shape} top_at_1={top_at_1} {c}: {e[cls == c].max():.3g} eps")
                    assert e[cls == c].max() <= 8 * RECORD[dt][c], (shape, top_at_1, c)
            assert eb.max() <= 8


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_conditions_the_gpu_tests_rely_on(dt):
    for ncol, nlay in SHAPES[dt]:
        for by_layer, with_g in ((False, True), (False, False), (True, True)):      # (g = 0: the fused clear-sky form, mu0 per column only)
            cls = sw2s_ref.input_classes(dt, ncol, nlay, by_layer, with_g)
            n = {c: int((cls == c).sum()) for c in CLASSES}
            share = {c: n[c] / cls.size for c in CLASSES}
            print(f"{dt} ({ncol}, {nlay}) by_layer={by_layer} g={with_g}: " + ", ".join(f"{c} n {n[c]} share {share[c]:.2f}" for c in CLASSES))
            assert share["conservative"] <= 0.10
            assert n["conservative"] == ncol                       # one g-point: what the fused runs "without it" leave out
            assert n["plain"] >= 20
            if not by_layer or nlay <= 140:
                assert share["plain"] >= 0.40
            if nlay >= 40:
                assert n["resonant"] >= 20
        I = sw2s_ref.inputs(dt, ncol, nlay)
        keep = sw2s_ref.not_conservative(I)
        assert keep.size == sw2s_ref.NGPT - 1 and 1 not in keep
        assert np.all(I["tau"][0, 0] == 0) and np.all(I["ssa"][2, ::5] == 0) and np.all(I["ssa"][1, ::7] == 1)


def test_classes_and_profile_error_by_hand():
    ssa = np.full((3, 4, 2), 0.5); g = np.zeros_like(ssa); tau = np.ones_like(ssa)
    # ssa = 0.5, g = 0: gamma1 = 1.375, gamma2 = 0.375, k^2 = 1.75
    mu0 = np.array([0.3, 1 / np.sqrt(1.75) * (1 + 2e-3)])
    ssa[2, 1, 0] = 1.0
    cls = sw2s_ref.classes(tau, ssa, g, mu0)
    assert cls.tolist() == [["plain", "resonant"], ["plain", "resonant"], ["conservative", "resonant"]]
    assert sw2s_ref.column_classes(cls).tolist() == ["conservative", "resonant"]
    mu_lay = np.repeat(mu0[None], 4, axis=0); mu_lay[:3, 1] = 0.3            # the resonant cosine in one layer only
    assert sw2s_ref.classes(tau, ssa, None, mu_lay)[0].tolist() == ["plain", "resonant"]
    mu_lay[3, 1] = 0.3
    assert sw2s_ref.classes(tau, ssa, None, mu_lay)[0].tolist() == ["plain", "plain"]
    # profile_error: (ngpt, nlev, ncol) -> (ngpt, ncol); broadband: the truth's g-points are summed
    tu = np.arange(24, dtype=L).reshape(2, 3, 4) + 1; td = 2 * tu
    gu, gd = np.array(tu, dtype=np.float64), np.array(td, dtype=np.float64)
    gu[1, 2, 3] += 0.5; gd[0, 0, 1] -= 0.25
    e = sw2s_ref.profile_error(gu, gd, tu, td)
    want = np.zeros((2, 4)); want[1, 3] = 0.5 / td[1, :, 3].max(); want[0, 1] = 0.25 / td[0, :, 1].max()
    assert e.shape == (2, 4) and np.allclose(e, want, rtol=1e-15, atol=0)
    eb = sw2s_ref.profile_error(gu.sum(axis=0), gd.sum(axis=0), tu, td)
    wb = np.zeros(4); wb[3] = 0.5 / td.sum(axis=0)[:, 3].max(); wb[1] = 0.25 / td.sum(axis=0)[:, 1].max()
    assert eb.shape == (4,) and np.allclose(eb, wb, rtol=1e-15, atol=0)


def test_arithmetic_runs_in_the_dtype_asked_for():
    I = sw2s_ref.inputs("f64", 11, 15)
    a = (I["tau"], I["ssa"], I["g"], I["mu0"], I["adir"], I["adif"], I["inc"])
    t = sw2s_ref.solve(*a)
    d = sw2s_ref.solve(*a, dtype=np.float64)
    s = sw2s_ref.solve(*a, dtype=np.float32, work=np.float32)
    assert [x.dtype for x in t] == [np.dtype(L)] * 3 and [x.dtype for x in d] == [np.dtype(np.float64)] * 3 and s[0].dtype == np.float32
    plain = sw2s_ref.input_classes("f64", 11, 15) == "plain"
    e64 = sw2s_ref.profile_error(d[0], d[1], t[0], t[1])[plain].max()
    assert 0 < e64 <= 8 * RECORD["f64"]["plain"] * np.finfo(np.float64).eps          # fp64 numpy is as close as the fp64 oracle
    assert sw2s_ref.profile_error(s[0], s[1], t[0], t[1])[plain].max() > 1e-8        # ... and fp32 is not
    # the clamp constants follow `work`, not the arithmetic: k_min = 1e-4 moves the conservative g-point
    w32 = sw2s_ref.solve(*a, work=np.float32)
    cons = sw2s_ref.input_classes("f64", 11, 15) == "conservative"
    assert sw2s_ref.profile_error(w32[0], w32[1], t[0], t[1])[cons].max() > 1e-6
    assert sw2s_ref.clamp_constants(np.float32) == (np.float32(2.0**-23), np.float32(1e-4))
    assert sw2s_ref.clamp_constants(np.float64) == (2.0**-52, 1e-12)


# ---- closed forms, in longdouble ----------------------------------------------------------------------------------------------------
def _small(seed, ngpt=3, nlay=12, ncol=5):
    rng = np.random.default_rng(seed)
    shp = (ngpt, nlay, ncol)
    return dict(tau=10.0**rng.uniform(-3, 1, shp), ssa=rng.uniform(0., 1., shp), g=rng.uniform(-0.3, 0.9, shp), mu0=rng.uniform(0.05, 1., ncol),
                mu0_lay=rng.uniform(0.05, 1., (nlay, ncol)), adir=rng.uniform(0.05, 0.6, (ngpt, ncol)), adif=rng.uniform(0.05, 0.6, (ngpt, ncol)),
                inc=rng.uniform(0.5, 5., (ngpt, ncol)), inc_dif=rng.uniform(0.1, 1., (ngpt, ncol)))


@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("by_layer", [False, True])
def test_transparent_atmosphere_reflects_at_the_surface_only(top_at_1, by_layer):
    """tau = 0: the beam inc mu0(top layer) reaches the surface whole, flux_dn is beam + diffuse incidence at every level and flux_up
    the surface's reflection of the two. RTE's clamp keeps Rdir, Tdir >= eps(work), so each layer adds eps of the beam: 4 nlay eps."""
    d = _small(1)
    nlay = d["tau"].shape[1]
    mu = d["mu0_lay"] if by_layer else d["mu0"]
    up, dn, beam = sw2s_ref.solve(np.zeros_like(d["tau"]), d["ssa"], d["g"], mu, d["adir"], d["adif"], d["inc"], d["inc_dif"], top_at_1=top_at_1)
    top_mu = (d["mu0_lay"][0 if top_at_1 else -1] if by_layer else d["mu0"]).astype(L)
    b = d["inc"].astype(L) * top_mu[None]
    tol = 4 * nlay * np.finfo(np.float64).eps * b.max()
    assert np.array_equal(beam, np.broadcast_to(b[:, None], beam.shape))
    assert np.abs(dn - (b + d["inc_dif"])[:, None]).max() <= tol
    assert np.abs(up - (d["adir"] * b + d["adif"] * d["inc_dif"].astype(L))[:, None]).max() <= tol
    top = 0 if top_at_1 else nlay
    assert np.array_equal(dn[:, top], b + d["inc_dif"].astype(L))          # the boundary condition itself: exact


@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("with_dif", [False, True])
@pytest.mark.parametrize("scale", [1e-3, 1.0], ids=["thin", "thick"])
def test_conservative_scattering_conserves_energy(scale, top_at_1, with_dif):
    """ssa = 1, albedos in (0, 1): what enters at the top either leaves there or is absorbed by the surface -- as far as the build's
    k^2 = k_min = 1e-12 in place of 0 lets it. A round 1e-15 is out of reach of these formulas with that constant, in any arithmetic:
      - a layer loses 1 - Rdif - Tdif = k (1 - exp(-k tau))^2 / (k (1 + e2) + gamma1 (1 - e2)) <= (k tau)^2 / 2 of the diffuse flux that
        crosses it and of the order of k^2 tau / mu0 of the beam: k_min (sum of tau^2 + sum of tau / mu0) over the layers
        (measured: 0.25 x that at tau up to 10, where the balance closes to 4.0e-11);
      - Rdir and Tdir are 1/(2k) times a difference of terms that cancel to O(k): the longdouble rounding comes back multiplied by
        1/k = 1e6 per layer (measured floor, tau <= 1e-2: 4.4e-13 = 4 eps_longdouble / k; bound 2 nlay eps_longdouble / k).
    The same clamp is what makes the conservative class of the table ill-conditioned."""
    d = _small(2)
    nlay = d["tau"].shape[1]
    tau = d["tau"] * scale
    inc_dif = d["inc_dif"] if with_dif else None
    up, dn, beam = sw2s_ref.solve(tau, np.ones_like(d["ssa"]), d["g"], d["mu0"], d["adir"], d["adif"], d["inc"], inc_dif, top_at_1=top_at_1)
    top, sfc = (0, nlay) if top_at_1 else (nlay, 0)
    incident = d["inc"].astype(L) * d["mu0"].astype(L)[None] + (d["inc_dif"].astype(L) if with_dif else 0)
    absorbed = (1 - d["adir"].astype(L)) * beam[:, sfc] + (1 - d["adif"].astype(L)) * (dn[:, sfc] - beam[:, sfc])
    assert np.array_equal(dn[:, top], incident)
    e = np.abs(up[:, top] + absorbed - incident) / incident
    k_min = L(1e-12)
    bound = k_min * ((tau.astype(L)**2).sum(axis=1) + tau.astype(L).sum(axis=1) / d["mu0"].astype(L)[None]) + 2 * nlay * np.finfo(L).eps / np.sqrt(k_min)
    print(f"energy balance, ssa = 1, tau x {scale}: {float(e.max()):.3e} (bound {float(bound[np.unravel_index(np.argmax(e), e.shape)]):.1e})")
    assert np.all(e <= bound)
    if scale == 1.0:
        assert np.all(up[:, top] > 0.05 * incident)                         # (something does come back)


@pytest.mark.parametrize("top_at_1", [False, True])
@pytest.mark.parametrize("by_layer", [False, True])
def test_pure_absorption_is_beers_law(top_at_1, by_layer):
    """ssa = 0: flux_dir = inc mu0(top) exp(-sum of tau / mu0 over the layers above); without diffuse incidence flux_dn is the beam
    (to the eps(work) per layer of the Tdir clamp) and flux_up the surface's reflection attenuated on its way up"""
    d = _small(3)
    nlay = d["tau"].shape[1]
    mu = d["mu0_lay"] if by_layer else np.repeat(d["mu0"][None], nlay, axis=0)
    up, dn, beam = sw2s_ref.solve(d["tau"], np.zeros_like(d["ssa"]), d["g"], d["mu0_lay"] if by_layer else d["mu0"], d["adir"], d["adif"], d["inc"],
                                  top_at_1=top_at_1)
    if not top_at_1:
        beam, dn, tau, mu = beam[:, ::-1], dn[:, ::-1], d["tau"][:, ::-1], mu[::-1]
    else:
        tau = d["tau"]
    path = np.concatenate([np.zeros((3, 1, 5), dtype=L), np.cumsum(tau.astype(L) / mu.astype(L)[None], axis=1)], axis=1)
    want = (d["inc"].astype(L) * mu[0].astype(L)[None])[:, None] * np.exp(-path)
    assert np.abs(beam - want).max() <= 64 * np.finfo(L).eps * want.max()
    assert np.abs(dn - beam).max() <= 4 * nlay * np.finfo(np.float64).eps * want.max()
    assert np.all(dn >= beam)
