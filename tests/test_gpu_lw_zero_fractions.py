"""GPU tests of the fused LW entries on Planck fractions that are exactly zero.

The fractions forms build the source of an interior level as sqrt(pfrac(above) pfrac(below)) B_lev. Every other test draws pfrac from
[0.05, 1] or from a strictly positive table, so the product was never zero; the materialised route (rrx_planck_sources_from_fractions,
library sqrt) and the numpy references give an exact 0 there, and the entries' headers say they reproduce that route.

Inputs: the builder of tests/test_gpu_lw_2stream.py cut to 8 g-points in two uneven bands (3 + 5), with zeros planted in three of the
eleven columns (the other columns show that nothing leaks across):
  a  one whole g-point of a band that has others
  b  one interior layer of one g-point (two levels' sources are zero)
  c  the top layer only          d  the bottom layer only
  e  two adjacent interior layers (both factors of one product are zero)
Entries: rrx_lw_solver_noscat_fractions, _jac, _byband, _angles (3 angles), _optimal, rrx_lw_solver_2stream_fractions,
rrx_lw_solver_noscat_fractions_rescaled. For each: every output is finite; it equals the materialised route (Planck sources from
fractions, the per-g-point solver, the in-order sums) at the tolerance the neighbouring test of the entry uses with positive fractions;
it equals the numpy reference (lw1r_ref / lw2s_ref, evaluated in float64). Case a also against the materialised route with that g-point's layer and level
sources set to exact zeros, so that only its sfc_src (and incident flux) contributes."""
import types

import numpy as np
import pytest

import cases
import lw1r_ref
import lw2s_ref
from test_gpu_lw_2stream import inputs as lw_inputs, F64_TOL as LW2S_F64, F32_TOL as LW2S_F32
from test_gpu_lw_angles import F64_FLUX_TOL, F64_JAC_TOL, F32_FLUX_TOL, F32_JAC_TOL
from test_gpu_lw_rescaled import SAME_TOL as LW1R_SAME64, F32_SAME_TOL as LW1R_SAME32, F64_TOL as LW1R_F64, F32_TOL as LW1R_F32
from test_gpu_lw_optimal_angles import numpy_secants

pytestmark = pytest.mark.gpu
FLOOR = {"f64": 1e-6, "f32": 1e-2}
GSEL = [0, 1, 2, 5, 6, 7, 8, 9]                      # three g-points of the builder's first band, five of its second
LIMS = np.array([[1, 3], [4, 8]], dtype=np.int32)
GB = np.array([1, 1, 1, 2, 2, 2, 2, 2], dtype=np.int32)
COLS = [0, 3, 10]
ENTRIES = ("fractions", "jac", "byband", "angles", "optimal", "2stream", "rescaled")
# (against the materialised route, against numpy) per dtype: the neighbouring tests' bounds. Against numpy the no-scattering entries
# take the project's LW bounds against the CPU oracle (1e-10 / 3e-5, tests/test_gpu_parity.py; by band 1e-9, tests/test_gpu_byband.py)
TOL = {"f64": dict(fractions=(F64_FLUX_TOL, 1e-10), jac=(F64_FLUX_TOL, 1e-10), byband=(1e-11, 1e-9), angles=(F64_FLUX_TOL, 1e-10),
                   optimal=(F64_FLUX_TOL, 1e-10), rescaled=(LW1R_SAME64, LW1R_F64)),
       "f32": dict(fractions=(F32_FLUX_TOL, 3e-5), jac=(F32_FLUX_TOL, 3e-5), byband=(3e-5, 3e-5), angles=(F32_FLUX_TOL, 3e-5),
                   optimal=(F32_FLUX_TOL, 3e-5), rescaled=(LW1R_SAME32, LW1R_F32))}
TOL["f64"]["2stream"] = (LW2S_F64, LW2S_F64)
TOL["f32"]["2stream"] = (LW2S_F32, LW2S_F32)
JAC_TOL = {"f64": F64_JAC_TOL, "f32": F32_JAC_TOL}


def plant(pfrac, which, top_at_1):
    """Zeros in pfrac (ngpt, nlay, ncol), columns COLS; returns the g-point that is zero as a whole (case a) or None"""
    nlay = pfrac.shape[1]
    top, bot = (0, nlay - 1) if top_at_1 else (nlay - 1, 0)
    mid = nlay // 2
    c = np.array(COLS)
    if which == "a":
        pfrac[4][:, c] = 0
        return 4
    if which == "b":
        pfrac[1, mid, c] = 0
    elif which == "c":
        pfrac[0, top, c] = 0; pfrac[5, top, c] = 0
    elif which == "d":
        pfrac[0, bot, c] = 0; pfrac[5, bot, c] = 0
    elif which == "e":
        pfrac[2, mid, c] = 0; pfrac[2, mid + 1, c] = 0
    else:
        raise ValueError(which)
    return None


def build(npdt, ncol, nlay, top_at_1, which):
    B = lw_inputs(ncol, nlay, seed=nlay + ncol, dtype=npdt)
    I = {k: np.ascontiguousarray(B[k][GSEL]) for k in ("tau", "pfrac", "emis", "ssrc", "inc")}
    I.update({k: np.ascontiguousarray(B[k][:2]) for k in ("blay", "blev", "ct", "cw", "cg")})
    rng = np.random.default_rng(1000 + nlay)
    I["sec"] = np.ascontiguousarray(rng.uniform(1.2, 2.2, (3, 8, ncol)).astype(npdt))
    I["wts"] = rng.uniform(0.2, 0.6, 3).astype(npdt)
    I["sjac"] = np.ascontiguousarray(rng.uniform(0.1, 0.5, (8, ncol)).astype(npdt))
    I["fit"] = np.stack([rng.uniform(-0.3, 0.3, 2), rng.uniform(1.5, 1.8, 2)])
    I["gb"], I["lims"] = GB, LIMS
    zero_g = plant(I["pfrac"], which, top_at_1)
    assert (I["pfrac"] == 0).any() and (I["pfrac"][:, :, 1] > 0).all()
    return I, zero_g


class Case:
    def __init__(self, be, npdt, I, top_at_1):
        self.be, self.npdt, self.I, self.top = be, npdt, I, bool(top_at_1)
        up = be.asarray
        self.tau, self.emis, self.inc, self.sjac = up(I["tau"]), up(I["emis"]), up(I["inc"]), up(I["sjac"])
        self.sec3, self.w3 = up(I["sec"]), up(I["wts"])
        self.sec1, self.w1 = up(np.ascontiguousarray(I["sec"][:1])), up(I["wts"][:1])
        self.fr = dict(pfrac=up(I["pfrac"]), blay=up(I["blay"]), blev=up(I["blev"]), sfc_src=up(I["ssrc"]), sfc_src_jac=self.sjac)
        self.kd = types.SimpleNamespace(band_lims_gpt=up(LIMS), gpoint_bands=up(GB))
        self.fit = up(np.ascontiguousarray(I["fit"].T.astype(npdt)))          # the C ABI's layout
        self.cld = (up(I["ct"]), up(I["cw"]), up(I["cg"]))

    # ---- the fused entries
    def fused(self, entry):
        be = self.be
        if entry == "fractions":
            r = be.lw_solver_noscat_fractions(self.top, self.kd, self.sec1, self.w1, self.tau, self.fr, self.emis, inc_flux=self.inc)
        elif entry == "jac":
            r = be.lw_solver_noscat_fractions_jac(self.top, self.kd, self.sec1, self.w1, self.tau, self.fr, self.emis, inc_flux=self.inc)
        elif entry == "byband":
            r = be.lw_solver_noscat_fractions_byband(self.top, self.kd, self.sec1, self.w1, self.tau, self.fr, self.emis, inc_flux=self.inc)
        elif entry == "angles":
            r = be.lw_solver_noscat_fractions_angles(self.top, self.kd, self.sec3, self.w3, self.tau, self.fr, self.emis, inc_flux=self.inc,
                                                     jacobian=True)
        elif entry == "optimal":
            r = be.lw_solver_noscat_fractions_optimal(self.top, self.kd, self.w1, self.tau, self.fr, self.emis, fit=self.fit, inc_flux=self.inc,
                                                      jacobian=True)
        elif entry == "2stream":
            r = be.lw_solver_2stream_fractions(self.top, self.kd, self.tau, self.fr, self.emis, cloud=self.cld, inc_flux=self.inc)
        else:
            r = be.lw_solver_noscat_fractions_rescaled(self.top, self.kd, self.sec1, self.w1, self.tau, self.fr, self.emis, cloud=self.cld,
                                                       inc_flux=self.inc)
        return {k: be.to_numpy(v) for k, v in r.items()}

    # ---- the materialised route: per-g-point fluxes on the device
    def _angles_of(self, entry):
        if entry == "angles":
            return self.sec3, self.w3
        if entry == "optimal":
            return self.be.lw_optimal_secants(self.kd, self.tau, fit=self.fit)[None].contiguous(), self.w1
        return self.sec1, self.w1

    def per_gpoint(self, entry, zero_g=None):
        be = self.be
        lay, lev = be.planck_sources_from_fractions(self.kd, self.fr)
        if zero_g is not None:
            lay[zero_g, :, COLS] = 0; lev[zero_g, :, COLS] = 0          # (the columns that hold the zeros)
        if entry in ("2stream", "rescaled"):
            tau, ssa, g = self.tau.clone(), be.zeros(tuple(self.tau.shape)), be.zeros(tuple(self.tau.shape))
            be.inc_2stream_by_2stream_bybnd(tau, ssa, g, *self.cld, self.kd.band_lims_gpt)
            if entry == "2stream":
                return be.lw_solver_2stream(self.top, tau, ssa, g, lev, self.emis, self.fr["sfc_src"], inc_flux=self.inc)
            return be.lw_solver_noscat_rescaled(self.top, self.sec1, self.w1, tau, ssa, g, lay, lev, self.emis, self.fr["sfc_src"],
                                                inc_flux=self.inc)
        sec, w = self._angles_of(entry)
        return be.lw_solver_noscat(self.top, sec, w, self.tau, lay, lev, self.emis, self.fr["sfc_src"], inc_flux=self.inc,
                                   do_jacobians=True, sfc_src_jac=self.sjac)

    def materialised(self, entry, zero_g=None):
        be = self.be
        r = self.per_gpoint(entry, zero_g)
        out = {k: be.to_numpy(be.sum_broadband(v)) for k, v in r.items()}
        if entry == "byband":
            for k in ("up", "dn"):
                out["bnd_flux_" + k] = be.to_numpy(be.sum_byband(r["flux_" + k], self.kd.band_lims_gpt))
        return out

    # ---- numpy, in float64 on the inputs of the run (widening float32 is exact). On these inputs the float32 evaluation of the
    # references is itself 1.0e-4 ... 5.8e-4 (lw2s_ref) and 2.0e-6 ... 5.1e-6 (lw1r_ref) from their float64 evaluation -- the cancelling
    # source terms of thin layers that the neighbouring files describe -- which is at or beyond the fp32 bounds taken from them
    def numpy(self, entry):
        I = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in self.I.items()}
        z = np.zeros_like(I["tau"])
        cld_np = (I["ct"], I["cw"], I["cg"])
        lev = lw2s_ref.level_sources(I["pfrac"], I["blev"], GB)
        assert (lev == 0).any()
        if entry == "2stream":
            tau, ssa, g = lw2s_ref.combine(I["tau"], cld_np, GB)
            up, dn = lw2s_ref.solve(tau, ssa, g, lev, I["emis"], I["ssrc"], I["inc"], self.top)
            return dict(flux_up=lw2s_ref.broadband(up), flux_dn=lw2s_ref.broadband(dn))
        lay = lw1r_ref.layer_sources(I["pfrac"], I["blay"], GB)
        if entry == "rescaled":
            tau, ssa, g = lw1r_ref.combine(I["tau"], cld_np, GB)
            up, dn = lw1r_ref.solve(I["sec"][:1], I["wts"][:1], tau, ssa, g, lay, lev, I["emis"], I["ssrc"], I["inc"], self.top)
            return dict(flux_up=lw1r_ref.broadband(up), flux_dn=lw1r_ref.broadband(dn))
        if entry == "angles":
            sec, w = I["sec"], I["wts"]
        elif entry == "optimal":
            sec, w = np.ascontiguousarray(numpy_secants(I, I["fit"], self.npdt)[None]), I["wts"][:1]
        else:
            sec, w = I["sec"][:1], I["wts"][:1]
        up, dn, jac = lw1r_ref.solve(sec, w, I["tau"], z, z, lay, lev, I["emis"], I["ssrc"], I["inc"], self.top, sfc_src_jac=I["sjac"],
                                     rescale=False)
        out = dict(flux_up=lw1r_ref.broadband(up), flux_dn=lw1r_ref.broadband(dn), flux_up_jac=lw1r_ref.broadband(jac))
        if entry == "byband":
            for k, a in (("up", up), ("dn", dn)):
                out["bnd_flux_" + k] = np.stack([lw1r_ref.broadband(a[lo - 1:hi]) for lo, hi in LIMS])
        return out


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("which", ["a", "b", "c", "d", "e"])
@pytest.mark.parametrize("top_at_1", [False, True], ids=["top0", "top1"])
@pytest.mark.parametrize("ncol,nlay", [(11, 15), (11, 140)])
def test_zero_fractions_give_the_materialised_routes_fluxes(dt, ncol, nlay, top_at_1, which, hip_f64, hip_f32):
    be, npdt = (hip_f64, np.float64) if dt == "f64" else (hip_f32, np.float32)
    I, zero_g = build(npdt, ncol, nlay, top_at_1, which)
    c = Case(be, npdt, I, top_at_1)
    failures = []
    for entry in ENTRIES:
        got = c.fused(entry)
        tag = f"LWZERO {dt} {ncol}x{nlay} top{int(top_at_1)} case {which} {entry}"
        bad = [k for k, v in got.items() if not np.isfinite(v).all()]
        if bad:
            n = sum(int((~np.isfinite(got[k])).sum()) for k in bad)
            print(f"{tag}: NOT FINITE in {bad} ({n} values)")
            failures.append(f"{entry}: not finite: {bad}")
            continue
        refs = [("materialised", c.materialised(entry), TOL[dt][entry][0]), ("numpy", c.numpy(entry), TOL[dt][entry][1])]
        if zero_g is not None:
            refs.append(("materialised, exact-zero sources", c.materialised(entry, zero_g), TOL[dt][entry][0]))
        for name, want, tol in refs:
            for k in got:
                if k == "bnd_flux_net":          # a difference of the two: held to the returned band sums bit for bit, as tests/test_gpu_byband.py does
                    assert np.array_equal(got[k], got["bnd_flux_dn"] - got["bnd_flux_up"]), (entry, k)
                    continue
                t = JAC_TOL[dt] if (k == "flux_up_jac" and name != "numpy") else tol
                e = cases.rel_err(got[k], want[k], floor=FLOOR[dt])
                print(f"{tag} vs {name} {k}: {e:.3e} (bound {t:.1e})")
                if not e <= t:
                    failures.append(f"{entry} vs {name} {k}: {e:.3e} > {t:.1e}")
    assert not failures, "\n".join(failures)
