#!/usr/bin/env python3
"""Digests of every public output of pipeline.ResidentSolver after its first and its second step(), on seeded synthetic inputs, one
JSON line per case. Two versions of the Python modules that print the same lines launched the same kernels on the same arguments: the
check of a change to the solver's host code that moves no arithmetic.

  python tools/resident_digest.py > profiles/resident_digests.jsonl

Shape: 32 g-points in 4 bands, 30 layers, 40 columns with a +-35 % surface-pressure spread, fp64 and fp32. Every case runs twice: in the
caller's column order unpadded (RRX_PAD_COLUMNS=0, sort_columns="0"), and sorted and padded to 48 columns (RRX_PAD_COLUMNS=1,
sort_columns="1"). Cases: every LW form (fractions, 3 angles, optimal angles with keep_secants, each also with the Jacobian; by band;
two-stream; rescaled), clear and with cloud tables; per-g-point fluxes with 1 and 3 angles; sunlit-only SW with 13 of the 40 columns
dark, all dark and all lit, by band too; mu0_lay= and altitude=, plain and by band, and altitude= with sunlit; cloud_fraction under
both overlaps (the seed advances between the steps); overlap=True. Outputs: fluxes and, where they exist, bnd_fluxes[*],
lw_flux_up_jac, lw_secants, mu0_lay_step (not with sunlit: the columns past the sunlit ones are never written)."""
import hashlib, json, os, sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rte_rrtmgp_cpp_amd as R
from rte_rrtmgp_cpp_amd import pipeline, synthetic

NGPT, NBND, NLAY, NCOL, NDARK = 32, 4, 30, 40, 13


def digest(t):
    return hashlib.blake2b(t.contiguous().cpu().numpy().tobytes(), digest_size=8).hexdigest()


def cases():
    lw_forms = {"fractions": {}, "angles3": dict(n_gauss_angles=3), "optimal": dict(optimal_angles=True, keep_secants=True)}
    out = {}
    for clouds in (False, True):
        c = "_cloud" if clouds else ""
        for name, kw in lw_forms.items():
            out[name + c] = dict(kw, clouds=clouds)
            out[name + "_jac" + c] = dict(kw, jacobian=True, clouds=clouds)
        out["byband" + c] = dict(byband=True, clouds=clouds)
        out["two_stream" + c] = dict(lw_scattering=True, clouds=clouds)
        out["rescaled" + c] = dict(lw_rescaling=True, clouds=clouds)
        out["per_gpoint" + c] = dict(do_broadband=False, clouds=clouds)
        out["sunlit" + c] = dict(sunlit=True, dark=NDARK, clouds=clouds)
    out["per_gpoint_angles3"] = dict(do_broadband=False, n_gauss_angles=3)
    out["per_gpoint_sunlit"] = dict(do_broadband=False, sunlit=True, dark=NDARK)
    out["byband_sunlit"] = dict(byband=True, sunlit=True, dark=NDARK)
    out["byband_sunlit_all_dark"] = dict(byband=True, sunlit=True, dark=NCOL)
    out["byband_sunlit_all_lit"] = dict(byband=True, sunlit=True, dark=0)
    out["sunlit_all_dark"] = dict(sunlit=True, dark=NCOL)
    for c, kw in (("", {}), ("_byband", dict(byband=True))):
        out["mu0_lay" + c] = dict(kw, mu0_lay=True)
        out["altitude" + c] = dict(kw, altitude=True)
    out["altitude_sunlit_cloud"] = dict(altitude=True, sunlit=True, dark=NDARK, clouds=True)
    out["mcica_max_ran"] = dict(clouds=True, mcica="max_ran")
    out["mcica_exp_ran_byband"] = dict(clouds=True, mcica="exp_ran", byband=True)
    out["mcica_per_gpoint"] = dict(clouds=True, mcica="max_ran", do_broadband=False)
    out["overlap"] = dict(overlap=True)
    out["overlap_byband_cloud_sunlit"] = dict(overlap=True, byband=True, clouds=True, sunlit=True, dark=NDARK)
    return out


def run(be, dtype, name, spec, ordered):
    spec = dict(spec)
    rng = np.random.default_rng(4242)
    kdkw = dict(ngpt=NGPT, nbnd=NBND, npres=20, nflav=4, nminor_lower=9, nminor_upper=5)
    kl, ks = be.upload_kdist(synthetic.make_kdist("lw", **kdkw)), be.upload_kdist(synthetic.make_kdist("sw", **kdkw))
    clouds, dark, mcica = spec.pop("clouds", False), spec.pop("dark", 0), spec.pop("mcica", None)
    atm0 = synthetic.make_atmosphere(NCOL, NLAY, nbnd_lw=NBND, nbnd_sw=NBND, clouds=clouds, seed=7)
    f = rng.uniform(0.65, 1.35, NCOL)
    atm0.p_lay = np.ascontiguousarray(atm0.p_lay * f); atm0.p_lev = np.ascontiguousarray(atm0.p_lev * f)
    night = rng.permutation(NCOL)[:dark]
    atm0.mu0 = atm0.mu0.copy()
    atm0.mu0[night] = np.where(np.arange(dark) % 2 == 0, 0.0, -0.3)
    atm = pipeline.upload_atmosphere(be, atm0.astype(dtype))
    kw = dict(do_broadband=True, sort_columns="1" if ordered else "0")
    if clouds:
        kw["cloud_luts"] = (be.upload_lut(synthetic.make_cloud_lut(NBND, "lw")), be.upload_lut(synthetic.make_cloud_lut(NBND, "sw")))
    if spec.pop("mu0_lay", False):
        kw["mu0_lay"] = be.asarray(rng.uniform(0.05, 1.0, (NLAY, NCOL)))
    if spec.pop("altitude", False):
        z = (np.arange(NLAY) + 0.5) * (70.e3 / NLAY)
        kw["altitude"] = be.asarray(np.repeat(z[:, None], NCOL, axis=1) + rng.uniform(0., 500., NCOL)[None, :] + 600.)
        kw["ref_altitude"] = be.asarray(rng.uniform(0., 600., NCOL))
    if mcica:
        kw.update(cloud_fraction=be.asarray(rng.uniform(0., 1., (NLAY, NCOL))), cloud_overlap=mcica, mcica_seed=5, mcica_col_offset=100)
        if mcica == "exp_ran":
            kw["overlap_param"] = be.asarray(rng.uniform(0.2, 0.9, (NLAY-1, NCOL)))
    kw.update(spec)
    os.environ["RRX_PAD_COLUMNS"] = "1" if ordered else "0"
    sv = pipeline.ResidentSolver(be, kl, ks, atm, **kw)
    assert (sv.npad, sv.sort_columns) == ((8, True) if ordered else (0, False))
    line = {"dtype": "f64" if dtype == np.float64 else "f32", "order": "sorted_padded" if ordered else "caller", "case": name}
    for istep in (1, 2):
        sv.step()
        be.synchronize()
        outs = {"fluxes": sv.fluxes, "lw_flux_up_jac": sv.lw_flux_up_jac, "lw_secants": sv.lw_secants}
        outs.update({"bnd_" + k: v for k, v in (sv.bnd_fluxes or {}).items()})
        if not kw.get("sunlit"):
            outs["mu0_lay_step"] = sv.mu0_lay_step
        line.update({f"{k}@{istep}": digest(v) for k, v in sorted(outs.items()) if v is not None})
        sv.mcica_seed += 1
    print(json.dumps(line, separators=(",", ":")), flush=True)


for dtype in (np.float64, np.float32):
    be = R.HipKernels(dtype, "cuda:0")
    for ordered in (False, True):
        for name, spec in cases().items():
            run(be, dtype, name, spec, ordered)
