#!/usr/bin/env python3
"""Digests of what every fused solver entry writes, on seeded inputs, one JSON line per case. Two builds that print the same lines
computed the same bits: the check of a change that moves no arithmetic (host launch code, say).

  python tools/solver_digest.py

Cases, 32 g-points in 4 bands, fp64 and fp32: (ncol, nlay) = (6, 60), (45, 140), (46, 200), (6, 300), (6, 600) -- six columns split
the g-point loop into 8 ranges, 45 / 46 are the odd / even column counts of the fp32 geometries, 600 layers lie outside the tilings;
rrx_set_broadband_gsplit 1 and 4 at (46, 140); LW and SW variant 7 at (45, 140); LW variant 15 in fp32 at (46, 140). Entries:
lw_solver_noscat with do_broadband, lw_solver_noscat_fractions, _jac, _angles with 1 and 3 angles, _optimal with secants_out,
_byband, _rescaled and lw_solver_2stream_fractions with and without cloud, sw_solver_2stream broadband without and with g,
sw_solver_2stream_byband."""
import hashlib, json, os, sys, types
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rte_rrtmgp_cpp_amd as R

NGPT, NBND = 32, 4


def digest(t):
    return hashlib.blake2b(t.contiguous().cpu().numpy().tobytes(), digest_size=8).hexdigest()


def run(be, dtype, ncol, nlay, setting):
    rng = np.random.default_rng(20240 + 1000*ncol + nlay)
    u = lambda lo, hi, *shape: be.asarray(rng.uniform(lo, hi, shape).astype(dtype))
    gpt, bnd = (NGPT, nlay, ncol), (NBND, nlay, ncol)
    per = NGPT // NBND
    lims = np.array([[b*per + 1, (b + 1)*per] for b in range(NBND)], dtype=np.int32)
    kd = types.SimpleNamespace(band_lims_gpt=be.asarray(lims), gpoint_bands=be.asarray(np.repeat(np.arange(1, NBND + 1, dtype=np.int32), per)))
    tau = u(1e-3, 0.5, *gpt)
    fr = dict(pfrac=u(0.01, 0.2, *gpt), blay=u(50., 150., *bnd), blev=u(50., 150., NBND, nlay + 1, ncol), sfc_src=u(5., 30., NGPT, ncol),
              sfc_src_jac=u(0.1, 0.5, NGPT, ncol))
    lay_src, lev_src = u(1., 20., *gpt), u(1., 20., NGPT, nlay + 1, ncol)
    emis, inc = u(0.8, 1.0, NGPT, ncol), u(0., 5., NGPT, ncol)
    sec3, wts3 = u(1.2, 2.2, 3, NGPT, ncol), u(0.2, 0.6, 3)
    sec1, wts1 = sec3[:1].contiguous(), wts3[:1].contiguous()
    fit = be.asarray(np.stack([rng.uniform(-0.3, 0.3, NBND), rng.uniform(1.5, 1.8, NBND)], axis=1).astype(dtype))
    cloud = (u(0., 2., *bnd), u(0.5, 1., *bnd), u(0., 0.9, *bnd))
    ssa, g, mu0 = u(0.1, 1., *gpt), u(0., 0.9, *gpt), u(0.1, 1., ncol)
    alb_dir, alb_dif, inc_dir, inc_dif = u(0.05, 0.6, NGPT, ncol), u(0.05, 0.6, NGPT, ncol), u(1., 40., NGPT, ncol), u(0., 2., NGPT, ncol)
    top = True
    entries = {
        "lw_noscat_broadband": lambda: be.lw_solver_noscat(top, sec1, wts1, tau, lay_src, lev_src, emis, fr["sfc_src"], inc_flux=inc,
                                                           do_broadband=True),
        "lw_fractions": lambda: be.lw_solver_noscat_fractions(top, kd, sec1, wts1, tau, fr, emis, inc_flux=inc),
        "lw_fractions_jac": lambda: be.lw_solver_noscat_fractions_jac(top, kd, sec1, wts1, tau, fr, emis, inc_flux=inc),
        "lw_fractions_angles1": lambda: be.lw_solver_noscat_fractions_angles(top, kd, sec1, wts1, tau, fr, emis, inc_flux=inc),
        "lw_fractions_angles1_jac": lambda: be.lw_solver_noscat_fractions_angles(top, kd, sec1, wts1, tau, fr, emis, inc_flux=inc, jacobian=True),
        "lw_fractions_angles3": lambda: be.lw_solver_noscat_fractions_angles(top, kd, sec3, wts3, tau, fr, emis, inc_flux=inc),
        "lw_fractions_angles3_jac": lambda: be.lw_solver_noscat_fractions_angles(top, kd, sec3, wts3, tau, fr, emis, inc_flux=inc, jacobian=True),
        "lw_fractions_optimal": lambda: be.lw_solver_noscat_fractions_optimal(top, kd, wts1, tau, fr, emis, fit=fit, inc_flux=inc, keep_secants=True),
        "lw_fractions_optimal_jac": lambda: be.lw_solver_noscat_fractions_optimal(top, kd, wts1, tau, fr, emis, fit=fit, inc_flux=inc,
                                                                                  jacobian=True, keep_secants=True),
        "lw_fractions_byband": lambda: be.lw_solver_noscat_fractions_byband(top, kd, sec1, wts1, tau, fr, emis, inc_flux=inc),
        "lw_fractions_rescaled": lambda: be.lw_solver_noscat_fractions_rescaled(top, kd, sec1, wts1, tau, fr, emis, inc_flux=inc),
        "lw_fractions_rescaled_cloud": lambda: be.lw_solver_noscat_fractions_rescaled(top, kd, sec1, wts1, tau, fr, emis, cloud=cloud, inc_flux=inc),
        "lw_2stream_fractions": lambda: be.lw_solver_2stream_fractions(top, kd, tau, fr, emis, inc_flux=inc),
        "lw_2stream_fractions_cloud": lambda: be.lw_solver_2stream_fractions(top, kd, tau, fr, emis, cloud=cloud, inc_flux=inc),
        "sw_2stream_broadband": lambda: be.sw_solver_2stream(top, tau, ssa, None, mu0, alb_dir, alb_dif, inc_dir, inc_flux_dif=inc_dif,
                                                             do_broadband=True),
        "sw_2stream_broadband_g": lambda: be.sw_solver_2stream(top, tau, ssa, g, mu0, alb_dir, alb_dif, inc_dir, inc_flux_dif=inc_dif,
                                                               do_broadband=True),
        "sw_2stream_byband": lambda: be.sw_solver_2stream_byband(top, tau, ssa, g, mu0, alb_dir, alb_dif, inc_dir, kd.band_lims_gpt,
                                                                 inc_flux_dif=inc_dif),
    }
    for name, call in entries.items():
        out = call()
        be.synchronize()
        line = {"dtype": "f64" if dtype == np.float64 else "f32", "ncol": ncol, "nlay": nlay, "setting": setting, "entry": name}
        line.update({k: digest(v) for k, v in sorted(out.items())})
        print(json.dumps(line, separators=(",", ":")), flush=True)


for dtype in (np.float64, np.float32):
    be = R.HipKernels(dtype, "cuda:0")
    for ncol, nlay in ((6, 60), (45, 140), (46, 200), (6, 300), (6, 600)):
        run(be, dtype, ncol, nlay, "default")
    for n in (1, 4):
        be.set_broadband_gsplit(n)
        run(be, dtype, 46, 140, f"gsplit{n}")
    be.set_broadband_gsplit(0)
    be.set_variant(lw=7, sw=7)
    run(be, dtype, 45, 140, "variant7")
    be.set_variant(lw=0, sw=0)
    if dtype == np.float32:
        be.set_variant(lw=15)
        run(be, dtype, 46, 140, "lw_variant15")
        be.set_variant(lw=0)
