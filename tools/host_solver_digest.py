#!/usr/bin/env python3
"""Digests of every variable the stand-alone C++ driver writes (rte_rrtmgp_output.nc), one JSON line per run, over flag sets that
reach every branch of Radiation_solver_longwave / _shortwave::solve_gpu. Two versions of the host sources that print the same lines
launched the same kernels on the same arguments: the check of a change to the host classes that moves no arithmetic.

  python tools/host_solver_digest.py > profiles/host_solver_digests.jsonl

Case (synthetic_files.write_case): 45 columns x 60 layers with a +-35 % surface-pressure spread, 48 g-points in 3 bands, cloud and
aerosol tables, cloud_frac, overlap_param, z_lay and z_ref in the input. The sunlit-only sets read an input with 13 columns dark
("dark13") or all of them ("dark45"); every other set has all columns lit. Each set runs through rrx_host_main four times -- in
column blocks of 7 (six blocks and a residual of 3) and as one block, each with the columns ordered on the host and with
--device-sort-columns (sorted and padded to 48 inside solve_gpu) -- and in both precisions (fp32: the _sp library, in a child
process of its own). A refused flag set is recorded by its non-zero status."""
import ctypes, hashlib, json, os, subprocess, sys, tempfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rte_rrtmgp_cpp_amd import synthetic, synthetic_files, rrxio

NGPT, NBND, NLAY, NCOL, NDARK = 48, 3, 60, 45, 13
CLOUD, BND, BYBAND, PERG = "--cloud-optics", "--output-bnd-fluxes", "--byband-solvers", "--no-broadband-solvers"
ANG3, JAC, OPT, SCAT, RESC = "--lw-gauss-angles=3", "--lw-jacobian", "--lw-optimal-angles", "--lw-scattering", "--lw-rescaling"
SUN, SPH, FRAC, AER, HEAT = "--sunlit-columns", "--sw-spherical-mu0", "--cloud-fraction", "--aerosol-optics", "--heating-rates"


def flag_sets():
    """name -> (input file variant, flags)"""
    s = {"default": [], "bnd": [BND], "bnd_byband": [BND, BYBAND], "byband_setting_only": [BYBAND], "per_gpoint": [PERG],
         "per_gpoint_bnd": [PERG, BND], "per_gpoint_bnd_byband": [PERG, BND, BYBAND],
         "optical": ["--output-optical"], "optical_no_fluxes": ["--output-optical", "--no-fluxes"], "optical_cloud_bnd": ["--output-optical", CLOUD, BND],
         "cloud": [CLOUD], "cloud_no_delta": [CLOUD, "--no-delta-cloud"], "cloud_bnd": [CLOUD, BND], "cloud_bnd_byband": [CLOUD, BND, BYBAND],
         "cloud_per_gpoint": [CLOUD, PERG],
         "angles3": [ANG3], "angles3_jac": [ANG3, JAC], "angles3_per_gpoint": [ANG3, PERG],
         "angles3_per_gpoint_jac": [ANG3, PERG, JAC], "angles3_bnd": [ANG3, BND], "angles3_bnd_byband": [ANG3, BND, BYBAND],
         "jac": [JAC], "jac_per_gpoint": [JAC, PERG], "jac_bnd": [JAC, BND], "jac_byband": [JAC, BYBAND],
         "jac_bnd_byband": [JAC, BND, BYBAND],
         "optimal": [OPT], "optimal_jac": [OPT, JAC], "optimal_per_gpoint": [OPT, PERG],
         "optimal_per_gpoint_jac": [OPT, PERG, JAC], "optimal_bnd": [OPT, BND], "optimal_angles3": [OPT, ANG3], "optimal_byband": [OPT, BYBAND],
         "scattering": [SCAT], "scattering_cloud": [SCAT, CLOUD], "scattering_jac": [SCAT, JAC], "scattering_bnd": [SCAT, BND],
         "scattering_per_gpoint": [SCAT, PERG], "scattering_angles3": [SCAT, ANG3], "scattering_optimal": [SCAT, OPT],
         "scattering_optical_no_fluxes": [SCAT, CLOUD, "--output-optical", "--no-fluxes"],
         "rescaling": [RESC], "rescaling_cloud": [RESC, CLOUD], "rescaling_jac": [RESC, JAC], "rescaling_bnd": [RESC, BND],
         "rescaling_scattering": [RESC, SCAT], "rescaling_angles3": [RESC, ANG3],
         "spherical": [SPH], "spherical_bnd_byband": [SPH, BND, BYBAND], "spherical_per_gpoint": [SPH, PERG],
         "mcica": [CLOUD, FRAC, "--mcica-seed=5"], "mcica_exp_ran": [CLOUD, FRAC, "--cloud-overlap=exp-ran", "--mcica-seed=6"],
         "mcica_bnd_byband": [CLOUD, FRAC, BND, BYBAND], "mcica_per_gpoint": [CLOUD, FRAC, PERG], "mcica_jac_angles3": [CLOUD, FRAC, JAC, ANG3],
         "mcica_spherical": [CLOUD, FRAC, SPH], "mcica_no_cloud_optics": [FRAC], "mcica_scattering": [CLOUD, FRAC, SCAT],
         "mcica_rescaling": [CLOUD, FRAC, RESC], "mcica_sunlit": [CLOUD, FRAC, SUN],
         "aerosol": [AER], "aerosol_delta_cloud_bnd": [AER, "--delta-aerosol", CLOUD, BND],
         "heating": [HEAT], "heating_cloud_bnd_byband": [HEAT, CLOUD, BND, BYBAND],
         "no_longwave": ["--no-longwave"], "no_shortwave": ["--no-shortwave"]}
    out = {k: ("lit", v) for k, v in s.items()}
    for variant in ("lit", "dark13", "dark45"):
        out["sunlit_" + variant] = (variant, [SUN])
        out["sunlit_bnd_byband_" + variant] = (variant, [SUN, BND, BYBAND])
    out.update({"sunlit_bnd": ("dark13", [SUN, BND]), "sunlit_per_gpoint": ("dark13", [SUN, PERG]), "sunlit_cloud": ("dark13", [SUN, CLOUD]),
                "sunlit_aerosol": ("dark13", [SUN, AER]), "sunlit_spherical": ("dark13", [SUN, SPH]),
                "sunlit_spherical_bnd_byband": ("dark13", [SUN, SPH, BND, BYBAND])})
    return out


def write_cases(top):
    """One working directory per input variant; they differ in mu0 only."""
    rng = np.random.default_rng(4242)
    kw = dict(ngpt=NGPT, nbnd=NBND, npres=12, nflav=4, nminor_lower=7, nminor_upper=4)
    kl, ks = synthetic.make_kdist("lw", **kw), synthetic.make_kdist("sw", **kw)
    atm = synthetic.make_atmosphere(NCOL, NLAY, nbnd_lw=NBND, nbnd_sw=NBND, clouds=True, aerosols=True, seed=7)
    f = rng.uniform(0.65, 1.35, NCOL)
    atm.p_lay = np.ascontiguousarray(atm.p_lay * f); atm.p_lev = np.ascontiguousarray(atm.p_lev * f)
    frac = rng.uniform(0., 1., (NLAY, NCOL)) * ((atm.lwp + atm.iwp) > 0)
    alpha = rng.uniform(0.2, 0.9, (NLAY-1, NCOL))
    z_lay = np.repeat(((np.arange(NLAY) + 0.5) * (70.e3 / NLAY))[:, None], NCOL, axis=1) + rng.uniform(0., 500., NCOL)[None, :] + 600.
    z_ref = rng.uniform(0., 600., NCOL)
    order, mu0 = rng.permutation(NCOL), atm.mu0.copy()
    dirs = {}
    for variant, ndark in (("lit", 0), ("dark13", NDARK), ("dark45", NCOL)):
        atm.mu0 = mu0.copy()
        atm.mu0[order[:ndark]] = np.where(np.arange(ndark) % 2 == 0, 0.0, -0.3)
        dirs[variant] = os.path.join(top, variant)
        synthetic_files.write_case(dirs[variant], atm, kl, ks, synthetic.make_cloud_lut(NBND, "lw"), synthetic.make_cloud_lut(NBND, "sw"),
                                   synthetic.make_aerosol_lut(NBND), cloud_frac=frac, overlap_param=alpha, z_lay=z_lay, z_ref=z_ref)
    return dirs


def run_precision(sfx):
    lib = ctypes.CDLL(os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", f"librte_rrtmgp_hip{sfx}.so"))
    # (the driver's own messages go to its standard output: only the digest lines leave through the saved one)
    sys.stdout.flush()
    lines = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    with tempfile.TemporaryDirectory() as top:
        dirs = write_cases(top)
        for name, (variant, flags) in flag_sets().items():
            for block in ("7", "16384"):
                for device_sort in (False, True):
                    argv = [b"test_rte_rrtmgp_gpu"] + [a.encode() for a in flags + (["--device-sort-columns"] if device_sort else [])]
                    out = os.path.join(dirs[variant], "rte_rrtmgp_output.nc")
                    if os.path.exists(out):
                        os.remove(out)
                    os.environ["RRX_COL_BLOCK"] = block
                    os.chdir(dirs[variant])
                    status = lib.rrx_host_main(len(argv), (ctypes.c_char_p * len(argv))(*argv))
                    os.chdir(ROOT)
                    line = {"dtype": "f32" if sfx else "f64", "case": name, "col_block": int(block), "device_sort": device_sort, "status": status}
                    if status == 0:
                        for k, (a, _) in sorted(rrxio.read(out)[1].items()):
                            line[k] = hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=6).hexdigest()
                    lines.write(json.dumps(line, separators=(",", ":")) + "\n"); lines.flush()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        run_precision({"dp": "", "sp": "_sp"}[sys.argv[1]])
    else:
        for p in ("dp", "sp"):
            subprocess.run([sys.executable, os.path.abspath(__file__), p], check=True)
