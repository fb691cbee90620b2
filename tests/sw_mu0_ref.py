"""NumPy reference of the spherical-geometry correction of the solar zenith angle (rrx_zenith_angle_spherical_correction; upstream
RTE's zenith_angle_spherical_correction) and the seeded inputs of the mu0-by-layer solver tests.

    mu(c, l) = sqrt(max(0, 1 - (1 - ref_mu(c)^2) ((R + ref_alt(c)) / (R + alt(c, l)))^2))      where ref_mu(c) > 0
    mu(c, l) = ref_mu(c)                                                                       otherwise (a dark column stays dark)

Arrays are numpy C order with the column last: alt and the result (nlay, ncol), ref_mu and ref_alt (ncol). Every operation is done in
the precision of ref_mu, one at a time in the order of the formula, like the kernel."""
import numpy as np

EARTH_RADIUS = 6.37123e6


def spherical_mu0(ref_mu, alt, ref_alt=None, planet_radius=EARTH_RADIUS):
    F = np.asarray(ref_mu).dtype.type
    ref_mu = np.asarray(ref_mu)
    alt = np.asarray(alt, dtype=F)
    R = F(planet_radius)
    r0 = R + (np.zeros_like(ref_mu) if ref_alt is None else np.asarray(ref_alt, dtype=F))
    sin2 = F(1.) - ref_mu*ref_mu
    ratio = r0[None, :] / (R + alt)
    c2 = F(1.) - sin2[None, :]*(ratio*ratio)
    mu = np.sqrt(np.maximum(F(0.), c2))
    return np.where(ref_mu[None, :] > 0, mu, np.broadcast_to(ref_mu[None, :], mu.shape)).astype(F)


def solver_inputs(seed, ncol, nlay, ngpt):
    """fp64 inputs drawn like the random golden case (oracle/make_golden.py:random_solver_case: optical depths over eight decades, one
    transparent layer, a conservative and a non-scattering g-point where there are that many), with the cosine drawn independently
    per layer and column from that case's [0.05, 1]."""
    rng = np.random.default_rng(seed)
    shp = (ngpt, nlay, ncol)
    d = dict(tau=10.0**rng.uniform(-6, 2, shp), ssa=rng.uniform(0., 1., shp), g=rng.uniform(-0.3, 0.9, shp),
             mu0_lay=rng.uniform(0.05, 1.0, (nlay, ncol)), adif=rng.uniform(0., 0.6, (ngpt, ncol)), inc=rng.uniform(0., 5., (ngpt, ncol)),
             inc_dif=rng.uniform(0., 1., (ngpt, ncol)))
    d["adir"] = np.ascontiguousarray(np.repeat(rng.uniform(0., 0.6, ncol)[None, :], ngpt, axis=0))
    d["tau"][0, 0, :] = 0.0
    if ngpt > 1:
        d["ssa"][1, :, :] = 1.0
    if ngpt > 2:
        d["ssa"][2, :, :] = 0.0
    return d
