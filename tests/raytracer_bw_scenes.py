"""The fixed-seed scenes, sensors and comparisons of the backward ray tracer tests (test_raytracer_bw_ref.py on the numpy
restatement, test_gpu_raytracer_bw.py on the GPU), on the scenes of raytracer_scenes.py.

S1 Bernoulli surface: horizontally uniform absorbing layers, k_null grid = grid (the first collision kills: f_no_abs = 0), uniform
   albedo 0.4, orthographic sensors. A ray reaches the surface with probability p = exp(-tau/|e_d.z|) and then deposits exactly
   c = albedo mu0/pi exp(-tau/mu0): counts/(N c 2^32) is a Bernoulli mean, standard deviation sqrt(p (1 - p)/N).
S2 shadow: the opaque block of raytracer_scenes.shadow over albedo 0.5 under a nadir orthographic camera of nx x ny pixels: integers.
S3 forward against backward: the general scene without diffuse incident light; flux sensors of nx x ny pixels at the surface
   (facing up) and at the top (facing down) against the forward tracer's sfc_dn_dif and tod_up."""
import math

import numpy as np

import raytracer_scenes as S
import raytracer_bw_ref as B

ONE = float(1 << 32)
S1_RAYS = 4096                     # per pixel
S1_ALBEDO = 0.4
S3_RANGES = 16
S3_RAYS = 16*64                    # backward rays per pixel, in 16 disjoint ranges of 64 per pixel
S3_PHOTONS = 1024                  # forward photons per pixel


def bernoulli(dtype):
    sc = S.slant(dtype)
    sc.sfc_albedo = np.full(sc.ncol, S1_ALBEDO, dtype=dtype)
    sc.kn_grid = (sc.nx, sc.ny, sc.nz)
    sc.seed = S.SEED + 11
    return sc


def bernoulli_sensors():
    return {"nadir": B.orthographic(4, 4, (0., 0., -1.)), "slant": B.orthographic(4, 4, (0.5, -0.3, -0.8))}


def bernoulli_expected(sc, sensor, igpt):
    """(p, c) in float64"""
    tau = float(sc.tau[igpt].astype(np.float64).sum(axis=0)[0])
    mu0 = float(sc.dtype.type(sc.mu0))
    return math.exp(-tau/abs(sensor.e_d[2])), S1_ALBEDO*mu0/math.pi*math.exp(-tau/mu0)


def check_bernoulli(sc, sensor, igpt, counts, label):
    """every pixel and the image mean within 5 sigma; returns the worst deviation in sigmas"""
    p, c = bernoulli_expected(sc, sensor, igpt)
    got = counts.astype(np.float64) / (S1_RAYS*c*ONE)
    dev = np.abs(got - p) / S.sigma(p, S1_RAYS)
    dev_mean = abs(got.mean() - p) / S.sigma(p, S1_RAYS*counts.size)
    worst = max(float(dev.max()), float(dev_mean))
    print(f"raytracer_bw S1 {label} g-point {igpt}: p = {p:.4f}, worst deviation {worst:.2f} sigma (bound 5)")
    assert np.all(dev <= 5) and dev_mean <= 5, (label, igpt, worst)
    return worst


def shadow(dtype, along, top_at_1):
    sc = S.shadow(dtype, along, top_at_1)
    sc.sfc_albedo = np.full(sc.ncol, 0.5, dtype=dtype)
    return sc


def shadow_classes(sc):
    """(dark, full): the pixels that must count 0 (above the block: the camera's own ray dies in it with probability 1 - e^-50; or
    with every sun path of the pixel longer than tau = 40: llrint(e^-40 2^32) = 0), and the pixels that must count full (no sun path
    of the pixel touches the block, and the pixel is not above it). The pixels at the shadow's two edges belong to neither."""
    import raytracer_ref as R
    lo, hi = R.pixel_path_range(sc, 0)
    above = (sc.tau[0].sum(axis=0) > 0)
    return above | (lo > 40.0), (hi == 0.0) & ~above


def shadow_full_count(sc, rays):
    F = sc.dtype.type
    d = (F(0.5)*F(sc.mu0)) / F(B.PI)
    return rays * int(np.rint(np.float64(d) * ONE))


def general_direct(dtype):
    sc = S.general(dtype)
    sc.inc_dif = np.zeros_like(sc.inc_dif)
    return sc


def flux_sensors(sc):
    """sensor -> the forward tally it measures"""
    return {"sfc_dn_dif": B.flux_sensor(sc.nx, sc.ny, True), "tod_up": B.flux_sensor(sc.nx, sc.ny, False)}


def compare_forward_backward(sc, igpt, name, forward_counts, range_counts, label):
    """forward_counts: the forward tally `name` (ncol,) of S3_PHOTONS photons per pixel; range_counts: (S3_RANGES, ncol) backward
    counts of S3_RAYS/S3_RANGES rays per pixel each. Irradiances in W m-2, per pixel and domain mean: the forward side gets the derived
    bound (a per-photon contribution in [0, 1] with mean p: sqrt(p (1 - p)/N); for sfc_dn_dif a photon that the surface reflects may
    come down again, so this is the bound of the first arrival), the backward side the standard error of its 16 range means; the
    difference is allowed 5 combined sigma. Returns the worst difference in combined sigmas."""
    inc, mu0, ncol = float(sc.inc_dir[igpt]), float(sc.dtype.type(sc.mu0)), sc.ncol
    n_f = S3_PHOTONS*ncol
    p = forward_counts.astype(np.float64) / ONE / n_f
    f_pix, s_pix = p*ncol*inc, ncol*inc*S.sigma(p, n_f)
    f_mean, s_mean = p.sum()*inc, inc*S.sigma(p.sum(), n_f)
    e = math.pi * range_counts.astype(np.float64) / ONE / (S3_RAYS//S3_RANGES) * inc/mu0          # (ranges, ncol)
    b_pix, se_pix = e.mean(axis=0), e.std(axis=0, ddof=1) / math.sqrt(S3_RANGES)
    em = e.mean(axis=1)
    b_mean, se_mean = em.mean(), em.std(ddof=1) / math.sqrt(S3_RANGES)
    dev_pix = np.abs(b_pix - f_pix) / np.sqrt(s_pix**2 + se_pix**2)
    dev_mean = abs(b_mean - f_mean) / math.sqrt(s_mean**2 + se_mean**2)
    print(f"raytracer_bw S3 {label} {name} g-point {igpt}: domain mean backward {b_mean:.2f} +- {se_mean:.2f} against forward "
          f"{f_mean:.2f} +- {s_mean:.2f} W m-2 ({dev_mean:.2f} sigma); worst pixel {float(dev_pix.max()):.2f} sigma (bound 5)")
    assert f_mean > 0 and b_mean > 0
    assert dev_mean <= 5 and np.all(dev_pix <= 5), (label, name, igpt, dev_mean, float(dev_pix.max()))
    return max(float(dev_mean), float(dev_pix.max()))
