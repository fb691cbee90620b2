"""numpy restatement of the backward tracer with the rays of all g-points in one launch (the SPECTRAL instantiation of
csrc/rrx_raytracer_bw.hip), in the scene's precision. What is stated here is the spectral form's own:
  - the allocation's ray list: ray_end, weight0 and the common unit U (ray_list);
  - the ranges per g-point of a range of the list (raytracer_spectral_ref.ranges_by_gpt: the kernel's search);
  - the tally by band: counts (nbnd, npix), the counts of g-point g added into row band(g);
  - the channel matrix (channels).
The transport of a ray is that of ray q of g-point g in raytracer_bw_ref.trace_counts_bw, called with weight0[g]: the deposit is
llrint(min(d weight0[g], 2^20) 2^32) there, clamped AFTER the weight."""
import numpy as np

import raytracer_ref as R
import raytracer_bw_ref as B
from raytracer_spectral_ref import ranges_by_gpt


def ray_list(scene, sensor, m):
    """ray_end (ngpt+1,) int64, weight0 (ngpt,) in the scene's precision, and U = S / P: what rrx_camera_render_spectral forms from m
    (ngpt,) rays per pixel. weight0[g] = (inc_dir[g] / F(m_g)) / (S / F(P)); S sums inc_dir[g] over m_g > 0 in index order."""
    dt = scene.dtype
    F = dt.type
    m = np.asarray(m, dtype=np.int64)
    ngpt = scene.tau.shape[0]
    npix = int(sensor.npx)*int(sensor.npy)
    ray_end = np.zeros(ngpt + 1, dtype=np.int64)
    ray_end[1:] = np.cumsum(m*npix)
    P, S = int(m.sum()), F(0.)
    for g in range(ngpt):
        if m[g] > 0:
            S = S + F(scene.inc_dir[g])
    U = S / F(P)
    weight0 = np.zeros(ngpt, dtype=dt)
    for g in range(ngpt):
        if m[g] > 0:
            weight0[g] = (F(scene.inc_dir[g]) / F(m[g])) / U
    return ray_end, weight0, U


def trace_counts(scene, bg, sensor, ray_end, weight0, ray0, nrays, max_events=1 << 20, table=None):
    """rrx_camera_trace_counts_spectral: counts (nbnd, npix) uint64, n_dep (nbnd, npix), n_capped, n_clamped and events, added in
    integers over the g-points that the range meets"""
    npix = int(sensor.npx)*int(sensor.npy)
    nbnd = len(scene.band_lims)
    band = R.band_of_gpt(scene.band_lims, scene.tau.shape[0])
    out = dict(counts=np.zeros((nbnd, npix), dtype=np.uint64), n_dep=np.zeros((nbnd, npix), dtype=np.int64), n_capped=0, n_clamped=0,
               events=0)
    for g, q0, n in ranges_by_gpt(ray_end, ray0, nrays):
        c = B.trace_counts_bw(scene, sensor, g, q0, n, max_events, table=table, bg=bg, weight0=weight0[g])
        b = int(band[g])
        if b >= 0:
            out["counts"][b] = out["counts"][b] + c["counts"]
            out["n_dep"][b] += c["n_dep"]
        for k in ("n_capped", "n_clamped", "events"):
            out[k] += c[k]
    return out


def channels(counts, M, scale, dtype):
    """rrx_camera_channels: out[c, pix] = scale sum_b M[c, b] (counts[b, pix] 2^-32), the sum in band order in the precision dtype"""
    F = np.dtype(dtype).type
    M = np.asarray(M, dtype=dtype)
    x = (counts.astype(np.float64) * 2.3283064365386963e-10).astype(dtype)
    out = np.zeros((M.shape[0], counts.shape[1]), dtype=dtype)
    for c in range(M.shape[0]):
        total = np.zeros(counts.shape[1], dtype=dtype)
        for b in range(M.shape[1]):
            total = total + M[c, b]*x[b]
        out[c] = F(scale)*total
    return out


def render(scene, bg, sensor, m, M, max_events=1 << 20, table=None):
    """rrx_camera_render_spectral: radiance (nchan, npix) from one conversion with scale = U / mu0; also the counts, n_dep, U and
    weight0"""
    F = scene.dtype.type
    ray_end, weight0, U = ray_list(scene, sensor, m)
    c = trace_counts(scene, bg, sensor, ray_end, weight0, 0, int(ray_end[-1]), max_events, table)
    c.update(radiance=channels(c["counts"], M, U / F(scene.mu0), scene.dtype), U=U, weight0=weight0)
    return c
