"""numpy restatement of the thermal tracer with the rays of all g-points in one launch (the SPECTRAL instantiation of
csrc/rrx_raytracer_thermal.hip), in the scene's precision. What is stated here is the spectral form's own:
  - the allocation's ray list: ray_end, weight0 and the common unit U (ray_list);
  - the scaled scene: the three source arrays multiplied by weight0[g] in the scene's precision (scaled_scene). The device scales the
    source that a deposit reads, and scales it first, so that the transport and the deposits of ray q of g-point g are those of
    raytracer_thermal_ref.trace_counts_thermal, called unchanged on the scaled scene;
  - the ranges per g-point of a range of the list (raytracer_spectral_ref.ranges_by_gpt: the kernel's search);
  - the tally by band: counts (nbnd, npix), the counts of g-point g added into row band(g);
  - the channel matrix (raytracer_bw_spectral_ref.channels) with scale = U."""
import numpy as np

import raytracer_ref as R
import raytracer_thermal_ref as T
from raytracer_bw_spectral_ref import channels
from raytracer_spectral_ref import ranges_by_gpt


def ray_list(scene, sensor, m):
    """ray_end (ngpt+1,) int64, weight0 (ngpt,) in the scene's precision, and U: what rrx_thermal_render_spectral forms from m (ngpt,)
    rays per pixel. weight0[g] = (F(1) / F(m_g)) / U, U = F(n_act) / F(P), n_act the number of g-points with m_g > 0, P = sum(m)."""
    dt = scene.dtype
    F = dt.type
    m = np.asarray(m, dtype=np.int64)
    ngpt = scene.tau.shape[0]
    npix = int(sensor.npx)*int(sensor.npy)
    ray_end = np.zeros(ngpt + 1, dtype=np.int64)
    ray_end[1:] = np.cumsum(m*npix)
    P, n_act = int(m.sum()), int((m > 0).sum())
    U = F(n_act) / F(P)
    weight0 = np.zeros(ngpt, dtype=dt)
    for g in range(ngpt):
        if m[g] > 0:
            weight0[g] = (F(1.) / F(m[g])) / U
    return ray_end, weight0, U


def scaled_scene(scene, weight0):
    """the ThermalScene whose lay_src, sfc_src and top_radiance of g-point g are multiplied by weight0[g], each product rounded once
    in the scene's precision"""
    dt = scene.dtype
    w = np.asarray(weight0, dtype=dt)
    out = T.ThermalScene(scene.medium, (scene.lay_src.astype(dt)*w[:, None, None]).astype(dt), (scene.sfc_src.astype(dt)*w[:, None]).astype(dt),
                         scene.sfc_emis, (np.asarray(scene.top_radiance, dtype=dt)*w).astype(dt))
    out.gas_scatters = getattr(scene, "gas_scatters", True)
    return out


def trace_counts(scene, sensor, ray_end, weight0, ray0, nrays, max_events=1 << 20):
    """rrx_thermal_trace_counts_spectral: counts (nbnd, npix) uint64, n_dep (nbnd, npix), n_capped, n_clamped (of all g-points, in a
    band or not) and events, added in integers over the g-points that the range meets"""
    npix = int(sensor.npx)*int(sensor.npy)
    nbnd = len(scene.band_lims)
    band = R.band_of_gpt(scene.band_lims, scene.tau.shape[0])
    scaled = scaled_scene(scene, weight0)
    out = dict(counts=np.zeros((nbnd, npix), dtype=np.uint64), n_dep=np.zeros((nbnd, npix), dtype=np.int64), n_capped=0, n_clamped=0,
               events=0)
    for g, q0, n in ranges_by_gpt(ray_end, ray0, nrays):
        c = T.trace_counts_thermal(scaled, sensor, g, q0, n, max_events)
        b = int(band[g])
        if b >= 0:
            out["counts"][b] = out["counts"][b] + c["counts"]
            out["n_dep"][b] += c["n_dep"]
        for k in ("n_capped", "n_clamped", "events"):
            out[k] += c[k]
    return out


def render(scene, sensor, m, M, max_events=1 << 20):
    """rrx_thermal_render_spectral: radiance (nchan, npix) from one conversion with scale = U; also the counts, n_dep, U and weight0"""
    ray_end, weight0, U = ray_list(scene, sensor, m)
    c = trace_counts(scene, sensor, ray_end, weight0, 0, int(ray_end[-1]), max_events)
    c.update(radiance=channels(c["counts"], M, U, scene.dtype), U=U, weight0=weight0)
    return c
