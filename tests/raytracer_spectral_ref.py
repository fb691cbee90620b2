"""numpy restatement of the forward tracer with all g-points in one launch (the SPECTRAL instantiation of csrc/rrx_raytracer.hip,
csrc/rrx_rt_common.h), in the scene's precision. What is stated here is the spectral form's own:
  - the allocation's photon list: photon_end, weight0, dif_frac and the common unit U (photon_list);
  - the g-point and the local index of a global photon index (gpt_of_photon, the kernel's search, and its ranges);
  - the sum in integers over the g-points that a range meets, and the one conversion to fluxes with U.
The transport of a photon is that of photon q of g-point g in raytracer_ref.trace_counts, called with weight0[g]: every
to_count(w) of the tallies becomes to_count(w weight0[g]) there."""
import numpy as np

import raytracer_ref as R


def photon_list(scene, m):
    """photon_end (ngpt+1,) int64, weight0, dif_frac (ngpt,) in the scene's precision, and U = S / P: what rrx_raytracer_sw_spectral
    forms from m (ngpt,) photons per pixel. weight0[g] = (inc_g / F(m_g)) / (S / F(P)); S sums inc_g over m_g > 0 in index order."""
    dt = scene.dtype
    F = dt.type
    m = np.asarray(m, dtype=np.int64)
    ngpt = scene.tau.shape[0]
    photon_end = np.zeros(ngpt + 1, dtype=np.int64)
    photon_end[1:] = np.cumsum(m*scene.ncol)
    P, S = int(m.sum()), F(0.)
    for g in range(ngpt):
        if m[g] > 0:
            S = S + (F(scene.inc_dir[g]) + F(scene.inc_dif[g]))
    U = S / F(P)
    weight0, dif_frac = np.zeros(ngpt, dtype=dt), np.zeros(ngpt, dtype=dt)
    for g in range(ngpt):
        if m[g] > 0:
            inc = F(scene.inc_dir[g]) + F(scene.inc_dif[g])
            weight0[g] = (inc / F(m[g])) / U
            dif_frac[g] = F(scene.inc_dif[g]) / inc
    return photon_end, weight0, dif_frac, U


def gpt_of_photon(photon_end, p):
    """the kernel's search: the smallest g with photon_end[g+1] > p (empty ranges are stepped over); ngpt beyond the list"""
    lo, hi = 0, len(photon_end) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if photon_end[mid + 1] <= p:
            lo = mid + 1
        else:
            hi = mid
    return lo


def ranges_by_gpt(photon_end, photon0, nphotons):
    """[(g, q0, n)]: the local ranges [q0, q0 + n) of the g-points that the global range [photon0, photon0 + nphotons) meets"""
    out = []
    p, end = int(photon0), int(photon0) + int(nphotons)
    while p < end:
        g = gpt_of_photon(photon_end, p)
        if g >= len(photon_end) - 1:
            break
        stop = min(end, int(photon_end[g + 1]))
        out.append((g, p - int(photon_end[g]), stop - p))
        p = stop
    return out


def trace_counts(scene, bg, photon_end, weight0, photon0, nphotons, max_events=1 << 20, table=None):
    """rrx_rt_trace_counts_spectral: the counts of raytracer_ref.trace_counts, added in integers over the g-points that the range
    meets, every deposit weighted; n_capped and events are sums too. (dif_frac is the scene's own inc_dif / (inc_dir + inc_dif),
    which raytracer_ref.trace_counts forms per g-point.)"""
    out = R.tallies(scene, bg, np.uint64)
    out["n_capped"], out["events"] = 0, 0
    for g, q0, n in ranges_by_gpt(photon_end, photon0, nphotons):
        c = R.trace_counts(scene, g, q0, n, max_events, table, bg, weight0[g])
        for k in R.ALL_COUNTS + ("n_capped", "events"):
            out[k] = out[k] + c[k]
    return out


def raytracer_sw(scene, bg, m, max_events=1 << 20, table=None):
    """rrx_raytracer_sw_spectral: the fluxes of raytracer_ref.raytracer_sw from one conversion with the common unit U"""
    photon_end, weight0, _, U = photon_list(scene, m)
    c = trace_counts(scene, bg, photon_end, weight0, 0, int(photon_end[-1]), max_events, table)
    flux = R.tallies(scene, bg, scene.dtype)
    R.add_fluxes(flux, c, U, scene, bg)
    flux["n_capped"], flux["events"], flux["U"], flux["weight0"] = c["n_capped"], c["events"], U, weight0
    return flux
