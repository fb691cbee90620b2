"""Sensors of the backward ray tracer (rrx_rt_bw_trace_counts / rrx_raytracer_bw): a Camera holds the sensor type, the
image size and the 12 numbers the entries take (position, e_w, e_h, e_d), built here from yaw / pitch / roll.

Convention: x, y horizontal, z upward from the surface, metres. The viewing direction of yaw y and pitch p (radians) is
d = (cos p cos y, cos p sin y, sin p): yaw turns from +x towards +y, a negative pitch looks down. With z up the viewer's right is
r0 = d x z / |d x z| = (sin y, -cos y, 0) and the viewer's up is u0 = r0 x d; a roll by q about d turns them to
r = r0 cos q + u0 sin q, u = -r0 sin q + u0 cos q. Across the image a in [0, 1] runs along r (pixel column ipx) and b along u (pixel row
ipy: row 0 is the bottom of the picture)."""
import math
from dataclasses import dataclass

import numpy as np

PERSPECTIVE, FISHEYE, ORTHOGRAPHIC, FLUX = 0, 1, 2, 3


@dataclass
class Camera:
    type: int
    npx: int
    npy: int
    fov: float
    position: tuple
    e_w: tuple
    e_h: tuple
    e_d: tuple

    @property
    def npix(self):
        return self.npx * self.npy

    def numbers(self, dtype=np.float64):
        """position, e_w, e_h, e_d as the 12 host numbers of the C entries"""
        return np.ascontiguousarray(np.concatenate([self.position, self.e_w, self.e_h, self.e_d]).astype(dtype))


def view_axes(yaw, pitch, roll=0.0):
    """(right, up, direction): three orthonormal vectors"""
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    d = np.array([cp*cy, cp*sy, sp])
    r0 = np.array([sy, -cy, 0.0])
    u0 = np.cross(r0, d)
    cq, sq = math.cos(roll), math.sin(roll)
    return r0*cq + u0*sq, -r0*sq + u0*cq, d


def perspective(npx, npy, position, yaw, pitch, roll=0.0, fov=math.radians(60.), aspect=None):
    """A pinhole camera. fov: the full horizontal opening angle (< pi); aspect = width / height of the image plane (default
    npx / npy: square pixels). The ray of image point (a, b) has the direction e_w (2a - 1) + e_h (2b - 1) + e_d."""
    if not 0. < fov < math.pi:
        raise ValueError("perspective: fov must be in (0, pi)")
    aspect = npx / npy if aspect is None else float(aspect)
    r, u, d = view_axes(yaw, pitch, roll)
    half = math.tan(0.5*fov)
    return Camera(PERSPECTIVE, int(npx), int(npy), float(fov), tuple(map(float, position)), tuple(r*half), tuple(u*(half/aspect)), tuple(d))


def fisheye(npx, npy, position, yaw=0.0, pitch=0.5*math.pi, roll=0.0, fov=math.pi):
    """An equidistant fisheye about the viewing direction (default the zenith): pixel column -> angle from the axis, a fov / 2, pixel
    row -> angle about the axis, 2 pi b. fov: the full opening angle, up to 2 pi."""
    r, u, d = view_axes(yaw, pitch, roll)
    return Camera(FISHEYE, int(npx), int(npy), float(fov), tuple(map(float, position)), tuple(r), tuple(u), tuple(d))


def orthographic(npx, npy, yaw=0.0, pitch=-0.5*math.pi, roll=0.0):
    """Parallel rays along the viewing direction (it must look down: pitch < 0) from the whole domain top: image point (a, b) starts
    at (a Lx, b Ly, top). The default is the nadir view of a satellite."""
    r, u, d = view_axes(yaw, pitch, roll)
    if not d[2] < 0.:
        raise ValueError("orthographic: the viewing direction must point downward (pitch < 0)")
    return Camera(ORTHOGRAPHIC, int(npx), int(npy), 0.0, (0., 0., 0.), tuple(r), tuple(u), tuple(d / np.linalg.norm(d)))


def flux_sensor(npx, npy, up=True):
    """Cosine-weighted rays from every point of the surface, facing up (downwelling irradiance = pi x radiance), or from every point of
    the domain top, facing down (upwelling irradiance)."""
    return Camera(FLUX, int(npx), int(npy), 0.0, (0., 0., 0.), (1., 0., 0.), (0., 1., 0.), (0., 0., 1. if up else -1.))


def _planck_wavenumber(nu, t):
    """Planck's law per unit wavenumber nu (cm-1) at temperature t (K), up to a constant factor"""
    return nu**3 / np.expm1(1.4387768775 * nu / t)


def band_weights(band_lims_wavenumber, wavelength_nm, response, t_sun=5772.0):
    """M (nchan, nbnd), the matrix from the bands of a k-distribution to the channels of a sensor (render_sw(channels=M)).
    M[c, b] is the share of band b's solar energy that response curve c passes: the integral of response x Planck(t_sun) over the band
    divided by the integral of Planck(t_sun) over the band, by the trapezoid rule in wavenumber on a grid that is halved until both
    integrals stand to 1e-10.

    band_lims_wavenumber (nbnd, 2) in cm-1, as a k-distribution holds them. wavelength_nm (nw,) ascending; two equal wavelengths
    make a step. response (nchan, nw) or (nw,): the curves at those wavelengths, linear in wavelength between them and zero outside
    [wavelength_nm[0], wavelength_nm[-1]]. The user brings the curves: colour-matching functions, a satellite's filter, a
    pyranometer's window. Colour made from the shortwave bands of a k-distribution is as coarse as its visible bands are: a
    k-distribution with two or three bands between 400 and 700 nm tells hues apart no better than that."""
    lims = np.asarray(band_lims_wavenumber, dtype=np.float64).reshape(-1, 2)
    lam = np.asarray(wavelength_nm, dtype=np.float64).reshape(-1)
    resp = np.atleast_2d(np.asarray(response, dtype=np.float64))
    if lam.size < 2 or np.any(lam <= 0.) or np.any(np.diff(lam) < 0.):
        raise ValueError("band_weights: wavelength_nm holds at least two positive wavelengths that do not descend")
    if resp.shape[1] != lam.size:
        raise ValueError(f"band_weights: response is (nchan, nw = {lam.size}), got {resp.shape}")
    if np.any(lims <= 0.) or not t_sun > 0.:
        raise ValueError("band_weights: band limits and t_sun must be > 0")
    nu_nodes = 1.0e7 / lam
    M = np.zeros((resp.shape[0], lims.shape[0]))
    for b, (lo, hi) in enumerate(np.sort(lims, axis=1)):
        inside = nu_nodes[(nu_nodes > lo) & (nu_nodes < hi)]
        edges = np.unique(np.concatenate([[lo, hi], inside]))
        den, num = 0.0, np.zeros(resp.shape[0])
        for p0, p1 in zip(edges[:-1], edges[1:]):
            # the piece lies inside one segment of the curves (or outside them): the segment of its midpoint
            lam_mid = 1.0e7 / (0.5*(p0 + p1))
            k = int(np.searchsorted(lam, lam_mid, side="right")) - 1
            covered = lam[0] <= lam_mid <= lam[-1] and 0 <= k < lam.size - 1 and lam[k+1] > lam[k]
            n, last = 8, None
            while True:
                nu = np.linspace(p0, p1, n + 1)
                planck = _planck_wavenumber(nu, float(t_sun))
                w = np.full(n + 1, (p1 - p0)/n); w[0] *= 0.5; w[-1] *= 0.5
                if covered:
                    f = (np.clip(1.0e7/nu, lam[k], lam[k+1]) - lam[k]) / (lam[k+1] - lam[k])
                    r = resp[:, k:k+1]*(1.0 - f) + resp[:, k+1:k+2]*f
                else:
                    r = np.zeros((resp.shape[0], n + 1))
                now = np.concatenate([[np.sum(planck*w)], (r*planck) @ w])
                if last is not None and np.all(np.abs(now - last) <= 1e-10*np.abs(now[0])) or n >= 1 << 16:
                    break
                n, last = 2*n, now
            den += now[0]
            num += now[1:]
        M[:, b] = num / den
    return M
