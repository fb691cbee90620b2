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
