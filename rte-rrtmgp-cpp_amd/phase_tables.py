"""Tabulated cloud phase functions for the two ray tracers (the specification: csrc/rrx_rt_phase.h).

A table is nmu nodes mu[0] = -1 < ... < mu[nmu-1] = +1 (cosines of the scattering angle, dense near +1) and, per band and effective
radius re0 + dre ire, the phase function at the nodes, piecewise linear in mu between them. build() normalises raw values on the
device (rrx_rt_phase_tables) and returns a PhaseTable; with_radius() attaches the cells' radius, which is what the `phase=` argument
of HipKernels.rt_trace_counts / raytracer_sw / rt_bw_trace_counts / raytracer_bw and `phase_table=` of pipeline.raytrace_sw /
render_sw take. Raw arrays are (nbnd, nre, nmu) in the package's tensor convention (the memory of phase(nmu, nre, nbnd))."""
from dataclasses import dataclass, replace
from typing import Any, Optional

import numpy as np

from . import rrxio

# the radius grid of the reference's Mie files: 2.5 + 1 i micron
MIE_RE0, MIE_DRE = 2.5, 1.0


@dataclass
class PhaseTable:
    mu: Any                 # (nmu,)
    phase: Any              # (nbnd, nre, nmu), 1/2 int P dmu = 1
    cdf: Any                # (nbnd, nre, nmu), 0 at mu = -1, 1 at mu = +1
    re0: float
    dre: float
    cld_re: Optional[Any] = None          # (nz, ncol): the cells' radius, in the unit of re0 and dre

    @property
    def nmu(self):
        return int(self.mu.shape[0])

    @property
    def nre(self):
        return int(self.phase.shape[1])

    @property
    def nbnd(self):
        return int(self.phase.shape[0])

    def with_radius(self, cld_re):
        return replace(self, cld_re=cld_re)


def build(be, mu, phase_raw, re0=MIE_RE0, dre=MIE_DRE):
    """The normalised tables of phase_raw (nbnd, nre, nmu) >= 0 on the nodes mu, on the backend's device."""
    phase_raw = np.asarray(phase_raw)
    if phase_raw.ndim != 3 or phase_raw.shape[2] != np.asarray(mu).shape[0]:
        raise ValueError(f"phase_tables.build: phase_raw is (nbnd, nre, nmu), got {phase_raw.shape} for {np.asarray(mu).shape[0]} nodes")
    mu_d, raw_d = be.asarray(np.asarray(mu, dtype=np.float64)), be.asarray(phase_raw.astype(np.float64))
    phase, cdf = be.rt_phase_tables(mu_d, raw_d)
    return PhaseTable(mu=mu_d, phase=phase, cdf=cdf, re0=float(re0), dre=float(dre))


def nodes(nmu, power=2.0):
    """nmu cosines from -1 to +1 whose spacing shrinks towards +1: mu = 1 - 2 (1 - x)^power on a uniform x (both ends exact). The
    last spacing is 2/(nmu-1)^power; in fp32 it must stay above a few steps of 6e-8, or two nodes round to the same number and
    rrx_rt_phase_tables refuses them (power 2 allows 4096 nodes, power 3 about 200)."""
    x = np.linspace(0.0, 1.0, nmu)
    mu = 1.0 - 2.0*(1.0 - x)**power
    mu[0], mu[-1] = -1.0, 1.0
    return mu


def henyey_greenstein(mu, g):
    mu = np.asarray(mu, dtype=np.float64)
    return (1.0 - g*g) / (1.0 + g*g - 2.0*g*mu)**1.5


def double_hg(mu, g1, g2, share):
    """share HG(g1) + (1 - share) HG(g2): a forward peak and a backward lobe with g2 < 0"""
    return share*henyey_greenstein(mu, g1) + (1.0 - share)*henyey_greenstein(mu, g2)


def from_angles(angle, phase, degrees=True):
    """An ascending-angle table, as in the reference's Mie files (0 = forward), to ascending-mu nodes: returns (mu, phase) with the
    last axis of phase reversed. The ends are moved onto mu = +1 / -1 exactly when the angles reach 0 / 180 degrees to rounding;
    angles that do not span [0, 180] are an error (the table is defined on the whole interval)."""
    angle = np.asarray(angle, dtype=np.float64)
    phase = np.asarray(phase)
    if angle.ndim != 1 or phase.shape[-1] != angle.shape[0] or np.any(np.diff(angle) <= 0):
        raise ValueError("phase_tables.from_angles: angle must be strictly ascending and match the last axis of phase")
    rad = np.deg2rad(angle) if degrees else angle
    if abs(rad[0]) > 1e-9 or abs(rad[-1] - np.pi) > 1e-9:
        raise ValueError("phase_tables.from_angles: the angles must run from 0 to 180 degrees")
    mu = np.cos(rad)[::-1].copy()
    mu[0], mu[-1] = -1.0, 1.0
    if np.any(np.diff(mu) <= 0):
        raise ValueError("phase_tables.from_angles: two angles give the same cosine")
    return mu, np.ascontiguousarray(phase[..., ::-1])


def read_mie(path, re0=MIE_RE0, dre=MIE_DRE):
    """The reference's Mie file layout in the RRXB container: phase(band, r_eff, n_ang) and phase_angle(n_ang) in degrees, ascending
    from 0. Returns (mu, phase_raw (nbnd, nre, nmu), re0, dre), ready for build()."""
    _, variables = rrxio.read(path)
    for name in ("phase", "phase_angle"):
        if name not in variables:
            raise ValueError(f"phase_tables.read_mie: {path} has no variable {name}")
    (phase, pdims), (angle, adims) = variables["phase"], variables["phase_angle"]
    if list(pdims) != ["band", "r_eff", "n_ang"] or list(adims) != ["n_ang"]:
        raise ValueError(f"phase_tables.read_mie: expected phase(band, r_eff, n_ang) and phase_angle(n_ang), got {pdims} and {adims}")
    mu, raw = from_angles(angle, phase)
    return mu, raw, float(re0), float(dre)
