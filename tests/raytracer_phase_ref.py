"""numpy restatement of the tabulated cloud phase functions of the ray tracers (csrc/rrx_rt_phase.h, rrx_rt_phase.hip):
the table builder, the index, the sampler and the evaluator in the entry's precision, operation for operation, and their longdouble
counterparts (the exact inverse and the exact density of the table that is stored). The table specification only: the tracers'
restatements (raytracer_ref.py, raytracer_bw_ref.py) import it and take a Table with cld_re as their cloud species (table=).
Tables are in the package's tensor convention: phase, cdf (nbnd, nre, nmu)."""
from dataclasses import dataclass

import numpy as np

LD = np.longdouble


@dataclass
class Table:
    mu: np.ndarray          # (nmu,)
    phase: np.ndarray       # (nbnd, nre, nmu)
    cdf: np.ndarray
    re0: float
    dre: float
    cld_re: np.ndarray = None          # (nz, ncol)

    @property
    def nre(self):
        return self.phase.shape[1]


def nodes(nmu, power=2.0):
    x = np.linspace(0.0, 1.0, nmu)
    mu = 1.0 - 2.0*(1.0 - x)**power
    mu[0], mu[-1] = -1.0, 1.0
    return mu


def hg(mu, g):
    return (1.0 - g*g) / (1.0 + g*g - 2.0*g*np.asarray(mu, dtype=np.float64))**1.5


def double_hg(mu, g1, g2, share):
    return share*hg(mu, g1) + (1.0 - share)*hg(mu, g2)


def hg_cdf(mu, g):
    """1/2 int_{-1}^{mu} HG dmu', analytic"""
    mu = np.asarray(mu, dtype=np.float64)
    return (1.0 - g*g)/(2.0*g) * (1.0/np.sqrt(1.0 + g*g - 2.0*g*mu) - 1.0/(1.0 + g))


def build_tables(mu, phase_raw, dtype, re0=2.5, dre=1.0):
    """rrx_rt_phase_tables: the inputs are rounded to dtype as the device sees them; the trapezoid sums run in double in node order
    (np.cumsum adds sequentially), cdf = F(A_i/A_last), phase = F(raw/(A_last/2))."""
    mu = np.asarray(mu).astype(dtype)
    raw = np.asarray(phase_raw).astype(dtype)
    m, r = mu.astype(np.float64), raw.astype(np.float64)
    seg = (0.5*(r[..., :-1] + r[..., 1:]))*(m[1:] - m[:-1])
    A = np.cumsum(seg, axis=-1)
    total = A[..., -1:]
    cdf = np.concatenate([np.zeros_like(total), A/total], axis=-1).astype(dtype)
    phase = (r/(0.5*total)).astype(dtype)
    return Table(mu=mu, phase=np.ascontiguousarray(phase), cdf=np.ascontiguousarray(cdf), re0=re0, dre=dre)


def index(t, re):
    """(ire, jre, f) of phase_index, in the dtype of re"""
    dt = re.dtype
    F = dt.type
    if t.nre == 1:
        z = np.zeros(re.shape, dtype=np.int64)
        return z, z, np.zeros(re.shape, dtype=dt)
    with np.errstate(invalid="ignore"):
        q = (re - F(t.re0)) / F(t.dre)
        ire = np.fmin(np.fmax(q, F(0.)), F(t.nre - 2)).astype(np.int64)
        f = np.fmin(np.fmax(q - ire.astype(dt), F(0.)), F(1.))
    return ire, ire + 1, f


def sample(t, ibnd, re, u, with_interval=False):
    """phase_sample in the dtype of the table"""
    dt = t.mu.dtype
    F = dt.type
    re, u = np.asarray(re, dtype=dt), np.asarray(u, dtype=dt)
    C, P, mu = t.cdf[ibnd], t.phase[ibnd], t.mu
    ire, jre, f = index(t, re)
    lo = np.zeros(u.shape, dtype=np.int64)
    hi = np.full(u.shape, mu.size - 1, dtype=np.int64)
    while np.any(hi - lo > 1):
        act = hi - lo > 1
        mid = (lo + hi) >> 1
        a, b = C[ire, mid], C[jre, mid]
        le = (a + f*(b - a)) <= u
        lo = np.where(act & le, mid, lo)
        hi = np.where(act & ~le, mid, hi)
    ca, cb = C[ire, lo], C[jre, lo]
    c = ca + f*(cb - ca)
    pa0, pb0, pa1, pb1 = P[ire, lo], P[jre, lo], P[ire, lo+1], P[jre, lo+1]
    p0, p1 = pa0 + f*(pb0 - pa0), pa1 + f*(pb1 - pa1)
    m0, m1 = mu[lo], mu[lo+1]
    r = F(2.)*(u - c)
    s = (p1 - p0) / (m1 - m0)
    den = p0 + np.sqrt(np.maximum(F(0.), p0*p0 + (F(2.)*s)*r))
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = np.where(den > F(0.), (F(2.)*r)/den, F(0.)).astype(dt)
    out = np.minimum(np.maximum(m0 + tt, m0), m1).astype(dt)
    return (out, lo) if with_interval else out


def evaluate(t, ibnd, re, cs):
    """phase_eval in the dtype of the table (cs already in [-1, 1])"""
    dt = t.mu.dtype
    F = dt.type
    re, cs = np.asarray(re, dtype=dt), np.asarray(cs, dtype=dt)
    P, mu = t.phase[ibnd], t.mu
    ire, jre, f = index(t, re)
    lo = np.zeros(cs.shape, dtype=np.int64)
    hi = np.full(cs.shape, mu.size - 1, dtype=np.int64)
    while np.any(hi - lo > 1):
        act = hi - lo > 1
        mid = (lo + hi) >> 1
        le = mu[mid] <= cs
        lo = np.where(act & le, mid, lo)
        hi = np.where(act & ~le, mid, hi)
    m0, m1 = mu[lo], mu[lo+1]
    w = np.fmin(np.fmax((cs - m0) / (m1 - m0), F(0.)), F(1.))
    a0, a1, b0, b1 = P[ire, lo], P[ire, lo+1], P[jre, lo], P[jre, lo+1]
    pa, pb = a0 + w*(a1 - a0), b0 + w*(b1 - b0)
    return (pa + f*(pb - pa)).astype(dt)


# ---- longdouble: the exact inverse and density of the table as it is stored (rounded nodes, phase and cdf), with the index and the
# blend weight computed in longdouble from the same re0, dre

def _ld_blend(t, ibnd, re):
    """the blended phase function and CDF (nmu,) of ONE radius, in longdouble"""
    re = LD(re)
    ire, jre, f = 0, 0, LD(0.)
    if t.nre > 1:
        q = (re - LD(t.re0)) / LD(t.dre)
        if not np.isnan(q):
            ire = int(min(max(q, LD(0.)), LD(t.nre - 2)))
            f = min(max(q - LD(ire), LD(0.)), LD(1.))
        jre = ire + 1
    P, C = t.phase[ibnd].astype(LD), t.cdf[ibnd].astype(LD)
    return P[ire] + f*(P[jre] - P[ire]), C[ire] + f*(C[jre] - C[ire])


def _per_radius(fn, t, ibnd, re, x):
    """fn(mu, Pb, Cb, x) per distinct radius (a NaN radius is one of them)"""
    re, x = np.asarray(re), np.asarray(x).astype(LD)
    out = np.empty(x.shape, dtype=LD)
    mu = t.mu.astype(LD)
    key = np.where(np.isnan(re), -np.inf, re)
    for k in np.unique(key):
        sel = key == k
        Pb, Cb = _ld_blend(t, ibnd, np.nan if k == -np.inf else k)
        out[sel] = fn(mu, Pb, Cb, x[sel])
    return out


def sample_ld(t, ibnd, re, u):
    def fn(mu, Pb, Cb, u):
        i = np.clip(np.searchsorted(Cb, u, side="right") - 1, 0, mu.size - 2)
        r = LD(2.)*(u - Cb[i])
        p0, p1 = Pb[i], Pb[i+1]
        s = (p1 - p0) / (mu[i+1] - mu[i])
        den = p0 + np.sqrt(np.maximum(LD(0.), p0*p0 + LD(2.)*s*r))
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = np.where(den > 0, LD(2.)*r/den, LD(0.))
        return np.clip(mu[i] + tt, mu[i], mu[i+1])
    return _per_radius(fn, t, ibnd, re, u)


def cdf_ld(t, ibnd, re, cs):
    """C(cs) of the blended table: the stored node values plus the exact integral of the linear piece"""
    def fn(mu, Pb, Cb, cs):
        i = np.clip(np.searchsorted(mu, cs, side="right") - 1, 0, mu.size - 2)
        d = cs - mu[i]
        s = (Pb[i+1] - Pb[i]) / (mu[i+1] - mu[i])
        return Cb[i] + LD(0.5)*(Pb[i]*d + LD(0.5)*s*d*d)
    return _per_radius(fn, t, ibnd, re, cs)


def evaluate_ld(t, ibnd, re, cs):
    def fn(mu, Pb, Cb, cs):
        i = np.clip(np.searchsorted(mu, cs, side="right") - 1, 0, mu.size - 2)
        w = np.clip((cs - mu[i]) / (mu[i+1] - mu[i]), 0, 1)
        return Pb[i] + w*(Pb[i+1] - Pb[i])
    return _per_radius(fn, t, ibnd, re, cs)
