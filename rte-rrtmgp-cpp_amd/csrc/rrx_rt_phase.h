// Tabulated cloud phase functions of the two ray tracers: what trace_kernel<F,true>, trace_bw_kernel<F,true> and the
// array entries of rrx_rt_phase.hip share. ONE table serves the sampling of the scattering angle and the evaluation of the phase
// function towards the sun, so that the forward and the backward tracer stay estimators of the same quantity.
//
// THE TABLE. nmu nodes mu[0] = -1 < ... < mu[nmu-1] = +1 (cosines of the scattering angle, shared by every table); P is piecewise
// linear in mu between the nodes; phase(nmu, nre, nbnd) with 1/2 int P dmu = 1, and cdf(nmu, nre, nbnd) with
// C_i = 1/2 int_{-1}^{mu_i} P dmu, C_0 = 0, C_last = 1 (rrx_rt_phase_tables makes both). The radii are re0 + dre ire, ire < nre.
//   index     nre = 1: ire = 0, f = 0, no blend. Else q = (re - re0)/dre, ire = int(fmin(fmax(q, 0), nre-2)),
//             f = fmin(fmax(q - ire, 0), 1): a NaN radius gives ire = 0, f = 0.
//   blend     X = X_lo + f (X_hi - X_lo) for the phase function and, the nodes being shared, for its CDF: equal tables blend to
//             themselves exactly.
//   sampling  u -> cos, the one draw that gives the cosine in scatter_direction: the largest i <= nmu-2 with C_i <= u (binary
//             search on the blended CDF, two loads per probe); r = 2 (u - C_i); s = (P_i+1 - P_i)/(mu_i+1 - mu_i);
//             t = 2 r/(P_i + sqrt(max(0, P_i^2 + 2 s r))), 0 when the denominator is 0; cos = clamp(mu_i + t, mu_i, mu_i+1): the exact
//             inverse of the piecewise-quadratic CDF with + - x / sqrt only.
//   evaluation the largest i <= nmu-2 with mu_i <= cs; w = clamp((cs - mu_i)/(mu_i+1 - mu_i), 0, 1); on each of the two radii
//             P = P_i + w (P_i+1 - P_i); then the blend: the density that the sampler draws from.
#ifndef RRX_RT_PHASE_H
#define RRX_RT_PHASE_H

#include "rrx_rt_common.h"

namespace rrx
{
namespace rt
{
constexpr int RT_PHASE_MAX_NMU = 4096;          // the nodes of trace_bw_kernel<F,true> live in LDS: 32 KB in fp64

// the tables of one band: phase, cdf (nmu, nre)
template<typename F>
struct PhaseTable
{
    int nmu, nre;
    F re0, dre;
    const F* phase; const F* cdf;
};

// what the entries are given: the tables of every band, the nodes and the cell radius; all four pointers NULL: no table
template<typename F>
struct PhaseIn
{
    int nmu, nre;
    F re0, dre;
    const F* mu; const F* phase; const F* cdf; const F* cld_re;
    bool given() const { return mu != nullptr; }
};

// the kernels' second argument: empty in the Henyey-Greenstein instantiations
template<typename F, bool TABLE> struct PhaseArgs {};
template<typename F> struct PhaseArgs<F,true> { PhaseIn<F> in; };

template<typename F>
__device__ __forceinline__ PhaseTable<F> table_of_band(const PhaseIn<F>& in, const int ibnd)
{
    const size_t off = ibnd >= 0 ? size_t(in.nmu)*in.nre*ibnd : size_t(0);
    return PhaseTable<F>{in.nmu, in.nre, in.re0, in.dre, in.phase + off, in.cdf + off};
}

template<typename F>
__device__ __forceinline__ void phase_index(const PhaseTable<F>& t, const F re, int& ire, int& jre, F& f)
{
    ire = 0; jre = 0; f = F(0.);
    if (t.nre > 1)
    {
        const F q = (re - t.re0) / t.dre;
        ire = int(fmin(fmax(q, F(0.)), F(t.nre - 2)));
        f = fmin(fmax(q - F(ire), F(0.)), F(1.));
        jre = ire + 1;
    }
}

// u in [0, 1) -> the cosine of the scattering angle; mu: the nodes (global memory or LDS)
template<typename F>
__device__ __forceinline__ F phase_sample(const PhaseTable<F>& t, const F* mu, const F re, const F u)
{
    int ire, jre; F f;
    phase_index(t, re, ire, jre, f);
    const F* __restrict__ c_lo = t.cdf + size_t(ire)*t.nmu;
    const F* __restrict__ c_hi = t.cdf + size_t(jre)*t.nmu;
    int lo = 0, hi = t.nmu - 1;          // C_lo <= u < C_hi (C_0 = 0; the last node is never probed)
    while (hi - lo > 1)
    {
        const int mid = (lo + hi) >> 1;
        const F a = c_lo[mid], b = c_hi[mid];
        if (a + f*(b - a) <= u) lo = mid; else hi = mid;
    }
    const F* __restrict__ p_lo = t.phase + size_t(ire)*t.nmu;
    const F* __restrict__ p_hi = t.phase + size_t(jre)*t.nmu;
    const F ca = c_lo[lo], cb = c_hi[lo];
    const F c = ca + f*(cb - ca);
    const F pa0 = p_lo[lo], pb0 = p_hi[lo], pa1 = p_lo[lo+1], pb1 = p_hi[lo+1];
    const F p0 = pa0 + f*(pb0 - pa0), p1 = pa1 + f*(pb1 - pa1);
    const F m0 = mu[lo], m1 = mu[lo+1];
    const F r = F(2.)*(u - c);
    const F s = (p1 - p0) / (m1 - m0);
    const F den = p0 + sqrt(max(F(0.), p0*p0 + (F(2.)*s)*r));
    const F tt = den > F(0.) ? (F(2.)*r)/den : F(0.);
    return clampf(m0 + tt, m0, m1);
}

// P(cs), the density of phase_sample
template<typename F>
__device__ __forceinline__ F phase_eval(const PhaseTable<F>& t, const F* mu, const F re, const F cs)
{
    int ire, jre; F f;
    phase_index(t, re, ire, jre, f);
    int lo = 0, hi = t.nmu - 1;
    while (hi - lo > 1)
    {
        const int mid = (lo + hi) >> 1;
        if (mu[mid] <= cs) lo = mid; else hi = mid;
    }
    const F m0 = mu[lo], m1 = mu[lo+1];
    const F w = fmin(fmax((cs - m0) / (m1 - m0), F(0.)), F(1.));
    const F* __restrict__ p_lo = t.phase + size_t(ire)*t.nmu;
    const F* __restrict__ p_hi = t.phase + size_t(jre)*t.nmu;
    const F a0 = p_lo[lo], a1 = p_lo[lo+1], b0 = p_hi[lo], b1 = p_hi[lo+1];
    const F pa = a0 + w*(a1 - a0), pb = b0 + w*(b1 - b0);
    return pa + f*(pb - pa);
}

// scatter_direction with the table in place of Henyey-Greenstein: the same two draws in the same order
template<typename F>
__device__ __forceinline__ void scatter_direction_table(Stream& rng, const bool cloud, const PhaseTable<F>& t, const F* mu, const F re,
                                                        F& ux, F& uy, F& uz)
{
    const F u = rng.next<F>();
    const F cos_s = cloud ? phase_sample(t, mu, re, u) : rayleigh_cos(u);
    rotate_direction(rng, clampf(cos_s, F(-1.), F(1.)), ux, uy, uz);
}

// ---- host side

template<typename F>
void check_phase_extents(const int nmu, const int nre, const F dre)
{
    if (nmu < 2) throw std::runtime_error("nmu must be >= 2");
    if (nmu > RT_PHASE_MAX_NMU) throw std::runtime_error("nmu must be <= 4096");
    if (nre < 1) throw std::runtime_error("nre must be >= 1");
    if (nre > 1 && !(dre > F(0.))) throw std::runtime_error("dre must be > 0 with nre > 1");
}

template<typename F>
void check_phase(const PhaseIn<F>& ph, const void* cld_tau)
{
    const int given = (ph.mu != nullptr) + (ph.phase != nullptr) + (ph.cdf != nullptr) + (ph.cld_re != nullptr);
    if (given != 0 && given != 4) throw std::runtime_error("mu, phase, cdf, cld_re must be all NULL or all given");
    if (given == 0) return;
    if (cld_tau == nullptr) throw std::runtime_error("a phase table needs the cloud triple cld_tau, cld_ssa, cld_g");
    check_phase_extents(ph.nmu, ph.nre, ph.dre);
}
}  // namespace rt
}  // namespace rrx

#endif
