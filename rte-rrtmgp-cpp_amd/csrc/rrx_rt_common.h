// What the two Monte Carlo ray tracers share (rrx_raytracer.hip: forward, fluxes; rrx_raytracer_bw.hip: backward,
// radiances): the Philox stream of a photon or ray, the clamps, the fine cell of a coordinate, the integer tally, the
// band of a g-point, k_ext, the Lambertian direction, the scattering direction, the launch cap and the host-side argument checks.
// Everything here is inlined into the kernels; each file documents its own counter and draw order.
#ifndef RRX_RT_COMMON_H
#define RRX_RT_COMMON_H

#include "rrx_common.h"
#include "rrx_philox.h"

namespace rrx
{
namespace rt
{
typedef unsigned long long u64;

constexpr int RT_BLOCK = 256;
constexpr int RT_MAX_BLOCKS = 1024;         // 256 CUs x 4 workgroups: one wave per SIMD and workgroup

// workgroups a trace launch is capped at (the photons beyond are the threads' second, third, ... ones). Measured on the
// broken-cloud field of tools/raytracer_bench.py (profiles/raytracer_bench_caps.txt): 1 024 / 2 048 / 4 096 / 8 192 workgroups take
// 22.0 / 23.7 / 26.7 / 26.8 ms in fp64 and 15.6 / 16.1 / 16.9 / 16.8 ms in fp32 (3-D mode; one photon per thread from 4 096 on).
// RRX_RT_MAX_BLOCKS in the environment overrides it, read at every launch (tests run deep lists on a few threads).
inline int max_blocks()
{
    if (const char* e = std::getenv("RRX_RT_MAX_BLOCKS")) { const int n = std::atoi(e); if (n >= 1) return n; }
    return RT_MAX_BLOCKS;
}

struct Stream
{
    unsigned c0, c1, c2, block, k0, k1;
    int used;
    Philox words;
    __device__ __forceinline__ void start(const u64 photon, const unsigned igpt)
    {
        c0 = unsigned(photon & 0xFFFFFFFFull); c1 = unsigned(photon >> 32); c2 = igpt; block = 0u; used = 4;
    }
    template<typename F> __device__ __forceinline__ F next()
    {
        if (used == 4) { words = philox4x32_10(c0, c1, c2, block, k0, k1); ++block; used = 0; }
        const int s = used++;
        const unsigned x = s == 0 ? words.w[0] : (s == 1 ? words.w[1] : (s == 2 ? words.w[2] : words.w[3]));
        return uniform<F>(x);
    }
};

template<typename F> __device__ __forceinline__ F clampf(const F v, const F lo, const F hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int clampi(const int v, const int lo, const int hi) { return min(max(v, lo), hi); }

// the fine cell of a coordinate inside block `blk` of r cells of width d
template<typename F> __device__ __forceinline__ int fine_cell(const F pos, const F d, const int blk, const int r)
{
    return clampi(int(pos / d), blk*r, blk*r + r - 1);
}

template<typename F> __device__ __forceinline__ u64 to_count(const F weight)
{
    return u64(llrint(double(weight) * 4294967296.0));
}

__device__ __forceinline__ void tally(u64* __restrict__ counts, const size_t i, const u64 c)
{
    if (c != 0ull) atomicAdd(&counts[i], c);
}

// 0-based band of 0-based g-point igpt, -1 when it lies in no band; band_lims_gpt (2, nbnd), 1-based inclusive
__device__ __forceinline__ int band_of(const int igpt, const int nbnd, const int* __restrict__ band_lims_gpt)
{
    int ibnd = -1;
    for (int b=nbnd-1; b>=0; --b)
        if (igpt+1 >= band_lims_gpt[2*b] && igpt+1 <= band_lims_gpt[2*b+1]) ibnd = b;
    return ibnd;
}

template<typename F> __device__ __forceinline__ F k_ext_of(const F tau, const F tau_c, const F dz) { return (tau + tau_c) / dz; }

// cosine-weighted direction about the vertical; sign = -1 downward, +1 upward
template<typename F>
__device__ __forceinline__ void lambert(Stream& rng, const F sign, F& ux, F& uy, F& uz)
{
    const F mu = sqrt(rng.next<F>());
    const F phi = F(6.283185307179586) * rng.next<F>();
    const F s = sqrt(F(1.) - mu*mu);
    ux = s*cos(phi); uy = s*sin(phi); uz = sign*mu;
}

// the cosine of a Rayleigh scattering angle from one uniform: the root of mu^3 + 3 mu = 2 q, q = 4u - 2
template<typename F> __device__ __forceinline__ F rayleigh_cos(const F u)
{
    const F q = F(4.)*u - F(2.);
    const F A = cbrt(q + sqrt(F(1.) + q*q));
    return A - F(1.)/A;
}

// the direction at the angle acos(cos_s) from u: u -> phi
template<typename F>
__device__ __forceinline__ void rotate_direction(Stream& rng, const F cos_s, F& ux, F& uy, F& uz)
{
    const F sin_s = sqrt(max(F(0.), F(1.) - cos_s*cos_s));
    const F phi = F(6.283185307179586) * rng.next<F>();
    const F cp = cos(phi), sp = sin(phi);
    F vx, vy, vz;
    if (fabs(uz) > F(0.99999))
    {
        vx = sin_s*cp; vy = sin_s*sp; vz = uz > F(0.) ? cos_s : -cos_s;
    }
    else
    {
        const F den = sqrt(F(1.) - uz*uz);
        vx = (sin_s*((ux*uz)*cp - uy*sp))/den + ux*cos_s;
        vy = (sin_s*((uy*uz)*cp + ux*sp))/den + uy*cos_s;
        vz = uz*cos_s - (sin_s*cp)*den;
    }
    const F nrm = sqrt((vx*vx + vy*vy) + vz*vz);
    ux = vx/nrm; uy = vy/nrm; uz = vz/nrm;
}

// the new direction after a scattering: u -> cos of the scattering angle (Henyey-Greenstein with g = min(gc, g_max) for cloud,
// Rayleigh otherwise), u -> phi
template<typename F>
__device__ __forceinline__ void scatter_direction(Stream& rng, const bool cloud, const F gc, const F g_max, F& ux, F& uy, F& uz)
{
    const F u = rng.next<F>();
    F cos_s;
    if (cloud)
    {
        const F g = min(gc, g_max);
        if (fabs(g) < F(1.e-6)) cos_s = F(2.)*u - F(1.);
        else
        {
            const F s = (F(1.) - g*g) / ((F(1.) - g) + (F(2.)*g)*u);
            cos_s = ((F(1.) + g*g) - s*s) / (F(2.)*g);
        }
    }
    else cos_s = rayleigh_cos(u);
    rotate_direction(rng, clampf(cos_s, F(-1.), F(1.)), ux, uy, uz);
}

// ---- host side: the argument checks of the entries (they throw; RRX_CATCH names the entry)

inline void check_grid(const int nx, const int ny, const int nz, const int knx, const int kny, const int knz)
{
    if (knx < 1 || kny < 1 || knz < 1) throw std::runtime_error("knx, kny, knz must be >= 1");
    if (nx % knx != 0) throw std::runtime_error("knx does not divide nx");
    if (ny % kny != 0) throw std::runtime_error("kny does not divide ny");
    if (nz % knz != 0) throw std::runtime_error("knz does not divide nz");
    if ((long long)nx*ny*nz > 0x7FFFFFFFll) throw std::runtime_error("nx ny nz exceeds 2^31 - 1");
}

template<typename F>
void check_cloud(const int nbnd, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g)
{
    const int given = (cld_tau != nullptr) + (cld_ssa != nullptr) + (cld_g != nullptr);
    if (given != 0 && given != 3) throw std::runtime_error("cld_tau, cld_ssa, cld_g must be all NULL or all given");
    if (given == 3 && band_lims_gpt == nullptr) throw std::runtime_error("band_lims_gpt is NULL");
    if (given == 3 && nbnd < 1) throw std::runtime_error("nbnd must be >= 1 with a cloud triple");
}

// true: nothing to do
inline bool check_extents(std::initializer_list<std::pair<const char*, long long>> extents)
{
    bool empty = false;
    for (const auto& e : extents)
    {
        if (e.second < 0) throw std::runtime_error(std::string(e.first) + " is negative");
        if (e.second == 0) empty = true;
    }
    return empty;
}

inline void check_needed(std::initializer_list<std::pair<const char*, const void*>> needed)
{
    for (const auto& p : needed)
        if (p.second == nullptr) throw std::runtime_error(std::string(p.first) + " is NULL");
}

template<typename F>
void check_scene(const F dx, const F dy, const F dz, const F mu0)
{
    if (!(dx > F(0.)) || !(dy > F(0.)) || !(dz > F(0.))) throw std::runtime_error("dx, dy, dz must be > 0");
    if (!(mu0 > F(0.)) || mu0 > F(1.)) throw std::runtime_error("mu0 must be in (0, 1]");
}
}  // namespace rt
}  // namespace rrx

#endif
