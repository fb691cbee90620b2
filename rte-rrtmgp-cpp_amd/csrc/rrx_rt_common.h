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

// ---- aerosol as a third scattering species: a band triple aer_tau, aer_ssa, aer_g with the layout of the cloud triple,
// in the grid and (bg_aer_*) in the background. Per cell, with the parentheses as written:
//   k_ext = ((tau + tau_c) + tau_a)/dz,  k_sca = ((tau ssa + tau_c ssa_c) + tau_a ssa_a)/dz,  k_sca_aer = (tau_a ssa_a)/dz;
// tau_a = 0 gives the bits of the medium without aerosol. SPECIES DRAW from the one uniform u that is drawn today: cloud iff
// u k_sca < k_sca_cld (unchanged), otherwise aerosol iff u k_sca < k_sca_cld + k_sca_aer, otherwise gas. Aerosol scatters by
// Henyey-Greenstein with min(g_a, 1 - eps) everywhere: a phase table stays the cloud's alone.
template<typename F> __device__ __forceinline__ F k_ext_of(const F tau, const F tau_c, const F tau_a, const F dz) { return ((tau + tau_c) + tau_a) / dz; }
template<typename F> __device__ __forceinline__ F k_sca_of(const F tau, const F ssa, const F tau_c, const F ssa_c, const F tau_a, const F ssa_a, const F dz)
{
    return ((tau*ssa + tau_c*ssa_c) + tau_a*ssa_a) / dz;
}

// the grid's aerosol triple as the kernels take it, behind their background argument (NULL: no aerosol in the grid)
template<typename F> struct AerIn { const F* tau; const F* ssa; const F* g; };

// the Henyey-Greenstein density of cos_s, 4 pi normalised, g already limited: only + - x / and sqrt
template<typename F> __device__ __forceinline__ F hg_phase(const F g, const F cos_s)
{
    const F q = (F(1.) + g*g) - (F(2.)*g)*cos_s;
    return (F(1.) - g*g) / (q*sqrt(q));
}

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

// ---- the background atmosphere between the domain top and TOA: nbg plane-parallel, horizontally uniform layers of
// unequal thickness above the grid, counted UPWARD from the domain top whatever top_at_1 is. Layer b lies between z[b] and z[b+1];
// z[0] = F(knz) (F(nz/knz) dz), the domain top exactly as the kernels form it, z[b+1] = z[b] + dz_bg[b] in index order, z[nbg] is TOA.
// Per g-point rrx_rt_bg_profile writes the profile (BG_ROWS, nbg+1), layer fastest: k_ext, k_sca, k_sca_cld by the formulas of the
// grid with dz_bg[b] in place of dz, g = min(g_c, 1 - eps), and tau_above[b] = the vertical optical depth tau + tau_c of the layers
// b+1 .. nbg-1 added in index order from 0; slot nbg of tau_above holds the sum over all layers (what a walk that starts in the grid
// reads), slot nbg of the other rows is 0.
//
// TRANSPORT (both kernels): a background layer is a block whose k_null is its own k_ext and that has z faces only. A photon or ray
// in layer b carries the block index kn = knz + b. The collision is the grid's, draw for draw: f_no_abs = 1 - (k_ext - k_sca)/k_null,
// the roulette, the scatter-or-null draw (still made; it always scatters), the species draw, then Rayleigh or Henyey-Greenstein
// (the phase table applies inside the grid only). A layer with k_ext = 0 is crossed without a collision. A face crossing carries the
// rest of tau, between layers and through the domain top in either direction, and counts as an event. x and y advance UNWRAPPED and
// unclamped in the background (frozen under independent_column); on entering the grid from above they are wrapped by
// x - floor(x/Lx) Lx and the block found by integer division and clamping (enter_grid; under independent_column the photon keeps
// its x, y and block). uz = 0 in a layer with k_ext = 0: dropped into n_capped. No epsilon nudges.
constexpr int RT_BG_MAX = 256;         // the largest nbg: the levels travel to the kernels by value and live in LDS with the profile
enum { BG_K_EXT = 0, BG_K_SCA = 1, BG_K_SCA_CLD = 2, BG_G = 3, BG_TAU_ABOVE = 4, BG_ROWS = 5 };
// with aerosol (rrx_rt_bg_profile_aer) the profile is (BG_ROWS_AER, nbg+1): the five rows above by the formulas with tau_a, tau_above
// the sum of (tau + tau_c) + tau_a, then k_sca_aer = (tau_a ssa_a)/dz_bg and g_aer = min(g_a, 1 - eps); slot nbg of the two is 0
enum { BG_K_SCA_AER = 5, BG_G_AER = 6, BG_ROWS_AER = 7 };

// nbg + 1 numbers by value: the levels z (trace kernels), or one number per layer (rrx_rt_bg_profile: dz_bg)
template<typename F> struct BgLevels { F v[RT_BG_MAX + 1]; };

template<typename F> struct BgIn { int nbg; const F* profile; BgLevels<F> z; };

// the kernels' background argument: empty in the instantiations without one; AER: the aerosol form, built on the background form
template<typename F, bool BG, bool AER = false> struct BgArgs {};
template<typename F> struct BgArgs<F,true,false> { BgIn<F> in; };
template<typename F> struct BgArgs<F,true,true> { BgIn<F> in; AerIn<F> aer; };

// the profile and the levels in LDS: 6 (nbg + 1) numbers
template<typename F>
struct BgView
{
    int nbg;
    const F* k_ext; const F* k_sca; const F* k_sca_cld; const F* g; const F* tau_above; const F* z;
};

inline size_t bg_lds_numbers(const int nbg, const int rows = BG_ROWS) { return nbg > 0 ? size_t(rows + 1)*(nbg + 1) : size_t(0); }

// every thread of the workgroup calls it before its loop; lds: bg_lds_numbers(nbg, ROWS) numbers. ROWS = BG_ROWS_AER: the rows
// k_sca_aer and g_aer lie behind tau_above, at k_ext + BG_K_SCA_AER (nbg + 1) and k_ext + BG_G_AER (nbg + 1), the levels behind them
template<typename F, int ROWS = BG_ROWS>
__device__ __forceinline__ BgView<F> stage_background(const BgIn<F>& in, F* lds)
{
    const int n1 = in.nbg + 1;
    if (in.nbg > 0)
    {
        for (int n=threadIdx.x; n<ROWS*n1; n+=blockDim.x) lds[n] = in.profile[n];
        for (int n=threadIdx.x; n<n1; n+=blockDim.x) lds[ROWS*n1 + n] = in.z.v[n];
    }
    __syncthreads();
    return BgView<F>{in.nbg, lds + BG_K_EXT*n1, lds + BG_K_SCA*n1, lds + BG_K_SCA_CLD*n1, lds + BG_G*n1, lds + BG_TAU_ABOVE*n1,
                     lds + ROWS*n1};
}

// the layer of a height above the domain top: the largest b <= nbg-1 with z[b] <= height (nbg >= 1)
template<typename F> __device__ __forceinline__ int bg_layer_of(const BgView<F>& v, const F height)
{
    int b = 0;
    while (b + 1 < v.nbg && v.z[b+1] <= height) ++b;
    return b;
}

// a coordinate that comes down into the grid: wrapped into [0, len], its block of width kd and clamped into it
template<typename F> __device__ __forceinline__ void enter_grid(F& pos, int& blk, const F len, const F kd, const int nblk)
{
    pos = pos - floor(pos/len)*len;
    blk = clampi(int(pos/kd), 0, nblk - 1);
    pos = clampf(pos, F(blk)*kd, F(blk+1)*kd);
}

// the fine cell (of n, width d) of an unwrapped coordinate
template<typename F> __device__ __forceinline__ int wrapped_cell(const F pos, const F len, const F d, const int n)
{
    return clampi(int((pos - floor(pos/len)*len) / d), 0, n - 1);
}

// ---- all g-points in one launch of the forward tracer: the photons of a launch are the concatenation, in g-point order,
// of n_g photons per g-point; photon_end (ngpt + 1) holds the prefix sums, photon_end[0] = 0. Global index p belongs to the g with
// photon_end[g] <= p < photon_end[g+1] (empty ranges are stepped over), its local index is q = p - photon_end[g], its stream
// Stream::start(q, g) and its pixel q mod ncol: photon q of the per-g-point launch of g. Every deposit is to_count(w weight0[g]).
constexpr int RT_SPECTRAL_MAX_GPT = 1024;          // photon_end and the band table live in LDS: 12 bytes per g-point

// kn_g0: the g-point of the first slice of the k_null array that the launch is given (0 for the array of all g-points)
template<typename F> struct SpecIn { int ngpt; int kn_g0; const long long* photon_end; const F* weight0; const F* dif_frac; };

// photon_end and the band of every g-point (-1: in no band, or no band_lims_gpt) in LDS
struct SpecView { const long long* photon_end; const int* band; int ngpt; };

// LDS of the spectral form: photon_end, the background's levels, the band table (the profile rows stay in global memory)
inline size_t spectral_lds_bytes(const int ngpt, const int nbg, const size_t size_of_f)
{
    return size_t(ngpt + 1)*sizeof(long long) + size_t(nbg + 1)*size_of_f + size_t(ngpt)*sizeof(int);
}

// every thread of the workgroup calls it before its loop; lds: spectral_lds_bytes. bg gets nbg and the levels; its profile rows are
// set per photon (they point into the profile of all g-points)
template<typename F>
__device__ __forceinline__ SpecView stage_spectral(const SpecIn<F>& sp, const BgIn<F>& in, const int nbnd, const int* __restrict__ band_lims_gpt,
                                                   double* lds, BgView<F>& bg)
{
    long long* pe = reinterpret_cast<long long*>(lds);
    F* lev = reinterpret_cast<F*>(pe + sp.ngpt + 1);
    int* band = reinterpret_cast<int*>(lev + in.nbg + 1);
    for (int n=threadIdx.x; n<=sp.ngpt; n+=blockDim.x) pe[n] = sp.photon_end[n];
    for (int n=threadIdx.x; n<in.nbg+1; n+=blockDim.x) lev[n] = in.nbg > 0 ? in.z.v[n] : F(0.);
    for (int g=threadIdx.x; g<sp.ngpt; g+=blockDim.x) band[g] = band_lims_gpt != nullptr ? band_of(g, nbnd, band_lims_gpt) : -1;
    __syncthreads();
    bg = BgView<F>{in.nbg, nullptr, nullptr, nullptr, nullptr, nullptr, lev};
    return SpecView{pe, band, sp.ngpt};
}

// the g-point of global photon p: the smallest g with photon_end[g+1] > p; ngpt when p lies beyond the list
__device__ __forceinline__ int gpt_of_photon(const long long* photon_end, const int ngpt, const long long p)
{
    int lo = 0, hi = ngpt;
    while (lo < hi)
    {
        const int mid = (lo + hi) >> 1;
        if (photon_end[mid + 1] <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the profile rows of g-point igpt in the profile (ngpt, ROWS, nbg+1) of all g-points
template<typename F, int ROWS>
__device__ __forceinline__ void bg_rows_of_gpt(BgView<F>& bg, const F* __restrict__ profile_all, const int igpt)
{
    const int n1 = bg.nbg + 1;
    const F* p = profile_all + size_t(igpt)*ROWS*n1;
    bg.k_ext = p + BG_K_EXT*n1; bg.k_sca = p + BG_K_SCA*n1; bg.k_sca_cld = p + BG_K_SCA_CLD*n1; bg.g = p + BG_G*n1;
    bg.tau_above = p + BG_TAU_ABOVE*n1;
}

// ---- host side: the argument checks of the entries (they throw; RRX_CATCH names the entry; rrx_rt_host.h runs them in their order)

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

// mu0: NULL for a tracer without a sun
template<typename F>
void check_scene(const F dx, const F dy, const F dz, const F* mu0)
{
    if (!(dx > F(0.)) || !(dy > F(0.)) || !(dz > F(0.))) throw std::runtime_error("dx, dy, dz must be > 0");
    if (mu0 != nullptr && (!(*mu0 > F(0.)) || *mu0 > F(1.))) throw std::runtime_error("mu0 must be in (0, 1]");
}

// ---- the background's arguments

// the levels of a background: throws on a non-positive (or NaN) thickness
template<typename F>
BgLevels<F> bg_levels(const int nbg, const F* dz_bg, const int nz, const int knz, const F dz)
{
    BgLevels<F> lev{};
    lev.v[0] = F(knz)*(F(nz/knz)*dz);
    for (int b=0; b<nbg; ++b)
    {
        if (!(dz_bg[b] > F(0.)) || !(dz_bg[b] < F(INFINITY))) throw std::runtime_error("dz_bg must be > 0");
        lev.v[b+1] = lev.v[b] + dz_bg[b];
    }
    return lev;
}

// what the _bg entries check of their background arguments; nbg = 0: none of them is read
template<typename F>
void check_bg_medium(const int nbg, const int nbnd, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const int* band_lims_gpt,
                     const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g)
{
    if (nbg == 0) return;
    check_needed({{"dz_bg", dz_bg}, {"bg_tau", bg_tau}, {"bg_ssa", bg_ssa}});
    const int given = (bg_cld_tau != nullptr) + (bg_cld_ssa != nullptr) + (bg_cld_g != nullptr);
    if (given != 0 && given != 3) throw std::runtime_error("bg_cld_tau, bg_cld_ssa, bg_cld_g must be all NULL or all given");
    if (given == 3 && band_lims_gpt == nullptr) throw std::runtime_error("band_lims_gpt is NULL");
    if (given == 3 && nbnd < 1) throw std::runtime_error("nbnd must be >= 1 with a background cloud triple");
}

// what the _aer entries check of an aerosol triple (the grid's: aer_*, the background's: bg_aer_*)
template<typename F>
void check_aerosol(const char* which, const int nbnd, const int* band_lims_gpt, const F* tau, const F* ssa, const F* g)
{
    const int given = (tau != nullptr) + (ssa != nullptr) + (g != nullptr);
    const std::string w(which);
    if (given != 0 && given != 3) throw std::runtime_error(w + "tau, " + w + "ssa, " + w + "g must be all NULL or all given");
    if (given == 3 && band_lims_gpt == nullptr) throw std::runtime_error("band_lims_gpt is NULL");
    if (given == 3 && nbnd < 1) throw std::runtime_error("nbnd must be >= 1 with an aerosol triple");
}

inline void check_nbg(const int nbg)
{
    if (nbg < 0) throw std::runtime_error("nbg is negative");
    if (nbg > RT_BG_MAX) throw std::runtime_error("nbg must be <= 256");
}
}  // namespace rt
}  // namespace rrx

#endif
