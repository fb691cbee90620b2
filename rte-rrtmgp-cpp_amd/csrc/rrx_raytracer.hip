// Forward Monte Carlo ray tracer for 3-D shortwave fluxes. The algorithm is that of the reference's
// ray_tracer_kernel (src_kernels_cuda_rt/raytracer_kernels.cu): null-collision tracking on a coarse grid of maximum extinction,
// expected-value absorption at every collision (Iwabuchi 2006), Russian roulette below weight 0.5, a Lambertian surface, periodic
// x / y, an independent-column switch. Written for this project's arrays and with these departures:
//   - inputs are the clear g-point arrays tau, ssa (ncol = nx ny with x fastest, nz, ngpt) and the band cloud triple (ncol, nz, nbnd);
//     k_ext = (tau + tau_c)/dz, k_sca = (tau ssa + tau_c ssa_c)/dz, k_sca_cld = (tau_c ssa_c)/dz; gas scattering is Rayleigh, cloud
//     scattering Henyey-Greenstein with min(g_c, 1 - eps);
//   - nothing is divided by the local extinction: f_no_abs = 1 - (k_ext - k_sca)/k_null (clamped to [0, 1]), a surviving photon
//     scatters iff u (k_sca + (k_null - k_ext)) < k_sca and the scatterer is cloud iff u k_sca < k_sca_cld, so a cell with k_ext = 0
//     inside a block with k_null > 0 is well defined; a block with k_null = 0 is crossed without a collision;
//   - a photon carries the integer indices (in, jn, kn) of its block of the k_null grid; a crossing moves the index by one (wrapping
//     in x / y) and puts the coordinate on the face, a collision clamps the position into the block, and the fine cell is
//     clamp(int(x/dx), block's first cell, block's last cell): no epsilon nudges, no fmod, the same code in both precisions;
//   - photon p of a g-point starts in pixel p mod (nx ny): every pixel gets exactly photons_per_pixel photons;
//   - tallies are unsigned 64-bit integers in units of 2^-32 photon, llrint(weight 2^32) added with integer atomics: the result of
//     a launch does not depend on the order of arrival, is bit-reproducible and additive over photon ranges;
//   - a photon is dropped after max_events events (collisions + crossings, surface hits and exits among them) and counted in
//     n_capped, and a thread traces a fixed list of photons: every loop is bounded by construction.
//
// Coordinates: x, y, z in metres, z upward from the surface (z = 0) to the domain top; block kn = 0 is the lowest. Fine cell
// k (counted upward) is array layer nz-1-k with top_at_1, k otherwise. k_null(knx, kny, knz): x fastest, kn upward.
//
// Random numbers: Philox4x32-10, key = (low, high) words of the seed, counter = (photon index low, photon index high, g-point,
// block number 0, 1, 2, ...); the four words of a block are consumed in order, uniform = ((x >> 9) + 0.5) 2^-23. DRAW ORDER of a
// photon (part of the specification; tests/raytracer_ref.py restates it):
//   start:     u -> x = (ix + u) dx;  u -> y = (iy + u) dy;  u -> diffuse iff u < inc_dif/(inc_dir + inc_dif);
//              diffuse only: u -> mu = sqrt(u);  u -> phi = 2 pi u;  direction (s cos phi, s sin phi, -mu), s = sqrt(1 - mu^2)
//   each event: u -> tau = -log(u), unless the previous event was a crossing between blocks (the remaining tau is carried)
//     crossing (tau >= d_max k_null, or k_null = 0): tau -= d_max k_null; at the surface: tally, weight *= albedo, tally,
//              weight < 0.5: u -> survives (weight = 1) iff u <= weight;  survivor: u -> mu = sqrt(u);  u -> phi; direction upward
//     collision: deposit weight (1 - f_no_abs), weight *= f_no_abs;  weight < 0.5: u -> roulette as above;
//              survivor: u -> scatter or null collision;  scatter: u -> species;  u -> cos of the scattering angle;  u -> phi
//
// WITH A BACKGROUND (trace_kernel<F,TABLE,true>, the rrx_*_bg entries; rrx_rt_common.h; tests/raytracer_bg_ref.py
// restates it) the DRAW ORDER is the same:
//   start:     the same draws; the photon starts at TOA, z = z_bg[nbg], in layer nbg-1 (block index knz + nbg - 1) with the x, y,
//              pixel and block (in, jn) of the start without a background
//   each event in layer b: u -> tau = -log(u), unless the previous event was a crossing (between layers, between blocks, or
//              through the domain top in either direction: the remaining tau is carried)
//     crossing (tau >= d_max k_ext_b with d_max the distance to the z face, or k_ext_b = 0): tau -= d_max k_ext_b; no draw. Upward
//              from layer nbg-1: toa_up, the photon ends. Downward from layer 0: enter_grid (x, y wrapped, their block by integer
//              division and clamping; not under independent_column), block knz-1, z = the domain top, tod_dn_dir / tod_dn_dif.
//              Upward out of block knz-1 of the grid: tod_up, then layer 0 (the photon ends there only when nbg = 0).
//     collision: deposit weight (1 - f_no_abs) into bg_abs_dir / bg_abs_dif [b], weight *= f_no_abs, f_no_abs = 1 - (k_ext_b - k_sca_b)/k_ext_b;
//              weight < 0.5: u -> roulette;  survivor: u -> scatter or null collision (it always scatters);  u -> species;
//              u -> cos of the scattering angle (Rayleigh, or Henyey-Greenstein with the layer's g, with a phase table too);  u -> phi
//   uz = 0 in a layer with k_ext = 0: the photon is dropped into n_capped.
// The spectral loop scales toa_up, tod_dn_dir, tod_dn_dif like the other fluxes and bg_abs_* [b] by (scale/dz_bg[b])/F(ncol): W m-3 of
// a layer that spans the whole domain.
//
// WITH AEROSOL (trace_kernel<F,TABLE,true,true>, the rrx_*_aer entries; rrx_rt_common.h; tests/raytracer_aer_ref.py restates
// it): a third species with its own band triple in the grid and in the background. k_ext, k_sca and k_null take tau_a as
// rrx_rt_common.h writes them, abs_* and bg_abs_* take what aerosol absorbs through f_no_abs, and the draw count and DRAW ORDER are
// unchanged: the species uniform u picks cloud iff u k_sca < k_sca_cld, otherwise aerosol iff u k_sca < k_sca_cld + k_sca_aer,
// otherwise gas; aerosol scatters by Henyey-Greenstein with min(g_a, 1 - eps), in the grid and aloft, with a phase table too.
// DEPARTURE: the reference draws aerosol, cloud, gas in that order; cloud comes first here so that a scene without aerosol draws
// exactly what it draws without this form.
//
// Shape: one photon per lane at a time; a lane whose photon ends takes the next one of its list in the same loop, so the lanes
// of a wave stay busy until the lists run out (the grid is capped and the photons dealt round-robin over the threads).
#include "rrx_rt_phase.h"
#include "rrx_hip.h"

namespace
{
using namespace rrx;
using namespace rrx::rt;

// the maximum of ((tau + tau_c) + tau_a)/dz over the cells of block n of the k_null grid, for g-point igpt
template<typename F>
__device__ __forceinline__ F k_null_aer_of_block(
        const int n, const int nx, const int ny, const int nz, const int nbnd, const int igpt, const int top_at_1,
        const F* __restrict__ tau, const int* __restrict__ band_lims_gpt, const F* __restrict__ cld_tau, const F* __restrict__ aer_tau,
        const F dz, const int knx, const int kny, const int knz)
{
    const int in = n % knx, jn = (n / knx) % kny, kn = n / (knx*kny);
    const int rx = nx/knx, ry = ny/kny, rz = nz/knz;
    const size_t ncol = size_t(nx)*ny;
    const int ibnd = (cld_tau != nullptr || aer_tau != nullptr) ? band_of(igpt, nbnd, band_lims_gpt) : -1;
    F m = F(0.);
    for (int k=kn*rz; k<(kn+1)*rz; ++k)
    {
        const int lay = top_at_1 ? nz-1-k : k;
        for (int j=jn*ry; j<(jn+1)*ry; ++j)
            for (int i=in*rx; i<(in+1)*rx; ++i)
            {
                const size_t cell = size_t(i) + size_t(j)*nx + ncol*lay;
                const F tc = (ibnd >= 0 && cld_tau != nullptr) ? cld_tau[cell + ncol*nz*ibnd] : F(0.);
                const F ta = (ibnd >= 0 && aer_tau != nullptr) ? aer_tau[cell + ncol*nz*ibnd] : F(0.);
                m = max(m, k_ext_of(tau[cell + ncol*nz*igpt], tc, ta, dz));
            }
    }
    return m;
}

// k_null_kernel with aerosol
template<typename F>
__global__ void __launch_bounds__(256) k_null_aer_kernel(
        const int nx, const int ny, const int nz, const int nbnd, const int igpt, const int top_at_1,
        const F* __restrict__ tau, const int* __restrict__ band_lims_gpt, const F* __restrict__ cld_tau, const F* __restrict__ aer_tau,
        const F dz, const int knx, const int kny, const int knz, F* __restrict__ k_null)
{
    const int n = blockIdx.x*blockDim.x + threadIdx.x;
    if (n >= knx*kny*knz) return;
    k_null[n] = k_null_aer_of_block<F>(n, nx, ny, nz, nbnd, igpt, top_at_1, tau, band_lims_gpt, cld_tau, aer_tau, dz, knx, kny, knz);
}

// k_null_aer_kernel for the ng g-points from g0 on, blockIdx.y counting them: slice g - g0 of k_null (ng, knz, kny, knx)
// holds what k_null_aer_kernel(igpt = g) writes
template<typename F>
__global__ void __launch_bounds__(256) k_null_all_kernel(
        const int nx, const int ny, const int nz, const int nbnd, const int g0, const int top_at_1,
        const F* __restrict__ tau, const int* __restrict__ band_lims_gpt, const F* __restrict__ cld_tau, const F* __restrict__ aer_tau,
        const F dz, const int knx, const int kny, const int knz, F* __restrict__ k_null)
{
    const int n = blockIdx.x*blockDim.x + threadIdx.x;
    if (n >= knx*kny*knz) return;
    k_null[size_t(blockIdx.y)*(size_t(knx)*kny*knz) + n] =
        k_null_aer_of_block<F>(n, nx, ny, nz, nbnd, g0 + int(blockIdx.y), top_at_1, tau, band_lims_gpt, cld_tau, aer_tau, dz, knx, kny, knz);
}

// k_null(in, jn, kn) = the maximum of k_ext over the block's cells, for one g-point
template<typename F>
__global__ void __launch_bounds__(256) k_null_kernel(
        const int nx, const int ny, const int nz, const int nbnd, const int igpt, const int top_at_1,
        const F* __restrict__ tau, const int* __restrict__ band_lims_gpt, const F* __restrict__ cld_tau, const F dz,
        const int knx, const int kny, const int knz, F* __restrict__ k_null)
{
    const int n = blockIdx.x*blockDim.x + threadIdx.x;
    if (n >= knx*kny*knz) return;
    const int in = n % knx, jn = (n / knx) % kny, kn = n / (knx*kny);
    const int rx = nx/knx, ry = ny/kny, rz = nz/knz;
    const size_t ncol = size_t(nx)*ny;
    const int ibnd = cld_tau != nullptr ? band_of(igpt, nbnd, band_lims_gpt) : -1;
    F m = F(0.);
    for (int k=kn*rz; k<(kn+1)*rz; ++k)
    {
        const int lay = top_at_1 ? nz-1-k : k;
        for (int j=jn*ry; j<(jn+1)*ry; ++j)
            for (int i=in*rx; i<(in+1)*rx; ++i)
            {
                const size_t cell = size_t(i) + size_t(j)*nx + ncol*lay;
                const F tc = ibnd >= 0 ? cld_tau[cell + ncol*nz*ibnd] : F(0.);
                m = max(m, k_ext_of(tau[cell + ncol*nz*igpt], tc, dz));
            }
    }
    k_null[n] = m;
}

template<typename F>
struct TraceArgs
{
    int nx, ny, nz, nbnd, igpt, top_at_1, independent_column;
    const F* tau; const F* ssa; const int* band_lims_gpt; const F* cld_tau; const F* cld_ssa; const F* cld_g;
    F dx, dy, dz;
    const F* sfc_albedo;
    F sun_x, sun_y, sun_z, dif_frac;
    int knx, kny, knz;
    const F* k_null;
    unsigned k0, k1;
    u64 photon0; long long nphotons; int max_events;
    u64* sfc_dn_dir; u64* sfc_dn_dif; u64* sfc_up; u64* tod_up; u64* abs_dir; u64* abs_dif; u64* n_capped;
};

// TABLE: cloud scatters by the tabulated phase function of the cell's radius (rrx_rt_phase.h) in place of
// Henyey-Greenstein; cld_g is then not read, and the radius only once the scatterer has been drawn as cloud
//
// BG: the background atmosphere above the grid (rrx_rt_common.h). Photons start at TOA in layer nbg-1 with the same
// pixel and the same start draws; tod_up tallies every upward crossing of the domain top (those photons may come back), tod_dn_dir /
// tod_dn_dif every downward one by the pixel they enter, toa_up the photons that leave through TOA by the pixel of the wrapped exit
// position, bg_abs_dir / bg_abs_dif (nbg) the expected absorbed share at background collisions. With nbg = 0 it is the medium
// without a background: the integers of the other instantiations.
template<typename F>
struct BgTallies { u64* toa_up; u64* tod_dn_dir; u64* tod_dn_dif; u64* bg_abs_dir; u64* bg_abs_dif; };
template<typename F, bool BG, bool AER = false, bool SPECTRAL = false> struct FwBg {};
template<typename F> struct FwBg<F,true,false,false> { BgIn<F> in; BgTallies<F> t; };
template<typename F> struct FwBg<F,true,true,false> { BgIn<F> in; BgTallies<F> t; AerIn<F> aer; };
// the spectral form (below): in.profile is the profile of all g-points, (ngpt, BG_ROWS_AER, nbg+1)
template<typename F> struct FwBg<F,true,true,true> { BgIn<F> in; BgTallies<F> t; AerIn<F> aer; SpecIn<F> sp; };

// AER: aerosol as a third species (rrx_rt_common.h), built on top of the BG form only, which handles nbg = 0: the grid's
// triple in bgin.aer (NULL: none in the grid), the background's in rows BG_K_SCA_AER and BG_G_AER of the 7-row profile.
//
// SPECTRAL: all g-points in one launch (rrx_rt_common.h), built on the aerosol form only. a.photon0 / a.nphotons address the
// concatenated list; the g-point is state of the photon, set when a lane takes its next one, and the band, the tau / ssa / k_null slices
// and the background's profile rows are derived from it at every event (carried, they cost a wave per SIMD in registers). a.igpt and
// a.dif_frac are not read. The transport is that of photon q of g-point g in the per-g-point launch, draw for draw; every deposit is
// to_count(w weight0[g]).
template<typename F, bool TABLE, bool BG, bool AER, bool SPECTRAL = false>
__global__ void __launch_bounds__(RT_BLOCK) trace_kernel(const TraceArgs<F> a, const PhaseArgs<F,TABLE> ph, const FwBg<F,BG,AER,SPECTRAL> bgin)
{
    static_assert(BG || !AER, "the aerosol form is built on the background form");
    static_assert(AER || !SPECTRAL, "the spectral form is built on the aerosol form");
    [[maybe_unused]] BgView<F> bg{};
    [[maybe_unused]] SpecView sv{};
    if constexpr (SPECTRAL)
    {
        extern __shared__ double bg_lds[];
        sv = stage_spectral<F>(bgin.sp, bgin.in, a.nbnd, a.band_lims_gpt, bg_lds, bg);
    }
    else if constexpr (BG)
    {
        extern __shared__ double bg_lds[];
        bg = stage_background<F, AER ? BG_ROWS_AER : BG_ROWS>(bgin.in, reinterpret_cast<F*>(bg_lds));
    }
    const long long nthreads = (long long)gridDim.x*blockDim.x;
    long long next_photon = (long long)blockIdx.x*blockDim.x + threadIdx.x;

    const int nx = a.nx, ny = a.ny, nz = a.nz;
    const size_t ncol = size_t(nx)*ny;
    const int rx = nx/a.knx, ry = ny/a.kny, rz = nz/a.knz;
    const F kdx = F(rx)*a.dx, kdy = F(ry)*a.dy, kdz = F(rz)*a.dz;
    [[maybe_unused]] const F len_x = F(a.knx)*kdx, len_y = F(a.kny)*kdy;
    const bool ic = a.independent_column != 0;
    // (what follows of the g-point is fixed for the launch, or under SPECTRAL set with every photon)
    int igpt = SPECTRAL ? 0 : a.igpt;
    int ibnd = -1;
    const F* __restrict__ tau_g = a.tau;
    const F* __restrict__ ssa_g = a.ssa;
    const F* __restrict__ kn_g = a.k_null;
    if constexpr (!SPECTRAL)
    {
        ibnd = a.cld_tau != nullptr ? band_of(a.igpt, a.nbnd, a.band_lims_gpt) : -1;
        tau_g = a.tau + ncol*nz*a.igpt;
        ssa_g = a.ssa + ncol*nz*a.igpt;
    }
    const F inf = F(INFINITY);
    [[maybe_unused]] const F g_max = F(1.) - Lim<F>::eps();
    [[maybe_unused]] int ibnd_a = -1;
    if constexpr (AER && !SPECTRAL) ibnd_a = bgin.aer.tau != nullptr ? band_of(a.igpt, a.nbnd, a.band_lims_gpt) : -1;
    // a deposit of weight w, in units of 2^-32 photon
    const auto count_of = [&](const F w) { if constexpr (SPECTRAL) return to_count(w*bgin.sp.weight0[igpt]); else return to_count(w); };

    Stream rng; rng.k0 = a.k0; rng.k1 = a.k1; rng.used = 4; rng.block = 0u; rng.c0 = rng.c1 = rng.c2 = 0u;
    bool alive = false, pending = false;
    int in = 0, jn = 0, kn = 0, kind = 0, nev = 0;
    F x = F(0.), y = F(0.), z = F(0.), ux = F(0.), uy = F(0.), uz = F(-1.), weight = F(0.), tau = F(0.);

    for (;;)
    {
        if (!alive)
        {
            if (next_photon >= a.nphotons) break;          // the list is finite and every photon ends within max_events events
            u64 p = a.photon0 + u64(next_photon);
            next_photon += nthreads;
            [[maybe_unused]] F dif_frac = a.dif_frac;
            if constexpr (SPECTRAL)
            {
                igpt = gpt_of_photon(sv.photon_end, sv.ngpt, (long long)p);
                if (igpt >= sv.ngpt) continue;          // (beyond the list)
                p = p - u64(sv.photon_end[igpt]);
                dif_frac = bgin.sp.dif_frac[igpt];
            }
            rng.start(p, unsigned(igpt));
            const int pix = int(p % u64(ncol));
            const int ix = pix % nx, iy = pix / nx;
            in = ix / rx; jn = iy / ry; kn = a.knz - 1;
            x = clampf((F(ix) + rng.next<F>())*a.dx, F(in)*kdx, F(in+1)*kdx);
            y = clampf((F(iy) + rng.next<F>())*a.dy, F(jn)*kdy, F(jn+1)*kdy);
            z = F(a.knz)*kdz;
            if constexpr (BG) { if (bg.nbg > 0) { kn = a.knz + bg.nbg - 1; z = bg.z[bg.nbg]; } }
            if (rng.next<F>() < dif_frac) { lambert(rng, F(-1.), ux, uy, uz); kind = 1; }
            else { ux = a.sun_x; uy = a.sun_y; uz = a.sun_z; kind = 0; }
            weight = F(1.); pending = false; nev = 0; alive = true;
        }
        if (nev >= a.max_events) { atomicAdd(a.n_capped, 1ull); alive = false; continue; }
        ++nev;
        if constexpr (SPECTRAL)
        {
            // what the event reads of the photon's g-point, derived again at every event: the lane carries igpt only (weight0 is read at a deposit)
            const int band = sv.band[igpt];
            ibnd = a.cld_tau != nullptr ? band : -1;
            ibnd_a = bgin.aer.tau != nullptr ? band : -1;
            tau_g = a.tau + ncol*nz*igpt;
            ssa_g = a.ssa + ncol*nz*igpt;
            kn_g = a.k_null + (size_t(a.knx)*a.kny*a.knz)*size_t(igpt - bgin.sp.kn_g0);
            if (bg.nbg > 0) bg_rows_of_gpt<F, BG_ROWS_AER>(bg, bgin.in.profile, igpt);
        }

        // in_bg: the photon is in background layer kn - knz, a block with z faces only whose k_null is its own k_ext
        [[maybe_unused]] bool in_bg = false;
        if constexpr (BG) in_bg = kn >= a.knz;
        const F x_lo = F(in)*kdx, x_hi = F(in+1)*kdx, y_lo = F(jn)*kdy, y_hi = F(jn+1)*kdy;
        F z_lo = F(kn)*kdz, z_hi = F(kn+1)*kdz;
        if constexpr (BG) { if (in_bg) { z_lo = bg.z[kn - a.knz]; z_hi = bg.z[kn - a.knz + 1]; } }
        const bool flat = ic || in_bg;
        const F sz = uz > F(0.) ? (z_hi - z)/uz : (uz < F(0.) ? (z_lo - z)/uz : inf);
        const F sx = flat ? inf : (ux > F(0.) ? (x_hi - x)/ux : (ux < F(0.) ? (x_lo - x)/ux : inf));
        const F sy = flat ? inf : (uy > F(0.) ? (y_hi - y)/uy : (uy < F(0.) ? (y_lo - y)/uy : inf));
        const F d_max = min(sz, min(sx, sy));
        const int axis = (sz <= sx && sz <= sy) ? 2 : (sx <= sy ? 0 : 1);
        F kn_val;
        if constexpr (BG) kn_val = in_bg ? bg.k_ext[kn - a.knz] : kn_g[in + a.knx*(jn + a.kny*min(kn, a.knz - 1))];
        else kn_val = kn_g[in + a.knx*(jn + a.kny*kn)];
        if (!pending) tau = -log(rng.next<F>());
        pending = false;
        const bool empty = !(kn_val > F(0.));
        const F tau_cell = empty ? F(0.) : d_max*kn_val;

        if (empty || tau >= tau_cell)
        {
            // ---- the photon leaves the block through the face of `axis`
            if (!(d_max < inf)) { atomicAdd(a.n_capped, 1ull); alive = false; continue; }      // (a direction along no axis it may move on)
            tau = tau - tau_cell; pending = true;
            if (!ic)
            {
                if (in_bg) { x = x + ux*d_max; y = y + uy*d_max; }
                else { x = clampf(x + ux*d_max, x_lo, x_hi); y = clampf(y + uy*d_max, y_lo, y_hi); }
            }
            z = clampf(z + uz*d_max, z_lo, z_hi);
            [[maybe_unused]] bool handled = false;
            if constexpr (BG)
            {
                if (in_bg)
                {
                    // ---- a z face of a background layer: TOA, the next layer, or the domain top from above
                    handled = true;
                    if (uz > F(0.))
                    {
                        if (kn == a.knz + bg.nbg - 1)
                        {
                            const int pix = wrapped_cell(x, len_x, a.dx, nx) + nx*wrapped_cell(y, len_y, a.dy, ny);
                            tally(bgin.t.toa_up, pix, count_of(weight));
                            alive = false;
                        }
                        else { ++kn; z = bg.z[kn - a.knz]; }
                    }
                    else if (kn == a.knz)
                    {
                        if (!ic) { enter_grid(x, in, len_x, kdx, a.knx); enter_grid(y, jn, len_y, kdy, a.kny); }
                        kn = a.knz - 1; z = F(a.knz)*kdz;
                        const int pix = fine_cell(x, a.dx, in, rx) + nx*fine_cell(y, a.dy, jn, ry);
                        tally(kind == 0 ? bgin.t.tod_dn_dir : bgin.t.tod_dn_dif, pix, count_of(weight));
                    }
                    else { --kn; z = bg.z[kn - a.knz + 1]; }
                }
            }
            if (handled) {}          // (the background's face, above)
            else if (axis == 0)
            {
                if (ux > F(0.)) { in = (in + 1 == a.knx) ? 0 : in + 1; x = F(in)*kdx; }
                else { in = (in == 0) ? a.knx - 1 : in - 1; x = F(in+1)*kdx; }
            }
            else if (axis == 1)
            {
                if (uy > F(0.)) { jn = (jn + 1 == a.kny) ? 0 : jn + 1; y = F(jn)*kdy; }
                else { jn = (jn == 0) ? a.kny - 1 : jn - 1; y = F(jn+1)*kdy; }
            }
            else if (uz > F(0.))
            {
                if (kn == a.knz - 1)          // out through the domain top
                {
                    const int pix = fine_cell(x, a.dx, in, rx) + nx*fine_cell(y, a.dy, jn, ry);
                    tally(a.tod_up, pix, count_of(weight));
                    alive = false;
                    if constexpr (BG) { if (bg.nbg > 0) { alive = true; kn = a.knz; z = bg.z[0]; } }
                }
                else { ++kn; z = F(kn)*kdz; }
            }
            else if (kn == 0)                 // the surface
            {
                z = F(0.);
                const int pix = fine_cell(x, a.dx, in, rx) + nx*fine_cell(y, a.dy, jn, ry);
                tally(kind == 0 ? a.sfc_dn_dir : a.sfc_dn_dif, pix, count_of(weight));
                weight = weight * a.sfc_albedo[pix];
                tally(a.sfc_up, pix, count_of(weight));
                if (weight < F(0.5)) weight = (rng.next<F>() > weight) ? F(0.) : F(1.);
                if (weight > F(0.)) { lambert(rng, F(1.), ux, uy, uz); kind = 1; pending = false; }
                else alive = false;
            }
            else { --kn; z = F(kn+1)*kdz; }
        }
        else
        {
            // ---- a collision inside the block
            const F dn = tau / kn_val;
            if (!ic)
            {
                if (in_bg) { x = x + ux*dn; y = y + uy*dn; }
                else { x = clampf(x + ux*dn, x_lo, x_hi); y = clampf(y + uy*dn, y_lo, y_hi); }
            }
            z = clampf(z + uz*dn, z_lo, z_hi);
            // the cell and its k_ext, k_sca, k_sca_cld: a cell of the grid, or the photon's background layer
            size_t cell = 0;
            F k_ext = F(0.), k_sca = F(0.), k_sca_cld = F(0.);
            [[maybe_unused]] F gc = F(0.), k_sca_aer = F(0.), ga = F(0.);
            u64* abs_to = kind == 0 ? a.abs_dir : a.abs_dif;
            if (in_bg)
            {
                if constexpr (BG)
                {
                    cell = size_t(kn - a.knz);
                    k_ext = kn_val; k_sca = bg.k_sca[cell]; k_sca_cld = bg.k_sca_cld[cell]; gc = bg.g[cell];
                    if constexpr (AER)
                    {
                        k_sca_aer = bg.k_ext[BG_K_SCA_AER*(bg.nbg + 1) + cell]; ga = bg.k_ext[BG_G_AER*(bg.nbg + 1) + cell];
                    }
                    abs_to = kind == 0 ? bgin.t.bg_abs_dir : bgin.t.bg_abs_dif;
                }
            }
            else
            {
                const int i = fine_cell(x, a.dx, in, rx), j = fine_cell(y, a.dy, jn, ry), k = fine_cell(z, a.dz, kn, rz);
                const int lay = a.top_at_1 ? nz-1-k : k;
                cell = size_t(i) + size_t(j)*nx + ncol*lay;
                const F t = tau_g[cell], w0 = ssa_g[cell];
                F tc = F(0.), wc = F(0.);
                if (ibnd >= 0)
                {
                    const size_t cb = cell + ncol*nz*ibnd;
                    tc = a.cld_tau[cb]; wc = a.cld_ssa[cb];
                    if constexpr (!TABLE) gc = a.cld_g[cb];
                }
                if constexpr (AER)
                {
                    F ta = F(0.), wa = F(0.);
                    if (ibnd_a >= 0)
                    {
                        const size_t cb = cell + ncol*nz*ibnd_a;
                        ta = bgin.aer.tau[cb]; wa = bgin.aer.ssa[cb]; ga = bgin.aer.g[cb];
                    }
                    k_ext = k_ext_of(t, tc, ta, a.dz);
                    k_sca = k_sca_of(t, w0, tc, wc, ta, wa, a.dz);
                    k_sca_aer = (ta*wa) / a.dz;
                }
                else
                {
                    k_ext = k_ext_of(t, tc, a.dz);
                    k_sca = (t*w0 + tc*wc) / a.dz;
                }
                k_sca_cld = (tc*wc) / a.dz;
            }
            const F f_no_abs = clampf(F(1.) - (k_ext - k_sca)/kn_val, F(0.), F(1.));
            tally(abs_to, cell, count_of(weight*(F(1.) - f_no_abs)));
            weight = weight * f_no_abs;
            if (weight < F(0.5)) weight = (rng.next<F>() > weight) ? F(0.) : F(1.);
            if (!(weight > F(0.))) { alive = false; continue; }
            if (rng.next<F>()*(k_sca + (kn_val - k_ext)) < k_sca)
            {
                const F us = rng.next<F>()*k_sca;
                const bool cloud = us < k_sca_cld;
                [[maybe_unused]] bool aerosol = false;
                if constexpr (AER) aerosol = !cloud && us < k_sca_cld + k_sca_aer;
                if (aerosol) scatter_direction(rng, true, ga, g_max, ux, uy, uz);          // Henyey-Greenstein, with a phase table too
                else if constexpr (TABLE)
                {
                    if (in_bg) scatter_direction(rng, cloud, gc, g_max, ux, uy, uz);          // the table applies inside the grid only
                    else
                    {
                        const F re = cloud ? ph.in.cld_re[cell] : F(0.);          // cld_re (ncol, nz): one radius for all bands
                        scatter_direction_table(rng, cloud, table_of_band(ph.in, ibnd), ph.in.mu, re, ux, uy, uz);
                    }
                }
                else scatter_direction(rng, cloud, gc, g_max, ux, uy, uz);
                kind = 1;
            }
        }
    }
}

template<typename F>
__global__ void counts_to_flux_kernel(const size_t n, const u64* __restrict__ counts, const F scale, F* __restrict__ out)
{
    const size_t i = size_t(blockIdx.x)*blockDim.x + threadIdx.x;
    if (i < n) out[i] = out[i] + F(double(counts[i]) * 2.3283064365386963e-10) * scale;
}

// ---- host side

template<typename F>
void launch_k_null(int nx, int ny, int nz, int nbnd, int igpt, int top_at_1, const F* tau, const int* band_lims_gpt,
                   const F* cld_tau, F dz, int knx, int kny, int knz, F* k_null, hipStream_t st, const F* aer_tau = nullptr)
{
    const int n = knx*kny*knz;
    if (aer_tau != nullptr)
        k_null_aer_kernel<F><<<ceil_div(n, 256), 256, 0, st>>>(nx, ny, nz, nbnd, igpt, top_at_1, tau, band_lims_gpt, cld_tau, aer_tau, dz,
                                                               knx, kny, knz, k_null);
    else
        k_null_kernel<F><<<ceil_div(n, 256), 256, 0, st>>>(nx, ny, nz, nbnd, igpt, top_at_1, tau, band_lims_gpt, cld_tau, dz,
                                                           knx, kny, knz, k_null);
}

template<typename F>
void launch_trace(TraceArgs<F> a, const PhaseIn<F>& ph, const F mu0, const F azimuth, const F inc_dir, const F inc_dif, const u64 seed,
                  hipStream_t st, const FwBg<F,true>* bg = nullptr, const AerIn<F>* aer = nullptr)
{
    const double st_ = std::sqrt(std::max(0.0, 1.0 - double(mu0)*double(mu0)));
    a.sun_x = F(st_*std::cos(double(azimuth))); a.sun_y = F(st_*std::sin(double(azimuth))); a.sun_z = -mu0;
    a.dif_frac = inc_dif / (inc_dir + inc_dif);
    a.k0 = unsigned(seed & 0xFFFFFFFFull); a.k1 = unsigned(seed >> 32);
    const int blocks = int(std::min<long long>((a.nphotons + RT_BLOCK - 1) / RT_BLOCK, max_blocks()));
    if (bg != nullptr && aer != nullptr)
    {
        // the aerosol form: the background's profile has BG_ROWS_AER rows
        const size_t lds = bg_lds_numbers(bg->in.nbg, BG_ROWS_AER)*sizeof(F);
        const FwBg<F,true,true> ba{bg->in, bg->t, *aer};
        if (ph.given()) trace_kernel<F,true,true,true><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,true>{ph}, ba);
        else trace_kernel<F,false,true,true><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,false>{}, ba);
    }
    else if (bg != nullptr)
    {
        const size_t lds = bg_lds_numbers(bg->in.nbg)*sizeof(F);
        if (ph.given()) trace_kernel<F,true,true,false><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,true>{ph}, *bg);
        else trace_kernel<F,false,true,false><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,false>{}, *bg);
    }
    else if (ph.given()) trace_kernel<F,true,false,false><<<blocks, RT_BLOCK, 0, st>>>(a, PhaseArgs<F,true>{ph}, FwBg<F,false>{});
    else trace_kernel<F,false,false,false><<<blocks, RT_BLOCK, 0, st>>>(a, PhaseArgs<F,false>{}, FwBg<F,false>{});
}

// one number per background layer: out[b] += F(counts[b] 2^-32) scale[b]
template<typename F>
__global__ void bg_counts_to_flux_kernel(const int nbg, const u64* __restrict__ counts, const BgLevels<F> scale, F* __restrict__ out)
{
    const int b = blockIdx.x*blockDim.x + threadIdx.x;
    if (b < nbg) out[b] = out[b] + F(double(counts[b]) * 2.3283064365386963e-10) * scale.v[b];
}

// the profile of the background for one g-point (rrx_rt_common.h): one thread per layer
// AER: the 7-row profile with the background's aerosol triple (rrx_rt_common.h); a NULL triple writes zeros into the two new rows
template<typename F, bool AER>
__device__ __forceinline__ void bg_profile_layer(const int nbg, const int nbnd, const int igpt, const BgLevels<F>& dz_bg,
        const F* __restrict__ bg_tau, const F* __restrict__ bg_ssa, const int* __restrict__ band_lims_gpt,
        const F* __restrict__ bg_cld_tau, const F* __restrict__ bg_cld_ssa, const F* __restrict__ bg_cld_g,
        const AerIn<F> aer, F* __restrict__ profile)
{
    const int b = blockIdx.x*blockDim.x + threadIdx.x;
    if (b > nbg) return;
    const int n1 = nbg + 1;
    const int ibnd = bg_cld_tau != nullptr ? band_of(igpt, nbnd, band_lims_gpt) : -1;
    const F* __restrict__ tau_g = bg_tau + size_t(nbg)*igpt;
    const F* __restrict__ ctau_b = ibnd >= 0 ? bg_cld_tau + size_t(nbg)*ibnd : nullptr;
    [[maybe_unused]] int ibnd_a = -1;
    [[maybe_unused]] const F* __restrict__ atau_b = nullptr;
    if constexpr (AER)
    {
        ibnd_a = aer.tau != nullptr ? band_of(igpt, nbnd, band_lims_gpt) : -1;
        atau_b = ibnd_a >= 0 ? aer.tau + size_t(nbg)*ibnd_a : nullptr;
    }
    // the layers above b in index order; slot nbg: all of them
    F above = F(0.);
    for (int l = (b == nbg ? 0 : b + 1); l < nbg; ++l)
    {
        if constexpr (AER) above = above + ((tau_g[l] + (ctau_b != nullptr ? ctau_b[l] : F(0.))) + (atau_b != nullptr ? atau_b[l] : F(0.)));
        else above = above + (tau_g[l] + (ctau_b != nullptr ? ctau_b[l] : F(0.)));
    }
    profile[BG_TAU_ABOVE*n1 + b] = above;
    F k_ext = F(0.), k_sca = F(0.), k_sca_cld = F(0.), g = F(0.);
    [[maybe_unused]] F k_sca_aer = F(0.), g_aer = F(0.);
    if (b < nbg)
    {
        const F t = tau_g[b], w0 = bg_ssa[size_t(nbg)*igpt + b], dz = dz_bg.v[b];
        F tc = F(0.), wc = F(0.), gc = F(0.);
        if (ibnd >= 0) { tc = ctau_b[b]; wc = bg_cld_ssa[size_t(nbg)*ibnd + b]; gc = bg_cld_g[size_t(nbg)*ibnd + b]; }
        if constexpr (AER)
        {
            F ta = F(0.), wa = F(0.), ga = F(0.);
            if (ibnd_a >= 0) { ta = atau_b[b]; wa = aer.ssa[size_t(nbg)*ibnd_a + b]; ga = aer.g[size_t(nbg)*ibnd_a + b]; }
            k_ext = k_ext_of(t, tc, ta, dz);
            k_sca = k_sca_of(t, w0, tc, wc, ta, wa, dz);
            k_sca_aer = (ta*wa) / dz;
            g_aer = min(ga, F(1.) - Lim<F>::eps());
        }
        else
        {
            k_ext = k_ext_of(t, tc, dz);
            k_sca = (t*w0 + tc*wc) / dz;
        }
        k_sca_cld = (tc*wc) / dz;
        g = min(gc, F(1.) - Lim<F>::eps());
    }
    profile[BG_K_EXT*n1 + b] = k_ext; profile[BG_K_SCA*n1 + b] = k_sca; profile[BG_K_SCA_CLD*n1 + b] = k_sca_cld; profile[BG_G*n1 + b] = g;
    if constexpr (AER) { profile[BG_K_SCA_AER*n1 + b] = k_sca_aer; profile[BG_G_AER*n1 + b] = g_aer; }
}

template<typename F>
__global__ void bg_profile_kernel(const int nbg, const int ngpt, const int nbnd, const int igpt, const BgLevels<F> dz_bg,
        const F* __restrict__ bg_tau, const F* __restrict__ bg_ssa, const int* __restrict__ band_lims_gpt,
        const F* __restrict__ bg_cld_tau, const F* __restrict__ bg_cld_ssa, const F* __restrict__ bg_cld_g, F* __restrict__ profile)
{
    bg_profile_layer<F,false>(nbg, nbnd, igpt, dz_bg, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, bg_cld_g, AerIn<F>{}, profile);
}

template<typename F>
__global__ void bg_profile_aer_kernel(const int nbg, const int ngpt, const int nbnd, const int igpt, const BgLevels<F> dz_bg,
        const F* __restrict__ bg_tau, const F* __restrict__ bg_ssa, const int* __restrict__ band_lims_gpt,
        const F* __restrict__ bg_cld_tau, const F* __restrict__ bg_cld_ssa, const F* __restrict__ bg_cld_g, const AerIn<F> aer,
        F* __restrict__ profile)
{
    bg_profile_layer<F,true>(nbg, nbnd, igpt, dz_bg, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, bg_cld_g, aer, profile);
}

template<typename F>
BgLevels<F> bg_thicknesses(const int nbg, const F* dz_bg)
{
    BgLevels<F> d{};
    for (int b=0; b<nbg; ++b) d.v[b] = dz_bg[b];
    return d;
}

template<typename F>
void launch_bg_profile(int nbg, int ngpt, int nbnd, int igpt, const BgLevels<F>& dz_bg, const F* bg_tau, const F* bg_ssa,
                       const int* band_lims_gpt, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, F* profile, hipStream_t st,
                       const AerIn<F>* aer = nullptr)
{
    if (aer != nullptr)
        bg_profile_aer_kernel<F><<<ceil_div(nbg + 1, 64), 64, 0, st>>>(nbg, ngpt, nbnd, igpt, dz_bg, bg_tau, bg_ssa, band_lims_gpt,
                                                                      bg_cld_tau, bg_cld_ssa, bg_cld_g, *aer, profile);
    else
        bg_profile_kernel<F><<<ceil_div(nbg + 1, 64), 64, 0, st>>>(nbg, ngpt, nbnd, igpt, dz_bg, bg_tau, bg_ssa, band_lims_gpt,
                                                                  bg_cld_tau, bg_cld_ssa, bg_cld_g, profile);
}

template<typename F>
int bg_profile_entry(const char* entry, int nbg, int ngpt, int nbnd, int igpt, const F* dz_bg, const F* bg_tau, const F* bg_ssa,
                     const int* band_lims_gpt, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, F* profile, void* stream,
                     const AerIn<F>* aer = nullptr)
{
    // aer: the 7-row profile of rrx_rt_bg_profile_aer (its triple may be NULL)
    RRX_TRY
    check_nbg(nbg);
    if (check_extents({{"nbg", nbg}, {"ngpt", ngpt}})) return 0;
    if (nbnd < 0) throw std::runtime_error("nbnd is negative");
    if (igpt < 0 || igpt >= ngpt) throw std::runtime_error("igpt is outside [0, ngpt)");
    check_bg_medium(nbg, nbnd, dz_bg, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, bg_cld_g);
    if (aer != nullptr) check_aerosol("bg_aer_", nbnd, band_lims_gpt, aer->tau, aer->ssa, aer->g);
    check_needed({{"bg_profile", profile}});
    bg_levels<F>(nbg, dz_bg, 1, 1, F(1.));          // (the thicknesses are > 0)
    launch_bg_profile<F>(nbg, ngpt, nbnd, igpt, bg_thicknesses(nbg, dz_bg), bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa,
                         bg_cld_g, profile, static_cast<hipStream_t>(stream), aer);
    RRX_CATCH(entry)
}

template<typename F>
void launch_counts_to_flux(const size_t n, const u64* counts, const F scale, F* out, hipStream_t st)
{
    counts_to_flux_kernel<F><<<unsigned(ceil_div((long long)n, 256)), 256, 0, st>>>(n, counts, scale, out);
}

template<typename F>
int k_null_entry(const char* entry, int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, const F* tau,
                 const int* band_lims_gpt, const F* cld_tau, F dz, int knx, int kny, int knz, F* k_null, void* stream,
                 const F* aer_tau = nullptr)
{
    RRX_TRY
    if (check_extents({{"nx", nx}, {"ny", ny}, {"nz", nz}, {"ngpt", ngpt}})) return 0;
    if (nbnd < 0) throw std::runtime_error("nbnd is negative");
    check_needed({{"tau", tau}, {"k_null", k_null}});
    if (cld_tau != nullptr && band_lims_gpt == nullptr) throw std::runtime_error("band_lims_gpt is NULL");
    if (aer_tau != nullptr && band_lims_gpt == nullptr) throw std::runtime_error("band_lims_gpt is NULL");
    if (aer_tau != nullptr && nbnd < 1) throw std::runtime_error("nbnd must be >= 1 with an aerosol triple");
    if (igpt < 0 || igpt >= ngpt) throw std::runtime_error("igpt is outside [0, ngpt)");
    if (!(dz > F(0.))) throw std::runtime_error("dz must be > 0");
    check_grid(nx, ny, nz, knx, kny, knz);
    launch_k_null<F>(nx, ny, nz, nbnd, igpt, top_at_1 ? 1 : 0, tau, band_lims_gpt, cld_tau, dz, knx, kny, knz, k_null,
                     static_cast<hipStream_t>(stream), aer_tau);
    RRX_CATCH(entry)
}

template<typename F>
int trace_entry(const char* entry, int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, RrxBool independent_column,
                const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g,
                F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, F inc_dir, F inc_dif,
                int knx, int kny, int knz, const F* k_null, u64 seed, long long photon0, long long nphotons, int max_events,
                u64* sfc_dn_dir, u64* sfc_dn_dif, u64* sfc_up, u64* tod_up, u64* abs_dir, u64* abs_dif, u64* n_capped, void* stream,
                const PhaseIn<F> ph = PhaseIn<F>{}, const bool with_bg = false, const BgTallies<F> bt = BgTallies<F>{},
                const int nbg = 0, const F* dz_bg = nullptr, const F* bg_profile = nullptr, const AerIn<F>* aer = nullptr)
{
    // aer: rrx_rt_trace_counts_aer. With nbg > 0 bg_profile then has BG_ROWS_AER rows and the aerosol form runs whatever the grid's
    // triple is; with nbg = 0 and a NULL triple it is the _bg entry.
    RRX_TRY
    check_nbg(nbg);
    if (check_extents({{"nx", nx}, {"ny", ny}, {"nz", nz}, {"ngpt", ngpt}, {"nphotons", nphotons}})) return 0;
    if (nbnd < 0) throw std::runtime_error("nbnd is negative");
    if (photon0 < 0) throw std::runtime_error("photon0 is negative");
    check_needed({{"tau", tau}, {"ssa", ssa}, {"sfc_albedo", sfc_albedo}, {"k_null", k_null}, {"sfc_dn_dir", sfc_dn_dir},
                  {"sfc_dn_dif", sfc_dn_dif}, {"sfc_up", sfc_up}, {"tod_up", tod_up}, {"abs_dir", abs_dir}, {"abs_dif", abs_dif},
                  {"n_capped", n_capped}});
    check_cloud(nbnd, band_lims_gpt, cld_tau, cld_ssa, cld_g);
    if (aer != nullptr) check_aerosol("aer_", nbnd, band_lims_gpt, aer->tau, aer->ssa, aer->g);
    check_phase(ph, cld_tau);
    if (igpt < 0 || igpt >= ngpt) throw std::runtime_error("igpt is outside [0, ngpt)");
    check_scene(dx, dy, dz, mu0);
    if (inc_dir < F(0.) || inc_dif < F(0.) || !(inc_dir + inc_dif > F(0.))) throw std::runtime_error("inc_dir, inc_dif must be >= 0 with a positive sum");
    if (max_events < 1) throw std::runtime_error("max_events must be >= 1");
    check_grid(nx, ny, nz, knx, kny, knz);
    TraceArgs<F> a{nx, ny, nz, nbnd, igpt, top_at_1 ? 1 : 0, independent_column ? 1 : 0, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g,
                   dx, dy, dz, sfc_albedo, F(0.), F(0.), F(0.), F(0.), knx, kny, knz, k_null, 0u, 0u, u64(photon0), nphotons, max_events,
                   sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped};
    if (with_bg)
    {
        FwBg<F,true> bg{BgIn<F>{nbg, bg_profile, BgLevels<F>{}}, bt};
        if (nbg > 0)
        {
            check_needed({{"dz_bg", dz_bg}, {"bg_profile", bg_profile}, {"toa_up", bt.toa_up}, {"tod_dn_dir", bt.tod_dn_dir},
                          {"tod_dn_dif", bt.tod_dn_dif}, {"bg_abs_dir", bt.bg_abs_dir}, {"bg_abs_dif", bt.bg_abs_dif}});
            bg.in.z = bg_levels<F>(nbg, dz_bg, nz, knz, dz);
        }
        if (aer != nullptr && (aer->tau != nullptr || nbg > 0))
        {
            launch_trace<F>(a, ph, mu0, azimuth, inc_dir, inc_dif, seed, static_cast<hipStream_t>(stream), &bg, aer);
            return 0;
        }
        launch_trace<F>(a, ph, mu0, azimuth, inc_dir, inc_dif, seed, static_cast<hipStream_t>(stream), &bg);
        return 0;
    }
    launch_trace<F>(a, ph, mu0, azimuth, inc_dir, inc_dif, seed, static_cast<hipStream_t>(stream));
    RRX_CATCH(entry)
}

template<typename F>
int counts_to_flux_entry(const char* entry, long long n, const u64* counts, F scale, F* out, void* stream)
{
    RRX_TRY
    if (check_extents({{"n", n}})) return 0;
    check_needed({{"counts", counts}, {"out", out}});
    launch_counts_to_flux<F>(size_t(n), counts, scale, out, static_cast<hipStream_t>(stream));
    RRX_CATCH(entry)
}

template<typename F>
int raytracer_sw_entry(const char* entry, int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column,
                       const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g,
                       F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, const F* inc_dif,
                       int knx, int kny, int knz, long long photons_per_pixel, u64 seed, int max_events,
                       F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, u64* n_capped, void* stream,
                       const PhaseIn<F> ph = PhaseIn<F>{}, const bool with_bg = false, F* const* bg_out = nullptr, const int nbg = 0,
                       const F* dz_bg = nullptr, const F* bg_tau = nullptr, const F* bg_ssa = nullptr, const F* bg_cld_tau = nullptr,
                       const F* bg_cld_ssa = nullptr, const F* bg_cld_g = nullptr, const AerIn<F>* aer = nullptr,
                       const AerIn<F>* bg_aer = nullptr)
{
    // bg_out: toa_up, tod_dn_dir, tod_dn_dif (ncol), bg_abs_dir, bg_abs_dif (nbg)
    // aer, bg_aer: rrx_raytracer_sw_aer; with both triples NULL (bg_aer is not read when nbg = 0) it is the _bg entry
    RRX_TRY
    check_nbg(nbg);
    if (check_extents({{"nx", nx}, {"ny", ny}, {"nz", nz}, {"ngpt", ngpt}, {"photons_per_pixel", photons_per_pixel}})) return 0;
    if (nbnd < 0) throw std::runtime_error("nbnd is negative");
    check_needed({{"tau", tau}, {"ssa", ssa}, {"sfc_albedo", sfc_albedo}, {"inc_dir", inc_dir}, {"inc_dif", inc_dif},
                  {"sfc_dn_dir", sfc_dn_dir}, {"sfc_dn_dif", sfc_dn_dif}, {"sfc_up", sfc_up}, {"tod_up", tod_up}, {"abs_dir", abs_dir},
                  {"abs_dif", abs_dif}, {"n_capped", n_capped}});
    check_cloud(nbnd, band_lims_gpt, cld_tau, cld_ssa, cld_g);
    if (aer != nullptr) check_aerosol("aer_", nbnd, band_lims_gpt, aer->tau, aer->ssa, aer->g);
    check_phase(ph, cld_tau);
    check_scene(dx, dy, dz, mu0);
    for (int g=0; g<ngpt; ++g)
        if (inc_dir[g] < F(0.) || inc_dif[g] < F(0.)) throw std::runtime_error("inc_dir, inc_dif must be >= 0");
    if (max_events < 1) throw std::runtime_error("max_events must be >= 1");
    check_grid(nx, ny, nz, knx, kny, knz);
    const bool bg_on = with_bg && nbg > 0;
    BgLevels<F> lev{}, thick{};
    if (bg_on && bg_aer != nullptr) check_aerosol("bg_aer_", nbnd, band_lims_gpt, bg_aer->tau, bg_aer->ssa, bg_aer->g);
    // the aerosol form runs when either triple is given
    const AerIn<F> aer_grid = aer != nullptr ? *aer : AerIn<F>{}, aer_bg = (bg_on && bg_aer != nullptr) ? *bg_aer : AerIn<F>{};
    const bool aer_on = with_bg && (aer_grid.tau != nullptr || aer_bg.tau != nullptr);
    if (bg_on)
    {
        check_bg_medium(nbg, nbnd, dz_bg, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, bg_cld_g);
        check_needed({{"toa_up", bg_out[0]}, {"tod_dn_dir", bg_out[1]}, {"tod_dn_dif", bg_out[2]}, {"bg_abs_dir", bg_out[3]},
                      {"bg_abs_dif", bg_out[4]}});
        lev = bg_levels<F>(nbg, dz_bg, nz, knz, dz);
        thick = bg_thicknesses(nbg, dz_bg);
    }

    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t ncol = size_t(nx)*ny, n_sfc = 4*ncol, n_abs = 2*ncol*nz;
    const size_t n_bgc = bg_on ? 3*ncol + 2*size_t(nbg) : 0, n_counts = n_sfc + n_abs + n_bgc;
    const size_t n_kn = (size_t(knx)*kny*knz*sizeof(F) + sizeof(u64) - 1) / sizeof(u64);
    const size_t n_prof = bg_on ? (size_t(aer_on ? BG_ROWS_AER : BG_ROWS)*(nbg + 1)*sizeof(F) + sizeof(u64) - 1) / sizeof(u64) : 0;
    WorkspaceLease lease(st);
    u64* counts = lease.get<u64>(n_counts + n_kn + n_prof);
    F* k_null = reinterpret_cast<F*>(counts + n_counts);
    F* profile = reinterpret_cast<F*>(counts + n_counts + n_kn);
    bool ok = hipMemsetAsync(n_capped, 0, sizeof(u64), st) == hipSuccess;
    if (bg_on)
    {
        for (int n=0; n<3; ++n) ok = ok && hipMemsetAsync(bg_out[n], 0, ncol*sizeof(F), st) == hipSuccess;
        for (int n=3; n<5; ++n) ok = ok && hipMemsetAsync(bg_out[n], 0, size_t(nbg)*sizeof(F), st) == hipSuccess;
    }
    for (F* out : {sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up}) ok = ok && hipMemsetAsync(out, 0, ncol*sizeof(F), st) == hipSuccess;
    for (F* out : {abs_dir, abs_dif}) ok = ok && hipMemsetAsync(out, 0, ncol*nz*sizeof(F), st) == hipSuccess;
    if (!ok) throw std::runtime_error("zeroing the outputs failed");
    const long long nphotons = photons_per_pixel*(long long)ncol;
    for (int g=0; g<ngpt; ++g)
    {
        if (!(inc_dir[g] + inc_dif[g] > F(0.))) continue;
        if (hipMemsetAsync(counts, 0, n_counts*sizeof(u64), st) != hipSuccess) throw std::runtime_error("zeroing the counts failed");
        launch_k_null<F>(nx, ny, nz, nbnd, g, top_at_1 ? 1 : 0, tau, band_lims_gpt, cld_tau, dz, knx, kny, knz, k_null, st, aer_grid.tau);
        u64* c = counts;
        TraceArgs<F> a{nx, ny, nz, nbnd, g, top_at_1 ? 1 : 0, independent_column ? 1 : 0, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g,
                       dx, dy, dz, sfc_albedo, F(0.), F(0.), F(0.), F(0.), knx, kny, knz, k_null, 0u, 0u, 0ull, nphotons, max_events,
                       c, c + ncol, c + 2*ncol, c + 3*ncol, c + n_sfc, c + n_sfc + ncol*nz, n_capped};
        const F scale = (inc_dir[g] + inc_dif[g]) / F(photons_per_pixel);
        if (with_bg)
        {
            u64* cb = c + n_sfc + n_abs;
            FwBg<F,true> bg{BgIn<F>{bg_on ? nbg : 0, profile, lev}, BgTallies<F>{cb, cb + ncol, cb + 2*ncol, cb + 3*ncol, cb + 3*ncol + nbg}};
            if (bg_on) launch_bg_profile<F>(nbg, ngpt, nbnd, g, thick, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, bg_cld_g, profile, st,
                                            aer_on ? &aer_bg : nullptr);
            launch_trace<F>(a, ph, mu0, azimuth, inc_dir[g], inc_dif[g], seed, st, &bg, aer_on ? &aer_grid : nullptr);
            if (bg_on)
            {
                launch_counts_to_flux<F>(ncol, bg.t.toa_up, scale, bg_out[0], st);
                launch_counts_to_flux<F>(ncol, bg.t.tod_dn_dir, scale, bg_out[1], st);
                launch_counts_to_flux<F>(ncol, bg.t.tod_dn_dif, scale, bg_out[2], st);
                // W m-3 of a domain-wide layer: the counts of all columns over the layer's thickness and the number of columns
                BgLevels<F> per_layer{};
                for (int b=0; b<nbg; ++b) per_layer.v[b] = (scale / dz_bg[b]) / F(ncol);
                bg_counts_to_flux_kernel<F><<<ceil_div(nbg, 64), 64, 0, st>>>(nbg, bg.t.bg_abs_dir, per_layer, bg_out[3]);
                bg_counts_to_flux_kernel<F><<<ceil_div(nbg, 64), 64, 0, st>>>(nbg, bg.t.bg_abs_dif, per_layer, bg_out[4]);
            }
        }
        else launch_trace<F>(a, ph, mu0, azimuth, inc_dir[g], inc_dif[g], seed, st);
        launch_counts_to_flux<F>(ncol, a.sfc_dn_dir, scale, sfc_dn_dir, st);
        launch_counts_to_flux<F>(ncol, a.sfc_dn_dif, scale, sfc_dn_dif, st);
        launch_counts_to_flux<F>(ncol, a.sfc_up, scale, sfc_up, st);
        launch_counts_to_flux<F>(ncol, a.tod_up, scale, tod_up, st);
        launch_counts_to_flux<F>(ncol*nz, a.abs_dir, scale / dz, abs_dir, st);
        launch_counts_to_flux<F>(ncol*nz, a.abs_dif, scale / dz, abs_dif, st);
    }
    RRX_CATCH(entry)
}

// ---- all g-points in one launch (rrx_rt_common.h)

// bg_profile_aer_kernel for every g-point, blockIdx.y counting them: slice g of profile (ngpt, BG_ROWS_AER, nbg+1)
template<typename F>
__global__ void bg_profile_all_kernel(const int nbg, const int nbnd, const BgLevels<F> dz_bg,
        const F* __restrict__ bg_tau, const F* __restrict__ bg_ssa, const int* __restrict__ band_lims_gpt,
        const F* __restrict__ bg_cld_tau, const F* __restrict__ bg_cld_ssa, const F* __restrict__ bg_cld_g, const AerIn<F> aer,
        F* __restrict__ profile)
{
    bg_profile_layer<F,true>(nbg, nbnd, int(blockIdx.y), dz_bg, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, bg_cld_g, aer,
                             profile + size_t(blockIdx.y)*BG_ROWS_AER*(nbg + 1));
}

// k_null of the ng g-points from g0 on
template<typename F>
void launch_k_null_all(int nx, int ny, int nz, int nbnd, int g0, int ng, int top_at_1, const F* tau, const int* band_lims_gpt,
                       const F* cld_tau, const F* aer_tau, F dz, int knx, int kny, int knz, F* k_null, hipStream_t st)
{
    const dim3 grid(unsigned(ceil_div(knx*kny*knz, 256)), unsigned(ng));
    k_null_all_kernel<F><<<grid, 256, 0, st>>>(nx, ny, nz, nbnd, g0, top_at_1, tau, band_lims_gpt, cld_tau, aer_tau, dz, knx, kny, knz, k_null);
}

template<typename F>
void launch_bg_profile_all(int nbg, int ngpt, int nbnd, const BgLevels<F>& dz_bg, const F* bg_tau, const F* bg_ssa, const int* band_lims_gpt,
                           const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, const AerIn<F>& aer, F* profile, hipStream_t st)
{
    const dim3 grid(unsigned(ceil_div(nbg + 1, 64)), unsigned(ngpt));
    bg_profile_all_kernel<F><<<grid, 64, 0, st>>>(nbg, nbnd, dz_bg, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, bg_cld_g, aer, profile);
}

// a.photon0 / a.nphotons: the range of the concatenated list; a.k_null: the slices from g-point b.sp.kn_g0 on
template<typename F>
void launch_trace_spectral(TraceArgs<F> a, const PhaseIn<F>& ph, const F mu0, const F azimuth, const u64 seed, hipStream_t st,
                           const FwBg<F,true,true,true>& b)
{
    const double st_ = std::sqrt(std::max(0.0, 1.0 - double(mu0)*double(mu0)));
    a.sun_x = F(st_*std::cos(double(azimuth))); a.sun_y = F(st_*std::sin(double(azimuth))); a.sun_z = -mu0;
    a.k0 = unsigned(seed & 0xFFFFFFFFull); a.k1 = unsigned(seed >> 32);
    const int blocks = int(std::min<long long>((a.nphotons + RT_BLOCK - 1) / RT_BLOCK, max_blocks()));
    const size_t lds = spectral_lds_bytes(b.sp.ngpt, b.in.nbg, sizeof(F));
    if (ph.given()) trace_kernel<F,true,true,true,true><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,true>{ph}, b);
    else trace_kernel<F,false,true,true,true><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,false>{}, b);
}

inline void check_spectral_ngpt(const int ngpt)
{
    if (ngpt > RT_SPECTRAL_MAX_GPT) throw std::runtime_error("ngpt must be <= 1024 in the spectral form");
}

template<typename F>
int k_null_all_entry(const char* entry, int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, const F* tau,
                     const int* band_lims_gpt, const F* cld_tau, F dz, int knx, int kny, int knz, F* k_null, const F* aer_tau, void* stream)
{
    RRX_TRY
    if (check_extents({{"nx", nx}, {"ny", ny}, {"nz", nz}, {"ngpt", ngpt}})) return 0;
    if (nbnd < 0) throw std::runtime_error("nbnd is negative");
    check_spectral_ngpt(ngpt);
    check_needed({{"tau", tau}, {"k_null", k_null}});
    if ((cld_tau != nullptr || aer_tau != nullptr) && band_lims_gpt == nullptr) throw std::runtime_error("band_lims_gpt is NULL");
    if (aer_tau != nullptr && nbnd < 1) throw std::runtime_error("nbnd must be >= 1 with an aerosol triple");
    if (!(dz > F(0.))) throw std::runtime_error("dz must be > 0");
    check_grid(nx, ny, nz, knx, kny, knz);
    launch_k_null_all<F>(nx, ny, nz, nbnd, 0, ngpt, top_at_1 ? 1 : 0, tau, band_lims_gpt, cld_tau, aer_tau, dz, knx, kny, knz, k_null,
                         static_cast<hipStream_t>(stream));
    RRX_CATCH(entry)
}

template<typename F>
int bg_profile_all_entry(const char* entry, int nbg, int ngpt, int nbnd, const F* dz_bg, const F* bg_tau, const F* bg_ssa,
                         const int* band_lims_gpt, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, F* profile,
                         const AerIn<F> aer, void* stream)
{
    RRX_TRY
    check_nbg(nbg);
    if (check_extents({{"nbg", nbg}, {"ngpt", ngpt}})) return 0;
    if (nbnd < 0) throw std::runtime_error("nbnd is negative");
    check_spectral_ngpt(ngpt);
    check_bg_medium(nbg, nbnd, dz_bg, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, bg_cld_g);
    check_aerosol("bg_aer_", nbnd, band_lims_gpt, aer.tau, aer.ssa, aer.g);
    check_needed({{"bg_profile", profile}});
    bg_levels<F>(nbg, dz_bg, 1, 1, F(1.));          // (the thicknesses are > 0)
    launch_bg_profile_all<F>(nbg, ngpt, nbnd, bg_thicknesses(nbg, dz_bg), bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, bg_cld_g, aer,
                             profile, static_cast<hipStream_t>(stream));
    RRX_CATCH(entry)
}

// photon_end, weight0, dif_frac are device arrays: the entry cannot look into them. The kernel stays inside its arrays whatever
// photon_end holds (the search is bounded by ngpt and a photon beyond photon_end[ngpt] is stepped over); the callers that form the
// list on the host (rrx_raytracer_sw_spectral, the Python binding) refuse a list that does not ascend.
template<typename F>
int trace_spectral_entry(const char* entry, int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column,
                         const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g,
                         F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const long long* photon_end, const F* weight0, const F* dif_frac,
                         int knx, int kny, int knz, const F* k_null, u64 seed, long long photon0, long long nphotons, int max_events,
                         u64* sfc_dn_dir, u64* sfc_dn_dif, u64* sfc_up, u64* tod_up, u64* abs_dir, u64* abs_dif, u64* n_capped,
                         const BgTallies<F> bt, const PhaseIn<F> ph, const int nbg, const F* dz_bg, const F* bg_profile, const AerIn<F> aer,
                         void* stream)
{
    RRX_TRY
    check_nbg(nbg);
    if (check_extents({{"nx", nx}, {"ny", ny}, {"nz", nz}, {"ngpt", ngpt}, {"nphotons", nphotons}})) return 0;
    if (nbnd < 0) throw std::runtime_error("nbnd is negative");
    check_spectral_ngpt(ngpt);
    if (photon0 < 0) throw std::runtime_error("photon0 is negative");
    check_needed({{"tau", tau}, {"ssa", ssa}, {"sfc_albedo", sfc_albedo}, {"photon_end", photon_end}, {"weight0", weight0},
                  {"dif_frac", dif_frac}, {"k_null", k_null}, {"sfc_dn_dir", sfc_dn_dir}, {"sfc_dn_dif", sfc_dn_dif}, {"sfc_up", sfc_up},
                  {"tod_up", tod_up}, {"abs_dir", abs_dir}, {"abs_dif", abs_dif}, {"n_capped", n_capped}});
    check_cloud(nbnd, band_lims_gpt, cld_tau, cld_ssa, cld_g);
    check_aerosol("aer_", nbnd, band_lims_gpt, aer.tau, aer.ssa, aer.g);
    check_phase(ph, cld_tau);
    check_scene(dx, dy, dz, mu0);
    if (max_events < 1) throw std::runtime_error("max_events must be >= 1");
    check_grid(nx, ny, nz, knx, kny, knz);
    TraceArgs<F> a{nx, ny, nz, nbnd, 0, top_at_1 ? 1 : 0, independent_column ? 1 : 0, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g,
                   dx, dy, dz, sfc_albedo, F(0.), F(0.), F(0.), F(0.), knx, kny, knz, k_null, 0u, 0u, u64(photon0), nphotons, max_events,
                   sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped};
    FwBg<F,true,true,true> b{BgIn<F>{nbg, bg_profile, BgLevels<F>{}}, bt, aer, SpecIn<F>{ngpt, 0, photon_end, weight0, dif_frac}};
    if (nbg > 0)
    {
        check_needed({{"dz_bg", dz_bg}, {"bg_profile", bg_profile}, {"toa_up", bt.toa_up}, {"tod_dn_dir", bt.tod_dn_dir},
                      {"tod_dn_dif", bt.tod_dn_dif}, {"bg_abs_dir", bt.bg_abs_dir}, {"bg_abs_dif", bt.bg_abs_dif}});
        b.in.z = bg_levels<F>(nbg, dz_bg, nz, knz, dz);
    }
    launch_trace_spectral<F>(a, ph, mu0, azimuth, seed, static_cast<hipStream_t>(stream), b);
    RRX_CATCH(entry)
}

// g-points per trace launch of rrx_raytracer_sw_spectral: the largest chunk whose k_null fits 1 GiB, or
// RRX_RT_SPECTRAL_GPT_PER_LAUNCH from the environment, read at every call. The result does not depend on it.
inline int spectral_gpt_per_launch(const size_t k_null_bytes_per_gpt, const int ngpt)
{
    if (const char* e = std::getenv("RRX_RT_SPECTRAL_GPT_PER_LAUNCH")) { const int n = std::atoi(e); if (n >= 1) return std::min(n, ngpt); }
    const size_t fit = (size_t(1) << 30) / std::max<size_t>(k_null_bytes_per_gpt, 1);
    return int(std::min<size_t>(std::max<size_t>(fit, 1), size_t(ngpt)));
}

// rrx_raytracer_sw_aer with photons_per_pixel_gpt[g] = m_g photons per pixel of g-point g (host array): one trace launch per chunk of
// consecutive g-points, the counts of all chunks added in integers and converted once with the common unit U = S/P
template<typename F>
int raytracer_sw_spectral_entry(const char* entry, int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column,
                       const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g,
                       F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, const F* inc_dif,
                       int knx, int kny, int knz, const long long* m, u64 seed, int max_events,
                       F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, u64* n_capped, void* stream,
                       const PhaseIn<F> ph, F* const* bg_out, const int nbg, const F* dz_bg, const F* bg_tau, const F* bg_ssa,
                       const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, const AerIn<F> aer, const AerIn<F> bg_aer)
{
    RRX_TRY
    check_nbg(nbg);
    if (check_extents({{"nx", nx}, {"ny", ny}, {"nz", nz}, {"ngpt", ngpt}})) return 0;
    if (nbnd < 0) throw std::runtime_error("nbnd is negative");
    check_spectral_ngpt(ngpt);
    check_needed({{"tau", tau}, {"ssa", ssa}, {"sfc_albedo", sfc_albedo}, {"inc_dir", inc_dir}, {"inc_dif", inc_dif},
                  {"photons_per_pixel_gpt", m}, {"sfc_dn_dir", sfc_dn_dir}, {"sfc_dn_dif", sfc_dn_dif}, {"sfc_up", sfc_up}, {"tod_up", tod_up},
                  {"abs_dir", abs_dir}, {"abs_dif", abs_dif}, {"n_capped", n_capped}});
    check_cloud(nbnd, band_lims_gpt, cld_tau, cld_ssa, cld_g);
    check_aerosol("aer_", nbnd, band_lims_gpt, aer.tau, aer.ssa, aer.g);
    check_phase(ph, cld_tau);
    check_scene(dx, dy, dz, mu0);
    const size_t ncol = size_t(nx)*ny;
    // the photon list, the weights and the common unit U = S/P (rrx_rt_common.h)
    std::vector<long long> photon_end(size_t(ngpt) + 1, 0);
    std::vector<F> weight0(ngpt, F(0.)), dif_frac(ngpt, F(0.));
    long long P = 0;
    F S = F(0.);
    for (int g=0; g<ngpt; ++g)
    {
        if (inc_dir[g] < F(0.) || inc_dif[g] < F(0.)) throw std::runtime_error("inc_dir, inc_dif must be >= 0");
        if (m[g] < 0) throw std::runtime_error("photons_per_pixel_gpt is negative at g-point " + std::to_string(g));
        if (m[g] > 0 && !(inc_dir[g] + inc_dif[g] > F(0.)))
            throw std::runtime_error("photons_per_pixel_gpt is > 0 at g-point " + std::to_string(g) + ", which has no incident flux");
        if (m[g] > (0x7FFFFFFFFFFFFFFFll - photon_end[g]) / (long long)ncol) throw std::runtime_error("the photon list exceeds 2^63 - 1");
        photon_end[g+1] = photon_end[g] + m[g]*(long long)ncol;
        P += m[g];
        if (m[g] > 0) S = S + (inc_dir[g] + inc_dif[g]);
    }
    if (max_events < 1) throw std::runtime_error("max_events must be >= 1");
    check_grid(nx, ny, nz, knx, kny, knz);
    const F U = P > 0 ? S / F(P) : F(0.);
    for (int g=0; g<ngpt; ++g)
        if (m[g] > 0)
        {
            const F inc = inc_dir[g] + inc_dif[g];
            weight0[g] = (inc / F(m[g])) / U;
            dif_frac[g] = inc_dif[g] / inc;
        }
    const bool bg_on = nbg > 0;
    BgLevels<F> lev{}, thick{};
    AerIn<F> aer_bg{};
    if (bg_on)
    {
        check_aerosol("bg_aer_", nbnd, band_lims_gpt, bg_aer.tau, bg_aer.ssa, bg_aer.g);
        aer_bg = bg_aer;
        check_bg_medium(nbg, nbnd, dz_bg, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, bg_cld_g);
        check_needed({{"toa_up", bg_out[0]}, {"tod_dn_dir", bg_out[1]}, {"tod_dn_dif", bg_out[2]}, {"bg_abs_dir", bg_out[3]},
                      {"bg_abs_dif", bg_out[4]}});
        lev = bg_levels<F>(nbg, dz_bg, nz, knz, dz);
        thick = bg_thicknesses(nbg, dz_bg);
    }

    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n_sfc = 4*ncol, n_abs = 2*ncol*nz;
    const size_t n_bgc = bg_on ? 3*ncol + 2*size_t(nbg) : 0, n_counts = n_sfc + n_abs + n_bgc;
    const size_t nkn = size_t(knx)*kny*knz;
    const int chunk = spectral_gpt_per_launch(nkn*sizeof(F), ngpt);
    const auto words = [](const size_t bytes) { return (bytes + sizeof(u64) - 1) / sizeof(u64); };
    const size_t n_kn = words(nkn*chunk*sizeof(F));
    const size_t n_prof = bg_on ? words(size_t(ngpt)*BG_ROWS_AER*(nbg + 1)*sizeof(F)) : 0;
    const size_t n_pe = size_t(ngpt) + 1, n_w = words(size_t(ngpt)*sizeof(F));
    WorkspaceLease lease(st);
    u64* counts = lease.get<u64>(n_counts + n_kn + n_prof + n_pe + 2*n_w);
    F* k_null = reinterpret_cast<F*>(counts + n_counts);
    F* profile = reinterpret_cast<F*>(counts + n_counts + n_kn);
    long long* d_pe = reinterpret_cast<long long*>(counts + n_counts + n_kn + n_prof);
    F* d_w0 = reinterpret_cast<F*>(counts + n_counts + n_kn + n_prof + n_pe);
    F* d_df = reinterpret_cast<F*>(counts + n_counts + n_kn + n_prof + n_pe + n_w);
    bool ok = hipMemsetAsync(n_capped, 0, sizeof(u64), st) == hipSuccess;
    if (bg_on)
    {
        for (int n=0; n<3; ++n) ok = ok && hipMemsetAsync(bg_out[n], 0, ncol*sizeof(F), st) == hipSuccess;
        for (int n=3; n<5; ++n) ok = ok && hipMemsetAsync(bg_out[n], 0, size_t(nbg)*sizeof(F), st) == hipSuccess;
    }
    for (F* out : {sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up}) ok = ok && hipMemsetAsync(out, 0, ncol*sizeof(F), st) == hipSuccess;
    for (F* out : {abs_dir, abs_dif}) ok = ok && hipMemsetAsync(out, 0, ncol*nz*sizeof(F), st) == hipSuccess;
    if (!ok) throw std::runtime_error("zeroing the outputs failed");
    if (P == 0) return 0;
    ok = hipMemsetAsync(counts, 0, n_counts*sizeof(u64), st) == hipSuccess
      && hipMemcpyAsync(d_pe, photon_end.data(), n_pe*sizeof(long long), hipMemcpyHostToDevice, st) == hipSuccess
      && hipMemcpyAsync(d_w0, weight0.data(), size_t(ngpt)*sizeof(F), hipMemcpyHostToDevice, st) == hipSuccess
      && hipMemcpyAsync(d_df, dif_frac.data(), size_t(ngpt)*sizeof(F), hipMemcpyHostToDevice, st) == hipSuccess
      && hipStreamSynchronize(st) == hipSuccess;          // (the host arrays end with this call)
    if (!ok) throw std::runtime_error("zeroing the counts or copying the photon list failed");
    if (bg_on) launch_bg_profile_all<F>(nbg, ngpt, nbnd, thick, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, bg_cld_g, aer_bg, profile, st);
    u64* c = counts;
    u64* cb = c + n_sfc + n_abs;
    FwBg<F,true,true,true> b{BgIn<F>{bg_on ? nbg : 0, profile, lev}, BgTallies<F>{cb, cb + ncol, cb + 2*ncol, cb + 3*ncol, cb + 3*ncol + nbg}, aer,
                             SpecIn<F>{ngpt, 0, d_pe, d_w0, d_df}};
    for (int g0=0; g0<ngpt; g0+=chunk)
    {
        const int g1 = std::min(g0 + chunk, ngpt);
        const long long n = photon_end[g1] - photon_end[g0];
        if (n == 0) continue;
        launch_k_null_all<F>(nx, ny, nz, nbnd, g0, g1 - g0, top_at_1 ? 1 : 0, tau, band_lims_gpt, cld_tau, aer.tau, dz, knx, kny, knz, k_null, st);
        TraceArgs<F> a{nx, ny, nz, nbnd, 0, top_at_1 ? 1 : 0, independent_column ? 1 : 0, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g,
                       dx, dy, dz, sfc_albedo, F(0.), F(0.), F(0.), F(0.), knx, kny, knz, k_null, 0u, 0u, u64(photon_end[g0]), n, max_events,
                       c, c + ncol, c + 2*ncol, c + 3*ncol, c + n_sfc, c + n_sfc + ncol*nz, n_capped};
        b.sp.kn_g0 = g0;
        launch_trace_spectral<F>(a, ph, mu0, azimuth, seed, st, b);
    }
    if (bg_on)
    {
        launch_counts_to_flux<F>(ncol, b.t.toa_up, U, bg_out[0], st);
        launch_counts_to_flux<F>(ncol, b.t.tod_dn_dir, U, bg_out[1], st);
        launch_counts_to_flux<F>(ncol, b.t.tod_dn_dif, U, bg_out[2], st);
        BgLevels<F> per_layer{};
        for (int l=0; l<nbg; ++l) per_layer.v[l] = (U / dz_bg[l]) / F(ncol);
        bg_counts_to_flux_kernel<F><<<ceil_div(nbg, 64), 64, 0, st>>>(nbg, b.t.bg_abs_dir, per_layer, bg_out[3]);
        bg_counts_to_flux_kernel<F><<<ceil_div(nbg, 64), 64, 0, st>>>(nbg, b.t.bg_abs_dif, per_layer, bg_out[4]);
    }
    launch_counts_to_flux<F>(ncol, c, U, sfc_dn_dir, st);
    launch_counts_to_flux<F>(ncol, c + ncol, U, sfc_dn_dif, st);
    launch_counts_to_flux<F>(ncol, c + 2*ncol, U, sfc_up, st);
    launch_counts_to_flux<F>(ncol, c + 3*ncol, U, tod_up, st);
    launch_counts_to_flux<F>(ncol*nz, c + n_sfc, U / dz, abs_dir, st);
    launch_counts_to_flux<F>(ncol*nz, c + n_sfc + ncol*nz, U / dz, abs_dif, st);
    RRX_CATCH(entry)
}
}  // namespace

extern "C"
{
#define RRX_DEFINE_RT(F, SFX) \
int rrx_rt_k_null##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, const F* tau, const int* band_lims_gpt, \
        const F* cld_tau, F dz, int knx, int kny, int knz, F* k_null, void* stream) \
{ return k_null_entry<F>("rrx_rt_k_null" #SFX, nx, ny, nz, ngpt, nbnd, igpt, top_at_1, tau, band_lims_gpt, cld_tau, dz, knx, kny, knz, k_null, stream); } \
int rrx_rt_trace_counts##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, F inc_dir, F inc_dif, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long photon0, long long nphotons, int max_events, \
        unsigned long long* sfc_dn_dir, unsigned long long* sfc_dn_dif, unsigned long long* sfc_up, unsigned long long* tod_up, \
        unsigned long long* abs_dir, unsigned long long* abs_dif, unsigned long long* n_capped, void* stream) \
{ return trace_entry<F>("rrx_rt_trace_counts" #SFX, nx, ny, nz, ngpt, nbnd, igpt, top_at_1, independent_column, tau, ssa, band_lims_gpt, \
                        cld_tau, cld_ssa, cld_g, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, k_null, seed, \
                        photon0, nphotons, max_events, sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped, stream); } \
int rrx_rt_counts_to_flux##SFX(long long n, const unsigned long long* counts, F scale, F* out, void* stream) \
{ return counts_to_flux_entry<F>("rrx_rt_counts_to_flux" #SFX, n, counts, scale, out, stream); } \
int rrx_raytracer_sw##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, const F* inc_dif, int knx, int kny, int knz, \
        long long photons_per_pixel, unsigned long long seed, int max_events, \
        F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, unsigned long long* n_capped, void* stream) \
{ return raytracer_sw_entry<F>("rrx_raytracer_sw" #SFX, nx, ny, nz, ngpt, nbnd, top_at_1, independent_column, tau, ssa, band_lims_gpt, \
                               cld_tau, cld_ssa, cld_g, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, \
                               photons_per_pixel, seed, max_events, sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped, stream); } \
int rrx_rt_trace_counts_phase##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, F inc_dir, F inc_dif, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long photon0, long long nphotons, int max_events, \
        unsigned long long* sfc_dn_dir, unsigned long long* sfc_dn_dif, unsigned long long* sfc_up, unsigned long long* tod_up, \
        unsigned long long* abs_dir, unsigned long long* abs_dif, unsigned long long* n_capped, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, void* stream) \
{ return trace_entry<F>("rrx_rt_trace_counts_phase" #SFX, nx, ny, nz, ngpt, nbnd, igpt, top_at_1, independent_column, tau, ssa, band_lims_gpt, \
                        cld_tau, cld_ssa, cld_g, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, k_null, seed, \
                        photon0, nphotons, max_events, sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped, stream, \
                        PhaseIn<F>{nmu, nre, re0, dre, mu, phase, cdf, cld_re}); } \
int rrx_raytracer_sw_phase##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, const F* inc_dif, int knx, int kny, int knz, \
        long long photons_per_pixel, unsigned long long seed, int max_events, \
        F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, unsigned long long* n_capped, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, void* stream) \
{ return raytracer_sw_entry<F>("rrx_raytracer_sw_phase" #SFX, nx, ny, nz, ngpt, nbnd, top_at_1, independent_column, tau, ssa, band_lims_gpt, \
                               cld_tau, cld_ssa, cld_g, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, \
                               photons_per_pixel, seed, max_events, sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped, stream, \
                               PhaseIn<F>{nmu, nre, re0, dre, mu, phase, cdf, cld_re}); } \
int rrx_rt_bg_profile##SFX(int nbg, int ngpt, int nbnd, int igpt, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const int* band_lims_gpt, \
        const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, F* bg_profile, void* stream) \
{ return bg_profile_entry<F>("rrx_rt_bg_profile" #SFX, nbg, ngpt, nbnd, igpt, dz_bg, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, \
                             bg_cld_g, bg_profile, stream); } \
int rrx_rt_trace_counts_bg##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, F inc_dir, F inc_dif, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long photon0, long long nphotons, int max_events, \
        unsigned long long* sfc_dn_dir, unsigned long long* sfc_dn_dif, unsigned long long* sfc_up, unsigned long long* tod_up, \
        unsigned long long* abs_dir, unsigned long long* abs_dif, unsigned long long* n_capped, \
        unsigned long long* toa_up, unsigned long long* tod_dn_dir, unsigned long long* tod_dn_dif, \
        unsigned long long* bg_abs_dir, unsigned long long* bg_abs_dif, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_profile, void* stream) \
{ return trace_entry<F>("rrx_rt_trace_counts_bg" #SFX, nx, ny, nz, ngpt, nbnd, igpt, top_at_1, independent_column, tau, ssa, band_lims_gpt, \
                        cld_tau, cld_ssa, cld_g, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, k_null, seed, \
                        photon0, nphotons, max_events, sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped, stream, \
                        PhaseIn<F>{nmu, nre, re0, dre, mu, phase, cdf, cld_re}, true, \
                        BgTallies<F>{toa_up, tod_dn_dir, tod_dn_dif, bg_abs_dir, bg_abs_dif}, nbg, dz_bg, bg_profile); } \
int rrx_raytracer_sw_bg##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, const F* inc_dif, int knx, int kny, int knz, \
        long long photons_per_pixel, unsigned long long seed, int max_events, \
        F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, unsigned long long* n_capped, \
        F* toa_up, F* tod_dn_dir, F* tod_dn_dif, F* bg_abs_dir, F* bg_abs_dif, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, void* stream) \
{ F* const bg_out[5] = {toa_up, tod_dn_dir, tod_dn_dif, bg_abs_dir, bg_abs_dif}; \
  return raytracer_sw_entry<F>("rrx_raytracer_sw_bg" #SFX, nx, ny, nz, ngpt, nbnd, top_at_1, independent_column, tau, ssa, band_lims_gpt, \
                               cld_tau, cld_ssa, cld_g, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, \
                               photons_per_pixel, seed, max_events, sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped, stream, \
                               PhaseIn<F>{nmu, nre, re0, dre, mu, phase, cdf, cld_re}, true, bg_out, nbg, dz_bg, bg_tau, bg_ssa, \
                               bg_cld_tau, bg_cld_ssa, bg_cld_g); } \
int rrx_rt_k_null_aer##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, const F* tau, const int* band_lims_gpt, \
        const F* cld_tau, F dz, int knx, int kny, int knz, F* k_null, const F* aer_tau, void* stream) \
{ return k_null_entry<F>("rrx_rt_k_null_aer" #SFX, nx, ny, nz, ngpt, nbnd, igpt, top_at_1, tau, band_lims_gpt, cld_tau, dz, knx, kny, knz, k_null, \
                         stream, aer_tau); } \
int rrx_rt_bg_profile_aer##SFX(int nbg, int ngpt, int nbnd, int igpt, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const int* band_lims_gpt, \
        const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, F* bg_profile, \
        const F* bg_aer_tau, const F* bg_aer_ssa, const F* bg_aer_g, void* stream) \
{ const AerIn<F> bg_aer{bg_aer_tau, bg_aer_ssa, bg_aer_g}; \
  return bg_profile_entry<F>("rrx_rt_bg_profile_aer" #SFX, nbg, ngpt, nbnd, igpt, dz_bg, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, \
                             bg_cld_g, bg_profile, stream, &bg_aer); } \
int rrx_rt_trace_counts_aer##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, F inc_dir, F inc_dif, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long photon0, long long nphotons, int max_events, \
        unsigned long long* sfc_dn_dir, unsigned long long* sfc_dn_dif, unsigned long long* sfc_up, unsigned long long* tod_up, \
        unsigned long long* abs_dir, unsigned long long* abs_dif, unsigned long long* n_capped, \
        unsigned long long* toa_up, unsigned long long* tod_dn_dir, unsigned long long* tod_dn_dif, \
        unsigned long long* bg_abs_dir, unsigned long long* bg_abs_dif, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_profile, const F* aer_tau, const F* aer_ssa, const F* aer_g, void* stream) \
{ const AerIn<F> aer{aer_tau, aer_ssa, aer_g}; \
  return trace_entry<F>("rrx_rt_trace_counts_aer" #SFX, nx, ny, nz, ngpt, nbnd, igpt, top_at_1, independent_column, tau, ssa, band_lims_gpt, \
                        cld_tau, cld_ssa, cld_g, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, k_null, seed, \
                        photon0, nphotons, max_events, sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped, stream, \
                        PhaseIn<F>{nmu, nre, re0, dre, mu, phase, cdf, cld_re}, true, \
                        BgTallies<F>{toa_up, tod_dn_dir, tod_dn_dif, bg_abs_dir, bg_abs_dif}, nbg, dz_bg, bg_profile, &aer); } \
int rrx_raytracer_sw_aer##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, const F* inc_dif, int knx, int kny, int knz, \
        long long photons_per_pixel, unsigned long long seed, int max_events, \
        F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, unsigned long long* n_capped, \
        F* toa_up, F* tod_dn_dir, F* tod_dn_dif, F* bg_abs_dir, F* bg_abs_dif, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, \
        const F* const* aer3, const F* const* bg_aer3, void* stream) \
{ F* const bg_out[5] = {toa_up, tod_dn_dir, tod_dn_dif, bg_abs_dir, bg_abs_dif}; \
  /* each triple is a host array of three device pointers (tau, ssa, g); a NULL array is a triple of NULLs */ \
  const AerIn<F> aer = aer3 != nullptr ? AerIn<F>{aer3[0], aer3[1], aer3[2]} : AerIn<F>{}; \
  const AerIn<F> bg_aer = bg_aer3 != nullptr ? AerIn<F>{bg_aer3[0], bg_aer3[1], bg_aer3[2]} : AerIn<F>{}; \
  return raytracer_sw_entry<F>("rrx_raytracer_sw_aer" #SFX, nx, ny, nz, ngpt, nbnd, top_at_1, independent_column, tau, ssa, band_lims_gpt, \
                               cld_tau, cld_ssa, cld_g, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, \
                               photons_per_pixel, seed, max_events, sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped, stream, \
                               PhaseIn<F>{nmu, nre, re0, dre, mu, phase, cdf, cld_re}, true, bg_out, nbg, dz_bg, bg_tau, bg_ssa, \
                               bg_cld_tau, bg_cld_ssa, bg_cld_g, &aer, &bg_aer); } \
int rrx_rt_k_null_all##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, const F* tau, const int* band_lims_gpt, \
        const F* cld_tau, F dz, int knx, int kny, int knz, F* k_null, const F* aer_tau, void* stream) \
{ return k_null_all_entry<F>("rrx_rt_k_null_all" #SFX, nx, ny, nz, ngpt, nbnd, top_at_1, tau, band_lims_gpt, cld_tau, dz, knx, kny, knz, k_null, \
                             aer_tau, stream); } \
int rrx_rt_bg_profile_all##SFX(int nbg, int ngpt, int nbnd, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const int* band_lims_gpt, \
        const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, F* bg_profile, \
        const F* bg_aer_tau, const F* bg_aer_ssa, const F* bg_aer_g, void* stream) \
{ return bg_profile_all_entry<F>("rrx_rt_bg_profile_all" #SFX, nbg, ngpt, nbnd, dz_bg, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, \
                                 bg_cld_g, bg_profile, AerIn<F>{bg_aer_tau, bg_aer_ssa, bg_aer_g}, stream); } \
int rrx_rt_trace_counts_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const long long* photon_end, const F* weight0, const F* dif_frac, \
        int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long photon0, long long nphotons, int max_events, \
        unsigned long long* sfc_dn_dir, unsigned long long* sfc_dn_dif, unsigned long long* sfc_up, unsigned long long* tod_up, \
        unsigned long long* abs_dir, unsigned long long* abs_dif, unsigned long long* n_capped, \
        unsigned long long* toa_up, unsigned long long* tod_dn_dir, unsigned long long* tod_dn_dif, \
        unsigned long long* bg_abs_dir, unsigned long long* bg_abs_dif, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_profile, const F* aer_tau, const F* aer_ssa, const F* aer_g, void* stream) \
{ return trace_spectral_entry<F>("rrx_rt_trace_counts_spectral" #SFX, nx, ny, nz, ngpt, nbnd, top_at_1, independent_column, tau, ssa, \
                                 band_lims_gpt, cld_tau, cld_ssa, cld_g, dx, dy, dz, sfc_albedo, mu0, azimuth, photon_end, weight0, dif_frac, \
                                 knx, kny, knz, k_null, seed, photon0, nphotons, max_events, sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, \
                                 abs_dif, n_capped, BgTallies<F>{toa_up, tod_dn_dir, tod_dn_dif, bg_abs_dir, bg_abs_dif}, \
                                 PhaseIn<F>{nmu, nre, re0, dre, mu, phase, cdf, cld_re}, nbg, dz_bg, bg_profile, \
                                 AerIn<F>{aer_tau, aer_ssa, aer_g}, stream); } \
int rrx_raytracer_sw_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, const F* inc_dif, int knx, int kny, int knz, \
        const long long* photons_per_pixel_gpt, unsigned long long seed, int max_events, \
        F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, unsigned long long* n_capped, \
        F* toa_up, F* tod_dn_dir, F* tod_dn_dif, F* bg_abs_dir, F* bg_abs_dif, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, \
        const F* const* aer3, const F* const* bg_aer3, void* stream) \
{ F* const bg_out[5] = {toa_up, tod_dn_dir, tod_dn_dif, bg_abs_dir, bg_abs_dif}; \
  const AerIn<F> aer = aer3 != nullptr ? AerIn<F>{aer3[0], aer3[1], aer3[2]} : AerIn<F>{}; \
  const AerIn<F> bg_aer = bg_aer3 != nullptr ? AerIn<F>{bg_aer3[0], bg_aer3[1], bg_aer3[2]} : AerIn<F>{}; \
  return raytracer_sw_spectral_entry<F>("rrx_raytracer_sw_spectral" #SFX, nx, ny, nz, ngpt, nbnd, top_at_1, independent_column, tau, ssa, \
                               band_lims_gpt, cld_tau, cld_ssa, cld_g, dx, dy, dz, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, \
                               photons_per_pixel_gpt, seed, max_events, sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped, stream, \
                               PhaseIn<F>{nmu, nre, re0, dre, mu, phase, cdf, cld_re}, bg_out, nbg, dz_bg, bg_tau, bg_ssa, \
                               bg_cld_tau, bg_cld_ssa, bg_cld_g, aer, bg_aer); }

RRX_DEFINE_RT(double, _f64)
RRX_DEFINE_RT(float, _f32)
}
