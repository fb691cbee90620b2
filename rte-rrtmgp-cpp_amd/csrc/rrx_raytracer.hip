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
// WITH A BACKGROUND (trace_kernel<F,TABLE,true>, the rrx_*_bg entries; rrx_rt_common.h; tests/raytracer_ref.py
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
// WITH AEROSOL (trace_kernel<F,TABLE,true,true>, the rrx_*_aer entries; rrx_rt_common.h; tests/raytracer_ref.py restates
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
#include "rrx_rt_host.h"

namespace
{
using namespace rrx;
using namespace rrx::rt;

// the maximum of k_ext over the cells of block n of the k_null grid, for g-point igpt: ((tau + tau_c) + tau_a)/dz with AER (aer_tau is
// then not NULL), otherwise the two-term (tau + tau_c)/dz, not (tau + tau_c) + 0
template<typename F, bool AER>
__device__ __forceinline__ F k_null_of_block(
        const int n, const int nx, const int ny, const int nz, const int nbnd, const int igpt, const int top_at_1,
        const F* __restrict__ tau, const int* __restrict__ band_lims_gpt, const F* __restrict__ cld_tau, const F* __restrict__ aer_tau,
        const F dz, const int knx, const int kny, const int knz)
{
    const int in = n % knx, jn = (n / knx) % kny, kn = n / (knx*kny);
    const int rx = nx/knx, ry = ny/kny, rz = nz/knz;
    const size_t ncol = size_t(nx)*ny;
    const int ibnd = (cld_tau != nullptr || AER) ? band_of(igpt, nbnd, band_lims_gpt) : -1;
    F m = F(0.);
    for (int k=kn*rz; k<(kn+1)*rz; ++k)
    {
        const int lay = top_at_1 ? nz-1-k : k;
        for (int j=jn*ry; j<(jn+1)*ry; ++j)
            for (int i=in*rx; i<(in+1)*rx; ++i)
            {
                const size_t cell = size_t(i) + size_t(j)*nx + ncol*lay;
                const F tc = (ibnd >= 0 && cld_tau != nullptr) ? cld_tau[cell + ncol*nz*ibnd] : F(0.);
                if constexpr (AER) m = max(m, k_ext_of(tau[cell + ncol*nz*igpt], tc, ibnd >= 0 ? aer_tau[cell + ncol*nz*ibnd] : F(0.), dz));
                else m = max(m, k_ext_of(tau[cell + ncol*nz*igpt], tc, dz));
            }
    }
    return m;
}

// k_null (ng, knz, kny, knx) of the ng g-points from g0 on (one of them: rrx_rt_k_null and the per-g-point loops),
// blockIdx.y counting them. aer_tau: NULL for a medium without aerosol; the test is uniform over the launch.
template<typename F>
__global__ void __launch_bounds__(256) k_null_kernel(
        const int nx, const int ny, const int nz, const int nbnd, const int g0, const int top_at_1,
        const F* __restrict__ tau, const int* __restrict__ band_lims_gpt, const F* __restrict__ cld_tau, const F* __restrict__ aer_tau,
        const F dz, const int knx, const int kny, const int knz, F* __restrict__ k_null)
{
    const int n = blockIdx.x*blockDim.x + threadIdx.x;
    if (n >= knx*kny*knz) return;
    const int igpt = g0 + int(blockIdx.y);
    k_null[size_t(blockIdx.y)*(size_t(knx)*kny*knz) + n] = aer_tau != nullptr
        ? k_null_of_block<F,true>(n, nx, ny, nz, nbnd, igpt, top_at_1, tau, band_lims_gpt, cld_tau, aer_tau, dz, knx, kny, knz)
        : k_null_of_block<F,false>(n, nx, ny, nz, nbnd, igpt, top_at_1, tau, band_lims_gpt, cld_tau, aer_tau, dz, knx, kny, knz);
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

// ---- host side (rrx_rt_host.h)

// the tallies of a trace entry (T = u64) or the fluxes of a loop (T = F); the last five are read only with nbg > 0
template<typename T>
struct FwOut
{
    T* sfc_dn_dir; T* sfc_dn_dif; T* sfc_up; T* tod_up; T* abs_dir; T* abs_dif;
    u64* n_capped;
    T* toa_up; T* tod_dn_dir; T* tod_dn_dif; T* bg_abs_dir; T* bg_abs_dif;
};

// the checks of the forward entries: check_entry with the names of the outputs
template<typename F, typename T, typename A, typename B, typename C>
bool check_forward(const Medium<F>& m, const Sun<F>& sun, const PhaseIn<F>& ph, const Background<F>& bg, const int max_events,
                   Extents extents, Needed inputs, const FwOut<T>& o, A after_nbnd, B after_phase, C after_scene)
{
    return check_entry(m, RT_NEEDED_SOLAR(m), &sun, ph, bg, max_events, extents, inputs,
                       {{"sfc_dn_dir", o.sfc_dn_dir}, {"sfc_dn_dif", o.sfc_dn_dif}, {"sfc_up", o.sfc_up}, {"tod_up", o.tod_up},
                        {"abs_dir", o.abs_dir}, {"abs_dif", o.abs_dif}, {"n_capped", o.n_capped}}, after_nbnd, after_phase, after_scene, nothing);
}

template<typename T>
void check_bg_outputs(const FwOut<T>& o)
{
    check_needed({{"toa_up", o.toa_up}, {"tod_dn_dir", o.tod_dn_dir}, {"tod_dn_dif", o.tod_dn_dif}, {"bg_abs_dir", o.bg_abs_dir},
                  {"bg_abs_dif", o.bg_abs_dif}});
}

// THE BUILDER of the kernel arguments; the sun, dif_frac and the key are the launch's (launch_trace, launch_trace_spectral)
template<typename F>
TraceArgs<F> trace_args(const Medium<F>& m, const int igpt, const F* k_null, const u64 photon0, const long long nphotons, const int max_events,
                        const FwOut<u64>& t)
{
    TraceArgs<F> a{};
    set_medium(a, m, igpt, k_null, max_events);
    a.sfc_albedo = m.sfc_albedo;
    a.independent_column = m.independent_column ? 1 : 0;
    a.photon0 = photon0; a.nphotons = nphotons;
    a.sfc_dn_dir = t.sfc_dn_dir; a.sfc_dn_dif = t.sfc_dn_dif; a.sfc_up = t.sfc_up; a.tod_up = t.tod_up; a.abs_dir = t.abs_dir;
    a.abs_dif = t.abs_dif; a.n_capped = t.n_capped;
    return a;
}

template<typename F> BgTallies<F> bg_tallies(const FwOut<u64>& t) { return {t.toa_up, t.tod_dn_dir, t.tod_dn_dif, t.bg_abs_dir, t.bg_abs_dif}; }

// k_null of the ng g-points from g0 on; aer_tau: NULL for a medium without aerosol
template<typename F>
void launch_k_null(const Medium<F>& m, const int g0, const int ng, const F* aer_tau, F* k_null, hipStream_t st)
{
    const dim3 grid(unsigned(ceil_div(m.knx*m.kny*m.knz, 256)), unsigned(ng));
    k_null_kernel<F><<<grid, 256, 0, st>>>(m.nx, m.ny, m.nz, m.nbnd, g0, m.top_at_1 ? 1 : 0, m.tau, m.band_lims_gpt, m.cld_tau, aer_tau, m.dz,
                                           m.knx, m.kny, m.knz, k_null);
}

// form: which instantiation runs; b is read in the forms with a background (its aerosol triple in FORM_AER, whose profile has
// BG_ROWS_AER rows)
template<typename F>
void launch_trace(TraceArgs<F> a, const PhaseIn<F>& ph, const Sun<F>& sun, const F inc_dir, const F inc_dif, const u64 seed, hipStream_t st,
                  const Form form, const FwBg<F,true,true>& b)
{
    set_sun_and_key(a, sun, seed);
    a.dif_frac = inc_dif / (inc_dir + inc_dif);
    const int blocks = int(std::min<long long>((a.nphotons + RT_BLOCK - 1) / RT_BLOCK, max_blocks()));
    const size_t lds = form == FORM_GRID ? 0 : bg_lds_numbers(b.in.nbg, form == FORM_AER ? BG_ROWS_AER : BG_ROWS)*sizeof(F);
    const FwBg<F,true> bg{b.in, b.t};
    switch (2*form + (ph.given() ? 1 : 0))
    {
        case 2*FORM_AER + 1: trace_kernel<F,true,true,true><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,true>{ph}, b); break;
        case 2*FORM_AER: trace_kernel<F,false,true,true><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,false>{}, b); break;
        case 2*FORM_BG + 1: trace_kernel<F,true,true,false><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,true>{ph}, bg); break;
        case 2*FORM_BG: trace_kernel<F,false,true,false><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,false>{}, bg); break;
        case 2*FORM_GRID + 1: trace_kernel<F,true,false,false><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,true>{ph}, FwBg<F,false>{}); break;
        default: trace_kernel<F,false,false,false><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,false>{}, FwBg<F,false>{});
    }
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

// the profiles (ng, ROWS, nbg+1) of the ng g-points from g0 on, blockIdx.y counting them; ROWS: BG_ROWS_AER with AER, else BG_ROWS
template<typename F, bool AER>
__global__ void bg_profile_kernel(const int nbg, const int nbnd, const int g0, const BgLevels<F> dz_bg,
        const F* __restrict__ bg_tau, const F* __restrict__ bg_ssa, const int* __restrict__ band_lims_gpt,
        const F* __restrict__ bg_cld_tau, const F* __restrict__ bg_cld_ssa, const F* __restrict__ bg_cld_g, const AerIn<F> aer,
        F* __restrict__ profile)
{
    bg_profile_layer<F,AER>(nbg, nbnd, g0 + int(blockIdx.y), dz_bg, bg_tau, bg_ssa, band_lims_gpt, bg_cld_tau, bg_cld_ssa, bg_cld_g, aer,
                            profile + size_t(blockIdx.y)*(AER ? BG_ROWS_AER : BG_ROWS)*(nbg + 1));
}

template<typename F>
BgLevels<F> bg_thicknesses(const int nbg, const F* dz_bg)
{
    BgLevels<F> d{};
    for (int b=0; b<nbg; ++b) d.v[b] = dz_bg[b];
    return d;
}

// The profiles of the ng g-points from g0 on from a background's medium (bg.tau .. bg.cld_g). seven_rows: the BG_ROWS_AER profile with
// the triple aer (NULLs write zeros into its two rows), otherwise the BG_ROWS one. lims: band_lims_gpt.
template<typename F>
void launch_bg_profile(const Background<F>& bg, const int nbnd, const int* lims, const int g0, const int ng, const BgLevels<F>& dz_bg,
                       const bool seven_rows, const AerIn<F>& aer, F* profile, hipStream_t st)
{
    const dim3 grid(unsigned(ceil_div(bg.nbg + 1, 64)), unsigned(ng));
    if (seven_rows)
        bg_profile_kernel<F,true><<<grid, 64, 0, st>>>(bg.nbg, nbnd, g0, dz_bg, bg.tau, bg.ssa, lims, bg.cld_tau, bg.cld_ssa, bg.cld_g, aer, profile);
    else
        bg_profile_kernel<F,false><<<grid, 64, 0, st>>>(bg.nbg, nbnd, g0, dz_bg, bg.tau, bg.ssa, lims, bg.cld_tau, bg.cld_ssa, bg.cld_g, AerIn<F>{},
                                                        profile);
}

// rrx_rt_bg_profile (bg.form = FORM_BG), _aer (FORM_AER: the 7-row profile, its triple may be NULL) and _all (FORM_AER, ALL: the
// profiles of all g-points, igpt is not read)
template<typename F, bool ALL>
int bg_profile_entry(const char* entry, const Background<F>& bg, const int ngpt, const int nbnd, const int* lims, const int igpt, F* profile,
                     void* stream)
{
    RRX_TRY
    check_nbg(bg.nbg);
    if (check_extents({{"nbg", bg.nbg}, {"ngpt", ngpt}})) return 0;
    if (nbnd < 0) throw std::runtime_error("nbnd is negative");
    if constexpr (ALL) check_spectral_ngpt(ngpt); else check_igpt(igpt, ngpt);
    check_bg_medium(bg.nbg, nbnd, bg.dz_bg, bg.tau, bg.ssa, lims, bg.cld_tau, bg.cld_ssa, bg.cld_g);
    if (bg.form == FORM_AER) check_aerosol("bg_aer_", nbnd, lims, bg.aer.tau, bg.aer.ssa, bg.aer.g);
    check_needed({{"bg_profile", profile}});
    bg_levels<F>(bg.nbg, bg.dz_bg, 1, 1, F(1.));          // (the thicknesses are > 0)
    hipStream_t st = static_cast<hipStream_t>(stream);
    launch_bg_profile<F>(bg, nbnd, lims, ALL ? 0 : igpt, ALL ? ngpt : 1, bg_thicknesses(bg.nbg, bg.dz_bg), bg.form == FORM_AER, bg.aer, profile, st);
    RRX_CATCH(entry)
}

template<typename F>
void launch_counts_to_flux(const size_t n, const u64* counts, const F scale, F* out, hipStream_t st)
{
    counts_to_flux_kernel<F><<<unsigned(ceil_div((long long)n, 256)), 256, 0, st>>>(n, counts, scale, out);
}

// rrx_rt_k_null, _aer (m.aer.tau may be NULL) and _all (ALL: every g-point, igpt is not read); of m only what k_null depends on is set
template<typename F, bool ALL>
int k_null_entry(const char* entry, const Medium<F>& m, const int igpt, F* k_null, void* stream)
{
    RRX_TRY
    const F* aer_tau = m.aer.tau;
    if (check_extents({{"nx", m.nx}, {"ny", m.ny}, {"nz", m.nz}, {"ngpt", m.ngpt}})) return 0;
    if (m.nbnd < 0) throw std::runtime_error("nbnd is negative");
    if constexpr (ALL) check_spectral_ngpt(m.ngpt);
    check_needed({{"tau", m.tau}, {"k_null", k_null}});
    if ((m.cld_tau != nullptr || aer_tau != nullptr) && m.band_lims_gpt == nullptr) throw std::runtime_error("band_lims_gpt is NULL");
    if (aer_tau != nullptr && m.nbnd < 1) throw std::runtime_error("nbnd must be >= 1 with an aerosol triple");
    if constexpr (!ALL) check_igpt(igpt, m.ngpt);
    if (!(m.dz > F(0.))) throw std::runtime_error("dz must be > 0");
    check_grid(m.nx, m.ny, m.nz, m.knx, m.kny, m.knz);
    launch_k_null<F>(m, ALL ? 0 : igpt, ALL ? m.ngpt : 1, aer_tau, k_null, static_cast<hipStream_t>(stream));
    RRX_CATCH(entry)
}

// a.photon0 / a.nphotons: the range of the concatenated list; a.k_null: the slices from g-point b.sp.kn_g0 on
template<typename F>
void launch_trace_spectral(TraceArgs<F> a, const PhaseIn<F>& ph, const Sun<F>& sun, const u64 seed, hipStream_t st,
                           const FwBg<F,true,true,true>& b)
{
    set_sun_and_key(a, sun, seed);
    const int blocks = int(std::min<long long>((a.nphotons + RT_BLOCK - 1) / RT_BLOCK, max_blocks()));
    const size_t lds = spectral_lds_bytes(b.sp.ngpt, b.in.nbg, sizeof(F));
    switch (ph.given() ? 1 : 0)
    {
        case 1: trace_kernel<F,true,true,true,true><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,true>{ph}, b); break;
        default: trace_kernel<F,false,true,true,true><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,false>{}, b);
    }
}

// The single-launch trace entries: rrx_rt_trace_counts, _phase (bg.form = FORM_GRID), _bg, _aer, and with SPECTRAL
// rrx_rt_trace_counts_spectral (sp is read; igpt, inc_dir, inc_dif are not). sp.photon_end, weight0, dif_frac are device arrays: the
// entry cannot look into them. The kernel stays inside its arrays whatever photon_end holds (the search is bounded by ngpt and a photon
// beyond photon_end[ngpt] is stepped over); the callers that form the list on the host (rrx_raytracer_sw_spectral, the Python binding)
// refuse a list that does not ascend.
template<typename F, bool SPECTRAL>
int trace_entry(const char* entry, const Medium<F>& m, const Sun<F>& sun, const PhaseIn<F>& ph, const Background<F>& bg, const Run& run,
                const int igpt, const F inc_dir, const F inc_dif, const SpecIn<F>& sp, const F* k_null, const long long photon0,
                const long long nphotons, const FwOut<u64>& t)
{
    RRX_TRY
    const Needed own = {{"k_null", k_null}};
    const Needed own_spectral = {{"photon_end", sp.photon_end}, {"weight0", sp.weight0}, {"dif_frac", sp.dif_frac}, {"k_null", k_null}};
    if (check_forward(m, sun, ph, bg, run.max_events, {{"nphotons", nphotons}}, SPECTRAL ? own_spectral : own, t,
            [&] { if (SPECTRAL) check_spectral_ngpt(m.ngpt); if (photon0 < 0) throw std::runtime_error("photon0 is negative"); },
            [&] { if (!SPECTRAL) check_igpt(igpt, m.ngpt); },
            [&] { if (!SPECTRAL && (inc_dir < F(0.) || inc_dif < F(0.) || !(inc_dir + inc_dif > F(0.))))
                      throw std::runtime_error("inc_dir, inc_dif must be >= 0 with a positive sum"); }))
        return 0;
    const TraceArgs<F> a = trace_args<F>(m, SPECTRAL ? 0 : igpt, k_null, u64(photon0), nphotons, run.max_events, t);
    hipStream_t st = static_cast<hipStream_t>(run.stream);
    FwBg<F,true,true> b{BgIn<F>{}, bg_tallies<F>(t), m.aer};
    if (bg.form != FORM_GRID) b.in = background_of(bg, m, [&] { check_bg_outputs(t); });
    if constexpr (SPECTRAL) launch_trace_spectral<F>(a, ph, sun, run.seed, st, FwBg<F,true,true,true>{b.in, b.t, b.aer, sp});
    else launch_trace<F>(a, ph, sun, inc_dir, inc_dif, run.seed, st, form_of(bg, m), b);
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

// THE WORKSPACE of the forward loops, in u64 words: | the six grid tallies | the five background tallies (nbg > 0) | k_null | the
// background's profile | photon_end, weight0, dif_frac (spectral_ngpt > 0) |
template<typename F>
struct FwWorkspace
{
    size_t ncol, nz, nbg, n_counts;
    u64* counts; F* k_null; F* profile; long long* photon_end; F* weight0; F* dif_frac;
    // nbg: 0 without a background; kn_numbers, profile_numbers: the F of k_null and of the profile
    FwWorkspace(WorkspaceLease& lease, const Medium<F>& m, const int nbg, const size_t kn_numbers, const size_t profile_numbers,
                const int spectral_ngpt)
        : ncol(size_t(m.nx)*m.ny), nz(m.nz), nbg(nbg), n_counts(4*ncol + 2*ncol*nz + (nbg > 0 ? 3*ncol + 2*size_t(nbg) : 0))
    {
        const size_t n_kn = words_of(kn_numbers*sizeof(F)), n_prof = words_of(profile_numbers*sizeof(F));
        const size_t n_pe = spectral_ngpt > 0 ? size_t(spectral_ngpt) + 1 : 0, n_w = words_of(size_t(spectral_ngpt)*sizeof(F));
        counts = lease.get<u64>(n_counts + n_kn + n_prof + n_pe + 2*n_w);
        k_null = reinterpret_cast<F*>(counts + n_counts);
        profile = reinterpret_cast<F*>(counts + n_counts + n_kn);
        photon_end = reinterpret_cast<long long*>(counts + n_counts + n_kn + n_prof);
        weight0 = reinterpret_cast<F*>(counts + n_counts + n_kn + n_prof + n_pe);
        dif_frac = reinterpret_cast<F*>(counts + n_counts + n_kn + n_prof + n_pe + n_w);
    }
    FwOut<u64> tallies(u64* n_capped) const
    {
        u64* c = counts;
        u64* cb = c + 4*ncol + 2*ncol*nz;
        return {c, c + ncol, c + 2*ncol, c + 3*ncol, c + 4*ncol, c + 4*ncol + ncol*nz, n_capped,
                cb, cb + ncol, cb + 2*ncol, cb + 3*ncol, cb + 3*ncol + nbg};
    }
    void zero_counts(hipStream_t st) const
    {
        if (hipMemsetAsync(counts, 0, n_counts*sizeof(u64), st) != hipSuccess) throw std::runtime_error("zeroing the counts failed");
    }
    // THE OUTPUTS start at zero
    void zero_outputs(const FwOut<F>& out, hipStream_t st) const
    {
        bool ok = hipMemsetAsync(out.n_capped, 0, sizeof(u64), st) == hipSuccess;
        if (nbg > 0)
        {
            for (F* o : {out.toa_up, out.tod_dn_dir, out.tod_dn_dif}) ok = ok && hipMemsetAsync(o, 0, ncol*sizeof(F), st) == hipSuccess;
            for (F* o : {out.bg_abs_dir, out.bg_abs_dif}) ok = ok && hipMemsetAsync(o, 0, nbg*sizeof(F), st) == hipSuccess;
        }
        for (F* o : {out.sfc_dn_dir, out.sfc_dn_dif, out.sfc_up, out.tod_up}) ok = ok && hipMemsetAsync(o, 0, ncol*sizeof(F), st) == hipSuccess;
        for (F* o : {out.abs_dir, out.abs_dif}) ok = ok && hipMemsetAsync(o, 0, ncol*nz*sizeof(F), st) == hipSuccess;
        if (!ok) throw std::runtime_error("zeroing the outputs failed");
    }
    // COUNTS TO FLUXES: out += counts 2^-32 scale; abs_* in W m-3 by scale / dz, bg_abs_* [b] in W m-3 of a domain-wide layer: the counts
    // of all columns over the layer's thickness and the number of columns
    void add_fluxes(const F scale, const F dz, const F* dz_bg, const FwOut<F>& out, hipStream_t st) const
    {
        const FwOut<u64> t = tallies(nullptr);
        if (nbg > 0)
        {
            launch_counts_to_flux<F>(ncol, t.toa_up, scale, out.toa_up, st);
            launch_counts_to_flux<F>(ncol, t.tod_dn_dir, scale, out.tod_dn_dir, st);
            launch_counts_to_flux<F>(ncol, t.tod_dn_dif, scale, out.tod_dn_dif, st);
            BgLevels<F> per_layer{};
            for (size_t b=0; b<nbg; ++b) per_layer.v[b] = (scale / dz_bg[b]) / F(ncol);
            bg_counts_to_flux_kernel<F><<<ceil_div(int(nbg), 64), 64, 0, st>>>(int(nbg), t.bg_abs_dir, per_layer, out.bg_abs_dir);
            bg_counts_to_flux_kernel<F><<<ceil_div(int(nbg), 64), 64, 0, st>>>(int(nbg), t.bg_abs_dif, per_layer, out.bg_abs_dif);
        }
        launch_counts_to_flux<F>(ncol, t.sfc_dn_dir, scale, out.sfc_dn_dir, st);
        launch_counts_to_flux<F>(ncol, t.sfc_dn_dif, scale, out.sfc_dn_dif, st);
        launch_counts_to_flux<F>(ncol, t.sfc_up, scale, out.sfc_up, st);
        launch_counts_to_flux<F>(ncol, t.tod_up, scale, out.tod_up, st);
        launch_counts_to_flux<F>(ncol*nz, t.abs_dir, scale / dz, out.abs_dir, st);
        launch_counts_to_flux<F>(ncol*nz, t.abs_dif, scale / dz, out.abs_dif, st);
    }
};

// The loops over the g-points. photons_per_pixel: rrx_raytracer_sw, _phase, _bg, _aer, one k_null, profile and trace launch per
// g-point with incident flux, each g-point's counts converted with its own scale. SPECTRAL (m_gpt, a host array; bg.form = FORM_AER):
// rrx_raytracer_sw_spectral with m_gpt[g] photons per pixel of g-point g: one trace launch per chunk of consecutive g-points, the counts
// of all chunks added in integers and converted once with the common unit U = S/P (rrx_rt_common.h).
template<typename F, bool SPECTRAL>
int raytracer_sw_entry(const char* entry, const Medium<F>& m, const Sun<F>& sun, const PhaseIn<F>& ph, const Background<F>& bg, const Run& run,
                       const F* inc_dir, const F* inc_dif, const long long photons_per_pixel, const long long* m_gpt, const FwOut<F>& out)
{
    RRX_TRY
    constexpr bool spectral = SPECTRAL;
    const size_t ncol = size_t(m.nx)*m.ny;
    // the spectral form's photon list, its weights and the sums of U = S/P
    std::vector<long long> photon_end;
    long long P = 0;
    F S = F(0.);
    const Needed own = {{"inc_dir", inc_dir}, {"inc_dif", inc_dif}};
    const Needed own_spectral = {{"inc_dir", inc_dir}, {"inc_dif", inc_dif}, {"photons_per_pixel_gpt", m_gpt}};
    const Extents work = {{"photons_per_pixel", photons_per_pixel}};
    if (check_forward(m, sun, ph, bg, run.max_events, spectral ? Extents{} : work, spectral ? own_spectral : own, out,
            [&] { if (spectral) check_spectral_ngpt(m.ngpt); }, nothing,
            [&] {
                if (spectral) photon_end.assign(size_t(m.ngpt) + 1, 0);
                for (int g=0; g<m.ngpt; ++g)
                {
                    if (inc_dir[g] < F(0.) || inc_dif[g] < F(0.)) throw std::runtime_error("inc_dir, inc_dif must be >= 0");
                    if (!spectral) continue;
                    if (m_gpt[g] < 0) throw std::runtime_error("photons_per_pixel_gpt is negative at g-point " + std::to_string(g));
                    if (m_gpt[g] > 0 && !(inc_dir[g] + inc_dif[g] > F(0.)))
                        throw std::runtime_error("photons_per_pixel_gpt is > 0 at g-point " + std::to_string(g) + ", which has no incident flux");
                    if (m_gpt[g] > (0x7FFFFFFFFFFFFFFFll - photon_end[g]) / (long long)ncol) throw std::runtime_error("the photon list exceeds 2^63 - 1");
                    photon_end[g+1] = photon_end[g] + m_gpt[g]*(long long)ncol;
                    P += m_gpt[g];
                    if (m_gpt[g] > 0) S = S + (inc_dir[g] + inc_dif[g]);
                }
            }))
        return 0;
    const LoopBg<F> lb = loop_background(bg, m, [&] { check_bg_outputs(out); });
    const BgLevels<F> thick = lb.on ? bg_thicknesses(bg.nbg, bg.dz_bg) : BgLevels<F>{};

    hipStream_t st = static_cast<hipStream_t>(run.stream);
    const size_t nkn = size_t(m.knx)*m.kny*m.knz;
    const int chunk = spectral ? spectral_gpt_per_launch(nkn*sizeof(F), m.ngpt) : 1;
    const size_t profile_numbers = size_t(spectral ? m.ngpt : 1)*(spectral || lb.form == FORM_AER ? BG_ROWS_AER : BG_ROWS)*(lb.nbg + 1);
    WorkspaceLease lease(st);
    const FwWorkspace<F> w(lease, m, lb.nbg, nkn*chunk, lb.on ? profile_numbers : 0, spectral ? m.ngpt : 0);
    const FwOut<u64> t = w.tallies(out.n_capped);
    w.zero_outputs(out, st);
    FwBg<F,true,true> b{BgIn<F>{lb.nbg, w.profile, lb.lev}, bg_tallies<F>(t), m.aer};
    if constexpr (!SPECTRAL)
    {
        const long long nphotons = photons_per_pixel*(long long)ncol;
        for (int g=0; g<m.ngpt; ++g)
        {
            if (!(inc_dir[g] + inc_dif[g] > F(0.))) continue;
            w.zero_counts(st);
            launch_k_null<F>(m, g, 1, m.aer.tau, w.k_null, st);
            const F scale = (inc_dir[g] + inc_dif[g]) / F(photons_per_pixel);
            if (lb.on) launch_bg_profile<F>(bg, m.nbnd, m.band_lims_gpt, g, 1, thick, lb.form == FORM_AER, lb.aer, w.profile, st);
            launch_trace<F>(trace_args<F>(m, g, w.k_null, 0ull, nphotons, run.max_events, t), ph, sun, inc_dir[g], inc_dif[g], run.seed, st,
                            lb.form, b);
            w.add_fluxes(scale, m.dz, bg.dz_bg, out, st);
        }
    }
    else
    {
        if (P == 0) return 0;
        const F U = S / F(P);
        std::vector<F> weight0(m.ngpt, F(0.)), dif_frac(m.ngpt, F(0.));
        for (int g=0; g<m.ngpt; ++g)
            if (m_gpt[g] > 0)
            {
                const F inc = inc_dir[g] + inc_dif[g];
                weight0[g] = (inc / F(m_gpt[g])) / U;
                dif_frac[g] = inc_dif[g] / inc;
            }
        const bool ok = hipMemsetAsync(w.counts, 0, w.n_counts*sizeof(u64), st) == hipSuccess
          && hipMemcpyAsync(w.photon_end, photon_end.data(), photon_end.size()*sizeof(long long), hipMemcpyHostToDevice, st) == hipSuccess
          && hipMemcpyAsync(w.weight0, weight0.data(), size_t(m.ngpt)*sizeof(F), hipMemcpyHostToDevice, st) == hipSuccess
          && hipMemcpyAsync(w.dif_frac, dif_frac.data(), size_t(m.ngpt)*sizeof(F), hipMemcpyHostToDevice, st) == hipSuccess
          && hipStreamSynchronize(st) == hipSuccess;          // (the host arrays end with this call)
        if (!ok) throw std::runtime_error("zeroing the counts or copying the photon list failed");
        if (lb.on) launch_bg_profile<F>(bg, m.nbnd, m.band_lims_gpt, 0, m.ngpt, thick, true, lb.aer, w.profile, st);
        FwBg<F,true,true,true> bs{b.in, b.t, b.aer, SpecIn<F>{m.ngpt, 0, w.photon_end, w.weight0, w.dif_frac}};
        for (int g0=0; g0<m.ngpt; g0+=chunk)
        {
            const int g1 = std::min(g0 + chunk, m.ngpt);
            const long long n = photon_end[g1] - photon_end[g0];
            if (n == 0) continue;
            launch_k_null<F>(m, g0, g1 - g0, m.aer.tau, w.k_null, st);
            bs.sp.kn_g0 = g0;
            launch_trace_spectral<F>(trace_args<F>(m, 0, w.k_null, u64(photon_end[g0]), n, run.max_events, t), ph, sun, run.seed, st, bs);
        }
        w.add_fluxes(U, m.dz, bg.dz_bg, out, st);
    }
    RRX_CATCH(entry)
}
}  // namespace

// ---- the C entries: each builds the structs and calls its family's one function
#define RT_P_HEAD int nx, int ny, int nz, int ngpt, int nbnd
#define RT_P_KNULL(F) RrxBool top_at_1, const F* tau, const int* band_lims_gpt, const F* cld_tau, F dz, int knx, int kny, int knz, F* k_null
#define RT_P_COUNTS \
        unsigned long long* sfc_dn_dir, unsigned long long* sfc_dn_dif, unsigned long long* sfc_up, unsigned long long* tod_up, \
        unsigned long long* abs_dir, unsigned long long* abs_dif, unsigned long long* n_capped
#define RT_P_BG_COUNTS \
        unsigned long long* toa_up, unsigned long long* tod_dn_dir, unsigned long long* tod_dn_dif, \
        unsigned long long* bg_abs_dir, unsigned long long* bg_abs_dif
#define RT_P_TRACE(F) \
        RT_P_GRID(F), F inc_dir, F inc_dif, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long photon0, long long nphotons, int max_events, RT_P_COUNTS
#define RT_P_LOOP(F, PHOTONS) \
        RT_P_HEAD, RrxBool top_at_1, RrxBool independent_column, RT_P_GRID(F), const F* inc_dir, const F* inc_dif, int knx, int kny, int knz, \
        PHOTONS, unsigned long long seed, int max_events, \
        F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, unsigned long long* n_capped
#define RT_P_BG_FLUXES(F) F* toa_up, F* tod_dn_dir, F* tod_dn_dif, F* bg_abs_dir, F* bg_abs_dif
#define RT_KNULL_MEDIUM(F, AER_TAU) \
        Medium<F>{nx, ny, nz, ngpt, nbnd, top_at_1, 0, tau, nullptr, band_lims_gpt, cld_tau, nullptr, nullptr, F(0.), F(0.), dz, nullptr, \
                  knx, kny, knz, AerIn<F>{AER_TAU, nullptr, nullptr}}
#define RT_OUT(T) FwOut<T>{sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped, nullptr, nullptr, nullptr, nullptr, nullptr}
#define RT_OUT_BG(T) FwOut<T>{sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up, abs_dir, abs_dif, n_capped, toa_up, tod_dn_dir, tod_dn_dif, bg_abs_dir, bg_abs_dif}
#define RT_TRACE(F, NAME, AER, PHASE, BG, OUT) \
        trace_entry<F,false>(NAME, RT_MEDIUM(F, independent_column, AER), RT_SUN(F), PHASE, BG, RT_RUN, igpt, inc_dir, inc_dif, SpecIn<F>{}, k_null, \
                       photon0, nphotons, OUT)
#define RT_LOOP(F, NAME, AER, PHASE, BG, OUT) \
        raytracer_sw_entry<F,false>(NAME, RT_MEDIUM(F, independent_column, AER), RT_SUN(F), PHASE, BG, RT_RUN, inc_dir, inc_dif, \
                              photons_per_pixel, nullptr, OUT)

extern "C"
{
#define RRX_DEFINE_RT(F, SFX) \
int rrx_rt_k_null##SFX(RT_P_HEAD, int igpt, RT_P_KNULL(F), void* stream) \
{ return k_null_entry<F,false>("rrx_rt_k_null" #SFX, RT_KNULL_MEDIUM(F, nullptr), igpt, k_null, stream); } \
int rrx_rt_trace_counts##SFX(RT_P_HEAD, int igpt, RrxBool top_at_1, RrxBool independent_column, RT_P_TRACE(F), void* stream) \
{ return RT_TRACE(F, "rrx_rt_trace_counts" #SFX, AerIn<F>{}, PhaseIn<F>{}, RT_NO_BG(F), RT_OUT(u64)); } \
int rrx_rt_counts_to_flux##SFX(long long n, const unsigned long long* counts, F scale, F* out, void* stream) \
{ return counts_to_flux_entry<F>("rrx_rt_counts_to_flux" #SFX, n, counts, scale, out, stream); } \
int rrx_raytracer_sw##SFX(RT_P_LOOP(F, long long photons_per_pixel), void* stream) \
{ return RT_LOOP(F, "rrx_raytracer_sw" #SFX, AerIn<F>{}, PhaseIn<F>{}, RT_NO_BG(F), RT_OUT(F)); } \
int rrx_rt_trace_counts_phase##SFX(RT_P_HEAD, int igpt, RrxBool top_at_1, RrxBool independent_column, RT_P_TRACE(F), RT_P_PHASE(F), void* stream) \
{ return RT_TRACE(F, "rrx_rt_trace_counts_phase" #SFX, AerIn<F>{}, RT_PHASE(F), RT_NO_BG(F), RT_OUT(u64)); } \
int rrx_raytracer_sw_phase##SFX(RT_P_LOOP(F, long long photons_per_pixel), RT_P_PHASE(F), void* stream) \
{ return RT_LOOP(F, "rrx_raytracer_sw_phase" #SFX, AerIn<F>{}, RT_PHASE(F), RT_NO_BG(F), RT_OUT(F)); } \
int rrx_rt_bg_profile##SFX(int nbg, int ngpt, int nbnd, int igpt, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const int* band_lims_gpt, \
        const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, F* bg_profile, void* stream) \
{ return bg_profile_entry<F,false>("rrx_rt_bg_profile" #SFX, RT_BG_MEDIUM(F, FORM_BG, AerIn<F>{}), ngpt, nbnd, band_lims_gpt, igpt, bg_profile, stream); } \
int rrx_rt_trace_counts_bg##SFX(RT_P_HEAD, int igpt, RrxBool top_at_1, RrxBool independent_column, RT_P_TRACE(F), RT_P_BG_COUNTS, RT_P_PHASE(F), \
        int nbg, const F* dz_bg, const F* bg_profile, void* stream) \
{ return RT_TRACE(F, "rrx_rt_trace_counts_bg" #SFX, AerIn<F>{}, RT_PHASE(F), RT_BG_PROFILE(F, FORM_BG), RT_OUT_BG(u64)); } \
int rrx_raytracer_sw_bg##SFX(RT_P_LOOP(F, long long photons_per_pixel), RT_P_BG_FLUXES(F), RT_P_PHASE(F), RT_P_BG(F), void* stream) \
{ return RT_LOOP(F, "rrx_raytracer_sw_bg" #SFX, AerIn<F>{}, RT_PHASE(F), RT_BG_MEDIUM(F, FORM_BG, AerIn<F>{}), RT_OUT_BG(F)); } \
int rrx_rt_k_null_aer##SFX(RT_P_HEAD, int igpt, RT_P_KNULL(F), const F* aer_tau, void* stream) \
{ return k_null_entry<F,false>("rrx_rt_k_null_aer" #SFX, RT_KNULL_MEDIUM(F, aer_tau), igpt, k_null, stream); } \
int rrx_rt_bg_profile_aer##SFX(int nbg, int ngpt, int nbnd, int igpt, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const int* band_lims_gpt, \
        const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, F* bg_profile, \
        const F* bg_aer_tau, const F* bg_aer_ssa, const F* bg_aer_g, void* stream) \
{ const AerIn<F> bg_aer{bg_aer_tau, bg_aer_ssa, bg_aer_g}; \
  return bg_profile_entry<F,false>("rrx_rt_bg_profile_aer" #SFX, RT_BG_MEDIUM(F, FORM_AER, bg_aer), ngpt, nbnd, band_lims_gpt, igpt, bg_profile, stream); } \
int rrx_rt_trace_counts_aer##SFX(RT_P_HEAD, int igpt, RrxBool top_at_1, RrxBool independent_column, RT_P_TRACE(F), RT_P_BG_COUNTS, RT_P_PHASE(F), \
        int nbg, const F* dz_bg, const F* bg_profile, const F* aer_tau, const F* aer_ssa, const F* aer_g, void* stream) \
{ const AerIn<F> aer{aer_tau, aer_ssa, aer_g}; \
  return RT_TRACE(F, "rrx_rt_trace_counts_aer" #SFX, aer, RT_PHASE(F), RT_BG_PROFILE(F, FORM_AER), RT_OUT_BG(u64)); } \
int rrx_raytracer_sw_aer##SFX(RT_P_LOOP(F, long long photons_per_pixel), RT_P_BG_FLUXES(F), RT_P_PHASE(F), RT_P_BG(F), \
        const F* const* aer3, const F* const* bg_aer3, void* stream) \
{ return RT_LOOP(F, "rrx_raytracer_sw_aer" #SFX, aer_of(aer3), RT_PHASE(F), RT_BG_MEDIUM(F, FORM_AER, aer_of(bg_aer3)), RT_OUT_BG(F)); } \
int rrx_rt_k_null_all##SFX(RT_P_HEAD, RT_P_KNULL(F), const F* aer_tau, void* stream) \
{ return k_null_entry<F,true>("rrx_rt_k_null_all" #SFX, RT_KNULL_MEDIUM(F, aer_tau), 0, k_null, stream); } \
int rrx_rt_bg_profile_all##SFX(int nbg, int ngpt, int nbnd, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const int* band_lims_gpt, \
        const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, F* bg_profile, \
        const F* bg_aer_tau, const F* bg_aer_ssa, const F* bg_aer_g, void* stream) \
{ const AerIn<F> bg_aer{bg_aer_tau, bg_aer_ssa, bg_aer_g}; \
  return bg_profile_entry<F,true>("rrx_rt_bg_profile_all" #SFX, RT_BG_MEDIUM(F, FORM_AER, bg_aer), ngpt, nbnd, band_lims_gpt, 0, bg_profile, stream); } \
int rrx_rt_trace_counts_spectral##SFX(RT_P_HEAD, RrxBool top_at_1, RrxBool independent_column, RT_P_GRID(F), \
        const long long* photon_end, const F* weight0, const F* dif_frac, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long photon0, long long nphotons, int max_events, RT_P_COUNTS, RT_P_BG_COUNTS, RT_P_PHASE(F), \
        int nbg, const F* dz_bg, const F* bg_profile, const F* aer_tau, const F* aer_ssa, const F* aer_g, void* stream) \
{ const AerIn<F> aer{aer_tau, aer_ssa, aer_g}; \
  const SpecIn<F> sp{ngpt, 0, photon_end, weight0, dif_frac}; \
  return trace_entry<F,true>("rrx_rt_trace_counts_spectral" #SFX, RT_MEDIUM(F, independent_column, aer), RT_SUN(F), RT_PHASE(F), \
                        RT_BG_PROFILE(F, FORM_AER), RT_RUN, 0, F(0.), F(0.), sp, k_null, photon0, nphotons, RT_OUT_BG(u64)); } \
int rrx_raytracer_sw_spectral##SFX(RT_P_LOOP(F, const long long* photons_per_pixel_gpt), RT_P_BG_FLUXES(F), RT_P_PHASE(F), RT_P_BG(F), \
        const F* const* aer3, const F* const* bg_aer3, void* stream) \
{ return raytracer_sw_entry<F,true>("rrx_raytracer_sw_spectral" #SFX, RT_MEDIUM(F, independent_column, aer_of(aer3)), RT_SUN(F), RT_PHASE(F), \
                               RT_BG_MEDIUM(F, FORM_AER, aer_of(bg_aer3)), RT_RUN, inc_dir, inc_dif, 0, photons_per_pixel_gpt, RT_OUT_BG(F)); }

RRX_DEFINE_RT(double, _f64)
RRX_DEFINE_RT(float, _f32)
}
