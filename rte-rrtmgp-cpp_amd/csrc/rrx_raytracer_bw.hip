// Backward Monte Carlo ray tracer: shortwave radiances for a virtual camera or a flux sensor. The counterpart of
// the reference's ray_tracer_kernel_bw (src_kernels_cuda_rt/raytracer_kernels_bw.cu) on this project's arrays, with the medium, the
// tracking and the scattering of the forward tracer (rrx_raytracer.hip) and one deliberate departure (T_sun below).
//
// THE ESTIMATOR. Rays start at the sensor and travel AGAINST the light, along u, through the medium of the forward tracer: per
// g-point k_ext = (tau + tau_c)/dz, k_sca = (tau ssa + tau_c ssa_c)/dz, k_sca_cld = (tau_c ssa_c)/dz from the clear tau, ssa
// (ncol, nz, ngpt) and the band cloud triple; null-collision tracking on the k_null grid with integer block indices (in, jn, kn);
// f_no_abs = 1 - (k_ext - k_sca)/k_null; Russian roulette below weight 0.5; a Lambertian surface; periodic x / y; the same
// scatter-or-null and species decisions and the same Rayleigh / Henyey-Greenstein sampling. No absorption tallies, no
// independent-column switch. A ray is scored by LOCAL ESTIMATES OF THE DIRECT SOLAR BEAM, which travels along
// s = (sin cos(azimuth), sin sin(azimuth), -mu0). A deposit d is made
//   - at a surface hit: first weight *= albedo[pixel], then d = weight mu0/pi T_sun, before the roulette draw;
//   - at a collision that scatters (after weight *= f_no_abs, the roulette, the scatter-or-null draw and the species draw, before
//     the new direction is drawn): d = weight P(cos)/(4 pi) T_sun, cos = -(u.s) clamped to [-1, 1], Rayleigh P = 3/4 (1 + cos^2),
//     cloud P = (1 - g^2)/(q sqrt(q)), q = 1 + g^2 - 2 g cos, g = min(g_c, 1 - eps): only + - x / and sqrt.
// T_sun = exp(-tau_sun), tau_sun the EXACT optical path from the event's position to the domain top along -s, cell by cell through
// the fine grid: the walk carries integer cell indices (i, j, k), wrapping in x / y by index, and the three distances to the next
// face along each axis (a first distance that rounding made negative is 0), and steps one index at a time until k = nz. It draws
// no random numbers and takes at most nz + ceil(H tan/dx) + ceil(H tan/dy) + 2 steps (H = nz dz, tan of the solar zenith angle);
// a walk that exceeds this count (only a NaN among the inputs can do it) drops the ray into n_capped. The reference estimates this
// transmission stochastically; here the shadow term has no variance. The sun's disk is not imaged, there is no diffuse incident
// light.
//
// TALLY. One unsigned 64-bit count per camera pixel in units of 2^-32: llrint(min(d, 2^20) 2^32), added with an integer atomic; a
// clamped deposit is counted in n_clamped; a ray alive after max_events events (collisions + crossings) is dropped and counted in
// n_capped. Radiance of a g-point = counts 2^-32 / rays_per_pixel inc_dir/mu0 (W m-2 sr-1). Bit-reproducible, independent of the
// order of arrival, additive over ray ranges.
//
// RANDOM NUMBERS. Philox4x32-10, key = seed, counter (ray low, ray high, igpt | 0x80000000, block). Ray r belongs to camera pixel
// pix = r mod npix, ipx = pix mod npx, ipy = pix / npx. DRAW ORDER (tests/raytracer_bw_ref.py restates it):
//   start:     u -> a = (ipx + u)/npx;  u -> b = (ipy + u)/npy;  sensor type 3 only: u -> mu = sqrt(u);  u -> phi = 2 pi u
//   each event: u -> tau = -log(u), unless the previous event was a crossing between blocks
//     surface:   weight *= albedo; deposit; weight < 0.5: u -> survives (weight = 1) iff u <= weight; survivor: u -> mu; u -> phi
//     collision: weight *= f_no_abs; weight < 0.5: u -> roulette; survivor: u -> scatter or null; scatter: u -> species; deposit;
//                u -> cos of the scattering angle; u -> phi
//
// SENSORS (12 host numbers: position, e_w, e_h, e_d; Lx = nx dx, Ly = ny dy, z_top = nz dz):
//   0 perspective    direction normalize(e_w (2a-1) + e_h (2b-1) + e_d), from position
//   1 fisheye        theta = a fov/2, phi = 2 pi b; direction normalize(e_d cos(theta) + sin(theta) (e_w cos(phi) + e_h sin(phi)))
//   2 orthographic   direction e_d (unit, e_d.z < 0), from (a Lx, b Ly, z_top)
//   3 flux sensor    cosine-weighted about +z from (a Lx, b Ly, 0) when e_d.z > 0, about -z from (a Lx, b Ly, z_top) when
//                    e_d.z < 0: pi x the mean radiance is an irradiance
// A start at or above the top with a downward direction is moved along the ray to the top; one that does not point downward ends
// at once. x, y are wrapped into the domain and the block found by integer division and clamping.
//
// SHAPE. One ray per lane, lanes refill from a round-robin list inside the event loop, the grid is capped as in trace_kernel. The
// sun walk is a STATE of that one loop, which has one back edge: in a pass a lane either traces one event or walks one cell to the
// sun, so that one lane's long walk does not idle the other 63 behind an inner loop (measured both ways: DESIGN 4.15).
//
// TABLE (trace_bw_kernel<F,true>; rrx_rt_phase.h): the cloud species scatters by the tabulated phase function of the
// cell's radius: phase_eval towards the sun in the deposit, phase_sample for the new direction, the same draws in the same order.
// The walk carries the radius where the Henyey-Greenstein form carries g_c; the nodes are staged in LDS once per workgroup.
#include "rrx_rt_phase.h"
#include "rrx_rt_host.h"

namespace
{
using namespace rrx;
using namespace rrx::rt;

template<typename F>
struct BwArgs
{
    int nx, ny, nz, nbnd, igpt, top_at_1;
    const F* tau; const F* ssa; const int* band_lims_gpt; const F* cld_tau; const F* cld_ssa; const F* cld_g;
    F dx, dy, dz;
    const F* sfc_albedo;
    F mu0, sun_x, sun_y, sun_z;
    int knx, kny, knz;
    const F* k_null;
    unsigned k0, k1;
    u64 ray0; long long nrays; int max_events, max_walk;
    int type, npx, npy;
    F fov, px, py, pz, wx, wy, wz, hx, hy, hz, ex, ey, ez;
    u64* counts; u64* n_capped; u64* n_clamped;
};

// the state of a walk to the sun: cell indices, the distances along -s to the next face of each axis, the distance covered, the
// optical path so far, the deposit's factor in front of T_sun, and what follows the deposit (0: the surface's roulette, 1: a
// Rayleigh scattering, 2: a cloud scattering with asymmetry gc; with a phase table gc holds the cell's radius, 3: an aerosol
// scattering, Henyey-Greenstein with gc = g_a whether there is a table or not)
template<typename F>
struct Walk
{
    int i, j, k, steps, then;
    F tx, ty, tz, t, tau, dep, gc;
};

template<typename F>
__device__ __forceinline__ void begin_walk(Walk<F>& w, const BwArgs<F>& a, const F vx, const F vy, const F vz,
                                           const F x, const F y, const F z, const int i, const int j, const int k,
                                           const F dep, const int then, const F gc)
{
    const F inf = F(INFINITY);
    w.i = i; w.j = j; w.k = k; w.steps = 0; w.then = then; w.t = F(0.); w.tau = F(0.); w.dep = dep; w.gc = gc;
    w.tx = vx > F(0.) ? max(F(0.), (F(i+1)*a.dx - x)/vx) : (vx < F(0.) ? max(F(0.), (F(i)*a.dx - x)/vx) : inf);
    w.ty = vy > F(0.) ? max(F(0.), (F(j+1)*a.dy - y)/vy) : (vy < F(0.) ? max(F(0.), (F(j)*a.dy - y)/vy) : inf);
    w.tz = max(F(0.), (F(k+1)*a.dz - z)/vz);
}

// what follows the deposit of a surface hit: the roulette and the reflected direction; false: the ray ends
template<typename F>
__device__ __forceinline__ bool after_surface(Stream& rng, F& weight, F& ux, F& uy, F& uz)
{
    if (weight < F(0.5)) weight = (rng.next<F>() > weight) ? F(0.) : F(1.);
    if (!(weight > F(0.))) return false;
    lambert(rng, F(1.), ux, uy, uz);
    return true;
}

// DRAW ORDER WITH A BACKGROUND (tests/raytracer_bw_ref.py restates it): that of the header. start: the same draws. each event in layer b: u -> tau = -log(u) unless the
// previous event was a crossing (between layers, between blocks or through the domain top in either direction); a crossing draws
// nothing; collision: weight *= f_no_abs; weight < 0.5: u -> roulette; survivor: u -> scatter or null (it always scatters);
// u -> species; deposit (no walk); u -> cos of the scattering angle; u -> phi.
//
// BG (trace_bw_kernel<F,TABLE,true>; rrx_rt_common.h): the background atmosphere above the grid. A ray that leaves the
// grid upward goes on through the layers and ends only at TOA; one that comes down through the domain top enters the grid by
// enter_grid. The top of the medium is TOA: a start at or above it is moved along the ray to it. The orthographic sensor and the
// flux sensor facing down start at the height clamp(position.z, domain top, TOA): position.z = 0 is the domain top as without a
// background, any position.z >= TOA is TOA. A start above the domain top lies in layer bg_layer_of(z) with x, y as they are.
// A scattering in layer b at height z deposits as a grid scattering does, with T_sun = exp(-(k_ext_b (z[b+1] - z) + tau_above[b])/mu0)
// and no walk: it is made inside the event, Henyey-Greenstein for the cloud species. A deposit from inside the grid ends its walk
// with exp(-(tau_walk + tau_above[nbg]/mu0)): one exp of the summed path. The draw order is that of the header. nbg = 0: the
// integers of the other instantiations.
//
// AER (trace_bw_kernel<F,TABLE,true,true>, the rrx_*_aer entries; rrx_rt_common.h; tests/raytracer_bw_ref.py restates it):
// aerosol as a third species, built on top of the BG form only, which handles nbg = 0. k_ext and k_sca take tau_a as rrx_rt_common.h
// writes them, the walk to the sun sums that k_ext and tau_above holds the aerosol's share. The draw count and DRAW ORDER are
// unchanged: the species uniform u picks cloud iff u k_sca < k_sca_cld, otherwise aerosol iff u k_sca < k_sca_cld + k_sca_aer,
// otherwise gas. An aerosol scattering deposits with the Henyey-Greenstein density of g = min(g_a, 1 - eps) and draws its new
// direction from it, in the grid (after the walk: then = 3) and aloft, with a phase table too. DEPARTURE: the reference draws
// aerosol, cloud, gas in that order; cloud comes first here so that a scene without aerosol draws exactly what it draws without
// this form.
//
// SPECTRAL (trace_bw_kernel<F,TABLE,true,true,true>, the rrx_camera_* entries; rrx_rt_common.h): the rays of all g-points in
// one launch, built on the aerosol form only. a.ray0 / a.nrays address the concatenated list whose prefix sums are sp.photon_end (here:
// ray_end); the g-point is state of the ray, set when a lane takes its next one. The band, the tau / ssa / cloud / aerosol slices, the
// k_null slice, the background's profile rows and the band's phase table are derived from it at the event and at every cell of the
// walk: the lane carries no pointers. The transport is that of ray q of g-point g in the per-g-point launch, draw for draw; a deposit
// is min(d weight0[g], 2^20), tallied into counts[band(g) npix + pix]; a.igpt is not read. A g-point that lies in no band has no
// row of counts: its deposits are dropped.
template<typename F> struct BwSpecArgs { BgIn<F> in; AerIn<F> aer; SpecIn<F> sp; };
template<typename F, bool BG, bool AER, bool SPECTRAL>
using BwBgArgs = std::conditional_t<SPECTRAL, BwSpecArgs<F>, BgArgs<F,BG,AER>>;

// LDS of the spectral form: what stage_spectral lays out (ray_end, the levels, the band table: spectral_lds_bytes), rounded up to 8
// bytes, then the phase nodes
__host__ __device__ inline size_t bw_nodes_offset(const int ngpt, const int nbg, const size_t size_of_f)
{
    return (size_t(ngpt + 1)*sizeof(long long) + size_t(nbg + 1)*size_of_f + size_t(ngpt)*sizeof(int) + 7)/8*8;
}
inline size_t bw_spectral_lds_bytes(const int ngpt, const int nbg, const int nmu, const size_t size_of_f)
{
    return bw_nodes_offset(ngpt, nbg, size_of_f) + size_t(nmu)*size_of_f;
}

template<typename F, bool TABLE, bool BG, bool AER, bool SPECTRAL = false>
__global__ void __launch_bounds__(RT_BLOCK) trace_bw_kernel(const BwArgs<F> a, const PhaseArgs<F,TABLE> ph, const BwBgArgs<F,BG,AER,SPECTRAL> bgin)
{
    static_assert(BG || !AER, "the aerosol form is built on the background form");
    static_assert(AER || !SPECTRAL, "the spectral form is built on the aerosol form");
    const long long nthreads = (long long)gridDim.x*blockDim.x;
    long long next_ray = (long long)blockIdx.x*blockDim.x + threadIdx.x;

    // the nodes, searched by every cloud scattering and shared by all lanes: nmu numbers of dynamic LDS (nmu <= 4096 on the host);
    // behind them the background's profile and levels
    [[maybe_unused]] const F* mu_s = nullptr;
    [[maybe_unused]] PhaseTable<F> tab{};
    [[maybe_unused]] BgView<F> bg{};
    [[maybe_unused]] SpecView sv{};
    if constexpr (SPECTRAL)
    {
        extern __shared__ double phase_lds[];
        if constexpr (TABLE)
        {
            F* nodes = reinterpret_cast<F*>(reinterpret_cast<char*>(phase_lds) + bw_nodes_offset(bgin.sp.ngpt, bgin.in.nbg, sizeof(F)));
            for (int n=threadIdx.x; n<ph.in.nmu; n+=blockDim.x) nodes[n] = ph.in.mu[n];
            mu_s = nodes;
        }
        sv = stage_spectral<F>(bgin.sp, bgin.in, a.nbnd, a.band_lims_gpt, phase_lds, bg);          // (it ends with the barrier)
    }
    else if constexpr (TABLE || BG)
    {
        extern __shared__ double phase_lds[];
        F* stage = reinterpret_cast<F*>(phase_lds);
        if constexpr (TABLE)
        {
            for (int n=threadIdx.x; n<ph.in.nmu; n+=blockDim.x) stage[n] = ph.in.mu[n];
            if constexpr (!BG) __syncthreads();
            mu_s = stage;
            stage += ph.in.nmu;
        }
        if constexpr (BG) bg = stage_background<F, AER ? BG_ROWS_AER : BG_ROWS>(bgin.in, stage);
    }

    const int nx = a.nx, ny = a.ny, nz = a.nz;
    const size_t ncol = size_t(nx)*ny;
    const int rx = nx/a.knx, ry = ny/a.kny, rz = nz/a.knz;
    const F kdx = F(rx)*a.dx, kdy = F(ry)*a.dy, kdz = F(rz)*a.dz;
    const F len_x = F(a.knx)*kdx, len_y = F(a.kny)*kdy, z_top = F(a.knz)*kdz;
    const int npix = a.npx*a.npy;
    // (what follows of the g-point is fixed for the launch, or under SPECTRAL derived from the lane's igpt by of_gpt below)
    [[maybe_unused]] int igpt = SPECTRAL ? 0 : a.igpt;
    int ibnd = -1;
    const F* __restrict__ tau_g = a.tau;
    const F* __restrict__ ssa_g = a.ssa;
    const F* __restrict__ ctau_b = nullptr;
    [[maybe_unused]] const F* __restrict__ kn_g = a.k_null;
    [[maybe_unused]] int ibnd_a = -1;
    [[maybe_unused]] const F* __restrict__ atau_b = nullptr;
    if constexpr (!SPECTRAL)
    {
        ibnd = a.cld_tau != nullptr ? band_of(a.igpt, a.nbnd, a.band_lims_gpt) : -1;
        tau_g = a.tau + ncol*nz*a.igpt;
        ssa_g = a.ssa + ncol*nz*a.igpt;
        ctau_b = ibnd >= 0 ? a.cld_tau + ncol*nz*ibnd : nullptr;
        if constexpr (TABLE) tab = table_of_band(ph.in, ibnd);
        if constexpr (AER)
        {
            ibnd_a = bgin.aer.tau != nullptr ? band_of(a.igpt, a.nbnd, a.band_lims_gpt) : -1;
            atau_b = ibnd_a >= 0 ? bgin.aer.tau + ncol*nz*ibnd_a : nullptr;
        }
    }
    const F inf = F(INFINITY);
    [[maybe_unused]] const F g_max = F(1.) - Lim<F>::eps();
    const F pi = F(3.141592653589793);
    // towards the sun, and the distance along it across one cell of each axis
    const F vx = -a.sun_x, vy = -a.sun_y, vz = -a.sun_z;
    const F dtx = vx != F(0.) ? a.dx/fabs(vx) : inf, dty = vy != F(0.) ? a.dy/fabs(vy) : inf, dtz = a.dz/vz;
    // the top of the medium, and the slant optical path of the whole background
    [[maybe_unused]] F z_toa = z_top, tau_bg_sun = F(0.);
    if constexpr (SPECTRAL) { if (bg.nbg > 0) z_toa = bg.z[bg.nbg]; }          // (tau_bg_sun is the g-point's: formed where its walk ends)
    else if constexpr (BG) { if (bg.nbg > 0) { z_toa = bg.z[bg.nbg]; tau_bg_sun = bg.tau_above[bg.nbg]/a.mu0; } }
    // SPECTRAL: what a pass reads of the lane's g-point, derived again in every pass
    [[maybe_unused]] const auto of_gpt = [&]() {
        if constexpr (SPECTRAL)
        {
            const int band = sv.band[igpt];
            ibnd = a.cld_tau != nullptr ? band : -1;
            ibnd_a = bgin.aer.tau != nullptr ? band : -1;
            tau_g = a.tau + ncol*nz*igpt;
            ssa_g = a.ssa + ncol*nz*igpt;
            ctau_b = ibnd >= 0 ? a.cld_tau + ncol*nz*ibnd : nullptr;
            atau_b = ibnd_a >= 0 ? bgin.aer.tau + ncol*nz*ibnd_a : nullptr;
            kn_g = a.k_null + (size_t(a.knx)*a.kny*a.knz)*size_t(igpt - bgin.sp.kn_g0);
            if constexpr (TABLE) tab = table_of_band(ph.in, ibnd);
            // (unconditional, like every line here: a value kept from the pass before would be carried around the loop, which cost 30 - 38
            // VGPRs; with nbg = 0 the rows are not read)
            bg_rows_of_gpt<F, BG_ROWS_AER>(bg, bgin.in.profile, igpt);
        }
    };
    // a deposit d of the lane's ray: clamped at 2^20 (after the g-point's weight under SPECTRAL) and tallied into its pixel
    const auto deposit = [&](F d, const int pix) {
        size_t slot = size_t(pix);
        if constexpr (SPECTRAL)
        {
            const int band = sv.band[igpt];
            if (band < 0) return;
            d = d*bgin.sp.weight0[igpt];
            slot += size_t(band)*size_t(npix);
        }
        const bool clamped = d > F(1048576.);
        if (clamped) atomicAdd(a.n_clamped, 1ull);
        tally(a.counts, slot, to_count(clamped ? F(1048576.) : d));
    };

    Stream rng; rng.k0 = a.k0; rng.k1 = a.k1; rng.used = 4; rng.block = 0u; rng.c0 = rng.c1 = rng.c2 = 0u;
    bool alive = false, pending = false, walking = false;
    int in = 0, jn = 0, kn = 0, nev = 0, pix = 0;
    F x = F(0.), y = F(0.), z = F(0.), ux = F(0.), uy = F(0.), uz = F(-1.), weight = F(0.), tau = F(0.);
    Walk<F> w; w.i = w.j = w.k = w.steps = w.then = 0; w.tx = w.ty = w.tz = w.t = w.tau = w.dep = w.gc = F(0.);

    // One loop with ONE back edge: in a pass a lane either walks one cell towards the sun or traces one event. The form matters:
    // with the walk first and `continue` after it the compiler makes the walk an inner loop of the wave (the same instructions as a
    // `do while` around it) and the tracking lanes wait for the longest walk; profiles/raytracer_bw_bench.txt has the times.
    bool done = false;
    for (;;)
    {
        if (walking)
        {
            // ---- one cell of the walk to the sun
            of_gpt();
            const F tn = min(w.tz, min(w.tx, w.ty));
            const int axis = (w.tz <= w.tx && w.tz <= w.ty) ? 2 : (w.tx <= w.ty ? 0 : 1);
            const int lay = a.top_at_1 ? nz-1-w.k : w.k;
            const size_t cell = size_t(w.i) + size_t(w.j)*nx + ncol*lay;
            const F tc = ibnd >= 0 ? ctau_b[cell] : F(0.);
            if constexpr (AER) w.tau = w.tau + k_ext_of(tau_g[cell], tc, ibnd_a >= 0 ? atau_b[cell] : F(0.), a.dz)*(tn - w.t);
            else w.tau = w.tau + k_ext_of(tau_g[cell], tc, a.dz)*(tn - w.t);
            w.t = tn;
            if (axis == 0)
            {
                w.i = vx > F(0.) ? (w.i + 1 == nx ? 0 : w.i + 1) : (w.i == 0 ? nx - 1 : w.i - 1);
                w.tx = w.tx + dtx;
            }
            else if (axis == 1)
            {
                w.j = vy > F(0.) ? (w.j + 1 == ny ? 0 : w.j + 1) : (w.j == 0 ? ny - 1 : w.j - 1);
                w.ty = w.ty + dty;
            }
            else { ++w.k; w.tz = w.tz + dtz; }
            ++w.steps;
            if (w.k == nz)
            {
                if constexpr (SPECTRAL) tau_bg_sun = bg.nbg > 0 ? bg.tau_above[bg.nbg]/a.mu0 : F(0.);
                F d;
                if constexpr (BG) d = w.dep*exp(-(w.tau + tau_bg_sun));
                else d = w.dep*exp(-w.tau);
                deposit(d, pix);
                walking = false;
                if (w.then == 0) { alive = after_surface(rng, weight, ux, uy, uz); pending = false; }
                else if (AER && w.then == 3) scatter_direction(rng, true, w.gc, g_max, ux, uy, uz);
                else if constexpr (TABLE) scatter_direction_table(rng, w.then == 2, tab, mu_s, w.gc, ux, uy, uz);
                else scatter_direction(rng, w.then == 2, w.gc, g_max, ux, uy, uz);
            }
            else if (w.steps >= a.max_walk) { atomicAdd(a.n_capped, 1ull); walking = false; alive = false; }
        }
        else
        {
            // one event of a tracking lane: a block that the lane leaves with `break` when the event is over (or, with done, when its
            // list has run out)
            do
            {
                if (!alive)
                {
                    if (next_ray >= a.nrays) { done = true; break; }          // the list is finite, every ray ends within max_events events and every walk is bounded
                    u64 r = a.ray0 + u64(next_ray);
                    next_ray += nthreads;
                    if constexpr (SPECTRAL)
                    {
                        igpt = gpt_of_photon(sv.photon_end, sv.ngpt, (long long)r);
                        if (igpt >= sv.ngpt) { igpt = 0; break; }          // (beyond the list)
                        r = r - u64(sv.photon_end[igpt]);
                    }
                    rng.start(r, unsigned(igpt) | 0x80000000u);
                    pix = int(r % u64(npix));
                    const int ipx = pix % a.npx, ipy = pix / a.npx;
                    const F fa = (F(ipx) + rng.next<F>()) / F(a.npx);
                    const F fb = (F(ipy) + rng.next<F>()) / F(a.npy);
                    F sx = a.px, sy = a.py, sz = a.pz;
                    if (a.type == 0 || a.type == 1)
                    {
                        F qx, qy, qz;
                        if (a.type == 0)
                        {
                            const F ca = F(2.)*fa - F(1.), cb = F(2.)*fb - F(1.);
                            qx = (a.wx*ca + a.hx*cb) + a.ex; qy = (a.wy*ca + a.hy*cb) + a.ey; qz = (a.wz*ca + a.hz*cb) + a.ez;
                        }
                        else
                        {
                            const F th = (fa*a.fov)*F(0.5), ph = F(6.283185307179586)*fb;
                            const F ct = cos(th), st = sin(th), cp = cos(ph), sp = sin(ph);
                            qx = a.ex*ct + st*(a.wx*cp + a.hx*sp); qy = a.ey*ct + st*(a.wy*cp + a.hy*sp); qz = a.ez*ct + st*(a.wz*cp + a.hz*sp);
                        }
                        const F nrm = sqrt((qx*qx + qy*qy) + qz*qz);
                        ux = qx/nrm; uy = qy/nrm; uz = qz/nrm;
                    }
                    else
                    {
                        sx = fa*len_x; sy = fb*len_y;
                        if constexpr (BG)
                        {
                            if (a.type == 2) { ux = a.ex; uy = a.ey; uz = a.ez; sz = clampf(a.pz, z_top, z_toa); }
                            else if (a.ez > F(0.)) { lambert(rng, F(1.), ux, uy, uz); sz = F(0.); }
                            else { lambert(rng, F(-1.), ux, uy, uz); sz = clampf(a.pz, z_top, z_toa); }
                        }
                        else if (a.type == 2) { ux = a.ex; uy = a.ey; uz = a.ez; sz = z_top; }
                        else if (a.ez > F(0.)) { lambert(rng, F(1.), ux, uy, uz); sz = F(0.); }
                        else { lambert(rng, F(-1.), ux, uy, uz); sz = z_top; }
                    }
                    if (sz >= z_toa)
                    {
                        if (!(uz < F(0.))) break;          // it looks away from the medium: the ray ends with nothing
                        if (sz > z_toa) { const F t = (z_toa - sz)/uz; sx = sx + ux*t; sy = sy + uy*t; }
                        sz = z_toa;
                    }
                    [[maybe_unused]] bool starts_in_bg = false;
                    if constexpr (BG) starts_in_bg = sz > z_top;
                    if (starts_in_bg)
                    {
                        if constexpr (BG)
                        {
                            const int b = bg_layer_of(bg, sz);
                            in = 0; jn = 0; kn = a.knz + b;
                            x = sx; y = sy; z = clampf(sz, bg.z[b], bg.z[b+1]);
                        }
                    }
                    else
                    {
                        sx = sx - floor(sx/len_x)*len_x; sy = sy - floor(sy/len_y)*len_y;
                        in = clampi(int(sx/kdx), 0, a.knx - 1); jn = clampi(int(sy/kdy), 0, a.kny - 1); kn = clampi(int(sz/kdz), 0, a.knz - 1);
                        x = clampf(sx, F(in)*kdx, F(in+1)*kdx); y = clampf(sy, F(jn)*kdy, F(jn+1)*kdy); z = clampf(sz, F(kn)*kdz, F(kn+1)*kdz);
                    }
                    weight = F(1.); pending = false; nev = 0; alive = true;
                }
                if (nev >= a.max_events) { atomicAdd(a.n_capped, 1ull); alive = false; break; }
                ++nev;
                of_gpt();

                // in_bg: the ray is in background layer kn - knz, a block with z faces only whose k_null is its own k_ext
                [[maybe_unused]] bool in_bg = false;
                if constexpr (BG) in_bg = kn >= a.knz;
                const F x_lo = F(in)*kdx, x_hi = F(in+1)*kdx, y_lo = F(jn)*kdy, y_hi = F(jn+1)*kdy;
                F z_lo = F(kn)*kdz, z_hi = F(kn+1)*kdz;
                if constexpr (BG) { if (in_bg) { z_lo = bg.z[kn - a.knz]; z_hi = bg.z[kn - a.knz + 1]; } }
                const F sz = uz > F(0.) ? (z_hi - z)/uz : (uz < F(0.) ? (z_lo - z)/uz : inf);
                const F sx = in_bg ? inf : (ux > F(0.) ? (x_hi - x)/ux : (ux < F(0.) ? (x_lo - x)/ux : inf));
                const F sy = in_bg ? inf : (uy > F(0.) ? (y_hi - y)/uy : (uy < F(0.) ? (y_lo - y)/uy : inf));
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
                    // ---- the ray leaves the block through the face of `axis`
                    if (!(d_max < inf)) { atomicAdd(a.n_capped, 1ull); alive = false; break; }
                    tau = tau - tau_cell; pending = true;
                    if (in_bg) { x = x + ux*d_max; y = y + uy*d_max; }
                    else { x = clampf(x + ux*d_max, x_lo, x_hi); y = clampf(y + uy*d_max, y_lo, y_hi); }
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
                                if (kn == a.knz + bg.nbg - 1) alive = false;
                                else { ++kn; z = bg.z[kn - a.knz]; }
                            }
                            else if (kn == a.knz)
                            {
                                enter_grid(x, in, len_x, kdx, a.knx); enter_grid(y, jn, len_y, kdy, a.kny);
                                kn = a.knz - 1; z = z_top;
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
                            alive = false;
                            if constexpr (BG) { if (bg.nbg > 0) { alive = true; kn = a.knz; z = bg.z[0]; } }
                        }
                        else { ++kn; z = F(kn)*kdz; }
                    }
                    else if (kn == 0)                 // the surface
                    {
                        z = F(0.);
                        const int i = fine_cell(x, a.dx, in, rx), j = fine_cell(y, a.dy, jn, ry);
                        weight = weight * a.sfc_albedo[i + nx*j];
                        const F dep = (weight*a.mu0)/pi;
                        if (dep > F(0.)) { begin_walk(w, a, vx, vy, vz, x, y, z, i, j, 0, dep, 0, F(0.)); walking = true; }
                        else { alive = after_surface(rng, weight, ux, uy, uz); pending = false; }
                    }
                    else { --kn; z = F(kn+1)*kdz; }
                }
                else
                {
                    // ---- a collision inside the block
                    const F dn = tau / kn_val;
                    if (in_bg) { x = x + ux*dn; y = y + uy*dn; }
                    else { x = clampf(x + ux*dn, x_lo, x_hi); y = clampf(y + uy*dn, y_lo, y_hi); }
                    z = clampf(z + uz*dn, z_lo, z_hi);
                    // the cell and its k_ext, k_sca, k_sca_cld: a cell of the grid, or the ray's background layer
                    int i = 0, j = 0, k = 0;
                    size_t cell = 0;
                    F k_ext = F(0.), k_sca = F(0.), k_sca_cld = F(0.), gc = F(0.);
                    [[maybe_unused]] F k_sca_aer = F(0.), ga = F(0.);
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
                        }
                    }
                    else
                    {
                        i = fine_cell(x, a.dx, in, rx); j = fine_cell(y, a.dy, jn, ry); k = fine_cell(z, a.dz, kn, rz);
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
                    weight = weight * f_no_abs;
                    if (weight < F(0.5)) weight = (rng.next<F>() > weight) ? F(0.) : F(1.);
                    if (!(weight > F(0.))) { alive = false; break; }
                    if (rng.next<F>()*(k_sca + (kn_val - k_ext)) < k_sca)
                    {
                        const F us = rng.next<F>()*k_sca;
                        const bool cloud = us < k_sca_cld;
                        [[maybe_unused]] bool aerosol = false;
                        if constexpr (AER) aerosol = !cloud && us < k_sca_cld + k_sca_aer;
                        const F cs = clampf(-((ux*a.sun_x + uy*a.sun_y) + uz*a.sun_z), F(-1.), F(1.));
                        F phase;
                        [[maybe_unused]] bool bg_done = false;
                        if constexpr (BG)
                        {
                            if (in_bg)
                            {
                                // ---- a scattering in background layer b: the deposit needs no walk (the layers are horizontally uniform)
                                bg_done = true;
                                if (aerosol) { gc = ga; phase = hg_phase(min(ga, g_max), cs); }
                                else if (cloud)
                                {
                                    const F g = min(gc, g_max);
                                    const F q = (F(1.) + g*g) - (F(2.)*g)*cs;
                                    phase = (F(1.) - g*g) / (q*sqrt(q));
                                }
                                else phase = F(0.75)*(F(1.) + cs*cs);
                                const F dep = (weight*phase)/(F(4.)*pi);
                                deposit(dep*exp(-((k_ext*(z_hi - z) + bg.tau_above[cell])/a.mu0)), pix);
                                scatter_direction(rng, cloud || aerosol, gc, g_max, ux, uy, uz);
                            }
                        }
                        if (bg_done) break;
                        if (aerosol) { gc = ga; phase = hg_phase(min(ga, g_max), cs); }
                        else if constexpr (TABLE)
                        {
                            if (cloud) { gc = ph.in.cld_re[cell]; phase = phase_eval(tab, mu_s, gc, cs); }          // cld_re (ncol, nz): one radius for all bands
                            else phase = F(0.75)*(F(1.) + cs*cs);
                        }
                        else if (cloud)
                        {
                            const F g = min(gc, g_max);
                            const F q = (F(1.) + g*g) - (F(2.)*g)*cs;
                            phase = (F(1.) - g*g) / (q*sqrt(q));
                        }
                        else phase = F(0.75)*(F(1.) + cs*cs);
                        begin_walk(w, a, vx, vy, vz, x, y, z, i, j, k, (weight*phase)/(F(4.)*pi), aerosol ? 3 : (cloud ? 2 : 1), gc);
                        walking = true;
                    }
                }
            } while (false);
            if (done) break;
        }
    }
}

// ---- host side (rrx_rt_host.h)

// the checks of the backward entries: check_entry with the sensor's extents and checks; max_walk: the bound of the walk to the sun
template<typename F, typename A, typename B, typename C>
bool check_backward(const Medium<F>& m, const Sun<F>& sun, const PhaseIn<F>& ph, const Background<F>& bg, const int max_events,
                    const Sensor<F>& sensor, std::pair<const char*, long long> work, Needed inputs, Needed outputs, int& max_walk,
                    A after_nbnd, B after_phase, C after_scene)
{
    return check_entry(m, RT_NEEDED_SOLAR(m), &sun, ph, bg, max_events, {{"npx", sensor.npx}, {"npy", sensor.npy}, work}, inputs, outputs,
                       after_nbnd, after_phase, after_scene, [&] { check_sensor(sensor); max_walk = walk_bound(m, sun.mu0); });
}

// THE BUILDER of the kernel arguments
template<typename F>
BwArgs<F> scene_args(const Medium<F>& m, const Sun<F>& sun, const Sensor<F>& sensor, const int igpt, const F* k_null, const u64 seed,
                     const u64 ray0, const long long nrays, const int max_events, const int max_walk, u64* counts, u64* n_capped, u64* n_clamped)
{
    BwArgs<F> a{};
    set_medium(a, m, igpt, k_null, max_events);
    set_sun_and_key(a, sun, seed);
    set_sensor(a, sensor);
    a.sfc_albedo = m.sfc_albedo; a.mu0 = sun.mu0;
    a.ray0 = ray0; a.nrays = nrays; a.max_walk = max_walk;
    a.counts = counts; a.n_capped = n_capped; a.n_clamped = n_clamped;
    return a;
}

// form: which instantiation runs; b is read in the forms with a background (its aerosol triple in FORM_AER, whose profile has
// BG_ROWS_AER rows)
// FORM_SPECTRAL: a.ray0 / a.nrays are a range of the concatenated list sp.photon_end, a.k_null holds the slices from g-point sp.kn_g0 on
// and b.in.profile is the profile of all g-points
template<typename F>
void launch_trace_bw(const BwArgs<F>& a, const PhaseIn<F>& ph, hipStream_t st, const Form form, const BgArgs<F,true,true>& b,
                     const SpecIn<F>& sp = SpecIn<F>{})
{
    const int blocks = int(std::min<long long>((a.nrays + RT_BLOCK - 1) / RT_BLOCK, max_blocks()));
    const size_t lds = form == FORM_SPECTRAL ? bw_spectral_lds_bytes(sp.ngpt, b.in.nbg, ph.given() ? ph.nmu : 0, sizeof(F))
                     : (ph.given() ? size_t(ph.nmu)*sizeof(F) : 0)
                     + (form == FORM_GRID ? 0 : bg_lds_numbers(b.in.nbg, form == FORM_AER ? BG_ROWS_AER : BG_ROWS)*sizeof(F));
    const BgArgs<F,true> bg{b.in};
    switch (2*form + (ph.given() ? 1 : 0))
    {
        case 2*FORM_AER + 1: trace_bw_kernel<F,true,true,true><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,true>{ph}, b); break;
        case 2*FORM_AER: trace_bw_kernel<F,false,true,true><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,false>{}, b); break;
        case 2*FORM_BG + 1: trace_bw_kernel<F,true,true,false><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,true>{ph}, bg); break;
        case 2*FORM_BG: trace_bw_kernel<F,false,true,false><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,false>{}, bg); break;
        case 2*FORM_GRID + 1: trace_bw_kernel<F,true,false,false><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,true>{ph}, BgArgs<F,false>{}); break;
        case 2*FORM_SPECTRAL + 1:
            trace_bw_kernel<F,true,true,true,true><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,true>{ph}, BwSpecArgs<F>{b.in, b.aer, sp}); break;
        case 2*FORM_SPECTRAL:
            trace_bw_kernel<F,false,true,true,true><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,false>{}, BwSpecArgs<F>{b.in, b.aer, sp}); break;
        default: trace_bw_kernel<F,false,false,false><<<blocks, RT_BLOCK, lds, st>>>(a, PhaseArgs<F,false>{}, BgArgs<F,false>{});
    }
}

// rrx_rt_bw_trace_counts, _phase (bg.form = FORM_GRID), _bg, _aer
template<typename F>
int trace_bw_entry(const char* entry, const Medium<F>& m, const Sun<F>& sun, const PhaseIn<F>& ph, const Background<F>& bg, const Run& run,
                   const Sensor<F>& sensor, const int igpt, const F* k_null, const long long ray0, const long long nrays,
                   u64* counts, u64* n_capped, u64* n_clamped)
{
    RRX_TRY
    int max_walk = 0;
    if (check_backward(m, sun, ph, bg, run.max_events, sensor, {"nrays", nrays}, {{"k_null", k_null}, {"sensor", sensor.s}},
                       {{"counts", counts}, {"n_capped", n_capped}, {"n_clamped", n_clamped}}, max_walk,
                       [&] { if (ray0 < 0) throw std::runtime_error("ray0 is negative"); }, [&] { check_igpt(igpt, m.ngpt); }, nothing))
        return 0;
    BgArgs<F,true,true> b{BgIn<F>{}, m.aer};
    if (bg.form != FORM_GRID) b.in = background_of(bg, m, nothing);
    launch_trace_bw<F>(scene_args<F>(m, sun, sensor, igpt, k_null, run.seed, u64(ray0), nrays, run.max_events, max_walk, counts, n_capped, n_clamped),
                       ph, static_cast<hipStream_t>(run.stream), form_of(bg, m), b);
    RRX_CATCH(entry)
}

// rrx_raytracer_bw, _phase (bg.form = FORM_GRID), _bg, _aer
template<typename F>
int raytracer_bw_entry(const char* entry, const Medium<F>& m, const Sun<F>& sun, const PhaseIn<F>& ph, const Background<F>& bg, const Run& run,
                       const Sensor<F>& sensor, const F* inc_dir, const long long rays_per_pixel, F* radiance, u64* n_capped, u64* n_clamped)
{
    RRX_TRY
    typedef ForwardEntries<F> Fw;
    int max_walk = 0;
    if (check_backward(m, sun, ph, bg, run.max_events, sensor, {"rays_per_pixel", rays_per_pixel}, {{"inc_dir", inc_dir}, {"sensor", sensor.s}},
                       {{"radiance", radiance}, {"n_capped", n_capped}, {"n_clamped", n_clamped}}, max_walk, nothing, nothing,
                       [&] { for (int g=0; g<m.ngpt; ++g)
                                 if (inc_dir[g] < F(0.)) throw std::runtime_error("inc_dir must be >= 0"); }))
        return 0;
    const LoopBg<F> lb = loop_background(bg, m, nothing);

    // the workspace, in u64 words: | counts (npix) | k_null | the background's profile |
    hipStream_t st = static_cast<hipStream_t>(run.stream);
    const size_t npix = size_t(sensor.npx)*sensor.npy;
    const size_t n_kn = words_of(size_t(m.knx)*m.kny*m.knz*sizeof(F));
    const size_t n_prof = lb.on ? words_of(size_t(lb.form == FORM_AER ? BG_ROWS_AER : BG_ROWS)*(lb.nbg + 1)*sizeof(F)) : 0;
    WorkspaceLease lease(st);
    u64* counts = lease.get<u64>(npix + n_kn + n_prof);
    F* k_null = reinterpret_cast<F*>(counts + npix);
    F* profile = reinterpret_cast<F*>(counts + npix + n_kn);
    zero_outputs(radiance, npix, n_capped, n_clamped, st);
    const long long nrays = rays_per_pixel*(long long)npix;
    const BgArgs<F,true,true> b{BgIn<F>{lb.nbg, profile, lb.lev}, m.aer};
    for (int g=0; g<m.ngpt; ++g)
    {
        if (!(inc_dir[g] > F(0.))) continue;
        if (hipMemsetAsync(counts, 0, npix*sizeof(u64), st) != hipSuccess) throw std::runtime_error("zeroing the counts failed");
        if (m.aer.tau != nullptr)
            forward(Fw::k_null_aer(m.nx, m.ny, m.nz, m.ngpt, m.nbnd, g, m.top_at_1, m.tau, m.band_lims_gpt, m.cld_tau, m.dz, m.knx, m.kny, m.knz,
                                   k_null, m.aer.tau, run.stream));
        else
            forward(Fw::k_null(m.nx, m.ny, m.nz, m.ngpt, m.nbnd, g, m.top_at_1, m.tau, m.band_lims_gpt, m.cld_tau, m.dz, m.knx, m.kny, m.knz,
                               k_null, run.stream));
        if (lb.on && lb.form == FORM_AER)
            forward(Fw::bg_profile_aer(bg.nbg, m.ngpt, m.nbnd, g, bg.dz_bg, bg.tau, bg.ssa, m.band_lims_gpt, bg.cld_tau, bg.cld_ssa, bg.cld_g, profile,
                                       lb.aer.tau, lb.aer.ssa, lb.aer.g, run.stream));
        else if (lb.on)
            forward(Fw::bg_profile(bg.nbg, m.ngpt, m.nbnd, g, bg.dz_bg, bg.tau, bg.ssa, m.band_lims_gpt, bg.cld_tau, bg.cld_ssa, bg.cld_g, profile,
                                   run.stream));
        launch_trace_bw<F>(scene_args<F>(m, sun, sensor, g, k_null, run.seed, 0ull, nrays, run.max_events, max_walk, counts, n_capped, n_clamped),
                           ph, st, lb.form, b);
        const F scale = inc_dir[g] / (sun.mu0*F(rays_per_pixel));
        forward(Fw::counts_to_flux((long long)npix, counts, scale, radiance, run.stream));
    }
    RRX_CATCH(entry)
}

// ---- the camera's spectral form: rays of all g-points in one launch, counts by band, bands to channels

// out[c, pix] = scale sum_b M[c, b] (counts[b, pix] 2^-32), the sum in band order in F: one thread per pixel and channel
template<typename F>
__global__ void channels_kernel(const size_t npix, const int nbnd, const int nchan, const u64* __restrict__ counts, const F* __restrict__ M,
                                const F scale, F* __restrict__ out)
{
    const size_t i = size_t(blockIdx.x)*blockDim.x + threadIdx.x;
    if (i >= npix*size_t(nchan)) return;
    const size_t c = i / npix, pix = i - c*npix;
    F sum = F(0.);
    for (int b=0; b<nbnd; ++b) sum = sum + M[c*nbnd + b]*F(double(counts[size_t(b)*npix + pix]) * 2.3283064365386963e-10);
    out[i] = scale*sum;
}

template<typename F>
void launch_channels(const size_t npix, const int nbnd, const int nchan, const u64* counts, const F* M, const F scale, F* out, hipStream_t st)
{
    channels_kernel<F><<<unsigned(ceil_div((long long)(npix*size_t(nchan)), 256)), 256, 0, st>>>(npix, nbnd, nchan, counts, M, scale, out);
}

// rrx_camera_channels
template<typename F>
int camera_channels_entry(const char* entry, const long long npix, const int nbnd, const int nchan, const u64* counts, const F* chan_weights,
                          const F scale, F* out, void* stream)
{
    RRX_TRY
    if (check_extents({{"npix", npix}})) return 0;
    check_channels(nbnd, nchan);
    if (npix > 0x7FFFFFFFll) throw std::runtime_error("npix exceeds 2^31 - 1");
    if ((long long)nchan > (0x7FFFFFFFll << 8) / npix) throw std::runtime_error("nchan npix exceeds 2^39: one thread per pixel and channel");
    check_needed({{"counts", counts}, {"chan_weights", chan_weights}, {"out", out}});
    launch_channels<F>(size_t(npix), nbnd, nchan, counts, chan_weights, scale, out, static_cast<hipStream_t>(stream));
    RRX_CATCH(entry)
}

// rrx_camera_trace_counts_spectral: sp.photon_end (the ray list's prefix sums) and sp.weight0 are device arrays that the entry cannot
// look into. The kernel stays inside its arrays whatever they hold (the search is bounded by ngpt, a ray beyond the list is stepped over,
// the pixel is taken modulo npix); the callers that form the list on the host refuse one that does not ascend. k_null and bg.profile
// are those of all g-points.
template<typename F>
int camera_trace_entry(const char* entry, const Medium<F>& m, const Sun<F>& sun, const PhaseIn<F>& ph, const Background<F>& bg, const Run& run,
                       const Sensor<F>& sensor, const SpecIn<F>& sp, const F* k_null, const long long ray0, const long long nrays,
                       u64* counts, u64* n_capped, u64* n_clamped)
{
    RRX_TRY
    int max_walk = 0;
    if (check_backward(m, sun, ph, bg, run.max_events, sensor, {"nrays", nrays},
                       {{"band_lims_gpt", m.band_lims_gpt}, {"ray_end", sp.photon_end}, {"weight0", sp.weight0}, {"k_null", k_null}, {"sensor", sensor.s}},
                       {{"counts", counts}, {"n_capped", n_capped}, {"n_clamped", n_clamped}}, max_walk,
                       [&] { check_spectral_ngpt(m.ngpt);
                             if (m.nbnd < 1) throw std::runtime_error("nbnd must be >= 1: the counts are kept by band");
                             if (ray0 < 0) throw std::runtime_error("ray0 is negative"); }, nothing, nothing))
        return 0;
    const BgArgs<F,true,true> b{background_of(bg, m, nothing), m.aer};
    launch_trace_bw<F>(scene_args<F>(m, sun, sensor, 0, k_null, run.seed, u64(ray0), nrays, run.max_events, max_walk, counts, n_capped, n_clamped),
                       ph, static_cast<hipStream_t>(run.stream), FORM_SPECTRAL, b, sp);
    RRX_CATCH(entry)
}

// rrx_camera_render_spectral: m_gpt[g] rays per pixel of g-point g (a host array). One trace launch per chunk of consecutive g-points,
// the counts of all chunks added in integers by band and converted once, with the common unit U = S/P over mu0, through the channel
// matrix. The list, the workspace and the chunk loop are rrx_rt_host.h's; the workspace's mid section is the profile of all g-points.
template<typename F>
int camera_render_entry(const char* entry, const Medium<F>& m, const Sun<F>& sun, const PhaseIn<F>& ph, const Background<F>& bg, const Run& run,
                        const Sensor<F>& sensor, const F* inc_dir, const long long* m_gpt, const int nchan, const F* chan_weights,
                        F* radiance, u64* n_capped, u64* n_clamped)
{
    RRX_TRY
    typedef ForwardEntries<F> Fw;
    int max_walk = 0;
    const long long npix_ll = (long long)sensor.npx*sensor.npy;
    std::vector<long long> ray_end;
    long long P = 0;
    F S = F(0.);
    if (check_backward(m, sun, ph, bg, run.max_events, sensor, {"ngpt", m.ngpt},
                       {{"band_lims_gpt", m.band_lims_gpt}, {"inc_dir", inc_dir}, {"rays_per_pixel_gpt", m_gpt}, {"chan_weights", chan_weights},
                        {"sensor", sensor.s}},
                       {{"radiance", radiance}, {"n_capped", n_capped}, {"n_clamped", n_clamped}}, max_walk,
                       [&] { check_spectral_ngpt(m.ngpt); check_channels(m.nbnd, nchan); }, nothing,
                       [&] {
                           check_npix(sensor);
                           ray_list(m.ngpt, npix_ll, m_gpt, ray_end, P, [&](const int g) {
                               if (inc_dir[g] < F(0.)) throw std::runtime_error("inc_dir must be >= 0");
                               if (!(m_gpt[g] > 0)) return;
                               if (!(inc_dir[g] > F(0.)))
                                   throw std::runtime_error("rays_per_pixel_gpt is > 0 at g-point " + std::to_string(g) + ", which has no incident flux");
                               S = S + inc_dir[g];
                           });
                       }))
        return 0;
    const LoopBg<F> lb = loop_background(bg, m, nothing);

    hipStream_t st = static_cast<hipStream_t>(run.stream);
    const size_t npix = size_t(npix_ll);
    zero_outputs(radiance, size_t(nchan)*npix, n_capped, n_clamped, st);
    if (P == 0) return 0;
    const F U = S / F(P);
    std::vector<F> weight0(m.ngpt, F(0.));
    for (int g=0; g<m.ngpt; ++g)
        if (m_gpt[g] > 0) weight0[g] = (inc_dir[g] / F(m_gpt[g])) / U;

    const size_t n_prof = lb.on ? words_of(size_t(m.ngpt)*BG_ROWS_AER*(lb.nbg + 1)*sizeof(F)) : 0;
    SpectralWork<F> w(m, st, npix, nchan, ray_end, weight0, chan_weights, n_prof, 0, nullptr, 0);
    if (lb.on)
        forward(Fw::bg_profile_all(bg.nbg, m.ngpt, m.nbnd, bg.dz_bg, bg.tau, bg.ssa, m.band_lims_gpt, bg.cld_tau, bg.cld_ssa, bg.cld_g, w.mid,
                                   lb.aer.tau, lb.aer.ssa, lb.aer.g, run.stream));
    const BgArgs<F,true,true> b{BgIn<F>{lb.nbg, w.mid, lb.lev}, m.aer};
    w.trace(m, run.stream,
            [&](const int g, F* k_null) {
                forward(Fw::k_null_aer(m.nx, m.ny, m.nz, m.ngpt, m.nbnd, g, m.top_at_1, m.tau, m.band_lims_gpt, m.cld_tau, m.dz, m.knx, m.kny, m.knz,
                                       k_null, m.aer.tau, run.stream)); },
            [&](const SpecIn<F>& sp, const u64 ray0, const long long n) {
                launch_trace_bw<F>(scene_args<F>(m, sun, sensor, 0, w.k_null, run.seed, ray0, n, run.max_events, max_walk, w.counts, n_capped, n_clamped),
                                   ph, st, FORM_SPECTRAL, b, sp); });
    launch_channels<F>(npix, m.nbnd, nchan, w.counts, w.chan, U / sun.mu0, radiance, st);
    RRX_CATCH(entry)
}
}  // namespace

// ---- the C entries: each builds the structs and calls its family's one function
#define RT_P_BW_TRACE(F) \
        int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, RT_P_GRID(F), int knx, int kny, int knz, const F* k_null, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, unsigned long long seed, long long ray0, long long nrays, int max_events, \
        unsigned long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped
#define RT_P_BW_LOOP(F) \
        int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RT_P_GRID(F), const F* inc_dir, int knx, int kny, int knz, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, long long rays_per_pixel, unsigned long long seed, int max_events, \
        F* radiance, unsigned long long* n_capped, unsigned long long* n_clamped
#define RT_SENSOR(F) Sensor<F>{sensor_type, npx, npy, fov, sensor}
#define RT_BW_TRACE(F, NAME, AER, PHASE, BG) \
        trace_bw_entry<F>(NAME, RT_MEDIUM(F, 0, AER), RT_SUN(F), PHASE, BG, RT_RUN, RT_SENSOR(F), igpt, k_null, ray0, nrays, counts, n_capped, n_clamped)
#define RT_BW_LOOP(F, NAME, AER, PHASE, BG) \
        raytracer_bw_entry<F>(NAME, RT_MEDIUM(F, 0, AER), RT_SUN(F), PHASE, BG, RT_RUN, RT_SENSOR(F), inc_dir, rays_per_pixel, radiance, n_capped, n_clamped)

extern "C"
{
#define RRX_DEFINE_RT_BW(F, SFX) \
int rrx_rt_bw_trace_counts##SFX(RT_P_BW_TRACE(F), void* stream) \
{ return RT_BW_TRACE(F, "rrx_rt_bw_trace_counts" #SFX, AerIn<F>{}, PhaseIn<F>{}, RT_NO_BG(F)); } \
int rrx_raytracer_bw##SFX(RT_P_BW_LOOP(F), void* stream) \
{ return RT_BW_LOOP(F, "rrx_raytracer_bw" #SFX, AerIn<F>{}, PhaseIn<F>{}, RT_NO_BG(F)); } \
int rrx_rt_bw_trace_counts_phase##SFX(RT_P_BW_TRACE(F), RT_P_PHASE(F), void* stream) \
{ return RT_BW_TRACE(F, "rrx_rt_bw_trace_counts_phase" #SFX, AerIn<F>{}, RT_PHASE(F), RT_NO_BG(F)); } \
int rrx_raytracer_bw_phase##SFX(RT_P_BW_LOOP(F), RT_P_PHASE(F), void* stream) \
{ return RT_BW_LOOP(F, "rrx_raytracer_bw_phase" #SFX, AerIn<F>{}, RT_PHASE(F), RT_NO_BG(F)); } \
int rrx_rt_bw_trace_counts_bg##SFX(RT_P_BW_TRACE(F), RT_P_PHASE(F), int nbg, const F* dz_bg, const F* bg_profile, void* stream) \
{ return RT_BW_TRACE(F, "rrx_rt_bw_trace_counts_bg" #SFX, AerIn<F>{}, RT_PHASE(F), RT_BG_PROFILE(F, FORM_BG)); } \
int rrx_raytracer_bw_bg##SFX(RT_P_BW_LOOP(F), RT_P_PHASE(F), RT_P_BG(F), void* stream) \
{ return RT_BW_LOOP(F, "rrx_raytracer_bw_bg" #SFX, AerIn<F>{}, RT_PHASE(F), RT_BG_MEDIUM(F, FORM_BG, AerIn<F>{})); } \
int rrx_rt_bw_trace_counts_aer##SFX(RT_P_BW_TRACE(F), RT_P_PHASE(F), int nbg, const F* dz_bg, const F* bg_profile, \
        const F* aer_tau, const F* aer_ssa, const F* aer_g, void* stream) \
{ const AerIn<F> aer{aer_tau, aer_ssa, aer_g}; \
  return RT_BW_TRACE(F, "rrx_rt_bw_trace_counts_aer" #SFX, aer, RT_PHASE(F), RT_BG_PROFILE(F, FORM_AER)); } \
int rrx_raytracer_bw_aer##SFX(RT_P_BW_LOOP(F), RT_P_PHASE(F), RT_P_BG(F), \
        const F* aer_tau, const F* aer_ssa, const F* aer_g, const F* bg_aer_tau, const F* bg_aer_ssa, const F* bg_aer_g, void* stream) \
{ const AerIn<F> aer{aer_tau, aer_ssa, aer_g}, bg_aer{bg_aer_tau, bg_aer_ssa, bg_aer_g}; \
  return RT_BW_LOOP(F, "rrx_raytracer_bw_aer" #SFX, aer, RT_PHASE(F), RT_BG_MEDIUM(F, FORM_AER, bg_aer)); }

RRX_DEFINE_RT_BW(double, _f64)
RRX_DEFINE_RT_BW(float, _f32)

// The camera's spectral form. The prefix is rrx_camera_: the set of rrx_rt_ / rrx_raytracer_ symbols is closed.
#define RRX_DEFINE_CAMERA(F, SFX) \
int rrx_camera_trace_counts_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RT_P_GRID(F), \
        const long long* ray_end, const F* weight0, int knx, int kny, int knz, const F* k_null, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, unsigned long long seed, long long ray0, long long nrays, int max_events, \
        unsigned long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, \
        RT_P_PHASE(F), int nbg, const F* dz_bg, const F* bg_profile, const F* aer_tau, const F* aer_ssa, const F* aer_g, void* stream) \
{ const AerIn<F> aer{aer_tau, aer_ssa, aer_g}; \
  return camera_trace_entry<F>("rrx_camera_trace_counts_spectral" #SFX, RT_MEDIUM(F, 0, aer), RT_SUN(F), RT_PHASE(F), RT_BG_PROFILE(F, FORM_AER), \
                               RT_RUN, RT_SENSOR(F), SpecIn<F>{ngpt, 0, ray_end, weight0, nullptr}, k_null, ray0, nrays, counts, n_capped, n_clamped); } \
int rrx_camera_channels##SFX(long long npix, int nbnd, int nchan, const unsigned long long* counts, const F* chan_weights, F scale, F* out, \
        void* stream) \
{ return camera_channels_entry<F>("rrx_camera_channels" #SFX, npix, nbnd, nchan, counts, chan_weights, scale, out, stream); } \
int rrx_camera_render_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RT_P_GRID(F), const F* inc_dir, \
        int knx, int kny, int knz, int sensor_type, int npx, int npy, F fov, const F* sensor, const long long* rays_per_pixel_gpt, \
        unsigned long long seed, int max_events, int nchan, const F* chan_weights, \
        F* radiance, unsigned long long* n_capped, unsigned long long* n_clamped, RT_P_PHASE(F), RT_P_BG(F), \
        const F* aer_tau, const F* aer_ssa, const F* aer_g, const F* bg_aer_tau, const F* bg_aer_ssa, const F* bg_aer_g, void* stream) \
{ const AerIn<F> aer{aer_tau, aer_ssa, aer_g}, bg_aer{bg_aer_tau, bg_aer_ssa, bg_aer_g}; \
  return camera_render_entry<F>("rrx_camera_render_spectral" #SFX, RT_MEDIUM(F, 0, aer), RT_SUN(F), RT_PHASE(F), RT_BG_MEDIUM(F, FORM_AER, bg_aer), \
                                RT_RUN, RT_SENSOR(F), inc_dir, rays_per_pixel_gpt, nchan, chan_weights, radiance, n_capped, n_clamped); }

RRX_DEFINE_CAMERA(double, _f64)
RRX_DEFINE_CAMERA(float, _f32)
}
