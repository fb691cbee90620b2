// Thermal emission in the backward Monte Carlo ray tracer: longwave radiances for a virtual camera, 3-D longwave fluxes for a flux
// sensor. The longwave twin of rrx_raytracer_bw.hip: the same sensors, the same start, the same
// tracking through the grid, operation for operation, and NO SUN: the source that scores a ray is the Planck emission of the medium,
// of the surface and of whatever lies above the domain top. There is no walk, so this is a kernel of its own and not a flag of
// trace_bw_kernel; the kernel states its start and its tracking itself, as the two other trace kernels do (DESIGN 4.23 has what was
// tried of sharing them). Its host side is rrx_rt_host.h's: the sensor, the checks, the ray list and the spectral loop.
//
// THE ESTIMATOR. Rays start at the sensor and travel AGAINST the light through the medium of one g-point: k_ext = (tau + tau_c)/dz,
// k_sca = (tau ssa + tau_c ssa_c)/dz, k_sca_cld = (tau_c ssa_c)/dz from the clear tau, ssa (ncol, nz, ngpt) and the band cloud triple;
// a NULL ssa is a gas that does not scatter (ssa = 0, what the LW gas optics give). Null-collision tracking on the k_null grid of
// rrx_rt_k_null with integer block indices (in, jn, kn); a free path that is carried across a face (pending); periodic x / y;
// f_no_abs = clampf(1 - (k_ext - k_sca)/k_null, 0, 1); Russian roulette below weight 0.5; the scatter-or-null draw and the species draw;
// Rayleigh on the gas, Henyey-Greenstein with g = min(g_c, 1 - eps) on the cloud; a Lambertian surface of emissivity sfc_emis[col]
// that reflects 1 - sfc_emis[col]. The sources are radiances (W m-2 sr-1): lay_src (ncol, nz, ngpt), constant within a cell,
// sfc_src (ncol, ngpt), and top_radiance, one isotropic downward radiance at the domain top. A deposit d is made BEFORE the weight
// changes
//   - at a collision in a cell:  d = (weight (1 - f_no_abs)) lay_src[cell, g];   then weight *= f_no_abs
//   - at a surface hit:          d = (weight sfc_emis[col]) sfc_src[col, g];     then weight *= 1 - sfc_emis[col]
//   - where the ray ends at the top (it leaves through it, or starts at or above it and does not look down): d = weight top_radiance
// The collision's deposit is the expected value of "absorbed here with probability 1 - f_no_abs: score the local source"; the two
// others follow the same pattern, so with the roulette the estimate is unbiased. Nothing is deposited at a scattering.
//
// TALLY. One unsigned 64-bit count per camera pixel in units of 2^-32: llrint(min(d, 2^20) 2^32), added with an integer atomic; a
// clamped deposit is counted in n_clamped; a ray alive after max_events events (collisions + crossings) is dropped and counted in
// n_capped, and so is one that no face stops. Radiance of a g-point = counts 2^-32 / rays_per_pixel (W m-2 sr-1). Bit-reproducible,
// independent of the order of arrival, additive over ray ranges.
//
// RANDOM NUMBERS. Philox4x32-10, key = seed, counter (ray low, ray high, igpt | 0xC0000000, block): disjoint from the forward tracer's
// (igpt) and the backward one's (igpt | 0x80000000). Ray r belongs to camera pixel pix = r mod npix, ipx = pix mod npx,
// ipy = pix / npx. DRAW ORDER (tests/raytracer_thermal_ref.py restates it):
//   start:     u -> a = (ipx + u)/npx;  u -> b = (ipy + u)/npy;  sensor type 3 only: u -> mu = sqrt(u);  u -> phi = 2 pi u
//   each event: u -> tau = -log(u), unless the previous event was a crossing between blocks
//     surface:   deposit; weight *= 1 - emis; weight < 0.5: u -> survives (weight = 1) iff u <= weight; survivor: u -> mu; u -> phi
//     collision: deposit; weight *= f_no_abs; weight < 0.5: u -> roulette; survivor: u -> scatter or null; scatter: u -> species
//                (cloud iff u k_sca < k_sca_cld, drawn with a NULL ssa too); u -> cos of the scattering angle; u -> phi
//
// SENSORS: those of rrx_raytracer_bw.hip without a background (12 host numbers: position, e_w, e_h, e_d): 0 perspective, 1 fisheye,
// 2 orthographic from the domain top, 3 flux sensor (cosine-weighted, at the surface facing up or at the top facing down: pi x the
// mean radiance is an irradiance). A start at or above the top with a downward direction is moved along the ray to the top.
//
// SHAPE. One ray per lane, lanes refill from a round-robin list inside the one event loop, RT_BLOCK threads, the grid capped by
// max_blocks(). No LDS in the per-g-point form. Registers: DESIGN 4.23.
//
// SPECTRAL (trace_thermal_kernel<F,true>, the _spectral entries; rrx_rt_common.h): the rays of all g-points in one launch.
// a.ray0 / a.nrays address the concatenated list whose prefix sums are sp.photon_end (here: ray_end); the g-point is state of the ray,
// set when a lane takes its next one. Ray p of the list is ray q = p - ray_end[g] of g-point g in the per-g-point launch, draw for draw.
// The g-point is not a register of its own: it is read back from word 2 of the ray's Philox counter (g | 0xC0000000), which the lane
// carries anyway. The k_null slice, the tau / ssa / lay_src / cloud slices and the sfc_src slice are derived from it where they are
// read (the block's k_null, the collision, the surface hit): the lane carries no pointers around the loop (registers: DESIGN 4.24).
// Only the source that a deposit reads is scaled, and it is scaled first:
//   d = (weight (1 - f_no_abs)) (lay_src[cell, g] weight0[g]),  (weight sfc_emis[col]) (sfc_src[col, g] weight0[g]),
//   weight (top_radiance[g] weight0[g]);  top_radiance is a device array here, NULL = 0;
// then the clamp at 2^20, and the tally into counts[band(g) npix + pix]; a.igpt and a.top_radiance are not read. A g-point that lies
// in no band has no row of counts: its deposits are dropped (a clamped one is still counted). ray_end and the band table live in LDS.
//
// LIMITS: no background layers above the grid (top_radiance closes the medium), no aerosol, no phase table, a cell-constant source (no
// interpolation between level sources), no brightness temperatures.
#include "rrx_rt_host.h"

namespace
{
using namespace rrx;
using namespace rrx::rt;

template<typename F>
struct ThermalArgs
{
    int nx, ny, nz, nbnd, igpt, top_at_1;
    const F* tau; const F* ssa; const int* band_lims_gpt; const F* cld_tau; const F* cld_ssa; const F* cld_g;
    F dx, dy, dz;
    const F* sfc_emis; const F* lay_src; const F* sfc_src;
    F top_radiance;
    int knx, kny, knz;
    const F* k_null;
    unsigned k0, k1;
    u64 ray0; long long nrays; int max_events;
    int type, npx, npy;
    F fov, px, py, pz, wx, wy, wz, hx, hy, hz, ex, ey, ez;
    u64* counts; u64* n_capped; u64* n_clamped;
};

// what the spectral form takes beside ThermalArgs: the ray list and the weights (SpecIn; dif_frac is not read) and the top radiance of
// every g-point on the device (NULL: 0); empty in the per-g-point form
template<typename F, bool SPECTRAL> struct ThermalSpecArgs {};
template<typename F> struct ThermalSpecArgs<F,true> { SpecIn<F> sp; const F* top_radiance; };

template<typename F, bool SPECTRAL>
__global__ void __launch_bounds__(RT_BLOCK) trace_thermal_kernel(const ThermalArgs<F> a, const ThermalSpecArgs<F,SPECTRAL> s)
{
    [[maybe_unused]] SpecView sv{};
    if constexpr (SPECTRAL)
    {
        extern __shared__ double spectral_lds[];
        BgView<F> no_bg{};
        sv = stage_spectral<F>(s.sp, BgIn<F>{}, a.nbnd, a.band_lims_gpt, spectral_lds, no_bg);          // (it ends with the barrier)
    }
    const long long nthreads = (long long)gridDim.x*blockDim.x;
    long long next_ray = (long long)blockIdx.x*blockDim.x + threadIdx.x;

    const int nx = a.nx, ny = a.ny, nz = a.nz;
    const size_t ncol = size_t(nx)*ny;
    const int rx = nx/a.knx, ry = ny/a.kny, rz = nz/a.knz;
    const F kdx = F(rx)*a.dx, kdy = F(ry)*a.dy, kdz = F(rz)*a.dz;
    const F len_x = F(a.knx)*kdx, len_y = F(a.kny)*kdy, z_top = F(a.knz)*kdz;
    const int npix = a.npx*a.npy;
    // the g-point is fixed for the launch, or under SPECTRAL state of the lane's ray (word 2 of its Philox counter): what follows is
    // then derived from it where it is read
    Stream rng; rng.k0 = a.k0; rng.k1 = a.k1; rng.used = 4; rng.block = 0u; rng.c0 = rng.c1 = rng.c2 = 0u;
    const auto gpt = [&]() {
        if constexpr (SPECTRAL) return int(rng.c2 & 0x3FFFFFFFu);
        else return a.igpt;
    };
    int ibnd = -1;
    const F* __restrict__ tau_g = a.tau;
    const F* __restrict__ ssa_g = a.ssa;
    const F* __restrict__ lay_src_g = a.lay_src;
    const F* __restrict__ sfc_src_g = a.sfc_src;
    const F* __restrict__ kn_g = a.k_null;
    if constexpr (!SPECTRAL)
    {
        ibnd = a.cld_tau != nullptr ? band_of(a.igpt, a.nbnd, a.band_lims_gpt) : -1;
        tau_g = a.tau + ncol*nz*a.igpt;
        ssa_g = a.ssa != nullptr ? a.ssa + ncol*nz*a.igpt : nullptr;
        lay_src_g = a.lay_src + ncol*nz*a.igpt;
        sfc_src_g = a.sfc_src + ncol*a.igpt;
    }
    const F inf = F(INFINITY);
    const F g_max = F(1.) - Lim<F>::eps();
    // a source as a deposit reads it: under SPECTRAL scaled by the g-point's weight, before anything else
    const auto source = [&](const F v) {
        if constexpr (SPECTRAL) return v*s.sp.weight0[gpt()];
        else return v;
    };
    const auto top_source = [&]() {
        if constexpr (SPECTRAL) return (s.top_radiance != nullptr ? s.top_radiance[gpt()] : F(0.))*s.sp.weight0[gpt()];
        else return a.top_radiance;
    };
    // a deposit d of the lane's ray: clamped at 2^20 and tallied into its pixel (SPECTRAL: of its g-point's band)
    const auto deposit = [&](const F d, const int pix) {
        size_t slot = size_t(pix);
        [[maybe_unused]] int band = 0;
        if constexpr (SPECTRAL) { band = sv.band[gpt()]; slot += size_t(band < 0 ? 0 : band)*size_t(npix); }
        const bool clamped = d > F(1048576.);
        if (clamped) atomicAdd(a.n_clamped, 1ull);
        if constexpr (SPECTRAL) { if (band < 0) return; }
        tally(a.counts, slot, to_count(clamped ? F(1048576.) : d));
    };

    bool alive = false, pending = false;
    int in = 0, jn = 0, kn = 0, nev = 0, pix = 0;
    F x = F(0.), y = F(0.), z = F(0.), ux = F(0.), uy = F(0.), uz = F(-1.), weight = F(0.), tau = F(0.);

    // One loop with one back edge: a pass is one event of the lane's ray; a lane whose ray has ended takes its next one in the same pass
    for (;;)
    {
        if (!alive)
        {
            if (next_ray >= a.nrays) break;          // the list is finite and every ray ends within max_events events
            u64 r = a.ray0 + u64(next_ray);
            next_ray += nthreads;
            int igpt = a.igpt;
            if constexpr (SPECTRAL)
            {
                igpt = gpt_of_photon(sv.photon_end, sv.ngpt, (long long)r);
                if (igpt >= sv.ngpt) continue;          // (beyond the list)
                r = r - u64(sv.photon_end[igpt]);
            }
            rng.start(r, unsigned(igpt) | 0xC0000000u);
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
                if (a.type == 2) { ux = a.ex; uy = a.ey; uz = a.ez; sz = z_top; }
                else if (a.ez > F(0.)) { lambert(rng, F(1.), ux, uy, uz); sz = F(0.); }
                else { lambert(rng, F(-1.), ux, uy, uz); sz = z_top; }
            }
            if (sz >= z_top)
            {
                // it looks away from the medium: the ray ends at the top, with what comes down through it
                if (!(uz < F(0.))) { deposit(top_source(), pix); continue; }
                if (sz > z_top) { const F t = (z_top - sz)/uz; sx = sx + ux*t; sy = sy + uy*t; }
                sz = z_top;
            }
            sx = sx - floor(sx/len_x)*len_x; sy = sy - floor(sy/len_y)*len_y;
            in = clampi(int(sx/kdx), 0, a.knx - 1); jn = clampi(int(sy/kdy), 0, a.kny - 1); kn = clampi(int(sz/kdz), 0, a.knz - 1);
            x = clampf(sx, F(in)*kdx, F(in+1)*kdx); y = clampf(sy, F(jn)*kdy, F(jn+1)*kdy); z = clampf(sz, F(kn)*kdz, F(kn+1)*kdz);
            weight = F(1.); pending = false; nev = 0; alive = true;
        }
        if (nev >= a.max_events) { atomicAdd(a.n_capped, 1ull); alive = false; continue; }
        ++nev;

        const F x_lo = F(in)*kdx, x_hi = F(in+1)*kdx, y_lo = F(jn)*kdy, y_hi = F(jn+1)*kdy, z_lo = F(kn)*kdz, z_hi = F(kn+1)*kdz;
        const F sz = uz > F(0.) ? (z_hi - z)/uz : (uz < F(0.) ? (z_lo - z)/uz : inf);
        const F sx = ux > F(0.) ? (x_hi - x)/ux : (ux < F(0.) ? (x_lo - x)/ux : inf);
        const F sy = uy > F(0.) ? (y_hi - y)/uy : (uy < F(0.) ? (y_lo - y)/uy : inf);
        const F d_max = min(sz, min(sx, sy));
        const int axis = (sz <= sx && sz <= sy) ? 2 : (sx <= sy ? 0 : 1);
        if constexpr (SPECTRAL) kn_g = a.k_null + (size_t(a.knx)*a.kny*a.knz)*size_t(gpt() - s.sp.kn_g0);
        const F kn_val = kn_g[in + a.knx*(jn + a.kny*kn)];
        if (!pending) tau = -log(rng.next<F>());
        pending = false;
        const bool empty = !(kn_val > F(0.));
        const F tau_cell = empty ? F(0.) : d_max*kn_val;

        if (empty || tau >= tau_cell)
        {
            // ---- the ray leaves the block through the face of `axis`
            if (!(d_max < inf)) { atomicAdd(a.n_capped, 1ull); alive = false; continue; }
            tau = tau - tau_cell; pending = true;
            x = clampf(x + ux*d_max, x_lo, x_hi); y = clampf(y + uy*d_max, y_lo, y_hi); z = clampf(z + uz*d_max, z_lo, z_hi);
            if (axis == 0)
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
                if (kn == a.knz - 1) { deposit(weight*top_source(), pix); alive = false; }          // out through the domain top
                else { ++kn; z = F(kn)*kdz; }
            }
            else if (kn == 0)                 // the surface: it emits, and reflects the rest
            {
                z = F(0.);
                const int col = fine_cell(x, a.dx, in, rx) + nx*fine_cell(y, a.dy, jn, ry);
                const F emis = a.sfc_emis[col];
                if constexpr (SPECTRAL) sfc_src_g = a.sfc_src + ncol*gpt();
                deposit((weight*emis)*source(sfc_src_g[col]), pix);
                weight = weight * (F(1.) - emis);
                if (weight < F(0.5)) weight = (rng.next<F>() > weight) ? F(0.) : F(1.);
                if (!(weight > F(0.))) { alive = false; continue; }
                lambert(rng, F(1.), ux, uy, uz);
                pending = false;
            }
            else { --kn; z = F(kn+1)*kdz; }
        }
        else
        {
            // ---- a collision inside the block
            const F dn = tau / kn_val;
            x = clampf(x + ux*dn, x_lo, x_hi); y = clampf(y + uy*dn, y_lo, y_hi); z = clampf(z + uz*dn, z_lo, z_hi);
            const int i = fine_cell(x, a.dx, in, rx), j = fine_cell(y, a.dy, jn, ry), k = fine_cell(z, a.dz, kn, rz);
            const int lay = a.top_at_1 ? nz-1-k : k;
            const size_t cell = size_t(i) + size_t(j)*nx + ncol*lay;
            if constexpr (SPECTRAL)
            {
                ibnd = a.cld_tau != nullptr ? sv.band[gpt()] : -1;
                tau_g = a.tau + ncol*nz*gpt();
                ssa_g = a.ssa != nullptr ? a.ssa + ncol*nz*gpt() : nullptr;
                lay_src_g = a.lay_src + ncol*nz*gpt();
            }
            const F t = tau_g[cell], w0 = ssa_g != nullptr ? ssa_g[cell] : F(0.);
            F tc = F(0.), wc = F(0.), gc = F(0.);
            if (ibnd >= 0)
            {
                const size_t cb = cell + ncol*nz*ibnd;
                tc = a.cld_tau[cb]; wc = a.cld_ssa[cb]; gc = a.cld_g[cb];
            }
            const F k_ext = k_ext_of(t, tc, a.dz);
            const F k_sca = (t*w0 + tc*wc) / a.dz;
            const F k_sca_cld = (tc*wc) / a.dz;
            const F f_no_abs = clampf(F(1.) - (k_ext - k_sca)/kn_val, F(0.), F(1.));
            deposit((weight*(F(1.) - f_no_abs))*source(lay_src_g[cell]), pix);
            weight = weight * f_no_abs;
            if (weight < F(0.5)) weight = (rng.next<F>() > weight) ? F(0.) : F(1.);
            if (!(weight > F(0.))) { alive = false; continue; }
            if (rng.next<F>()*(k_sca + (kn_val - k_ext)) < k_sca)
            {
                const bool cloud = rng.next<F>()*k_sca < k_sca_cld;
                scatter_direction(rng, cloud, gc, g_max, ux, uy, uz);
            }
        }
    }
}

// ---- host side (rrx_rt_host.h): the scene structs, the sensor with its checks and the one check sequence of the two other
// tracers, which is told what this tracer needs of the medium (tau and the sources below; ssa may be NULL) and that it has no sun.

// the surface and the sources
template<typename F> struct ThermalSources { const F* sfc_emis; const F* lay_src; const F* sfc_src; };

inline void check_top_radiance(const double v)
{
    if (!std::isfinite(v) || v < 0.) throw std::runtime_error("top_radiance must be finite and >= 0");
}

// the checks of the thermal entries: check_entry with the sensor's extents and checks
template<typename F, typename A, typename B, typename C>
bool check_thermal(const Medium<F>& m, const ThermalSources<F>& src, const int max_events, const Sensor<F>& sensor,
                   std::pair<const char*, long long> work, Needed inputs, Needed outputs, A after_nbnd, B after_phase, C after_scene)
{
    const Sun<F>* no_sun = nullptr;
    return check_entry(m, {{"tau", m.tau}, {"sfc_emis", src.sfc_emis}, {"lay_src", src.lay_src}, {"sfc_src", src.sfc_src}}, no_sun, PhaseIn<F>{},
                       RT_NO_BG(F), max_events, {{"npx", sensor.npx}, {"npy", sensor.npy}, work}, inputs, outputs,
                       after_nbnd, after_phase, after_scene, [&] { check_sensor(sensor); });
}

// THE BUILDER of the kernel arguments
template<typename F>
ThermalArgs<F> thermal_args(const Medium<F>& m, const ThermalSources<F>& src, const F top_radiance, const Sensor<F>& sensor, const int igpt,
                            const F* k_null, const u64 seed, const u64 ray0, const long long nrays, const int max_events,
                            u64* counts, u64* n_capped, u64* n_clamped)
{
    ThermalArgs<F> a{};
    set_medium(a, m, igpt, k_null, max_events);
    set_key(a, seed);
    set_sensor(a, sensor);
    a.sfc_emis = src.sfc_emis; a.lay_src = src.lay_src; a.sfc_src = src.sfc_src; a.top_radiance = top_radiance;
    a.ray0 = ray0; a.nrays = nrays;
    a.counts = counts; a.n_capped = n_capped; a.n_clamped = n_clamped;
    return a;
}

template<typename F>
void launch_trace_thermal(const ThermalArgs<F>& a, hipStream_t st)
{
    const int blocks = int(std::min<long long>((a.nrays + RT_BLOCK - 1) / RT_BLOCK, max_blocks()));
    trace_thermal_kernel<F,false><<<blocks, RT_BLOCK, 0, st>>>(a, ThermalSpecArgs<F,false>{});
}

// the spectral form: a.ray0 / a.nrays are a range of the concatenated list sp.photon_end, a.k_null holds the slices from g-point
// sp.kn_g0 on, top_radiance is a device array (ngpt) or NULL
template<typename F>
void launch_trace_thermal_spectral(const ThermalArgs<F>& a, const SpecIn<F>& sp, const F* top_radiance, hipStream_t st)
{
    const int blocks = int(std::min<long long>((a.nrays + RT_BLOCK - 1) / RT_BLOCK, max_blocks()));
    trace_thermal_kernel<F,true><<<blocks, RT_BLOCK, spectral_lds_bytes(sp.ngpt, 0, sizeof(F)), st>>>(a, ThermalSpecArgs<F,true>{sp, top_radiance});
}

// rrx_thermal_trace_counts
template<typename F>
int thermal_trace_entry(const char* entry, const Medium<F>& m, const ThermalSources<F>& src, const F top_radiance, const Run& run,
                        const Sensor<F>& sensor, const int igpt, const F* k_null, const long long ray0, const long long nrays,
                        u64* counts, u64* n_capped, u64* n_clamped)
{
    RRX_TRY
    if (check_thermal(m, src, run.max_events, sensor, {"nrays", nrays}, {{"k_null", k_null}, {"sensor", sensor.s}},
                      {{"counts", counts}, {"n_capped", n_capped}, {"n_clamped", n_clamped}},
                      [&] { if (ray0 < 0) throw std::runtime_error("ray0 is negative"); }, [&] { check_igpt(igpt, m.ngpt); },
                      [&] { check_top_radiance(double(top_radiance)); }))
        return 0;
    launch_trace_thermal<F>(thermal_args<F>(m, src, top_radiance, sensor, igpt, k_null, run.seed, u64(ray0), nrays, run.max_events,
                                            counts, n_capped, n_clamped), static_cast<hipStream_t>(run.stream));
    RRX_CATCH(entry)
}

// rrx_thermal_render: the loop over all g-points. by_band: the band of a g-point is looked up in a host copy of band_lims_gpt, for which
// the call waits for its stream once, before its first launch.
template<typename F>
int thermal_render_entry(const char* entry, const Medium<F>& m, const ThermalSources<F>& src, const F* top_radiance, const Run& run,
                         const Sensor<F>& sensor, const long long rays_per_pixel, const bool by_band, F* radiance, u64* n_capped, u64* n_clamped)
{
    RRX_TRY
    typedef ForwardEntries<F> Fw;
    // (the loop calls this file's own trace entry as a caller outside would, like the entries of the forward file)
    constexpr auto trace = [] { if constexpr (sizeof(F) == 8) return rrx_thermal_trace_counts_f64; else return rrx_thermal_trace_counts_f32; }();
    if (check_thermal(m, src, run.max_events, sensor, {"rays_per_pixel", rays_per_pixel}, {{"sensor", sensor.s}},
                      {{"radiance", radiance}, {"n_capped", n_capped}, {"n_clamped", n_clamped}},
                      [&] { if (by_band && m.band_lims_gpt == nullptr) throw std::runtime_error("band_lims_gpt is NULL");
                            if (by_band && m.nbnd < 1) throw std::runtime_error("nbnd must be >= 1: the radiances are kept by band"); },
                      nothing,
                      [&] { if (top_radiance != nullptr) for (int g=0; g<m.ngpt; ++g) check_top_radiance(double(top_radiance[g])); }))
        return 0;

    // the workspace, in u64 words: | counts (npix) | k_null |
    hipStream_t st = static_cast<hipStream_t>(run.stream);
    const size_t npix = size_t(sensor.npx)*sensor.npy;
    const size_t n_kn = words_of(size_t(m.knx)*m.kny*m.knz*sizeof(F));
    const size_t n_out = by_band ? npix*size_t(m.nbnd) : npix;
    WorkspaceLease lease(st);
    u64* counts = lease.get<u64>(npix + n_kn);
    F* k_null = reinterpret_cast<F*>(counts + npix);
    zero_outputs(radiance, n_out, n_capped, n_clamped, st);
    std::vector<int> lims;
    if (by_band)
    {
        lims.resize(2*size_t(m.nbnd));
        if (hipMemcpyAsync(lims.data(), m.band_lims_gpt, lims.size()*sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess
            || hipStreamSynchronize(st) != hipSuccess)
            throw std::runtime_error("copying band_lims_gpt failed");
    }
    const long long nrays = rays_per_pixel*(long long)npix;
    for (int g=0; g<m.ngpt; ++g)
    {
        F* out = radiance;
        if (by_band)
        {
            int band = -1;
            for (int b=m.nbnd-1; b>=0; --b)
                if (g+1 >= lims[2*b] && g+1 <= lims[2*b+1]) band = b;
            if (band < 0) continue;
            out = radiance + npix*size_t(band);
        }
        if (hipMemsetAsync(counts, 0, npix*sizeof(u64), st) != hipSuccess) throw std::runtime_error("zeroing the counts failed");
        forward(Fw::k_null(m.nx, m.ny, m.nz, m.ngpt, m.nbnd, g, m.top_at_1, m.tau, m.band_lims_gpt, m.cld_tau, m.dz, m.knx, m.kny, m.knz,
                           k_null, run.stream));
        forward(trace(m.nx, m.ny, m.nz, m.ngpt, m.nbnd, g, m.top_at_1, m.tau, m.ssa, m.band_lims_gpt, m.cld_tau, m.cld_ssa, m.cld_g,
                      m.dx, m.dy, m.dz, src.sfc_emis, src.lay_src, src.sfc_src, top_radiance != nullptr ? top_radiance[g] : F(0.),
                      m.knx, m.kny, m.knz, k_null, sensor.type, sensor.npx, sensor.npy, sensor.fov, sensor.s, run.seed, 0ll, nrays,
                      run.max_events, counts, n_capped, n_clamped, run.stream));
        forward(Fw::counts_to_flux((long long)npix, counts, F(1.)/F(rays_per_pixel), out, run.stream));
    }
    RRX_CATCH(entry)
}

// ---- the spectral form: rays of all g-points in one launch, counts by band, bands to channels

// rrx_thermal_trace_counts_spectral: top_radiance, sp.photon_end (the ray list's prefix sums) and sp.weight0 are device arrays that the
// entry cannot look into. The kernel stays inside its arrays whatever they hold (the search is bounded by ngpt, a ray beyond the list is
// stepped over, the pixel is taken modulo npix); the callers that form the list on the host refuse one that does not ascend. k_null is
// that of all g-points.
template<typename F>
int thermal_trace_spectral_entry(const char* entry, const Medium<F>& m, const ThermalSources<F>& src, const F* top_radiance, const Run& run,
                                 const Sensor<F>& sensor, const SpecIn<F>& sp, const F* k_null, const long long ray0, const long long nrays,
                                 u64* counts, u64* n_capped, u64* n_clamped)
{
    RRX_TRY
    if (check_thermal(m, src, run.max_events, sensor, {"nrays", nrays},
                      {{"band_lims_gpt", m.band_lims_gpt}, {"ray_end", sp.photon_end}, {"weight0", sp.weight0}, {"k_null", k_null}, {"sensor", sensor.s}},
                      {{"counts", counts}, {"n_capped", n_capped}, {"n_clamped", n_clamped}},
                      [&] { check_spectral_ngpt(m.ngpt);
                            if (m.nbnd < 1) throw std::runtime_error("nbnd must be >= 1: the counts are kept by band");
                            if (ray0 < 0) throw std::runtime_error("ray0 is negative"); }, nothing, nothing))
        return 0;
    launch_trace_thermal_spectral<F>(thermal_args<F>(m, src, F(0.), sensor, 0, k_null, run.seed, u64(ray0), nrays, run.max_events,
                                                     counts, n_capped, n_clamped), sp, top_radiance, static_cast<hipStream_t>(run.stream));
    RRX_CATCH(entry)
}

// rrx_thermal_render_spectral: m_gpt[g] rays per pixel of g-point g (a host array). One trace launch per chunk of consecutive g-points,
// the counts of all chunks added in integers by band and converted once, with the common unit U = n_act / P, through the channel
// matrix. The list, the workspace and the chunk loop are rrx_rt_host.h's; the workspace's late section is top_radiance.
template<typename F>
int thermal_render_spectral_entry(const char* entry, const Medium<F>& m, const ThermalSources<F>& src, const F* top_radiance, const Run& run,
                                  const Sensor<F>& sensor, const long long* m_gpt, const int nchan, const F* chan_weights,
                                  F* radiance, u64* n_capped, u64* n_clamped)
{
    RRX_TRY
    typedef ForwardEntries<F> Fw;
    const long long npix_ll = (long long)sensor.npx*sensor.npy;
    std::vector<long long> ray_end;
    long long P = 0, n_act = 0;
    if (check_thermal(m, src, run.max_events, sensor, {"ngpt", m.ngpt},
                      {{"band_lims_gpt", m.band_lims_gpt}, {"rays_per_pixel_gpt", m_gpt}, {"chan_weights", chan_weights}, {"sensor", sensor.s}},
                      {{"radiance", radiance}, {"n_capped", n_capped}, {"n_clamped", n_clamped}},
                      [&] { check_spectral_ngpt(m.ngpt); check_channels(m.nbnd, nchan); }, nothing,
                      [&] {
                          check_npix(sensor);
                          if (top_radiance != nullptr) for (int g=0; g<m.ngpt; ++g) check_top_radiance(double(top_radiance[g]));
                          ray_list(m.ngpt, npix_ll, m_gpt, ray_end, P, [&](const int g) { if (m_gpt[g] > 0) ++n_act; });
                      }))
        return 0;

    hipStream_t st = static_cast<hipStream_t>(run.stream);
    zero_outputs(radiance, size_t(nchan)*size_t(npix_ll), n_capped, n_clamped, st);
    if (P == 0) return 0;
    const F U = F(n_act) / F(P);
    std::vector<F> weight0(m.ngpt, F(0.));
    for (int g=0; g<m.ngpt; ++g)
        if (m_gpt[g] > 0) weight0[g] = (F(1.) / F(m_gpt[g])) / U;

    SpectralWork<F> w(m, st, size_t(npix_ll), nchan, ray_end, weight0, chan_weights, 0, words_of(size_t(m.ngpt)*sizeof(F)), top_radiance, m.ngpt);
    w.trace(m, run.stream,
            [&](const int g, F* k_null) {
                forward(Fw::k_null(m.nx, m.ny, m.nz, m.ngpt, m.nbnd, g, m.top_at_1, m.tau, m.band_lims_gpt, m.cld_tau, m.dz, m.knx, m.kny, m.knz,
                                   k_null, run.stream)); },
            [&](const SpecIn<F>& sp, const u64 ray0, const long long n) {
                launch_trace_thermal_spectral<F>(thermal_args<F>(m, src, F(0.), sensor, 0, w.k_null, run.seed, ray0, n, run.max_events,
                                                                 w.counts, n_capped, n_clamped), sp, top_radiance != nullptr ? w.late : nullptr, st); });
    forward(Fw::channels(npix_ll, m.nbnd, nchan, w.counts, w.chan, U, radiance, run.stream));
    RRX_CATCH(entry)
}
}  // namespace

// ---- the C entries: each builds the structs and calls its one function
#define TH_P_SCENE(F) \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_emis, const F* lay_src, const F* sfc_src
#define TH_MEDIUM(F) \
        rrx::rt::Medium<F>{nx, ny, nz, ngpt, nbnd, top_at_1, 0, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, dx, dy, dz, nullptr, \
                           knx, kny, knz, rrx::rt::AerIn<F>{}}
#define TH_SOURCES(F) ThermalSources<F>{sfc_emis, lay_src, sfc_src}
#define TH_SENSOR(F) Sensor<F>{sensor_type, npx, npy, fov, sensor}

extern "C"
{
#define RRX_DEFINE_THERMAL(F, SFX) \
int rrx_thermal_trace_counts##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, TH_P_SCENE(F), F top_radiance, \
        int knx, int kny, int knz, const F* k_null, int sensor_type, int npx, int npy, F fov, const F* sensor, \
        unsigned long long seed, long long ray0, long long nrays, int max_events, \
        unsigned long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream) \
{ return thermal_trace_entry<F>("rrx_thermal_trace_counts" #SFX, TH_MEDIUM(F), TH_SOURCES(F), top_radiance, RT_RUN, TH_SENSOR(F), igpt, k_null, \
                                ray0, nrays, counts, n_capped, n_clamped); } \
int rrx_thermal_render##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, TH_P_SCENE(F), const F* top_radiance, \
        int knx, int kny, int knz, int sensor_type, int npx, int npy, F fov, const F* sensor, long long rays_per_pixel, \
        unsigned long long seed, int max_events, RrxBool by_band, F* radiance, unsigned long long* n_capped, unsigned long long* n_clamped, \
        void* stream) \
{ return thermal_render_entry<F>("rrx_thermal_render" #SFX, TH_MEDIUM(F), TH_SOURCES(F), top_radiance, RT_RUN, TH_SENSOR(F), rays_per_pixel, \
                                 by_band != 0, radiance, n_capped, n_clamped); } \
int rrx_thermal_trace_counts_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, TH_P_SCENE(F), const F* top_radiance, \
        const long long* ray_end, const F* weight0, int knx, int kny, int knz, const F* k_null, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, unsigned long long seed, long long ray0, long long nrays, int max_events, \
        unsigned long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream) \
{ return thermal_trace_spectral_entry<F>("rrx_thermal_trace_counts_spectral" #SFX, TH_MEDIUM(F), TH_SOURCES(F), top_radiance, RT_RUN, TH_SENSOR(F), \
                                         SpecIn<F>{ngpt, 0, ray_end, weight0, nullptr}, k_null, ray0, nrays, counts, n_capped, n_clamped); } \
int rrx_thermal_render_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, TH_P_SCENE(F), const F* top_radiance, \
        int knx, int kny, int knz, int sensor_type, int npx, int npy, F fov, const F* sensor, const long long* rays_per_pixel_gpt, \
        unsigned long long seed, int max_events, int nchan, const F* chan_weights, F* radiance, unsigned long long* n_capped, \
        unsigned long long* n_clamped, void* stream) \
{ return thermal_render_spectral_entry<F>("rrx_thermal_render_spectral" #SFX, TH_MEDIUM(F), TH_SOURCES(F), top_radiance, RT_RUN, TH_SENSOR(F), \
                                          rays_per_pixel_gpt, nchan, chan_weights, radiance, n_capped, n_clamped); }

RRX_DEFINE_THERMAL(double, _f64)
RRX_DEFINE_THERMAL(float, _f32)
}
