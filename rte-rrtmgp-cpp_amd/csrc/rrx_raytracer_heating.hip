// 3-D longwave heating from cell sensors in the thermal ray tracer: the net radiative power that every cell of the grid
// takes up, per unit horizontal area, by the emission-reciprocity estimator. The tracking is trace_thermal_kernel's
// (rrx_raytracer_thermal.hip), operation for operation: null-collision tracking on the k_null grid with integer block
// indices, a pending free path across a face, periodic x / y, fine_cell, f_no_abs, roulette below 0.5, the scatter-or-null draw and the
// species draw, scatter_direction and lambert, max_events and n_capped. The kernel states its start and its tracking itself, as the
// three other trace kernels do. It differs from the thermal kernel in the start, the lane's reference state, the deposits and the tally.
//
// THE ESTIMATOR. For one g-point a cell with absorption optical depth tau_abs = tau (1 - ssa) + cld_tau (1 - cld_ssa) and the
// cell-constant source B0 takes up C = integral over the cell of k_abs integral over 4 pi of (L - B0) = 4 pi tau_abs (<L> - B0) W m-2,
// <L> the radiance averaged over uniformly distributed points of the cell and isotropic directions: what the thermal tracer estimates
// for rays that start that way. Every deposit is scored as a difference, w (S - B0) s0 with s0 = 4 pi tau_abs: the variance is that of
// the difference, a cell whose rays die inside it gets a clean zero, and a black-body cavity gives 0 in integers.
//
// START. With ncell = nx ny nz, ray r belongs to cell c = r mod ncell: i = c mod nx, j = (c / nx) mod ny, k = c / (nx ny), the height
// index (0 at the surface), lay = top_at_1 ? nz-1-k : k. THE LANE'S REFERENCE is read once from that cell, cell0 = i + j nx + ncol lay:
// B0 = lay_src[cell0, g], s0 = F(4 pi) ((t (1 - w0)) + (tc (1 - wc))), under SPECTRAL then multiplied by weight0[g]. A cell with s0 == 0
// ends its ray at once, with no events and no deposit. DRAW ORDER (tests/raytracer_heating_ref.py restates it):
//   start:     u -> x = (i + u) dx;  u -> y = (j + u) dy;  u -> z = (k + u) dz;  u -> uz = 1 - 2u;  u -> phi = 2 pi u,
//              ux = sqrt(max(0, 1 - uz^2)) cos phi, uy likewise with sin phi; the block (in, jn, kn) and the clamps of the thermal start
//   each event: as in trace_thermal_kernel
// Philox4x32-10, key = seed, counter (ray low, ray high, igpt | 0x40000000, block): the one two-bit prefix that no other tracer uses.
//
// DEPOSITS, each made before the weight changes, all signed:
//   - at a collision in a cell:  d = (weight (1 - f_no_abs)) ((lay_src[cell, g] - B0) s0);   then weight *= f_no_abs
//   - at a surface hit:          d = (weight sfc_emis[col]) ((sfc_src[col, g] - B0) s0);     then weight *= 1 - sfc_emis[col]
//   - where the ray leaves through the top:  d = weight ((top_radiance[g] - B0) s0)
//
// TALLY. One signed 64-bit count per cell in units of 2^-32 W m-2. A deposit is rounded by itself, llrint(clamp(d, -2^20, 2^20) 2^32) (a
// clamped one is counted in n_clamped); the rounded deposits are summed in the lane in a 64-bit integer, and ONE integer atomic adds the
// sum into counts[cell0] when the ray ends, for any reason (the roulette, the top, max_events, a ray that no face stops; the last two
// also count in n_capped). Bit-reproducible, independent of the order of arrival, additive over ray ranges. Consecutive lanes own
// consecutive cells, so the atomics of a wave do not collide.
//
// SPECTRAL (trace_heating_kernel<F,true>): the rays of all g-points in one launch, as in DESIGN 4.24. The list is the concatenation in
// g-point order of m_g ncell rays; ray p of the list is ray q = p - ray_end[g] of the per-g-point launch of g, draw for draw. The g-point
// is read back from word 2 of the ray's Philox counter (c2 & 0x3FFFFFFF). All g-points add into the same ncell counts: the result is
// broadband; the band table only finds the cloud triple, and a g-point that lies in no band has no cloud and is still tallied.
// top_radiance is a device array here, NULL = 0; a.igpt and a.top_radiance are not read.
//
// LIMITS: those of the thermal tracer (no background, no aerosol, no phase table, a cell-constant source), and no heating by band.
#include "rrx_rt_host.h"

namespace
{
using namespace rrx;
using namespace rrx::rt;

template<typename F>
struct HeatingArgs
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
    long long* counts; u64* n_capped; u64* n_clamped;
};

// what the spectral form takes beside HeatingArgs: the ray list and the weights (SpecIn; dif_frac is not read) and the top radiance of
// every g-point on the device (NULL: 0); empty in the per-g-point form
template<typename F, bool SPECTRAL> struct HeatingSpecArgs {};
template<typename F> struct HeatingSpecArgs<F,true> { SpecIn<F> sp; const F* top_radiance; };

template<typename F, bool SPECTRAL>
__global__ void __launch_bounds__(RT_BLOCK) trace_heating_kernel(const HeatingArgs<F> a, const HeatingSpecArgs<F,SPECTRAL> s)
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
    const auto top_source = [&]() {
        if constexpr (SPECTRAL) return s.top_radiance != nullptr ? s.top_radiance[gpt()] : F(0.);
        else return a.top_radiance;
    };
    // the slices of the lane's g-point and the band of its cloud (SPECTRAL: derived where they are read)
    const auto slices = [&]() {
        if constexpr (SPECTRAL)
        {
            ibnd = a.cld_tau != nullptr ? sv.band[gpt()] : -1;
            tau_g = a.tau + ncol*nz*gpt();
            ssa_g = a.ssa != nullptr ? a.ssa + ncol*nz*gpt() : nullptr;
            lay_src_g = a.lay_src + ncol*nz*gpt();
        }
    };

    bool alive = false, pending = false;
    int in = 0, jn = 0, kn = 0, nev = 0, cell0 = 0;
    F x = F(0.), y = F(0.), z = F(0.), ux = F(0.), uy = F(0.), uz = F(-1.), weight = F(0.), tau = F(0.);
    F B0 = F(0.), s0 = F(0.);          // the lane's reference: the source and 4 pi tau_abs of its ray's own cell
    long long sum = 0;                 // the rounded deposits of the lane's ray

    // a deposit d of the lane's ray: clamped at +-2^20, rounded by itself and added to the lane's sum
    const auto deposit = [&](const F d) {
        const bool clamped = fabs(d) > F(1048576.);
        if (clamped) atomicAdd(a.n_clamped, 1ull);
        sum += llrint(double(clamped ? copysign(F(1048576.), d) : d) * 4294967296.0);
    };

    // One loop with one back edge: a pass is one event of the lane's ray; a lane whose ray has ended adds its sum into its cell and takes
    // its next ray in the same pass
    for (;;)
    {
        if (!alive)
        {
            if (sum != 0) { atomicAdd(reinterpret_cast<u64*>(a.counts) + cell0, u64(sum)); sum = 0; }
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
            rng.start(r, unsigned(igpt) | 0x40000000u);
            const int c = int(r % u64(ncol*nz));
            const int i = c % nx, j = (c / nx) % ny, k = c / (nx*ny);
            cell0 = i + j*nx + int(ncol)*(a.top_at_1 ? nz-1-k : k);
            slices();
            {
                const F t = tau_g[cell0], w0 = ssa_g != nullptr ? ssa_g[cell0] : F(0.);
                F tc = F(0.), wc = F(0.);
                if (ibnd >= 0)
                {
                    const size_t cb = size_t(cell0) + ncol*nz*ibnd;
                    tc = a.cld_tau[cb]; wc = a.cld_ssa[cb];
                }
                B0 = lay_src_g[cell0];
                s0 = F(12.566370614359172)*((t*(F(1.) - w0)) + (tc*(F(1.) - wc)));
                if constexpr (SPECTRAL) s0 = s0*s.sp.weight0[gpt()];
            }
            if (s0 == F(0.)) continue;          // the cell absorbs nothing: no events, no deposit
            const F sx = (F(i) + rng.next<F>())*a.dx;
            const F sy = (F(j) + rng.next<F>())*a.dy;
            const F sz = (F(k) + rng.next<F>())*a.dz;
            uz = F(1.) - F(2.)*rng.next<F>();
            const F phi = F(6.283185307179586)*rng.next<F>();
            const F st = sqrt(max(F(0.), F(1.) - uz*uz));
            ux = st*cos(phi); uy = st*sin(phi);
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
                if (kn == a.knz - 1) { deposit(weight*((top_source() - B0)*s0)); alive = false; }          // out through the domain top
                else { ++kn; z = F(kn)*kdz; }
            }
            else if (kn == 0)                 // the surface: it emits, and reflects the rest
            {
                z = F(0.);
                const int col = fine_cell(x, a.dx, in, rx) + nx*fine_cell(y, a.dy, jn, ry);
                const F emis = a.sfc_emis[col];
                if constexpr (SPECTRAL) sfc_src_g = a.sfc_src + ncol*gpt();
                deposit((weight*emis)*((sfc_src_g[col] - B0)*s0));
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
            slices();
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
            deposit((weight*(F(1.) - f_no_abs))*((lay_src_g[cell] - B0)*s0));
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

// flux_conv[cell] = F(counts[cell] 2^-32) scale: the conversion of the signed counts, once per render
template<typename F>
__global__ void heating_counts_to_flux_kernel(const size_t n, const long long* __restrict__ counts, const F scale, F* __restrict__ out)
{
    const size_t i = size_t(blockIdx.x)*blockDim.x + threadIdx.x;
    if (i < n) out[i] = F(double(counts[i]) * 2.3283064365386963e-10) * scale;
}

// ---- host side (rrx_rt_host.h): the scene structs and the one check sequence of the tracers, which is told what this
// tracer needs of the medium (tau and the sources; ssa may be NULL), that it has no sun and that it has no sensor.

// the surface and the sources
template<typename F> struct HeatingSources { const F* sfc_emis; const F* lay_src; const F* sfc_src; };

inline void check_top_radiance(const double v)
{
    if (!std::isfinite(v) || v < 0.) throw std::runtime_error("top_radiance must be finite and >= 0");
}

// the checks of the heating entries: check_entry with the entry's one extent of work and no sensor
template<typename F, typename A, typename B, typename C>
bool check_heating(const Medium<F>& m, const HeatingSources<F>& src, const int max_events, std::pair<const char*, long long> work,
                   Needed inputs, Needed outputs, A after_nbnd, B after_phase, C after_scene)
{
    const Sun<F>* no_sun = nullptr;
    return check_entry(m, {{"tau", m.tau}, {"sfc_emis", src.sfc_emis}, {"lay_src", src.lay_src}, {"sfc_src", src.sfc_src}}, no_sun, PhaseIn<F>{},
                       RT_NO_BG(F), max_events, {work}, inputs, outputs, after_nbnd, after_phase, after_scene, nothing);
}

// THE BUILDER of the kernel arguments
template<typename F>
HeatingArgs<F> heating_args(const Medium<F>& m, const HeatingSources<F>& src, const F top_radiance, const int igpt, const F* k_null,
                            const u64 seed, const u64 ray0, const long long nrays, const int max_events,
                            long long* counts, u64* n_capped, u64* n_clamped)
{
    HeatingArgs<F> a{};
    set_medium(a, m, igpt, k_null, max_events);
    set_key(a, seed);
    a.sfc_emis = src.sfc_emis; a.lay_src = src.lay_src; a.sfc_src = src.sfc_src; a.top_radiance = top_radiance;
    a.ray0 = ray0; a.nrays = nrays;
    a.counts = counts; a.n_capped = n_capped; a.n_clamped = n_clamped;
    return a;
}

template<typename F>
void launch_trace_heating(const HeatingArgs<F>& a, hipStream_t st)
{
    const int blocks = int(std::min<long long>((a.nrays + RT_BLOCK - 1) / RT_BLOCK, max_blocks()));
    trace_heating_kernel<F,false><<<blocks, RT_BLOCK, 0, st>>>(a, HeatingSpecArgs<F,false>{});
}

// the spectral form: a.ray0 / a.nrays are a range of the concatenated list sp.photon_end, a.k_null holds the slices from g-point
// sp.kn_g0 on, top_radiance is a device array (ngpt) or NULL
template<typename F>
void launch_trace_heating_spectral(const HeatingArgs<F>& a, const SpecIn<F>& sp, const F* top_radiance, hipStream_t st)
{
    const int blocks = int(std::min<long long>((a.nrays + RT_BLOCK - 1) / RT_BLOCK, max_blocks()));
    trace_heating_kernel<F,true><<<blocks, RT_BLOCK, spectral_lds_bytes(sp.ngpt, 0, sizeof(F)), st>>>(a, HeatingSpecArgs<F,true>{sp, top_radiance});
}

// rrx_heating3d_counts
template<typename F>
int heating_counts_entry(const char* entry, const Medium<F>& m, const HeatingSources<F>& src, const F top_radiance, const Run& run,
                         const int igpt, const F* k_null, const long long ray0, const long long nrays,
                         long long* counts, u64* n_capped, u64* n_clamped)
{
    RRX_TRY
    if (check_heating(m, src, run.max_events, {"nrays", nrays}, {{"k_null", k_null}},
                      {{"counts", counts}, {"n_capped", n_capped}, {"n_clamped", n_clamped}},
                      [&] { if (ray0 < 0) throw std::runtime_error("ray0 is negative"); }, [&] { check_igpt(igpt, m.ngpt); },
                      [&] { check_top_radiance(double(top_radiance)); }))
        return 0;
    launch_trace_heating<F>(heating_args<F>(m, src, top_radiance, igpt, k_null, run.seed, u64(ray0), nrays, run.max_events,
                                            counts, n_capped, n_clamped), static_cast<hipStream_t>(run.stream));
    RRX_CATCH(entry)
}

// rrx_heating3d_counts_spectral: top_radiance, sp.photon_end (the ray list's prefix sums) and sp.weight0 are device arrays that
// the entry cannot look into. The kernel stays inside its arrays whatever they hold (the search is bounded by ngpt, a ray beyond the
// list is stepped over, the cell is taken modulo ncell); the callers that form the list on the host refuse one that does not ascend.
// k_null is that of all g-points.
template<typename F>
int heating_counts_spectral_entry(const char* entry, const Medium<F>& m, const HeatingSources<F>& src, const F* top_radiance, const Run& run,
                                  const SpecIn<F>& sp, const F* k_null, const long long ray0, const long long nrays,
                                  long long* counts, u64* n_capped, u64* n_clamped)
{
    RRX_TRY
    if (check_heating(m, src, run.max_events, {"nrays", nrays},
                      {{"band_lims_gpt", m.band_lims_gpt}, {"ray_end", sp.photon_end}, {"weight0", sp.weight0}, {"k_null", k_null}},
                      {{"counts", counts}, {"n_capped", n_capped}, {"n_clamped", n_clamped}},
                      [&] { check_spectral_ngpt(m.ngpt);
                            if (ray0 < 0) throw std::runtime_error("ray0 is negative"); }, nothing, nothing))
        return 0;
    launch_trace_heating_spectral<F>(heating_args<F>(m, src, F(0.), 0, k_null, run.seed, u64(ray0), nrays, run.max_events,
                                                     counts, n_capped, n_clamped), sp, top_radiance, static_cast<hipStream_t>(run.stream));
    RRX_CATCH(entry)
}

// rrx_heating3d_render: m_gpt[g] rays per cell of g-point g (a host array). One trace launch per chunk of consecutive g-points
// that has rays, all chunks into the same ncell counts, converted once with the common unit U = n_act / P. The ray list is
// rrx_rt_host.h's; the workspace, in u64 words: | counts (ncell) | k_null of a chunk | ray_end | weight0 | top_radiance |.
template<typename F>
int heating_render_entry(const char* entry, const Medium<F>& m, const HeatingSources<F>& src, const F* top_radiance, const Run& run,
                         const long long* m_gpt, F* flux_conv, u64* n_capped, u64* n_clamped)
{
    RRX_TRY
    typedef ForwardEntries<F> Fw;
    const long long ncell_ll = (long long)m.nx*m.ny*m.nz;
    std::vector<long long> ray_end;
    long long P = 0, n_act = 0;
    if (check_heating(m, src, run.max_events, {"ngpt", m.ngpt},
                      {{"band_lims_gpt", m.band_lims_gpt}, {"rays_per_cell_gpt", m_gpt}},
                      {{"flux_conv", flux_conv}, {"n_capped", n_capped}, {"n_clamped", n_clamped}},
                      [&] { check_spectral_ngpt(m.ngpt); }, nothing,
                      [&] {
                          if (top_radiance != nullptr) for (int g=0; g<m.ngpt; ++g) check_top_radiance(double(top_radiance[g]));
                          ray_list(m.ngpt, ncell_ll, m_gpt, ray_end, P, [&](const int g) {
                              if (m_gpt[g] < 0) throw std::runtime_error("rays_per_cell_gpt is negative at g-point " + std::to_string(g));
                              if (m_gpt[g] > 0) ++n_act; });
                      }))
        return 0;

    hipStream_t st = static_cast<hipStream_t>(run.stream);
    const size_t ncell = size_t(ncell_ll);
    zero_outputs(flux_conv, ncell, n_capped, n_clamped, st);
    if (P == 0) return 0;
    const F U = F(n_act) / F(P);
    std::vector<F> weight0(m.ngpt, F(0.));
    for (int g=0; g<m.ngpt; ++g)
        if (m_gpt[g] > 0) weight0[g] = (F(1.) / F(m_gpt[g])) / U;

    const size_t nkn = size_t(m.knx)*m.kny*m.knz;
    const int chunk = spectral_gpt_per_launch(nkn*sizeof(F), m.ngpt);
    const size_t n_kn = words_of(nkn*size_t(chunk)*sizeof(F)), n_re = size_t(m.ngpt) + 1, n_w = words_of(size_t(m.ngpt)*sizeof(F));
    WorkspaceLease lease(st);
    u64* work = lease.get<u64>(ncell + n_kn + n_re + 2*n_w);
    long long* counts = reinterpret_cast<long long*>(work);
    F* k_null = reinterpret_cast<F*>(work + ncell);
    long long* ray_end_dev = reinterpret_cast<long long*>(work + ncell + n_kn);
    F* weight0_dev = reinterpret_cast<F*>(work + ncell + n_kn + n_re);
    F* top_dev = reinterpret_cast<F*>(work + ncell + n_kn + n_re + n_w);
    // (the host arrays end with the call: it waits for its stream once)
    const bool ok = hipMemsetAsync(counts, 0, ncell*sizeof(long long), st) == hipSuccess
      && hipMemcpyAsync(ray_end_dev, ray_end.data(), ray_end.size()*sizeof(long long), hipMemcpyHostToDevice, st) == hipSuccess
      && hipMemcpyAsync(weight0_dev, weight0.data(), size_t(m.ngpt)*sizeof(F), hipMemcpyHostToDevice, st) == hipSuccess
      && (top_radiance == nullptr || hipMemcpyAsync(top_dev, top_radiance, size_t(m.ngpt)*sizeof(F), hipMemcpyHostToDevice, st) == hipSuccess)
      && hipStreamSynchronize(st) == hipSuccess;
    if (!ok) throw std::runtime_error("zeroing the counts or copying the ray list failed");

    for (int g0=0; g0<m.ngpt; g0+=chunk)
    {
        const int g1 = std::min(g0 + chunk, m.ngpt);
        const long long n = ray_end[g1] - ray_end[g0];
        if (n == 0) continue;
        if (chunk == m.ngpt)
            forward(Fw::k_null_all(m.nx, m.ny, m.nz, m.ngpt, m.nbnd, m.top_at_1, m.tau, m.band_lims_gpt, m.cld_tau, m.dz, m.knx, m.kny, m.knz,
                                   k_null, nullptr, run.stream));
        else
            for (int g=g0; g<g1; ++g)
                if (ray_end[g+1] > ray_end[g])
                    forward(Fw::k_null(m.nx, m.ny, m.nz, m.ngpt, m.nbnd, g, m.top_at_1, m.tau, m.band_lims_gpt, m.cld_tau, m.dz, m.knx, m.kny, m.knz,
                                       k_null + nkn*size_t(g - g0), run.stream));
        launch_trace_heating_spectral<F>(heating_args<F>(m, src, F(0.), 0, k_null, run.seed, u64(ray_end[g0]), n, run.max_events,
                                                         counts, n_capped, n_clamped),
                                         SpecIn<F>{m.ngpt, g0, ray_end_dev, weight0_dev, nullptr}, top_radiance != nullptr ? top_dev : nullptr, st);
    }
    heating_counts_to_flux_kernel<F><<<unsigned(ceil_div(ncell_ll, 256)), 256, 0, st>>>(ncell, counts, U, flux_conv);
    RRX_CATCH(entry)
}
}  // namespace

// ---- the C entries: each builds the structs and calls its one function
#define HT_P_SCENE(F) \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_emis, const F* lay_src, const F* sfc_src
#define HT_MEDIUM(F) \
        rrx::rt::Medium<F>{nx, ny, nz, ngpt, nbnd, top_at_1, 0, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, dx, dy, dz, nullptr, \
                           knx, kny, knz, rrx::rt::AerIn<F>{}}
#define HT_SOURCES(F) HeatingSources<F>{sfc_emis, lay_src, sfc_src}

extern "C"
{
#define RRX_DEFINE_HEATING(F, SFX) \
int rrx_heating3d_counts##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, HT_P_SCENE(F), F top_radiance, \
        int knx, int kny, int knz, const F* k_null, unsigned long long seed, long long ray0, long long nrays, int max_events, \
        long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream) \
{ return heating_counts_entry<F>("rrx_heating3d_counts" #SFX, HT_MEDIUM(F), HT_SOURCES(F), top_radiance, RT_RUN, igpt, k_null, \
                                 ray0, nrays, counts, n_capped, n_clamped); } \
int rrx_heating3d_counts_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, HT_P_SCENE(F), const F* top_radiance, \
        const long long* ray_end, const F* weight0, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long ray0, long long nrays, int max_events, \
        long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream) \
{ return heating_counts_spectral_entry<F>("rrx_heating3d_counts_spectral" #SFX, HT_MEDIUM(F), HT_SOURCES(F), top_radiance, RT_RUN, \
                                          SpecIn<F>{ngpt, 0, ray_end, weight0, nullptr}, k_null, ray0, nrays, counts, n_capped, n_clamped); } \
int rrx_heating3d_render##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, HT_P_SCENE(F), const F* top_radiance, \
        int knx, int kny, int knz, const long long* rays_per_cell_gpt, unsigned long long seed, int max_events, \
        F* flux_conv, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream) \
{ return heating_render_entry<F>("rrx_heating3d_render" #SFX, HT_MEDIUM(F), HT_SOURCES(F), top_radiance, RT_RUN, \
                                 rays_per_cell_gpt, flux_conv, n_capped, n_clamped); }

RRX_DEFINE_HEATING(double, _f64)
RRX_DEFINE_HEATING(float, _f32)
}
