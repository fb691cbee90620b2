// The host side that the three Monte Carlo ray tracers share: what an entry is given, as plain structs that the extern "C"
// wrappers fill once per call, the one sequence of argument checks that every trace entry and loop of the tracers runs, the sensor of
// the backward and the thermal tracer, the ray list and the workspace of their spectral loops, and the parameter groups of those
// wrappers. Nothing here reaches a kernel: the kernel arguments (TraceArgs, BwArgs, ThermalArgs, FwBg, BgArgs, SpecIn) stay in the
// tracers' own files.
#ifndef RRX_RT_HOST_H
#define RRX_RT_HOST_H

#include "rrx_rt_phase.h"
#include "rrx_hip.h"

namespace rrx
{
namespace rt
{
// the grid medium; independent_column: the forward tracer's switch; sfc_albedo: the solar tracers' surface (NULL in the thermal one,
// whose surface is in its ThermalSources); aer: the grid's aerosol triple (NULLs in the entries without one)
template<typename F>
struct Medium
{
    int nx, ny, nz, ngpt, nbnd;
    RrxBool top_at_1, independent_column;
    const F* tau; const F* ssa; const int* band_lims_gpt; const F* cld_tau; const F* cld_ssa; const F* cld_g;
    F dx, dy, dz;
    const F* sfc_albedo;
    int knx, kny, knz;
    AerIn<F> aer;
};

template<typename F> struct Sun { F mu0, azimuth; };

// the virtual camera of the backward and the thermal tracer: s is (12,): position, w, h, e_d
template<typename F> struct Sensor { int type, npx, npy; F fov; const F* s; };

struct Run { u64 seed; int max_events; void* stream; };

// The generation of an entry, which is also the kernel form it asks for: the plain and _phase entries have no background argument
// (the instantiations without the BG flag), the _bg entries no aerosol argument, the _aer and _spectral entries both. FORM_SPECTRAL
// is a launcher's alone (launch_trace_bw): an entry of the spectral form is checked as FORM_AER, on which the form is built.
enum Form { FORM_GRID = 0, FORM_BG = 1, FORM_AER = 2, FORM_SPECTRAL = 3 };

// The optional background. profile: the single-g-point entries, what rrx_rt_bg_profile* wrote; the medium (tau .. aer): the loops.
// With nbg = 0 nothing but nbg is read.
template<typename F>
struct Background
{
    Form form;
    int nbg;
    const F* dz_bg;
    const F* profile;
    const F* tau; const F* ssa; const F* cld_tau; const F* cld_ssa; const F* cld_g;
    AerIn<F> aer;
};

// a host array of three device pointers (tau, ssa, g); a NULL array is a triple of NULLs
template<typename F> AerIn<F> aer_of(const F* const* three)
{
    return three != nullptr ? AerIn<F>{three[0], three[1], three[2]} : AerIn<F>{};
}

typedef std::initializer_list<std::pair<const char*, long long>> Extents;
typedef std::initializer_list<std::pair<const char*, const void*>> Needed;
inline void nothing() {}

// THE CHECKS of a trace entry or a loop, of any tracer, in the order that is part of their behaviour (tests/
// test_raytracer_refusal_order.py holds it). needed: what the tracer reads of the medium whatever the entry (the solar ones: tau, ssa,
// sfc_albedo; the thermal one: tau and its sources); sun: NULL for a tracer without one. An entry's own checks run at the places they
// have always had: its extents behind the grid's, after_nbnd (check_spectral_ngpt, photon0 / ray0), its inputs and outputs behind the
// needed ones, after_phase (igpt), after_scene (the inc_* loops, top_radiance, the photon or ray list), after_grid (check_sensor,
// walk_bound). What an entry checks of its background follows (background_of, loop_background). true: an extent is zero and there is
// nothing to do.
template<typename F, typename A, typename B, typename C, typename D>
bool check_entry(const Medium<F>& m, Needed needed, const Sun<F>* sun, const PhaseIn<F>& ph, const Background<F>& bg, const int max_events,
                 Extents extents, Needed inputs, Needed outputs, A after_nbnd, B after_phase, C after_scene, D after_grid)
{
    check_nbg(bg.nbg);
    const bool no_grid = check_extents({{"nx", m.nx}, {"ny", m.ny}, {"nz", m.nz}, {"ngpt", m.ngpt}});
    const bool no_work = check_extents(extents);
    if (no_grid || no_work) return true;
    if (m.nbnd < 0) throw std::runtime_error("nbnd is negative");
    after_nbnd();
    check_needed(needed);
    check_needed(inputs);
    check_needed(outputs);
    check_cloud(m.nbnd, m.band_lims_gpt, m.cld_tau, m.cld_ssa, m.cld_g);
    if (bg.form == FORM_AER) check_aerosol("aer_", m.nbnd, m.band_lims_gpt, m.aer.tau, m.aer.ssa, m.aer.g);
    check_phase(ph, m.cld_tau);
    after_phase();
    check_scene(m.dx, m.dy, m.dz, sun != nullptr ? &sun->mu0 : nullptr);
    after_scene();
    if (max_events < 1) throw std::runtime_error("max_events must be >= 1");
    check_grid(m.nx, m.ny, m.nz, m.knx, m.kny, m.knz);
    after_grid();
    return false;
}

// what the solar tracers need of the medium
#define RT_NEEDED_SOLAR(m) {{"tau", (m).tau}, {"ssa", (m).ssa}, {"sfc_albedo", (m).sfc_albedo}}

inline void check_igpt(const int igpt, const int ngpt)
{
    if (igpt < 0 || igpt >= ngpt) throw std::runtime_error("igpt is outside [0, ngpt)");
}

// the background of a single-g-point entry as the kernels take it (check_outputs: the forward tracer's five tallies)
template<typename F, typename O>
BgIn<F> background_of(const Background<F>& bg, const Medium<F>& m, O check_outputs)
{
    BgIn<F> in{bg.nbg, bg.profile, BgLevels<F>{}};
    if (bg.nbg > 0)
    {
        check_needed({{"dz_bg", bg.dz_bg}, {"bg_profile", bg.profile}});
        check_outputs();
        in.z = bg_levels<F>(bg.nbg, bg.dz_bg, m.nz, m.knz, m.dz);
    }
    return in;
}

// The form a single-g-point entry runs: the aerosol form whenever an _aer entry has a triple in the grid or a background (whose profile
// then has BG_ROWS_AER rows); with nbg = 0 and a NULL triple it is the _bg entry.
template<typename F> Form form_of(const Background<F>& bg, const Medium<F>& m)
{
    return (bg.form == FORM_AER && !(m.aer.tau != nullptr || bg.nbg > 0)) ? FORM_BG : bg.form;
}

// The background of a loop. on: there are layers; nbg: their number, 0 when off; form: what the loop's launches run, the aerosol form
// when either triple is given (the background's is not looked at when nbg = 0); aer: the background's triple, NULLs when off.
template<typename F>
struct LoopBg
{
    bool on;
    int nbg;
    Form form;
    AerIn<F> aer;
    BgLevels<F> lev;
};

template<typename F, typename O>
LoopBg<F> loop_background(const Background<F>& bg, const Medium<F>& m, O check_outputs)
{
    LoopBg<F> b{bg.form != FORM_GRID && bg.nbg > 0, 0, bg.form, AerIn<F>{}, BgLevels<F>{}};
    if (b.on && bg.form == FORM_AER)
    {
        check_aerosol("bg_aer_", m.nbnd, m.band_lims_gpt, bg.aer.tau, bg.aer.ssa, bg.aer.g);
        b.aer = bg.aer;
    }
    if (bg.form == FORM_AER && m.aer.tau == nullptr && b.aer.tau == nullptr) b.form = FORM_BG;
    if (b.on)
    {
        b.nbg = bg.nbg;
        check_bg_medium(bg.nbg, m.nbnd, bg.dz_bg, bg.tau, bg.ssa, m.band_lims_gpt, bg.cld_tau, bg.cld_ssa, bg.cld_g);
        check_outputs();
        b.lev =bg_levels<F>(bg.nbg, bg.dz_bg, m.nz, m.knz, m.dz);
    }
    return b;
}

// ---- into the kernel arguments of any tracer: the Philox key of a launch, the sun's direction, the medium (the surface is the
// tracer's own: a.sfc_albedo, or the thermal sources), the sensor
template<typename Args>
void set_key(Args& a, const u64 seed)
{
    a.k0 = unsigned(seed & 0xFFFFFFFFull); a.k1 = unsigned(seed >> 32);
}

template<typename Args, typename F>
void set_sun_and_key(Args& a, const Sun<F>& sun, const u64 seed)
{
    const double st_ = std::sqrt(std::max(0.0, 1.0 - double(sun.mu0)*double(sun.mu0)));
    a.sun_x = F(st_*std::cos(double(sun.azimuth))); a.sun_y = F(st_*std::sin(double(sun.azimuth))); a.sun_z = -sun.mu0;
    set_key(a, seed);
}

template<typename F, typename Args>
void set_medium(Args& a, const Medium<F>& m, const int igpt, const F* k_null, const int max_events)
{
    a.nx = m.nx; a.ny = m.ny; a.nz = m.nz; a.nbnd = m.nbnd; a.igpt = igpt; a.top_at_1 = m.top_at_1 ? 1 : 0;
    a.tau = m.tau; a.ssa = m.ssa; a.band_lims_gpt = m.band_lims_gpt; a.cld_tau = m.cld_tau; a.cld_ssa = m.cld_ssa; a.cld_g = m.cld_g;
    a.dx = m.dx; a.dy = m.dy; a.dz = m.dz; a.knx = m.knx; a.kny = m.kny; a.knz = m.knz; a.k_null = k_null;
    a.max_events = max_events;
}

template<typename F, typename Args>
void set_sensor(Args& a, const Sensor<F>& sensor)
{
    const F* s = sensor.s;
    a.type = sensor.type; a.npx = sensor.npx; a.npy = sensor.npy; a.fov = sensor.fov;
    a.px = s[0]; a.py = s[1]; a.pz = s[2]; a.wx = s[3]; a.wy = s[4]; a.wz = s[5]; a.hx = s[6]; a.hy = s[7]; a.hz = s[8];
    a.ex = s[9]; a.ey = s[10]; a.ez = s[11];
}

// ---- the sensor's checks

// (the spectral loops make it ahead of their ray list as well)
template<typename F>
void check_npix(const Sensor<F>& sensor)
{
    if ((long long)sensor.npx*sensor.npy > 0x7FFFFFFFll) throw std::runtime_error("npx npy exceeds 2^31 - 1");
}

// what the backward and the thermal entries refuse of a sensor: its geometry
template<typename F>
void check_sensor(const Sensor<F>& sensor)
{
    const int type = sensor.type;
    const F fov = sensor.fov;
    const F* s = sensor.s;
    check_npix(sensor);
    if (type < 0 || type > 3) throw std::runtime_error("sensor_type must be 0 (perspective), 1 (fisheye), 2 (orthographic) or 3 (flux sensor)");
    for (int i=0; i<12; ++i)
        if (!std::isfinite(double(s[i]))) throw std::runtime_error("sensor holds a number that is not finite");
    const double ex = s[9], ey = s[10], ez = s[11];
    const double len = std::sqrt(ex*ex + ey*ey + ez*ez);
    if (type == 0 || type == 1)
    {
        if (!(len > 0.)) throw std::runtime_error("sensor e_d is zero");
        if (s[2] < F(0.)) throw std::runtime_error("sensor position lies below the surface");
    }
    if (type == 1 && (!(fov > F(0.)) || double(fov) > 6.283185307179586 + 1e-6)) throw std::runtime_error("fov must be in (0, 2 pi] for a fisheye sensor");
    if (type == 2 && (std::fabs(len - 1.) > 1.e-5 || !(ez < 0.))) throw std::runtime_error("sensor e_d must be a unit vector with e_d.z < 0 for an orthographic sensor");
    if (type == 3 && ez == 0.) throw std::runtime_error("sensor e_d.z must be > 0 (at the surface, facing up) or < 0 (at the top, facing down) for a flux sensor");
}

// the bound of the walk to the sun: nz + ceil(H tan / dx) + ceil(H tan / dy) + 2
template<typename F>
int walk_bound(const Medium<F>& m, const F mu0)
{
    const double tn = std::sqrt(std::max(0., 1. - double(mu0)*double(mu0))) / double(mu0), height = double(m.nz)*double(m.dz);
    const double bound = double(m.nz) + std::ceil(height*tn/double(m.dx)) + std::ceil(height*tn/double(m.dy)) + 2.;
    if (!(bound < 2.0e9)) throw std::runtime_error("mu0 is too small for this domain: the walk to the sun would take more than 2e9 cells");
    return int(bound);
}

// ---- all g-points in one launch
inline void check_spectral_ngpt(const int ngpt)
{
    if (ngpt > RT_SPECTRAL_MAX_GPT) throw std::runtime_error("ngpt must be <= 1024 in the spectral form");
}

// g-points per trace launch of rrx_raytracer_sw_spectral and rrx_camera_render_spectral: the largest chunk whose k_null fits 1 GiB, or
// RRX_RT_SPECTRAL_GPT_PER_LAUNCH from the environment, read at every call. The result does not depend on it.
inline int spectral_gpt_per_launch(const size_t k_null_bytes_per_gpt, const int ngpt)
{
    if (const char* e = std::getenv("RRX_RT_SPECTRAL_GPT_PER_LAUNCH")) { const int n = std::atoi(e); if (n >= 1) return std::min(n, ngpt); }
    const size_t fit = (size_t(1) << 30) / std::max<size_t>(k_null_bytes_per_gpt, 1);
    return int(std::min<size_t>(std::max<size_t>(fit, 1), size_t(ngpt)));
}

inline size_t words_of(const size_t bytes) { return (bytes + sizeof(u64) - 1) / sizeof(u64); }

// ---- what the loops of the backward and the thermal tracer are made of

// The small entries of the forward and the backward file that the loops call, by precision. They are called as a caller outside would:
// their own checks run again and a refusal comes back with its text.
template<typename F> struct ForwardEntries;
template<> struct ForwardEntries<double>
{
    static constexpr auto k_null = rrx_rt_k_null_f64; static constexpr auto k_null_aer = rrx_rt_k_null_aer_f64;
    static constexpr auto bg_profile = rrx_rt_bg_profile_f64; static constexpr auto bg_profile_aer = rrx_rt_bg_profile_aer_f64;
    static constexpr auto counts_to_flux = rrx_rt_counts_to_flux_f64;
    static constexpr auto k_null_all = rrx_rt_k_null_all_f64; static constexpr auto bg_profile_all = rrx_rt_bg_profile_all_f64;
    static constexpr auto channels = rrx_camera_channels_f64;
};
template<> struct ForwardEntries<float>
{
    static constexpr auto k_null = rrx_rt_k_null_f32; static constexpr auto k_null_aer = rrx_rt_k_null_aer_f32;
    static constexpr auto bg_profile = rrx_rt_bg_profile_f32; static constexpr auto bg_profile_aer = rrx_rt_bg_profile_aer_f32;
    static constexpr auto counts_to_flux = rrx_rt_counts_to_flux_f32;
    static constexpr auto k_null_all = rrx_rt_k_null_all_f32; static constexpr auto bg_profile_all = rrx_rt_bg_profile_all_f32;
    static constexpr auto channels = rrx_camera_channels_f32;
};
inline void forward(const int status) { if (status != 0) throw std::runtime_error(rrx_last_error()); }

// what a loop zeroes before anything else: the radiance (n numbers) and the two tallies
template<typename F>
void zero_outputs(F* radiance, const size_t n, u64* n_capped, u64* n_clamped, hipStream_t st)
{
    bool ok = hipMemsetAsync(n_capped, 0, sizeof(u64), st) == hipSuccess;
    ok = ok && hipMemsetAsync(n_clamped, 0, sizeof(u64), st) == hipSuccess;
    ok = ok && hipMemsetAsync(radiance, 0, n*sizeof(F), st) == hipSuccess;
    if (!ok) throw std::runtime_error("zeroing the outputs failed");
}

inline void check_channels(const int nbnd, const int nchan)
{
    if (nbnd < 1) throw std::runtime_error("nbnd must be >= 1: the counts are kept by band");
    if (nchan < 1) throw std::runtime_error("nchan must be >= 1");
}

// THE RAY LIST of a spectral loop: ray_end, the prefix sums of m_gpt[g] npix rays, and P = sum m_gpt. before(g): what the caller checks
// of g-point g ahead of its rays.
template<typename B>
void ray_list(const int ngpt, const long long npix, const long long* m_gpt, std::vector<long long>& ray_end, long long& P, B before)
{
    ray_end.assign(size_t(ngpt) + 1, 0);
    for (int g=0; g<ngpt; ++g)
    {
        before(g);
        if (m_gpt[g] < 0) throw std::runtime_error("rays_per_pixel_gpt is negative at g-point " + std::to_string(g));
        if (m_gpt[g] > (0x7FFFFFFFFFFFFFFFll - ray_end[g]) / npix) throw std::runtime_error("the ray list exceeds 2^63 - 1");
        ray_end[g+1] = ray_end[g] + m_gpt[g]*npix;
        P += m_gpt[g];
    }
}

// THE WORKSPACE of a spectral loop, in u64 words:
//   | counts (nbnd, npix) | k_null of a chunk | mid | ray_end | weight0 | late | the channel matrix |
// mid (n_mid words) and late (n_late words) are the caller's: the camera's profile of all g-points, the thermal tracer's top_radiance.
// The constructor zeroes the counts, copies ray_end, weight0, the channel matrix and late_host (n_late_host numbers; NULL: none) and
// waits for the stream once: the host arrays end with the call.
template<typename F>
struct SpectralWork
{
    WorkspaceLease lease;
    const std::vector<long long>& ray_end_host;
    size_t nkn;
    int chunk;
    u64* counts; F* k_null; F* mid; long long* ray_end; F* weight0; F* late; F* chan;

    SpectralWork(const Medium<F>& m, hipStream_t st, const size_t npix, const int nchan, const std::vector<long long>& list,
                 const std::vector<F>& weight0_host, const F* chan_weights, const size_t n_mid, const size_t n_late, const F* late_host,
                 const size_t n_late_host)
        : lease(st), ray_end_host(list), nkn(size_t(m.knx)*m.kny*m.knz), chunk(spectral_gpt_per_launch(nkn*sizeof(F), m.ngpt))
    {
        const size_t n_counts = size_t(m.nbnd)*npix, n_kn = words_of(nkn*size_t(chunk)*sizeof(F));
        const size_t n_re = size_t(m.ngpt) + 1, n_w = words_of(size_t(m.ngpt)*sizeof(F)), n_cw = words_of(size_t(nchan)*m.nbnd*sizeof(F));
        counts = lease.get<u64>(n_counts + n_kn + n_mid + n_re + n_w + n_late + n_cw);
        k_null = reinterpret_cast<F*>(counts + n_counts);
        mid = reinterpret_cast<F*>(counts + n_counts + n_kn);
        ray_end = reinterpret_cast<long long*>(counts + n_counts + n_kn + n_mid);
        weight0 = reinterpret_cast<F*>(counts + n_counts + n_kn + n_mid + n_re);
        late = reinterpret_cast<F*>(counts + n_counts + n_kn + n_mid + n_re + n_w);
        chan = reinterpret_cast<F*>(counts + n_counts + n_kn + n_mid + n_re + n_w + n_late);
        const bool ok = hipMemsetAsync(counts, 0, n_counts*sizeof(u64), st) == hipSuccess
          && hipMemcpyAsync(ray_end, ray_end_host.data(), ray_end_host.size()*sizeof(long long), hipMemcpyHostToDevice, st) == hipSuccess
          && hipMemcpyAsync(weight0, weight0_host.data(), size_t(m.ngpt)*sizeof(F), hipMemcpyHostToDevice, st) == hipSuccess
          && (late_host == nullptr || hipMemcpyAsync(late, late_host, n_late_host*sizeof(F), hipMemcpyHostToDevice, st) == hipSuccess)
          && hipMemcpyAsync(chan, chan_weights, size_t(nchan)*m.nbnd*sizeof(F), hipMemcpyHostToDevice, st) == hipSuccess
          && hipStreamSynchronize(st) == hipSuccess;
        if (!ok) throw std::runtime_error("zeroing the counts or copying the ray list failed");
    }

    // THE CHUNK LOOP: one trace launch per chunk of consecutive g-points that has rays. k_null of the chunk's g-points comes from
    // rrx_rt_k_null_all when the chunk is the whole list, otherwise slice by slice (the same bits) from k_null_slice(g, out), the
    // caller's entry for one g-point; launch(sp, ray0, n) traces the rays [ray0, ray0 + n) of the list on this->k_null into this->counts.
    template<typename K, typename L>
    void trace(const Medium<F>& m, void* stream, K k_null_slice, L launch)
    {
        for (int g0=0; g0<m.ngpt; g0+=chunk)
        {
            const int g1 = std::min(g0 + chunk, m.ngpt);
            const long long n = ray_end_host[g1] - ray_end_host[g0];
            if (n == 0) continue;
            if (chunk == m.ngpt)
                forward(ForwardEntries<F>::k_null_all(m.nx, m.ny, m.nz, m.ngpt, m.nbnd, m.top_at_1, m.tau, m.band_lims_gpt, m.cld_tau, m.dz,
                                                      m.knx, m.kny, m.knz, k_null, m.aer.tau, stream));
            else
                for (int g=g0; g<g1; ++g)
                    if (ray_end_host[g+1] > ray_end_host[g]) k_null_slice(g, k_null + nkn*size_t(g - g0));
            launch(SpecIn<F>{m.ngpt, g0, ray_end, weight0, nullptr}, u64(ray_end_host[g0]), n);
        }
    }
};
}  // namespace rt
}  // namespace rrx

// ---- the parameter groups of the extern "C" wrappers (include/rrx_hip.h declares every entry in full) and the structs made of them
#define RT_P_GRID(F) \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth
#define RT_P_PHASE(F) int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re
#define RT_P_BG(F) int nbg, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g
#define RT_MEDIUM(F, INDEPENDENT_COLUMN, AER) \
        rrx::rt::Medium<F>{nx, ny, nz, ngpt, nbnd, top_at_1, INDEPENDENT_COLUMN, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, \
                           dx, dy, dz, sfc_albedo, knx, kny, knz, AER}
#define RT_SUN(F) rrx::rt::Sun<F>{mu0, azimuth}
#define RT_RUN rrx::rt::Run{seed, max_events, stream}
#define RT_PHASE(F) rrx::rt::PhaseIn<F>{nmu, nre, re0, dre, mu, phase, cdf, cld_re}
#define RT_NO_BG(F) rrx::rt::Background<F>{rrx::rt::FORM_GRID, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rrx::rt::AerIn<F>{}}
#define RT_BG_PROFILE(F, FORM) \
        rrx::rt::Background<F>{FORM, nbg, dz_bg, bg_profile, nullptr, nullptr, nullptr, nullptr, nullptr, rrx::rt::AerIn<F>{}}
#define RT_BG_MEDIUM(F, FORM, AER) \
        rrx::rt::Background<F>{FORM, nbg, dz_bg, nullptr, bg_tau, bg_ssa, bg_cld_tau, bg_cld_ssa, bg_cld_g, AER}

#endif
