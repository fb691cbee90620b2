// The host side that the two Monte Carlo ray tracers share: what an entry is given, as plain structs that the extern "C"
// wrappers fill once per call, the one sequence of argument checks that every trace entry and loop of both tracers runs, and the
// parameter groups of those wrappers. Nothing here reaches a kernel: the kernel arguments (TraceArgs, BwArgs, FwBg, BgArgs, SpecIn)
// stay in the tracers' own files.
#ifndef RRX_RT_HOST_H
#define RRX_RT_HOST_H

#include "rrx_rt_phase.h"
#include "rrx_hip.h"

namespace rrx
{
namespace rt
{
// the grid medium; independent_column: the forward tracer's switch; aer: the grid's aerosol triple (NULLs in the entries without one)
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

// THE CHECKS of a trace entry or a loop, of either tracer, in the order that is part of their behaviour (tests/
// test_raytracer_refusal_order.py holds it). An entry's own checks run at the places they have always had: its extents behind the
// grid's, after_nbnd (check_spectral_ngpt, photon0 / ray0), its inputs and outputs behind tau, ssa, sfc_albedo, after_phase (igpt),
// after_scene (the inc_* loops, the photon list), after_grid (npx npy, check_sensor). What an entry checks of its background follows
// (background_of, loop_background). true: an extent is zero and there is nothing to do.
template<typename F, typename A, typename B, typename C, typename D>
bool check_entry(const Medium<F>& m, const Sun<F>& sun, const PhaseIn<F>& ph, const Background<F>& bg, const int max_events,
                 Extents extents, Needed inputs, Needed outputs, A after_nbnd, B after_phase, C after_scene, D after_grid)
{
    check_nbg(bg.nbg);
    const bool no_grid = check_extents({{"nx", m.nx}, {"ny", m.ny}, {"nz", m.nz}, {"ngpt", m.ngpt}});
    const bool no_work = check_extents(extents);
    if (no_grid || no_work) return true;
    if (m.nbnd < 0) throw std::runtime_error("nbnd is negative");
    after_nbnd();
    check_needed({{"tau", m.tau}, {"ssa", m.ssa}, {"sfc_albedo", m.sfc_albedo}});
    check_needed(inputs);
    check_needed(outputs);
    check_cloud(m.nbnd, m.band_lims_gpt, m.cld_tau, m.cld_ssa, m.cld_g);
    if (bg.form == FORM_AER) check_aerosol("aer_", m.nbnd, m.band_lims_gpt, m.aer.tau, m.aer.ssa, m.aer.g);
    check_phase(ph, m.cld_tau);
    after_phase();
    check_scene(m.dx, m.dy, m.dz, sun.mu0);
    after_scene();
    if (max_events < 1) throw std::runtime_error("max_events must be >= 1");
    check_grid(m.nx, m.ny, m.nz, m.knx, m.kny, m.knz);
    after_grid();
    return false;
}

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

// the sun's direction and the Philox key of a launch, into the kernel arguments of either tracer
template<typename Args, typename F>
void set_sun_and_key(Args& a, const Sun<F>& sun, const u64 seed)
{
    const double st_ = std::sqrt(std::max(0.0, 1.0 - double(sun.mu0)*double(sun.mu0)));
    a.sun_x = F(st_*std::cos(double(sun.azimuth))); a.sun_y = F(st_*std::sin(double(sun.azimuth))); a.sun_z = -sun.mu0;
    a.k0 = unsigned(seed & 0xFFFFFFFFull); a.k1 = unsigned(seed >> 32);
}

template<typename F, typename Args>
void set_medium(Args& a, const Medium<F>& m, const int igpt, const F* k_null, const int max_events)
{
    a.nx = m.nx; a.ny = m.ny; a.nz = m.nz; a.nbnd = m.nbnd; a.igpt = igpt; a.top_at_1 = m.top_at_1 ? 1 : 0;
    a.tau = m.tau; a.ssa = m.ssa; a.band_lims_gpt = m.band_lims_gpt; a.cld_tau = m.cld_tau; a.cld_ssa = m.cld_ssa; a.cld_g = m.cld_g;
    a.dx = m.dx; a.dy = m.dy; a.dz = m.dz; a.sfc_albedo = m.sfc_albedo; a.knx = m.knx; a.kny = m.kny; a.knz = m.knz; a.k_null = k_null;
    a.max_events = max_events;
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
