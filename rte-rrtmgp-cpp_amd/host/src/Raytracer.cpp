// Raytracer_gpu: checks the shapes and forwards to rrx_raytracer_sw; a non-zero status becomes std::runtime_error.
#include "Raytracer.h"
#include "Raytracer_members.h"
#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

namespace
{
typedef std::initializer_list<const Array_gpu<Float,1>*> Arrays1;

// THE SHAPE CHECK of the three trace_rays* methods, who: the prefix of its messages. per_gpt: the sizes of the (ngpt) host arrays, named
// in per_gpt_names; flux: the (nx ny) outputs; with_bg: bg_flux (nx ny) and bg_abs (nbg) and the background's members are checked;
// refuse_bg: the form without the background's outputs, which a background that is set makes an error.
void check_shapes(const std::string& who, const Rt_members& m, const int nx, const int ny, const int nz,
                  const Array_gpu<Float,3>& tau, const Array_gpu<Float,3>& ssa, const Array_gpu<int,2>& band_lims_gpt,
                  const Array_gpu<Float,3>& cld_tau, const Array_gpu<Float,3>& cld_ssa, const Array_gpu<Float,3>& cld_g,
                  const Array_gpu<Float,1>& sfc_albedo, std::initializer_list<int> per_gpt, const std::string& per_gpt_names,
                  Arrays1 flux, const Array_gpu<Float,2>& abs_dir, const Array_gpu<Float,2>& abs_dif,
                  const bool with_bg, Arrays1 bg_flux, Arrays1 bg_abs, const bool refuse_bg)
{
    if (nx < 0 || ny < 0 || nz < 0) throw std::runtime_error(who + "negative extent");
    const long long ncol = (long long)nx*ny;
    const int ngpt = tau.dim(3), nbnd = band_lims_gpt.dim(2);
    if (tau.dim(1) != ncol || tau.dim(2) != nz || ssa.get_dims() != tau.get_dims()) throw std::runtime_error(who + "tau, ssa are not (nx ny, nz, ngpt)");
    const bool cloudy = cld_tau.size() > 0;
    if (cloudy && (cld_tau.dim(1) != ncol || cld_tau.dim(2) != nz || cld_tau.dim(3) != nbnd || cld_ssa.get_dims() != cld_tau.get_dims() ||
                   cld_g.get_dims() != cld_tau.get_dims()))
        throw std::runtime_error(who + "the cloud arrays are not (nx ny, nz, nbnd)");
    if (!cloudy && (cld_ssa.size() > 0 || cld_g.size() > 0)) throw std::runtime_error(who + "the cloud arrays are all empty or all given");
    if (sfc_albedo.size() != ncol || std::any_of(per_gpt.begin(), per_gpt.end(), [&](const int n) { return n != ngpt; }))
        throw std::runtime_error(who + "sfc_albedo is not (nx ny) or " + per_gpt_names + " are not (ngpt)");
    for (const Array_gpu<Float,1>* a : flux)
        if (a->size() != ncol) throw std::runtime_error(who + "a flux array is not (nx ny)");
    for (const Array_gpu<Float,2>* a : {&abs_dir, &abs_dif})
        if (a->dim(1) != ncol || a->dim(2) != nz) throw std::runtime_error(who + "an absorption array is not (nx ny, nz)");
    if (with_bg)
    {
        for (const Array_gpu<Float,1>* a : bg_flux)
            if (a->size() != ncol) throw std::runtime_error(who + "a flux array is not (nx ny)");
        for (const Array_gpu<Float,1>* a : bg_abs)
            if (a->size() != m.nbg()) throw std::runtime_error(who + "a background absorption array is not (nbg)");
        if (m.bg_tau.dim(2) != ngpt) throw std::runtime_error(who + "the background's bg_tau, bg_ssa are not (nbg, ngpt)");
        if (m.bg_cloudy() && m.bg_cld_tau.dim(2) != nbnd) throw std::runtime_error(who + "the background's cloud arrays are not (nbg, nbnd)");
    }
    m.check_table(who, ncol, nz, nbnd);
    if (refuse_bg && m.has_bg) throw std::runtime_error(who + "a background is set: call the form with the background's outputs");
    m.check_aerosol(who, ncol, nz, nbnd);
    m.check_no_bg_aerosol_alone(who);
    m.check_bg_aerosol(who, nbnd);
}
}

// the arguments that the five forward loops begin with
#define RT_LOOP_HEAD(p, photons) \
        nx, ny, nz, tau.dim(3), band_lims_gpt.dim(2), RrxBool(top_at_1), RrxBool(independent_column), tau.ptr(), ssa.ptr(), band_lims_gpt.ptr(), \
        RT_CLOUD(p), dx, dy, dz, sfc_albedo.ptr(), mu0, azimuth, inc_dir.ptr(), inc_dif.ptr(), knx, kny, knz, photons, seed, max_events, \
        sfc_dn_dir.ptr(), sfc_dn_dif.ptr(), sfc_up.ptr(), tod_up.ptr(), abs_dir.ptr(), abs_dif.ptr(), n_capped.ptr()

unsigned long long Raytracer_gpu::trace_rays(
        const int nx, const int ny, const int nz,
        const Float dx, const Float dy, const Float dz,
        const bool top_at_1, const bool independent_column,
        const Array_gpu<Float,3>& tau, const Array_gpu<Float,3>& ssa,
        const Array_gpu<int,2>& band_lims_gpt,
        const Array_gpu<Float,3>& cld_tau, const Array_gpu<Float,3>& cld_ssa, const Array_gpu<Float,3>& cld_g,
        const Array_gpu<Float,1>& sfc_albedo,
        const Float mu0, const Float azimuth,
        const Array<Float,1>& inc_dir, const Array<Float,1>& inc_dif,
        const int knx, const int kny, const int knz,
        const long long photons_per_pixel, const unsigned long long seed, const int max_events,
        Array_gpu<Float,1>& sfc_dn_dir, Array_gpu<Float,1>& sfc_dn_dif, Array_gpu<Float,1>& sfc_up, Array_gpu<Float,1>& tod_up,
        Array_gpu<Float,2>& abs_dir, Array_gpu<Float,2>& abs_dif)
{
    const Rt_members m = RT_MEMBERS;
    check_shapes("Raytracer_gpu::trace_rays: ", m, nx, ny, nz, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_albedo,
                 {inc_dir.size(), inc_dif.size()}, "inc_dir, inc_dif", {&sfc_dn_dir, &sfc_dn_dif, &sfc_up, &tod_up}, abs_dir, abs_dif,
                 false, {}, {}, true);
    const Rt_pointers p(m, cld_tau, cld_ssa, cld_g);
    Array_gpu<unsigned long long,1> n_capped({1});
    Float* no_out = nullptr;
    // (rrx_raytracer_sw_aer takes each triple as a host array of its three device pointers; there is no background here)
    const Float* const* no_triple = nullptr;
    if (has_aer)
        RRX_CALL(rrx_raytracer_sw_aer, RT_LOOP_HEAD(p, photons_per_pixel), no_out, no_out, no_out, no_out, no_out, RT_TABLE(p), RT_BACKGROUND(p),
                 p.aer, no_triple);
    else if (has_table)
        RRX_CALL(rrx_raytracer_sw_phase, RT_LOOP_HEAD(p, photons_per_pixel), RT_TABLE(p));
    else
        RRX_CALL(rrx_raytracer_sw, RT_LOOP_HEAD(p, photons_per_pixel));
    return n_capped({1});
}

unsigned long long Raytracer_gpu::trace_rays(
        const int nx, const int ny, const int nz,
        const Float dx, const Float dy, const Float dz,
        const bool top_at_1, const bool independent_column,
        const Array_gpu<Float,3>& tau, const Array_gpu<Float,3>& ssa,
        const Array_gpu<int,2>& band_lims_gpt,
        const Array_gpu<Float,3>& cld_tau, const Array_gpu<Float,3>& cld_ssa, const Array_gpu<Float,3>& cld_g,
        const Array_gpu<Float,1>& sfc_albedo,
        const Float mu0, const Float azimuth,
        const Array<Float,1>& inc_dir, const Array<Float,1>& inc_dif,
        const int knx, const int kny, const int knz,
        const long long photons_per_pixel, const unsigned long long seed, const int max_events,
        Array_gpu<Float,1>& sfc_dn_dir, Array_gpu<Float,1>& sfc_dn_dif, Array_gpu<Float,1>& sfc_up, Array_gpu<Float,1>& tod_up,
        Array_gpu<Float,2>& abs_dir, Array_gpu<Float,2>& abs_dif,
        Array_gpu<Float,1>& toa_up, Array_gpu<Float,1>& tod_dn_dir, Array_gpu<Float,1>& tod_dn_dif,
        Array_gpu<Float,1>& bg_abs_dir, Array_gpu<Float,1>& bg_abs_dif)
{
    if (!has_bg) throw std::runtime_error("Raytracer_gpu::trace_rays: no background is set (set_background)");
    const Rt_members m = RT_MEMBERS;
    check_shapes("Raytracer_gpu::trace_rays: ", m, nx, ny, nz, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_albedo,
                 {inc_dir.size(), inc_dif.size()}, "inc_dir, inc_dif",
                 {&sfc_dn_dir, &sfc_dn_dif, &sfc_up, &tod_up, &toa_up, &tod_dn_dir, &tod_dn_dif}, abs_dir, abs_dif,
                 true, {}, {&bg_abs_dir, &bg_abs_dif}, false);
    const Rt_pointers p(m, cld_tau, cld_ssa, cld_g);
    Array_gpu<unsigned long long,1> n_capped({1});
    if (has_aer)
        RRX_CALL(rrx_raytracer_sw_aer, RT_LOOP_HEAD(p, photons_per_pixel), toa_up.ptr(), tod_dn_dir.ptr(), tod_dn_dif.ptr(), bg_abs_dir.ptr(),
                 bg_abs_dif.ptr(), RT_TABLE(p), RT_BACKGROUND(p), p.aer, p.bg_aer);
    else
        RRX_CALL(rrx_raytracer_sw_bg, RT_LOOP_HEAD(p, photons_per_pixel), toa_up.ptr(), tod_dn_dir.ptr(), tod_dn_dif.ptr(), bg_abs_dir.ptr(),
                 bg_abs_dif.ptr(), RT_TABLE(p), RT_BACKGROUND(p));
    return n_capped({1});
}

unsigned long long Raytracer_gpu::trace_rays_spectral(
        const int nx, const int ny, const int nz,
        const Float dx, const Float dy, const Float dz,
        const bool top_at_1, const bool independent_column,
        const Array_gpu<Float,3>& tau, const Array_gpu<Float,3>& ssa,
        const Array_gpu<int,2>& band_lims_gpt,
        const Array_gpu<Float,3>& cld_tau, const Array_gpu<Float,3>& cld_ssa, const Array_gpu<Float,3>& cld_g,
        const Array_gpu<Float,1>& sfc_albedo,
        const Float mu0, const Float azimuth,
        const Array<Float,1>& inc_dir, const Array<Float,1>& inc_dif,
        const int knx, const int kny, const int knz,
        const Array<long long,1>& photons_per_pixel_gpt, const unsigned long long seed, const int max_events,
        Array_gpu<Float,1>& sfc_dn_dir, Array_gpu<Float,1>& sfc_dn_dif, Array_gpu<Float,1>& sfc_up, Array_gpu<Float,1>& tod_up,
        Array_gpu<Float,2>& abs_dir, Array_gpu<Float,2>& abs_dif,
        Array_gpu<Float,1>& toa_up, Array_gpu<Float,1>& tod_dn_dir, Array_gpu<Float,1>& tod_dn_dif,
        Array_gpu<Float,1>& bg_abs_dir, Array_gpu<Float,1>& bg_abs_dif)
{
    const Rt_members m = RT_MEMBERS;
    check_shapes("Raytracer_gpu::trace_rays_spectral: ", m, nx, ny, nz, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_albedo,
                 {inc_dir.size(), inc_dif.size(), photons_per_pixel_gpt.size()}, "inc_dir, inc_dif, photons_per_pixel_gpt",
                 {&sfc_dn_dir, &sfc_dn_dif, &sfc_up, &tod_up}, abs_dir, abs_dif,
                 has_bg, {&toa_up, &tod_dn_dir, &tod_dn_dif}, {&bg_abs_dir, &bg_abs_dif}, false);
    const Rt_pointers p(m, cld_tau, cld_ssa, cld_g);
    Array_gpu<unsigned long long,1> n_capped({1});
    Float* no_out = nullptr;
    RRX_CALL(rrx_raytracer_sw_spectral, RT_LOOP_HEAD(p, photons_per_pixel_gpt.ptr()),
             has_bg ? toa_up.ptr() : no_out, has_bg ? tod_dn_dir.ptr() : no_out, has_bg ? tod_dn_dif.ptr() : no_out,
             has_bg ? bg_abs_dir.ptr() : no_out, has_bg ? bg_abs_dif.ptr() : no_out, RT_TABLE(p), RT_BACKGROUND(p), p.aer, p.bg_aer);
    return n_capped({1});
}

// The allocation of pipeline.spectral_allocation, operation for operation in double: the floor takes out the g-points whose
// proportional share of what the others leave is below it, the rest is dealt by largest remainders, ties to the lower g.
Array<long long,1> Raytracer_gpu::spectral_allocation(const Array<Float,1>& inc_in, const long long P, const long long floor_)
{
    const std::string who = "Raytracer_gpu::spectral_allocation: ";
    const int ngpt = inc_in.size();
    std::vector<double> inc(ngpt);
    for (int g=0; g<ngpt; ++g)
    {
        inc[g] = double(inc_in({g+1}));
        if (!(inc[g] >= 0.) || !std::isfinite(inc[g])) throw std::runtime_error(who + "inc must be finite and >= 0");
    }
    if (floor_ < 0) throw std::runtime_error(who + "min_per_gpt must be >= 0");
    std::vector<char> active(ngpt), free_(ngpt);
    long long n_active = 0;
    for (int g=0; g<ngpt; ++g) { active[g] = inc[g] > 0.; free_[g] = active[g]; n_active += active[g]; }
    if (P < 0 || P < floor_*n_active || (P > 0 && n_active == 0))
        throw std::runtime_error(who + "P = " + std::to_string(P) + " photons per pixel cannot give " + std::to_string(floor_) + " to each of "
                                 + std::to_string(n_active) + " active g-points");
    std::vector<long long> m(ngpt);
    for (int g=0; g<ngpt; ++g) m[g] = active[g] ? floor_ : 0;
    const auto rest_and_total = [&](long long& rest, double& total, bool& any)
    {
        rest = P; total = 0.; any = false;
        for (int g=0; g<ngpt; ++g) { if (free_[g]) { total += inc[g]; any = true; } else rest -= m[g]; }
    };
    long long rest; double total; bool any;
    for (;;)
    {
        rest_and_total(rest, total, any);
        if (!any || total <= 0.) break;
        bool bound = false;
        for (int g=0; g<ngpt; ++g)
            if (free_[g] && double(rest)*(inc[g]/total) < double(floor_)) { free_[g] = 0; bound = true; }
        if (!bound) break;
    }
    rest_and_total(rest, total, any);
    std::vector<int> order(ngpt);
    std::iota(order.begin(), order.end(), 0);
    if (any)
    {
        std::vector<double> remainder(ngpt, -1.);
        long long left = rest;
        for (int g=0; g<ngpt; ++g)
            if (free_[g])
            {
                const double quota = double(rest)*(inc[g]/total);
                m[g] = (long long)std::floor(quota);
                remainder[g] = quota - double(m[g]);
                left -= m[g];
            }
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return remainder[a] > remainder[b]; });
        for (long long i=0; i<left; ++i) m[order[i]] += 1;
    }
    // (the floor never binds everywhere: the shares of the free g-points add up to what is left, which is at least their floors)
    Array<long long,1> out({ngpt});
    for (int g=0; g<ngpt; ++g) out({g+1}) = m[g];
    return out;
}

void Raytracer_gpu::set_background(const Array<Float,1>& dz_in, const Array_gpu<Float,2>& tau_in, const Array_gpu<Float,2>& ssa_in,
                                   const Array_gpu<Float,2>& ctau_in, const Array_gpu<Float,2>& cssa_in, const Array_gpu<Float,2>& cg_in)
{
    const int nbg = dz_in.size();
    if (nbg < 1 || tau_in.dim(1) != nbg || ssa_in.get_dims() != tau_in.get_dims())
        throw std::runtime_error("Raytracer_gpu::set_background: dz_bg is not (nbg >= 1) or bg_tau, bg_ssa are not (nbg, ngpt)");
    const bool cloudy = ctau_in.size() > 0;
    if (cloudy ? (ctau_in.dim(1) != nbg || cssa_in.get_dims() != ctau_in.get_dims() || cg_in.get_dims() != ctau_in.get_dims())
               : (cssa_in.size() > 0 || cg_in.size() > 0))
        throw std::runtime_error("Raytracer_gpu::set_background: the background's cloud arrays are all empty or all (nbg, nbnd)");
    dz_bg = dz_in; bg_tau = tau_in; bg_ssa = ssa_in; bg_cld_tau = ctau_in; bg_cld_ssa = cssa_in; bg_cld_g = cg_in;
    has_bg = true;
}


void Raytracer_gpu::set_aerosol(const Array_gpu<Float,3>& tau_in, const Array_gpu<Float,3>& ssa_in, const Array_gpu<Float,3>& g_in,
                        const Array_gpu<Float,2>& btau_in, const Array_gpu<Float,2>& bssa_in, const Array_gpu<Float,2>& bg_in)
{
    const bool grid = tau_in.size() > 0, aloft = btau_in.size() > 0;
    if (grid ? (ssa_in.get_dims() != tau_in.get_dims() || g_in.get_dims() != tau_in.get_dims()) : (ssa_in.size() > 0 || g_in.size() > 0))
        throw std::runtime_error("Raytracer_gpu::set_aerosol: the aerosol arrays are all empty or all (nx ny, nz, nbnd)");
    if (aloft ? (bssa_in.get_dims() != btau_in.get_dims() || bg_in.get_dims() != btau_in.get_dims()) : (bssa_in.size() > 0 || bg_in.size() > 0))
        throw std::runtime_error("Raytracer_gpu::set_aerosol: the background's aerosol arrays are all empty or all (nbg, nbnd)");
    if (aloft && !has_bg) throw std::runtime_error("Raytracer_gpu::set_aerosol: a background aerosol needs a background (set_background)");
    if (aloft && btau_in.dim(1) != dz_bg.size())
        throw std::runtime_error("Raytracer_gpu::set_aerosol: the background's aerosol arrays are not (nbg, nbnd)");
    aer_tau = tau_in; aer_ssa = ssa_in; aer_g = g_in; bg_aer_tau = btau_in; bg_aer_ssa = bssa_in; bg_aer_g = bg_in;
    has_aer = grid || aloft;
}

void Raytracer_gpu::set_phase_table(const Array_gpu<Float,1>& mu_in, const Array_gpu<Float,3>& phase_in, const Array_gpu<Float,3>& cdf_in,
                            const Float re0_in, const Float dre_in, const Array_gpu<Float,2>& cld_re_in)
{
    if (mu_in.size() < 2 || phase_in.dim(1) != mu_in.size() || cdf_in.get_dims() != phase_in.get_dims())
        throw std::runtime_error("Raytracer_gpu::set_phase_table: mu is not (nmu >= 2) or phase, cdf are not (nmu, nre, nbnd)");
    if (cld_re_in.size() == 0) throw std::runtime_error("Raytracer_gpu::set_phase_table: cld_re is empty");
    mu = mu_in; phase = phase_in; cdf = cdf_in; cld_re = cld_re_in; re0 = re0_in; dre = dre_in;
    has_table = true;
}
