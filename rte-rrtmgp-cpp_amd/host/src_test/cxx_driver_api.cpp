// C entry points around Radiation_solver_longwave / _shortwave for a foreign host (bench.py --driver cxx, tests): the reference's
// class structure -- Gas_concs_gpu, Gas_optics_rrtmgp_gpu, Cloud_optics_gpu, Rte_lw_gpu / Rte_sw_gpu, Fluxes_broadband_gpu inside
// solve_gpu (include_test/Radiation_solver.h = /root/reference/include_test/Radiation_solver.h:33-235) -- driven on device arrays the
// caller owns. Coefficients come from the files the reference's driver reads (coefficients_lw.nc, ...); the atmosphere is handed
// over as device pointers in the Array layout (column index fastest). Nothing here synchronises: rrx_cxx_driver_solve enqueues one
// LW + SW solve on the given stream and returns.
#include <memory>
#include <string>
#include "Radiation_solver.h"
#include "Raytracer.h"
#include "Raytracer_bw.h"
#include "Raytracer_thermal.h"
#include "rrx_cxx_driver.h"

namespace
{
    thread_local std::string g_error;

    struct Driver
    {
        std::unique_ptr<Radiation_solver_longwave> lw;
        std::unique_ptr<Radiation_solver_shortwave> sw;
        Gas_concs_gpu gases;
        bool clouds = false;
        int ncol = 0, nlay = 0;
        // broadband outputs of the last solve, (ncol, nlay+1) each: LW up, dn, net; SW up, dn, dn_dir, net
        Array_gpu<Float,2> lw_up, lw_dn, lw_net, sw_up, sw_dn, sw_dir, sw_net;
        Array_gpu<Float,2> cloud_frac, overlap_param;        // views of the caller's McICA fields (rrx_cxx_cloud_sampling)
        Array_gpu<Float,2> alt_lay; Array_gpu<Float,1> ref_alt;   // views of the caller's altitudes (rrx_cxx_spherical_mu0)
    };

    template<typename Fn> int guarded(Fn&& f)
    {
        try { f(); return 0; }
        catch (const std::exception& e) { g_error = e.what(); return 1; }
    }
    Array_gpu<Float,2> view2(const Float* p, const int n1, const int n2) { return p ? Array_gpu<Float,2>(const_cast<Float*>(p), {n1, n2}) : Array_gpu<Float,2>(); }
    Array_gpu<Float,1> view1(const Float* p, const int n1) { return p ? Array_gpu<Float,1>(const_cast<Float*>(p), {n1}) : Array_gpu<Float,1>(); }
}

extern "C"
{
const char* rrx_cxx_driver_error() { return g_error.c_str(); }

// gas_names: the gases the caller will provide (rrx_cxx_driver_set_gas), needed when the k-distributions are loaded
void* rrx_cxx_driver_create(const char* dir, const int ngas, const char* const* gas_names, const int clouds, const int top_at_1)
{
    Driver* d = nullptr;
    const int rc = guarded([&]
    {
        const std::string base = std::string(dir) + "/";
        std::unique_ptr<Driver> drv = std::make_unique<Driver>();
        Gas_concs host_gases;                                       // (names only: availability is what the constructors look at)
        for (int i=0; i<ngas; ++i) host_gases.set_vmr(gas_names[i], Float(0.));
        drv->gases = Gas_concs_gpu(host_gases);
        drv->clouds = clouds != 0;
        drv->lw = std::make_unique<Radiation_solver_longwave>(drv->gases, base + "coefficients_lw.nc", clouds ? base + "cloud_coefficients_lw.nc" : std::string());
        drv->sw = std::make_unique<Radiation_solver_shortwave>(drv->gases, clouds != 0, false, base + "coefficients_sw.nc",
                                                               clouds ? base + "cloud_coefficients_sw.nc" : std::string(), std::string());
        drv->lw->set_vertical_ordering(top_at_1); drv->sw->set_vertical_ordering(top_at_1);       // stated: no read-backs inside solve_gpu
        d = drv.release();
    });
    return rc == 0 ? d : nullptr;
}

void rrx_cxx_driver_destroy(void* h) { delete static_cast<Driver*>(h); }

// vmr: device pointer to a (n1, n2) array in the Array layout: (1,1) scalar, (1,nlay) profile or (ncol,nlay) field; the values are COPIED (call again when they change)
int rrx_cxx_driver_set_gas(void* h, const char* name, const Float* vmr, const int n1, const int n2)
{
    return guarded([&] { static_cast<Driver*>(h)->gases.set_vmr(name, view2(vmr, n1, n2)); });
}

int rrx_cxx_driver_settings(void* h, const int column_block, const int broadband, const int sort_mode, const int pad)
{
    return guarded([&]
    {
        Driver& d = *static_cast<Driver*>(h);
        d.lw->set_column_block(column_block); d.sw->set_column_block(column_block);
        d.lw->set_broadband_solvers(broadband != 0); d.sw->set_broadband_solvers(broadband != 0);
        d.lw->set_column_sorting(sort_mode); d.sw->set_column_sorting(sort_mode);
        d.lw->set_column_padding(pad != 0); d.sw->set_column_padding(pad != 0);
    });
}

int rrx_cxx_sunlit_columns(void* h, const int sunlit)
{
    return guarded([&] { static_cast<Driver*>(h)->sw->set_sunlit_columns(sunlit != 0); });
}

int rrx_cxx_lw_gauss_angles(void* h, const int n)
{
    return guarded([&] { static_cast<Driver*>(h)->lw->set_gauss_angles(n); });
}

int rrx_cxx_lw_scattering(void* h, const int on)
{
    return guarded([&] { static_cast<Driver*>(h)->lw->set_lw_scattering(on != 0); });
}

int rrx_cxx_lw_rescaling(void* h, const int on)
{
    return guarded([&] { static_cast<Driver*>(h)->lw->set_lw_rescaling(on != 0); });
}

int rrx_cxx_lw_optimal_angles(void* h, const int on)
{
    return guarded([&] { static_cast<Driver*>(h)->lw->set_optimal_angles(on != 0); });
}

int rrx_cxx_lw_jacobian(void* h, const int on)
{
    return guarded([&] { static_cast<Driver*>(h)->lw->set_jacobian(on != 0); });
}

int rrx_cxx_cloud_sampling(void* h, const Float* cloud_frac, const int ncol, const int nlay, const int overlap, const Float* overlap_param,
                           const unsigned long long seed, const int col_offset)
{
    return guarded([&]
    {
        Driver& d = *static_cast<Driver*>(h);
        d.cloud_frac = view2(cloud_frac, ncol, nlay);
        d.overlap_param = view2(overlap_param, ncol, nlay-1);
        const Array_gpu<Float,2>* f = cloud_frac ? &d.cloud_frac : nullptr;
        const Array_gpu<Float,2>* a = overlap_param ? &d.overlap_param : nullptr;
        d.lw->set_cloud_sampling(f, overlap, a, seed, col_offset);
        d.sw->set_cloud_sampling(f, overlap, a, seed, col_offset);
    });
}

int rrx_cxx_spherical_mu0(void* h, const Float* alt_lay, const int ncol, const int nlay, const Float* ref_alt, const double planet_radius)
{
    return guarded([&]
    {
        Driver& d = *static_cast<Driver*>(h);
        d.alt_lay = view2(alt_lay, ncol, nlay);
        d.ref_alt = view1(ref_alt, ncol);
        d.sw->set_spherical_mu0(alt_lay ? &d.alt_lay : nullptr, ref_alt ? &d.ref_alt : nullptr, Float(planet_radius));
    });
}

// the (ncol, nlay+1) surface-temperature Jacobian of the LW upward flux of the last solve, copied to `out` on `stream`
int rrx_cxx_lw_flux_up_jac(void* h, Float* out, void* stream)
{
    return guarded([&]
    {
        const Array_gpu<Float,2>& j = static_cast<Driver*>(h)->lw->get_lw_flux_up_jac();
        if (j.size() == 0) throw std::runtime_error("rrx_cxx_lw_flux_up_jac: no Jacobian (rrx_cxx_lw_jacobian, then a solve)");
        rrx_host::check(rrx_memcpy_d2d(out, j.ptr(), (unsigned long long)j.size()*sizeof(Float), stream));
    });
}

// One LW + SW solve (fluxes only) on `stream`. Arrays: (ncol,nlay) / (ncol,nlay+1) fields, (ncol) vectors, surface properties (nbnd,ncol);
// lwp, iwp, rel, dei may be NULL without clouds. out7: seven device arrays (ncol, nlay+1) for LW up, dn, net and SW up, dn, dn_dir, net,
// or NULL: the driver keeps them (rrx_cxx_driver_fluxes).
int rrx_cxx_driver_solve(void* h, const int ncol, const int nlay, const int nbnd_lw, const int nbnd_sw,
        const Float* p_lay, const Float* p_lev, const Float* t_lay, const Float* t_lev, const Float* t_sfc,
        const Float* emis_sfc, const Float* sfc_alb_dir, const Float* sfc_alb_dif, const Float* tsi_scaling, const Float* mu0,
        const Float* lwp, const Float* iwp, const Float* rel, const Float* dei, Float* const* out7, void* stream)
{
    return guarded([&]
    {
        Driver& d = *static_cast<Driver*>(h);
        rrx_host::set_stream(stream);
        const int nlev = nlay + 1;
        Array_gpu<Float,2>* outs[7] = {&d.lw_up, &d.lw_dn, &d.lw_net, &d.sw_up, &d.sw_dn, &d.sw_dir, &d.sw_net};
        if (out7 != nullptr)                      // the caller's seven (ncol, nlay+1) arrays: the solvers write there
        {
            for (int i=0; i<7; ++i) *outs[i] = Array_gpu<Float,2>(out7[i], {ncol, nlev});
            d.ncol = ncol; d.nlay = nlay;
        }
        else if (d.ncol != ncol || d.nlay != nlay)
        {
            for (Array_gpu<Float,2>* a : outs) { *a = Array_gpu<Float,2>(); a->set_dims({ncol, nlev}); }
            d.ncol = ncol; d.nlay = nlay;
        }
        const Array_gpu<Float,2> pl = view2(p_lay, ncol, nlay), pv = view2(p_lev, ncol, nlev), tl = view2(t_lay, ncol, nlay), tv = view2(t_lev, ncol, nlev);
        const Array_gpu<Float,2> c_lwp = view2(lwp, ncol, nlay), c_iwp = view2(iwp, ncol, nlay), c_rel = view2(rel, ncol, nlay), c_dei = view2(dei, ncol, nlay);
        const Array_gpu<Float,2> no_col_dry, no_rh;
        Array_gpu<Float,3> o3a, o3b, o3c, b1, b2, b3, b4; Array_gpu<Float,2> o2;
        d.lw->solve_gpu(true, d.clouds, false, false, d.gases, pl, pv, tl, tv, no_col_dry, view1(t_sfc, ncol), view2(emis_sfc, nbnd_lw, ncol),
                        c_lwp, c_iwp, c_rel, c_dei, o3a, o3b, o3c, o2, d.lw_up, d.lw_dn, d.lw_net, b1, b2, b3);
        Aerosol_concs_gpu no_aerosols;
        d.sw->solve_gpu(true, d.clouds, false, false, false, true, false, d.gases, pl, pv, tl, tv, no_col_dry,
                        view2(sfc_alb_dir, nbnd_sw, ncol), view2(sfc_alb_dif, nbnd_sw, ncol), view1(tsi_scaling, ncol), view1(mu0, ncol),
                        c_lwp, c_iwp, c_rel, c_dei, no_rh, no_aerosols, o3a, o3b, o3c, o2, d.sw_up, d.sw_dn, d.sw_dir, d.sw_net, b1, b2, b3, b4);
    });
}

// device pointers of the seven broadband flux arrays of the last solve, (ncol, nlay+1) each
int rrx_cxx_driver_fluxes(void* h, const Float** ptrs)
{
    return guarded([&]
    {
        Driver& d = *static_cast<Driver*>(h);
        const Array_gpu<Float,2>* a[7] = {&d.lw_up, &d.lw_dn, &d.lw_net, &d.sw_up, &d.sw_dn, &d.sw_dir, &d.sw_net};
        for (int i=0; i<7; ++i) ptrs[i] = a[i]->ptr();
    });
}

// Raytracer_gpu::trace_rays on device arrays the caller owns (views; needs no driver handle). tau, ssa (ncol, nz, ngpt); band_lims_gpt
// (2, nbnd); cld_* (ncol, nz, nbnd) or all NULL; sfc_albedo (ncol); inc_dir, inc_dif (ngpt) on the HOST; out6: device arrays sfc_dn_dir,
// sfc_dn_dif, sfc_up, tod_up (ncol), abs_dir, abs_dif (ncol, nz). Runs on `stream` and waits for the count of dropped photons.
// rrx_cxx_trace_rays_phase: the same after Raytracer_gpu::set_phase_table(mu (nmu), phase, cdf (nmu, nre, nbnd), re0, dre, cld_re (ncol, nz)),
// device arrays; with mu NULL no table is set.
// rrx_cxx_trace_rays_bg: the same after Raytracer_gpu::set_background(dz_bg (nbg) on the HOST, bg_tau, bg_ssa (nbg, ngpt), bg_cld_* (nbg, nbnd)
// or all NULL); out5: device arrays toa_up, tod_dn_dir, tod_dn_dif (ncol), bg_abs_dir, bg_abs_dif (nbg). nbg = 0: no background is set
// and out5 is not written.
// rrx_cxx_trace_rays_aer: the same after Raytracer_gpu::set_aerosol(aer_* (ncol, nz, nbnd) or all NULL, bg_aer_* (nbg, nbnd) or all NULL), called
// when any of the six is given; a background aerosol with nbg = 0 is handed over as one layer, so that the class refuses it.
// rrx_cxx_trace_rays_spectral: the same through Raytracer_gpu::trace_rays_spectral with photons_per_pixel_gpt (ngpt) on the HOST
// (DESIGN.md 4.19); rrx_cxx_spectral_allocation: Raytracer_gpu::spectral_allocation into m (ngpt) on the HOST.
static int trace_rays_forward(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy, const Float dz,
        const int top_at_1, const int independent_column, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const Float* inc_dif, const int knx, const int kny, const int knz, const long long photons_per_pixel,
        const long long* photons_per_pixel_gpt,
        const unsigned long long seed, const int max_events, Float* const* out6, unsigned long long* n_capped, Float* const* out5,
        const int nmu, const int nre, const Float re0, const Float dre, const Float* mu, const Float* phase, const Float* cdf, const Float* cld_re,
        const int nbg, const Float* dz_bg, const Float* bg_tau, const Float* bg_ssa, const Float* bg_cld_tau, const Float* bg_cld_ssa,
        const Float* bg_cld_g, const Float* aer_tau, const Float* aer_ssa, const Float* aer_g, const Float* bg_aer_tau, const Float* bg_aer_ssa,
        const Float* bg_aer_g, void* stream)
{
    return guarded([&]
    {
        void* const before = rrx_host::current_stream();
        rrx_host::set_stream(stream);
        try
        {
            const int ncol = nx*ny;
            auto view3 = [](const Float* p, int a, int b, int c) { return p ? Array_gpu<Float,3>(const_cast<Float*>(p), {a, b, c}) : Array_gpu<Float,3>(); };
            auto bview = [](const Float* p, int a, int b) { return p ? Array_gpu<Float,2>(const_cast<Float*>(p), {a, b}) : Array_gpu<Float,2>(); };
            Array<Float,1> h_dir({ngpt}), h_dif({ngpt});
            for (int g=1; g<=ngpt; ++g) { h_dir({g}) = inc_dir[g-1]; h_dif({g}) = inc_dif[g-1]; }
            Array_gpu<Float,1> o0 = view1(out6[0], ncol), o1 = view1(out6[1], ncol), o2 = view1(out6[2], ncol), o3 = view1(out6[3], ncol);
            Array_gpu<Float,2> o4 = view2(out6[4], ncol, nz), o5 = view2(out6[5], ncol, nz);
            Raytracer_gpu raytracer;
            if (mu != nullptr)
                raytracer.set_phase_table(view1(mu, nmu), view3(phase, nmu, nre, nbnd), view3(cdf, nmu, nre, nbnd), re0, dre, view2(cld_re, ncol, nz));
            const bool any_aer = aer_tau || aer_ssa || aer_g || bg_aer_tau || bg_aer_ssa || bg_aer_g;
            const int nb = nbg > 0 ? nbg : 1;
            if (nbg > 0)
            {
                Array<Float,1> h_dz({nbg});
                for (int b=1; b<=nbg; ++b) h_dz({b}) = dz_bg[b-1];
                raytracer.set_background(h_dz, bview(bg_tau, nbg, ngpt), bview(bg_ssa, nbg, ngpt), bview(bg_cld_tau, nbg, nbnd),
                                         bview(bg_cld_ssa, nbg, nbnd), bview(bg_cld_g, nbg, nbnd));
            }
            if (any_aer)
                raytracer.set_aerosol(view3(aer_tau, ncol, nz, nbnd), view3(aer_ssa, ncol, nz, nbnd), view3(aer_g, ncol, nz, nbnd),
                                      bview(bg_aer_tau, nb, nbnd), bview(bg_aer_ssa, nb, nbnd), bview(bg_aer_g, nb, nbnd));
            if (photons_per_pixel_gpt != nullptr)
            {
                Array<long long,1> h_m({ngpt});
                for (int g=1; g<=ngpt; ++g) h_m({g}) = photons_per_pixel_gpt[g-1];
                Array_gpu<Float,1> b0, b1, b2, b3, b4;
                if (nbg > 0) { b0 = view1(out5[0], ncol); b1 = view1(out5[1], ncol); b2 = view1(out5[2], ncol); b3 = view1(out5[3], nbg); b4 = view1(out5[4], nbg); }
                *n_capped = raytracer.trace_rays_spectral(nx, ny, nz, dx, dy, dz, top_at_1 != 0, independent_column != 0,
                        view3(tau, ncol, nz, ngpt), view3(ssa, ncol, nz, ngpt), Array_gpu<int,2>(const_cast<int*>(band_lims_gpt), {2, nbnd}),
                        view3(cld_tau, ncol, nz, nbnd), view3(cld_ssa, ncol, nz, nbnd), view3(cld_g, ncol, nz, nbnd), view1(sfc_albedo, ncol),
                        mu0, azimuth, h_dir, h_dif, knx, kny, knz, h_m, seed, max_events, o0, o1, o2, o3, o4, o5, b0, b1, b2, b3, b4);
            }
            else if (nbg > 0)
            {
                Array_gpu<Float,1> b0 = view1(out5[0], ncol), b1 = view1(out5[1], ncol), b2 = view1(out5[2], ncol);
                Array_gpu<Float,1> b3 = view1(out5[3], nbg), b4 = view1(out5[4], nbg);
                *n_capped = raytracer.trace_rays(nx, ny, nz, dx, dy, dz, top_at_1 != 0, independent_column != 0,
                        view3(tau, ncol, nz, ngpt), view3(ssa, ncol, nz, ngpt), Array_gpu<int,2>(const_cast<int*>(band_lims_gpt), {2, nbnd}),
                        view3(cld_tau, ncol, nz, nbnd), view3(cld_ssa, ncol, nz, nbnd), view3(cld_g, ncol, nz, nbnd), view1(sfc_albedo, ncol),
                        mu0, azimuth, h_dir, h_dif, knx, kny, knz, photons_per_pixel, seed, max_events, o0, o1, o2, o3, o4, o5, b0, b1, b2, b3, b4);
            }
            else
                *n_capped = raytracer.trace_rays(nx, ny, nz, dx, dy, dz, top_at_1 != 0, independent_column != 0,
                        view3(tau, ncol, nz, ngpt), view3(ssa, ncol, nz, ngpt), Array_gpu<int,2>(const_cast<int*>(band_lims_gpt), {2, nbnd}),
                        view3(cld_tau, ncol, nz, nbnd), view3(cld_ssa, ncol, nz, nbnd), view3(cld_g, ncol, nz, nbnd), view1(sfc_albedo, ncol),
                        mu0, azimuth, h_dir, h_dif, knx, kny, knz, photons_per_pixel, seed, max_events, o0, o1, o2, o3, o4, o5);
        }
        catch (...) { rrx_host::set_stream(before); throw; }
        rrx_host::set_stream(before);
    });
}

int rrx_cxx_trace_rays_aer(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy, const Float dz,
        const int top_at_1, const int independent_column, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const Float* inc_dif, const int knx, const int kny, const int knz, const long long photons_per_pixel,
        const unsigned long long seed, const int max_events, Float* const* out6, unsigned long long* n_capped, Float* const* out5,
        const int nmu, const int nre, const Float re0, const Float dre, const Float* mu, const Float* phase, const Float* cdf, const Float* cld_re,
        const int nbg, const Float* dz_bg, const Float* bg_tau, const Float* bg_ssa, const Float* bg_cld_tau, const Float* bg_cld_ssa,
        const Float* bg_cld_g, const Float* aer_tau, const Float* aer_ssa, const Float* aer_g, const Float* bg_aer_tau, const Float* bg_aer_ssa,
        const Float* bg_aer_g, void* stream)
{
    return trace_rays_forward(nx, ny, nz, ngpt, nbnd, dx, dy, dz, top_at_1, independent_column, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g,
                              sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, photons_per_pixel, nullptr, seed, max_events, out6, n_capped,
                              out5, nmu, nre, re0, dre, mu, phase, cdf, cld_re, nbg, dz_bg, bg_tau, bg_ssa, bg_cld_tau, bg_cld_ssa, bg_cld_g,
                              aer_tau, aer_ssa, aer_g, bg_aer_tau, bg_aer_ssa, bg_aer_g, stream);
}

int rrx_cxx_trace_rays_spectral(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy, const Float dz,
        const int top_at_1, const int independent_column, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const Float* inc_dif, const int knx, const int kny, const int knz, const long long* photons_per_pixel_gpt,
        const unsigned long long seed, const int max_events, Float* const* out6, unsigned long long* n_capped, Float* const* out5,
        const int nmu, const int nre, const Float re0, const Float dre, const Float* mu, const Float* phase, const Float* cdf, const Float* cld_re,
        const int nbg, const Float* dz_bg, const Float* bg_tau, const Float* bg_ssa, const Float* bg_cld_tau, const Float* bg_cld_ssa,
        const Float* bg_cld_g, const Float* aer_tau, const Float* aer_ssa, const Float* aer_g, const Float* bg_aer_tau, const Float* bg_aer_ssa,
        const Float* bg_aer_g, void* stream)
{
    if (photons_per_pixel_gpt == nullptr) return guarded([&] { throw std::runtime_error("rrx_cxx_trace_rays_spectral: photons_per_pixel_gpt is NULL"); });
    return trace_rays_forward(nx, ny, nz, ngpt, nbnd, dx, dy, dz, top_at_1, independent_column, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g,
                              sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, 0, photons_per_pixel_gpt, seed, max_events, out6, n_capped,
                              out5, nmu, nre, re0, dre, mu, phase, cdf, cld_re, nbg, dz_bg, bg_tau, bg_ssa, bg_cld_tau, bg_cld_ssa, bg_cld_g,
                              aer_tau, aer_ssa, aer_g, bg_aer_tau, bg_aer_ssa, bg_aer_g, stream);
}

int rrx_cxx_spectral_allocation(const int ngpt, const Float* inc, const long long P, const long long min_per_gpt, long long* m)
{
    return guarded([&]
    {
        Array<Float,1> h_inc({ngpt});
        for (int g=1; g<=ngpt; ++g) h_inc({g}) = inc[g-1];
        const Array<long long,1> out = Raytracer_gpu::spectral_allocation(h_inc, P, min_per_gpt);
        for (int g=1; g<=ngpt; ++g) m[g-1] = out({g});
    });
}

int rrx_cxx_trace_rays_bg(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy, const Float dz,
        const int top_at_1, const int independent_column, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const Float* inc_dif, const int knx, const int kny, const int knz, const long long photons_per_pixel,
        const unsigned long long seed, const int max_events, Float* const* out6, unsigned long long* n_capped, Float* const* out5,
        const int nmu, const int nre, const Float re0, const Float dre, const Float* mu, const Float* phase, const Float* cdf, const Float* cld_re,
        const int nbg, const Float* dz_bg, const Float* bg_tau, const Float* bg_ssa, const Float* bg_cld_tau, const Float* bg_cld_ssa,
        const Float* bg_cld_g, void* stream)
{
    return rrx_cxx_trace_rays_aer(nx, ny, nz, ngpt, nbnd, dx, dy, dz, top_at_1, independent_column, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g,
                                  sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, photons_per_pixel, seed, max_events, out6, n_capped,
                                  out5, nmu, nre, re0, dre, mu, phase, cdf, cld_re, nbg, dz_bg, bg_tau, bg_ssa, bg_cld_tau, bg_cld_ssa, bg_cld_g,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int rrx_cxx_trace_rays_phase(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy, const Float dz,
        const int top_at_1, const int independent_column, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const Float* inc_dif, const int knx, const int kny, const int knz, const long long photons_per_pixel,
        const unsigned long long seed, const int max_events, Float* const* out6, unsigned long long* n_capped,
        const int nmu, const int nre, const Float re0, const Float dre, const Float* mu, const Float* phase, const Float* cdf, const Float* cld_re,
        void* stream)
{
    return guarded([&]
    {
        void* const before = rrx_host::current_stream();
        rrx_host::set_stream(stream);
        try
        {
            const int ncol = nx*ny;
            auto view3 = [](const Float* p, int a, int b, int c) { return p ? Array_gpu<Float,3>(const_cast<Float*>(p), {a, b, c}) : Array_gpu<Float,3>(); };
            Array<Float,1> h_dir({ngpt}), h_dif({ngpt});
            for (int g=1; g<=ngpt; ++g) { h_dir({g}) = inc_dir[g-1]; h_dif({g}) = inc_dif[g-1]; }
            Array_gpu<Float,1> o0 = view1(out6[0], ncol), o1 = view1(out6[1], ncol), o2 = view1(out6[2], ncol), o3 = view1(out6[3], ncol);
            Array_gpu<Float,2> o4 = view2(out6[4], ncol, nz), o5 = view2(out6[5], ncol, nz);
            Raytracer_gpu raytracer;
            if (mu != nullptr)
                raytracer.set_phase_table(view1(mu, nmu), view3(phase, nmu, nre, nbnd), view3(cdf, nmu, nre, nbnd), re0, dre, view2(cld_re, ncol, nz));
            *n_capped = raytracer.trace_rays(nx, ny, nz, dx, dy, dz, top_at_1 != 0, independent_column != 0,
                    view3(tau, ncol, nz, ngpt), view3(ssa, ncol, nz, ngpt), Array_gpu<int,2>(const_cast<int*>(band_lims_gpt), {2, nbnd}),
                    view3(cld_tau, ncol, nz, nbnd), view3(cld_ssa, ncol, nz, nbnd), view3(cld_g, ncol, nz, nbnd), view1(sfc_albedo, ncol),
                    mu0, azimuth, h_dir, h_dif, knx, kny, knz, photons_per_pixel, seed, max_events, o0, o1, o2, o3, o4, o5);
        }
        catch (...) { rrx_host::set_stream(before); throw; }
        rrx_host::set_stream(before);
    });
}

int rrx_cxx_trace_rays(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy, const Float dz,
        const int top_at_1, const int independent_column, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const Float* inc_dif, const int knx, const int kny, const int knz, const long long photons_per_pixel,
        const unsigned long long seed, const int max_events, Float* const* out6, unsigned long long* n_capped, void* stream)
{
    return rrx_cxx_trace_rays_phase(nx, ny, nz, ngpt, nbnd, dx, dy, dz, top_at_1, independent_column, tau, ssa, band_lims_gpt, cld_tau, cld_ssa,
                                    cld_g, sfc_albedo, mu0, azimuth, inc_dir, inc_dif, knx, kny, knz, photons_per_pixel, seed, max_events, out6,
                                    n_capped, 0, 0, Float(0.), Float(0.), nullptr, nullptr, nullptr, nullptr, stream);
}

// Raytracer_bw_gpu::trace_rays_bw on device arrays the caller owns (views; needs no driver handle). The scene as for rrx_cxx_trace_rays;
// inc_dir (ngpt) and sensor (12 numbers: position, e_w, e_h, e_d) on the HOST; radiance: a device array (npx, npy). Runs on `stream`
// and waits for the counts of dropped rays and clamped deposits.
// rrx_cxx_trace_rays_bw_phase: the same after Raytracer_bw_gpu::set_phase_table, as rrx_cxx_trace_rays_phase.
int rrx_cxx_trace_rays_bw_bg(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy, const Float dz,
        const int top_at_1, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const int knx, const int kny, const int knz, const int sensor_type, const int npx, const int npy, const Float fov,
        const Float* sensor, const long long rays_per_pixel, const unsigned long long seed, const int max_events, Float* radiance,
        unsigned long long* n_capped, unsigned long long* n_clamped,
        const int nmu, const int nre, const Float re0, const Float dre, const Float* mu, const Float* phase, const Float* cdf, const Float* cld_re,
        const int nbg, const Float* dz_bg, const Float* bg_tau, const Float* bg_ssa, const Float* bg_cld_tau, const Float* bg_cld_ssa,
        const Float* bg_cld_g, void* stream);

int rrx_cxx_trace_rays_bw_phase(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy, const Float dz,
        const int top_at_1, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const int knx, const int kny, const int knz, const int sensor_type, const int npx, const int npy, const Float fov,
        const Float* sensor, const long long rays_per_pixel, const unsigned long long seed, const int max_events, Float* radiance,
        unsigned long long* n_capped, unsigned long long* n_clamped,
        const int nmu, const int nre, const Float re0, const Float dre, const Float* mu, const Float* phase, const Float* cdf, const Float* cld_re,
        void* stream)
{
    return rrx_cxx_trace_rays_bw_bg(nx, ny, nz, ngpt, nbnd, dx, dy, dz, top_at_1, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_albedo,
                                    mu0, azimuth, inc_dir, knx, kny, knz, sensor_type, npx, npy, fov, sensor, rays_per_pixel, seed, max_events,
                                    radiance, n_capped, n_clamped, nmu, nre, re0, dre, mu, phase, cdf, cld_re, 0, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, stream);
}

// rrx_cxx_trace_rays_bw_bg: rrx_cxx_trace_rays_bw_phase after Raytracer_bw_gpu::set_background, as rrx_cxx_trace_rays_bg; nbg = 0: no background
// rrx_cxx_trace_rays_bw_aer: the same after Raytracer_bw_gpu::set_aerosol, as rrx_cxx_trace_rays_aer
}

// what rrx_cxx_trace_rays_bw_aer and rrx_cxx_trace_rays_bw_spectral (rays_per_pixel_gpt given) share
static int trace_rays_bw_any(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy, const Float dz,
        const int top_at_1, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const int knx, const int kny, const int knz, const int sensor_type, const int npx, const int npy, const Float fov,
        const Float* sensor, const long long rays_per_pixel, const long long* rays_per_pixel_gpt, const int nchan, const Float* chan_weights,
        const unsigned long long seed, const int max_events, Float* radiance,
        unsigned long long* n_capped, unsigned long long* n_clamped,
        const int nmu, const int nre, const Float re0, const Float dre, const Float* mu, const Float* phase, const Float* cdf, const Float* cld_re,
        const int nbg, const Float* dz_bg, const Float* bg_tau, const Float* bg_ssa, const Float* bg_cld_tau, const Float* bg_cld_ssa,
        const Float* bg_cld_g, const Float* aer_tau, const Float* aer_ssa, const Float* aer_g, const Float* bg_aer_tau, const Float* bg_aer_ssa,
        const Float* bg_aer_g, void* stream)
{
    return guarded([&]
    {
        void* const before = rrx_host::current_stream();
        rrx_host::set_stream(stream);
        try
        {
            const int ncol = nx*ny;
            auto view3 = [](const Float* p, int a, int b, int c) { return p ? Array_gpu<Float,3>(const_cast<Float*>(p), {a, b, c}) : Array_gpu<Float,3>(); };
            Array<Float,1> h_dir({ngpt});
            for (int g=1; g<=ngpt; ++g) h_dir({g}) = inc_dir[g-1];
            Sensor_bw s;
            s.sensor_type = sensor_type; s.npx = npx; s.npy = npy; s.fov = fov;
            for (int i=0; i<3; ++i) { s.position[i] = sensor[i]; s.e_w[i] = sensor[3+i]; s.e_h[i] = sensor[6+i]; s.e_d[i] = sensor[9+i]; }
            Array_gpu<Float,2> out = view2(radiance, npx, npy);
            Raytracer_bw_gpu raytracer;
            if (mu != nullptr)
                raytracer.set_phase_table(view1(mu, nmu), view3(phase, nmu, nre, nbnd), view3(cdf, nmu, nre, nbnd), re0, dre, view2(cld_re, ncol, nz));
            if (nbg > 0)
            {
                auto bview = [](const Float* p, int a, int b) { return p ? Array_gpu<Float,2>(const_cast<Float*>(p), {a, b}) : Array_gpu<Float,2>(); };
                Array<Float,1> h_dz({nbg});
                for (int b=1; b<=nbg; ++b) h_dz({b}) = dz_bg[b-1];
                raytracer.set_background(h_dz, bview(bg_tau, nbg, ngpt), bview(bg_ssa, nbg, ngpt), bview(bg_cld_tau, nbg, nbnd),
                                         bview(bg_cld_ssa, nbg, nbnd), bview(bg_cld_g, nbg, nbnd));
            }
            if (aer_tau || aer_ssa || aer_g || bg_aer_tau || bg_aer_ssa || bg_aer_g)
            {
                auto bview = [](const Float* p, int a, int b) { return p ? Array_gpu<Float,2>(const_cast<Float*>(p), {a, b}) : Array_gpu<Float,2>(); };
                const int nb = nbg > 0 ? nbg : 1;
                raytracer.set_aerosol(view3(aer_tau, ncol, nz, nbnd), view3(aer_ssa, ncol, nz, nbnd), view3(aer_g, ncol, nz, nbnd),
                                      bview(bg_aer_tau, nb, nbnd), bview(bg_aer_ssa, nb, nbnd), bview(bg_aer_g, nb, nbnd));
            }
            if (rays_per_pixel_gpt != nullptr)
            {
                // the spectral form: m_g from the caller, or (total_rays >= 0) dealt by Raytracer_gpu::spectral_allocation
                Array<long long,1> h_m({ngpt});
                for (int g=1; g<=ngpt; ++g) h_m({g}) = rays_per_pixel_gpt[g-1];
                if (rays_per_pixel >= 0) h_m = Raytracer_gpu::spectral_allocation(h_dir, rays_per_pixel, 1);
                if (chan_weights == nullptr) throw std::runtime_error("rrx_cxx_trace_rays_bw_spectral: chan_weights is NULL");
                if (nchan < 1 || nbnd < 1) throw std::runtime_error("rrx_cxx_trace_rays_bw_spectral: nchan and nbnd must be >= 1");
                Array<Float,2> h_w({nbnd, nchan});
                for (int c=1; c<=nchan; ++c)
                    for (int b=1; b<=nbnd; ++b) h_w({b, c}) = chan_weights[(c-1)*nbnd + (b-1)];
                Array_gpu<Float,3> out3(radiance, {npx, npy, nchan});
                *n_capped = raytracer.trace_rays_bw_spectral(nx, ny, nz, dx, dy, dz, top_at_1 != 0,
                        view3(tau, ncol, nz, ngpt), view3(ssa, ncol, nz, ngpt), Array_gpu<int,2>(const_cast<int*>(band_lims_gpt), {2, nbnd}),
                        view3(cld_tau, ncol, nz, nbnd), view3(cld_ssa, ncol, nz, nbnd), view3(cld_g, ncol, nz, nbnd), view1(sfc_albedo, ncol),
                        mu0, azimuth, h_dir, knx, kny, knz, s, h_m, seed, max_events, h_w, out3, n_clamped);
            }
            else
            *n_capped = raytracer.trace_rays_bw(nx, ny, nz, dx, dy, dz, top_at_1 != 0,
                    view3(tau, ncol, nz, ngpt), view3(ssa, ncol, nz, ngpt), Array_gpu<int,2>(const_cast<int*>(band_lims_gpt), {2, nbnd}),
                    view3(cld_tau, ncol, nz, nbnd), view3(cld_ssa, ncol, nz, nbnd), view3(cld_g, ncol, nz, nbnd), view1(sfc_albedo, ncol),
                    mu0, azimuth, h_dir, knx, kny, knz, s, rays_per_pixel, seed, max_events, out, n_clamped);
        }
        catch (...) { rrx_host::set_stream(before); throw; }
        rrx_host::set_stream(before);
    });
}

extern "C"
{
int rrx_cxx_trace_rays_bw_aer(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy, const Float dz,
        const int top_at_1, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const int knx, const int kny, const int knz, const int sensor_type, const int npx, const int npy, const Float fov,
        const Float* sensor, const long long rays_per_pixel, const unsigned long long seed, const int max_events, Float* radiance,
        unsigned long long* n_capped, unsigned long long* n_clamped,
        const int nmu, const int nre, const Float re0, const Float dre, const Float* mu, const Float* phase, const Float* cdf, const Float* cld_re,
        const int nbg, const Float* dz_bg, const Float* bg_tau, const Float* bg_ssa, const Float* bg_cld_tau, const Float* bg_cld_ssa,
        const Float* bg_cld_g, const Float* aer_tau, const Float* aer_ssa, const Float* aer_g, const Float* bg_aer_tau, const Float* bg_aer_ssa,
        const Float* bg_aer_g, void* stream)
{
    return trace_rays_bw_any(nx, ny, nz, ngpt, nbnd, dx, dy, dz, top_at_1, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_albedo, mu0,
                             azimuth, inc_dir, knx, kny, knz, sensor_type, npx, npy, fov, sensor, rays_per_pixel, nullptr, 0, nullptr, seed,
                             max_events, radiance, n_capped, n_clamped, nmu, nre, re0, dre, mu, phase, cdf, cld_re, nbg, dz_bg, bg_tau, bg_ssa,
                             bg_cld_tau, bg_cld_ssa, bg_cld_g, aer_tau, aer_ssa, aer_g, bg_aer_tau, bg_aer_ssa, bg_aer_g, stream);
}

// rrx_cxx_trace_rays_bw_spectral: the same through Raytracer_bw_gpu::trace_rays_bw_spectral. rays_per_pixel_gpt (ngpt,
// HOST): the rays per pixel of every g-point when total_rays < 0; otherwise total_rays is dealt by Raytracer_gpu::spectral_allocation
// over inc_dir and the array's contents are not used. chan_weights (nchan, nbnd) on the HOST; radiance: a device array (nchan, npy, npx).
int rrx_cxx_trace_rays_bw_spectral(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy,
        const Float dz, const int top_at_1, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const int knx, const int kny, const int knz, const int sensor_type, const int npx, const int npy, const Float fov,
        const Float* sensor, const long long* rays_per_pixel_gpt, const long long total_rays, const unsigned long long seed, const int max_events,
        const int nchan, const Float* chan_weights, Float* radiance, unsigned long long* n_capped, unsigned long long* n_clamped,
        const int nmu, const int nre, const Float re0, const Float dre, const Float* mu, const Float* phase, const Float* cdf, const Float* cld_re,
        const int nbg, const Float* dz_bg, const Float* bg_tau, const Float* bg_ssa, const Float* bg_cld_tau, const Float* bg_cld_ssa,
        const Float* bg_cld_g, const Float* aer_tau, const Float* aer_ssa, const Float* aer_g, const Float* bg_aer_tau, const Float* bg_aer_ssa,
        const Float* bg_aer_g, void* stream)
{
    if (rays_per_pixel_gpt == nullptr) return guarded([&] { throw std::runtime_error("rrx_cxx_trace_rays_bw_spectral: rays_per_pixel_gpt is NULL"); });
    return trace_rays_bw_any(nx, ny, nz, ngpt, nbnd, dx, dy, dz, top_at_1, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_albedo, mu0,
                             azimuth, inc_dir, knx, kny, knz, sensor_type, npx, npy, fov, sensor, total_rays, rays_per_pixel_gpt, nchan,
                             chan_weights, seed, max_events, radiance, n_capped, n_clamped, nmu, nre, re0, dre, mu, phase, cdf, cld_re, nbg,
                             dz_bg, bg_tau, bg_ssa, bg_cld_tau, bg_cld_ssa, bg_cld_g, aer_tau, aer_ssa, aer_g, bg_aer_tau, bg_aer_ssa, bg_aer_g,
                             stream);
}

int rrx_cxx_trace_rays_bw_bg(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy, const Float dz,
        const int top_at_1, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const int knx, const int kny, const int knz, const int sensor_type, const int npx, const int npy, const Float fov,
        const Float* sensor, const long long rays_per_pixel, const unsigned long long seed, const int max_events, Float* radiance,
        unsigned long long* n_capped, unsigned long long* n_clamped,
        const int nmu, const int nre, const Float re0, const Float dre, const Float* mu, const Float* phase, const Float* cdf, const Float* cld_re,
        const int nbg, const Float* dz_bg, const Float* bg_tau, const Float* bg_ssa, const Float* bg_cld_tau, const Float* bg_cld_ssa,
        const Float* bg_cld_g, void* stream)
{
    return rrx_cxx_trace_rays_bw_aer(nx, ny, nz, ngpt, nbnd, dx, dy, dz, top_at_1, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_albedo, mu0,
                                     azimuth, inc_dir, knx, kny, knz, sensor_type, npx, npy, fov, sensor, rays_per_pixel, seed, max_events, radiance,
                                     n_capped, n_clamped, nmu, nre, re0, dre, mu, phase, cdf, cld_re, nbg, dz_bg, bg_tau, bg_ssa, bg_cld_tau,
                                     bg_cld_ssa, bg_cld_g, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int rrx_cxx_trace_rays_bw(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy, const Float dz,
        const int top_at_1, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_albedo, const Float mu0, const Float azimuth,
        const Float* inc_dir, const int knx, const int kny, const int knz, const int sensor_type, const int npx, const int npy, const Float fov,
        const Float* sensor, const long long rays_per_pixel, const unsigned long long seed, const int max_events, Float* radiance,
        unsigned long long* n_capped, unsigned long long* n_clamped, void* stream)
{
    return rrx_cxx_trace_rays_bw_phase(nx, ny, nz, ngpt, nbnd, dx, dy, dz, top_at_1, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_albedo,
                                       mu0, azimuth, inc_dir, knx, kny, knz, sensor_type, npx, npy, fov, sensor, rays_per_pixel, seed, max_events,
                                       radiance, n_capped, n_clamped, 0, 0, Float(0.), Float(0.), nullptr, nullptr, nullptr, nullptr, stream);
}
}

// Raytracer_thermal_gpu::trace_rays_thermal on device arrays the caller owns (views; needs no driver handle). ssa NULL: the
// gas does not scatter; top_radiance (ngpt) and sensor (12 numbers) on the HOST, top_radiance NULL: none; radiance: a device array
// (npy, npx), or with by_band (nbnd, npy, npx). Runs on `stream` and waits for the counts of dropped rays and clamped deposits.
extern "C" int rrx_cxx_trace_rays_thermal(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy,
        const Float dz, const int top_at_1, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_emis, const Float* lay_src, const Float* sfc_src,
        const Float* top_radiance, const int knx, const int kny, const int knz, const int sensor_type, const int npx, const int npy, const Float fov,
        const Float* sensor, const long long rays_per_pixel, const unsigned long long seed, const int max_events, const int by_band, Float* radiance,
        unsigned long long* n_capped, unsigned long long* n_clamped, void* stream)
{
    return guarded([&]
    {
        void* const before = rrx_host::current_stream();
        rrx_host::set_stream(stream);
        try
        {
            const int ncol = nx*ny;
            auto view3 = [](const Float* p, int a, int b, int c) { return p ? Array_gpu<Float,3>(const_cast<Float*>(p), {a, b, c}) : Array_gpu<Float,3>(); };
            Array<Float,1> h_top;
            if (top_radiance != nullptr)
            {
                h_top.set_dims({ngpt});
                for (int g=1; g<=ngpt; ++g) h_top({g}) = top_radiance[g-1];
            }
            Sensor_bw s;
            s.sensor_type = sensor_type; s.npx = npx; s.npy = npy; s.fov = fov;
            for (int i=0; i<3; ++i) { s.position[i] = sensor[i]; s.e_w[i] = sensor[3+i]; s.e_h[i] = sensor[6+i]; s.e_d[i] = sensor[9+i]; }
            Array_gpu<Float,3> out(radiance, {npx, npy, by_band ? nbnd : 1});
            Raytracer_thermal_gpu raytracer;
            *n_capped = raytracer.trace_rays_thermal(nx, ny, nz, dx, dy, dz, top_at_1 != 0, view3(tau, ncol, nz, ngpt), view3(ssa, ncol, nz, ngpt),
                    Array_gpu<int,2>(const_cast<int*>(band_lims_gpt), {2, nbnd}), view3(cld_tau, ncol, nz, nbnd), view3(cld_ssa, ncol, nz, nbnd),
                    view3(cld_g, ncol, nz, nbnd), view1(sfc_emis, ncol), view3(lay_src, ncol, nz, ngpt), view2(sfc_src, ncol, ngpt), h_top,
                    knx, kny, knz, s, rays_per_pixel, seed, max_events, out, n_clamped);
        }
        catch (...) { rrx_host::set_stream(before); throw; }
        rrx_host::set_stream(before);
    });
}

// Raytracer_thermal_gpu::trace_rays_thermal_spectral on device arrays the caller owns. rays_per_pixel_gpt (ngpt, HOST): the
// rays per pixel of every g-point when total_rays < 0; otherwise total_rays is dealt by Raytracer_gpu::spectral_allocation over emission
// (ngpt, HOST), the g-points' emission, and the array's contents are not used. chan_weights (nchan, nbnd) on the HOST; radiance: a device
// array (nchan, npy, npx).
extern "C" int rrx_cxx_trace_rays_thermal_spectral(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx,
        const Float dy, const Float dz, const int top_at_1, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_emis, const Float* lay_src, const Float* sfc_src,
        const Float* top_radiance, const int knx, const int kny, const int knz, const int sensor_type, const int npx, const int npy, const Float fov,
        const Float* sensor, const long long* rays_per_pixel_gpt, const long long total_rays, const Float* emission, const unsigned long long seed,
        const int max_events, const int nchan, const Float* chan_weights, Float* radiance, unsigned long long* n_capped, unsigned long long* n_clamped,
        void* stream)
{
    return guarded([&]
    {
        const std::string who = "rrx_cxx_trace_rays_thermal_spectral: ";
        if (rays_per_pixel_gpt == nullptr) throw std::runtime_error(who + "rays_per_pixel_gpt is NULL");
        if (chan_weights == nullptr) throw std::runtime_error(who + "chan_weights is NULL");
        if (nchan < 1 || nbnd < 1) throw std::runtime_error(who + "nchan and nbnd must be >= 1");
        if (total_rays >= 0 && emission == nullptr) throw std::runtime_error(who + "emission is NULL");
        void* const before = rrx_host::current_stream();
        rrx_host::set_stream(stream);
        try
        {
            const int ncol = nx*ny;
            auto view3 = [](const Float* p, int a, int b, int c) { return p ? Array_gpu<Float,3>(const_cast<Float*>(p), {a, b, c}) : Array_gpu<Float,3>(); };
            Array<Float,1> h_top;
            if (top_radiance != nullptr)
            {
                h_top.set_dims({ngpt});
                for (int g=1; g<=ngpt; ++g) h_top({g}) = top_radiance[g-1];
            }
            Array<long long,1> h_m({ngpt});
            for (int g=1; g<=ngpt; ++g) h_m({g}) = rays_per_pixel_gpt[g-1];
            if (total_rays >= 0)
            {
                Array<Float,1> h_e({ngpt});
                for (int g=1; g<=ngpt; ++g) h_e({g}) = emission[g-1];
                h_m = Raytracer_gpu::spectral_allocation(h_e, total_rays, 1);
            }
            Array<Float,2> h_w({nbnd, nchan});
            for (int c=1; c<=nchan; ++c)
                for (int b=1; b<=nbnd; ++b) h_w({b, c}) = chan_weights[(c-1)*nbnd + (b-1)];
            Sensor_bw s;
            s.sensor_type = sensor_type; s.npx = npx; s.npy = npy; s.fov = fov;
            for (int i=0; i<3; ++i) { s.position[i] = sensor[i]; s.e_w[i] = sensor[3+i]; s.e_h[i] = sensor[6+i]; s.e_d[i] = sensor[9+i]; }
            Array_gpu<Float,3> out(radiance, {npx, npy, nchan});
            Raytracer_thermal_gpu raytracer;
            *n_capped = raytracer.trace_rays_thermal_spectral(nx, ny, nz, dx, dy, dz, top_at_1 != 0, view3(tau, ncol, nz, ngpt),
                    view3(ssa, ncol, nz, ngpt), Array_gpu<int,2>(const_cast<int*>(band_lims_gpt), {2, nbnd}), view3(cld_tau, ncol, nz, nbnd),
                    view3(cld_ssa, ncol, nz, nbnd), view3(cld_g, ncol, nz, nbnd), view1(sfc_emis, ncol), view3(lay_src, ncol, nz, ngpt),
                    view2(sfc_src, ncol, ngpt), h_top, knx, kny, knz, s, h_m, seed, max_events, h_w, out, n_clamped);
        }
        catch (...) { rrx_host::set_stream(before); throw; }
        rrx_host::set_stream(before);
    });
}

// Raytracer_thermal_gpu::trace_heating on device arrays the caller owns. rays_per_cell_gpt (ngpt) and top_radiance (ngpt,
// or NULL: none) on the HOST; flux_conv: a device array (nz, ncol).
extern "C" int rrx_cxx_trace_heating(const int nx, const int ny, const int nz, const int ngpt, const int nbnd, const Float dx, const Float dy,
        const Float dz, const int top_at_1, const Float* tau, const Float* ssa, const int* band_lims_gpt,
        const Float* cld_tau, const Float* cld_ssa, const Float* cld_g, const Float* sfc_emis, const Float* lay_src, const Float* sfc_src,
        const Float* top_radiance, const int knx, const int kny, const int knz, const long long* rays_per_cell_gpt, const unsigned long long seed,
        const int max_events, Float* flux_conv, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream)
{
    return guarded([&]
    {
        if (rays_per_cell_gpt == nullptr) throw std::runtime_error("rrx_cxx_trace_heating: rays_per_cell_gpt is NULL");
        void* const before = rrx_host::current_stream();
        rrx_host::set_stream(stream);
        try
        {
            const int ncol = nx*ny;
            auto view3 = [](const Float* p, int a, int b, int c) { return p ? Array_gpu<Float,3>(const_cast<Float*>(p), {a, b, c}) : Array_gpu<Float,3>(); };
            Array<Float,1> h_top;
            if (top_radiance != nullptr)
            {
                h_top.set_dims({ngpt});
                for (int g=1; g<=ngpt; ++g) h_top({g}) = top_radiance[g-1];
            }
            Array<long long,1> h_m({ngpt});
            for (int g=1; g<=ngpt; ++g) h_m({g}) = rays_per_cell_gpt[g-1];
            Array_gpu<Float,2> out(flux_conv, {ncol, nz});
            Raytracer_thermal_gpu raytracer;
            *n_capped = raytracer.trace_heating(nx, ny, nz, dx, dy, dz, top_at_1 != 0, view3(tau, ncol, nz, ngpt), view3(ssa, ncol, nz, ngpt),
                    Array_gpu<int,2>(const_cast<int*>(band_lims_gpt), {2, nbnd}), view3(cld_tau, ncol, nz, nbnd), view3(cld_ssa, ncol, nz, nbnd),
                    view3(cld_g, ncol, nz, nbnd), view1(sfc_emis, ncol), view3(lay_src, ncol, nz, ngpt), view2(sfc_src, ncol, ngpt), h_top,
                    knx, kny, knz, h_m, seed, max_events, out, n_clamped);
        }
        catch (...) { rrx_host::set_stream(before); throw; }
        rrx_host::set_stream(before);
    });
}
