/* Raytracer_gpu -- forward Monte Carlo ray tracer for 3-D shortwave fluxes (rrx_raytracer_sw). A class of this
 * project's own shape: it takes the clear g-point arrays and the band cloud triple as the gas and cloud optics write them. (The
 * reference's Raytracer::trace_rays takes the structures of its _rt pipeline, which this project does not have: INTEGRATION.md.) */
#ifndef RAYTRACER_H
#define RAYTRACER_H
#include "Array.h"
#include "rrx_forward.h"

class Raytracer_gpu
{
    public:
        Raytracer_gpu() {}

        // tau, ssa (ncol = nx ny, nz, ngpt); band_lims_gpt (2, nbnd); cld_* (ncol, nz, nbnd), all three of size 0 for a clear sky;
        // sfc_albedo (ncol); inc_dir, inc_dif (ngpt) on the host; the flux arrays (ncol) in W m-2 and the absorption arrays
        // (ncol, nz) in W m-3 are overwritten. Returns the number of photons dropped at max_events (0 in a healthy run).
        unsigned long long trace_rays(
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
                Array_gpu<Float,2>& abs_dir, Array_gpu<Float,2>& abs_dif);

        // Tabulated cloud phase functions (rrx_*_phase): with a table set, cloud scatters by the phase function of the
        // cell's radius in place of Henyey-Greenstein. mu (nmu); phase, cdf (nmu, nre, nbnd) as rrx_rt_phase_tables makes them
        // (rrx_rt_phase_tables); the radii re0 + dre ire; cld_re (ncol, nz) in the unit of re0. The arrays are copied.
        void set_phase_table(const Array_gpu<Float,1>& mu, const Array_gpu<Float,3>& phase, const Array_gpu<Float,3>& cdf,
                             const Float re0, const Float dre, const Array_gpu<Float,2>& cld_re);
        void clear_phase_table() { has_table = false; mu = Array_gpu<Float,1>(); phase = Array_gpu<Float,3>(); cdf = Array_gpu<Float,3>(); cld_re = Array_gpu<Float,2>(); }

        // A background atmosphere between the domain top and TOA (rrx_raytracer_sw_bg): nbg horizontally uniform layers
        // counted upward from the domain top. dz_bg (nbg) on the host, all > 0; bg_tau, bg_ssa (nbg, ngpt); bg_cld_* (nbg, nbnd), all
        // three of size 0 for a clear background. The arrays are copied. With a background set, photons start at TOA and trace_rays is
        // called in the form below, which also fills toa_up, tod_dn_dir, tod_dn_dif (ncol) in W m-2 and bg_abs_dir, bg_abs_dif (nbg) in
        // W m-3 of a domain-wide layer; tod_up is then the flux through the domain top.
        void set_background(const Array<Float,1>& dz_bg, const Array_gpu<Float,2>& bg_tau, const Array_gpu<Float,2>& bg_ssa,
                            const Array_gpu<Float,2>& bg_cld_tau, const Array_gpu<Float,2>& bg_cld_ssa, const Array_gpu<Float,2>& bg_cld_g);
        void clear_background() { has_bg = false; dz_bg = Array<Float,1>(); bg_tau = Array_gpu<Float,2>(); bg_ssa = Array_gpu<Float,2>();
                                  bg_cld_tau = Array_gpu<Float,2>(); bg_cld_ssa = Array_gpu<Float,2>(); bg_cld_g = Array_gpu<Float,2>(); }
        unsigned long long trace_rays(
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
                Array_gpu<Float,1>& bg_abs_dir, Array_gpu<Float,1>& bg_abs_dif);

        // Aerosol as a third scattering species (rrx_raytracer_sw_aer): the grid's band triple aer_* (ncol, nz, nbnd) and
        // the background's bg_aer_* (nbg, nbnd); either triple may be three arrays of size 0. The arrays are copied. A background
        // aerosol needs a background (set_background first): without one it throws. With aerosol set both forms of trace_rays go
        // through rrx_raytracer_sw_aer; aerosol scatters by Henyey-Greenstein with its own g, with a phase table too.
        void set_aerosol(const Array_gpu<Float,3>& aer_tau, const Array_gpu<Float,3>& aer_ssa, const Array_gpu<Float,3>& aer_g,
                         const Array_gpu<Float,2>& bg_aer_tau, const Array_gpu<Float,2>& bg_aer_ssa, const Array_gpu<Float,2>& bg_aer_g);
        void clear_aerosol() { has_aer = false; aer_tau = Array_gpu<Float,3>(); aer_ssa = Array_gpu<Float,3>(); aer_g = Array_gpu<Float,3>();
                               bg_aer_tau = Array_gpu<Float,2>(); bg_aer_ssa = Array_gpu<Float,2>(); bg_aer_g = Array_gpu<Float,2>(); }

        // All g-points in one launch, photons dealt per g-point (rrx_raytracer_sw_spectral): trace_rays with
        // photons_per_pixel_gpt (ngpt) on the host, the photons per pixel of every g-point, in place of photons_per_pixel. It
        // honours the phase table, the background and the aerosol that are set; the five background outputs are filled with a
        // background set and not touched without one (they may then be empty). ngpt <= 1024.
        unsigned long long trace_rays_spectral(
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
                Array_gpu<Float,1>& bg_abs_dir, Array_gpu<Float,1>& bg_abs_dif);

        // photons_per_pixel_gpt for a total of P photons per pixel: dealt over the g-points with inc > 0 in proportion to inc by
        // largest remainders (ties to the lower g), at least min_per_gpt each; throws when P is below that floor.
        static Array<long long,1> spectral_allocation(const Array<Float,1>& inc, const long long P, const long long min_per_gpt = 1);

    private:
        bool has_aer = false;
        Array_gpu<Float,3> aer_tau, aer_ssa, aer_g;
        Array_gpu<Float,2> bg_aer_tau, bg_aer_ssa, bg_aer_g;
        bool has_bg = false;
        Array<Float,1> dz_bg;
        Array_gpu<Float,2> bg_tau, bg_ssa, bg_cld_tau, bg_cld_ssa, bg_cld_g;
        bool has_table = false;
        Float re0 = Float(0.), dre = Float(0.);
        Array_gpu<Float,1> mu;
        Array_gpu<Float,3> phase, cdf;
        Array_gpu<Float,2> cld_re;
};
#endif
