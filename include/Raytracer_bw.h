/* Raytracer_bw_gpu -- backward Monte Carlo ray tracer: shortwave radiances for a virtual camera or a flux sensor (rrx_raytracer_bw,
 * DESIGN.md 4.15). A class of this project's own shape, the twin of Raytracer_gpu: it takes the clear g-point arrays and the band
 * cloud triple as the gas and cloud optics write them. (The reference's Raytracer_bw::trace_rays_bw takes the structures of its _rt
 * pipeline and a Camera of its own, which this project does not have: INTEGRATION.md.) */
#ifndef RAYTRACER_BW_H
#define RAYTRACER_BW_H
#include "Array.h"
#include "rrx_forward.h"

// sensor_type 0 perspective, 1 fisheye, 2 orthographic, 3 flux sensor; npx x npy pixels; fov in radians (fisheye only); the image
// axes e_w, e_h and the viewing direction e_d as include/rrx_hip.h describes them
struct Sensor_bw
{
    int sensor_type = 0;
    int npx = 0, npy = 0;
    Float fov = Float(0.);
    Float position[3] = {Float(0.), Float(0.), Float(0.)};
    Float e_w[3] = {Float(1.), Float(0.), Float(0.)};
    Float e_h[3] = {Float(0.), Float(1.), Float(0.)};
    Float e_d[3] = {Float(0.), Float(0.), Float(-1.)};
};

class Raytracer_bw_gpu
{
    public:
        Raytracer_bw_gpu() {}

        // tau, ssa (ncol = nx ny, nz, ngpt); band_lims_gpt (2, nbnd); cld_* (ncol, nz, nbnd), all three of size 0 for a clear sky;
        // sfc_albedo (ncol); inc_dir (ngpt) on the host; radiance (npx, npy) in W m-2 sr-1 is overwritten. Returns the number of rays
        // dropped at max_events (0 in a healthy run); n_clamped, when given, receives the number of deposits clamped at 2^20.
        unsigned long long trace_rays_bw(
                const int nx, const int ny, const int nz,
                const Float dx, const Float dy, const Float dz,
                const bool top_at_1,
                const Array_gpu<Float,3>& tau, const Array_gpu<Float,3>& ssa,
                const Array_gpu<int,2>& band_lims_gpt,
                const Array_gpu<Float,3>& cld_tau, const Array_gpu<Float,3>& cld_ssa, const Array_gpu<Float,3>& cld_g,
                const Array_gpu<Float,1>& sfc_albedo,
                const Float mu0, const Float azimuth,
                const Array<Float,1>& inc_dir,
                const int knx, const int kny, const int knz,
                const Sensor_bw& sensor,
                const long long rays_per_pixel, const unsigned long long seed, const int max_events,
                Array_gpu<Float,2>& radiance, unsigned long long* n_clamped = nullptr);

        // The rays of all g-points in one launch, tallied by band, and a channel matrix from bands to what the sensor sees
        // (rrx_camera_render_spectral): trace_rays_bw with rays_per_pixel_gpt (ngpt) on the host, the rays per pixel of
        // every g-point (Raytracer_gpu::spectral_allocation deals a total by flux, or the caller brings its own), in place of
        // rays_per_pixel, and chan_weights (nbnd, nchan) on the host: channel c sees sum_b chan_weights(b, c) x the radiance of band b.
        // radiance (npx, npy, nchan) in W m-2 sr-1 is overwritten. It honours the phase table, the background and the aerosol that are
        // set. ngpt <= 1024.
        unsigned long long trace_rays_bw_spectral(
                const int nx, const int ny, const int nz,
                const Float dx, const Float dy, const Float dz,
                const bool top_at_1,
                const Array_gpu<Float,3>& tau, const Array_gpu<Float,3>& ssa,
                const Array_gpu<int,2>& band_lims_gpt,
                const Array_gpu<Float,3>& cld_tau, const Array_gpu<Float,3>& cld_ssa, const Array_gpu<Float,3>& cld_g,
                const Array_gpu<Float,1>& sfc_albedo,
                const Float mu0, const Float azimuth,
                const Array<Float,1>& inc_dir,
                const int knx, const int kny, const int knz,
                const Sensor_bw& sensor,
                const Array<long long,1>& rays_per_pixel_gpt, const unsigned long long seed, const int max_events,
                const Array<Float,2>& chan_weights,
                Array_gpu<Float,3>& radiance, unsigned long long* n_clamped = nullptr);

        // Tabulated cloud phase functions (rrx_*_phase): with a table set, cloud scatters by the phase function of the
        // cell's radius in place of Henyey-Greenstein. mu (nmu); phase, cdf (nmu, nre, nbnd) as rrx_rt_phase_tables makes them
        // (rrx_rt_phase_tables); the radii re0 + dre ire; cld_re (ncol, nz) in the unit of re0. The arrays are copied.
        void set_phase_table(const Array_gpu<Float,1>& mu, const Array_gpu<Float,3>& phase, const Array_gpu<Float,3>& cdf,
                             const Float re0, const Float dre, const Array_gpu<Float,2>& cld_re);
        void clear_phase_table() { has_table = false; mu = Array_gpu<Float,1>(); phase = Array_gpu<Float,3>(); cdf = Array_gpu<Float,3>(); cld_re = Array_gpu<Float,2>(); }

        // A background atmosphere between the domain top and TOA (rrx_raytracer_bw_bg), as Raytracer_gpu::set_background
        // takes it. With a background set, rays end only at TOA, a sensor may sit inside the background, and the orthographic and the
        // downward flux sensor start at clamp(position[2], domain top, TOA). The arrays are copied.
        void set_background(const Array<Float,1>& dz_bg, const Array_gpu<Float,2>& bg_tau, const Array_gpu<Float,2>& bg_ssa,
                            const Array_gpu<Float,2>& bg_cld_tau, const Array_gpu<Float,2>& bg_cld_ssa, const Array_gpu<Float,2>& bg_cld_g);
        void clear_background() { has_bg = false; dz_bg = Array<Float,1>(); bg_tau = Array_gpu<Float,2>(); bg_ssa = Array_gpu<Float,2>();
                                  bg_cld_tau = Array_gpu<Float,2>(); bg_cld_ssa = Array_gpu<Float,2>(); bg_cld_g = Array_gpu<Float,2>(); }

        // Aerosol as a third scattering species (rrx_raytracer_bw_aer): the grid's band triple aer_* (ncol, nz, nbnd) and
        // the background's bg_aer_* (nbg, nbnd); either triple may be three arrays of size 0. The arrays are copied. A background
        // aerosol needs a background (set_background first): without one it throws. With aerosol set trace_rays_bw goes
        // through rrx_raytracer_bw_aer; aerosol scatters by Henyey-Greenstein with its own g, with a phase table too.
        void set_aerosol(const Array_gpu<Float,3>& aer_tau, const Array_gpu<Float,3>& aer_ssa, const Array_gpu<Float,3>& aer_g,
                         const Array_gpu<Float,2>& bg_aer_tau, const Array_gpu<Float,2>& bg_aer_ssa, const Array_gpu<Float,2>& bg_aer_g);
        void clear_aerosol() { has_aer = false; aer_tau = Array_gpu<Float,3>(); aer_ssa = Array_gpu<Float,3>(); aer_g = Array_gpu<Float,3>();
                               bg_aer_tau = Array_gpu<Float,2>(); bg_aer_ssa = Array_gpu<Float,2>(); bg_aer_g = Array_gpu<Float,2>(); }

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
