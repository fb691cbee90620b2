/* Raytracer_thermal_gpu -- thermal emission in the backward Monte Carlo ray tracer: longwave radiances for a virtual camera, 3-D
 * longwave fluxes for a flux sensor (rrx_thermal_render; rrx_thermal_render_spectral). The longwave twin of Raytracer_bw_gpu, with the same
 * Sensor_bw: it takes the clear g-point optical depth, the Planck sources and the band cloud triple as the LW gas and cloud optics
 * write them. trace_heating (rrx_heating3d_render) gives the 3-D longwave heating of every cell from the same
 * scene. No background, no aerosol, no phase table. */
#ifndef RAYTRACER_THERMAL_H
#define RAYTRACER_THERMAL_H
#include "Raytracer_bw.h"

class Raytracer_thermal_gpu
{
    public:
        Raytracer_thermal_gpu() {}

        // tau (ncol = nx ny, nz, ngpt); ssa the same, or of size 0 for a gas that does not scatter; band_lims_gpt (2, nbnd); cld_*
        // (ncol, nz, nbnd), all three of size 0 for a clear sky; sfc_emis (ncol), one broadband emissivity per pixel; the sources are
        // radiances in W m-2 sr-1: lay_src (ncol, nz, ngpt), sfc_src (ncol, ngpt), and top_radiance (ngpt) on the host, the isotropic
        // downward radiance at the domain top, of size 0 for none. radiance in W m-2 sr-1 is overwritten: (npx, npy, 1), the sum over
        // the g-points, or (npx, npy, nbnd), radiance by band. With a flux sensor pi x radiance is the pixel's irradiance. Returns the
        // number of rays dropped at max_events (0 in a healthy run); n_clamped, when given, receives the number of deposits clamped at
        // 2^20.
        unsigned long long trace_rays_thermal(
                const int nx, const int ny, const int nz,
                const Float dx, const Float dy, const Float dz,
                const bool top_at_1,
                const Array_gpu<Float,3>& tau, const Array_gpu<Float,3>& ssa,
                const Array_gpu<int,2>& band_lims_gpt,
                const Array_gpu<Float,3>& cld_tau, const Array_gpu<Float,3>& cld_ssa, const Array_gpu<Float,3>& cld_g,
                const Array_gpu<Float,1>& sfc_emis,
                const Array_gpu<Float,3>& lay_src, const Array_gpu<Float,2>& sfc_src,
                const Array<Float,1>& top_radiance,
                const int knx, const int kny, const int knz,
                const Sensor_bw& sensor,
                const long long rays_per_pixel, const unsigned long long seed, const int max_events,
                Array_gpu<Float,3>& radiance, unsigned long long* n_clamped = nullptr);

        // The rays of all g-points in one launch, tallied by band, and a channel matrix from bands to what the sensor sees
        // (rrx_thermal_render_spectral): trace_rays_thermal with rays_per_pixel_gpt (ngpt) on the host, the rays per
        // pixel of every g-point (the caller's, or Raytracer_gpu::spectral_allocation's over the g-points' emission; a g-point with
        // none is left out of the result), and chan_weights (nbnd, nchan) on the host. radiance (npx, npy, nchan) is overwritten.
        unsigned long long trace_rays_thermal_spectral(
                const int nx, const int ny, const int nz,
                const Float dx, const Float dy, const Float dz,
                const bool top_at_1,
                const Array_gpu<Float,3>& tau, const Array_gpu<Float,3>& ssa,
                const Array_gpu<int,2>& band_lims_gpt,
                const Array_gpu<Float,3>& cld_tau, const Array_gpu<Float,3>& cld_ssa, const Array_gpu<Float,3>& cld_g,
                const Array_gpu<Float,1>& sfc_emis,
                const Array_gpu<Float,3>& lay_src, const Array_gpu<Float,2>& sfc_src,
                const Array<Float,1>& top_radiance,
                const int knx, const int kny, const int knz,
                const Sensor_bw& sensor,
                const Array<long long,1>& rays_per_pixel_gpt, const unsigned long long seed, const int max_events,
                const Array<Float,2>& chan_weights,
                Array_gpu<Float,3>& radiance, unsigned long long* n_clamped = nullptr);

        // 3-D longwave heating from cell sensors (rrx_heating3d_render): the scene of trace_rays_thermal without
        // a sensor, and rays_per_cell_gpt (ngpt) on the host, the rays per cell of every g-point (a g-point with none is left out of
        // the result). flux_conv (ncol, nz) in W m-2 is overwritten: the net radiative power that every cell takes up per unit
        // horizontal area, in the layout of a g-point's lay_src. Returns the number of rays dropped at max_events; n_clamped, when given,
        // receives the number of deposits clamped at +-2^20.
        unsigned long long trace_heating(
                const int nx, const int ny, const int nz,
                const Float dx, const Float dy, const Float dz,
                const bool top_at_1,
                const Array_gpu<Float,3>& tau, const Array_gpu<Float,3>& ssa,
                const Array_gpu<int,2>& band_lims_gpt,
                const Array_gpu<Float,3>& cld_tau, const Array_gpu<Float,3>& cld_ssa, const Array_gpu<Float,3>& cld_g,
                const Array_gpu<Float,1>& sfc_emis,
                const Array_gpu<Float,3>& lay_src, const Array_gpu<Float,2>& sfc_src,
                const Array<Float,1>& top_radiance,
                const int knx, const int kny, const int knz,
                const Array<long long,1>& rays_per_cell_gpt, const unsigned long long seed, const int max_events,
                Array_gpu<Float,2>& flux_conv, unsigned long long* n_clamped = nullptr);
};
#endif
