// Raytracer_thermal_gpu: checks the shapes and forwards to rrx_thermal_render, rrx_thermal_render_spectral or rrx_heating3d_render; a
// non-zero status becomes
// std::runtime_error.
#include "Raytracer_thermal.h"
#include "Raytracer_members.h"

namespace
{
// THE SHAPE CHECK of the three functions, up to the output
void check_shapes(const std::string& who, const int nx, const int ny, const int nz,
                  const Array_gpu<Float,3>& tau, const Array_gpu<Float,3>& ssa, const Array_gpu<int,2>& band_lims_gpt,
                  const Array_gpu<Float,3>& cld_tau, const Array_gpu<Float,3>& cld_ssa, const Array_gpu<Float,3>& cld_g,
                  const Array_gpu<Float,1>& sfc_emis, const Array_gpu<Float,3>& lay_src, const Array_gpu<Float,2>& sfc_src,
                  const Array<Float,1>& top_radiance)
{
    if (nx < 0 || ny < 0 || nz < 0) throw std::runtime_error(who + "negative extent");
    const long long ncol = (long long)nx*ny;
    const int ngpt = tau.dim(3), nbnd = band_lims_gpt.dim(2);
    if (tau.dim(1) != ncol || tau.dim(2) != nz) throw std::runtime_error(who + "tau is not (nx ny, nz, ngpt)");
    if (ssa.size() > 0 && ssa.get_dims() != tau.get_dims()) throw std::runtime_error(who + "ssa is neither empty nor (nx ny, nz, ngpt)");
    const bool cloudy = cld_tau.size() > 0;
    if (cloudy && (cld_tau.dim(1) != ncol || cld_tau.dim(2) != nz || cld_tau.dim(3) != nbnd || cld_ssa.get_dims() != cld_tau.get_dims() ||
                   cld_g.get_dims() != cld_tau.get_dims()))
        throw std::runtime_error(who + "the cloud arrays are not (nx ny, nz, nbnd)");
    if (!cloudy && (cld_ssa.size() > 0 || cld_g.size() > 0)) throw std::runtime_error(who + "the cloud arrays are all empty or all given");
    if (sfc_emis.size() != ncol || lay_src.get_dims() != tau.get_dims() || sfc_src.dim(1) != ncol || sfc_src.dim(2) != ngpt)
        throw std::runtime_error(who + "sfc_emis is not (nx ny), lay_src not (nx ny, nz, ngpt) or sfc_src not (nx ny, ngpt)");
    if (top_radiance.size() != 0 && top_radiance.size() != ngpt) throw std::runtime_error(who + "top_radiance is neither empty nor (ngpt)");
}
}

unsigned long long Raytracer_thermal_gpu::trace_rays_thermal(
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
        Array_gpu<Float,3>& radiance, unsigned long long* n_clamped_out)
{
    const std::string who = "Raytracer_thermal_gpu::trace_rays_thermal: ";
    check_shapes(who, nx, ny, nz, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_emis, lay_src, sfc_src, top_radiance);
    const int ngpt = tau.dim(3), nbnd = band_lims_gpt.dim(2);
    const bool cloudy = cld_tau.size() > 0;
    const bool by_band = radiance.dim(3) != 1;          // (one band: its slice is the sum)
    if (sensor.npx < 0 || sensor.npy < 0 || radiance.dim(1) != sensor.npx || radiance.dim(2) != sensor.npy ||
        (radiance.dim(3) != 1 && radiance.dim(3) != nbnd))
        throw std::runtime_error(who + "radiance is not (npx, npy, 1) or (npx, npy, nbnd)");
    const Rt_sensor_numbers numbers(sensor);
    Array_gpu<unsigned long long,1> tallies({2});
    RRX_CALL(rrx_thermal_render, nx, ny, nz, ngpt, nbnd, RrxBool(top_at_1), tau.ptr(), ssa.size() > 0 ? ssa.ptr() : nullptr,
             band_lims_gpt.ptr(), cloudy ? cld_tau.ptr() : nullptr, cloudy ? cld_ssa.ptr() : nullptr, cloudy ? cld_g.ptr() : nullptr,
             dx, dy, dz, sfc_emis.ptr(), lay_src.ptr(), sfc_src.ptr(), top_radiance.size() > 0 ? top_radiance.ptr() : nullptr, knx, kny, knz,
             sensor.sensor_type, sensor.npx, sensor.npy, sensor.fov, numbers.s, rays_per_pixel, seed, max_events,
             RrxBool(by_band), radiance.ptr(), tallies.ptr(), tallies.ptr() + 1);
    if (n_clamped_out != nullptr) *n_clamped_out = tallies({2});
    return tallies({1});
}

unsigned long long Raytracer_thermal_gpu::trace_rays_thermal_spectral(
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
        Array_gpu<Float,3>& radiance, unsigned long long* n_clamped_out)
{
    const std::string who = "Raytracer_thermal_gpu::trace_rays_thermal_spectral: ";
    check_shapes(who, nx, ny, nz, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_emis, lay_src, sfc_src, top_radiance);
    const int ngpt = tau.dim(3), nbnd = band_lims_gpt.dim(2), nchan = chan_weights.dim(2);
    const bool cloudy = cld_tau.size() > 0;
    if (chan_weights.dim(1) != nbnd || nchan < 1) throw std::runtime_error(who + "chan_weights is not (nbnd, nchan >= 1)");
    if (rays_per_pixel_gpt.size() != ngpt) throw std::runtime_error(who + "rays_per_pixel_gpt is not (ngpt)");
    if (sensor.npx < 0 || sensor.npy < 0 || radiance.dim(1) != sensor.npx || radiance.dim(2) != sensor.npy || radiance.dim(3) != nchan)
        throw std::runtime_error(who + "radiance is not (npx, npy, nchan)");
    const Rt_sensor_numbers numbers(sensor);
    Array_gpu<unsigned long long,1> tallies({2});
    RRX_CALL(rrx_thermal_render_spectral, nx, ny, nz, ngpt, nbnd, RrxBool(top_at_1), tau.ptr(), ssa.size() > 0 ? ssa.ptr() : nullptr,
             band_lims_gpt.ptr(), cloudy ? cld_tau.ptr() : nullptr, cloudy ? cld_ssa.ptr() : nullptr, cloudy ? cld_g.ptr() : nullptr,
             dx, dy, dz, sfc_emis.ptr(), lay_src.ptr(), sfc_src.ptr(), top_radiance.size() > 0 ? top_radiance.ptr() : nullptr, knx, kny, knz,
             sensor.sensor_type, sensor.npx, sensor.npy, sensor.fov, numbers.s, rays_per_pixel_gpt.ptr(), seed, max_events,
             nchan, chan_weights.ptr(), radiance.ptr(), tallies.ptr(), tallies.ptr() + 1);
    if (n_clamped_out != nullptr) *n_clamped_out = tallies({2});
    return tallies({1});
}

unsigned long long Raytracer_thermal_gpu::trace_heating(
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
        Array_gpu<Float,2>& flux_conv, unsigned long long* n_clamped_out)
{
    const std::string who = "Raytracer_thermal_gpu::trace_heating: ";
    check_shapes(who, nx, ny, nz, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_emis, lay_src, sfc_src, top_radiance);
    const int ngpt = tau.dim(3), nbnd = band_lims_gpt.dim(2);
    const bool cloudy = cld_tau.size() > 0;
    if (rays_per_cell_gpt.size() != ngpt) throw std::runtime_error(who + "rays_per_cell_gpt is not (ngpt)");
    if (flux_conv.dim(1) != (long long)nx*ny || flux_conv.dim(2) != nz) throw std::runtime_error(who + "flux_conv is not (nx ny, nz)");
    Array_gpu<unsigned long long,1> tallies({2});
    RRX_CALL(rrx_heating3d_render, nx, ny, nz, ngpt, nbnd, RrxBool(top_at_1), tau.ptr(), ssa.size() > 0 ? ssa.ptr() : nullptr,
             band_lims_gpt.ptr(), cloudy ? cld_tau.ptr() : nullptr, cloudy ? cld_ssa.ptr() : nullptr, cloudy ? cld_g.ptr() : nullptr,
             dx, dy, dz, sfc_emis.ptr(), lay_src.ptr(), sfc_src.ptr(), top_radiance.size() > 0 ? top_radiance.ptr() : nullptr, knx, kny, knz,
             rays_per_cell_gpt.ptr(), seed, max_events, flux_conv.ptr(), tallies.ptr(), tallies.ptr() + 1);
    if (n_clamped_out != nullptr) *n_clamped_out = tallies({2});
    return tallies({1});
}
