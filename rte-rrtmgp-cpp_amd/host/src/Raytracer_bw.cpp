// Raytracer_bw_gpu: checks the shapes and forwards to rrx_raytracer_bw or rrx_camera_render_spectral; a non-zero status becomes
// std::runtime_error.
#include "Raytracer_bw.h"
#include "Raytracer_members.h"

namespace
{
// THE SHAPE CHECK of trace_rays_bw
void check_shapes(const std::string& who, const Rt_members& m, const int nx, const int ny, const int nz,
                  const Array_gpu<Float,3>& tau, const Array_gpu<Float,3>& ssa, const Array_gpu<int,2>& band_lims_gpt,
                  const Array_gpu<Float,3>& cld_tau, const Array_gpu<Float,3>& cld_ssa, const Array_gpu<Float,3>& cld_g,
                  const Array_gpu<Float,1>& sfc_albedo, const Array<Float,1>& inc_dir, const Sensor_bw& sensor, const Array_gpu<Float,2>& radiance)
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
    if (sfc_albedo.size() != ncol || inc_dir.size() != ngpt) throw std::runtime_error(who + "sfc_albedo is not (nx ny) or inc_dir is not (ngpt)");
    if (sensor.npx < 0 || sensor.npy < 0 || radiance.dim(1) != sensor.npx || radiance.dim(2) != sensor.npy)
        throw std::runtime_error(who + "radiance is not (npx, npy)");
    m.check_table(who, ncol, nz, nbnd);
    m.check_aerosol(who, ncol, nz, nbnd);
    if (m.has_bg && (m.bg_tau.dim(2) != ngpt || (m.bg_cloudy() && m.bg_cld_tau.dim(2) != nbnd)))
        throw std::runtime_error(who + "the background's arrays are not (nbg, ngpt) and (nbg, nbnd)");
    m.check_bg_aerosol(who, nbnd);
    m.check_no_bg_aerosol_alone(who);
}
}

unsigned long long Raytracer_bw_gpu::trace_rays_bw(
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
        Array_gpu<Float,2>& radiance, unsigned long long* n_clamped_out)
{
    const Rt_members m = RT_MEMBERS;
    check_shapes("Raytracer_bw_gpu::trace_rays_bw: ", m, nx, ny, nz, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_albedo, inc_dir, sensor,
                 radiance);
    const Rt_pointers p(m, cld_tau, cld_ssa, cld_g);
    const Rt_sensor_numbers numbers(sensor);
    Array_gpu<unsigned long long,1> tallies({2});
// the arguments that the four backward loops begin with
#define RT_BW_LOOP_HEAD \
        nx, ny, nz, tau.dim(3), band_lims_gpt.dim(2), RrxBool(top_at_1), tau.ptr(), ssa.ptr(), band_lims_gpt.ptr(), RT_CLOUD(p), \
        dx, dy, dz, sfc_albedo.ptr(), mu0, azimuth, inc_dir.ptr(), knx, kny, knz, \
        sensor.sensor_type, sensor.npx, sensor.npy, sensor.fov, numbers.s, rays_per_pixel, seed, max_events, \
        radiance.ptr(), tallies.ptr(), tallies.ptr() + 1
    if (has_aer)
        RRX_CALL(rrx_raytracer_bw_aer, RT_BW_LOOP_HEAD, RT_TABLE(p), RT_BACKGROUND(p), p.aer[0], p.aer[1], p.aer[2], p.bg_aer[0], p.bg_aer[1], p.bg_aer[2]);
    else if (has_bg)
        RRX_CALL(rrx_raytracer_bw_bg, RT_BW_LOOP_HEAD, RT_TABLE(p), RT_BACKGROUND(p));
    else if (has_table)
        RRX_CALL(rrx_raytracer_bw_phase, RT_BW_LOOP_HEAD, RT_TABLE(p));
    else
        RRX_CALL(rrx_raytracer_bw, RT_BW_LOOP_HEAD);
    if (n_clamped_out != nullptr) *n_clamped_out = tallies({2});
    return tallies({1});
}

unsigned long long Raytracer_bw_gpu::trace_rays_bw_spectral(
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
        Array_gpu<Float,3>& radiance, unsigned long long* n_clamped_out)
{
    const std::string who = "Raytracer_bw_gpu::trace_rays_bw_spectral: ";
    const int nchan = chan_weights.dim(2);
    if (chan_weights.dim(1) != band_lims_gpt.dim(2) || nchan < 1) throw std::runtime_error(who + "chan_weights is not (nbnd, nchan >= 1)");
    if (rays_per_pixel_gpt.size() != tau.dim(3)) throw std::runtime_error(who + "rays_per_pixel_gpt is not (ngpt)");
    if (radiance.dim(3) != nchan) throw std::runtime_error(who + "radiance is not (npx, npy, nchan)");
    const Rt_members m = RT_MEMBERS;
    // (the image of one channel has the shape that trace_rays_bw checks)
    Array_gpu<Float,2> image(radiance.ptr(), {radiance.dim(1), radiance.dim(2)});
    check_shapes(who, m, nx, ny, nz, tau, ssa, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_albedo, inc_dir, sensor, image);
    const Rt_pointers p(m, cld_tau, cld_ssa, cld_g);
    const Rt_sensor_numbers numbers(sensor);
    Array_gpu<unsigned long long,1> tallies({2});
    RRX_CALL(rrx_camera_render_spectral, nx, ny, nz, tau.dim(3), band_lims_gpt.dim(2), RrxBool(top_at_1), tau.ptr(), ssa.ptr(),
             band_lims_gpt.ptr(), RT_CLOUD(p), dx, dy, dz, sfc_albedo.ptr(), mu0, azimuth, inc_dir.ptr(), knx, kny, knz,
             sensor.sensor_type, sensor.npx, sensor.npy, sensor.fov, numbers.s, rays_per_pixel_gpt.ptr(), seed, max_events,
             nchan, chan_weights.ptr(), radiance.ptr(), tallies.ptr(), tallies.ptr() + 1,
             RT_TABLE(p), RT_BACKGROUND(p), p.aer[0], p.aer[1], p.aer[2], p.bg_aer[0], p.bg_aer[1], p.bg_aer[2]);
    if (n_clamped_out != nullptr) *n_clamped_out = tallies({2});
    return tallies({1});
}

void Raytracer_bw_gpu::set_background(const Array<Float,1>& dz_in, const Array_gpu<Float,2>& tau_in, const Array_gpu<Float,2>& ssa_in,
                                      const Array_gpu<Float,2>& ctau_in, const Array_gpu<Float,2>& cssa_in, const Array_gpu<Float,2>& cg_in)
{
    const int nbg = dz_in.size();
    if (nbg < 1 || tau_in.dim(1) != nbg || ssa_in.get_dims() != tau_in.get_dims())
        throw std::runtime_error("Raytracer_bw_gpu::set_background: dz_bg is not (nbg >= 1) or bg_tau, bg_ssa are not (nbg, ngpt)");
    const bool cloudy = ctau_in.size() > 0;
    if (cloudy ? (ctau_in.dim(1) != nbg || cssa_in.get_dims() != ctau_in.get_dims() || cg_in.get_dims() != ctau_in.get_dims())
               : (cssa_in.size() > 0 || cg_in.size() > 0))
        throw std::runtime_error("Raytracer_bw_gpu::set_background: the background's cloud arrays are all empty or all (nbg, nbnd)");
    dz_bg = dz_in; bg_tau = tau_in; bg_ssa = ssa_in; bg_cld_tau = ctau_in; bg_cld_ssa = cssa_in; bg_cld_g = cg_in;
    has_bg = true;
}


void Raytracer_bw_gpu::set_aerosol(const Array_gpu<Float,3>& tau_in, const Array_gpu<Float,3>& ssa_in, const Array_gpu<Float,3>& g_in,
                        const Array_gpu<Float,2>& btau_in, const Array_gpu<Float,2>& bssa_in, const Array_gpu<Float,2>& bg_in)
{
    const bool grid = tau_in.size() > 0, aloft = btau_in.size() > 0;
    if (grid ? (ssa_in.get_dims() != tau_in.get_dims() || g_in.get_dims() != tau_in.get_dims()) : (ssa_in.size() > 0 || g_in.size() > 0))
        throw std::runtime_error("Raytracer_bw_gpu::set_aerosol: the aerosol arrays are all empty or all (nx ny, nz, nbnd)");
    if (aloft ? (bssa_in.get_dims() != btau_in.get_dims() || bg_in.get_dims() != btau_in.get_dims()) : (bssa_in.size() > 0 || bg_in.size() > 0))
        throw std::runtime_error("Raytracer_bw_gpu::set_aerosol: the background's aerosol arrays are all empty or all (nbg, nbnd)");
    if (aloft && !has_bg) throw std::runtime_error("Raytracer_bw_gpu::set_aerosol: a background aerosol needs a background (set_background)");
    if (aloft && btau_in.dim(1) != dz_bg.size())
        throw std::runtime_error("Raytracer_bw_gpu::set_aerosol: the background's aerosol arrays are not (nbg, nbnd)");
    aer_tau = tau_in; aer_ssa = ssa_in; aer_g = g_in; bg_aer_tau = btau_in; bg_aer_ssa = bssa_in; bg_aer_g = bg_in;
    has_aer = grid || aloft;
}

void Raytracer_bw_gpu::set_phase_table(const Array_gpu<Float,1>& mu_in, const Array_gpu<Float,3>& phase_in, const Array_gpu<Float,3>& cdf_in,
                            const Float re0_in, const Float dre_in, const Array_gpu<Float,2>& cld_re_in)
{
    if (mu_in.size() < 2 || phase_in.dim(1) != mu_in.size() || cdf_in.get_dims() != phase_in.get_dims())
        throw std::runtime_error("Raytracer_bw_gpu::set_phase_table: mu is not (nmu >= 2) or phase, cdf are not (nmu, nre, nbnd)");
    if (cld_re_in.size() == 0) throw std::runtime_error("Raytracer_bw_gpu::set_phase_table: cld_re is empty");
    mu = mu_in; phase = phase_in; cdf = cdf_in; cld_re = cld_re_in; re0 = re0_in; dre = dre_in;
    has_table = true;
}
