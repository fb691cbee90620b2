// Raytracer_bw_gpu: checks the shapes and forwards to rrx_raytracer_bw; a non-zero status becomes std::runtime_error.
#include "Raytracer_bw.h"

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
    if (nx < 0 || ny < 0 || nz < 0) throw std::runtime_error("Raytracer_bw_gpu::trace_rays_bw: negative extent");
    const long long ncol = (long long)nx*ny;
    const int ngpt = tau.dim(3);
    const int nbnd = band_lims_gpt.dim(2);
    if (tau.dim(1) != ncol || tau.dim(2) != nz || ssa.get_dims() != tau.get_dims())
        throw std::runtime_error("Raytracer_bw_gpu::trace_rays_bw: tau, ssa are not (nx ny, nz, ngpt)");
    const bool cloudy = cld_tau.size() > 0;
    if (cloudy && (cld_tau.dim(1) != ncol || cld_tau.dim(2) != nz || cld_tau.dim(3) != nbnd || cld_ssa.get_dims() != cld_tau.get_dims() ||
                   cld_g.get_dims() != cld_tau.get_dims()))
        throw std::runtime_error("Raytracer_bw_gpu::trace_rays_bw: the cloud arrays are not (nx ny, nz, nbnd)");
    if (!cloudy && (cld_ssa.size() > 0 || cld_g.size() > 0))
        throw std::runtime_error("Raytracer_bw_gpu::trace_rays_bw: the cloud arrays are all empty or all given");
    if (sfc_albedo.size() != ncol || inc_dir.size() != ngpt)
        throw std::runtime_error("Raytracer_bw_gpu::trace_rays_bw: sfc_albedo is not (nx ny) or inc_dir is not (ngpt)");
    if (sensor.npx < 0 || sensor.npy < 0 || radiance.dim(1) != sensor.npx || radiance.dim(2) != sensor.npy)
        throw std::runtime_error("Raytracer_bw_gpu::trace_rays_bw: radiance is not (npx, npy)");

    const Float numbers[12] = {sensor.position[0], sensor.position[1], sensor.position[2], sensor.e_w[0], sensor.e_w[1], sensor.e_w[2],
                               sensor.e_h[0], sensor.e_h[1], sensor.e_h[2], sensor.e_d[0], sensor.e_d[1], sensor.e_d[2]};
    if (has_table && (cld_re.dim(1) != ncol || cld_re.dim(2) != nz || phase.dim(3) != nbnd))
        throw std::runtime_error("Raytracer_bw_gpu::trace_rays_bw: the phase table's cld_re is not (nx ny, nz) or its tables are not (nmu, nre, nbnd)");
    Array_gpu<unsigned long long,1> tallies({2});
    const bool hazy = has_aer && aer_tau.size() > 0;
    if (hazy && (aer_tau.dim(1) != ncol || aer_tau.dim(2) != nz || aer_tau.dim(3) != nbnd))
        throw std::runtime_error("Raytracer_bw_gpu::trace_rays_bw: the aerosol arrays are not (nx ny, nz, nbnd)");
    if (has_aer)
    {
        const bool bg_cloudy = has_bg && bg_cld_tau.size() > 0, bg_hazy = has_bg && bg_aer_tau.size() > 0;
        const int nbg = has_bg ? dz_bg.size() : 0;
        if (has_bg && (bg_tau.dim(2) != ngpt || (bg_cloudy && bg_cld_tau.dim(2) != nbnd)))
            throw std::runtime_error("Raytracer_bw_gpu::trace_rays_bw: the background's arrays are not (nbg, ngpt) and (nbg, nbnd)");
        if (bg_hazy && (bg_aer_tau.dim(1) != nbg || bg_aer_tau.dim(2) != nbnd))
            throw std::runtime_error("Raytracer_bw_gpu::trace_rays_bw: the background's aerosol arrays are not (nbg, nbnd)");
        if (!has_bg && bg_aer_tau.size() > 0)
            throw std::runtime_error("Raytracer_bw_gpu::trace_rays_bw: a background aerosol is set without a background");
        const Float* none = nullptr;
        RRX_CALL(rrx_raytracer_bw_aer, nx, ny, nz, ngpt, nbnd, RrxBool(top_at_1),
                 tau.ptr(), ssa.ptr(), band_lims_gpt.ptr(),
                 cloudy ? cld_tau.ptr() : nullptr, cloudy ? cld_ssa.ptr() : nullptr, cloudy ? cld_g.ptr() : nullptr,
                 dx, dy, dz, sfc_albedo.ptr(), mu0, azimuth, inc_dir.ptr(), knx, kny, knz,
                 sensor.sensor_type, sensor.npx, sensor.npy, sensor.fov, numbers, rays_per_pixel, seed, max_events,
                 radiance.ptr(), tallies.ptr(), tallies.ptr() + 1,
                 has_table ? mu.dim(1) : 0, has_table ? phase.dim(2) : 0, re0, dre, has_table ? mu.ptr() : none, has_table ? phase.ptr() : none,
                 has_table ? cdf.ptr() : none, has_table ? cld_re.ptr() : none,
                 nbg, has_bg ? dz_bg.ptr() : none, has_bg ? bg_tau.ptr() : none, has_bg ? bg_ssa.ptr() : none,
                 bg_cloudy ? bg_cld_tau.ptr() : none, bg_cloudy ? bg_cld_ssa.ptr() : none, bg_cloudy ? bg_cld_g.ptr() : none,
                 hazy ? aer_tau.ptr() : none, hazy ? aer_ssa.ptr() : none, hazy ? aer_g.ptr() : none,
                 bg_hazy ? bg_aer_tau.ptr() : none, bg_hazy ? bg_aer_ssa.ptr() : none, bg_hazy ? bg_aer_g.ptr() : none);
    }
    else if (has_bg)
    {
        const bool bg_cloudy = bg_cld_tau.size() > 0;
        if (bg_tau.dim(2) != ngpt || (bg_cloudy && bg_cld_tau.dim(2) != nbnd))
            throw std::runtime_error("Raytracer_bw_gpu::trace_rays_bw: the background's arrays are not (nbg, ngpt) and (nbg, nbnd)");
        const Float* none = nullptr;
        RRX_CALL(rrx_raytracer_bw_bg, nx, ny, nz, ngpt, nbnd, RrxBool(top_at_1),
                 tau.ptr(), ssa.ptr(), band_lims_gpt.ptr(),
                 cloudy ? cld_tau.ptr() : nullptr, cloudy ? cld_ssa.ptr() : nullptr, cloudy ? cld_g.ptr() : nullptr,
                 dx, dy, dz, sfc_albedo.ptr(), mu0, azimuth, inc_dir.ptr(), knx, kny, knz,
                 sensor.sensor_type, sensor.npx, sensor.npy, sensor.fov, numbers, rays_per_pixel, seed, max_events,
                 radiance.ptr(), tallies.ptr(), tallies.ptr() + 1,
                 has_table ? mu.dim(1) : 0, has_table ? phase.dim(2) : 0, re0, dre, has_table ? mu.ptr() : none, has_table ? phase.ptr() : none,
                 has_table ? cdf.ptr() : none, has_table ? cld_re.ptr() : none,
                 dz_bg.size(), dz_bg.ptr(), bg_tau.ptr(), bg_ssa.ptr(), bg_cloudy ? bg_cld_tau.ptr() : none,
                 bg_cloudy ? bg_cld_ssa.ptr() : none, bg_cloudy ? bg_cld_g.ptr() : none);
    }
    else if (has_table)
        RRX_CALL(rrx_raytracer_bw_phase, nx, ny, nz, ngpt, nbnd, RrxBool(top_at_1),
                 tau.ptr(), ssa.ptr(), band_lims_gpt.ptr(),
                 cloudy ? cld_tau.ptr() : nullptr, cloudy ? cld_ssa.ptr() : nullptr, cloudy ? cld_g.ptr() : nullptr,
                 dx, dy, dz, sfc_albedo.ptr(), mu0, azimuth, inc_dir.ptr(), knx, kny, knz,
                 sensor.sensor_type, sensor.npx, sensor.npy, sensor.fov, numbers, rays_per_pixel, seed, max_events,
                 radiance.ptr(), tallies.ptr(), tallies.ptr() + 1,
                 mu.dim(1), phase.dim(2), re0, dre, mu.ptr(), phase.ptr(), cdf.ptr(), cld_re.ptr());
    else
    RRX_CALL(rrx_raytracer_bw, nx, ny, nz, ngpt, nbnd, RrxBool(top_at_1),
             tau.ptr(), ssa.ptr(), band_lims_gpt.ptr(),
             cloudy ? cld_tau.ptr() : nullptr, cloudy ? cld_ssa.ptr() : nullptr, cloudy ? cld_g.ptr() : nullptr,
             dx, dy, dz, sfc_albedo.ptr(), mu0, azimuth, inc_dir.ptr(), knx, kny, knz,
             sensor.sensor_type, sensor.npx, sensor.npy, sensor.fov, numbers, rays_per_pixel, seed, max_events,
             radiance.ptr(), tallies.ptr(), tallies.ptr() + 1);
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
