// Rte_lw_gpu / Rte_sw_gpu: /root/reference/src_cuda/Rte_lw.cu:60-159 and src_cuda/Rte_sw.cu:116-185.
#include "Rte_lw.h"
#include "Rte_sw.h"
#include "rte_solver_kernels_cuda.h"

namespace
{
    // Gauss-Jacobi-5 quadrature, Table 1 of R. J. Hogan 2023, doi:10.1002/qj.4598 (as in src/Rte_lw.cpp:140-152)
    constexpr int max_gauss_pts = 4;
    const std::vector<Float> gauss_Ds_v = {
        1./0.6096748751, 0.            , 0.             , 0.,
        1./0.2509907356, 1/0.7908473988, 0.             , 0.,
        1./0.1024922169, 1/0.4417960320, 1./0.8633751621, 0.,
        1./0.0454586727, 1/0.2322334416, 1./0.5740198775, 1./0.903077597 };
    const std::vector<Float> gauss_wts_v = {
        1.,           0.,           0.,           0.,
        0.2300253764, 0.7699746236, 0.,           0.,
        0.0437820218, 0.3875796738, 0.5686383044, 0.,
        0.0092068785, 0.1285704278, 0.4323381850, 0.4298845087 };

    void expand(const std::unique_ptr<Optical_props_arry_gpu>& ops, const Array_gpu<Float,2>& arr_in, Array_gpu<Float,2>& arr_out)
    {
        RRX_CALL(rrx_expand_and_transpose, arr_in.dim(2), ops->get_nband(), ops->get_band_lims_gpoint_gpu().ptr(), arr_in.ptr(), arr_out.ptr());
    }

    // optional outputs of the by-band solvers: an array of size 0 is not written
    template<int N> Float* opt(Array_gpu<Float,N>& a) { return a.size() == 0 ? nullptr : a.ptr(); }

    // flux arrays with one slab per band (fewer bands than g-points) select the by-band form
    bool is_byband(const std::unique_ptr<Optical_props_arry_gpu>& ops, const Array_gpu<Float,3>& flux)
    {
        return flux.dim(3) == ops->get_nband() && ops->get_nband() < ops->get_ngpt();
    }
}

void Rte_lw_gpu::rte_lw(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
        const Bool top_at_1,
        const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis,
        const Array_gpu<Float,2>& inc_flux,
        Array_gpu<Float,3>& gpt_flux_up,
        Array_gpu<Float,3>& gpt_flux_dn,
        const int n_gauss_angles)
{
    solve(optical_props, top_at_1, sources, sfc_emis, inc_flux, gpt_flux_up, gpt_flux_dn, nullptr, n_gauss_angles);
}

void Rte_lw_gpu::rte_lw(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
        const Bool top_at_1,
        const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis,
        const Array_gpu<Float,2>& inc_flux,
        Array_gpu<Float,3>& gpt_flux_up,
        Array_gpu<Float,3>& gpt_flux_dn,
        Array_gpu<Float,3>& flux_up_jac,
        const int n_gauss_angles)
{
    if (is_byband(optical_props, gpt_flux_up)) throw std::runtime_error("rte_lw: no Jacobian for by-band flux arrays");
    if (flux_up_jac.dim(1) != gpt_flux_up.dim(1) || flux_up_jac.dim(2) != gpt_flux_up.dim(2) || flux_up_jac.dim(3) != gpt_flux_up.dim(3))
        throw std::runtime_error("rte_lw: flux_up_jac must be shaped like the flux arrays");
    solve(optical_props, top_at_1, sources, sfc_emis, inc_flux, gpt_flux_up, gpt_flux_dn, &flux_up_jac, n_gauss_angles);
}

void Rte_lw_gpu::rte_lw_optimal(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis, const Array_gpu<Float,2>& inc_flux, const Array_gpu<Float,2>& optimal_angle_fit,
        Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn, Array_gpu<Float,3>* flux_up_jac, const int n_gauss_angles)
{
    if (n_gauss_angles != 1) throw std::runtime_error("rte_lw_optimal: optimal angles need one quadrature angle");
    if (optimal_angle_fit.dim(1) != 2 || optimal_angle_fit.dim(2) != optical_props->get_nband())
        throw std::runtime_error("rte_lw_optimal: optimal_angle_fit must be (2, nbnd)");
    solve(optical_props, top_at_1, sources, sfc_emis, inc_flux, gpt_flux_up, gpt_flux_dn, flux_up_jac, 1, &optimal_angle_fit, nullptr);
}

void Rte_lw_gpu::rte_lw_Ds(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis, const Array_gpu<Float,2>& inc_flux, const Array_gpu<Float,2>& lw_Ds,
        Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn, Array_gpu<Float,3>* flux_up_jac, const int n_gauss_angles)
{
    if (n_gauss_angles != 1) throw std::runtime_error("rte_lw_Ds: lw_Ds needs one quadrature angle");
    if (lw_Ds.dim(1) != optical_props->get_ncol() || lw_Ds.dim(2) != optical_props->get_ngpt())
        throw std::runtime_error("rte_lw_Ds: lw_Ds must be (ncol, ngpt)");
    solve(optical_props, top_at_1, sources, sfc_emis, inc_flux, gpt_flux_up, gpt_flux_dn, flux_up_jac, 1, nullptr, &lw_Ds);
}

// flux_up_jac: null = no Jacobian. optimal_angle_fit (2, nbnd) or lw_Ds (ncol, ngpt), at most one of them: the secants of the one angle
void Rte_lw_gpu::solve(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis, const Array_gpu<Float,2>& inc_flux,
        Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn, Array_gpu<Float,3>* flux_up_jac, const int n_gauss_angles,
        const Array_gpu<Float,2>* optimal_angle_fit, const Array_gpu<Float,2>* lw_Ds)
{
    if (n_gauss_angles < 1 || n_gauss_angles > max_gauss_pts) throw std::runtime_error("rte_lw: n_gauss_angles must be 1..4");
    const bool own_secants = optimal_angle_fit != nullptr || lw_Ds != nullptr;
    if (own_secants && is_byband(optical_props, gpt_flux_up))
        throw std::runtime_error("rte_lw: no by-band flux arrays with optimal angles / lw_Ds");
    if (own_secants && flux_up_jac != nullptr &&
        (flux_up_jac->dim(1) != gpt_flux_up.dim(1) || flux_up_jac->dim(2) != gpt_flux_up.dim(2) || flux_up_jac->dim(3) != gpt_flux_up.dim(3)))
        throw std::runtime_error("rte_lw: flux_up_jac must be shaped like the flux arrays");
    if (is_byband(optical_props, gpt_flux_up))
    {
        if (n_gauss_angles != 1) throw std::runtime_error("rte_lw: by-band fluxes need one quadrature angle");
        Array_gpu<Float,3> no3; Array_gpu<Float,2> no_up, no_dn;
        rte_lw_byband(optical_props, top_at_1, sources, sfc_emis, inc_flux, gpt_flux_up, gpt_flux_dn, no3, no_up, no_dn);
        return;
    }
    const int ncol = optical_props->get_ncol();
    const int nlay = optical_props->get_nlay();
    const int ngpt = optical_props->get_ngpt();

    Array_gpu<Float,2> sfc_emis_gpt({ncol, ngpt});
    expand_and_transpose(optical_props, sfc_emis, sfc_emis_gpt);

    if (gauss_angles_cached != n_gauss_angles)
    {
        gauss_Ds_gpu = Array_gpu<Float,2>(Array<Float,2>(gauss_Ds_v, {max_gauss_pts, max_gauss_pts}));
        const Array<Float,2> gauss_wts(gauss_wts_v, {max_gauss_pts, max_gauss_pts});
        gauss_wts_gpu = Array_gpu<Float,2>(gauss_wts.subset({{ {1, n_gauss_angles}, {n_gauss_angles, n_gauss_angles} }}));
        gauss_angles_cached = n_gauss_angles;
    }
    const Array_gpu<Float,2>& gauss_Ds = gauss_Ds_gpu;
    const Array_gpu<Float,2>& gauss_wts_subset = gauss_wts_gpu;

    const Bool do_broadband = (gpt_flux_up.dim(3) == 1 && ngpt != 1);
    const Bool do_jacobians = flux_up_jac != nullptr;
    const Float* inc_flux_ptr = (inc_flux.size() == 0) ? nullptr : inc_flux.ptr();

    if (optimal_angle_fit != nullptr && sources.holds_fractions() && do_broadband)
    {
        // the fused solver forms the optimal-angle secants from the g-point it holds: no secants array at all
        Rte_solver_kernels_cuda::lw_solver_noscat_fractions_optimal(
                ncol, nlay, ngpt, optical_props->get_nband(), top_at_1, gauss_wts_subset.ptr(),
                optical_props->get_tau().ptr(), sources.get_planck_frac().ptr(), sources.get_planck_lay().ptr(), sources.get_planck_lev().ptr(),
                optical_props->get_gpoint_bands_gpu().ptr(), optimal_angle_fit->ptr(), sfc_emis_gpt.ptr(), sources.get_sfc_source().ptr(),
                inc_flux_ptr, gpt_flux_up.ptr(), gpt_flux_dn.ptr(), do_jacobians ? sources.get_sfc_source_jac().ptr() : nullptr,
                do_jacobians ? flux_up_jac->ptr() : nullptr, nullptr);
        return;
    }
    // the secants of the solve: the caller's lw_Ds as they are, else an array of this call (optimal angles or the Gauss nodes)
    Array_gpu<Float,3> secants_own;
    if (lw_Ds == nullptr) secants_own.set_dims({ncol, ngpt, n_gauss_angles});
    Array_gpu<Float,3> secants(lw_Ds != nullptr ? const_cast<Float*>(lw_Ds->ptr()) : secants_own.ptr(), {ncol, ngpt, n_gauss_angles});
    if (optimal_angle_fit != nullptr)
        Rte_solver_kernels_cuda::lw_optimal_secants(ncol, nlay, ngpt, optical_props->get_nband(), optical_props->get_gpoint_bands_gpu().ptr(),
                                                    optimal_angle_fit->ptr(), optical_props->get_tau().ptr(), secants.ptr());
    else if (lw_Ds == nullptr)
        Rte_solver_kernels_cuda::lw_secants_array(ncol, ngpt, n_gauss_angles, max_gauss_pts, gauss_Ds.ptr(), secants.ptr());

    // Planck-lite state (set by Gas_optics_rrtmgp_gpu::gas_optics): the broadband solver forms the sources itself
    if (sources.holds_fractions() && do_broadband && n_gauss_angles > 1)
    {
        // several quadrature angles: one kernel reads each g-point once and solves it n_gauss_angles times (Jacobian pair optional)
        RRX_CALL(rrx_lw_solver_noscat_fractions_angles, ncol, nlay, ngpt, top_at_1, n_gauss_angles, secants.ptr(), gauss_wts_subset.ptr(),
                 optical_props->get_tau().ptr(), sources.get_planck_frac().ptr(), sources.get_planck_lay().ptr(), sources.get_planck_lev().ptr(),
                 optical_props->get_gpoint_bands_gpu().ptr(), sfc_emis_gpt.ptr(), sources.get_sfc_source().ptr(), inc_flux_ptr,
                 gpt_flux_up.ptr(), gpt_flux_dn.ptr(), do_jacobians ? sources.get_sfc_source_jac().ptr() : nullptr,
                 do_jacobians ? flux_up_jac->ptr() : nullptr);
        return;
    }
    if (sources.holds_fractions() && do_broadband && n_gauss_angles == 1 && do_jacobians)
    {
        RRX_CALL(rrx_lw_solver_noscat_fractions_jac, ncol, nlay, ngpt, top_at_1, secants.ptr(), gauss_wts_subset.ptr(),
                 optical_props->get_tau().ptr(), sources.get_planck_frac().ptr(), sources.get_planck_lay().ptr(), sources.get_planck_lev().ptr(),
                 optical_props->get_gpoint_bands_gpu().ptr(), sfc_emis_gpt.ptr(), sources.get_sfc_source().ptr(), inc_flux_ptr,
                 gpt_flux_up.ptr(), gpt_flux_dn.ptr(), sources.get_sfc_source_jac().ptr(), flux_up_jac->ptr());
        return;
    }
    if (sources.holds_fractions() && do_broadband && n_gauss_angles == 1)
    {
        RRX_CALL(rrx_lw_solver_noscat_fractions, ncol, nlay, ngpt, top_at_1, secants.ptr(), gauss_wts_subset.ptr(),
                 optical_props->get_tau().ptr(), sources.get_planck_frac().ptr(), sources.get_planck_lay().ptr(), sources.get_planck_lev().ptr(),
                 optical_props->get_gpoint_bands_gpu().ptr(), sfc_emis_gpt.ptr(), sources.get_sfc_source().ptr(), inc_flux_ptr,
                 gpt_flux_up.ptr(), gpt_flux_dn.ptr());
        return;
    }
    // general solver: per-g-point Jacobians (broadband flux arrays: into a block array, then summed over the g-points)
    Array_gpu<Float,3> jac_bb;
    Float* jac_gpt = do_jacobians ? flux_up_jac->ptr() : nullptr;
    if (do_jacobians && do_broadband) { jac_bb.set_dims({ncol, nlay + 1, ngpt}); jac_gpt = jac_bb.ptr(); }
    Rte_solver_kernels_cuda::lw_solver_noscat(
            ncol, nlay, ngpt, top_at_1, n_gauss_angles,
            secants.ptr(), gauss_wts_subset.ptr(),
            optical_props->get_tau().ptr(),
            sources.get_lay_source().ptr(), sources.get_lev_source().ptr(),
            sfc_emis_gpt.ptr(), sources.get_sfc_source().ptr(),
            inc_flux_ptr,
            gpt_flux_up.ptr(), gpt_flux_dn.ptr(),
            do_broadband, gpt_flux_up.ptr(), gpt_flux_dn.ptr(),
            do_jacobians, do_jacobians ? sources.get_sfc_source_jac().ptr() : nullptr, jac_gpt);
    if (jac_bb.size() != 0) RRX_CALL(rrx_sum_broadband, ncol, nlay + 1, ngpt, jac_gpt, flux_up_jac->ptr());
}

void Rte_lw_gpu::rte_lw_byband(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
        const Bool top_at_1,
        const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis,
        const Array_gpu<Float,2>& inc_flux,
        Array_gpu<Float,3>& bnd_flux_up,
        Array_gpu<Float,3>& bnd_flux_dn,
        Array_gpu<Float,3>& bnd_flux_net,
        Array_gpu<Float,2>& flux_up,
        Array_gpu<Float,2>& flux_dn)
{
    // (the by-band solver forms the sources from the Planck fractions: the reference-shaped lay_source / lev_source have no by-band form)
    if (!sources.holds_fractions()) throw std::runtime_error("rte_lw_byband: needs the Planck-lite sources (enable_planck_lite)");
    const int ncol = optical_props->get_ncol();
    const int nlay = optical_props->get_nlay();
    const int ngpt = optical_props->get_ngpt();
    const int nbnd = optical_props->get_nband();
    if (bnd_flux_up.dim(3) != nbnd || bnd_flux_dn.dim(3) != nbnd) throw std::runtime_error("rte_lw_byband: flux arrays need one slab per band");

    Array_gpu<Float,2> sfc_emis_gpt({ncol, ngpt});
    expand_and_transpose(optical_props, sfc_emis, sfc_emis_gpt);
    if (gauss_angles_cached != 1)
    {
        gauss_Ds_gpu = Array_gpu<Float,2>(Array<Float,2>(gauss_Ds_v, {max_gauss_pts, max_gauss_pts}));
        const Array<Float,2> gauss_wts(gauss_wts_v, {max_gauss_pts, max_gauss_pts});
        gauss_wts_gpu = Array_gpu<Float,2>(gauss_wts.subset({{ {1, 1}, {1, 1} }}));
        gauss_angles_cached = 1;
    }
    Array_gpu<Float,3> secants({ncol, ngpt, 1});
    Rte_solver_kernels_cuda::lw_secants_array(ncol, ngpt, 1, max_gauss_pts, gauss_Ds_gpu.ptr(), secants.ptr());
    const Float* inc_flux_ptr = (inc_flux.size() == 0) ? nullptr : inc_flux.ptr();
    RRX_CALL(rrx_lw_solver_noscat_fractions_byband, ncol, nlay, ngpt, nbnd, top_at_1, secants.ptr(), gauss_wts_gpu.ptr(),
             optical_props->get_tau().ptr(), sources.get_planck_frac().ptr(), sources.get_planck_lay().ptr(), sources.get_planck_lev().ptr(),
             optical_props->get_gpoint_bands_gpu().ptr(), optical_props->get_band_lims_gpoint_gpu().ptr(),
             sfc_emis_gpt.ptr(), sources.get_sfc_source().ptr(), inc_flux_ptr,
             bnd_flux_up.ptr(), bnd_flux_dn.ptr(), opt(bnd_flux_net), opt(flux_up), opt(flux_dn));
}

void Rte_lw_gpu::rte_lw_2stream(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis, const Array_gpu<Float,2>& inc_flux, const Optical_props_2str_gpu* cloud,
        Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn)
{
    if (!sources.holds_fractions()) throw std::runtime_error("rte_lw_2stream: needs the Planck-lite sources (enable_planck_lite)");
    if (gpt_flux_up.dim(3) != 1 || gpt_flux_dn.dim(3) != 1) throw std::runtime_error("rte_lw_2stream: needs broadband flux arrays (third dimension 1)");
    const int ncol = optical_props->get_ncol();
    const int nlay = optical_props->get_nlay();
    const int ngpt = optical_props->get_ngpt();
    const int nbnd = optical_props->get_nband();
    if (cloud != nullptr && (cloud->get_ncol() != ncol || cloud->get_nlay() != nlay || cloud->get_tau().dim(3) != nbnd))
        throw std::runtime_error("rte_lw_2stream: the cloud optical properties must be (ncol, nlay, nbnd)");

    Array_gpu<Float,2> sfc_emis_gpt({ncol, ngpt});
    expand_and_transpose(optical_props, sfc_emis, sfc_emis_gpt);
    const Float* inc_flux_ptr = (inc_flux.size() == 0) ? nullptr : inc_flux.ptr();
    const Float* none = nullptr;
    RRX_CALL(rrx_lw_solver_2stream_fractions, ncol, nlay, ngpt, nbnd, top_at_1,
             optical_props->get_tau().ptr(), sources.get_planck_frac().ptr(), sources.get_planck_lev().ptr(),
             optical_props->get_gpoint_bands_gpu().ptr(), optical_props->get_band_lims_gpoint_gpu().ptr(),
             cloud ? cloud->get_tau().ptr() : none, cloud ? cloud->get_ssa().ptr() : none, cloud ? cloud->get_g().ptr() : none,
             sfc_emis_gpt.ptr(), sources.get_sfc_source().ptr(), inc_flux_ptr, gpt_flux_up.ptr(), gpt_flux_dn.ptr());
}

void Rte_lw_gpu::rte_lw_rescaled(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis, const Array_gpu<Float,2>& inc_flux, const Optical_props_2str_gpu* cloud,
        Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn)
{
    if (!sources.holds_fractions()) throw std::runtime_error("rte_lw_rescaled: needs the Planck-lite sources (enable_planck_lite)");
    if (gpt_flux_up.dim(3) != 1 || gpt_flux_dn.dim(3) != 1) throw std::runtime_error("rte_lw_rescaled: needs broadband flux arrays (third dimension 1)");
    const int ncol = optical_props->get_ncol();
    const int nlay = optical_props->get_nlay();
    const int ngpt = optical_props->get_ngpt();
    const int nbnd = optical_props->get_nband();
    if (cloud != nullptr && (cloud->get_ncol() != ncol || cloud->get_nlay() != nlay || cloud->get_tau().dim(3) != nbnd))
        throw std::runtime_error("rte_lw_rescaled: the cloud optical properties must be (ncol, nlay, nbnd)");

    Array_gpu<Float,2> sfc_emis_gpt({ncol, ngpt});
    expand_and_transpose(optical_props, sfc_emis, sfc_emis_gpt);
    if (gauss_angles_cached != 1)
    {
        gauss_Ds_gpu = Array_gpu<Float,2>(Array<Float,2>(gauss_Ds_v, {max_gauss_pts, max_gauss_pts}));
        const Array<Float,2> gauss_wts(gauss_wts_v, {max_gauss_pts, max_gauss_pts});
        gauss_wts_gpu = Array_gpu<Float,2>(gauss_wts.subset({{ {1, 1}, {1, 1} }}));
        gauss_angles_cached = 1;
    }
    Array_gpu<Float,3> secants({ncol, ngpt, 1});
    Rte_solver_kernels_cuda::lw_secants_array(ncol, ngpt, 1, max_gauss_pts, gauss_Ds_gpu.ptr(), secants.ptr());
    const Float* inc_flux_ptr = (inc_flux.size() == 0) ? nullptr : inc_flux.ptr();
    const Float* none = nullptr;
    RRX_CALL(rrx_lw_solver_noscat_fractions_rescaled, ncol, nlay, ngpt, nbnd, top_at_1, secants.ptr(), gauss_wts_gpu.ptr(),
             optical_props->get_tau().ptr(), sources.get_planck_frac().ptr(), sources.get_planck_lay().ptr(), sources.get_planck_lev().ptr(),
             optical_props->get_gpoint_bands_gpu().ptr(), optical_props->get_band_lims_gpoint_gpu().ptr(),
             cloud ? cloud->get_tau().ptr() : none, cloud ? cloud->get_ssa().ptr() : none, cloud ? cloud->get_g().ptr() : none,
             sfc_emis_gpt.ptr(), sources.get_sfc_source().ptr(), inc_flux_ptr, gpt_flux_up.ptr(), gpt_flux_dn.ptr());
}

void Rte_lw_gpu::expand_and_transpose(const std::unique_ptr<Optical_props_arry_gpu>& ops, const Array_gpu<Float,2> arr_in, Array_gpu<Float,2>& arr_out)
{ expand(ops, arr_in, arr_out); }

void Rte_sw_gpu::rte_sw(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
        const Bool top_at_1,
        const Array_gpu<Float,1>& mu0,
        const Array_gpu<Float,2>& inc_flux_dir,
        const Array_gpu<Float,2>& sfc_alb_dir,
        const Array_gpu<Float,2>& sfc_alb_dif,
        const Array_gpu<Float,2>& inc_flux_dif,
        Array_gpu<Float,3>& gpt_flux_up,
        Array_gpu<Float,3>& gpt_flux_dn,
        Array_gpu<Float,3>& gpt_flux_dir)
{
    if (is_byband(optical_props, gpt_flux_up))
    {
        Array_gpu<Float,3> no3; Array_gpu<Float,2> no_up, no_dn, no_dir;
        rte_sw_byband(optical_props, top_at_1, mu0, inc_flux_dir, sfc_alb_dir, sfc_alb_dif, inc_flux_dif, gpt_flux_up, gpt_flux_dn,
                      gpt_flux_dir, no3, no_up, no_dn, no_dir);
        return;
    }
    const int ncol = optical_props->get_ncol();
    const int nlay = optical_props->get_nlay();
    const int ngpt = optical_props->get_ngpt();

    Array_gpu<Float,2> sfc_alb_dir_gpt({ncol, ngpt});
    Array_gpu<Float,2> sfc_alb_dif_gpt({ncol, ngpt});
    expand_and_transpose(optical_props, sfc_alb_dir, sfc_alb_dir_gpt);
    expand_and_transpose(optical_props, sfc_alb_dif, sfc_alb_dif_gpt);

    const Bool has_dif_bc = (inc_flux_dif.size() > 0);
    const Bool do_broadband = (gpt_flux_up.dim(3) == 1 && ngpt != 1);
    const Float* inc_flux_dif_ptr = has_dif_bc ? inc_flux_dif.ptr() : nullptr;

    Rte_solver_kernels_cuda::sw_solver_2stream(
            ncol, nlay, ngpt, top_at_1,
            optical_props->get_tau().ptr(), optical_props->get_ssa().ptr(),
            // "no g" is native to the fused broadband solver; the per-g-point forms read an array (zeros materialised here)
            do_broadband ? optical_props->get_g_or_null() : static_cast<const Float*>(optical_props->get_g().ptr()),
            mu0.ptr(),
            sfc_alb_dir_gpt.ptr(), sfc_alb_dif_gpt.ptr(),
            inc_flux_dir.ptr(),
            gpt_flux_up.ptr(), gpt_flux_dn.ptr(), gpt_flux_dir.ptr(),
            has_dif_bc, inc_flux_dif_ptr,
            do_broadband, gpt_flux_up.ptr(), gpt_flux_dn.ptr(), gpt_flux_dir.ptr());
}

void Rte_sw_gpu::rte_sw_byband(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
        const Bool top_at_1,
        const Array_gpu<Float,1>& mu0,
        const Array_gpu<Float,2>& inc_flux_dir,
        const Array_gpu<Float,2>& sfc_alb_dir,
        const Array_gpu<Float,2>& sfc_alb_dif,
        const Array_gpu<Float,2>& inc_flux_dif,
        Array_gpu<Float,3>& bnd_flux_up,
        Array_gpu<Float,3>& bnd_flux_dn,
        Array_gpu<Float,3>& bnd_flux_dir,
        Array_gpu<Float,3>& bnd_flux_net,
        Array_gpu<Float,2>& flux_up,
        Array_gpu<Float,2>& flux_dn,
        Array_gpu<Float,2>& flux_dir)
{
    const int ncol = optical_props->get_ncol();
    const int nlay = optical_props->get_nlay();
    const int ngpt = optical_props->get_ngpt();
    const int nbnd = optical_props->get_nband();
    if (bnd_flux_up.dim(3) != nbnd || bnd_flux_dn.dim(3) != nbnd || bnd_flux_dir.dim(3) != nbnd)
        throw std::runtime_error("rte_sw_byband: flux arrays need one slab per band");

    Array_gpu<Float,2> sfc_alb_dir_gpt({ncol, ngpt});
    Array_gpu<Float,2> sfc_alb_dif_gpt({ncol, ngpt});
    expand_and_transpose(optical_props, sfc_alb_dir, sfc_alb_dir_gpt);
    expand_and_transpose(optical_props, sfc_alb_dif, sfc_alb_dif_gpt);
    const Bool has_dif_bc = (inc_flux_dif.size() > 0);
    RRX_CALL(rrx_sw_solver_2stream_byband, ncol, nlay, ngpt, nbnd, top_at_1,
             optical_props->get_tau().ptr(), optical_props->get_ssa().ptr(), optical_props->get_g_or_null(), mu0.ptr(),
             sfc_alb_dir_gpt.ptr(), sfc_alb_dif_gpt.ptr(), inc_flux_dir.ptr(), has_dif_bc, has_dif_bc ? inc_flux_dif.ptr() : nullptr,
             optical_props->get_band_lims_gpoint_gpu().ptr(),
             bnd_flux_up.ptr(), bnd_flux_dn.ptr(), bnd_flux_dir.ptr(), opt(bnd_flux_net), opt(flux_up), opt(flux_dn), opt(flux_dir));
}

// mu0 (ncol, nlay): a cosine of the solar zenith angle per layer. The two methods above with the by-layer entries of
// the device layer in the place of the 1-D ones.
void Rte_sw_gpu::rte_sw(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
        const Bool top_at_1,
        const Array_gpu<Float,2>& mu0,
        const Array_gpu<Float,2>& inc_flux_dir,
        const Array_gpu<Float,2>& sfc_alb_dir,
        const Array_gpu<Float,2>& sfc_alb_dif,
        const Array_gpu<Float,2>& inc_flux_dif,
        Array_gpu<Float,3>& gpt_flux_up,
        Array_gpu<Float,3>& gpt_flux_dn,
        Array_gpu<Float,3>& gpt_flux_dir)
{
    if (is_byband(optical_props, gpt_flux_up))
    {
        Array_gpu<Float,3> no3; Array_gpu<Float,2> no_up, no_dn, no_dir;
        rte_sw_byband(optical_props, top_at_1, mu0, inc_flux_dir, sfc_alb_dir, sfc_alb_dif, inc_flux_dif, gpt_flux_up, gpt_flux_dn,
                      gpt_flux_dir, no3, no_up, no_dn, no_dir);
        return;
    }
    const int ncol = optical_props->get_ncol();
    const int nlay = optical_props->get_nlay();
    const int ngpt = optical_props->get_ngpt();
    if (mu0.dim(1) != ncol || mu0.dim(2) != nlay) throw std::runtime_error("rte_sw: mu0 by layer must be (ncol, nlay)");

    Array_gpu<Float,2> sfc_alb_dir_gpt({ncol, ngpt});
    Array_gpu<Float,2> sfc_alb_dif_gpt({ncol, ngpt});
    expand_and_transpose(optical_props, sfc_alb_dir, sfc_alb_dir_gpt);
    expand_and_transpose(optical_props, sfc_alb_dif, sfc_alb_dif_gpt);

    const Bool has_dif_bc = (inc_flux_dif.size() > 0);
    const Bool do_broadband = (gpt_flux_up.dim(3) == 1 && ngpt != 1);
    RRX_CALL(rrx_sw_solver_2stream_mu0lay, ncol, nlay, ngpt, top_at_1,
             optical_props->get_tau().ptr(), optical_props->get_ssa().ptr(),
             do_broadband ? optical_props->get_g_or_null() : static_cast<const Float*>(optical_props->get_g().ptr()),
             mu0.ptr(), sfc_alb_dir_gpt.ptr(), sfc_alb_dif_gpt.ptr(), inc_flux_dir.ptr(),
             gpt_flux_up.ptr(), gpt_flux_dn.ptr(), gpt_flux_dir.ptr(), has_dif_bc, has_dif_bc ? inc_flux_dif.ptr() : nullptr,
             do_broadband, gpt_flux_up.ptr(), gpt_flux_dn.ptr(), gpt_flux_dir.ptr());
}

void Rte_sw_gpu::rte_sw_byband(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
        const Bool top_at_1,
        const Array_gpu<Float,2>& mu0,
        const Array_gpu<Float,2>& inc_flux_dir,
        const Array_gpu<Float,2>& sfc_alb_dir,
        const Array_gpu<Float,2>& sfc_alb_dif,
        const Array_gpu<Float,2>& inc_flux_dif,
        Array_gpu<Float,3>& bnd_flux_up,
        Array_gpu<Float,3>& bnd_flux_dn,
        Array_gpu<Float,3>& bnd_flux_dir,
        Array_gpu<Float,3>& bnd_flux_net,
        Array_gpu<Float,2>& flux_up,
        Array_gpu<Float,2>& flux_dn,
        Array_gpu<Float,2>& flux_dir)
{
    const int ncol = optical_props->get_ncol();
    const int nlay = optical_props->get_nlay();
    const int ngpt = optical_props->get_ngpt();
    const int nbnd = optical_props->get_nband();
    if (mu0.dim(1) != ncol || mu0.dim(2) != nlay) throw std::runtime_error("rte_sw_byband: mu0 by layer must be (ncol, nlay)");
    if (bnd_flux_up.dim(3) != nbnd || bnd_flux_dn.dim(3) != nbnd || bnd_flux_dir.dim(3) != nbnd)
        throw std::runtime_error("rte_sw_byband: flux arrays need one slab per band");

    Array_gpu<Float,2> sfc_alb_dir_gpt({ncol, ngpt});
    Array_gpu<Float,2> sfc_alb_dif_gpt({ncol, ngpt});
    expand_and_transpose(optical_props, sfc_alb_dir, sfc_alb_dir_gpt);
    expand_and_transpose(optical_props, sfc_alb_dif, sfc_alb_dif_gpt);
    const Bool has_dif_bc = (inc_flux_dif.size() > 0);
    RRX_CALL(rrx_sw_solver_2stream_byband_mu0lay, ncol, nlay, ngpt, nbnd, top_at_1,
             optical_props->get_tau().ptr(), optical_props->get_ssa().ptr(), optical_props->get_g_or_null(), mu0.ptr(),
             sfc_alb_dir_gpt.ptr(), sfc_alb_dif_gpt.ptr(), inc_flux_dir.ptr(), has_dif_bc, has_dif_bc ? inc_flux_dif.ptr() : nullptr,
             optical_props->get_band_lims_gpoint_gpu().ptr(),
             bnd_flux_up.ptr(), bnd_flux_dn.ptr(), bnd_flux_dir.ptr(), opt(bnd_flux_net), opt(flux_up), opt(flux_dn), opt(flux_dir));
}

void Rte_sw_gpu::expand_and_transpose(const std::unique_ptr<Optical_props_arry_gpu>& ops, const Array_gpu<Float,2> arr_in, Array_gpu<Float,2>& arr_out)
{ expand(ops, arr_in, arr_out); }
