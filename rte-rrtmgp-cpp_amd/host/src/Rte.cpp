// Rte_lw_gpu / Rte_sw_gpu: /root/reference/src_cuda/Rte_lw.cu:60-159 and src_cuda/Rte_sw.cu:116-185.
// The public methods check and dispatch. What every entry of a family takes is gathered once per call (Lw_call, Sw_call); one function
// per C entry spells that entry's argument list, the argument runs that entries share are the three LW_*_ARGS.
#include "Rte_lw.h"
#include "Rte_sw.h"

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

    using Props = std::unique_ptr<Optical_props_arry_gpu>;

    void expand(const Props& ops, const Array_gpu<Float,2>& arr_in, Array_gpu<Float,2>& arr_out)
    {
        RRX_CALL(rrx_expand_and_transpose, arr_in.dim(2), ops->get_nband(), ops->get_band_lims_gpoint_gpu().ptr(), arr_in.ptr(), arr_out.ptr());
    }

    // optional arguments: an array of size 0 is a null pointer (an output that is not written, an input that is not there)
    template<int N> Float* opt(Array_gpu<Float,N>& a) { return a.size() == 0 ? nullptr : a.ptr(); }
    template<int N> const Float* opt(const Array_gpu<Float,N>& a) { return a.size() == 0 ? nullptr : a.ptr(); }
    Float* opt(Array_gpu<Float,3>* a) { return a == nullptr ? nullptr : a->ptr(); }

    // flux arrays with one slab per band (fewer bands than g-points) select the by-band form
    bool is_byband(const Props& ops, const Array_gpu<Float,3>& flux) { return flux.dim(3) == ops->get_nband() && ops->get_nband() < ops->get_ngpt(); }
    bool is_broadband(const Props& ops, const Array_gpu<Float,3>& flux) { return flux.dim(3) == 1 && ops->get_ngpt() != 1; }

    // ---- the checks that several methods make, under the name of the method that makes them
    void refuse(const char* method, const char* why) { throw std::runtime_error(std::string(method) + ": " + why); }

    void need_planck_lite(const char* method, const Source_func_lw_gpu& sources)
    { if (!sources.holds_fractions()) refuse(method, "needs the Planck-lite sources (enable_planck_lite)"); }

    void need_jacobian_like_fluxes(const char* method, const Array_gpu<Float,3>& jac, const Array_gpu<Float,3>& flux)
    { if (jac.get_dims() != flux.get_dims()) refuse(method, "flux_up_jac must be shaped like the flux arrays"); }

    void need_band_slabs(const char* method, const Props& ops, std::initializer_list<const Array_gpu<Float,3>*> fluxes)
    { for (const auto* f : fluxes) if (f->dim(3) != ops->get_nband()) refuse(method, "flux arrays need one slab per band"); }

    // what rte_lw_2stream and rte_lw_rescaled ask of their arguments: Planck-lite sources, broadband arrays, the cloud by band
    void check_cloudy_lw(const char* method, const Props& ops, const Source_func_lw_gpu& sources, const Optical_props_2str_gpu* cloud,
                         const Array_gpu<Float,3>& flux_up, const Array_gpu<Float,3>& flux_dn)
    {
        need_planck_lite(method, sources);
        if (flux_up.dim(3) != 1 || flux_dn.dim(3) != 1) refuse(method, "needs broadband flux arrays (third dimension 1)");
        if (cloud != nullptr && (cloud->get_ncol() != ops->get_ncol() || cloud->get_nlay() != ops->get_nlay() || cloud->get_tau().dim(3) != ops->get_nband()))
            refuse(method, "the cloud optical properties must be (ncol, nlay, nbnd)");
    }

    // ---- LW: what the entries of the family take, gathered once per call. The constructor expands sfc_emis (the call's first device work).
    struct Lw_call
    {
        const int ncol, nlay, ngpt, nbnd;
        const Bool top_at_1;
        const Float* tau;
        const int* gpoint_bands; const int* band_lims;
        const Source_func_lw_gpu& sources;                   // lay_source / lev_source: read where they are used, since reading materialises them
        const Float *pfrac, *blay, *blev;                    // the Planck-lite group (null arrays on sources that hold no fractions)
        const Float *sfc_source, *sfc_source_jac;
        Array_gpu<Float,2> sfc_emis_gpt;
        const Float* inc_flux;                               // or null
        const Float *cloud_tau, *cloud_ssa, *cloud_g;        // by band, or null

        Lw_call(const Props& ops, const Bool top_at_1, const Source_func_lw_gpu& sources, const Array_gpu<Float,2>& sfc_emis,
                const Array_gpu<Float,2>& inc_flux, const Optical_props_2str_gpu* cloud = nullptr) :
            ncol(ops->get_ncol()), nlay(ops->get_nlay()), ngpt(ops->get_ngpt()), nbnd(ops->get_nband()), top_at_1(top_at_1),
            tau(ops->get_tau().ptr()), gpoint_bands(ops->get_gpoint_bands_gpu().ptr()), band_lims(ops->get_band_lims_gpoint_gpu().ptr()),
            sources(sources), pfrac(sources.get_planck_frac().ptr()), blay(sources.get_planck_lay().ptr()), blev(sources.get_planck_lev().ptr()),
            sfc_source(sources.get_sfc_source().ptr()), sfc_source_jac(sources.get_sfc_source_jac().ptr()),
            sfc_emis_gpt({ncol, ngpt}), inc_flux(opt(inc_flux)),
            cloud_tau(cloud ? cloud->get_tau().ptr() : nullptr), cloud_ssa(cloud ? cloud->get_ssa().ptr() : nullptr),
            cloud_g(cloud ? cloud->get_g().ptr() : nullptr)
        {
            expand(ops, sfc_emis, sfc_emis_gpt);
        }
    };
    // the argument runs that the LW entries share
    #define LW_PLANCK_ARGS(c) c.tau, c.pfrac, c.blay, c.blev, c.gpoint_bands
    #define LW_SFC_ARGS(c)    c.sfc_emis_gpt.ptr(), c.sfc_source, c.inc_flux
    #define LW_CLOUD_ARGS(c)  c.cloud_tau, c.cloud_ssa, c.cloud_g

    // secants (ncol, ngpt, n) of the fixed Gauss rule with n angles, from the table on the device
    Array_gpu<Float,3> gauss_secants(const Lw_call& c, const int n, const Array_gpu<Float,2>& gauss_Ds)
    {
        Array_gpu<Float,3> secants({c.ncol, c.ngpt, n});
        RRX_CALL(rrx_lw_secants_array, c.ncol, c.ngpt, n, max_gauss_pts, gauss_Ds.ptr(), secants.ptr());
        return secants;
    }
    // secants (ncol, ngpt) of the optimal angle: from the optical depth of each column and g-point
    Array_gpu<Float,3> optimal_secants(const Lw_call& c, const Array_gpu<Float,2>& fit)
    {
        Array_gpu<Float,3> secants({c.ncol, c.ngpt, 1});
        RRX_CALL(rrx_lw_optimal_secants, c.ncol, c.nlay, c.ngpt, c.nbnd, c.gpoint_bands, fit.ptr(), c.tau, secants.ptr());
        return secants;
    }

    // One function per C entry. jac: null = no Jacobian, where the entry has it as an option.
    // Planck-lite sources and broadband arrays, one angle
    void lw_fractions(const Lw_call& c, const Float* secants, const Float* weights, Float* flux_up, Float* flux_dn)
    {
        RRX_CALL(rrx_lw_solver_noscat_fractions, c.ncol, c.nlay, c.ngpt, c.top_at_1, secants, weights, LW_PLANCK_ARGS(c), LW_SFC_ARGS(c),
                 flux_up, flux_dn);
    }
    void lw_fractions_jac(const Lw_call& c, const Float* secants, const Float* weights, Float* flux_up, Float* flux_dn, Float* jac)
    {
        RRX_CALL(rrx_lw_solver_noscat_fractions_jac, c.ncol, c.nlay, c.ngpt, c.top_at_1, secants, weights, LW_PLANCK_ARGS(c), LW_SFC_ARGS(c),
                 flux_up, flux_dn, c.sfc_source_jac, jac);
    }
    // several angles: one kernel reads each g-point once and solves it n times
    void lw_fractions_angles(const Lw_call& c, const int n, const Float* secants, const Float* weights, Float* flux_up, Float* flux_dn, Float* jac)
    {
        RRX_CALL(rrx_lw_solver_noscat_fractions_angles, c.ncol, c.nlay, c.ngpt, c.top_at_1, n, secants, weights, LW_PLANCK_ARGS(c), LW_SFC_ARGS(c),
                 flux_up, flux_dn, jac ? c.sfc_source_jac : nullptr, jac);
    }
    // the fused solver forms the optimal-angle secants from the g-point it holds: no secants array at all
    void lw_fractions_optimal(const Lw_call& c, const Float* weights, const Array_gpu<Float,2>& fit, Float* flux_up, Float* flux_dn, Float* jac)
    {
        RRX_CALL(rrx_lw_solver_noscat_fractions_optimal, c.ncol, c.nlay, c.ngpt, c.nbnd, c.top_at_1, weights, LW_PLANCK_ARGS(c), fit.ptr(),
                 LW_SFC_ARGS(c), flux_up, flux_dn, jac ? c.sfc_source_jac : nullptr, jac, nullptr);
    }
    void lw_fractions_byband(const Lw_call& c, const Float* secants, const Float* weights, Float* bnd_flux_up, Float* bnd_flux_dn,
                             Float* bnd_flux_net, Float* flux_up, Float* flux_dn)
    {
        RRX_CALL(rrx_lw_solver_noscat_fractions_byband, c.ncol, c.nlay, c.ngpt, c.nbnd, c.top_at_1, secants, weights, LW_PLANCK_ARGS(c),
                 c.band_lims, LW_SFC_ARGS(c), bnd_flux_up, bnd_flux_dn, bnd_flux_net, flux_up, flux_dn);
    }
    void lw_fractions_rescaled(const Lw_call& c, const Float* secants, const Float* weights, Float* flux_up, Float* flux_dn)
    {
        RRX_CALL(rrx_lw_solver_noscat_fractions_rescaled, c.ncol, c.nlay, c.ngpt, c.nbnd, c.top_at_1, secants, weights, LW_PLANCK_ARGS(c),
                 c.band_lims, LW_CLOUD_ARGS(c), LW_SFC_ARGS(c), flux_up, flux_dn);
    }
    // (two streams: no angles, and no Planck function of the layers)
    void lw_fractions_2stream(const Lw_call& c, Float* flux_up, Float* flux_dn)
    {
        RRX_CALL(rrx_lw_solver_2stream_fractions, c.ncol, c.nlay, c.ngpt, c.nbnd, c.top_at_1, c.tau, c.pfrac, c.blev, c.gpoint_bands,
                 c.band_lims, LW_CLOUD_ARGS(c), LW_SFC_ARGS(c), flux_up, flux_dn);
    }
    // the general solver, on lay_source / lev_source: per-g-point Jacobians. Broadband flux arrays: into an array of this call, then summed
    // over the g-points into jac.
    void lw_general(const Lw_call& c, const int n, const Float* secants, const Float* weights, Float* flux_up, Float* flux_dn,
                    const Bool do_broadband, Float* jac)
    {
        Array_gpu<Float,3> jac_bb;
        if (jac != nullptr && do_broadband) jac_bb.set_dims({c.ncol, c.nlay + 1, c.ngpt});
        Float* jac_gpt = jac_bb.size() != 0 ? jac_bb.ptr() : jac;
        RRX_CALL(rrx_lw_solver_noscat, c.ncol, c.nlay, c.ngpt, c.top_at_1, n, secants, weights,
                 c.tau, c.sources.get_lay_source().ptr(), c.sources.get_lev_source().ptr(), LW_SFC_ARGS(c),
                 flux_up, flux_dn, do_broadband, flux_up, flux_dn, Bool(jac != nullptr), jac ? c.sfc_source_jac : nullptr, jac_gpt);
        if (jac_bb.size() != 0) RRX_CALL(rrx_sum_broadband, c.ncol, c.nlay + 1, c.ngpt, jac_gpt, jac);
    }
}

// The table of the Gauss secants and the weights of the rule with n angles on the device, uploaded when n is not the rule of the last call
const Float* Rte_lw_gpu::gauss_weights(const int n)
{
    if (gauss_angles_cached != n)
    {
        gauss_Ds_gpu = Array_gpu<Float,2>(Array<Float,2>(gauss_Ds_v, {max_gauss_pts, max_gauss_pts}));
        const Array<Float,2> gauss_wts(gauss_wts_v, {max_gauss_pts, max_gauss_pts});
        gauss_wts_gpu = Array_gpu<Float,2>(gauss_wts.subset({{ {1, n}, {n, n} }}));
        gauss_angles_cached = n;
    }
    return gauss_wts_gpu.ptr();
}

void Rte_lw_gpu::rte_lw(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis, const Array_gpu<Float,2>& inc_flux, Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn,
        const int n_gauss_angles)
{
    solve(optical_props, top_at_1, sources, sfc_emis, inc_flux, gpt_flux_up, gpt_flux_dn, nullptr, n_gauss_angles);
}

void Rte_lw_gpu::rte_lw(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis, const Array_gpu<Float,2>& inc_flux, Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn,
        Array_gpu<Float,3>& flux_up_jac, const int n_gauss_angles)
{
    if (is_byband(optical_props, gpt_flux_up)) throw std::runtime_error("rte_lw: no Jacobian for by-band flux arrays");
    need_jacobian_like_fluxes("rte_lw", flux_up_jac, gpt_flux_up);
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
    if (own_secants && flux_up_jac != nullptr) need_jacobian_like_fluxes("rte_lw", *flux_up_jac, gpt_flux_up);
    if (is_byband(optical_props, gpt_flux_up))
    {
        if (n_gauss_angles != 1) throw std::runtime_error("rte_lw: by-band fluxes need one quadrature angle");
        Array_gpu<Float,3> no3; Array_gpu<Float,2> no_up, no_dn;
        rte_lw_byband(optical_props, top_at_1, sources, sfc_emis, inc_flux, gpt_flux_up, gpt_flux_dn, no3, no_up, no_dn);
        return;
    }
    const Lw_call c(optical_props, top_at_1, sources, sfc_emis, inc_flux);
    const int n = n_gauss_angles;
    const Float* weights = gauss_weights(n);
    Float* up = gpt_flux_up.ptr(); Float* dn = gpt_flux_dn.ptr(); Float* jac = opt(flux_up_jac);
    const Bool do_broadband = is_broadband(optical_props, gpt_flux_up);
    // Planck-lite state (set by Gas_optics_rrtmgp_gpu::gas_optics): the broadband solver forms the sources itself
    const bool fused = sources.holds_fractions() && do_broadband;

    if (fused && optimal_angle_fit != nullptr) return lw_fractions_optimal(c, weights, *optimal_angle_fit, up, dn, jac);

    // the secants of the solve: the caller's lw_Ds as they are, else an array of this call (optimal angles or the Gauss nodes)
    Array_gpu<Float,3> secants_own;
    if (optimal_angle_fit != nullptr) secants_own = optimal_secants(c, *optimal_angle_fit);
    else if (lw_Ds == nullptr)        secants_own = gauss_secants(c, n, gauss_Ds_gpu);
    const Float* secants = lw_Ds != nullptr ? lw_Ds->ptr() : secants_own.ptr();

    if (fused && n > 1)          return lw_fractions_angles(c, n, secants, weights, up, dn, jac);
    if (fused && jac != nullptr) return lw_fractions_jac(c, secants, weights, up, dn, jac);
    if (fused)                   return lw_fractions(c, secants, weights, up, dn);
    lw_general(c, n, secants, weights, up, dn, do_broadband, jac);
}

void Rte_lw_gpu::rte_lw_byband(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis, const Array_gpu<Float,2>& inc_flux, Array_gpu<Float,3>& bnd_flux_up, Array_gpu<Float,3>& bnd_flux_dn,
        Array_gpu<Float,3>& bnd_flux_net, Array_gpu<Float,2>& flux_up, Array_gpu<Float,2>& flux_dn)
{
    // (the by-band solver forms the sources from the Planck fractions: the reference-shaped lay_source / lev_source have no by-band form)
    need_planck_lite("rte_lw_byband", sources);
    need_band_slabs("rte_lw_byband", optical_props, {&bnd_flux_up, &bnd_flux_dn});
    const Lw_call c(optical_props, top_at_1, sources, sfc_emis, inc_flux);
    const Float* weights = gauss_weights(1);
    lw_fractions_byband(c, gauss_secants(c, 1, gauss_Ds_gpu).ptr(), weights, bnd_flux_up.ptr(), bnd_flux_dn.ptr(),
                        opt(bnd_flux_net), opt(flux_up), opt(flux_dn));
}

void Rte_lw_gpu::rte_lw_2stream(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis, const Array_gpu<Float,2>& inc_flux, const Optical_props_2str_gpu* cloud,
        Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn)
{
    check_cloudy_lw("rte_lw_2stream", optical_props, sources, cloud, gpt_flux_up, gpt_flux_dn);
    const Lw_call c(optical_props, top_at_1, sources, sfc_emis, inc_flux, cloud);
    lw_fractions_2stream(c, gpt_flux_up.ptr(), gpt_flux_dn.ptr());
}

void Rte_lw_gpu::rte_lw_rescaled(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Source_func_lw_gpu& sources,
        const Array_gpu<Float,2>& sfc_emis, const Array_gpu<Float,2>& inc_flux, const Optical_props_2str_gpu* cloud,
        Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn)
{
    check_cloudy_lw("rte_lw_rescaled", optical_props, sources, cloud, gpt_flux_up, gpt_flux_dn);
    const Lw_call c(optical_props, top_at_1, sources, sfc_emis, inc_flux, cloud);
    const Float* weights = gauss_weights(1);
    lw_fractions_rescaled(c, gauss_secants(c, 1, gauss_Ds_gpu).ptr(), weights, gpt_flux_up.ptr(), gpt_flux_dn.ptr());
}

void Rte_lw_gpu::expand_and_transpose(const std::unique_ptr<Optical_props_arry_gpu>& ops, const Array_gpu<Float,2> arr_in, Array_gpu<Float,2>& arr_out)
{ expand(ops, arr_in, arr_out); }

// ---- SW: the solve and the by-band solve, each once for both ranks of mu0: (ncol), or (ncol, nlay), a cosine of the solar zenith angle
// per layer. The rank picks the entry and the check of mu0, which the 1-D form never had.
namespace
{
    void check_mu0(const char*, const Props&, const Array_gpu<Float,1>&) {}
    void check_mu0(const char* method, const Props& ops, const Array_gpu<Float,2>& mu0)
    {
        if (mu0.dim(1) != ops->get_ncol() || mu0.dim(2) != ops->get_nlay()) refuse(method, "mu0 by layer must be (ncol, nlay)");
    }

    template<int N>
    void sw_solve_byband(
            const Props& ops, const Bool top_at_1, const Array_gpu<Float,N>& mu0, const Array_gpu<Float,2>& inc_flux_dir,
            const Array_gpu<Float,2>& sfc_alb_dir, const Array_gpu<Float,2>& sfc_alb_dif, const Array_gpu<Float,2>& inc_flux_dif,
            Array_gpu<Float,3>& bnd_flux_up, Array_gpu<Float,3>& bnd_flux_dn, Array_gpu<Float,3>& bnd_flux_dir, Array_gpu<Float,3>& bnd_flux_net,
            Array_gpu<Float,2>& flux_up, Array_gpu<Float,2>& flux_dn, Array_gpu<Float,2>& flux_dir)
    {
        check_mu0("rte_sw_byband", ops, mu0);
        need_band_slabs("rte_sw_byband", ops, {&bnd_flux_up, &bnd_flux_dn, &bnd_flux_dir});
        const int ncol = ops->get_ncol(), ngpt = ops->get_ngpt();
        Array_gpu<Float,2> alb_dir_gpt({ncol, ngpt}), alb_dif_gpt({ncol, ngpt});
        expand(ops, sfc_alb_dir, alb_dir_gpt);
        expand(ops, sfc_alb_dif, alb_dif_gpt);
        const Bool has_dif_bc = (inc_flux_dif.size() > 0);
        #define SW_BYBAND_ARGS \
            ncol, ops->get_nlay(), ngpt, ops->get_nband(), top_at_1, ops->get_tau().ptr(), ops->get_ssa().ptr(), ops->get_g_or_null(), mu0.ptr(), \
            alb_dir_gpt.ptr(), alb_dif_gpt.ptr(), inc_flux_dir.ptr(), has_dif_bc, opt(inc_flux_dif), ops->get_band_lims_gpoint_gpu().ptr(), \
            bnd_flux_up.ptr(), bnd_flux_dn.ptr(), bnd_flux_dir.ptr(), opt(bnd_flux_net), opt(flux_up), opt(flux_dn), opt(flux_dir)
        if constexpr (N == 1) RRX_CALL(rrx_sw_solver_2stream_byband, SW_BYBAND_ARGS);
        else                  RRX_CALL(rrx_sw_solver_2stream_byband_mu0lay, SW_BYBAND_ARGS);
        #undef SW_BYBAND_ARGS
    }

    template<int N>
    void sw_solve(
            const Props& ops, const Bool top_at_1, const Array_gpu<Float,N>& mu0, const Array_gpu<Float,2>& inc_flux_dir,
            const Array_gpu<Float,2>& sfc_alb_dir, const Array_gpu<Float,2>& sfc_alb_dif, const Array_gpu<Float,2>& inc_flux_dif,
            Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn, Array_gpu<Float,3>& gpt_flux_dir)
    {
        if (is_byband(ops, gpt_flux_up))
        {
            Array_gpu<Float,3> no3; Array_gpu<Float,2> no_up, no_dn, no_dir;
            return sw_solve_byband(ops, top_at_1, mu0, inc_flux_dir, sfc_alb_dir, sfc_alb_dif, inc_flux_dif, gpt_flux_up, gpt_flux_dn,
                                   gpt_flux_dir, no3, no_up, no_dn, no_dir);
        }
        check_mu0("rte_sw", ops, mu0);
        const int ncol = ops->get_ncol(), ngpt = ops->get_ngpt();
        Array_gpu<Float,2> alb_dir_gpt({ncol, ngpt}), alb_dif_gpt({ncol, ngpt});
        expand(ops, sfc_alb_dir, alb_dir_gpt);
        expand(ops, sfc_alb_dif, alb_dif_gpt);
        const Bool has_dif_bc = (inc_flux_dif.size() > 0);
        const Bool do_broadband = is_broadband(ops, gpt_flux_up);
        // "no g" is native to the fused broadband solver; the per-g-point forms read an array (zeros materialised here)
        const Float* g = do_broadband ? ops->get_g_or_null() : static_cast<const Float*>(ops->get_g().ptr());
        #define SW_ARGS \
            ncol, ops->get_nlay(), ngpt, top_at_1, ops->get_tau().ptr(), ops->get_ssa().ptr(), g, mu0.ptr(), \
            alb_dir_gpt.ptr(), alb_dif_gpt.ptr(), inc_flux_dir.ptr(), gpt_flux_up.ptr(), gpt_flux_dn.ptr(), gpt_flux_dir.ptr(), \
            has_dif_bc, opt(inc_flux_dif), do_broadband, gpt_flux_up.ptr(), gpt_flux_dn.ptr(), gpt_flux_dir.ptr()
        if constexpr (N == 1) RRX_CALL(rrx_sw_solver_2stream, SW_ARGS);
        else                  RRX_CALL(rrx_sw_solver_2stream_mu0lay, SW_ARGS);
        #undef SW_ARGS
    }
}

void Rte_sw_gpu::rte_sw(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Array_gpu<Float,1>& mu0,
        const Array_gpu<Float,2>& inc_flux_dir, const Array_gpu<Float,2>& sfc_alb_dir, const Array_gpu<Float,2>& sfc_alb_dif,
        const Array_gpu<Float,2>& inc_flux_dif, Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn, Array_gpu<Float,3>& gpt_flux_dir)
{
    sw_solve(optical_props, top_at_1, mu0, inc_flux_dir, sfc_alb_dir, sfc_alb_dif, inc_flux_dif, gpt_flux_up, gpt_flux_dn, gpt_flux_dir);
}

void Rte_sw_gpu::rte_sw(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Array_gpu<Float,2>& mu0,
        const Array_gpu<Float,2>& inc_flux_dir, const Array_gpu<Float,2>& sfc_alb_dir, const Array_gpu<Float,2>& sfc_alb_dif,
        const Array_gpu<Float,2>& inc_flux_dif, Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn, Array_gpu<Float,3>& gpt_flux_dir)
{
    sw_solve(optical_props, top_at_1, mu0, inc_flux_dir, sfc_alb_dir, sfc_alb_dif, inc_flux_dif, gpt_flux_up, gpt_flux_dn, gpt_flux_dir);
}

void Rte_sw_gpu::rte_sw_byband(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Array_gpu<Float,1>& mu0,
        const Array_gpu<Float,2>& inc_flux_dir, const Array_gpu<Float,2>& sfc_alb_dir, const Array_gpu<Float,2>& sfc_alb_dif,
        const Array_gpu<Float,2>& inc_flux_dif, Array_gpu<Float,3>& bnd_flux_up, Array_gpu<Float,3>& bnd_flux_dn, Array_gpu<Float,3>& bnd_flux_dir,
        Array_gpu<Float,3>& bnd_flux_net, Array_gpu<Float,2>& flux_up, Array_gpu<Float,2>& flux_dn, Array_gpu<Float,2>& flux_dir)
{
    sw_solve_byband(optical_props, top_at_1, mu0, inc_flux_dir, sfc_alb_dir, sfc_alb_dif, inc_flux_dif, bnd_flux_up, bnd_flux_dn, bnd_flux_dir,
                    bnd_flux_net, flux_up, flux_dn, flux_dir);
}

void Rte_sw_gpu::rte_sw_byband(
        const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Array_gpu<Float,2>& mu0,
        const Array_gpu<Float,2>& inc_flux_dir, const Array_gpu<Float,2>& sfc_alb_dir, const Array_gpu<Float,2>& sfc_alb_dif,
        const Array_gpu<Float,2>& inc_flux_dif, Array_gpu<Float,3>& bnd_flux_up, Array_gpu<Float,3>& bnd_flux_dn, Array_gpu<Float,3>& bnd_flux_dir,
        Array_gpu<Float,3>& bnd_flux_net, Array_gpu<Float,2>& flux_up, Array_gpu<Float,2>& flux_dn, Array_gpu<Float,2>& flux_dir)
{
    sw_solve_byband(optical_props, top_at_1, mu0, inc_flux_dir, sfc_alb_dir, sfc_alb_dif, inc_flux_dif, bnd_flux_up, bnd_flux_dn, bnd_flux_dir,
                    bnd_flux_net, flux_up, flux_dn, flux_dir);
}

void Rte_sw_gpu::expand_and_transpose(const std::unique_ptr<Optical_props_arry_gpu>& ops, const Array_gpu<Float,2> arr_in, Array_gpu<Float,2>& arr_out)
{ expand(ops, arr_in, arr_out); }
