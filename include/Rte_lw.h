/* Rte_lw_gpu -- interface of /root/reference/include/Rte_lw.h:62-80. Unlike the reference GPU class, broadband mode
 * (gpt_flux arrays with third dimension 1, as the CPU path uses: src/Rte_lw.cpp:176) and n_gauss_angles 1..4 work.
 * By-band mode: flux arrays with third dimension nband < ngpt receive the band sums of the g-point fluxes (the fused solver,
 * rrx_lw_solver_noscat_fractions_byband; Planck-lite sources and one quadrature angle). rte_lw_byband also gives the band net
 * flux and the broadband fluxes from the same solve. */
#ifndef RTE_LW_H
#define RTE_LW_H
#include <memory>
#include "Array.h"
#include "Optical_props.h"
#include "Source_functions.h"

class Rte_lw_gpu
{
    public:
        void rte_lw(
                const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
                const Bool top_at_1,
                const Source_func_lw_gpu& sources,
                const Array_gpu<Float,2>& sfc_emis,
                const Array_gpu<Float,2>& inc_flux,
                Array_gpu<Float,3>& gpt_flux_up,
                Array_gpu<Float,3>& gpt_flux_dn,
                const int n_gauss_angles);
        // the same plus flux_up_jac, the surface-temperature Jacobian of the upward flux [W m-2 K-1], shaped like the flux arrays:
        // third dimension 1 = broadband (with Planck-lite sources and one angle the fused solver, rrx_lw_solver_noscat_fractions_jac),
        // ngpt = per g-point (the general solver with do_jacobians). By-band flux arrays have no Jacobian form.
        void rte_lw(
                const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
                const Bool top_at_1,
                const Source_func_lw_gpu& sources,
                const Array_gpu<Float,2>& sfc_emis,
                const Array_gpu<Float,2>& inc_flux,
                Array_gpu<Float,3>& gpt_flux_up,
                Array_gpu<Float,3>& gpt_flux_dn,
                Array_gpu<Float,3>& flux_up_jac,
                const int n_gauss_angles);
        // Optimal-angle secants (upstream's compute_optimal_angles / lw_Ds; one angle: more throws, as do by-band flux arrays). These
        // two are named on their own, not overloads of rte_lw. flux_up_jac: null = no Jacobian.
        // rte_lw_optimal: optimal_angle_fit (2, nbnd) of the k-distribution (Gas_optics_rrtmgp_gpu::get_optimal_angle_fit_gpu). With
        // Planck-lite sources and broadband arrays the fused solver forms the secants itself (rrx_lw_solver_noscat_fractions_optimal);
        // otherwise they are computed (rrx_lw_optimal_secants) and the solve runs as rte_lw_Ds.
        void rte_lw_optimal(
                const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
                const Bool top_at_1,
                const Source_func_lw_gpu& sources,
                const Array_gpu<Float,2>& sfc_emis,
                const Array_gpu<Float,2>& inc_flux,
                const Array_gpu<Float,2>& optimal_angle_fit,
                Array_gpu<Float,3>& gpt_flux_up,
                Array_gpu<Float,3>& gpt_flux_dn,
                Array_gpu<Float,3>* flux_up_jac,
                const int n_gauss_angles);
        // rte_lw_Ds: lw_Ds (ncol, ngpt), the secant per column and g-point; any route of rte_lw runs with it
        void rte_lw_Ds(
                const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
                const Bool top_at_1,
                const Source_func_lw_gpu& sources,
                const Array_gpu<Float,2>& sfc_emis,
                const Array_gpu<Float,2>& inc_flux,
                const Array_gpu<Float,2>& lw_Ds,
                Array_gpu<Float,3>& gpt_flux_up,
                Array_gpu<Float,3>& gpt_flux_dn,
                Array_gpu<Float,3>* flux_up_jac,
                const int n_gauss_angles);
        // by-band fluxes (ncol, nlev, nband); bnd_flux_net (dn - up per band) and the broadband flux_up/dn (the band sums added in
        // band order) are written when their size is not 0
        void rte_lw_byband(
                const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
                const Bool top_at_1,
                const Source_func_lw_gpu& sources,
                const Array_gpu<Float,2>& sfc_emis,
                const Array_gpu<Float,2>& inc_flux,
                Array_gpu<Float,3>& bnd_flux_up,
                Array_gpu<Float,3>& bnd_flux_dn,
                Array_gpu<Float,3>& bnd_flux_net,
                Array_gpu<Float,2>& flux_up,
                Array_gpu<Float,2>& flux_dn);
        // LW two-stream solve WITH scattering (rrx_lw_solver_2stream_fractions; a name of its own, not an overload of rte_lw): the clear
        // gas optical depth of optical_props, Planck-lite sources (throws otherwise) and broadband flux arrays (third dimension 1;
        // throws otherwise). cloud: LW cloud tau / ssa / g by band, (ncol, nlay, nbnd), combined with the gas inside the kernel; null =
        // no clouds (ssa = 0). No quadrature angles, no Jacobian, no by-band form.
        void rte_lw_2stream(
                const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
                const Bool top_at_1,
                const Source_func_lw_gpu& sources,
                const Array_gpu<Float,2>& sfc_emis,
                const Array_gpu<Float,2>& inc_flux,
                const Optical_props_2str_gpu* cloud,
                Array_gpu<Float,3>& gpt_flux_up,
                Array_gpu<Float,3>& gpt_flux_dn);
        // LW no-scattering solve on rescaled optical depths with one correction sweep (rrx_lw_solver_noscat_fractions_rescaled; one
        // fixed Gauss angle): arguments and requirements as rte_lw_2stream.
        void rte_lw_rescaled(
                const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
                const Bool top_at_1,
                const Source_func_lw_gpu& sources,
                const Array_gpu<Float,2>& sfc_emis,
                const Array_gpu<Float,2>& inc_flux,
                const Optical_props_2str_gpu* cloud,
                Array_gpu<Float,3>& gpt_flux_up,
                Array_gpu<Float,3>& gpt_flux_dn);
        void expand_and_transpose(
                const std::unique_ptr<Optical_props_arry_gpu>& ops,
                const Array_gpu<Float,2> arr_in,
                Array_gpu<Float,2>& arr_out);
    private:
        void solve(
                const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1, const Source_func_lw_gpu& sources,
                const Array_gpu<Float,2>& sfc_emis, const Array_gpu<Float,2>& inc_flux,
                Array_gpu<Float,3>& gpt_flux_up, Array_gpu<Float,3>& gpt_flux_dn, Array_gpu<Float,3>* flux_up_jac, const int n_gauss_angles,
                const Array_gpu<Float,2>* optimal_angle_fit = nullptr, const Array_gpu<Float,2>* lw_Ds = nullptr);
        // Gauss-Jacobi secants (the whole table, in gauss_Ds_gpu) and the weights of the rule with n angles on the device, uploaded once
        // per object and angle count (an upload per call is a host copy the stream is synchronised for: the solver launch then waits
        // for the gas optics to finish before it is even enqueued). gauss_weights(n) does that and returns the weights; gauss_Ds_gpu is
        // good to read after it.
        const Float* gauss_weights(const int n);
        Array_gpu<Float,2> gauss_Ds_gpu, gauss_wts_gpu;
        int gauss_angles_cached = 0;
};
#endif
