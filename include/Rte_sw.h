/* Rte_sw_gpu -- interface of /root/reference/include/Rte_sw.h:62-81 (broadband mode and a diffuse boundary condition work).
 * By-band mode: flux arrays with third dimension nband < ngpt receive the band sums of the g-point fluxes (the fused solver,
 * rrx_sw_solver_2stream_byband); rte_sw_byband also gives the band net flux and the broadband fluxes from the same solve. */
#ifndef RTE_SW_H
#define RTE_SW_H
#include <memory>
#include "Array.h"
#include "Optical_props.h"

class Rte_sw_gpu
{
    public:
        void rte_sw(
                const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
                const Bool top_at_1,
                const Array_gpu<Float,1>& mu0,
                const Array_gpu<Float,2>& inc_flux_dir,
                const Array_gpu<Float,2>& sfc_alb_dir,
                const Array_gpu<Float,2>& sfc_alb_dif,
                const Array_gpu<Float,2>& inc_flux_dif,
                Array_gpu<Float,3>& gpt_flux_up,
                Array_gpu<Float,3>& gpt_flux_dn,
                Array_gpu<Float,3>& gpt_flux_dir);
        // mu0 (ncol, nlay): a cosine of the solar zenith angle per layer (rrx_sw_solver_2stream_mu0lay)
        void rte_sw(
                const std::unique_ptr<Optical_props_arry_gpu>& optical_props,
                const Bool top_at_1,
                const Array_gpu<Float,2>& mu0,
                const Array_gpu<Float,2>& inc_flux_dir,
                const Array_gpu<Float,2>& sfc_alb_dir,
                const Array_gpu<Float,2>& sfc_alb_dif,
                const Array_gpu<Float,2>& inc_flux_dif,
                Array_gpu<Float,3>& gpt_flux_up,
                Array_gpu<Float,3>& gpt_flux_dn,
                Array_gpu<Float,3>& gpt_flux_dir);
        // by-band fluxes (ncol, nlev, nband); bnd_flux_net (dn - up per band) and the broadband flux_up/dn/dir (the band sums
        // added in band order) are written when their size is not 0
        void rte_sw_byband(
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
                Array_gpu<Float,2>& flux_dir);
        void rte_sw_byband(
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
                Array_gpu<Float,2>& flux_dir);
        void expand_and_transpose(
                const std::unique_ptr<Optical_props_arry_gpu>& ops,
                const Array_gpu<Float,2> arr_in,
                Array_gpu<Float,2>& arr_out);
};
#endif
