/*
 * Radiation_solver_longwave / Radiation_solver_shortwave -- GPU solve path with the constructor and solve_gpu
 * argument lists of /root/reference/include_test/Radiation_solver.h:33-235, so that test_rte_rrtmgp-style drivers and a
 * host model (MicroHH) call it unchanged. Implementation: rte-rrtmgp-cpp_amd/host/src_test/Radiation_solver.cpp.
 *
 * Differences from the reference, all on the performance side:
 *   - the column block is a run-time setting (set_column_block; default 16384 instead of a fixed 1024): MI355X has
 *     288 GB of HBM, and bigger blocks mean fewer, larger launches;
 *   - block-sized workspaces (optical props, sources, g-point fluxes) are cached across calls;
 *   - without --output-bnd-fluxes the solvers can run in broadband mode (set_broadband_solvers(true)), the CPU path's
 *     convention (src_test/Radiation_solver.cpp:518-527), which never materialises per-g-point fluxes;
 *   - with --output-bnd-fluxes the fused solvers can write the band sums themselves (set_byband_solvers(true), default off).
 */
#ifndef RADIATION_SOLVER_H
#define RADIATION_SOLVER_H
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include "Array.h"
#include "Gas_concs.h"
#include "Gas_optics_rrtmgp.h"
#include "Cloud_optics.h"
#include "Aerosol_optics.h"
#include "Optical_props.h"
#include "Source_functions.h"
#include "Fluxes.h"
#include "Rte_lw.h"
#include "Rte_sw.h"

// Layer heating rates [K/s] from net (down - up) broadband fluxes and level pressures, on the device:
// -(g/cp) dF_net/dp with g = 9.80665 m s-2, cp = 1004.64 J kg-1 K-1 (dry air). flux_net, p_lev: (ncol, nlay+1); out: (ncol, nlay).
void compute_heating_rate(const Array_gpu<Float,2>& flux_net, const Array_gpu<Float,2>& p_lev, Array_gpu<Float,2>& heating_rate);

// ---- behind the two classes (Radiation_solver.cpp); not part of the argument lists a host model calls ----
// The LW options of a solve_gpu call -- the solver's settings, the call's switches, n_bnd < n_gpt -- and what lw_solve_plan() makes of
// them: it throws the refusal of a pair that is not available (the one table lw_refusals) or returns what the solve does. A pure host
// function: solve_gpu reads the plan from there on, and rrx_host_selftest_lw_plan serves it to tests/test_host_lw_options.py.
struct Lw_solve_options
{
    bool broadband_solvers, byband_solvers, jacobian; int n_gauss_angles; bool optimal_angles, lw_scattering, lw_rescaling, cloud_sampling;
    bool switch_fluxes, switch_output_bnd_fluxes, switch_cloud_optics, fewer_bands_than_gpoints;
};
enum class Lw_form { per_gpoint, fractions, angles, optimal, byband, two_stream, rescaled };   // per_gpoint: the general kernel; else a fused form
struct Lw_solve_plan
{
    Lw_form form;
    bool broadband, byband, jac;    // in effect: the solvers sum the g-points; the by-band solver is in use; the Jacobian is formed
    bool cloud_to_solver;           // the cloud goes to the solver as tau / ssa / g by band, the gas optics stay clear
};
Lw_solve_plan lw_solve_plan(const Lw_solve_options& o);

// McICA cloud sampling of either solver (set_cloud_sampling): the borrowed fields, the seed and the columns' identities.
struct Cloud_sampling
{
    const Array_gpu<Float,2>* frac = nullptr; const Array_gpu<Float,2>* alpha = nullptr;
    uint64_t seed = 0; int col_offset = 0;
    const int* col_id = nullptr;       // (a reordered solve: the identities of its columns, on the device)
    bool on() const { return frac != nullptr; }
    void set(const char* who, const Array_gpu<Float,2>* cloud_frac, const int overlap, const Array_gpu<Float,2>* overlap_param,
             const uint64_t seed_in, const int col_offset_in);
    void check(const char* who, const int n_col, const int n_lay, const bool cloud_optics) const;
};

class Radiation_solver_longwave
{
    public:
        Radiation_solver_longwave(
                const Gas_concs_gpu& gas_concs,
                const std::string& file_name_gas,
                const std::string& file_name_cloud);

        void solve_gpu(
                const bool switch_fluxes,
                const bool switch_cloud_optics,
                const bool switch_output_optical,
                const bool switch_output_bnd_fluxes,
                const Gas_concs_gpu& gas_concs,
                const Array_gpu<Float,2>& p_lay, const Array_gpu<Float,2>& p_lev,
                const Array_gpu<Float,2>& t_lay, const Array_gpu<Float,2>& t_lev,
                const Array_gpu<Float,2>& col_dry,
                const Array_gpu<Float,1>& t_sfc, const Array_gpu<Float,2>& emis_sfc,
                const Array_gpu<Float,2>& lwp, const Array_gpu<Float,2>& iwp,
                const Array_gpu<Float,2>& rel, const Array_gpu<Float,2>& dei,
                Array_gpu<Float,3>& tau, Array_gpu<Float,3>& lay_source,
                Array_gpu<Float,3>& lev_source, Array_gpu<Float,2>& sfc_source,
                Array_gpu<Float,2>& lw_flux_up, Array_gpu<Float,2>& lw_flux_dn, Array_gpu<Float,2>& lw_flux_net,
                Array_gpu<Float,3>& lw_bnd_flux_up, Array_gpu<Float,3>& lw_bnd_flux_dn, Array_gpu<Float,3>& lw_bnd_flux_net);

        int get_n_gpt_gpu() const { return this->kdist_gpu->get_ngpt(); }
        int get_n_bnd_gpu() const { return this->kdist_gpu->get_nband(); }
        Array<int,2> get_band_lims_gpoint_gpu() const { return this->kdist_gpu->get_band_lims_gpoint(); }
        Array<Float,2> get_band_lims_wavenumber_gpu() const { return this->kdist_gpu->get_band_lims_wavenumber(); }

        void set_column_block(const int n) { n_col_block = n; }
        void set_broadband_solvers(const bool b) { broadband_solvers = b; }
        // With switch_output_bnd_fluxes: band fluxes from the fused solvers (one slab per band in the block workspace, Planck-lite
        // LW chain) instead of per-g-point fluxes reduced by Fluxes_byband_gpu. Default off.
        void set_byband_solvers(const bool b) { byband_solvers = b; }
        // Host-model coupling: the solver object is persistent -- k-distribution and LUTs stay on the device, block
        // workspaces are cached across calls -- and with the vertical ordering stated (0 = surface first, 1 = top first; -1 =
        // detect with the reference's synchronous read-backs) solve_gpu() enqueues everything on the calling thread's stream
        // (rrx_host::set_stream) without synchronising, so a host model can overlap it with its own work.
        void set_vertical_ordering(const int top_at_1) { vertical_ordering = top_at_1; kdist_gpu->set_vertical_ordering(top_at_1); }
        // Column order of a solve (round 4; DESIGN "columns that differ"). Columns are independent, so solve_gpu may process them in
        // another order and on a padded count: sorted by surface pressure (neighbouring columns then share LUT boxes in the windowed
        // gas optics: 21 -> 13.5 ms per LW+SW solve at +-35 % pressure spread) and padded to a multiple of 16 columns (rows of the cell
        // arrays on 128-B lines: 16 385 columns cost 20 % more than 16 384 otherwise). Inputs are gathered on the device at the top
        // of the solve, outputs scattered back: the caller sees its own order. mode: 1 = always sort, 0 = never, -1 (default) = sort
        // when the surface pressure varies by more than 20 % inside some run of 256 columns -- decided ONCE per solver object, at its
        // first solve, with one synchronous read-back of a flag (a host model that must never synchronise states 0 or 1).
        // Not applied when optical properties are output (switch_output_optical).
        void set_column_sorting(const int mode) { column_sorting = mode; sort_decided = -1; }
        void set_column_padding(const bool b) { column_padding = b; }
        // The options below do not all combine: solve_gpu throws for the pairs of the table lw_refusals in Radiation_solver.cpp
        // (lw_solve_plan above), each with its reason.
        // Surface-temperature Jacobian of the upward flux (default off): with fluxes requested, solve_gpu also forms d flux_up /
        // d T_sfc [W m-2 K-1] per level from the same solve (the fused broadband solver's Jacobian form, or the general solver's
        // per-g-point Jacobians summed over the g-points); get_lw_flux_up_jac() returns the (ncol, nlev) result of the last solve in
        // the caller's column order. A host model updates flux_up (and flux_net) with it between radiation calls
        // (rrx_lw_flux_up_adjust).
        void set_jacobian(const bool b) { jacobian = b; }
        const Array_gpu<Float,2>& get_lw_flux_up_jac() const { return lw_flux_up_jac; }
        // Quadrature angles of the LW solver (1..4 Gauss-Jacobi-5 nodes, default 1; throws otherwise). With the broadband solvers more
        // than one takes the several-angle form of the fused solver (rrx_lw_solver_noscat_fractions_angles, Jacobian included), the
        // per-g-point solvers take the general kernel once per angle.
        void set_gauss_angles(const int n)
        {
            if (n < 1 || n > 4) throw std::runtime_error("Radiation_solver_longwave::set_gauss_angles: " + std::to_string(n) + " is outside 1..4");
            n_gauss_angles = n;
        }
        int get_gauss_angles() const { return n_gauss_angles; }
        // Optimal angles (default off): the secant of the one LW angle is the coefficient file's optimal_angle_fit of the column's
        // total optical depth per g-point (compute_optimal_angles / lw_Ds of current RTE+RRTMGP); with the broadband solvers the fused
        // solver forms it itself (rrx_lw_solver_noscat_fractions_optimal). Throws for a file without the fit.
        void set_optimal_angles(const bool b);
        bool get_optimal_angles() const { return optimal_angles; }
        // LW cloud scattering (default off): solve_gpu takes the clear gas optics, the LW cloud tau / ssa / g by band from
        // Cloud_optics_gpu (with cloud optics in use; else ssa = 0) and the two-stream solver with scattering
        // (Rte_lw_gpu::rte_lw_2stream, rrx_lw_solver_2stream_fractions). Broadband solvers only.
        void set_lw_scattering(const bool b) { lw_scattering = b; }
        bool get_lw_scattering() const { return lw_scattering; }
        // LW rescaled scattering (default off): solve_gpu takes the clear gas optics, the LW cloud tau / ssa / g by band from
        // Cloud_optics_gpu (with cloud optics in use; else ssa = 0) and the no-scattering solver on rescaled optical depths with one
        // correction sweep (Rte_lw_gpu::rte_lw_rescaled, rrx_lw_solver_noscat_fractions_rescaled). Broadband solvers only.
        void set_lw_rescaling(const bool b) { lw_rescaling = b; }
        bool get_lw_rescaling() const { return lw_rescaling; }
        // McICA cloud sampling (default off): with cloud optics in use, solve_gpu runs the CLEAR gas optics and then
        // rrx_mcica_increment_1scalar, which gives every g-point its own sub-column drawn from cloud_frac (ncol, nlay) and adds the band
        // cloud optical depth in the cloudy cells only. overlap: 0 = maximum-random (overlap_param unused, may be nullptr), 1 =
        // exponential-random with overlap_param (ncol, nlay-1), the overlap parameter between array layers l and l+1. The arrays are
        // BORROWED: they stay the caller's, are read at every solve (update them in place) and must outlive the solves; nullptr as
        // cloud_frac turns the sampling off. The mask is redrawn at every solve from `seed` (call again to advance it; domain 0). A
        // column's draws are keyed by col_offset + its index in the caller's arrays and follow it through the column blocks, the
        // device sort and the padding. solve_gpu throws without cloud optics.
        void set_cloud_sampling(const Array_gpu<Float,2>* cloud_frac, const int overlap, const Array_gpu<Float,2>* overlap_param,
                                const uint64_t seed, const int col_offset = 0);

    private:
        Cloud_sampling mcica;
        int column_sorting = -1, sort_decided = -1;
        bool column_padding = true, reordered_call = false, jacobian = false, optimal_angles = false, lw_scattering = false, lw_rescaling = false;
        int n_gauss_angles = 1;
        Array_gpu<Float,2> lw_flux_up_jac;
        std::unique_ptr<Gas_optics_rrtmgp_gpu> kdist_gpu;
        std::unique_ptr<Cloud_optics_gpu> cloud_optics_gpu;
        Rte_lw_gpu rte_lw;
        int vertical_ordering = -1;
        int n_col_block = 16384;
        bool broadband_solvers = true;
        bool byband_solvers = false;

        struct Workspace;
        std::shared_ptr<Workspace> ws_block, ws_residual;
};

class Radiation_solver_shortwave
{
    public:
        Radiation_solver_shortwave(
                const Gas_concs_gpu& gas_concs,
                const bool switch_cloud_optics,
                const bool switch_aerosol_optics,
                const std::string& file_name_gas,
                const std::string& file_name_cloud,
                const std::string& file_name_aerosol);

        void solve_gpu(
                const bool switch_fluxes,
                const bool switch_cloud_optics,
                const bool switch_aerosol_optics,
                const bool switch_output_optical,
                const bool switch_output_bnd_fluxes,
                const bool switch_delta_cloud,
                const bool switch_delta_aerosol,
                const Gas_concs_gpu& gas_concs,
                const Array_gpu<Float,2>& p_lay, const Array_gpu<Float,2>& p_lev,
                const Array_gpu<Float,2>& t_lay, const Array_gpu<Float,2>& t_lev,
                const Array_gpu<Float,2>& col_dry,
                const Array_gpu<Float,2>& sfc_alb_dir, const Array_gpu<Float,2>& sfc_alb_dif,
                const Array_gpu<Float,1>& tsi_scaling, const Array_gpu<Float,1>& mu0,
                const Array_gpu<Float,2>& lwp, const Array_gpu<Float,2>& iwp,
                const Array_gpu<Float,2>& rel, const Array_gpu<Float,2>& dei,
                const Array_gpu<Float,2>& rh,
                const Aerosol_concs_gpu& aerosol_concs,
                Array_gpu<Float,3>& tau, Array_gpu<Float,3>& ssa, Array_gpu<Float,3>& g,
                Array_gpu<Float,2>& toa_src,
                Array_gpu<Float,2>& sw_flux_up, Array_gpu<Float,2>& sw_flux_dn,
                Array_gpu<Float,2>& sw_flux_dn_dir, Array_gpu<Float,2>& sw_flux_net,
                Array_gpu<Float,3>& sw_bnd_flux_up, Array_gpu<Float,3>& sw_bnd_flux_dn,
                Array_gpu<Float,3>& sw_bnd_flux_dn_dir, Array_gpu<Float,3>& sw_bnd_flux_net);

        int get_n_gpt_gpu() const { return this->kdist_gpu->get_ngpt(); }
        int get_n_bnd_gpu() const { return this->kdist_gpu->get_nband(); }
        Float get_tsi_gpu() const { return this->kdist_gpu->get_tsi(); }
        Array<int,2> get_band_lims_gpoint_gpu() const { return this->kdist_gpu->get_band_lims_gpoint(); }
        Array<Float,2> get_band_lims_wavenumber_gpu() const { return this->kdist_gpu->get_band_lims_wavenumber(); }

        void set_column_block(const int n) { n_col_block = n; }
        void set_broadband_solvers(const bool b) { broadband_solvers = b; }
        // With switch_output_bnd_fluxes: band fluxes from the fused solvers (one slab per band in the block workspace, Planck-lite
        // LW chain) instead of per-g-point fluxes reduced by Fluxes_byband_gpu. Default off.
        void set_byband_solvers(const bool b) { byband_solvers = b; }
        void set_vertical_ordering(const int top_at_1) { vertical_ordering = top_at_1; kdist_gpu->set_vertical_ordering(top_at_1); }
        // column order of a solve: see Radiation_solver_longwave
        void set_column_sorting(const int mode) { column_sorting = mode; sort_decided = -1; }
        void set_column_padding(const bool b) { column_padding = b; }
        // Sunlit-only solve (default off): with fluxes requested and no optical output, solve_gpu lists the columns with mu0 > 0 on
        // the device (in the sorted order when sorting is on, padded when padding is on), solves only those and writes exact zeros
        // to every SW flux (broadband and band) of the other columns. mu0 <= 0 and NaN count as night. Reading the count back
        // synchronises the stream once per solve in this mode. Off, the solve still requires mu0 > 0 in every column.
        void set_sunlit_columns(const bool b);
        // McICA cloud sampling (default off): with cloud optics in use, solve_gpu runs the CLEAR gas optics and then
        // rrx_mcica_increment_2stream, which gives every g-point its own sub-column drawn from cloud_frac (ncol, nlay) and combines the band
        // cloud tau / ssa / g into the cloudy cells only. overlap: 0 = maximum-random (overlap_param unused, may be nullptr), 1 =
        // exponential-random with overlap_param (ncol, nlay-1), the overlap parameter between array layers l and l+1. The arrays are
        // BORROWED: they stay the caller's, are read at every solve (update them in place) and must outlive the solves; nullptr as
        // cloud_frac turns the sampling off. The mask is redrawn at every solve from `seed` (call again to advance it; domain 1). A
        // column's draws are keyed by col_offset + its index in the caller's arrays and follow it through the column blocks, the
        // device sort and the padding. solve_gpu throws without cloud optics, or with set_sunlit_columns (the sunlit-only solve
        // does not carry the column identities).
        void set_cloud_sampling(const Array_gpu<Float,2>* cloud_frac, const int overlap, const Array_gpu<Float,2>* overlap_param,
                                const uint64_t seed, const int col_offset = 0);
        // Spherical-geometry correction of the solar zenith angle (default off): solve_gpu forms a cosine per layer from
        // its mu0 (ncol), which holds at ref_alt (ncol; nullptr = altitude 0), and the layer altitudes alt_lay (ncol, nlay), metres, with
        // rrx_zenith_angle_spherical_correction, and the solvers take that cosine layer by layer (Rte_sw_gpu's mu0 (ncol, nlay) overloads).
        // The arrays are BORROWED like set_cloud_sampling's: read at every solve, sorted, padded, gathered to the sunlit columns (whose
        // list is still made from mu0) and cut into column blocks with the other inputs; nullptr as alt_lay turns it off. Altitudes
        // below a column's reference altitude are not looked for: the kernel clamps the radicand at 0.
        void set_spherical_mu0(const Array_gpu<Float,2>* alt_lay, const Array_gpu<Float,1>* ref_alt = nullptr, const Float planet_radius = Float(6.37123e6));

    private:
        Cloud_sampling mcica;
        const Array_gpu<Float,2>* sph_alt = nullptr;
        const Array_gpu<Float,1>* sph_ref_alt = nullptr;
        Float sph_radius = Float(6.37123e6);
        int column_sorting = -1, sort_decided = -1;
        bool column_padding = true, reordered_call = false, sunlit_columns = false;
        std::unique_ptr<Gas_optics_rrtmgp_gpu> kdist_gpu;
        std::unique_ptr<Cloud_optics_gpu> cloud_optics_gpu;
        std::unique_ptr<Aerosol_optics_gpu> aerosol_optics_gpu;
        Rte_sw_gpu rte_sw;
        int vertical_ordering = -1;
        int n_col_block = 16384;
        bool broadband_solvers = true;
        bool byband_solvers = false;

        struct Workspace;
        std::shared_ptr<Workspace> ws_block, ws_residual;
};
#endif
