/*
 * rrx_hip.h -- C ABI of librrx_hip.so, the MI355X (gfx950) device layer of the RTE+RRTMGP hot path.
 *
 * This is the drop-in boundary: every entry point replaces ONE launcher of the
 * reference's device-side boundary `include_kernels_cuda/{...}.h` (30 functions in 5 namespaces) or ONE of the small
 * inline kernels of `src_cuda/{...}.cu`. The reference's namespaces (Rte_solver_kernels_cuda, ...) are kept as
 * header-only forwarders onto these symbols in include/rte_solver_kernels_cuda.h etc., so driver code written
 * against the reference compiles unchanged.
 *
 * Conventions (identical to the reference launchers unless stated):
 *   - plain C: scalars by value, arrays as raw DEVICE pointers, caller owns every array;
 *   - arrays are column-major with the column index fastest: (icol,ilay,igpt) at icol + ilay*ncol + igpt*ncol*nlay;
 *   - index-valued arrays hold 1-based values (band_lims_gpt, gpoint_flavor, jeta, jtemp, ...);
 *   - Bool is `signed char` (RTE_USE_CBOOL, the only setting any shipped reference config uses);
 *   - two precisions in one library: suffix _f64 (Float = double, reference default) and _f32 (RTE_USE_SP);
 *   - every function returns 0 on success, non-zero on error (message: rrx_last_error()); the C++ forwarders
 *     turn that into std::runtime_error, mirroring the reference's exception behaviour;
 *   - last argument `stream` is a hipStream_t passed as void* (NULL = the default stream, what the reference uses).
 *   - no function synchronises the device or allocates with hipMalloc; scratch (only rrx_*_solver in
 *     do_broadband mode) comes from the stream-ordered pool (hipMallocAsync).
 *
 * Citations are file:line under /root/reference.
 */
#ifndef RRX_HIP_H
#define RRX_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef signed char RrxBool;

/* ------------------------------------------------------------------ runtime ---------------------------------- */
/* replaces include/tools_gpu.h:72-99 (Tools_gpu::allocate_gpu/free_gpu), src_cuda/tools_gpu.cu, mem_pool_gpu.cu */
const char* rrx_last_error(void);
int rrx_device_count(int* n);
int rrx_set_device(int dev);
int rrx_malloc(void** ptr, unsigned long long bytes);
int rrx_free(void* ptr);
/* stream-ordered twins (what Array_gpu uses): allocation from the device's default memory pool with the release threshold lifted,
   so freed blocks are reused by the next solve and no call synchronises the device; the copies are enqueued on `stream` and awaited */
int rrx_malloc_async(void** ptr, unsigned long long bytes, void* stream);
int rrx_free_async(void* ptr, void* stream);
/* release of a block allocated under `alloc_stream` that may have been used under `release_stream` as well: the release stream waits
   for the allocation stream's work first; falls back to hipFree if the stream-ordered free fails (never leaks). The pool keeps
   freed blocks for reuse; RRX_POOL_RELEASE_THRESHOLD=<bytes> in the environment caps that (default: keep everything). */
int rrx_free_async_ordered(void* ptr, void* alloc_stream, void* release_stream);
int rrx_memcpy_h2d_stream(void* dst, const void* src, unsigned long long bytes, void* stream);
int rrx_memcpy_d2h_stream(void* dst, const void* src, unsigned long long bytes, void* stream);
int rrx_memcpy_h2d(void* dst, const void* src, unsigned long long bytes);
int rrx_memcpy_d2h(void* dst, const void* src, unsigned long long bytes);
int rrx_memcpy_d2d(void* dst, const void* src, unsigned long long bytes, void* stream);
int rrx_memset(void* dst, int value, unsigned long long bytes, void* stream);
int rrx_synchronize(void* stream);
int rrx_stream_create(void** stream);
int rrx_stream_destroy(void* stream);
/* The any-nlay solver forms (LW with several quadrature angles or Jacobians, columns of 288 layers and more, do_broadband outside
   the fused tilings) keep ONE grow-only block of device memory per (calling thread, device, stream) for their per-g-point
   temporaries. The stream owns it: rrx_stream_destroy returns it to the pool, and so does rrx_release_workspace (for streams the
   caller created itself -- call it from the thread that made the solver calls, before destroying the stream). A block larger than
   RRX_WORKSPACE_KEEP bytes (environment, default 32 GiB) is returned at the end of the call that used it. */
int rrx_release_workspace(void* stream);
/* perm[i] = min(i, ncol-1), i < ncol + npad: the identity order, padded (see rrx_sort_columns). ncol <= 0 or npad < 0: non-zero,
   "empty problem" */
int rrx_identity_columns(int ncol, int npad, int* perm, void* stream);
/* McICA cloud sampling (rrx_mcica_*): the identities of columns taken through a gather index, col_id[i] = perm[i] + offset, i < n
   (device ints). n = 0: returns 0, writes nothing; n < 0 or a NULL: non-zero. */
int rrx_mcica_column_ids(int n, const int* perm, int offset, int* col_id, void* stream);
unsigned long long rrx_workspace_bytes(void* stream);
/* include/Array.h:311-350,579-622 (Array_gpu::subset / subset_kernel): N-D block gather, singleton dimensions are
   broadcast. sub_dims/strides/starts/spread are HOST arrays of length ndim (1..7); strides in elements, starts 0-based; elem_bytes
   1, 4 or 8 (anything else, like an ndim outside 1..7, returns non-zero). A sub_dims entry of 0: returns 0, writes nothing. */
int rrx_subset_nd(void* out, const void* in, int elem_bytes, int ndim, const int* sub_dims, const long long* strides,
                  const int* starts, const int* spread, void* stream);
/* kernel-variant switches used by bench.py A/B runs (0 = default), per calling thread. LW: 0 default, 1 serial kernel (the test
   reference; the path of columns too tall for the others), 4 general kernel with 64-B rows, 7 never the one-kernel broadband form
   (per-g-point fluxes in a workspace + sum), 15 fp32: the one-column-per-lane one-kernel broadband form ahead of the others.
   SW: 0 default, 1 serial kernel, 7 never the one-kernel broadband form. Any other value returns non-zero, leaves the setting as
   it was, and rrx_last_error() lists the accepted values. */
int rrx_set_lw_variant(int v);
int rrx_set_sw_variant(int v);
/* workgroups the one-kernel broadband solvers aim for: with fewer column groups they split their g-point loop (see
   rrx_set_broadband_gsplit; default 512; 1 = never split) */
int rrx_set_broadband_min_groups(int n);
/* g-point ranges per column group in the one-kernel broadband solvers: 0 (default) = as many (a power of two, at most 16) as it
   takes to reach the workgroup count above when columns are few, 1 = never split, n = n ranges. Partial sums are added in
   range order by a second kernel: deterministic, but not the association of the unsplit sum. */
int rrx_set_broadband_gsplit(int n);
/* 1 (default): the "direct" gas optics run the windowed kernel (LUT boxes staged in LDS) ahead of the gather kernel;
   0: gather kernel only (A/B runs, tests). Like the other switches it acts on the calling host thread. */
int rrx_set_gas_window(int on);
/* diagnostic: with RRX_GW_STATS set in the environment every windowed gas-optics launch waits for its kernel and counts the
   workgroups it handed back to the gather kernel; this returns (and optionally resets) the calling thread's totals */
int rrx_gas_window_stats(long long* handed_back, long long* workgroups, int reset);
/* diagnostic (tests): the index tables of the calling thread's last windowed gas-optics launch, copied to the host after a device
   synchronisation. layout[16]: ints in all (tables + header), ngpt, nmax, ncmax, the offsets of the chunk starts, contributor lists,
   contributor metadata, usable flags, chunk order, per-g-point bands and key species, unusable-chunk counts and chunk records, then
   ints per list, per metadata entry, per record and per record header. tables == NULL: the layout only. */
int rrx_gas_window_tables_read(int* tables, int capacity, int* layout);

#define RRX_DECLARE(F, SFX) \
/* ---- Rte_solver_kernels_cuda : include_kernels_cuda/rte_solver_kernels_cuda.h:33-64 ---- */ \
/* apply_BC x3: src_kernels_cuda/rte_solver_kernels_launchers.cu:20-45 */ \
int rrx_apply_BC_factor##SFX(int ncol, int nlay, int ngpt, RrxBool top_at_1, const F* inc_flux_dir, const F* mu0, F* gpt_flux_dir, void* stream); \
int rrx_apply_BC_0##SFX(int ncol, int nlay, int ngpt, RrxBool top_at_1, F* gpt_flux_dn, void* stream); \
int rrx_apply_BC_gpt##SFX(int ncol, int nlay, int ngpt, RrxBool top_at_1, const F* inc_flux_dif, F* gpt_flux_dn, void* stream); \
/* lw_secants_array: launchers.cu:48-58 */ \
int rrx_lw_secants_array##SFX(int ncol, int ngpt, int n_gauss_quad, int max_gauss_pts, const F* gauss_Ds, F* secants, void* stream); \
/* lw_solver_noscat: launchers.cu:61-286. Beyond the reference GPU path it honours do_broadband (flux_*_loc = \
   (ncol,nlay+1) g-point sums, the CPU/Fortran behaviour, src/Rte_lw.cpp:176), do_jacobians and nmus 1..4. */ \
int rrx_lw_solver_noscat##SFX( \
        int ncol, int nlay, int ngpt, RrxBool top_at_1, int nmus, \
        const F* secants, const F* weights, \
        const F* tau, const F* lay_source, const F* lev_source, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, \
        F* flux_up, F* flux_dn, \
        RrxBool do_broadband, F* flux_up_loc, F* flux_dn_loc, \
        RrxBool do_jacobians, const F* sfc_src_jac, F* flux_up_jac, void* stream); \
/* sw_solver_2stream: launchers.cu:289-447. mu0 is (ncol) as on the reference GPU path; sfc_alb_dir is indexed \
   per g-point (Fortran semantics); has_dif_bc and do_broadband are honoured. g may be NULL = asymmetry \
   identically zero (what clear-sky gas optics produce): same fluxes as with an array of zeros, which is not read. */ \
int rrx_sw_solver_2stream##SFX( \
        int ncol, int nlay, int ngpt, RrxBool top_at_1, \
        const F* tau, const F* ssa, const F* g, const F* mu0, \
        const F* sfc_alb_dir, const F* sfc_alb_dif, const F* inc_flux_dir, \
        F* flux_up, F* flux_dn, F* flux_dir, \
        RrxBool has_dif_bc, const F* inc_flux_dif, \
        RrxBool do_broadband, F* flux_up_loc, F* flux_dn_loc, F* flux_dir_loc, void* stream); \
/* sw_solver_2stream_byband: by-band fluxes from the fused broadband solver -- bnd_flux_* are (ncol, nlay+1, nbnd) arrays, \
   bnd_flux(icol, ilev, ibnd) = the sum of the band's g-point fluxes (the g-points in order, as rrx_sum_byband); band_lims_gpt is \
   (2, nbnd), 1-based and inclusive, a band with hi < lo is empty (zeros). bnd_flux_net = bnd_flux_dn - bnd_flux_up; flux_up/dn/dir \
   = the band sums added in band order. Those four are optional (NULL: not written). Other arguments as rrx_sw_solver_2stream. */ \
int rrx_sw_solver_2stream_byband##SFX( \
        int ncol, int nlay, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const F* g, const F* mu0, const F* sfc_alb_dir, const F* sfc_alb_dif, \
        const F* inc_flux_dir, RrxBool has_dif_bc, const F* inc_flux_dif, const int* band_lims_gpt, \
        F* bnd_flux_up, F* bnd_flux_dn, F* bnd_flux_dir, F* bnd_flux_net, \
        F* flux_up, F* flux_dn, F* flux_dir, void* stream); \
/* mu0 by layer (upstream RTE's mu0(ncol,nlay), no counterpart on the reference GPU path): the two solvers above with \
   mu0_lay (ncol, nlay) in the place of mu0. Layer l of a column takes mu0_lay(icol, l) in its two-stream coefficients and its direct \
   transmission; the direct beam at the top level is inc_flux_dir x mu0_lay(icol, top layer) (layer 0 with top_at_1, nlay-1 without). \
   All other arguments, do_broadband, has_dif_bc and g == NULL as there; with identical rows the fluxes of the 1-D entries. */ \
int rrx_sw_solver_2stream_mu0lay##SFX( \
        int ncol, int nlay, int ngpt, RrxBool top_at_1, \
        const F* tau, const F* ssa, const F* g, const F* mu0_lay, \
        const F* sfc_alb_dir, const F* sfc_alb_dif, const F* inc_flux_dir, \
        F* flux_up, F* flux_dn, F* flux_dir, \
        RrxBool has_dif_bc, const F* inc_flux_dif, \
        RrxBool do_broadband, F* flux_up_loc, F* flux_dn_loc, F* flux_dir_loc, void* stream); \
int rrx_sw_solver_2stream_byband_mu0lay##SFX( \
        int ncol, int nlay, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const F* g, const F* mu0_lay, const F* sfc_alb_dir, const F* sfc_alb_dif, \
        const F* inc_flux_dir, RrxBool has_dif_bc, const F* inc_flux_dif, const int* band_lims_gpt, \
        F* bnd_flux_up, F* bnd_flux_dn, F* bnd_flux_dir, F* bnd_flux_net, \
        F* flux_up, F* flux_dn, F* flux_dir, void* stream); \
/* Spherical-geometry correction of the solar zenith angle (upstream RTE's zenith_angle_spherical_correction): \
   mu0_lay(icol, l) = sqrt(max(0, 1 - (1 - ref_mu^2) ((R + ref_alt) / (R + alt(icol, l)))^2)) where ref_mu(icol) > 0, and ref_mu(icol) \
   otherwise (a dark column stays dark). alt (ncol, nlay): layer altitudes in metres; ref_alt (ncol): the altitude at which ref_mu \
   holds, NULL = 0; planet_radius R in metres (the Earth: 6.37123e6). ncol or nlay = 0: returns 0 without a launch; a negative \
   extent, a NULL that is needed or R <= 0: non-zero, before any HIP call. */ \
int rrx_zenith_angle_spherical_correction##SFX(int ncol, int nlay, const F* ref_alt, const F* ref_mu, const F* alt, F planet_radius, \
        F* mu0_lay, void* stream); \
/* ---- Gas_optics_rrtmgp_kernels_cuda : include_kernels_cuda/gas_optics_rrtmgp_kernels_cuda.h:33-132 ---- */ \
int rrx_reorder123x321##SFX(int ni, int nj, int nk, const F* arr_in, F* arr_out, void* stream); \
int rrx_reorder12x21##SFX(int ni, int nj, const F* arr_in, F* arr_out, void* stream); \
int rrx_zero_array##SFX(int ni, int nj, int nk, F* arr, void* stream); \
/* interpolation: gas_optics_rrtmgp_kernels_launchers.cu:91-125 */ \
int rrx_interpolation##SFX( \
        int ncol, int nlay, int ngas, int nflav, int neta, int npres, int ntemp, \
        const int* flavor, const F* press_ref_log, const F* temp_ref, \
        F press_ref_log_delta, F temp_ref_min, F temp_ref_delta, F press_ref_trop_log, \
        const F* vmr_ref, const F* play, const F* tlay, F* col_gas, \
        int* jtemp, F* fmajor, F* fminor, F* col_mix, RrxBool* tropo, int* jeta, int* jpress, void* stream); \
/* combine_abs_and_rayleigh: launchers.cu:128-165 (ssa threshold 2*epsilon: CPU semantics, src/Gas_optics_rrtmgp.cpp:378) */ \
int rrx_combine_abs_and_rayleigh##SFX(int ncol, int nlay, int ngpt, const F* tau_abs, const F* tau_rayleigh, F* tau, F* ssa, F* g, void* stream); \
/* compute_tau_rayleigh: launchers.cu:168-221 */ \
int rrx_compute_tau_rayleigh##SFX( \
        int ncol, int nlay, int nbnd, int ngpt, int ngas, int nflav, int neta, int npres, int ntemp, \
        const int* gpoint_flavor, const int* band_lims_gpt, const F* krayl, \
        int idx_h2o, const F* col_dry, const F* col_gas, \
        const F* fminor, const int* jeta, const RrxBool* tropo, const int* jtemp, F* tau_rayleigh, void* stream); \
/* compute_tau_absorption: launchers.cu:234-438 (major + minor lower + minor upper, ADDED onto tau) */ \
int rrx_compute_tau_absorption##SFX( \
        int ncol, int nlay, int nband, int ngpt, int ngas, int nflav, int neta, int npres, int ntemp, \
        int nminorlower, int nminorklower, int nminorupper, int nminorkupper, int idx_h2o, \
        const int* gpoint_flavor, const int* band_lims_gpt, \
        const F* kmajor, const F* kminor_lower, const F* kminor_upper, \
        const int* minor_limits_gpt_lower, const int* minor_limits_gpt_upper, \
        const RrxBool* minor_scales_with_density_lower, const RrxBool* minor_scales_with_density_upper, \
        const RrxBool* scale_by_complement_lower, const RrxBool* scale_by_complement_upper, \
        const int* idx_minor_lower, const int* idx_minor_upper, \
        const int* idx_minor_scaling_lower, const int* idx_minor_scaling_upper, \
        const int* kminor_start_lower, const int* kminor_start_upper, \
        const RrxBool* tropo, const F* col_mix, const F* fmajor, const F* fminor, \
        const F* play, const F* tlay, const F* col_gas, \
        const int* jeta, const int* jtemp, const int* jpress, F* tau, void* stream); \
/* addition: the same sum STORED into tau (what Gas_optics_rrtmgp_gpu needs after its zero fill: src_cuda/Gas_optics_rrtmgp.cu \
   compute_gas_taus; saves the fill and the read-back) */ \
int rrx_compute_tau_absorption_set##SFX( \
        int ncol, int nlay, int nband, int ngpt, int ngas, int nflav, int neta, int npres, int ntemp, \
        int nminorlower, int nminorklower, int nminorupper, int nminorkupper, int idx_h2o, \
        const int* gpoint_flavor, const int* band_lims_gpt, \
        const F* kmajor, const F* kminor_lower, const F* kminor_upper, \
        const int* minor_limits_gpt_lower, const int* minor_limits_gpt_upper, \
        const RrxBool* minor_scales_with_density_lower, const RrxBool* minor_scales_with_density_upper, \
        const RrxBool* scale_by_complement_lower, const RrxBool* scale_by_complement_upper, \
        const int* idx_minor_lower, const int* idx_minor_upper, \
        const int* idx_minor_scaling_lower, const int* idx_minor_scaling_upper, \
        const int* kminor_start_lower, const int* kminor_start_upper, \
        const RrxBool* tropo, const F* col_mix, const F* fmajor, const F* fminor, \
        const F* play, const F* tlay, const F* col_gas, \
        const int* jeta, const int* jtemp, const int* jpress, F* tau, void* stream); \
/* compute_planck_source: launchers.cu:441-521 */ \
int rrx_compute_planck_source##SFX( \
        int ncol, int nlay, int nbnd, int ngpt, int nflav, int neta, int npres, int ntemp, int nPlanckTemp, \
        const F* tlay, const F* tlev, const F* tsfc, int sfc_lay, \
        const F* fmajor, const int* jeta, const RrxBool* tropo, const int* jtemp, const int* jpress, \
        const int* gpoint_bands, const int* band_lims_gpt, const F* pfracin, \
        F temp_ref_min, F totplnk_delta, const F* totplnk, const int* gpoint_flavor, \
        F* sfc_src, F* lay_src, F* lev_src, F* sfc_src_jac, void* stream); \
/* fused SW gas optics used by Gas_optics_rrtmgp_gpu (tau_abs + tau_rayleigh + combine in one pass, tau/ssa/g \
   written once; same arithmetic as the three launchers above called in sequence on a zeroed tau). g may be NULL: \
   the asymmetry parameter of the gas optics is identically zero and is then not written */ \
int rrx_gas_optics_sw_fused##SFX( \
        int ncol, int nlay, int nband, int ngpt, int ngas, int nflav, int neta, int npres, int ntemp, \
        int nminorlower, int nminorklower, int nminorupper, int nminorkupper, int idx_h2o, \
        const int* gpoint_flavor, const int* band_lims_gpt, \
        const F* kmajor, const F* kminor_lower, const F* kminor_upper, \
        const int* minor_limits_gpt_lower, const int* minor_limits_gpt_upper, \
        const RrxBool* minor_scales_with_density_lower, const RrxBool* minor_scales_with_density_upper, \
        const RrxBool* scale_by_complement_lower, const RrxBool* scale_by_complement_upper, \
        const int* idx_minor_lower, const int* idx_minor_upper, \
        const int* idx_minor_scaling_lower, const int* idx_minor_scaling_upper, \
        const int* kminor_start_lower, const int* kminor_start_upper, \
        const RrxBool* tropo, const F* col_mix, const F* fmajor, const F* fminor, \
        const F* play, const F* tlay, const F* col_gas, const F* col_dry, \
        const int* jeta, const int* jtemp, const int* jpress, const F* krayl, \
        F* tau, F* ssa, F* g, void* stream); \
/* "direct" gas optics: the interpolation state (interpolation_kernel, gas_optics_rrtmgp_kernels.cu:317-395) is computed \
   inside the consumer from (play, tlay, col_gas) instead of being written by rrx_interpolation and read back by \
   rrx_compute_tau_absorption / rrx_compute_planck_source: same expressions in the same order, so the same bits, without \
   the seven intermediate arrays (jtemp, jpress, tropo, jeta, col_mix, fminor, fmajor). What Gas_optics_rrtmgp_gpu::gas_optics \
   (src_cuda/Gas_optics_rrtmgp.cu:907-1201) runs here. flavor(2,nflav), vmr_ref(2,0:ngas,ntemp) as for rrx_interpolation. */ \
int rrx_gas_optics_lw_direct##SFX( \
        int ncol, int nlay, int nband, int ngpt, int ngas, int nflav, int neta, int npres, int ntemp, \
        int nminorlower, int nminorklower, int nminorupper, int nminorkupper, int idx_h2o, \
        const int* gpoint_flavor, const int* band_lims_gpt, \
        const F* kmajor, const F* kminor_lower, const F* kminor_upper, \
        const int* minor_limits_gpt_lower, const int* minor_limits_gpt_upper, \
        const RrxBool* minor_scales_with_density_lower, const RrxBool* minor_scales_with_density_upper, \
        const RrxBool* scale_by_complement_lower, const RrxBool* scale_by_complement_upper, \
        const int* idx_minor_lower, const int* idx_minor_upper, \
        const int* idx_minor_scaling_lower, const int* idx_minor_scaling_upper, \
        const int* kminor_start_lower, const int* kminor_start_upper, \
        const int* flavor, const F* press_ref_log, const F* temp_ref, \
        F press_ref_log_delta, F temp_ref_min, F temp_ref_delta, F press_ref_trop_log, const F* vmr_ref, \
        const F* play, const F* tlay, const F* col_gas, F* tau, void* stream); \
/* rrx_gas_optics_lw_direct with optical properties given by band (clouds, aerosols: cld_* are (ncol,nlay,nbnd) arrays, bands delimited by \
   band_lims_gpt) added where the gas optics is stored -- increment_1scalar_by_1scalar_bybnd folded into the producer, same \
   arithmetic and bits, without reading and re-writing the g-point arrays; cld_tau = NULL: the plain entry */ \
int rrx_gas_optics_lw_direct_allsky##SFX( \
        int ncol, int nlay, int nband, int ngpt, int ngas, int nflav, int neta, int npres, int ntemp, \
        int nminorlower, int nminorklower, int nminorupper, int nminorkupper, int idx_h2o, \
        const int* gpoint_flavor, const int* band_lims_gpt, \
        const F* kmajor, const F* kminor_lower, const F* kminor_upper, \
        const int* minor_limits_gpt_lower, const int* minor_limits_gpt_upper, \
        const RrxBool* minor_scales_with_density_lower, const RrxBool* minor_scales_with_density_upper, \
        const RrxBool* scale_by_complement_lower, const RrxBool* scale_by_complement_upper, \
        const int* idx_minor_lower, const int* idx_minor_upper, \
        const int* idx_minor_scaling_lower, const int* idx_minor_scaling_upper, \
        const int* kminor_start_lower, const int* kminor_start_upper, \
        const int* flavor, const F* press_ref_log, const F* temp_ref, \
        F press_ref_log_delta, F temp_ref_min, F temp_ref_delta, F press_ref_trop_log, const F* vmr_ref, \
        const F* play, const F* tlay, const F* col_gas, F* tau, const F* cld_tau, void* stream); \
int rrx_gas_optics_sw_direct##SFX( \
        int ncol, int nlay, int nband, int ngpt, int ngas, int nflav, int neta, int npres, int ntemp, \
        int nminorlower, int nminorklower, int nminorupper, int nminorkupper, int idx_h2o, \
        const int* gpoint_flavor, const int* band_lims_gpt, \
        const F* kmajor, const F* kminor_lower, const F* kminor_upper, \
        const int* minor_limits_gpt_lower, const int* minor_limits_gpt_upper, \
        const RrxBool* minor_scales_with_density_lower, const RrxBool* minor_scales_with_density_upper, \
        const RrxBool* scale_by_complement_lower, const RrxBool* scale_by_complement_upper, \
        const int* idx_minor_lower, const int* idx_minor_upper, \
        const int* idx_minor_scaling_lower, const int* idx_minor_scaling_upper, \
        const int* kminor_start_lower, const int* kminor_start_upper, \
        const int* flavor, const F* press_ref_log, const F* temp_ref, \
        F press_ref_log_delta, F temp_ref_min, F temp_ref_delta, F press_ref_trop_log, const F* vmr_ref, \
        const F* play, const F* tlay, const F* col_gas, const F* col_dry, const F* krayl, \
        F* tau, F* ssa, F* g, void* stream); \
/* rrx_gas_optics_sw_direct with optical properties given by band (clouds, aerosols: cld_* are (ncol,nlay,nbnd) arrays, bands delimited by \
   band_lims_gpt) added where the gas optics is stored -- increment_2stream_by_2stream_bybnd folded into the producer, same \
   arithmetic and bits, without reading and re-writing the g-point arrays (g must be given); cld_tau = NULL: the plain entry */ \
int rrx_gas_optics_sw_direct_allsky##SFX( \
        int ncol, int nlay, int nband, int ngpt, int ngas, int nflav, int neta, int npres, int ntemp, \
        int nminorlower, int nminorklower, int nminorupper, int nminorkupper, int idx_h2o, \
        const int* gpoint_flavor, const int* band_lims_gpt, \
        const F* kmajor, const F* kminor_lower, const F* kminor_upper, \
        const int* minor_limits_gpt_lower, const int* minor_limits_gpt_upper, \
        const RrxBool* minor_scales_with_density_lower, const RrxBool* minor_scales_with_density_upper, \
        const RrxBool* scale_by_complement_lower, const RrxBool* scale_by_complement_upper, \
        const int* idx_minor_lower, const int* idx_minor_upper, \
        const int* idx_minor_scaling_lower, const int* idx_minor_scaling_upper, \
        const int* kminor_start_lower, const int* kminor_start_upper, \
        const int* flavor, const F* press_ref_log, const F* temp_ref, \
        F press_ref_log_delta, F temp_ref_min, F temp_ref_delta, F press_ref_trop_log, const F* vmr_ref, \
        const F* play, const F* tlay, const F* col_gas, const F* col_dry, const F* krayl, \
        F* tau, F* ssa, F* g, const F* cld_tau, const F* cld_ssa, const F* cld_g, void* stream); \
int rrx_planck_source_direct##SFX( \
        int ncol, int nlay, int nbnd, int ngpt, int ngas, int nflav, int neta, int npres, int ntemp, int nPlanckTemp, \
        const F* play, const F* tlay, const F* tlev, const F* tsfc, int sfc_lay, const F* col_gas, \
        const int* flavor, const F* press_ref_log, const F* temp_ref, \
        F press_ref_log_delta, F temp_ref_min, F temp_ref_delta, F press_ref_trop_log, const F* vmr_ref, \
        const int* gpoint_bands, const int* band_lims_gpt, const F* pfracin, \
        F totplnk_delta, const F* totplnk, const int* gpoint_flavor, \
        F* sfc_src, F* lay_src, F* lev_src, F* sfc_src_jac, void* stream); \
/* "Planck-lite" LW chain (what Gas_optics_rrtmgp_gpu::source + Rte_lw_gpu::rte_lw run here in broadband mode): \
   rrx_planck_fractions writes the Planck fractions pfrac(ncol,nlay,ngpt), the band Planck functions B(tlay)(ncol,nlay,nbnd) and \
   B(tlev)(ncol,nlay+1,nbnd) and the surface terms -- Planck_source_kernel (gas_optics_rrtmgp_kernels.cu:196-314) without its two \
   products; rrx_lw_solver_noscat_fractions (one quadrature angle, broadband fluxes) forms lay_source = pfrac*B_lay and \
   lev_source = sqrt(pfrac*pfrac')*B_lev on the fly; rrx_planck_sources_from_fractions materialises them for any other consumer \
   (bit-identical to rrx_compute_planck_source). */ \
int rrx_planck_fractions##SFX( \
        int ncol, int nlay, int nbnd, int ngpt, int ngas, int nflav, int neta, int npres, int ntemp, int nPlanckTemp, \
        const F* play, const F* tlay, const F* tlev, const F* tsfc, int sfc_lay, const F* col_gas, \
        const int* flavor, const F* press_ref_log, const F* temp_ref, \
        F press_ref_log_delta, F temp_ref_min, F temp_ref_delta, F press_ref_trop_log, const F* vmr_ref, \
        const int* gpoint_bands, const int* band_lims_gpt, const F* pfracin, \
        F totplnk_delta, const F* totplnk, const int* gpoint_flavor, \
        F* pfrac, F* blay, F* blev, F* sfc_src, F* sfc_src_jac, void* stream); \
/* rrx_gas_optics_lw_direct + rrx_planck_fractions in one pass over the cells: the interpolation state and the LUT windows are \
   shared -- the LW gas optics of Gas_optics_rrtmgp_gpu in broadband mode */ \
int rrx_gas_optics_lw_fractions##SFX( \
        int ncol, int nlay, int nband, int ngpt, int ngas, int nflav, int neta, int npres, int ntemp, int nPlanckTemp, \
        int nminorlower, int nminorklower, int nminorupper, int nminorkupper, int idx_h2o, \
        const int* gpoint_flavor, const int* band_lims_gpt, const int* gpoint_bands, \
        const F* kmajor, const F* kminor_lower, const F* kminor_upper, \
        const int* minor_limits_gpt_lower, const int* minor_limits_gpt_upper, \
        const RrxBool* minor_scales_with_density_lower, const RrxBool* minor_scales_with_density_upper, \
        const RrxBool* scale_by_complement_lower, const RrxBool* scale_by_complement_upper, \
        const int* idx_minor_lower, const int* idx_minor_upper, \
        const int* idx_minor_scaling_lower, const int* idx_minor_scaling_upper, \
        const int* kminor_start_lower, const int* kminor_start_upper, \
        const int* flavor, const F* press_ref_log, const F* temp_ref, \
        F press_ref_log_delta, F temp_ref_min, F temp_ref_delta, F press_ref_trop_log, const F* vmr_ref, \
        const F* play, const F* tlay, const F* tlev, const F* tsfc, int sfc_lay, const F* col_gas, \
        const F* pfracin, F totplnk_delta, const F* totplnk, \
        F* tau, F* pfrac, F* blay, F* blev, F* sfc_src, F* sfc_src_jac, void* stream); \
/* rrx_gas_optics_lw_fractions with optical properties given by band (clouds, aerosols: cld_* are (ncol,nlay,nbnd) arrays, bands delimited by \
   band_lims_gpt) added where the gas optics is stored -- increment_1scalar_by_1scalar_bybnd folded into the producer, same \
   arithmetic and bits, without reading and re-writing the g-point arrays; cld_tau = NULL: the plain entry */ \
int rrx_gas_optics_lw_fractions_allsky##SFX( \
        int ncol, int nlay, int nband, int ngpt, int ngas, int nflav, int neta, int npres, int ntemp, int nPlanckTemp, \
        int nminorlower, int nminorklower, int nminorupper, int nminorkupper, int idx_h2o, \
        const int* gpoint_flavor, const int* band_lims_gpt, const int* gpoint_bands, \
        const F* kmajor, const F* kminor_lower, const F* kminor_upper, \
        const int* minor_limits_gpt_lower, const int* minor_limits_gpt_upper, \
        const RrxBool* minor_scales_with_density_lower, const RrxBool* minor_scales_with_density_upper, \
        const RrxBool* scale_by_complement_lower, const RrxBool* scale_by_complement_upper, \
        const int* idx_minor_lower, const int* idx_minor_upper, \
        const int* idx_minor_scaling_lower, const int* idx_minor_scaling_upper, \
        const int* kminor_start_lower, const int* kminor_start_upper, \
        const int* flavor, const F* press_ref_log, const F* temp_ref, \
        F press_ref_log_delta, F temp_ref_min, F temp_ref_delta, F press_ref_trop_log, const F* vmr_ref, \
        const F* play, const F* tlay, const F* tlev, const F* tsfc, int sfc_lay, const F* col_gas, \
        const F* pfracin, F totplnk_delta, const F* totplnk, \
        F* tau, F* pfrac, F* blay, F* blev, F* sfc_src, F* sfc_src_jac, const F* cld_tau, void* stream); \
int rrx_planck_sources_from_fractions##SFX(int ncol, int nlay, int ngpt, const int* gpoint_bands, const F* pfrac, const F* blay, \
        const F* blev, F* lay_src, F* lev_src, void* stream); \
int rrx_lw_solver_noscat_fractions##SFX( \
        int ncol, int nlay, int ngpt, RrxBool top_at_1, const F* secants, const F* weights, \
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up_loc, F* flux_dn_loc, void* stream); \
/* by-band fluxes of rrx_lw_solver_noscat_fractions: bnd_flux_up/dn are (ncol, nlay+1, nbnd) band sums (layout and band_lims_gpt as \
   rrx_sw_solver_2stream_byband); bnd_flux_net = dn - up per band, flux_up/dn = the band sums added in band order (optional, NULL: \
   not written) */ \
int rrx_lw_solver_noscat_fractions_byband##SFX( \
        int ncol, int nlay, int ngpt, int nbnd, RrxBool top_at_1, const F* secants, const F* weights, \
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, const int* band_lims_gpt, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, \
        F* bnd_flux_up, F* bnd_flux_dn, F* bnd_flux_net, F* flux_up, F* flux_dn, void* stream); \
/* rrx_lw_solver_noscat_fractions plus the surface-temperature Jacobian of the upward flux from the same solve: sfc_src_jac is \
   (ngpt, ncol) (d sfc_src / d T_sfc over 1 K, as rrx_gas_optics_lw_fractions writes it), flux_up_jac (ncol, nlay+1) in W m-2 K-1 \
   = sum over g-points of pi*w*J_g, J_g(surface) = sfc_emis*sfc_src_jac, J_g(level) = trans(layer below)*J_g(level below). \
   flux_up_loc / flux_dn_loc are bit for bit those of rrx_lw_solver_noscat_fractions */ \
int rrx_lw_solver_noscat_fractions_jac##SFX( \
        int ncol, int nlay, int ngpt, RrxBool top_at_1, const F* secants, const F* weights, \
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up_loc, F* flux_dn_loc, \
        const F* sfc_src_jac, F* flux_up_jac, void* stream); \
/* rrx_lw_solver_noscat_fractions [_jac] with nmus = 1..4 quadrature angles in one kernel: every g-point's tau and Planck fractions \
   are read once and the solve runs nmus times on them. secants is (ncol, ngpt, nmus) and is read per column and g-point (it need \
   not be the broadcast of rrx_lw_secants_array), weights is (nmus). Each angle's pi*weights[imu]*radiance is added to the running \
   g-point sum in the order (g-point, angle); the per-g-point route adds a g-point's angles first, a difference of rounding only. \
   sfc_src_jac and flux_up_jac are both NULL (fluxes only) or both given (Jacobian as in the _jac entry, the same weights). \
   nmus = 1 forwards to the one-angle entries: the same bits. No by-band form. Shapes outside the one-kernel tilings take the \
   per-g-point kernels with the same nmus */ \
int rrx_lw_solver_noscat_fractions_angles##SFX( \
        int ncol, int nlay, int ngpt, RrxBool top_at_1, int nmus, const F* secants, const F* weights, \
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up_loc, F* flux_dn_loc, \
        const F* sfc_src_jac, F* flux_up_jac, void* stream); \
/* host-model update between radiation calls (no counterpart in the reference library): with d = flux_up_jac * (t_sfc_new - \
   t_sfc_old) of the level's column, flux_up += d and (flux_net not NULL) flux_net -= d; flux arrays (ncol, nlev), t_sfc (ncol) */ \
int rrx_lw_flux_up_adjust##SFX(int ncol, int nlev, const F* flux_up_jac, const F* t_sfc_old, const F* t_sfc_new, \
        F* flux_up, F* flux_net, void* stream); \
/* Optimal-angle secants (compute_optimal_angles / lw_Ds of current RTE+RRTMGP; no counterpart in the reference library): for column c \
   and g-point g of band b = gpoint_bands[g], S = the sum of tau(c, :, g) over all layers and D(c, g) = fit(1,b)*exp(-S) + fit(2,b), \
   the secant of a one-angle solve. optimal_angle_fit is (2, nbnd), first index fastest; D is not clamped. \
   rrx_lw_optimal_secants writes D to secants (ncol, ngpt) in one pass over tau (layers added in index order from zero). */ \
int rrx_lw_optimal_secants##SFX(int ncol, int nlay, int ngpt, int nbnd, const int* gpoint_bands, const F* optimal_angle_fit, \
        const F* tau, F* secants, void* stream); \
/* rrx_lw_solver_noscat_fractions [_jac] with those secants formed inside the kernel from the g-point it holds (tau is not read a \
   second time, no secants array is read): one angle, weights (1). sfc_src_jac and flux_up_jac are both NULL or both given, as in \
   the _angles entry. secants_out (ncol, ngpt) or NULL: the D the solve used. The kernel's sum over the layers is a tree over lanes \
   and waves, so D may differ from rrx_lw_optimal_secants in the last bits. No by-band form. Shapes outside the one-kernel tilings \
   take rrx_lw_optimal_secants and the per-g-point kernels */ \
int rrx_lw_solver_noscat_fractions_optimal##SFX( \
        int ncol, int nlay, int ngpt, int nbnd, RrxBool top_at_1, const F* weights, \
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, const F* optimal_angle_fit, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up_loc, F* flux_dn_loc, \
        const F* sfc_src_jac, F* flux_up_jac, F* secants_out, void* stream); \
/* Test entry (no counterpart in the reference library): the solvers' device math primitives of csrc/rrx_common.h applied element-wise, \
   y[i] = f(x[i]) for i < n, so that their documented accuracy can be measured on the device. which = 0: exp_neg (fp64: the \
   polynomial form; fp32: the v_exp_f32 form), 1: exp_neg in its LDS-table form, the table filled as the fused LW solver fills it \
   (fp32: the same function as 0), 2: fast_rcp, 3: sqrt_pos, 4: sqrt_nonneg. The arguments must lie in the primitive's documented \
   domain. Any other `which`, a negative n, or a NULL x or y with n > 0: non-zero, nothing launched; n = 0 returns 0. */ \
int rrx_math_selftest##SFX(int which, int n, const F* x, F* y, void* stream); \
/* lw_solver_2stream: the LW two-stream solver WITH scattering (current RTE+RRTMGP; the reference has none). Per g-point and column, \
   layers and levels in sweep order from the top, D = 1.66: \
     gamma1 = D (1 - ssa (1 + g)/2), gamma2 = D ssa (1 - g)/2, k = sqrt(max((gamma1 - gamma2)(gamma1 + gamma2), 1e-12)), \
     e1 = exp(-tau k), e2 = e1 e1, RT = 1/(k (1 + e2) + gamma1 (1 - e2)), Rdif = RT gamma2 (1 - e2), Tdif = 2 RT k e1; \
     tau > 1e-8: Z = (lev_bot - lev_top)/(tau (gamma1 + gamma2)), src_up = pi ((Z + lev_top) - Rdif (-Z + lev_top) - Tdif (Z + lev_bot)), \
     src_dn = pi ((-Z + lev_bot) - Rdif (Z + lev_bot) - Tdif (-Z + lev_top)), otherwise both 0 (lev_* = lev_source at the layer's upper \
     and lower level; no layer source is used); surface albedo 1 - sfc_emis and source pi sfc_emis sfc_src; flux_dn at the top = \
     inc_flux, or 0 when it is NULL; transport by the adding recurrences of rrx_sw_solver_2stream's diffuse part. \
   (The kernels evaluate the sources in a regrouped form of the same function that does not multiply a rounding error by Z.) \
   No secants and no weights: the outputs are fluxes. tau, ssa, g (ncol, nlay, ngpt), lev_source (ncol, nlay+1, ngpt); sfc_emis, \
   sfc_src, inc_flux (ncol, ngpt) as rrx_lw_solver_noscat takes them. do_broadband = 0: flux_up / flux_dn (ncol, nlay+1, ngpt). \
   do_broadband = 1: flux_up_loc / flux_dn_loc (ncol, nlay+1) = the g-point sums in rrx_sum_broadband's order; flux_up / flux_dn are \
   then optional per-g-point outputs (both NULL: the stream's workspace holds them). Any nlay, one thread per (column, g-point). \
   A NULL required pointer or a negative extent: non-zero, rrx_last_error() names the entry and the argument; an extent of 0 \
   returns 0 and writes nothing. */ \
int rrx_lw_solver_2stream##SFX( \
        int ncol, int nlay, int ngpt, RrxBool top_at_1, \
        const F* tau, const F* ssa, const F* g, const F* lev_source, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, \
        F* flux_up, F* flux_dn, RrxBool do_broadband, F* flux_up_loc, F* flux_dn_loc, void* stream); \
/* The same solve from Planck-lite inputs with band cloud properties, broadband outputs, in one kernel: tau (ncol, nlay, ngpt) is the \
   clear gas optical depth, lev_source is formed as rrx_planck_sources_from_fractions forms lev_src from pfrac (ncol, nlay, ngpt) and \
   blev (ncol, nlay+1, nbnd), and cld_tau / cld_ssa / cld_g (ncol, nlay, nbnd) are combined per g-point of their band with the \
   arithmetic of rrx_inc_2stream_by_2stream_bybnd on gas (tau, 0, 0): tau' = tau + tau_c, ssa = tau_c ssa_c / max(eps, tau'), \
   g = tau_c ssa_c g_c / max(eps, tau_c ssa_c) (the one-kernel form takes ssa = 0 where tau_c ssa_c = 0 and g = g_c: where these \
   differ from the formulas by more than a rounding, tau_c ssa_c is below eps, ssa = 0 and g multiplies nothing). The three cloud arrays are all NULL (pure absorption, ssa = 0: the bits of all-zero \
   arrays) or all given; a partly-NULL triple is refused. gpoint_bands (ngpt) and band_lims_gpt (2, nbnd) as everywhere, 1-based. \
   flux_up / flux_dn (ncol, nlay+1): g-point sums in rrx_sum_broadband's order. One-kernel tilings up to 575 layers; taller columns \
   and LW variants 1 and 7 materialise the combined properties and lev_source in the stream's workspace and take \
   rrx_lw_solver_2stream. Argument checks and empty problems as there. */ \
int rrx_lw_solver_2stream_fractions##SFX( \
        int ncol, int nlay, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* pfrac, const F* blev, const int* gpoint_bands, const int* band_lims_gpt, \
        const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up, F* flux_dn, void* stream); \
/* lw_solver_noscat_rescaled: the no-scattering solve on a rescaled optical depth with one correction sweep (Tang et al. 2018; \
   current RTE+RRTMGP's "1rescl" answer to two-stream optical properties in the longwave; do_rescaling of the reference's CPU \
   boundary). Per g-point, column and angle, layers i and levels in sweep order from the top: \
     wb = ssa (1 - g)/2, st = 1 - ssa + wb, Cn = 0.4 wb / max(st, 3 tiny), tl = tau D st, tr = exp(-tl), An = 1 - tr tr; \
     sdn, sup = rrx_lw_solver_noscat's layer sources evaluated with tl, tr; \
     pass 1 (down) dn[i+1] = tr dn[i] + sdn; surface up[nlay] = dn[nlay] (1 - sfc_emis) + sfc_emis sfc_src (pass 1's dn); \
     pass 2 (up)   up[i]   = tr up[i+1] + sup + Cn (An dn[i]   - tr sdn - sup)   (pass 1's dn); \
     pass 3 (down) dn[i+1] = tr dn[i]   + sdn + Cn (An up[i+1] - tr sup - sdn)   (pass 2's up; dn[0] as in pass 1); \
     Jacobian J[nlay] = sfc_emis sfc_src_jac, J[i] = tr J[i+1]. \
   Everything else (D = secants, top boundary from inc_flux, scaling by pi weights, the sum over the angles) is \
   rrx_lw_solver_noscat's; with ssa = 0 the solve is that one. Arguments as rrx_lw_solver_noscat takes them, plus ssa, g (ncol, nlay, \
   ngpt). nmus 1..4. One thread per (column, g-point), any nlay. With several angles or do_broadband one angle's radiances (and with \
   do_broadband the per-g-point fluxes; flux_up / flux_dn are not used then) live in the stream's workspace. do_jacobians with \
   sfc_src_jac and flux_up_jac (ncol, nlay+1, ngpt) given: the per-g-point Jacobian, also with do_broadband. Argument checks and \
   empty problems as rrx_lw_solver_2stream. */ \
int rrx_lw_solver_noscat_rescaled##SFX( \
        int ncol, int nlay, int ngpt, RrxBool top_at_1, int nmus, const F* secants, const F* weights, \
        const F* tau, const F* ssa, const F* g, const F* lay_source, const F* lev_source, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up, F* flux_dn, \
        RrxBool do_broadband, F* flux_up_loc, F* flux_dn_loc, RrxBool do_jacobians, const F* sfc_src_jac, F* flux_up_jac, void* stream); \
/* The same solve for one angle from Planck-lite inputs with band cloud properties, broadband outputs, in one kernel: the inputs of \
   rrx_lw_solver_noscat_fractions (tau = the clear gas optical depth) plus the band cloud triple of rrx_lw_solver_2stream_fractions, \
   combined per g-point with the arithmetic and eps stated there (all NULL: ssa = 0, the bits of all-zero arrays; a partly-NULL \
   triple is refused). flux_up / flux_dn (ncol, nlay+1): g-point sums in rrx_sum_broadband's order. One-kernel tilings up to 575 \
   layers; taller columns and LW variants 1 and 7 materialise [tau | ssa | g | lay_source | lev_source] in the stream's workspace \
   (rrx_inc_2stream_by_2stream_bybnd, rrx_planck_sources_from_fractions) and take rrx_lw_solver_noscat_rescaled. */ \
int rrx_lw_solver_noscat_fractions_rescaled##SFX( \
        int ncol, int nlay, int ngpt, int nbnd, RrxBool top_at_1, const F* secants, const F* weights, \
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, const int* band_lims_gpt, \
        const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up, F* flux_dn, void* stream); \
/* ---- Optical_props_kernels_cuda : include_kernels_cuda/optical_props_kernels_cuda.h:33-56 ---- */ \
/* Empty problems, for the entries from here to rrx_fill that say so: an extent of 0 returns 0 and writes nothing (no launch is \
   made, so no launch error is left behind); a negative extent returns non-zero. The _bybnd increments: the g-points of no band \
   (outside every [lo, hi], or of a band with hi < lo) are left as they are; ncol, nlay, ngpt or nbnd = 0: returns 0. \
   The full g-point increments, rrx_delta_scale_2str_k, rrx_net_broadband_precalc, rrx_get_col_dry, rrx_spread_col, \
   rrx_scaling_to_subset, rrx_aerosol_optics and the three rrx_cloud_optics_* follow the same rule for every extent they take \
   (ncol, nlay, nlev, ngpt, nbnd): 0 returns 0 without a launch, a negative one returns 1 with "<entry>: negative extent" in \
   rrx_last_error(), decided on the host before any launch. rrx_sum_broadband alike for ncol and nlev; its ngpt = 0 with a \
   non-empty (ncol, nlev) is no empty problem: flux is written, as zeros (ngpt < 0 is refused). rrx_toa_source refuses \
   ncol <= 0 or ngpt <= 0 ("empty problem"). The floors of the quotients: 3*tiny of F in the increments and in delta scaling. */ \
int rrx_increment_1scalar_by_1scalar##SFX(int ncol, int nlay, int ngpt, F* tau_inout, const F* tau_in, void* stream); \
int rrx_increment_2stream_by_2stream##SFX(int ncol, int nlay, int ngpt, F* tau_inout, F* ssa_inout, F* g_inout, const F* tau_in, const F* ssa_in, const F* g_in, void* stream); \
int rrx_inc_1scalar_by_1scalar_bybnd##SFX(int ncol, int nlay, int ngpt, F* tau_inout, const F* tau_in, int nbnd, const int* band_lims_gpoint, void* stream); \
int rrx_inc_2stream_by_2stream_bybnd##SFX(int ncol, int nlay, int ngpt, F* tau_inout, F* ssa_inout, F* g_inout, const F* tau_in, const F* ssa_in, const F* g_in, int nbnd, const int* band_lims_gpoint, void* stream); \
int rrx_delta_scale_2str_k##SFX(int ncol, int nlay, int ngpt, F* tau_inout, F* ssa_inout, F* g_inout, void* stream); \
/* ---- Fluxes_kernels_cuda : include_kernels_cuda/fluxes_kernels_cuda.h:33-51 ---- */ \
int rrx_sum_broadband##SFX(int ncol, int nlev, int ngpt, const F* gpt_flux, F* flux, void* stream); \
int rrx_net_broadband_precalc##SFX(int ncol, int nlev, const F* flux_dn, const F* flux_up, F* flux_net, void* stream); \
/* host-model coupling (no counterpart in the reference library): layer heating rate [K/s] from the net (down - up) \
   broadband flux flux_net(ncol,nlay+1) and the level pressures plev(ncol,nlay+1): -(g/cp) * dF_net/dp, either vertical ordering. \
   ncol or nlay = 0: returns 0, writes nothing. */ \
int rrx_heating_rate##SFX(int ncol, int nlay, F g_over_cp, const F* flux_net, const F* plev, F* heating_rate, void* stream); \
/* by-band: Fortran semantics (src_kernels/mo_fluxes_byband_kernels.F90:22-71; the CUDA text is buggy): \
   band_lims is (2,nbnd), 1-based inclusive, gpt_flux is the SPECTRAL (ncol,nlev,ngpt) array. The g-points of a band are added in \
   order, starting from the band's first g-point. A band with hi < lo is empty: exact zeros are written and nothing is read (its lo \
   may be ngpt+1), in the sum and in the net form alike. ncol, nlev or nbnd = 0: returns 0, writes nothing. */ \
int rrx_sum_byband##SFX(int ncol, int nlev, int ngpt, int nbnd, const int* band_lims, const F* gpt_flux, F* bnd_flux, void* stream); \
int rrx_net_byband_full##SFX(int ncol, int nlev, int ngpt, int nbnd, const int* band_lims, const F* gpt_flux_dn, const F* gpt_flux_up, F* bnd_flux_net, void* stream); \
/* ---- Subset_kernels_cuda : include_kernels_cuda/subset_kernels_cuda.h:33-56 (n = 1..4 arrays at once) ---- \
   var_full(ncol,nlay,nbnd): columns col_s_in .. col_s_in+ncol_in-1 (1-based) take var_sub(ncol_in,nlay,nbnd), the other columns are \
   not written. A range outside 1..ncol or narr outside 1..4: non-zero. ncol_in, nlay or nbnd = 0: returns 0, writes nothing. */ \
int rrx_get_from_subset##SFX(int ncol, int nlay, int nbnd, int ncol_in, int col_s_in, int narr, \
        F* const* var_full, const F* const* var_sub, void* stream); \
/* ---- small kernels the reference keeps inside its host classes ---- */ \
/* src_cuda/Gas_optics_rrtmgp.cu:392-422 fill_gases_kernel (one gas per call, igas = 0 copies col_dry). ncol or nlay = 0: returns 0, \
   writes nothing (rrx_fill_gases_all alike). */ \
int rrx_fill_gases##SFX(int ncol, int nlay, int dim1, int dim2, int ngas, int igas, F* vmr_out, const F* vmr_in, F* col_gas, const F* col_dry, void* stream); \
/* the same for all gases in one launch: vmr_in = HOST array of ngas device pointers, each (dim1[i], dim2[i]) = (1,1) scalar, \
   (1,nlay) profile or (ncol,nlay) field; col_gas(ncol,nlay,0:ngas) with slot 0 = col_dry (the per-gas vmr copy is not produced). \
   ngas = 0 writes slot 0 only; ngas outside 0..32: non-zero */ \
int rrx_fill_gases_all##SFX(int ncol, int nlay, int ngas, const F* const* vmr_in, const int* dim1, const int* dim2, F* col_gas, const F* col_dry, void* stream); \
/* src_cuda/Gas_optics_rrtmgp.cu:806-903 get_col_dry (three kernels fused) */ \
int rrx_get_col_dry##SFX(int ncol, int nlay, const F* vmr_h2o, const F* plev, F* col_dry, void* stream); \
/* src_cuda/Rte_lw.cu:37-56, Rte_sw.cu:34-54 expand_and_transpose: (nbnd,ncol) -> (ncol,ngpt); the g-points of no band are not \
   written. ncol or nbnd = 0: returns 0, writes nothing. */ \
int rrx_expand_and_transpose##SFX(int ncol, int nbnd, const int* band_lims_gpt, const F* arr_in, F* arr_out, void* stream); \
/* src_cuda/Gas_optics_rrtmgp.cu spread_col: toa_src(icol,igpt) = solar_source(igpt) */ \
int rrx_spread_col##SFX(int ncol, int ngpt, F* toa_src, const F* solar_source, void* stream); \
/* src_test/Radiation_solver.cu scaling_to_subset: toa_src(icol,igpt) *= tsi_scaling(icol) */ \
int rrx_scaling_to_subset##SFX(int ncol, int ngpt, F* toa_src, const F* tsi_scaling, void* stream); \
/* the two above in one pass: toa_src(icol,igpt) = solar_source(igpt) * tsi_scaling(icol) (tsi_scaling = NULL: no scaling) */ \
int rrx_toa_source##SFX(int ncol, int ngpt, F* toa_src, const F* solar_source, const F* tsi_scaling, void* stream); \
/* src_cuda/Aerosol_optics.cu:36-263 + Aerosol_optics_gpu::aerosol_optics (:305-345): CAMS aerosol optics per band in one kernel. \
   aermr: HOST array of 11 device pointers (aermr01..aermr11), each (ncol,nlay) or, where aermr_per_column[a] == 0, one (nlay) \
   profile shared by all columns (the reference materialises the broadcast, fill_aerosols_3d); aermr_per_column may be NULL \
   (all per column). rh, tau, ssa, g: (ncol,nlay[,nbnd]); plev (ncol,nlay+1); rh_upper (nhum); hydrophobic tables \
   (nbnd,nphobic), hydrophilic tables (nbnd,nhum,nphilic), band index fastest (Radiation_solver.cu:366-401). The humidity class of a \
   cell is the first one whose upper bound is >= rh; above every bound the last class is used (the reference reads past the table). \
   ssa and g are floored with the machine epsilon of F: a cell with all mixing ratios 0 gives tau = ssa = g = 0. ncol, nlay or \
   nbnd = 0: returns 0, writes nothing; a negative extent, nhum < 1, nphobic < 11, nphilic < 5 or a NULL mixing ratio: non-zero. */ \
int rrx_aerosol_optics##SFX(int ncol, int nlay, int nbnd, int nhum, int nphobic, int nphilic, const F* const* aermr, const int* aermr_per_column, \
        const F* rh, const F* plev, const F* rh_upper, const F* mext_phobic, const F* ssa_phobic, const F* g_phobic, \
        const F* mext_philic, const F* ssa_philic, const F* g_philic, F* tau, F* ssa, F* g, void* stream); \
/* src_cuda/Cloud_optics.cu:31-127,181-329: LUT cloud optics per band; luts are (nsize,nbnd), their nodes equidistant from *_lwr to \
   *_upr. With step = (upr - lwr)/(nsize - 1) and x = (size - lwr)/step, a phase with water path > 0 is interpolated between the \
   nodes index-1 and index (1-based), index = max(1, min(int(x)+1, nsize-1)): a size outside the table is extrapolated linearly \
   from the first / last interval and nothing outside the table is read (the reference clamps from above only and reads in front \
   of the table for x <= -1). NaN or infinite sizes in cloudy cells are outside the contract. A phase with water path <= 0 \
   contributes exact zeros whatever its size holds; a cell without either phase gives tau = ssa = g = 0 in all three forms. ssa and \
   g are floored with the machine epsilon of F, the delta step of the _delta form with 3*tiny as rrx_delta_scale_2str_k. \
   ncol, nlay or nbnd = 0: returns 0, writes nothing. A negative extent, or nsize_liq < 2 or nsize_ice < 2 (no interval; the step \
   would divide by zero): non-zero, before any launch. */ \
int rrx_cloud_optics_2str##SFX(int ncol, int nlay, int nbnd, int nsize_liq, int nsize_ice, \
        F radliq_lwr, F radliq_upr, F diamice_lwr, F diamice_upr, \
        const F* lut_extliq, const F* lut_ssaliq, const F* lut_asyliq, \
        const F* lut_extice, const F* lut_ssaice, const F* lut_asyice, \
        const F* clwp, const F* ciwp, const F* reliq, const F* deice, F* tau, F* ssa, F* g, void* stream); \
/* rrx_cloud_optics_2str followed by rrx_delta_scale_2str_k (the reference driver's pair, Radiation_solver.cu:773-792) in one pass */ \
int rrx_cloud_optics_2str_delta##SFX(int ncol, int nlay, int nbnd, int nsize_liq, int nsize_ice, \
        F radliq_lwr, F radliq_upr, F diamice_lwr, F diamice_upr, \
        const F* lut_extliq, const F* lut_ssaliq, const F* lut_asyliq, \
        const F* lut_extice, const F* lut_ssaice, const F* lut_asyice, \
        const F* clwp, const F* ciwp, const F* reliq, const F* deice, F* tau, F* ssa, F* g, void* stream); \
int rrx_cloud_optics_1scl##SFX(int ncol, int nlay, int nbnd, int nsize_liq, int nsize_ice, \
        F radliq_lwr, F radliq_upr, F diamice_lwr, F diamice_upr, \
        const F* lut_extliq, const F* lut_ssaliq, const F* lut_asyliq, \
        const F* lut_extice, const F* lut_ssaice, const F* lut_asyice, \
        const F* clwp, const F* ciwp, const F* reliq, const F* deice, F* tau, void* stream); \
/* include/Array.h:311-350,579-622: column-range gather (subset) of an array whose FIRST dimension is the column: \
   out(icol, r) = in(col_s-1+icol, r), r < nrest. A range outside 1..ncol_full: non-zero, "column range outside the full array". \
   ncol_sub or nrest = 0 (range inside): returns 0, writes nothing. */ \
int rrx_subset_cols##SFX(int ncol_full, int nrest, int col_s, int ncol_sub, const F* in, F* out, void* stream); \
/* same for arrays in(n1, ncol_full) whose LAST dimension is the column, e.g. emis_sfc(nbnd,ncol): out(b, icol) = in(b, col_s-1+icol); \
   the same range check against ncol_full, the same empty rule (n1 or ncol_sub = 0) */ \
int rrx_subset_lastdim##SFX(int n1, int ncol_full, int col_s, int ncol_sub, const F* in, F* out, void* stream); \
/* arr[0 .. n) = value; n = 0: returns 0, writes nothing */ \
int rrx_fill##SFX(unsigned long long n, F value, F* arr, void* stream); \
/* ---- column ordering of the product chain (csrc/rrx_columns.hip; no counterpart in the reference library): columns are independent, so \
   a solve may process them in any order. perm (ncol + npad ints on the device) is a gather index: rrx_sort_columns = ascending order of \
   key(ncol) (the surface pressure: neighbouring columns then share LUT boxes in the windowed gas optics), its last npad entries repeat \
   the last column (padding to a multiple of 16 columns); rrx_column_spread sets flag = 1 where a run of `block` consecutive columns \
   spans more than threshold x its mean. gather: out(i, r) = in(perm[i], r), i < nout, column FIRST (fastest) dimension; gather_lastdim: \
   out(b, i) = in(b, perm[i]) for (n1, ncol) arrays; scatter: out(perm[i], r) = in(i, r), i < n (arrays of ncol_src / ncol_dst columns). \
   The sort is stable (equal keys keep their order); key is not modified. rrx_column_spread looks at FULL runs only (a trailing run \
   of fewer than `block` columns is ignored, so ncol < block gives 0), takes the mean in the key's precision, and rewrites flag on \
   every call (0 or 1). Empty problems: rrx_sort_columns and rrx_column_spread return non-zero ("empty problem") for ncol <= 0, \
   npad < 0 or block <= 0; the gathers and the scatter return 0 and write nothing for nout, n, nrest or n1 = 0. */ \
int rrx_sort_columns##SFX(int ncol, const F* key, int npad, int* perm, void* stream); \
int rrx_column_spread##SFX(int ncol, const F* key, int block, F threshold, int* flag, void* stream); \
int rrx_gather_cols##SFX(int nout, unsigned long long nrest, const int* perm, int ncol_in, const F* in, F* out, void* stream); \
int rrx_scatter_cols##SFX(int n, unsigned long long nrest, const int* perm, int ncol_src, const F* in, int ncol_dst, F* out, void* stream); \
int rrx_gather_lastdim##SFX(int n1, int nout, const int* perm, const F* in, F* out, void* stream); \
/* sunlit-only shortwave: perm[0 .. *count) = the entries of order(ncol) (NULL: 0 .. ncol-1) with mu0 > 0, in their order (0, -0.0, \
   negative values and NaN are night); then repeats of the last kept entry up to a multiple of pad_to (none when nothing is kept). \
   perm holds at least ncol rounded up to pad_to ints; *count (device) gets the unpadded count. One workgroup, no scratch memory. \
   scatter_cols_fill: out(:, r) = 0 for all ncol_dst columns, then out(perm[i], r) = in(i, r) for i < n (n = 0: zeros only); \
   serves every column-first layout: (col, n2), (col, nlev, nbnd), packed (k, nlev, col) with nrest = the product of the rest. */ \
int rrx_sunlit_columns##SFX(int ncol, const F* mu0, const int* order, int pad_to, int* perm, int* count, void* stream); \
int rrx_scatter_cols_fill##SFX(int n, unsigned long long nrest, const int* perm, int ncol_src, const F* in, int ncol_dst, F* out, void* stream); \
/* ---- McICA cloud sampling (csrc/rrx_mcica.hip; no counterpart in the reference library): every g-point of a \
   column sees one sub-column, cloudy or clear per layer, drawn from cloud_frac(ncol,nlay) under an overlap rule, and the band cloud \
   properties cld_*(ncol,nlay,nbnd) are combined into the g-point arrays (ncol,nlay,ngpt) IN PLACE in the cloudy cells only, with the \
   arithmetic of rrx_increment_1scalar_by_1scalar / rrx_increment_2stream_by_2stream. Clear cells are not written; the layers with \
   cloud_frac <= 0 are not read either. Run the clear gas optics (with the g array written in SW), then this. \
   Random numbers: Philox4x32-10, key = (low, high) 32 bits of seed, counter = (column identity, igpt, ilay/4, 2*domain + which), \
   the cell's word is output word ilay%4; which = 0 is the rank draw u, 1 the overlap draw v; all indices are 0-based array indices \
   (ilay the array's layer index whatever the vertical ordering); domain is the caller's (the drivers: 0 = LW, 1 = SW). The column \
   identity is col_id[icol] (ncol ints on the device), or col_id0 + icol with col_id = NULL: pass the columns' global indices and \
   a column draws the same sub-columns in any launch, order or split. uniform = ((x >> 9) + 0.5) * 2^-23, the same value in both \
   precisions. Walk ilay = 0 .. nlay-1 in array order with a rank: rank = u at ilay = 0 and below a layer with cloud_frac <= 0; \
   else the rank from above is kept when v < alpha(icol, ilay-1) and redrawn (rank = u) otherwise. alpha(ncol,nlay-1) in [0, 1] is the \
   overlap parameter between array layers l and l+1 (exponential-random overlap, Raisanen et al. 2004, two-draw form); alpha = NULL \
   means 1 everywhere: maximum-random overlap. The cell is cloudy iff cloud_frac > 0 and rank > 1 - cloud_frac. \
   mask_out (unsigned char (ncol,nlay,ngpt)) may be NULL; given, it is written in full (0 or 1, clear layers included). The g-points \
   of no band (outside every [lo, hi], or of a band with hi < lo) are sampled but left as they are. ncol, nlay, ngpt or (the \
   increments) nbnd = 0: returns 0 without a launch; a negative extent or a NULL that is needed: non-zero, before any HIP call. */ \
int rrx_mcica_increment_1scalar##SFX(int ncol, int nlay, int ngpt, int nbnd, const int* band_lims_gpt, const F* cloud_frac, const F* alpha, \
        unsigned long long seed, int domain, const int* col_id, int col_id0, F* tau_inout, const F* cld_tau, unsigned char* mask_out, void* stream); \
int rrx_mcica_increment_2stream##SFX(int ncol, int nlay, int ngpt, int nbnd, const int* band_lims_gpt, const F* cloud_frac, const F* alpha, \
        unsigned long long seed, int domain, const int* col_id, int col_id0, F* tau_inout, F* ssa_inout, F* g_inout, \
        const F* cld_tau, const F* cld_ssa, const F* cld_g, unsigned char* mask_out, void* stream); \
int rrx_mcica_cloud_mask##SFX(int ncol, int nlay, int ngpt, const F* cloud_frac, const F* alpha, unsigned long long seed, int domain, \
        const int* col_id, int col_id0, unsigned char* mask_out, void* stream); \
/* ---- Forward Monte Carlo ray tracer for 3-D shortwave fluxes (csrc/rrx_raytracer.hip; the algorithm of the \
   reference's ray_tracer_kernel on this project's arrays). The domain is nx x ny x nz cells of dx x dy x dz metres, periodic in \
   x and y; column icol = ix + nx iy. tau, ssa (ncol, nz, ngpt): the clear g-point arrays of the SW gas optics (Rayleigh \
   scattering); cld_tau, cld_ssa, cld_g (ncol, nz, nbnd): the band cloud triple (Henyey-Greenstein, g = min(cld_g, 1 - eps)), all \
   NULL or all given, with band_lims_gpt (2, nbnd), 1-based, on the device (a g-point of no band sees no cloud). Per g-point \
   k_ext = (tau + cld_tau)/dz, k_sca = (tau ssa + cld_tau cld_ssa)/dz. sfc_albedo (ncol): Lambertian. The sun: one mu0 in (0, 1] for \
   the domain, the direct beam travels along (sin cos(azimuth), sin sin(azimuth), -mu0), azimuth in radians from +x. \
   independent_column freezes the horizontal motion. igpt is 0-based. All arrays are on the device but inc_dir / inc_dif of \
   rrx_raytracer_sw, which are ngpt numbers on the HOST (the entry skips the g-points without incident flux). \
   rrx_rt_k_null: k_null (knx, kny, knz), x fastest, kn counted UPWARD from the surface, = the maximum of k_ext over the block's \
   cells for g-point igpt; knx, kny, knz divide nx, ny, nz. \
   rrx_rt_trace_counts: traces the photons [photon0, photon0 + nphotons) of g-point igpt (photon p starts in pixel p mod ncol; \
   Philox4x32-10 keyed by seed with counter (p low, p high, igpt, block); draw order: the header of rrx_raytracer.hip) and ADDS \
   into six caller-zeroed arrays of unsigned 64-bit counts in units of 2^-32 photon: sfc_dn_dir, sfc_dn_dif, sfc_up, tod_up (ncol) \
   and abs_dir, abs_dif (ncol, nz) (dir / dif: the photon had not / had been scattered or reflected or started diffuse). Integer \
   adds: the result is independent of the order of arrival and additive over photon ranges. A photon still alive after max_events \
   events is dropped and counted in n_capped (one device counter, added into). inc_dir, inc_dif >= 0 set the diffuse share \
   inc_dif/(inc_dir + inc_dif) of the starts. \
   rrx_rt_counts_to_flux: out[i] += F(counts[i] 2^-32) scale, i < n. \
   rrx_raytracer_sw: the spectral loop. Zeroes the six outputs and n_capped, then for igpt = 0 .. ngpt-1 with \
   inc_dir[igpt] + inc_dif[igpt] > 0: zeroes counts in the stream's workspace, rrx_rt_k_null, rrx_rt_trace_counts of \
   photons_per_pixel ncol photons from 0, rrx_rt_counts_to_flux with scale = (inc_dir + inc_dif)/F(photons_per_pixel) for the \
   four surface / top arrays (W m-2) and scale/dz for the absorption (W m-3): the same bits as that loop made by hand. \
   An extent of 0 (nx, ny, nz, ngpt, nphotons, photons_per_pixel, n): returns 0 without a launch; a negative extent, a NULL that \
   is needed, a partly-NULL cloud triple, mu0 outside (0, 1], a non-positive dx / dy / dz, a kn grid that does not divide the grid: \
   non-zero, before any HIP call. */ \
int rrx_rt_k_null##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, const F* tau, const int* band_lims_gpt, \
        const F* cld_tau, F dz, int knx, int kny, int knz, F* k_null, void* stream); \
int rrx_rt_trace_counts##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, F inc_dir, F inc_dif, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long photon0, long long nphotons, int max_events, \
        unsigned long long* sfc_dn_dir, unsigned long long* sfc_dn_dif, unsigned long long* sfc_up, unsigned long long* tod_up, \
        unsigned long long* abs_dir, unsigned long long* abs_dif, unsigned long long* n_capped, void* stream); \
int rrx_rt_counts_to_flux##SFX(long long n, const unsigned long long* counts, F scale, F* out, void* stream); \
int rrx_raytracer_sw##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, const F* inc_dif, int knx, int kny, int knz, \
        long long photons_per_pixel, unsigned long long seed, int max_events, \
        F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, unsigned long long* n_capped, void* stream); \
/* ---- Backward Monte Carlo ray tracer: radiances for a virtual camera or a flux sensor (csrc/rrx_raytracer_bw.hip). \
   The scene arguments are those of the forward entries (no independent-column switch, no diffuse incident light), k_null is that \
   of rrx_rt_k_null. Rays start at the sensor, travel against the light and are scored by local estimates of the direct beam at \
   every surface hit and every scattering, with the EXACT transmission to the sun, walked cell by cell (the estimator, the draw \
   order and the bound of the walk: the header of rrx_raytracer_bw.hip). \
   The sensor: sensor_type 0 perspective, 1 fisheye, 2 orthographic, 3 flux sensor; npx x npy pixels (pixel = ipx + npx ipy); fov in \
   radians (fisheye only: the full opening angle, in (0, 2 pi]); sensor: 12 numbers on the HOST, position (m; z upward from the \
   surface), e_w, e_h, e_d. Perspective: direction normalize(e_w (2a-1) + e_h (2b-1) + e_d) from position, (a, b) in [0,1]^2 across \
   the image. Fisheye: theta = a fov/2, phi = 2 pi b about e_d. Orthographic: direction e_d (unit, e_d.z < 0) from (a Lx, b Ly, top). \
   Flux sensor: cosine-weighted, at the surface facing up (e_d.z > 0) or at the top facing down (e_d.z < 0); pi x the mean radiance \
   is an irradiance. A position with z < 0 is refused; one above the top is moved along the ray to the top. \
   rrx_rt_bw_trace_counts: traces the rays [ray0, ray0 + nrays) of g-point igpt (ray r belongs to pixel r mod (npx npy); \
   Philox4x32-10 keyed by seed with counter (r low, r high, igpt | 0x80000000, block)) and ADDS into the caller-zeroed counts (npx npy), \
   unsigned 64-bit in units of 2^-32: llrint(min(d, 2^20) 2^32) per deposit d; a clamped deposit is counted in n_clamped, a ray \
   dropped after max_events events in n_capped (one device counter each, added into). Integer adds: independent of the order of \
   arrival, additive over ray ranges. Radiance = counts 2^-32 / rays_per_pixel inc_dir/mu0, W m-2 sr-1. \
   rrx_raytracer_bw: the spectral loop. Zeroes radiance (npx npy), n_capped and n_clamped, then for igpt = 0 .. ngpt-1 with \
   inc_dir[igpt] > 0 (ngpt numbers on the HOST): zeroes counts in the stream's workspace, rrx_rt_k_null, rrx_rt_bw_trace_counts of \
   rays_per_pixel npx npy rays from 0, rrx_rt_counts_to_flux with scale = inc_dir/(mu0 F(rays_per_pixel)): the same bits as that loop \
   made by hand. An extent of 0 (nx, ny, nz, ngpt, npx, npy, nrays, rays_per_pixel): returns 0 without a launch; a negative extent, \
   a NULL that is needed, a scene the forward entries refuse, a sensor_type outside 0..3, a sensor that is not finite, lies below \
   the surface, has e_d = 0, is orthographic without a unit downward e_d or a flux sensor with e_d.z = 0, a fisheye fov outside \
   (0, 2 pi]: non-zero, before any HIP call. */ \
int rrx_rt_bw_trace_counts##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, int knx, int kny, int knz, const F* k_null, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, unsigned long long seed, long long ray0, long long nrays, int max_events, \
        unsigned long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream); \
int rrx_raytracer_bw##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, int knx, int kny, int knz, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, long long rays_per_pixel, unsigned long long seed, int max_events, \
        F* radiance, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream); \
/* ---- Tabulated cloud phase functions for both ray tracers (csrc/rrx_rt_phase.h, rrx_rt_phase.hip). ONE table is \
   sampled for the scattering angle and evaluated towards the sun. mu (nmu): the cosines of the scattering angle, strictly \
   increasing from -1 to +1, shared by all tables; P is piecewise linear in mu between them. phase, cdf (nmu, nre, nbnd), nmu fastest: \
   1/2 int P dmu = 1 and C_i = 1/2 int_{-1}^{mu_i} P dmu (C_0 = 0, C_last = 1), one table per effective radius re0 + dre ire and band. \
   A cell of radius re (cld_re (ncol, nz), the layout of one band of the cloud triple, the unit of re0 and dre) uses \
   X_lo + f (X_hi - X_lo) of the tables ire = clamp(int((re - re0)/dre), 0, nre-2) and ire + 1, f = clamp((re - re0)/dre - ire, 0, 1) \
   (a NaN radius: ire = 0, f = 0; nre = 1: no blend). Sampling inverts the piecewise-quadratic blended CDF exactly with + - x / sqrt \
   from the one uniform that gives the cosine today; no further random number is drawn. Rayleigh scattering on gas is unchanged; \
   cld_g is not read but the triple stays all or none. \
   rrx_rt_phase_tables: phase_raw (nmu, nre, nbnd) >= 0 of any normalisation -> phase and cdf; the trapezoid sums are accumulated in \
   double in node order in both precisions. It waits for its launch: nodes that do not increase strictly from -1 to +1, a table \
   whose integral is not > 0 or not finite or that holds a negative number: non-zero. nbnd = 0: returns 0 without a launch. \
   rrx_rt_phase_sample: cos_out[i] = the cosine that the tracers draw from the uniform u[i] in a cell of radius re[i], band ibnd \
   (0-based), i < n. rrx_rt_phase_eval: p_out[i] = P(clamp(cs[i], -1, 1)) at radius re[i], the density of that draw. n = 0: \
   returns 0 without a launch. \
   rrx_rt_trace_counts_phase, rrx_raytracer_sw_phase, rrx_rt_bw_trace_counts_phase, rrx_raytracer_bw_phase: the entries above with \
   nmu, nre, re0, dre, mu, phase, cdf, cld_re in front of the stream. With the four pointers NULL they are the entries above (nmu, \
   nre, re0, dre are not read); otherwise the cloud species scatters by the table. The spectral loops give the same bits as their \
   loops made by hand. Refused, before any HIP call: a partly-NULL table, a table without a cloud triple, nmu < 2, nmu > 4096 (the \
   backward tracer keeps the nodes in LDS), nre < 1, dre <= 0 with nre > 1, a negative extent, and what the entries above refuse. */ \
int rrx_rt_phase_tables##SFX(int nmu, int nre, int nbnd, const F* mu, const F* phase_raw, F* phase, F* cdf, void* stream); \
int rrx_rt_phase_sample##SFX(long long n, int nmu, int nre, int nbnd, int ibnd, F re0, F dre, const F* mu, const F* phase, const F* cdf, \
        const F* u, const F* re, F* cos_out, void* stream); \
int rrx_rt_phase_eval##SFX(long long n, int nmu, int nre, int nbnd, int ibnd, F re0, F dre, const F* mu, const F* phase, const F* cdf, \
        const F* cs, const F* re, F* p_out, void* stream); \
int rrx_rt_trace_counts_phase##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, F inc_dir, F inc_dif, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long photon0, long long nphotons, int max_events, \
        unsigned long long* sfc_dn_dir, unsigned long long* sfc_dn_dif, unsigned long long* sfc_up, unsigned long long* tod_up, \
        unsigned long long* abs_dir, unsigned long long* abs_dif, unsigned long long* n_capped, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, void* stream); \
int rrx_raytracer_sw_phase##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, const F* inc_dif, int knx, int kny, int knz, \
        long long photons_per_pixel, unsigned long long seed, int max_events, \
        F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, unsigned long long* n_capped, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, void* stream); \
int rrx_rt_bw_trace_counts_phase##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, int knx, int kny, int knz, const F* k_null, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, unsigned long long seed, long long ray0, long long nrays, int max_events, \
        unsigned long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, void* stream); \
int rrx_raytracer_bw_phase##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, int knx, int kny, int knz, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, long long rays_per_pixel, unsigned long long seed, int max_events, \
        F* radiance, unsigned long long* n_capped, unsigned long long* n_clamped, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, void* stream); \
/* ---- A background atmosphere between the domain top and TOA, for both ray tracers (csrc/rrx_rt_common.h). \
   nbg >= 1 plane-parallel, horizontally uniform layers above the grid, counted UPWARD from the domain top whatever top_at_1 is; \
   nbg <= 256. dz_bg (nbg): the thicknesses in metres, all > 0, on the HOST. Layer b lies between z_bg[b] and z_bg[b+1] with \
   z_bg[0] = F(knz) (F(nz/knz) dz), the domain top as the kernels form it, z_bg[b+1] = z_bg[b] + dz_bg[b], z_bg[nbg] = TOA. On the \
   device: the clear bg_tau, bg_ssa (nbg, ngpt), layer fastest, and the optional band triple bg_cld_tau, bg_cld_ssa, bg_cld_g \
   (nbg, nbnd), all NULL or all given (it needs band_lims_gpt and scatters by Henyey-Greenstein always: a phase table applies inside \
   the grid only). \
   rrx_rt_bg_profile: bg_profile (5, nbg+1), layer fastest, for g-point igpt: rows k_ext = (tau + tau_c)/dz_bg, \
   k_sca = (tau ssa + tau_c ssa_c)/dz_bg, k_sca_cld = (tau_c ssa_c)/dz_bg, g = min(g_c, 1 - eps), and tau_above[b] = the sum of \
   tau + tau_c over the layers b+1 .. nbg-1 in index order; slot nbg of tau_above holds the sum over all layers, slot nbg of the \
   other rows 0. nbg or ngpt = 0: returns 0 without a launch. \
   The _bg entries are the _phase entries (the table arguments may be NULL) with nbg, dz_bg and the background in front of the \
   stream, and the new outputs behind the existing ones. Transport in the background, the new tallies and the sensors: the headers \
   of rrx_rt_common.h, rrx_raytracer.hip and rrx_raytracer_bw.hip. In short: photons start at TOA; a background layer is a block \
   with z faces only whose k_null is its own k_ext; x and y run unwrapped there and are wrapped on entering the grid; a backward \
   ray ends only at TOA, a scattering in layer b deposits with T_sun = exp(-(k_ext_b (z_bg[b+1] - z) + tau_above[b])/mu0) and a \
   deposit from inside the grid multiplies its walked transmission by exp(-tau_above[nbg]/mu0), formed as one exp. \
   rrx_rt_trace_counts_bg: beside the six tallies (tod_up now counts EVERY upward crossing of the domain top), toa_up, tod_dn_dir, \
   tod_dn_dif (ncol) and bg_abs_dir, bg_abs_dif (nbg), caller-zeroed, added into, the same 2^-32 units; bg_profile from \
   rrx_rt_bg_profile for the same igpt. \
   rrx_raytracer_sw_bg: the spectral loop with rrx_rt_bg_profile in it; toa_up, tod_dn_dir, tod_dn_dif (ncol) in W m-2 with the \
   scale of the other fluxes; bg_abs_dir, bg_abs_dif (nbg) in W m-3 of a DOMAIN-WIDE layer: the counts of all columns times \
   (scale/dz_bg[b])/F(ncol). The same bits as the loop made by hand. \
   rrx_rt_bw_trace_counts_bg, rrx_raytracer_bw_bg: the top of the medium is TOA: a sensor at or above it is moved along the ray to it, \
   a sensor may sit inside the background, and the orthographic sensor and the flux sensor facing down start at the height \
   clamp(position.z, domain top, TOA) (position.z = 0: the domain top, as without a background; any position.z >= TOA: TOA). \
   nbg = 0: the medium without a background, the integers of the existing entries; dz_bg, the background arrays and the new \
   outputs are not read. Refused before any HIP call: nbg < 0 or > 256, a NULL that is needed, a partly-NULL background triple, a \
   dz_bg that is not > 0 and finite, and what the _phase entries refuse. */ \
int rrx_rt_bg_profile##SFX(int nbg, int ngpt, int nbnd, int igpt, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const int* band_lims_gpt, \
        const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, F* bg_profile, void* stream); \
int rrx_rt_trace_counts_bg##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, F inc_dir, F inc_dif, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long photon0, long long nphotons, int max_events, \
        unsigned long long* sfc_dn_dir, unsigned long long* sfc_dn_dif, unsigned long long* sfc_up, unsigned long long* tod_up, \
        unsigned long long* abs_dir, unsigned long long* abs_dif, unsigned long long* n_capped, \
        unsigned long long* toa_up, unsigned long long* tod_dn_dir, unsigned long long* tod_dn_dif, \
        unsigned long long* bg_abs_dir, unsigned long long* bg_abs_dif, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_profile, void* stream); \
int rrx_raytracer_sw_bg##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, const F* inc_dif, int knx, int kny, int knz, \
        long long photons_per_pixel, unsigned long long seed, int max_events, \
        F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, unsigned long long* n_capped, \
        F* toa_up, F* tod_dn_dir, F* tod_dn_dif, F* bg_abs_dir, F* bg_abs_dif, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, void* stream); \
int rrx_rt_bw_trace_counts_bg##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, int knx, int kny, int knz, const F* k_null, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, unsigned long long seed, long long ray0, long long nrays, int max_events, \
        unsigned long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_profile, void* stream); \
int rrx_raytracer_bw_bg##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, int knx, int kny, int knz, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, long long rays_per_pixel, unsigned long long seed, int max_events, \
        F* radiance, unsigned long long* n_capped, unsigned long long* n_clamped, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, void* stream); \
/* ---- Aerosol as a third scattering species of both ray tracers (csrc/rrx_rt_common.h). Opt-in: a band triple \
   aer_tau, aer_ssa, aer_g (ncol, nz, nbnd) in the grid, the layout of the cloud triple, and bg_aer_tau, bg_aer_ssa, bg_aer_g \
   (nbg, nbnd) in the background, the layout of the background's cloud triple. Each triple is all NULL or all given and needs \
   band_lims_gpt and nbnd >= 1; a g-point that lies in no band has no aerosol. Per cell, with the parentheses as written: \
   k_ext = ((tau + tau_c) + tau_a)/dz, k_sca = ((tau ssa + tau_c ssa_c) + tau_a ssa_a)/dz, k_sca_cld = (tau_c ssa_c)/dz, \
   k_sca_aer = (tau_a ssa_a)/dz (dz_bg[b] in a background layer); tau_a = 0 gives the bits of the medium without aerosol. The \
   species draw stays one uniform u: cloud iff u k_sca < k_sca_cld, otherwise aerosol iff u k_sca < k_sca_cld + k_sca_aer, \
   otherwise gas. Aerosol scatters by Henyey-Greenstein with min(g_a, 1 - eps), in the grid and in the background, with a phase \
   table too (the table stays the cloud's), and the backward deposit uses the same density. No new tallies: abs_* and bg_abs_* \
   include what aerosol absorbs. Each entry is its _bg (or plain) counterpart with the aerosol arguments in front of the stream. \
   rrx_rt_k_null_aer: the block maximum of the k_ext above. \
   rrx_rt_bg_profile_aer: bg_profile (7, nbg+1): the five rows of rrx_rt_bg_profile in its order by the formulas above (tau_above \
   sums (tau + tau_c) + tau_a in index order), then k_sca_aer and g_aer = min(g_a, 1 - eps); slot nbg of the two new rows is 0. \
   rrx_rt_trace_counts_aer, rrx_rt_bw_trace_counts_aer: the grid's triple; with nbg > 0 bg_profile is the 7-row profile. \
   rrx_raytracer_sw_aer, rrx_raytracer_bw_aer: the spectral loops with both triples; the same bits as the loops made by hand from \
   the entries above. rrx_raytracer_sw_aer alone takes each triple as ONE argument, a HOST array of its three device pointers in \
   the order tau, ssa, g: aer = {aer_tau, aer_ssa, aer_g}, bg_aer = {bg_aer_tau, bg_aer_ssa, bg_aer_g}; a NULL array is a triple of \
   NULLs. (With six pointers it would have 61 parameters; the longest entry of this header has 58, and the binding's signature \
   test pins that.) With nbg = 0 the background's aerosol arguments are not read. With every aerosol pointer NULL the loops are \
   the _bg entries and every entry gives the integers of its _bg (or plain) counterpart. Refused before any HIP call: a \
   partly-NULL aerosol triple, an aerosol triple without band_lims_gpt or with nbnd < 1, and what the counterpart refuses. */ \
int rrx_rt_k_null_aer##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, const F* tau, const int* band_lims_gpt, \
        const F* cld_tau, F dz, int knx, int kny, int knz, F* k_null, const F* aer_tau, void* stream); \
int rrx_rt_bg_profile_aer##SFX(int nbg, int ngpt, int nbnd, int igpt, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const int* band_lims_gpt, \
        const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, F* bg_profile, \
        const F* bg_aer_tau, const F* bg_aer_ssa, const F* bg_aer_g, void* stream); \
int rrx_rt_trace_counts_aer##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, F inc_dir, F inc_dif, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long photon0, long long nphotons, int max_events, \
        unsigned long long* sfc_dn_dir, unsigned long long* sfc_dn_dif, unsigned long long* sfc_up, unsigned long long* tod_up, \
        unsigned long long* abs_dir, unsigned long long* abs_dif, unsigned long long* n_capped, \
        unsigned long long* toa_up, unsigned long long* tod_dn_dir, unsigned long long* tod_dn_dif, \
        unsigned long long* bg_abs_dir, unsigned long long* bg_abs_dif, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_profile, const F* aer_tau, const F* aer_ssa, const F* aer_g, void* stream); \
int rrx_raytracer_sw_aer##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, const F* inc_dif, int knx, int kny, int knz, \
        long long photons_per_pixel, unsigned long long seed, int max_events, \
        F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, unsigned long long* n_capped, \
        F* toa_up, F* tod_dn_dir, F* tod_dn_dif, F* bg_abs_dir, F* bg_abs_dif, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, \
        const F* const* aer, const F* const* bg_aer, void* stream); \
int rrx_rt_bw_trace_counts_aer##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, int knx, int kny, int knz, const F* k_null, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, unsigned long long seed, long long ray0, long long nrays, int max_events, \
        unsigned long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_profile, const F* aer_tau, const F* aer_ssa, const F* aer_g, void* stream); \
int rrx_raytracer_bw_aer##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, int knx, int kny, int knz, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, long long rays_per_pixel, unsigned long long seed, int max_events, \
        F* radiance, unsigned long long* n_capped, unsigned long long* n_clamped, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, \
        const F* aer_tau, const F* aer_ssa, const F* aer_g, const F* bg_aer_tau, const F* bg_aer_ssa, const F* bg_aer_g, void* stream); \
/* ---- The forward tracer with all g-points in one launch and photons dealt per g-point (csrc/rrx_rt_common.h). \
   Forward only, ngpt <= 1024, built on the aerosol form (which covers nbg = 0 and NULL aerosol triples). The photons of a launch are \
   the concatenation, in g-point order, of n_g = m_g ncol photons per g-point, m_g >= 0 photons per pixel; photon_end (ngpt+1) holds \
   the prefix sums with photon_end[0] = 0. Global index p belongs to the g with photon_end[g] <= p < photon_end[g+1] (empty ranges are \
   stepped over); its local index is q = p - photon_end[g], its Philox stream that of photon q of g-point g and its pixel q mod ncol: \
   it is photon q of rrx_rt_trace_counts_aer(igpt = g), draw for draw. Only the deposits differ: every tally takes \
   llrint(w weight0[g] 2^32). weight0[g] = (inc_g / F(m_g)) / (S / F(P)) for m_g > 0, inc_g = inc_dir[g] + inc_dif[g], S the sum of \
   inc_g over the g-points with m_g > 0 in index order, P the sum of m_g; dif_frac[g] = inc_dif[g] / inc_g. The common unit is \
   U = S / F(P): flux = counts 2^-32 U, abs_* with U / dz and bg_abs_*[b] with (U / dz_bg[b]) / F(ncol). With weight0[g] = 1 the integers \
   are the sums over g of those of the per-g-point entry. \
   rrx_rt_k_null_all: k_null (ngpt, knz, kny, knx); slice g is bit for bit rrx_rt_k_null_aer(igpt = g). \
   rrx_rt_bg_profile_all: bg_profile (ngpt, 7, nbg+1); slice g is bit for bit rrx_rt_bg_profile_aer(igpt = g). \
   rrx_rt_trace_counts_spectral: rrx_rt_trace_counts_aer without igpt, inc_dir, inc_dif and with the DEVICE arrays photon_end (ngpt+1), \
   weight0, dif_frac (ngpt); k_null and bg_profile are those of all g-points; photon0 / nphotons address the concatenated list and the \
   counts are additive over its ranges. The entry cannot look into device arrays: a photon beyond photon_end[ngpt] is stepped over and \
   the kernel stays inside its arrays whatever photon_end holds; the callers that form the list on the host refuse one that does not \
   ascend. \
   rrx_raytracer_sw_spectral: rrx_raytracer_sw_aer with photons_per_pixel_gpt (ngpt, HOST) = m_g in place of photons_per_pixel. It forms \
   photon_end, weight0 and dif_frac as above, builds k_null and the profile, traces chunks of consecutive g-points (the largest chunk \
   whose k_null fits 1 GiB; RRX_RT_SPECTRAL_GPT_PER_LAUNCH in the environment overrides it, read at every call), adds the counts of \
   all chunks in integers and converts them once: the result does not depend on the chunking. It waits for its stream once, after \
   copying the photon list. Refused before any HIP call: what the _aer counterpart refuses, ngpt > 1024, m_g < 0, m_g > 0 where \
   inc_g <= 0. All m_g = 0: the outputs are zeroed and it returns 0. */ \
int rrx_rt_k_null_all##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, const F* tau, const int* band_lims_gpt, \
        const F* cld_tau, F dz, int knx, int kny, int knz, F* k_null, const F* aer_tau, void* stream); \
int rrx_rt_bg_profile_all##SFX(int nbg, int ngpt, int nbnd, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const int* band_lims_gpt, \
        const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, F* bg_profile, \
        const F* bg_aer_tau, const F* bg_aer_ssa, const F* bg_aer_g, void* stream); \
int rrx_rt_trace_counts_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const long long* photon_end, const F* weight0, const F* dif_frac, \
        int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long photon0, long long nphotons, int max_events, \
        unsigned long long* sfc_dn_dir, unsigned long long* sfc_dn_dif, unsigned long long* sfc_up, unsigned long long* tod_up, \
        unsigned long long* abs_dir, unsigned long long* abs_dif, unsigned long long* n_capped, \
        unsigned long long* toa_up, unsigned long long* tod_dn_dir, unsigned long long* tod_dn_dif, \
        unsigned long long* bg_abs_dir, unsigned long long* bg_abs_dif, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_profile, const F* aer_tau, const F* aer_ssa, const F* aer_g, void* stream); \
int rrx_raytracer_sw_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, RrxBool independent_column, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, const F* inc_dif, int knx, int kny, int knz, \
        const long long* photons_per_pixel_gpt, unsigned long long seed, int max_events, \
        F* sfc_dn_dir, F* sfc_dn_dif, F* sfc_up, F* tod_up, F* abs_dir, F* abs_dif, unsigned long long* n_capped, \
        F* toa_up, F* tod_dn_dir, F* tod_dn_dif, F* bg_abs_dir, F* bg_abs_dif, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, \
        const F* const* aer, const F* const* bg_aer, void* stream); \
/* ---- The backward tracer with the rays of all g-points in one launch, counts kept by band, and a channel matrix from bands to what a \
   sensor sees (csrc/rrx_raytracer_bw.hip). The backward counterpart of the entries above, ngpt <= 1024, built on the \
   aerosol form. The symbols begin rrx_camera_: the set of rrx_rt_ and rrx_raytracer_ symbols is closed. The rays of a launch are the \
   concatenation, in g-point order, of n_g = m_g npix rays per g-point, m_g >= 0 rays per pixel; ray_end (ngpt+1) holds the prefix sums \
   with ray_end[0] = 0. Global index p belongs to the g with ray_end[g] <= p < ray_end[g+1] (empty ranges are stepped over); its local \
   index is q = p - ray_end[g], its Philox stream that of ray q of g-point g and its pixel q mod npix: it is ray q of \
   rrx_rt_bw_trace_counts_aer(igpt = g), draw for draw. Only the deposits differ: a deposit d is tallied as \
   llrint(min(d weight0[g], 2^20) 2^32) into counts[band(g) npix + pix], counts (nbnd, npix); a clamped one is counted in n_clamped. \
   band_lims_gpt is always needed; a g-point that lies in no band has no row and its deposits are dropped. With weight0[g] = 1 the \
   counts of a band are the integer sums over its g-points of those of the per-g-point entry. \
   rrx_camera_trace_counts_spectral: rrx_rt_bw_trace_counts_aer without igpt and with the DEVICE arrays ray_end (ngpt+1) and weight0 \
   (ngpt); k_null is rrx_rt_k_null_all's and bg_profile rrx_rt_bg_profile_all's; ray0 / nrays are a range of the list; counts, n_capped, \
   n_clamped are caller-zeroed, added into, and additive over ranges of the list. The entry cannot look into device arrays: a ray \
   beyond ray_end[ngpt] is stepped over and the kernel stays inside its arrays whatever ray_end holds; the callers that form the list \
   on the host refuse one that does not ascend. \
   rrx_camera_channels: out[c, pix] = scale sum_b chan_weights[c, b] (counts[b, pix] 2^-32), the sum in band order in F; chan_weights \
   (nchan, nbnd) on the DEVICE, out (nchan, npix) is written, not added into. The identity gives radiance by band, a row of ones \
   broadband, three rows of colour-matching weights colour. npix = 0: returns 0 without a launch. \
   rrx_camera_render_spectral: rrx_raytracer_bw_aer with rays_per_pixel_gpt (ngpt, HOST) = m_g in place of rays_per_pixel, and nchan, \
   chan_weights (nchan, nbnd, HOST) and radiance (nchan, npix) in W m-2 sr-1. weight0[g] = (inc_dir[g] / F(m_g)) / U, U = S / F(P), S \
   the sum of inc_dir[g] over the g-points with m_g > 0 in index order, P the sum of m_g. It builds the profile, traces chunks of \
   consecutive g-points (the largest chunk whose k_null fits 1 GiB; RRX_RT_SPECTRAL_GPT_PER_LAUNCH in the environment overrides it, read \
   at every call), adds the counts of all chunks in integers and converts them once with scale = U / mu0: the result does not depend on \
   the chunking. It waits for its stream once, after copying the ray list. All m_g = 0: the outputs are zeroed and it returns 0. \
   Refused before any HIP call: what the _aer counterparts refuse, ngpt > 1024, nbnd < 1, a NULL band_lims_gpt, m_g < 0, m_g > 0 where \
   inc_dir[g] <= 0, nchan < 1, a NULL chan_weights. */ \
int rrx_camera_trace_counts_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const long long* ray_end, const F* weight0, \
        int knx, int kny, int knz, const F* k_null, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, unsigned long long seed, long long ray0, long long nrays, int max_events, \
        unsigned long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_profile, const F* aer_tau, const F* aer_ssa, const F* aer_g, void* stream); \
int rrx_camera_channels##SFX(long long npix, int nbnd, int nchan, const unsigned long long* counts, const F* chan_weights, F scale, F* out, \
        void* stream); \
int rrx_camera_render_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_albedo, F mu0, F azimuth, const F* inc_dir, int knx, int kny, int knz, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, const long long* rays_per_pixel_gpt, unsigned long long seed, int max_events, \
        int nchan, const F* chan_weights, F* radiance, unsigned long long* n_capped, unsigned long long* n_clamped, \
        int nmu, int nre, F re0, F dre, const F* mu, const F* phase, const F* cdf, const F* cld_re, \
        int nbg, const F* dz_bg, const F* bg_tau, const F* bg_ssa, const F* bg_cld_tau, const F* bg_cld_ssa, const F* bg_cld_g, \
        const F* aer_tau, const F* aer_ssa, const F* aer_g, const F* bg_aer_tau, const F* bg_aer_ssa, const F* bg_aer_g, void* stream); \
/* ---- Thermal emission in the backward tracer: longwave radiances for a virtual camera, 3-D longwave fluxes for a flux sensor \
   (csrc/rrx_raytracer_thermal.hip). The symbols begin rrx_thermal_: the set of rrx_rt_ and rrx_raytracer_ symbols is \
   closed. Rays start at the sensor as in rrx_rt_bw_trace_counts (the same four sensors, the same start) and travel through the grid \
   with that entry's tracking, draw for draw; there is no sun and no walk. The medium per g-point: k_ext = (tau + cld_tau)/dz, \
   k_sca = (tau ssa + cld_tau cld_ssa)/dz; ssa may be NULL: the gas does not scatter (what the LW gas optics give); k_null is \
   rrx_rt_k_null's. The sources are RADIANCES in W m-2 sr-1, the arrays the 1-D LW solver takes (its flux is pi w radiance): \
   lay_src (ncol, nz, ngpt), the layout of tau, constant within a cell; sfc_src (ncol, ngpt); sfc_emis (ncol), one broadband \
   Lambertian emissivity per pixel (the surface reflects 1 - sfc_emis); top_radiance, one isotropic downward radiance per g-point \
   at the domain top (it closes the medium when the grid does not reach TOA). A ray deposits, each before the weight changes: \
   at a collision weight (1 - f_no_abs) lay_src[cell, g], then weight *= f_no_abs; at the surface weight sfc_emis sfc_src[col, g], \
   then weight *= 1 - sfc_emis; where it ends at the top (it leaves through it, or starts at or above it looking away from the \
   medium) weight top_radiance. Nothing is deposited at a scattering. \
   rrx_thermal_trace_counts: traces the rays [ray0, ray0 + nrays) of g-point igpt (ray r belongs to pixel r mod (npx npy); \
   Philox4x32-10 keyed by seed with counter (r low, r high, igpt | 0xC0000000, block)) and ADDS into the caller-zeroed counts \
   (npx npy), unsigned 64-bit in units of 2^-32: llrint(min(d, 2^20) 2^32) per deposit d; n_clamped and n_capped as in \
   rrx_rt_bw_trace_counts. Integer adds: independent of the order of arrival, additive over ray ranges. Radiance of the g-point = \
   counts 2^-32 / rays_per_pixel. \
   rrx_thermal_render: the loop over all g-points. top_radiance: ngpt numbers on the HOST, NULL = 0. Zeroes radiance, n_capped and \
   n_clamped, then for igpt = 0 .. ngpt-1: zeroes counts in the stream's workspace, rrx_rt_k_null, rrx_thermal_trace_counts of \
   rays_per_pixel npx npy rays from 0, rrx_rt_counts_to_flux with scale = 1/F(rays_per_pixel) into radiance (npx npy) (by_band = 0: \
   the sum over g-points) or into the g-point's band's slice of radiance (npx npy, nbnd) (by_band = 1: band_lims_gpt is needed; a \
   g-point of no band is dropped): the same bits as that loop made by hand. With a flux sensor pi x radiance is an irradiance. \
   An extent of 0 (nx, ny, nz, ngpt, npx, npy, nrays, rays_per_pixel): returns 0 without a launch. Refused, non-zero, before any HIP \
   call: what the backward entries refuse of grid, cloud triple and sensor; a NULL tau, lay_src, sfc_src, sfc_emis, k_null, sensor, \
   counts, radiance or counter; a negative or non-finite top_radiance. LIMITS: no background layers, no aerosol, no phase table, a \
   cell-constant source, no brightness temperatures. \
   ---- The thermal tracer with the rays of all g-points in one launch, counts kept by band, and a channel matrix from bands to what a \
   sensor sees, ngpt <= 1024: the longwave counterpart of the rrx_camera_ entries. The rays of a launch are the \
   concatenation, in g-point order, of n_g = m_g npix rays per g-point, m_g >= 0 rays per pixel; ray_end (ngpt+1) holds the prefix sums \
   with ray_end[0] = 0. Global index p belongs to the g with ray_end[g] <= p < ray_end[g+1] (empty ranges are stepped over); its local \
   index is q = p - ray_end[g], its stream that of ray q of rrx_thermal_trace_counts(igpt = g) and its pixel q mod npix: the same path, \
   draw for draw. Only the source that a deposit reads is scaled, and it is scaled first: (weight (1 - f_no_abs)) (lay_src weight0[g]), \
   (weight sfc_emis) (sfc_src weight0[g]), weight (top_radiance[g] weight0[g]); then the clamp at 2^20 and the tally into \
   counts[band(g), pix] (nbnd, npix). band_lims_gpt is always needed; a g-point that lies in no band has no row and its deposits are \
   dropped. With weight0[g] = 1 the counts of a band are the integer sums over its g-points of those of rrx_thermal_trace_counts. \
   rrx_thermal_trace_counts_spectral: rrx_thermal_trace_counts without igpt; top_radiance is a DEVICE array (ngpt) or NULL for 0, and \
   behind it stand the DEVICE arrays ray_end (ngpt+1) and weight0 (ngpt); k_null is rrx_rt_k_null_all's (with a NULL aer_tau); ray0 / \
   nrays are a range of the list; counts, n_capped, n_clamped are caller-zeroed, added into, and additive over ranges of the list. The \
   entry cannot look into device arrays: a ray beyond ray_end[ngpt] is stepped over and the kernel stays inside its arrays whatever \
   ray_end holds; the callers that form the list on the host refuse one that does not ascend. \
   rrx_thermal_render_spectral: rrx_thermal_render with rays_per_pixel_gpt (ngpt, HOST) = m_g in place of rays_per_pixel, and nchan, \
   chan_weights (nchan, nbnd, HOST) and radiance (nchan, npix) in W m-2 sr-1 in place of by_band and radiance; top_radiance (ngpt, HOST) \
   or NULL. weight0[g] = (F(1) / F(m_g)) / U, U = F(n_act) / F(P), n_act the number of g-points with m_g > 0, P the sum of m_g: exactly 1 \
   for equal m_g. It traces chunks of consecutive g-points (as many as keep k_null within 1 GiB, or RRX_RT_SPECTRAL_GPT_PER_LAUNCH), \
   adds all chunks' counts in integers and converts once with rrx_camera_channels and scale = U; the result does not depend on the \
   chunking. A g-point with m_g = 0 is left out of the result: the caller answers for its sources being 0. All m_g = 0: zeroes its \
   outputs and returns 0. It waits for its stream once. Refused before any HIP call: what the two entries above refuse, ngpt > 1024, \
   nbnd < 1, a NULL band_lims_gpt, ray_end, weight0 or rays_per_pixel_gpt, m_g < 0, nchan < 1, a NULL chan_weights, a negative ray0. */ \
int rrx_thermal_trace_counts##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_emis, const F* lay_src, const F* sfc_src, F top_radiance, int knx, int kny, int knz, const F* k_null, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, unsigned long long seed, long long ray0, long long nrays, int max_events, \
        unsigned long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream); \
int rrx_thermal_render##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_emis, const F* lay_src, const F* sfc_src, const F* top_radiance, int knx, int kny, int knz, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, long long rays_per_pixel, unsigned long long seed, int max_events, \
        RrxBool by_band, F* radiance, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream); \
int rrx_thermal_trace_counts_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_emis, const F* lay_src, const F* sfc_src, const F* top_radiance, \
        const long long* ray_end, const F* weight0, int knx, int kny, int knz, const F* k_null, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, unsigned long long seed, long long ray0, long long nrays, int max_events, \
        unsigned long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream); \
int rrx_thermal_render_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_emis, const F* lay_src, const F* sfc_src, const F* top_radiance, int knx, int kny, int knz, \
        int sensor_type, int npx, int npy, F fov, const F* sensor, const long long* rays_per_pixel_gpt, unsigned long long seed, \
        int max_events, int nchan, const F* chan_weights, F* radiance, unsigned long long* n_capped, unsigned long long* n_clamped, \
        void* stream); \
/* ---- 3-D longwave heating from cell sensors (csrc/rrx_raytracer_heating.hip): the net radiative power that every \
   cell of the grid takes up per unit horizontal area, flux_conv in W m-2, by emission reciprocity. The symbols begin rrx_heating3d_: \
   the set of rrx_thermal_ symbols is closed. The scene is that of \
   rrx_thermal_trace_counts without the sensor, the tracking that entry's, draw for draw. Ray r belongs to cell c = r mod (nx ny nz), \
   i = c mod nx, j = (c / nx) mod ny, k = c / (nx ny) counted upward from the surface; it starts at a uniform point of the cell in an \
   isotropic direction (five draws: x, y, z, uz = 1 - 2u, phi); Philox4x32-10 keyed by seed with counter (r low, r high, \
   igpt | 0x40000000, block). Its reference is read once from its own cell: B0 = lay_src[cell0, g] and \
   s0 = F(4 pi) (tau (1 - ssa) + cld_tau (1 - cld_ssa)); a cell with s0 = 0 ends its ray at once. The deposits are signed differences, \
   each made before the weight changes: at a collision (weight (1 - f_no_abs)) ((lay_src[cell, g] - B0) s0), at the surface \
   (weight sfc_emis) ((sfc_src[col, g] - B0) s0), through the top weight ((top_radiance - B0) s0). Each is rounded by itself, \
   llrint(clamp(d, -2^20, 2^20) 2^32) (a clamped one counts in n_clamped), summed in 64-bit integers along the ray and added with one \
   integer atomic into counts[cell0] when the ray ends (the roulette, the top, max_events, no face: the last two count in n_capped). \
   rrx_heating3d_counts: traces the rays [ray0, ray0 + nrays) of g-point igpt and ADDS into the caller-zeroed counts (nx ny nz), \
   SIGNED 64-bit in units of 2^-32 W m-2, in the layout of lay_src (cell = icol + ncol lay), and into n_capped and n_clamped. Integer \
   adds: bit-reproducible, independent of the order of arrival, additive over ray ranges. With m rays per cell \
   flux_conv of the g-point = counts 2^-32 / m. \
   rrx_heating3d_counts_spectral: the same without igpt for the rays of all g-points in one launch, ngpt <= 1024, with the DEVICE \
   arrays top_radiance (ngpt, or NULL for 0), ray_end (ngpt+1) and weight0 (ngpt) as rrx_thermal_trace_counts_spectral has them: the \
   list is the concatenation in g-point order of m_g nx ny nz rays, m_g >= 0 rays per cell; ray p of the list is ray \
   q = p - ray_end[g] of rrx_heating3d_counts(igpt = g), draw for draw; s0 is multiplied by weight0[g]. All g-points add into \
   the same nx ny nz counts: the result is broadband. band_lims_gpt is always needed and only finds the cloud triple; a g-point \
   that lies in no band has no cloud and is still tallied. k_null is rrx_rt_k_null_all's (with a NULL aer_tau). \
   rrx_heating3d_render: rays_per_cell_gpt (ngpt, HOST) = m_g and top_radiance (ngpt, HOST, or NULL for 0). Forms the list and \
   weight0[g] = (F(1) / F(m_g)) / U, U = F(n_act) / F(P) as rrx_thermal_render_spectral does, traces chunks of consecutive g-points (as \
   many as keep k_null within 1 GiB, or RRX_RT_SPECTRAL_GPT_PER_LAUNCH), adds the chunks in integers and converts once: \
   flux_conv[cell] = F(counts 2^-32) U, (ncol, nz) in the layout of lay_src, W m-2. The result does not depend on the chunking. A \
   g-point with m_g = 0 is left out of the result. All m_g = 0: zeroes its outputs and returns 0. It waits for its stream once. \
   An extent of 0 (nx, ny, nz, ngpt, nrays): returns 0 without a launch. Refused before any HIP call: what the thermal entries refuse \
   of grid, cloud triple, sources and top_radiance; a NULL counts, flux_conv, counter, k_null, ray_end, weight0 or rays_per_cell_gpt; \
   m_g < 0; a negative ray0; ngpt > 1024 and a NULL band_lims_gpt in the spectral forms. LIMITS: those of the thermal tracer; no \
   heating by band. */ \
int rrx_heating3d_counts##SFX(int nx, int ny, int nz, int ngpt, int nbnd, int igpt, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_emis, const F* lay_src, const F* sfc_src, F top_radiance, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long ray0, long long nrays, int max_events, \
        long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream); \
int rrx_heating3d_counts_spectral##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_emis, const F* lay_src, const F* sfc_src, const F* top_radiance, \
        const long long* ray_end, const F* weight0, int knx, int kny, int knz, const F* k_null, \
        unsigned long long seed, long long ray0, long long nrays, int max_events, \
        long long* counts, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream); \
int rrx_heating3d_render##SFX(int nx, int ny, int nz, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* ssa, const int* band_lims_gpt, const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        F dx, F dy, F dz, const F* sfc_emis, const F* lay_src, const F* sfc_src, const F* top_radiance, int knx, int kny, int knz, \
        const long long* rays_per_cell_gpt, unsigned long long seed, int max_events, \
        F* flux_conv, unsigned long long* n_capped, unsigned long long* n_clamped, void* stream);

RRX_DECLARE(double, _f64)
RRX_DECLARE(float, _f32)

#ifdef __cplusplus
}
#endif
#endif
