// Radiation_solver_longwave / _shortwave (GPU path): load the k-distribution and cloud LUT, then run
// gas optics -> [clouds] -> solver -> flux reduction per column block, scattering block results into the full arrays.
// Flow of /root/reference/src_test/Radiation_solver.cu:405-950; coefficient loading as :70-357 of that file.
#include <algorithm>
#include <numeric>
#include "Radiation_solver.h"
#include "Netcdf_interface.h"
#include "subset_kernels_cuda.h"
#include "fluxes_kernels_cuda.h"

namespace
{
    std::vector<std::string> get_variable_string(const std::string& var_name, std::vector<int> i_count, Netcdf_handle& nc, const int string_len)
    {
        const int total = std::accumulate(i_count.begin(), i_count.end(), 1, std::multiplies<>());
        i_count.push_back(string_len);
        const std::vector<char> chars = nc.get_variable<char>(var_name, i_count);
        std::vector<std::string> out;
        for (int n=0; n<total; ++n)
        {
            std::string s(chars.begin() + n*string_len, chars.begin() + (n+1)*string_len);
            const auto b = s.find_first_not_of(std::string(" \0", 2));
            const auto e = s.find_last_not_of(std::string(" \0", 2));
            out.push_back(b == std::string::npos ? std::string() : s.substr(b, e - b + 1));
        }
        return out;
    }

    Gas_optics_rrtmgp_gpu load_and_init_gas_optics(const Gas_concs_gpu& gas_concs, const std::string& coef_file)
    {
        Netcdf_file coef_nc(coef_file, Netcdf_mode::Read);

        const int n_temps = coef_nc.get_dimension_size("temperature");
        const int n_press = coef_nc.get_dimension_size("pressure");
        const int n_absorbers = coef_nc.get_dimension_size("absorber");
        const int n_char = coef_nc.get_dimension_size("string_len");
        const int n_minorabsorbers = coef_nc.get_dimension_size("minor_absorber");
        const int n_extabsorbers = coef_nc.get_dimension_size("absorber_ext");
        const int n_mixingfracs = coef_nc.get_dimension_size("mixing_fraction");
        const int n_layers = coef_nc.get_dimension_size("atmos_layer");
        const int n_bnds = coef_nc.get_dimension_size("bnd");
        const int n_gpts = coef_nc.get_dimension_size("gpt");
        const int n_pairs = coef_nc.get_dimension_size("pair");
        const int n_lower = coef_nc.get_dimension_size("minor_absorber_intervals_lower");
        const int n_upper = coef_nc.get_dimension_size("minor_absorber_intervals_upper");
        const int n_contributors_lower = coef_nc.get_dimension_size("contributors_lower");
        const int n_contributors_upper = coef_nc.get_dimension_size("contributors_upper");

        // NetCDF (C order) dimensions are the reverse of the Array (column-major) dimensions.
        Array<std::string,1> gas_names(get_variable_string("gas_names", {n_absorbers}, coef_nc, n_char), {n_absorbers});
        Array<int,3> key_species(coef_nc.get_variable<int>("key_species", {n_bnds, n_layers, 2}), {2, n_layers, n_bnds});
        Array<Float,2> band_lims(coef_nc.get_variable<Float>("bnd_limits_wavenumber", {n_bnds, 2}), {2, n_bnds});
        Array<int,2> band2gpt(coef_nc.get_variable<int>("bnd_limits_gpt", {n_bnds, 2}), {2, n_bnds});
        Array<Float,1> press_ref(coef_nc.get_variable<Float>("press_ref", {n_press}), {n_press});
        Array<Float,1> temp_ref(coef_nc.get_variable<Float>("temp_ref", {n_temps}), {n_temps});
        const Float temp_ref_p = coef_nc.get_variable<Float>("absorption_coefficient_ref_P");
        const Float temp_ref_t = coef_nc.get_variable<Float>("absorption_coefficient_ref_T");
        const Float press_ref_trop = coef_nc.get_variable<Float>("press_ref_trop");

        Array<Float,3> kminor_lower(coef_nc.get_variable<Float>("kminor_lower", {n_temps, n_mixingfracs, n_contributors_lower}),
                                    {n_contributors_lower, n_mixingfracs, n_temps});
        Array<Float,3> kminor_upper(coef_nc.get_variable<Float>("kminor_upper", {n_temps, n_mixingfracs, n_contributors_upper}),
                                    {n_contributors_upper, n_mixingfracs, n_temps});
        Array<std::string,1> gas_minor(get_variable_string("gas_minor", {n_minorabsorbers}, coef_nc, n_char), {n_minorabsorbers});
        Array<std::string,1> identifier_minor(get_variable_string("identifier_minor", {n_minorabsorbers}, coef_nc, n_char), {n_minorabsorbers});
        Array<std::string,1> minor_gases_lower(get_variable_string("minor_gases_lower", {n_lower}, coef_nc, n_char), {n_lower});
        Array<std::string,1> minor_gases_upper(get_variable_string("minor_gases_upper", {n_upper}, coef_nc, n_char), {n_upper});
        Array<int,2> minor_limits_gpt_lower(coef_nc.get_variable<int>("minor_limits_gpt_lower", {n_lower, n_pairs}), {n_pairs, n_lower});
        Array<int,2> minor_limits_gpt_upper(coef_nc.get_variable<int>("minor_limits_gpt_upper", {n_upper, n_pairs}), {n_pairs, n_upper});
        Array<Bool,1> minor_scales_with_density_lower(coef_nc.get_variable<Bool>("minor_scales_with_density_lower", {n_lower}), {n_lower});
        Array<Bool,1> minor_scales_with_density_upper(coef_nc.get_variable<Bool>("minor_scales_with_density_upper", {n_upper}), {n_upper});
        Array<Bool,1> scale_by_complement_lower(coef_nc.get_variable<Bool>("scale_by_complement_lower", {n_lower}), {n_lower});
        Array<Bool,1> scale_by_complement_upper(coef_nc.get_variable<Bool>("scale_by_complement_upper", {n_upper}), {n_upper});
        Array<std::string,1> scaling_gas_lower(get_variable_string("scaling_gas_lower", {n_lower}, coef_nc, n_char), {n_lower});
        Array<std::string,1> scaling_gas_upper(get_variable_string("scaling_gas_upper", {n_upper}, coef_nc, n_char), {n_upper});
        Array<int,1> kminor_start_lower(coef_nc.get_variable<int>("kminor_start_lower", {n_lower}), {n_lower});
        Array<int,1> kminor_start_upper(coef_nc.get_variable<int>("kminor_start_upper", {n_upper}), {n_upper});
        Array<Float,3> vmr_ref(coef_nc.get_variable<Float>("vmr_ref", {n_temps, n_extabsorbers, n_layers}), {n_layers, n_extabsorbers, n_temps});
        Array<Float,4> kmajor(coef_nc.get_variable<Float>("kmajor", {n_temps, n_press+1, n_mixingfracs, n_gpts}),
                              {n_gpts, n_mixingfracs, n_press+1, n_temps});

        Array<Float,3> rayl_lower, rayl_upper;
        if (coef_nc.variable_exists("rayl_lower"))
        {
            rayl_lower = Array<Float,3>(coef_nc.get_variable<Float>("rayl_lower", {n_temps, n_mixingfracs, n_gpts}), {n_gpts, n_mixingfracs, n_temps});
            rayl_upper = Array<Float,3>(coef_nc.get_variable<Float>("rayl_upper", {n_temps, n_mixingfracs, n_gpts}), {n_gpts, n_mixingfracs, n_temps});
        }

        if (coef_nc.variable_exists("totplnk"))
        {
            const int n_internal_sourcetemps = coef_nc.get_dimension_size("temperature_Planck");
            Array<Float,2> totplnk(coef_nc.get_variable<Float>("totplnk", {n_bnds, n_internal_sourcetemps}), {n_internal_sourcetemps, n_bnds});
            Array<Float,4> planck_frac(coef_nc.get_variable<Float>("plank_fraction", {n_temps, n_press+1, n_mixingfracs, n_gpts}),
                                       {n_gpts, n_mixingfracs, n_press+1, n_temps});
            Gas_optics_rrtmgp_gpu kdist(
                    gas_concs, gas_names, key_species, band2gpt, band_lims, press_ref, press_ref_trop, temp_ref, temp_ref_p, temp_ref_t,
                    vmr_ref, kmajor, kminor_lower, kminor_upper, gas_minor, identifier_minor, minor_gases_lower, minor_gases_upper,
                    minor_limits_gpt_lower, minor_limits_gpt_upper, minor_scales_with_density_lower, minor_scales_with_density_upper,
                    scaling_gas_lower, scaling_gas_upper, scale_by_complement_lower, scale_by_complement_upper,
                    kminor_start_lower, kminor_start_upper, totplnk, planck_frac, rayl_lower, rayl_upper);
            if (coef_nc.variable_exists("optimal_angle_fit"))      // (current LW files; one without it loads as before)
            {
                // the file's (fit_coeffs, bnd) -> (2, nbnd) with the coefficient index fastest
                const Array<Float,2> in(coef_nc.get_variable<Float>("optimal_angle_fit", {2, n_bnds}), {n_bnds, 2});
                Array<Float,2> fit({2, n_bnds});
                for (int ib=1; ib<=n_bnds; ++ib)
                    for (int k=1; k<=2; ++k) fit({k, ib}) = in({ib, k});
                kdist.set_optimal_angle_fit(fit);
            }
            return kdist;
        }
        else
        {
            Array<Float,1> solar_src_quiet(coef_nc.get_variable<Float>("solar_source_quiet", {n_gpts}), {n_gpts});
            Array<Float,1> solar_src_facular(coef_nc.get_variable<Float>("solar_source_facular", {n_gpts}), {n_gpts});
            Array<Float,1> solar_src_sunspot(coef_nc.get_variable<Float>("solar_source_sunspot", {n_gpts}), {n_gpts});
            const Float tsi = coef_nc.get_variable<Float>("tsi_default");
            const Float mg_index = coef_nc.get_variable<Float>("mg_default");
            const Float sb_index = coef_nc.get_variable<Float>("sb_default");
            return Gas_optics_rrtmgp_gpu(
                    gas_concs, gas_names, key_species, band2gpt, band_lims, press_ref, press_ref_trop, temp_ref, temp_ref_p, temp_ref_t,
                    vmr_ref, kmajor, kminor_lower, kminor_upper, gas_minor, identifier_minor, minor_gases_lower, minor_gases_upper,
                    minor_limits_gpt_lower, minor_limits_gpt_upper, minor_scales_with_density_lower, minor_scales_with_density_upper,
                    scaling_gas_lower, scaling_gas_upper, scale_by_complement_lower, scale_by_complement_upper,
                    kminor_start_lower, kminor_start_upper, solar_src_quiet, solar_src_facular, solar_src_sunspot,
                    tsi, mg_index, sb_index, rayl_lower, rayl_upper);
        }
    }

    Cloud_optics_gpu load_and_init_cloud_optics(const std::string& coef_file)
    {
        Netcdf_file coef_nc(coef_file, Netcdf_mode::Read);
        const int n_band = coef_nc.get_dimension_size("nband");
        const int n_rghice = coef_nc.get_dimension_size("nrghice");
        const int n_size_liq = coef_nc.get_dimension_size("nsize_liq");
        const int n_size_ice = coef_nc.get_dimension_size("nsize_ice");
        Array<Float,2> band_lims_wvn(coef_nc.get_variable<Float>("bnd_limits_wavenumber", {n_band, 2}), {2, n_band});
        const Float radliq_lwr = coef_nc.get_variable<Float>("radliq_lwr");
        const Float radliq_upr = coef_nc.get_variable<Float>("radliq_upr");
        const Float radliq_fac = coef_nc.get_variable<Float>("radliq_fac");
        const Float diamice_lwr = coef_nc.get_variable<Float>("diamice_lwr");
        const Float diamice_upr = coef_nc.get_variable<Float>("diamice_upr");
        const Float diamice_fac = coef_nc.get_variable<Float>("diamice_fac");
        Array<Float,2> lut_extliq(coef_nc.get_variable<Float>("lut_extliq", {n_band, n_size_liq}), {n_size_liq, n_band});
        Array<Float,2> lut_ssaliq(coef_nc.get_variable<Float>("lut_ssaliq", {n_band, n_size_liq}), {n_size_liq, n_band});
        Array<Float,2> lut_asyliq(coef_nc.get_variable<Float>("lut_asyliq", {n_band, n_size_liq}), {n_size_liq, n_band});
        Array<Float,3> lut_extice(coef_nc.get_variable<Float>("lut_extice", {n_rghice, n_band, n_size_ice}), {n_size_ice, n_band, n_rghice});
        Array<Float,3> lut_ssaice(coef_nc.get_variable<Float>("lut_ssaice", {n_rghice, n_band, n_size_ice}), {n_size_ice, n_band, n_rghice});
        Array<Float,3> lut_asyice(coef_nc.get_variable<Float>("lut_asyice", {n_rghice, n_band, n_size_ice}), {n_size_ice, n_band, n_rghice});
        return Cloud_optics_gpu(band_lims_wvn, radliq_lwr, radliq_upr, radliq_fac, diamice_lwr, diamice_upr, diamice_fac,
                                lut_extliq, lut_ssaliq, lut_asyliq, lut_extice, lut_ssaice, lut_asyice);
    }

    // /root/reference/src_test/Radiation_solver.cu:366-401. The file holds no band limits for these tables: the reference hands
    // over an all-zero (2, n_band) array, and so does this loader (only the band COUNT is used, by add_to).
    Aerosol_optics_gpu load_and_init_aerosol_optics(const std::string& coef_file)
    {
        Netcdf_file coef_nc(coef_file, Netcdf_mode::Read);
        const int n_band = coef_nc.get_dimension_size("band_sw");
        const int n_hum = coef_nc.get_dimension_size("relative_humidity");
        const int n_philic = coef_nc.get_dimension_size("hydrophilic");
        const int n_phobic = coef_nc.get_dimension_size("hydrophobic");
        Array<Float,2> band_lims_wvn({2, n_band});
        Array<Float,2> mext_phobic(coef_nc.get_variable<Float>("mass_ext_sw_hydrophobic", {n_phobic, n_band}), {n_band, n_phobic});
        Array<Float,2> ssa_phobic(coef_nc.get_variable<Float>("ssa_sw_hydrophobic", {n_phobic, n_band}), {n_band, n_phobic});
        Array<Float,2> g_phobic(coef_nc.get_variable<Float>("asymmetry_sw_hydrophobic", {n_phobic, n_band}), {n_band, n_phobic});
        Array<Float,3> mext_philic(coef_nc.get_variable<Float>("mass_ext_sw_hydrophilic", {n_philic, n_hum, n_band}), {n_band, n_hum, n_philic});
        Array<Float,3> ssa_philic(coef_nc.get_variable<Float>("ssa_sw_hydrophilic", {n_philic, n_hum, n_band}), {n_band, n_hum, n_philic});
        Array<Float,3> g_philic(coef_nc.get_variable<Float>("asymmetry_sw_hydrophilic", {n_philic, n_hum, n_band}), {n_band, n_hum, n_philic});
        Array<Float,1> rh_upper(coef_nc.get_variable<Float>("relative_humidity2", {n_hum}), {n_hum});
        return Aerosol_optics_gpu(band_lims_wvn, rh_upper, mext_phobic, ssa_phobic, g_phobic, mext_philic, ssa_philic, g_philic);
    }

    // contiguous column blocks {1-based start, size}
    std::vector<std::pair<int,int>> column_blocks(const int n_col, const int n_col_block)
    {
        std::vector<std::pair<int,int>> b;
        for (int s=1; s<=n_col; s+=n_col_block) b.emplace_back(s, std::min(n_col_block, n_col - s + 1));
        return b;
    }

    // ---- column order of a solve (include_test/Radiation_solver.h: set_column_sorting / set_column_padding) ----
    // A gather index over the caller's columns: sorted by surface pressure and / or padded to a multiple of 16 by repeating the last one.
    // Sunlit-only SW (set_sunlit_columns): a subset -- perm[0 .. n_keep) lists the columns with mu0 > 0, padded to n_out -- and out()
    // writes zeros to every other column of the caller's arrays.
    struct Column_order
    {
        int n_col = 0, n_out = 0, n_keep = 0;
        bool subset = false;
        Array_gpu<int,1> perm;
        bool active() const { return n_out > 0 || subset; }
        // (col, n2) -> (n_out, n2); an absent (empty) array stays absent
        Array_gpu<Float,2> in2(const Array_gpu<Float,2>& a) const
        {
            if (a.size() == 0) return Array_gpu<Float,2>();
            Array_gpu<Float,2> o({n_out, a.dim(2)});
            RRX_CALL(rrx_gather_cols, n_out, (unsigned long long)a.dim(2), perm.ptr(), n_col, a.ptr(), o.ptr());
            return o;
        }
        Array_gpu<Float,1> in1(const Array_gpu<Float,1>& a) const
        {
            if (a.size() == 0) return Array_gpu<Float,1>();
            Array_gpu<Float,1> o({n_out});
            RRX_CALL(rrx_gather_cols, n_out, 1ull, perm.ptr(), n_col, a.ptr(), o.ptr());
            return o;
        }
        // (n1, col) -> (n1, n_out)
        Array_gpu<Float,2> in_last(const Array_gpu<Float,2>& a) const
        {
            if (a.size() == 0) return Array_gpu<Float,2>();
            Array_gpu<Float,2> o({a.dim(1), n_out});
            RRX_CALL(rrx_gather_lastdim, a.dim(1), n_out, perm.ptr(), a.ptr(), o.ptr());
            return o;
        }
        // results of the reordered solve back into the caller's arrays (first n_col entries of perm: the permutation proper)
        template<int N> void out(Array_gpu<Float,N>& dst, const Array_gpu<Float,N>& src) const
        {
            if (src.size() == 0) return;
            std::array<int,N> d; d[0] = n_col; unsigned long long rest = 1;
            for (int i=1; i<N; ++i) { d[i] = src.dim(i+1); rest *= (unsigned long long)src.dim(i+1); }
            if (dst.size() == 0) dst.set_dims(d);
            if (subset) RRX_CALL(rrx_scatter_cols_fill, n_keep, rest, perm.ptr(), n_out, src.ptr(), n_col, dst.ptr());
            else RRX_CALL(rrx_scatter_cols, n_col, rest, perm.ptr(), n_out, src.ptr(), n_col, dst.ptr());
        }
        // a subset without columns: the caller's (col, dims...) array is all zeros
        template<int N> void zeros(Array_gpu<Float,N>& dst, const std::array<int,N>& d) const
        {
            if (dst.size() == 0) dst.set_dims(d);
            unsigned long long rest = 1;
            for (int i=1; i<N; ++i) rest *= (unsigned long long)d[i];
            RRX_CALL(rrx_scatter_cols_fill, 0, rest, nullptr, 0, nullptr, n_col, dst.ptr());
        }
    };

    // The sunlit columns of a solve (mu0 > 0), in the order `co` gives them (sorting) or in the caller's, padded to a multiple of 16
    // when padding is on. The count sizes the solve, so it is read back here: this synchronises once per shortwave solve.
    Column_order sunlit_column_order(const Column_order& co, const int n_col, const Array_gpu<Float,1>& mu0, const bool pad)
    {
        Column_order day;
        const int pad_to = (pad && n_col > 16) ? 16 : 1;
        day.n_col = n_col; day.subset = true;
        day.perm.set_dims({std::max(1, (n_col + pad_to - 1) / pad_to * pad_to)});
        Array_gpu<int,1> count({1});
        RRX_CALL(rrx_sunlit_columns, n_col, mu0.ptr(), co.active() ? co.perm.ptr() : nullptr, pad_to, day.perm.ptr(), count.ptr());
        rrx_host::check(rrx_memcpy_d2h_stream(&day.n_keep, count.ptr(), sizeof(int), rrx_host::current_stream()));
        day.n_out = (day.n_keep + pad_to - 1) / pad_to * pad_to;
        return day;
    }

    // McICA cloud sampling of a reordered solve (set_cloud_sampling): the solver's borrowed fields are replaced by their gathered
    // copies and the columns' identities (perm + offset) for the duration of the inner solve, and put back afterwards.
    struct Sampling_reordered
    {
        Cloud_sampling& s; const Cloud_sampling s0;
        Array_gpu<Float,2> frac_r, alpha_r; Array_gpu<int,1> ids;
        Sampling_reordered(Cloud_sampling& s_, const Column_order& co) : s(s_), s0(s_)
        {
            if (!s0.on()) return;
            frac_r = co.in2(*s0.frac); s.frac = &frac_r;
            if (s0.alpha != nullptr) { alpha_r = co.in2(*s0.alpha); s.alpha = &alpha_r; }
            ids.set_dims({co.n_out});
            rrx_host::check(rrx_mcica_column_ids(co.n_out, co.perm.ptr(), s0.col_offset, ids.ptr(), rrx_host::current_stream()));
            s.col_id = ids.ptr();
        }
        ~Sampling_reordered() { s = s0; }
    };

    // The borrowed altitude fields of a reordered shortwave solve (set_spherical_mu0): replaced by their gathered copies for the
    // duration of the inner solve, and put back afterwards.
    struct Altitudes_reordered
    {
        const Array_gpu<Float,2>*& alt; const Array_gpu<Float,1>*& ref;
        const Array_gpu<Float,2>* alt0; const Array_gpu<Float,1>* ref0;
        Array_gpu<Float,2> alt_r; Array_gpu<Float,1> ref_r;
        Altitudes_reordered(const Array_gpu<Float,2>*& a, const Array_gpu<Float,1>*& r, const Column_order& co) : alt(a), ref(r), alt0(a), ref0(r)
        {
            if (alt0 == nullptr) return;
            alt_r = co.in2(*alt0); alt = &alt_r;
            if (ref0 != nullptr) { ref_r = co.in1(*ref0); ref = &ref_r; }
        }
        ~Altitudes_reordered() { alt = alt0; ref = ref0; }
    };

    // Marks the inner solve of a reordered one, which takes its columns as they come.
    struct Guard { bool& f; Guard(bool& f_) : f(f_) { f = true; } ~Guard() { f = false; } };

    // One column block of a solve: columns col_s .. col_s + n_in - 1 (1-based) of the caller's n_col. A single block (whole) views the
    // caller's arrays and gases -- no gather of the inputs, no device copies of the mixing-ratio fields -- and any other gets copies of
    // its columns.
    struct Block
    {
        int n_col, col_s, n_in;
        bool whole;
        std::unique_ptr<Gas_concs_gpu> gases_copy;
        const Gas_concs_gpu& gases;
        Block(const int n_col_, const std::pair<int,int>& b, const Gas_concs_gpu& all) :
            n_col(n_col_), col_s(b.first), n_in(b.second), whole(b.second == n_col_),
            gases_copy(whole ? nullptr : std::make_unique<Gas_concs_gpu>(all, col_s, n_in)), gases(whole ? all : *gases_copy) {}
        int col_e() const { return col_s + n_in - 1; }
        Array_gpu<Float,1> sub1(const Array_gpu<Float,1>& a) const
        { return whole ? Array_gpu<Float,1>(const_cast<Float*>(a.ptr()), {n_in}) : a.subset({{ {col_s, col_e()} }}); }
        // (col, n2)
        Array_gpu<Float,2> sub2(const Array_gpu<Float,2>& a, const int n2) const
        { return whole ? Array_gpu<Float,2>(const_cast<Float*>(a.ptr()), {n_in, n2}) : a.subset({{ {col_s, col_e()}, {1, n2} }}); }
        // (n_bnd, col)
        Array_gpu<Float,2> sub_last(const Array_gpu<Float,2>& a, const int n_bnd) const
        { return whole ? Array_gpu<Float,2>(const_cast<Float*>(a.ptr()), {n_bnd, n_in}) : a.subset({{ {1, n_bnd}, {col_s, col_e()} }}); }
        // the caller's dry-air column amounts, or those of the block's water vapour and pressures
        Array_gpu<Float,2> col_dry(const Array_gpu<Float,2>& col_dry, const Array_gpu<Float,2>& p_lev_s, const int n_lay) const
        {
            Array_gpu<Float,2> col_dry_s({n_in, n_lay});
            if (col_dry.size() == 0)
                Gas_optics_rrtmgp_gpu::get_col_dry(col_dry_s, gases.get_vmr("h2o"), p_lev_s);
            else
                col_dry_s = sub2(col_dry, n_lay);
            return col_dry_s;
        }
    };

    // Flux arrays, broadband (col, lev) and by band (col, lev, bnd), in the order of the solve_gpu argument lists: up, dn[, dn_dir], net.
    template<typename A2, typename A3> struct Flux_set { std::vector<A2> bb; std::vector<A3> bnd; };
    using Flux_arrays = Flux_set<Array_gpu<Float,2>, Array_gpu<Float,3>>;        // arrays of a solve's own
    struct Flux_outputs : Flux_set<Array_gpu<Float,2>*, Array_gpu<Float,3>*>     // the caller's
    {
        int n_col, n_lev, n_bnd;
        void allocate_bb() const { for (Array_gpu<Float,2>* a : bb) if (a->size() == 0) a->set_dims({n_col, n_lev}); }
        void allocate_bnd() const { for (Array_gpu<Float,3>* a : bnd) if (a->size() == 0) a->set_dims({n_col, n_lev, n_bnd}); }
        // a reordered solve: its output arrays on n_out columns, and their way back into the caller's
        Flux_arrays reordered(const int n_out, const bool with_bnd) const
        {
            Flux_arrays r{std::vector<Array_gpu<Float,2>>(bb.size()), std::vector<Array_gpu<Float,3>>(bnd.size())};
            for (auto& a : r.bb) a.set_dims({n_out, n_lev});
            if (with_bnd) for (auto& a : r.bnd) a.set_dims({n_out, n_lev, n_bnd});
            return r;
        }
        void from_reordered(const Column_order& co, const Flux_arrays& r, const bool with_bnd) const
        {
            for (size_t i=0; i<bb.size(); ++i) co.out(*bb[i], r.bb[i]);
            if (with_bnd) for (size_t i=0; i<bnd.size(); ++i) co.out(*bnd[i], r.bnd[i]);
        }
        // a sunlit-only solve without sunlit columns
        void zeros(const Column_order& co, const bool with_bnd) const
        {
            for (Array_gpu<Float,2>* a : bb) co.zeros<2>(*a, {n_col, n_lev});
            if (with_bnd) for (Array_gpu<Float,3>* a : bnd) co.zeros<3>(*a, {n_col, n_lev, n_bnd});
        }
        // a block's arrays into its columns of the caller's: the three- and four-array get_from_subset
        void from_block(const Block& b, const std::vector<const Float*>& s) const
        {
            if (s.size() == 3) Subset_kernels_cuda::get_from_subset(n_col, n_lev, b.n_in, b.col_s, bb[0]->ptr(), bb[1]->ptr(), bb[2]->ptr(), s[0], s[1], s[2]);
            else Subset_kernels_cuda::get_from_subset(n_col, n_lev, b.n_in, b.col_s, bb[0]->ptr(), bb[1]->ptr(), bb[2]->ptr(), bb[3]->ptr(), s[0], s[1], s[2], s[3]);
        }
        void bnd_from_block(const Block& b, const std::vector<const Float*>& s) const
        {
            if (s.size() == 3) Subset_kernels_cuda::get_from_subset(n_col, n_lev, n_bnd, b.n_in, b.col_s, bnd[0]->ptr(), bnd[1]->ptr(), bnd[2]->ptr(), s[0], s[1], s[2]);
            else Subset_kernels_cuda::get_from_subset(n_col, n_lev, n_bnd, b.n_in, b.col_s, bnd[0]->ptr(), bnd[1]->ptr(), bnd[2]->ptr(), bnd[3]->ptr(), s[0], s[1], s[2], s[3]);
        }
        // The general tail of a block: the g-point fluxes of the workspace (dir: null in the longwave) reduced to broadband and, where
        // asked for, band fluxes, and copied into the block's columns of the caller's arrays.
        void reduce_block(const Block& b, const bool with_bnd, const Array_gpu<Float,3>& up, const Array_gpu<Float,3>& dn, const Array_gpu<Float,3>* dir,
                          const std::unique_ptr<Optical_props_arry_gpu>& optical_props, const Bool top_at_1) const
        {
            Fluxes_broadband_gpu fluxes(b.n_in, n_lev);
            if (dir == nullptr) fluxes.reduce(up, dn, optical_props, top_at_1); else fluxes.reduce(up, dn, *dir, optical_props, top_at_1);
            if (dir == nullptr) from_block(b, {fluxes.get_flux_up().ptr(), fluxes.get_flux_dn().ptr(), fluxes.get_flux_net().ptr()});
            else from_block(b, {fluxes.get_flux_up().ptr(), fluxes.get_flux_dn().ptr(), fluxes.get_flux_dn_dir().ptr(), fluxes.get_flux_net().ptr()});
            if (!with_bnd) return;
            Fluxes_byband_gpu bnd_fluxes(b.n_in, n_lev, n_bnd);
            if (dir == nullptr) bnd_fluxes.reduce(up, dn, optical_props, top_at_1); else bnd_fluxes.reduce(up, dn, *dir, optical_props, top_at_1);
            if (dir == nullptr) bnd_from_block(b, {bnd_fluxes.get_bnd_flux_up().ptr(), bnd_fluxes.get_bnd_flux_dn().ptr(), bnd_fluxes.get_bnd_flux_net().ptr()});
            else bnd_from_block(b, {bnd_fluxes.get_bnd_flux_up().ptr(), bnd_fluxes.get_bnd_flux_dn().ptr(), bnd_fluxes.get_bnd_flux_dn_dir().ptr(),
                                    bnd_fluxes.get_bnd_flux_net().ptr()});
        }
    };

    // What the by-band solver of one block writes, as views in the order of Flux_outputs: the caller's arrays for a single block, else
    // block arrays -- the workspace's band slabs `ws_bnd` for all but the band net flux -- that finish() copies into place.
    struct Byband_block : Flux_arrays
    {
        Flux_arrays blk;
        Byband_block(const Block& b, const Flux_outputs& out, const std::vector<Array_gpu<Float,3>*>& ws_bnd)
        {
            out.allocate_bb(); out.allocate_bnd();
            const size_t n = out.bb.size();
            if (!b.whole)
            {
                blk.bnd.resize(1); blk.bnd[0].set_dims({b.n_in, out.n_lev, out.n_bnd});
                blk.bb.resize(n); for (auto& a : blk.bb) a.set_dims({b.n_in, out.n_lev});
            }
            for (size_t i=0; i<n; ++i)
            {
                Float* band = b.whole ? out.bnd[i]->ptr() : (i+1 < n ? ws_bnd[i]->ptr() : blk.bnd[0].ptr());
                bnd.emplace_back(band, std::array<int,3>{b.n_in, out.n_lev, out.n_bnd});
                bb.emplace_back(b.whole ? out.bb[i]->ptr() : blk.bb[i].ptr(), std::array<int,2>{b.n_in, out.n_lev});
            }
        }
        // the broadband net flux from the solver's up and dn; the block arrays into the caller's
        void finish(const Block& b, const Flux_outputs& out)
        {
            Fluxes_kernels_cuda::net_broadband_precalc(b.n_in, out.n_lev, bb[1].ptr(), bb[0].ptr(), bb.back().ptr());
            if (b.whole) return;
            std::vector<const Float*> s2, s3;
            for (const auto& a : bb) s2.push_back(a.ptr());
            for (const auto& a : bnd) s3.push_back(a.ptr());
            out.from_block(b, s2); out.bnd_from_block(b, s3);
        }
    };

    // The sub-columns of one block (rrx_mcica_increment_1scalar / _2stream): `launch` gets the arguments the two domains share.
    template<typename Launch> void sample_clouds(const Cloud_sampling& s, const Block& b, const int n_lay, const int n_gpt, const int n_bnd,
                                                 const int* band_lims_gpt, const int domain, Launch&& launch)
    {
        const Array_gpu<Float,2> frac_s = b.sub2(*s.frac, n_lay);
        const Array_gpu<Float,2> alpha_s = (s.alpha != nullptr && n_lay > 1) ? b.sub2(*s.alpha, n_lay-1) : Array_gpu<Float,2>();
        launch(b.n_in, n_lay, n_gpt, n_bnd, band_lims_gpt, frac_s.ptr(), s.alpha != nullptr ? alpha_s.ptr() : nullptr, (unsigned long long)s.seed, domain,
               s.col_id != nullptr ? s.col_id + (b.col_s-1) : nullptr, s.col_offset + b.col_s-1);
    }

    // Should this solve reorder its columns, and how? `sort_decided` caches the automatic decision of the solver object.
    Column_order column_order(const int mode, int& sort_decided, const bool pad, const Array_gpu<Float,2>& p_lev, const Bool top_at_1)
    {
        Column_order co;
        const int n_col = p_lev.dim(1), n_lev = p_lev.dim(2);
        const Float* p_sfc = p_lev.ptr() + size_t(top_at_1 ? n_lev-1 : 0)*n_col;
        bool sort = mode == 1;
        if (mode < 0 && n_col >= 256)
        {
            if (sort_decided < 0)
            {
                Array_gpu<int,1> flag({1});
                RRX_CALL(rrx_column_spread, n_col, p_sfc, 256, Float(0.2), flag.ptr());
                int h = 0;
                rrx_host::check(rrx_memcpy_d2h_stream(&h, flag.ptr(), sizeof(int), rrx_host::current_stream()));     // (synchronises: once per solver)
                sort_decided = h ? 1 : 0;
            }
            sort = sort_decided == 1;
        }
        const int n_pad = (pad && n_col > 16 && n_col % 16 != 0) ? 16 - n_col % 16 : 0;
        if (!sort && n_pad == 0) return co;
        co.n_col = n_col; co.n_out = n_col + n_pad;
        co.perm.set_dims({co.n_out});
        if (sort) RRX_CALL(rrx_sort_columns, n_col, p_sfc, n_pad, co.perm.ptr());
        else rrx_host::check(rrx_identity_columns(n_col, n_pad, co.perm.ptr(), rrx_host::current_stream()));
        return co;
    }
}


void compute_heating_rate(const Array_gpu<Float,2>& flux_net, const Array_gpu<Float,2>& p_lev, Array_gpu<Float,2>& heating_rate)
{
    const int n_col = flux_net.dim(1), n_lev = flux_net.dim(2);
    if (p_lev.dim(1) != n_col || p_lev.dim(2) != n_lev) throw std::runtime_error("compute_heating_rate: flux and pressure shapes differ");
    if (heating_rate.size() == 0) heating_rate.set_dims({n_col, n_lev-1});
    RRX_CALL(rrx_heating_rate, n_col, n_lev-1, Float(9.80665/1004.64), flux_net.ptr(), p_lev.ptr(), heating_rate.ptr());
}


// -------------------------------------------------------------------------------------------- longwave
struct Radiation_solver_longwave::Workspace
{
    int n_col = 0, n_lay = 0;
    bool broadband = false, byband = false, jacobian = false;
    std::unique_ptr<Optical_props_arry_gpu> optical_props;
    std::unique_ptr<Optical_props_1scl_gpu> cloud_optical_props;
    std::unique_ptr<Optical_props_2str_gpu> cloud_optical_props_2str;      // LW scattering: tau / ssa / g by band
    std::unique_ptr<Source_func_lw_gpu> sources;
    Array_gpu<Float,3> gpt_flux_up, gpt_flux_dn;       // (n_col, n_lev, 1 | n_bnd (by-band solvers) | n_gpt)
    Array_gpu<Float,3> gpt_flux_up_jac;                // (n_col, n_lev, 1 | n_gpt) with the Jacobian
    Array_gpu<Float,2> flux_up_jac;                    // (n_col, n_lev): its g-point sum (per-g-point solvers)
};

Radiation_solver_longwave::Radiation_solver_longwave(
        const Gas_concs_gpu& gas_concs, const std::string& file_name_gas, const std::string& file_name_cloud)
{
    this->kdist_gpu = std::make_unique<Gas_optics_rrtmgp_gpu>(load_and_init_gas_optics(gas_concs, file_name_gas));
    if (!file_name_cloud.empty())
        this->cloud_optics_gpu = std::make_unique<Cloud_optics_gpu>(load_and_init_cloud_optics(file_name_cloud));
}

void Cloud_sampling::set(const char* who, const Array_gpu<Float,2>* cloud_frac, const int overlap, const Array_gpu<Float,2>* overlap_param,
                         const uint64_t seed_in, const int col_offset_in)
{
    const std::string w = std::string(who) + "::set_cloud_sampling: ";
    if (overlap != 0 && overlap != 1)
        throw std::runtime_error(w + "overlap " + std::to_string(overlap) + " is not 0 (maximum-random) or 1 (exponential-random)");
    if (cloud_frac != nullptr && overlap == 1 && overlap_param == nullptr)
        throw std::runtime_error(w + "exponential-random overlap needs overlap_param");
    frac = cloud_frac; alpha = (cloud_frac != nullptr && overlap == 1) ? overlap_param : nullptr;
    seed = seed_in; col_offset = col_offset_in;
}

void Cloud_sampling::check(const char* who, const int n_col, const int n_lay, const bool cloud_optics) const
{
    const std::string w(who);
    if (!cloud_optics) throw std::runtime_error(w + ": cloud sampling (set_cloud_sampling) needs cloud optics: it samples their band properties");
    if (frac->dim(1) != n_col || frac->dim(2) != n_lay) throw std::runtime_error(w + ": set_cloud_sampling: cloud_frac is not (ncol, nlay)");
    if (alpha != nullptr && n_lay > 1 && (alpha->dim(1) != n_col || alpha->dim(2) != n_lay-1))
        throw std::runtime_error(w + ": set_cloud_sampling: overlap_param is not (ncol, nlay-1)");
}

void Radiation_solver_longwave::set_cloud_sampling(const Array_gpu<Float,2>* cloud_frac, const int overlap, const Array_gpu<Float,2>* overlap_param,
                                                   const uint64_t seed, const int col_offset)
{ mcica.set("Radiation_solver_longwave", cloud_frac, overlap, overlap_param, seed, col_offset); }

// ---- the LW options of the class API: what a solve_gpu call does, or why it is refused ----
namespace
{
    // An option as the refusals see it. Some look at the solver's setting, some at what the call makes of it (`in use`): the by-band
    // solvers and the Jacobian come in both kinds, and each row below says which one it means.
    enum Lw_option { jacobian_in_use, jacobian_set, byband_in_use, byband_set, several_angles, optimal, scattering, rescaling,
                     no_broadband_fluxes, sampling, n_lw_options };
    const char* const lw_option_name[n_lw_options] = {
        "the Jacobian (set_jacobian)", "the Jacobian (set_jacobian)", "the by-band solvers (set_byband_solvers)", "the by-band solvers (set_byband_solvers)",
        "several quadrature angles (set_gauss_angles)", "optimal angles (set_optimal_angles)", "LW scattering (set_lw_scattering)",
        "LW rescaling (set_lw_rescaling)", "the broadband solvers (set_broadband_solvers) without band flux output", "cloud sampling (set_cloud_sampling)"};
    // `option` is (are) not available with `other`; with no_broadband_fluxes as the other: `option` needs the broadband solvers ...
    struct Lw_refusal { Lw_option option, other; const char* reason; };
    const Lw_refusal lw_refusals[] = {
        {jacobian_in_use, byband_set,          "no by-band Jacobians"},
        {several_angles,  byband_in_use,       "the by-band solver has one angle"},
        {optimal,         several_angles,      "optimal angles are one angle"},
        {optimal,         byband_set,          "the by-band solver has the fixed angle"},
        {scattering,      several_angles,      "the two-stream solver has no angles"},
        {scattering,      optimal,             "the two-stream solver has no angles"},
        {scattering,      jacobian_set,        "no Jacobian form of the two-stream solver"},
        {scattering,      byband_set,          "no by-band form of the two-stream solver"},
        {scattering,      no_broadband_fluxes, "the two-stream solver gives broadband fluxes"},
        {rescaling,       scattering,          "one treatment of cloud scattering at a time"},
        {rescaling,       several_angles,      "the fused rescaled solver has one angle"},
        {rescaling,       optimal,             "the fused rescaled solver has the fixed angle"},
        {rescaling,       jacobian_set,        "no Jacobian form of the fused rescaled solver"},
        {rescaling,       byband_set,          "no by-band form of the rescaled solver"},
        {rescaling,       no_broadband_fluxes, "the fused rescaled solver gives broadband fluxes"},
        {sampling,        scattering,          "the two-stream solver combines the band clouds itself"},
        {sampling,        rescaling,           "the rescaled solver combines the band clouds itself"}};
}

Lw_solve_plan lw_solve_plan(const Lw_solve_options& o)
{
    Lw_solve_plan p;
    p.broadband = o.broadband_solvers && !o.switch_output_bnd_fluxes;
    p.byband = o.byband_solvers && o.switch_output_bnd_fluxes && o.switch_fluxes && o.fewer_bands_than_gpoints;
    p.jac = o.jacobian && o.switch_fluxes;
    p.cloud_to_solver = (o.lw_scattering || o.lw_rescaling) && o.switch_fluxes;

    bool on[n_lw_options];
    on[jacobian_in_use] = p.jac;                    on[jacobian_set] = o.jacobian;
    on[byband_in_use] = p.byband;                   on[byband_set] = o.byband_solvers;
    on[several_angles] = o.n_gauss_angles > 1;      on[optimal] = o.optimal_angles;
    on[scattering] = o.lw_scattering;               on[rescaling] = o.lw_rescaling;
    on[no_broadband_fluxes] = o.switch_fluxes && !p.broadband;
    on[sampling] = o.cloud_sampling;
    for (const Lw_refusal& r : lw_refusals)
        if (on[r.option] && on[r.other])
        {
            const bool plural = r.option == several_angles || r.option == optimal;
            throw std::runtime_error(std::string("Radiation_solver_longwave: ") + lw_option_name[r.option] +
                                     (r.other == no_broadband_fluxes ? " needs " : plural ? " are not available with " : " is not available with ") +
                                     lw_option_name[r.other] + ": " + r.reason);
        }

    if (p.byband) p.form = Lw_form::byband;
    else if (o.lw_rescaling && o.switch_fluxes) p.form = Lw_form::rescaled;
    else if (p.cloud_to_solver) p.form = Lw_form::two_stream;
    else if (o.optimal_angles) p.form = Lw_form::optimal;
    else if (!p.broadband) p.form = Lw_form::per_gpoint;
    else p.form = o.n_gauss_angles > 1 ? Lw_form::angles : Lw_form::fractions;
    return p;
}

void Radiation_solver_longwave::set_optimal_angles(const bool b)
{
    if (b && !kdist_gpu->has_optimal_angle_fit())
        throw std::runtime_error("Radiation_solver_longwave::set_optimal_angles: the longwave coefficient file has no optimal_angle_fit");
    optimal_angles = b;
}

void Radiation_solver_longwave::solve_gpu(
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
        Array_gpu<Float,3>& lw_bnd_flux_up, Array_gpu<Float,3>& lw_bnd_flux_dn, Array_gpu<Float,3>& lw_bnd_flux_net)
{
    const int n_col = p_lay.dim(1);
    const int n_lay = p_lay.dim(2);
    const int n_lev = p_lev.dim(2);
    const int n_gpt = this->kdist_gpu->get_ngpt();
    const int n_bnd = this->kdist_gpu->get_nband();
    const Bool top_at_1 = (vertical_ordering < 0) ? Bool(p_lay({1, 1}) < p_lay({1, n_lay})) : Bool(vertical_ordering == 1);
    if (switch_cloud_optics && !cloud_optics_gpu) throw std::runtime_error("cloud optics requested but no cloud coefficients loaded");
    // (throws what is not available: the one table of refusals)
    const Lw_solve_plan plan = lw_solve_plan({broadband_solvers, byband_solvers, jacobian, n_gauss_angles, optimal_angles, lw_scattering, lw_rescaling,
                                              mcica.on(), switch_fluxes, switch_output_bnd_fluxes, switch_cloud_optics, n_bnd < n_gpt});
    if (mcica.on()) mcica.check("Radiation_solver_longwave", n_col, n_lay, switch_cloud_optics);
    if (plan.jac && (lw_flux_up_jac.dim(1) != n_col || lw_flux_up_jac.dim(2) != n_lev))
    {
        lw_flux_up_jac = Array_gpu<Float,2>();
        lw_flux_up_jac.set_dims({n_col, n_lev});
    }
    const Flux_outputs out{{{&lw_flux_up, &lw_flux_dn, &lw_flux_net}, {&lw_bnd_flux_up, &lw_bnd_flux_dn, &lw_bnd_flux_net}}, n_col, n_lev, n_bnd};

    // columns in another order / on a padded count: gather the inputs, solve, scatter the fluxes back (see the header)
    if (!reordered_call && !switch_output_optical && switch_fluxes)
    {
        const Column_order co = column_order(column_sorting, sort_decided, column_padding, p_lev, top_at_1);
        if (co.active())
        {
            const Gas_concs_gpu gases = gas_concs.gathered(co.perm, n_col, co.n_out);
            Array_gpu<Float,3> no3a, no3b, no3c; Array_gpu<Float,2> no2;
            Flux_arrays r = out.reordered(co.n_out, switch_output_bnd_fluxes);
            Guard guard(reordered_call);
            Sampling_reordered sampling(mcica, co);
            this->solve_gpu(switch_fluxes, switch_cloud_optics, switch_output_optical, switch_output_bnd_fluxes, gases,
                            co.in2(p_lay), co.in2(p_lev), co.in2(t_lay), co.in2(t_lev), co.in2(col_dry), co.in1(t_sfc), co.in_last(emis_sfc),
                            co.in2(lwp), co.in2(iwp), co.in2(rel), co.in2(dei), no3a, no3b, no3c, no2,
                            r.bb[0], r.bb[1], r.bb[2], r.bnd[0], r.bnd[1], r.bnd[2]);
            out.from_reordered(co, r, switch_output_bnd_fluxes);
            if (plan.jac)
            {
                // (the inner solve left its (n_out, n_lev) Jacobian in lw_flux_up_jac)
                const Array_gpu<Float,2> jac_r = std::move(lw_flux_up_jac);
                lw_flux_up_jac = Array_gpu<Float,2>();
                lw_flux_up_jac.set_dims({n_col, n_lev});
                co.out(lw_flux_up_jac, jac_r);
            }
            return;
        }
    }

    const bool cloud_1scl = switch_cloud_optics && !plan.cloud_to_solver, cloud_2str = switch_cloud_optics && plan.cloud_to_solver;
    auto prepare = [&](std::shared_ptr<Workspace>& ws, const int n)
    {
        if (!ws || ws->n_col != n || ws->n_lay != n_lay || ws->broadband != plan.broadband || ws->byband != plan.byband || ws->jacobian != plan.jac)
        {
            ws = std::make_shared<Workspace>();
            ws->n_col = n; ws->n_lay = n_lay; ws->broadband = plan.broadband; ws->byband = plan.byband; ws->jacobian = plan.jac;
            ws->optical_props = std::make_unique<Optical_props_1scl_gpu>(n, n_lay, *kdist_gpu);
            ws->sources = std::make_unique<Source_func_lw_gpu>(n, n_lay, *kdist_gpu);
            // broadband and by-band solvers: Planck fractions instead of the two source arrays (they are materialised on demand,
            // e.g. for --output-optical)
            ws->sources->enable_planck_lite(plan.broadband || plan.byband);
            const int ng = plan.broadband ? 1 : (plan.byband ? n_bnd : n_gpt);
            ws->gpt_flux_up.set_dims({n, n_lev, ng});
            ws->gpt_flux_dn.set_dims({n, n_lev, ng});
            if (plan.jac)
            {
                ws->gpt_flux_up_jac.set_dims({n, n_lev, ng});
                if (!plan.broadband) ws->flux_up_jac.set_dims({n, n_lev});
            }
        }
        if (cloud_1scl && !ws->cloud_optical_props)
            ws->cloud_optical_props = std::make_unique<Optical_props_1scl_gpu>(n, n_lay, *cloud_optics_gpu);
        if (cloud_2str && !ws->cloud_optical_props_2str)
            ws->cloud_optical_props_2str = std::make_unique<Optical_props_2str_gpu>(n, n_lay, *cloud_optics_gpu);
    };

    for (const auto& columns : column_blocks(n_col, std::max(1, n_col_block)))
    {
        const int col_s = columns.first, n_in = columns.second;
        std::shared_ptr<Workspace>& wsp = (n_in == std::min(n_col_block, n_col)) ? ws_block : ws_residual;
        prepare(wsp, n_in);
        Workspace& ws = *wsp;
        const Block blk(n_col, columns, gas_concs);
        Array_gpu<Float,2> p_lay_s = blk.sub2(p_lay, n_lay), t_lay_s = blk.sub2(t_lay, n_lay);
        Array_gpu<Float,2> p_lev_s = blk.sub2(p_lev, n_lev), t_lev_s = blk.sub2(t_lev, n_lev);
        Array_gpu<Float,1> t_sfc_s = blk.sub1(t_sfc);
        Array_gpu<Float,2> col_dry_s = blk.col_dry(col_dry, p_lev_s, n_lay);

        // (cloud optics first: its by-band optical depth is added inside gas_optics where tau is stored -- the add_to() of
        //  Radiation_solver.cu:508-511 folded into the producer)
        // LW scattering: the gas optics stay clear; the band cloud tau / ssa / g (not delta-scaled) go to the two-stream solver
        if (cloud_2str)
            cloud_optics_gpu->cloud_optics(blk.sub2(lwp, n_lay), blk.sub2(iwp, n_lay), blk.sub2(rel, n_lay), blk.sub2(dei, n_lay), *ws.cloud_optical_props_2str);
        else if (cloud_1scl)
            cloud_optics_gpu->cloud_optics(blk.sub2(lwp, n_lay), blk.sub2(iwp, n_lay), blk.sub2(rel, n_lay), blk.sub2(dei, n_lay), *ws.cloud_optical_props);
        kdist_gpu->gas_optics(p_lay_s, p_lev_s, t_lay_s, t_sfc_s, blk.gases, ws.optical_props, *ws.sources, col_dry_s, t_lev_s,
                              (cloud_1scl && !mcica.on()) ? ws.cloud_optical_props.get() : nullptr);
        if (mcica.on())      // every g-point its own sub-column: the band cloud optical depth is added in the cloudy cells only
            sample_clouds(mcica, blk, n_lay, n_gpt, n_bnd, ws.optical_props->get_band_lims_gpoint_gpu().ptr(), 0, [&](auto... common)
            {
                RRX_CALL(rrx_mcica_increment_1scalar, common..., ws.optical_props->get_tau().ptr(), ws.cloud_optical_props->get_tau().ptr(),
                         static_cast<unsigned char*>(nullptr));
            });

        if (switch_output_optical)
        {
            // (the reference scatters lev_source with n_lay rows, Radiation_solver.cu:520-523, which drops the last level
            //  and misplaces the others; lev_source has n_lev rows)
            Float* full_lay[2] = {tau.ptr(), lay_source.ptr()};
            const Float* sub_lay[2] = {ws.optical_props->get_tau().ptr(), ws.sources->get_lay_source().ptr()};
            Subset_kernels_cuda::scatter_(n_col, n_lay, n_gpt, n_in, col_s, 2, full_lay, sub_lay);
            Float* full_lev[1] = {lev_source.ptr()};
            const Float* sub_lev[1] = {ws.sources->get_lev_source().ptr()};
            Subset_kernels_cuda::scatter_(n_col, n_lev, n_gpt, n_in, col_s, 1, full_lev, sub_lev);
            Subset_kernels_cuda::get_from_subset(n_col, n_gpt, n_in, col_s, sfc_source.ptr(), ws.sources->get_sfc_source().ptr());
        }
        if (!switch_fluxes)
            continue;

        const int n_ang = n_gauss_angles;
        Array_gpu<Float,2> emis_s = blk.sub_last(emis_sfc, n_bnd);
        const Array_gpu<Float,2> no_inc_flux;
        if (plan.byband)
        {
            // band sums, band net and broadband fluxes from one solve
            Byband_block v(blk, out, {&ws.gpt_flux_up, &ws.gpt_flux_dn});
            rte_lw.rte_lw_byband(ws.optical_props, top_at_1, *ws.sources, emis_s, no_inc_flux, v.bnd[0], v.bnd[1], v.bnd[2], v.bb[0], v.bb[1]);
            v.finish(blk, out);
            continue;
        }
        // every other form of the LW solve of this block (jc: null = no Jacobian)
        auto solve_block = [&](Array_gpu<Float,3>& up, Array_gpu<Float,3>& dn, Array_gpu<Float,3>* jc)
        {
            const Optical_props_2str_gpu* cloud = cloud_2str ? ws.cloud_optical_props_2str.get() : nullptr;
            switch (plan.form)
            {
                case Lw_form::rescaled:   rte_lw.rte_lw_rescaled(ws.optical_props, top_at_1, *ws.sources, emis_s, no_inc_flux, cloud, up, dn); break;
                case Lw_form::two_stream: rte_lw.rte_lw_2stream(ws.optical_props, top_at_1, *ws.sources, emis_s, no_inc_flux, cloud, up, dn); break;
                case Lw_form::optimal:    // the secants of the k-distribution's fit
                    rte_lw.rte_lw_optimal(ws.optical_props, top_at_1, *ws.sources, emis_s, no_inc_flux, kdist_gpu->get_optimal_angle_fit_gpu(), up, dn, jc, n_ang);
                    break;
                default:                  // fixed Gauss angles: per g-point, or the fused fractions form with one or several angles
                    if (jc != nullptr) rte_lw.rte_lw(ws.optical_props, top_at_1, *ws.sources, emis_s, no_inc_flux, up, dn, *jc, n_ang);
                    else rte_lw.rte_lw(ws.optical_props, top_at_1, *ws.sources, emis_s, no_inc_flux, up, dn, n_ang);
            }
        };
        if (blk.whole && plan.broadband)
        {
            // one block in broadband mode: the solver writes the caller's flux arrays, the net flux follows in place (no block
            // workspace, no copies: Fluxes_broadband_gpu::reduce + get_from_subset of the general path are 7 passes over the fluxes)
            out.allocate_bb();
            Array_gpu<Float,3> up3(lw_flux_up.ptr(), {n_col, n_lev, 1}), dn3(lw_flux_dn.ptr(), {n_col, n_lev, 1});
            Array_gpu<Float,3> jac3(lw_flux_up_jac.ptr(), {n_col, n_lev, 1});      // (a view: not used without the Jacobian)
            solve_block(up3, dn3, plan.jac ? &jac3 : nullptr);
            Fluxes_kernels_cuda::net_broadband_precalc(n_col, n_lev, lw_flux_dn.ptr(), lw_flux_up.ptr(), lw_flux_net.ptr());
            continue;
        }
        solve_block(ws.gpt_flux_up, ws.gpt_flux_dn, plan.jac ? &ws.gpt_flux_up_jac : nullptr);
        if (plan.jac)
        {
            const Float* jac_blk = ws.gpt_flux_up_jac.ptr();
            if (!plan.broadband)
            {
                RRX_CALL(rrx_sum_broadband, n_in, n_lev, n_gpt, ws.gpt_flux_up_jac.ptr(), ws.flux_up_jac.ptr());
                jac_blk = ws.flux_up_jac.ptr();
            }
            Subset_kernels_cuda::get_from_subset(n_col, n_lev, n_in, col_s, lw_flux_up_jac.ptr(), jac_blk);
        }
        out.reduce_block(blk, switch_output_bnd_fluxes, ws.gpt_flux_up, ws.gpt_flux_dn, nullptr, ws.optical_props, top_at_1);
    }
}


// -------------------------------------------------------------------------------------------- shortwave
struct Radiation_solver_shortwave::Workspace
{
    int n_col = 0, n_lay = 0;
    bool broadband = false, byband = false;
    std::unique_ptr<Optical_props_arry_gpu> optical_props;
    std::unique_ptr<Optical_props_2str_gpu> cloud_optical_props, aerosol_optical_props;
    Array_gpu<Float,3> gpt_flux_up, gpt_flux_dn, gpt_flux_dn_dir;
};

Radiation_solver_shortwave::Radiation_solver_shortwave(
        const Gas_concs_gpu& gas_concs,
        const bool switch_cloud_optics,
        const bool switch_aerosol_optics,
        const std::string& file_name_gas,
        const std::string& file_name_cloud,
        const std::string& file_name_aerosol)
{
    this->kdist_gpu = std::make_unique<Gas_optics_rrtmgp_gpu>(load_and_init_gas_optics(gas_concs, file_name_gas));
    if (switch_cloud_optics)
        this->cloud_optics_gpu = std::make_unique<Cloud_optics_gpu>(load_and_init_cloud_optics(file_name_cloud));
    if (switch_aerosol_optics)
    {
        this->aerosol_optics_gpu = std::make_unique<Aerosol_optics_gpu>(load_and_init_aerosol_optics(file_name_aerosol));
        if (this->aerosol_optics_gpu->get_nband() != this->kdist_gpu->get_nband())
            throw std::runtime_error("aerosol optics tables and the shortwave k-distribution disagree in the number of bands");
    }
}

void Radiation_solver_shortwave::solve_gpu(
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
        Array_gpu<Float,3>& sw_bnd_flux_dn_dir, Array_gpu<Float,3>& sw_bnd_flux_net)
{
    (void)t_lev;
    const int n_col = p_lay.dim(1);
    const int n_lay = p_lay.dim(2);
    const int n_lev = p_lev.dim(2);
    const int n_gpt = this->kdist_gpu->get_ngpt();
    const int n_bnd = this->kdist_gpu->get_nband();
    const Bool top_at_1 = (vertical_ordering < 0) ? Bool(p_lay({1, 1}) < p_lay({1, n_lay})) : Bool(vertical_ordering == 1);
    if (switch_cloud_optics && !cloud_optics_gpu) throw std::runtime_error("cloud optics requested but no cloud coefficients loaded");
    if (switch_aerosol_optics && !aerosol_optics_gpu) throw std::runtime_error("aerosol optics requested but no aerosol coefficients loaded");
    const bool broadband = broadband_solvers && !switch_output_bnd_fluxes;
    // by-band solvers: the band sums come straight out of the fused solver (one slab per band in the block workspace)
    const bool byband = byband_solvers && switch_output_bnd_fluxes && switch_fluxes && n_bnd < n_gpt;
    if (mcica.on() && sunlit_columns)
        throw std::runtime_error("Radiation_solver_shortwave: cloud sampling (set_cloud_sampling) is not available with the sunlit-only "
                                 "solve (set_sunlit_columns): it does not carry the column identities");
    if (mcica.on()) mcica.check("Radiation_solver_shortwave", n_col, n_lay, switch_cloud_optics);
    const bool spherical = sph_alt != nullptr;
    if (spherical && (sph_alt->dim(1) != n_col || sph_alt->dim(2) != n_lay))
        throw std::runtime_error("Radiation_solver_shortwave: set_spherical_mu0: alt_lay is not (ncol, nlay)");
    if (spherical && sph_ref_alt != nullptr && sph_ref_alt->dim(1) != n_col)
        throw std::runtime_error("Radiation_solver_shortwave: set_spherical_mu0: ref_alt is not (ncol)");
    const Flux_outputs out{{{&sw_flux_up, &sw_flux_dn, &sw_flux_dn_dir, &sw_flux_net}, {&sw_bnd_flux_up, &sw_bnd_flux_dn, &sw_bnd_flux_dn_dir, &sw_bnd_flux_net}},
                           n_col, n_lev, n_bnd};

    // columns in another order / on a padded count: gather the inputs, solve, scatter the fluxes back (see the header)
    if (!reordered_call && !switch_output_optical && switch_fluxes)
    {
        Column_order co = column_order(column_sorting, sort_decided, column_padding, p_lev, top_at_1);
        if (sunlit_columns)
        {
            // sunlit-only: the solve runs on the columns with mu0 > 0; all sunlit: the plain order below, bit for bit
            Column_order day = sunlit_column_order(co, n_col, mu0, column_padding);
            if (day.n_keep < n_col) co = std::move(day);
            if (co.subset && co.n_keep == 0)
            {
                out.zeros(co, switch_output_bnd_fluxes);
                return;
            }
        }
        if (co.active())
        {
            const Gas_concs_gpu gases = gas_concs.gathered(co.perm, n_col, co.n_out);
            Aerosol_concs_gpu aerosols = aerosol_concs.gathered(co.perm, n_col, co.n_out);
            Array_gpu<Float,3> no3a, no3b, no3c; Array_gpu<Float,2> no2;
            Flux_arrays r = out.reordered(co.n_out, switch_output_bnd_fluxes);
            Guard guard(reordered_call);
            Sampling_reordered sampling(mcica, co);
            Altitudes_reordered altitudes(sph_alt, sph_ref_alt, co);
            this->solve_gpu(switch_fluxes, switch_cloud_optics, switch_aerosol_optics, switch_output_optical, switch_output_bnd_fluxes,
                            switch_delta_cloud, switch_delta_aerosol, gases,
                            co.in2(p_lay), co.in2(p_lev), co.in2(t_lay), co.in2(t_lev), co.in2(col_dry),
                            co.in_last(sfc_alb_dir), co.in_last(sfc_alb_dif), co.in1(tsi_scaling), co.in1(mu0),
                            co.in2(lwp), co.in2(iwp), co.in2(rel), co.in2(dei), co.in2(rh), aerosols,
                            no3a, no3b, no3c, no2, r.bb[0], r.bb[1], r.bb[2], r.bb[3], r.bnd[0], r.bnd[1], r.bnd[2], r.bnd[3]);
            out.from_reordered(co, r, switch_output_bnd_fluxes);
            return;
        }
    }

    auto prepare = [&](std::shared_ptr<Workspace>& ws, const int n)
    {
        if (!ws || ws->n_col != n || ws->n_lay != n_lay || ws->broadband != broadband || ws->byband != byband)
        {
            ws = std::make_shared<Workspace>();
            ws->n_col = n; ws->n_lay = n_lay; ws->broadband = broadband; ws->byband = byband;
            ws->optical_props = std::make_unique<Optical_props_2str_gpu>(n, n_lay, *kdist_gpu);
            const int ng = broadband ? 1 : (byband ? n_bnd : n_gpt);
            ws->gpt_flux_up.set_dims({n, n_lev, ng}); ws->gpt_flux_dn.set_dims({n, n_lev, ng}); ws->gpt_flux_dn_dir.set_dims({n, n_lev, ng});
        }
        if (switch_cloud_optics && !ws->cloud_optical_props)
            ws->cloud_optical_props = std::make_unique<Optical_props_2str_gpu>(n, n_lay, *cloud_optics_gpu);
        if (switch_aerosol_optics && !ws->aerosol_optical_props)
            ws->aerosol_optical_props = std::make_unique<Optical_props_2str_gpu>(n, n_lay, *aerosol_optics_gpu);
    };

    for (const auto& columns : column_blocks(n_col, std::max(1, n_col_block)))
    {
        const int col_s = columns.first, n_in = columns.second;
        std::shared_ptr<Workspace>& wsp = (n_in == std::min(n_col_block, n_col)) ? ws_block : ws_residual;
        prepare(wsp, n_in);
        Workspace& ws = *wsp;
        const Block blk(n_col, columns, gas_concs);
        Array_gpu<Float,2> p_lay_s = blk.sub2(p_lay, n_lay), t_lay_s = blk.sub2(t_lay, n_lay), p_lev_s = blk.sub2(p_lev, n_lev);
        Array_gpu<Float,2> col_dry_s = blk.col_dry(col_dry, p_lev_s, n_lay);

        // (cloud optics first: gas and cloud properties are combined inside gas_optics where the g-point arrays are stored --
        //  the add_to() of Radiation_solver.cu:788-791 folded into the producer)
        if (switch_cloud_optics)
        {
            // (delta_scale() of Radiation_solver.cu:785 rides along in the same kernel)
            cloud_optics_gpu->cloud_optics(blk.sub2(lwp, n_lay), blk.sub2(iwp, n_lay), blk.sub2(rel, n_lay), blk.sub2(dei, n_lay), *ws.cloud_optical_props,
                                           switch_delta_cloud);
        }
        Array_gpu<Float,2> toa_src_s({n_in, n_gpt});
        kdist_gpu->gas_optics(p_lay_s, p_lev_s, t_lay_s, blk.gases, ws.optical_props, toa_src_s, col_dry_s,
                              (switch_cloud_optics && !mcica.on()) ? ws.cloud_optical_props.get() : nullptr);
        if (mcica.on())      // every g-point its own sub-column: the band cloud tau / ssa / g are combined in the cloudy cells only
        {
            Optical_props_2str_gpu& op = dynamic_cast<Optical_props_2str_gpu&>(*ws.optical_props);
            // (get_g(): the clear gas optics' g == 0 is materialised here, the kernel reads and writes the array)
            sample_clouds(mcica, blk, n_lay, n_gpt, n_bnd, op.get_band_lims_gpoint_gpu().ptr(), 1, [&](auto... common)
            {
                RRX_CALL(rrx_mcica_increment_2stream, common..., op.get_tau().ptr(), op.get_ssa().ptr(), op.get_g().ptr(),
                         ws.cloud_optical_props->get_tau().ptr(), ws.cloud_optical_props->get_ssa().ptr(), ws.cloud_optical_props->get_g().ptr(),
                         static_cast<unsigned char*>(nullptr));
            });
        }
        Array_gpu<Float,1> tsi_s = blk.sub1(tsi_scaling);
        RRX_CALL(rrx_scaling_to_subset, n_in, n_gpt, toa_src_s.ptr(), tsi_s.ptr());

        if (switch_aerosol_optics)
        {
            // the block's own columns (the reference subsets (1, n_col) here, Radiation_solver.cu:796, which is only right for
            // a single block)
            Aerosol_concs_gpu aerosol_concs_subset(aerosol_concs, col_s, n_in);
            aerosol_optics_gpu->aerosol_optics(aerosol_concs_subset, blk.sub2(rh, n_lay), p_lev_s, *ws.aerosol_optical_props);
            if (switch_delta_aerosol)
                ws.aerosol_optical_props->delta_scale();
            add_to(dynamic_cast<Optical_props_2str_gpu&>(*ws.optical_props), *ws.aerosol_optical_props);
        }

        if (switch_output_optical)
        {
            Subset_kernels_cuda::get_from_subset(n_col, n_lay, n_gpt, n_in, col_s, tau.ptr(), ssa.ptr(), g.ptr(),
                    ws.optical_props->get_tau().ptr(), ws.optical_props->get_ssa().ptr(), ws.optical_props->get_g().ptr());
            Subset_kernels_cuda::get_from_subset(n_col, n_gpt, n_in, col_s, toa_src.ptr(), toa_src_s.ptr());
        }
        if (!switch_fluxes)
            continue;

        // set_spherical_mu0: the block's cosines layer by layer, from its mu0, its altitudes and its reference altitudes
        Array_gpu<Float,2> mu0_lay_s;
        if (spherical)
        {
            mu0_lay_s.set_dims({n_in, n_lay});
            const Array_gpu<Float,2> alt_s = blk.sub2(*sph_alt, n_lay);
            const Array_gpu<Float,1> ref_s = (sph_ref_alt != nullptr) ? blk.sub1(*sph_ref_alt) : Array_gpu<Float,1>();
            const Array_gpu<Float,1> mu0_s = blk.sub1(mu0);
            RRX_CALL(rrx_zenith_angle_spherical_correction, n_in, n_lay, sph_ref_alt != nullptr ? ref_s.ptr() : nullptr, mu0_s.ptr(), alt_s.ptr(),
                     sph_radius, mu0_lay_s.ptr());
        }
        const Array_gpu<Float,2> no_inc_flux;
        // (the solvers take mu0 per column or, spherical, per column and layer)
        auto with_mu0 = [&](auto&& rte) { if (spherical) rte(mu0_lay_s); else rte(blk.sub1(mu0)); };
        if (byband)
        {
            // band sums, band net and broadband fluxes from one solve
            Byband_block v(blk, out, {&ws.gpt_flux_up, &ws.gpt_flux_dn, &ws.gpt_flux_dn_dir});
            with_mu0([&](const auto& mu) {
                rte_sw.rte_sw_byband(ws.optical_props, top_at_1, mu, toa_src_s, blk.sub_last(sfc_alb_dir, n_bnd), blk.sub_last(sfc_alb_dif, n_bnd),
                                     no_inc_flux, v.bnd[0], v.bnd[1], v.bnd[2], v.bnd[3], v.bb[0], v.bb[1], v.bb[2]); });
            v.finish(blk, out);
            continue;
        }
        auto solve = [&](Array_gpu<Float,3>& up3, Array_gpu<Float,3>& dn3, Array_gpu<Float,3>& dir3)
        {
            with_mu0([&](const auto& mu) {
                rte_sw.rte_sw(ws.optical_props, top_at_1, mu, toa_src_s, blk.sub_last(sfc_alb_dir, n_bnd), blk.sub_last(sfc_alb_dif, n_bnd), no_inc_flux, up3, dn3, dir3); });
        };
        if (blk.whole && broadband)
        {
            // one block in broadband mode: the solver writes the caller's flux arrays, the net flux follows in place
            out.allocate_bb();
            Array_gpu<Float,3> up3(sw_flux_up.ptr(), {n_col, n_lev, 1}), dn3(sw_flux_dn.ptr(), {n_col, n_lev, 1}), dir3(sw_flux_dn_dir.ptr(), {n_col, n_lev, 1});
            solve(up3, dn3, dir3);
            Fluxes_kernels_cuda::net_broadband_precalc(n_col, n_lev, sw_flux_dn.ptr(), sw_flux_up.ptr(), sw_flux_net.ptr());
            continue;
        }
        solve(ws.gpt_flux_up, ws.gpt_flux_dn, ws.gpt_flux_dn_dir);
        out.reduce_block(blk, switch_output_bnd_fluxes, ws.gpt_flux_up, ws.gpt_flux_dn, &ws.gpt_flux_dn_dir, ws.optical_props, top_at_1);
    }
}

void Radiation_solver_shortwave::set_sunlit_columns(const bool b) { sunlit_columns = b; }

void Radiation_solver_shortwave::set_spherical_mu0(const Array_gpu<Float,2>* alt_lay, const Array_gpu<Float,1>* ref_alt, const Float planet_radius)
{
    if (alt_lay == nullptr && ref_alt != nullptr)
        throw std::runtime_error("Radiation_solver_shortwave::set_spherical_mu0: ref_alt without alt_lay");
    if (!(planet_radius > Float(0.)))
        throw std::runtime_error("Radiation_solver_shortwave::set_spherical_mu0: planet_radius must be positive");
    sph_alt = alt_lay; sph_ref_alt = (alt_lay != nullptr) ? ref_alt : nullptr; sph_radius = planet_radius;
}

void Radiation_solver_shortwave::set_cloud_sampling(const Array_gpu<Float,2>* cloud_frac, const int overlap, const Array_gpu<Float,2>* overlap_param,
                                                   const uint64_t seed, const int col_offset)
{ mcica.set("Radiation_solver_shortwave", cloud_frac, overlap, overlap_param, seed, col_offset); }

