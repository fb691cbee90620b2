// Self-checks of the host classes that need a device but no input files; exported from librte_rrtmgp_hip.so for the GPU
// tests (tests/test_gpu_host_classes.py). Each returns 0 on success and a non-zero code naming the failed check.
#include <cmath>
#include <vector>
#include <cstdio>
#include <cstring>
#include <string>
#include <memory>
#include "Array.h"
#include "Optical_props.h"
#include "Source_functions.h"
#include "Rte_lw.h"
#include "Rte_sw.h"
#include "Netcdf_interface.h"
#include "Radiation_solver.h"

namespace
{
    Optical_props_gpu two_bands()
    {
        Array<Float,2> wvn({2, 2});
        wvn({1, 1}) = 10.; wvn({2, 1}) = 250.; wvn({1, 2}) = 250.; wvn({2, 2}) = 500.;
        Array<int,2> lims({2, 2});
        lims({1, 1}) = 1; lims({2, 1}) = 3; lims({1, 2}) = 4; lims({2, 2}) = 6;
        return Optical_props_gpu(wvn, lims);
    }

    // ---- rrx_host_selftest_rte: the smallest problem with every extent distinct, 5 columns x 4 layers x 6 g-points in 2 bands, every
    // input from a formula.
    constexpr int NCOL = 5, NLAY = 4, NLEV = NLAY + 1, NGPT = 6, NBND = 2;

    // element i = lo + step * ((7 i) mod m): positive, bounded by lo + step (m-1), no two neighbours alike
    template<int N> Array_gpu<Float,N> filled(const std::array<int,N>& dims, const double lo, const double step, const int m)
    {
        Array<Float,N> h(dims);
        for (int i=0; i<h.size(); ++i) h.ptr()[i] = Float(lo + step*double((7*i) % m));
        return Array_gpu<Float,N>(h);
    }

    // an output array, filled with a value no solver writes: two outputs that a call left alone do not compare equal by accident
    Array_gpu<Float,3> flux(const int n3, const Float mark) { Array_gpu<Float,3> a({NCOL, NLEV, n3}); a.fill(mark); return a; }

    template<int N> bool same(const Array_gpu<Float,N>& a, const Array_gpu<Float,N>& b)
    {
        const Array<Float,N> ha(a), hb(b);
        return ha.size() == hb.size() && ha.size() > 0 && std::memcmp(ha.ptr(), hb.ptr(), size_t(ha.size())*sizeof(Float)) == 0;
    }

    struct Rte_problem
    {
        Optical_props_gpu bands = two_bands();
        std::unique_ptr<Optical_props_arry_gpu> lw = std::make_unique<Optical_props_1scl_gpu>(NCOL, NLAY, bands);
        std::unique_ptr<Optical_props_arry_gpu> sw = std::make_unique<Optical_props_2str_gpu>(NCOL, NLAY, bands);
        Source_func_lw_gpu lite{NCOL, NLAY, bands};      // the Planck-lite state, set by hand
        Source_func_lw_gpu full{NCOL, NLAY, bands};      // lay_source / lev_source materialised from the same numbers
        Optical_props_2str_gpu cloud{NCOL, NLAY, Optical_props_gpu(bands.get_band_lims_wavenumber())};       // by band
        Optical_props_2str_gpu cloud_bad{NCOL, NLAY + 1, Optical_props_gpu(bands.get_band_lims_wavenumber())};
        Array_gpu<Float,2> sfc_emis = filled<2>({NBND, NCOL}, 0.90, 0.01, 9);
        Array_gpu<Float,2> inc_lw = filled<2>({NCOL, NGPT}, 2.0, 0.5, 11);
        Array_gpu<Float,2> none;
        Array_gpu<Float,2> fit = filled<2>({2, NBND}, 0.2, 0.7, 3);             // D = fit1 exp(-S) + fit2: 0.2 .. 1.6 each
        Array_gpu<Float,2> fit_bad = filled<2>({2, NBND + 1}, 0.2, 0.7, 3);
        Array_gpu<Float,2> Ds = Array_gpu<Float,2>({NCOL, NGPT});
        Array_gpu<Float,2> Ds_bad = Array_gpu<Float,2>({NCOL, NBND});
        Array_gpu<Float,1> mu0 = filled<1>({NCOL}, 0.3, 0.1, 6);
        Array_gpu<Float,2> mu0_lay = filled<2>({NCOL, NLAY}, 0.25, 0.05, 13);
        Array_gpu<Float,2> mu0_lay_bad = filled<2>({NCOL, NLAY + 1}, 0.25, 0.05, 13);
        Array_gpu<Float,2> inc_dir = filled<2>({NCOL, NGPT}, 20., 3., 7);
        Array_gpu<Float,2> inc_dif = filled<2>({NCOL, NGPT}, 1., 0.25, 5);
        Array_gpu<Float,2> alb_dir = filled<2>({NBND, NCOL}, 0.05, 0.03, 8);
        Array_gpu<Float,2> alb_dif = filled<2>({NBND, NCOL}, 0.07, 0.02, 9);

        Rte_problem()
        {
            lw->get_tau() = filled<3>({NCOL, NLAY, NGPT}, 0.02, 0.11, 17);
            sw->get_tau() = filled<3>({NCOL, NLAY, NGPT}, 0.05, 0.07, 19);
            sw->get_ssa() = filled<3>({NCOL, NLAY, NGPT}, 0.10, 0.04, 21);
            sw->get_g() = filled<3>({NCOL, NLAY, NGPT}, 0.00, 0.03, 23);
            cloud.get_tau() = filled<3>({NCOL, NLAY, NBND}, 0.0, 0.3, 5);
            cloud.get_ssa() = filled<3>({NCOL, NLAY, NBND}, 0.3, 0.05, 11);
            cloud.get_g() = filled<3>({NCOL, NLAY, NBND}, 0.6, 0.02, 13);
            for (Source_func_lw_gpu* s : {&lite, &full})
            {
                s->get_planck_frac() = filled<3>({NCOL, NLAY, NGPT}, 0.05, 0.02, 23);
                s->get_planck_lay() = filled<3>({NCOL, NLAY, NBND}, 30., 1.5, 13);
                s->get_planck_lev() = filled<3>({NCOL, NLEV, NBND}, 29., 1.5, 17);
                s->get_sfc_source() = filled<2>({NCOL, NGPT}, 4., 0.3, 11);
                s->get_sfc_source_jac() = filled<2>({NCOL, NGPT}, 0.05, 0.004, 13);
                s->set_fractions_valid(true);
            }
            full.get_lay_source();                       // materialises both arrays; full holds no fractions from here on
            Ds.fill(Float(1./0.6096748751));             // the secant of the one-angle Gauss rule
        }
        // the Planck-lite sources: a per-g-point solve on them would have materialised them, so the state is stated before every use
        const Source_func_lw_gpu& L() { lite.set_fractions_valid(true); return lite; }
    };

    // (a) equalities in bits between routes of the classes; each for both vertical orderings, with and without incident diffuse flux.
    // Returns the empty string, or what differed.
    std::string rte_equality(Rte_problem& p, const int which)
    {
        Rte_lw_gpu lw_a, lw_b; Rte_sw_gpu sw_a, sw_b;
        Array_gpu<Float,3> no3; Array_gpu<Float,2> no_up, no_dn, no_dir;
        for (int combo=0; combo<4; ++combo)
        {
            const Bool top_at_1 = Bool(combo & 1);
            const Array_gpu<Float,2>& inc = (combo & 2) ? p.inc_lw : p.none;
            const Array_gpu<Float,2>& inc_dif = (combo & 2) ? p.inc_dif : p.none;
            const std::string where = std::string(" (top_at_1 ") + (top_at_1 ? "1" : "0") + ((combo & 2) ? ", inc_flux)" : ", no inc_flux)");
            bool ok = true;
            switch (which)
            {
                case 0: case 1: case 2: case 3:
                {
                    // rte_lw_Ds with the Gauss secant everywhere = rte_lw with one angle: broadband on Planck-lite sources (0, 1) and
                    // per g-point (2, 3), without (0, 2) and with (1, 3) the Jacobian
                    const bool jac = which & 1;
                    const int n3 = which < 2 ? 1 : NGPT;
                    Array_gpu<Float,3> up_a = flux(n3, -1), dn_a = flux(n3, -2), jac_a = flux(n3, -3);
                    Array_gpu<Float,3> up_b = flux(n3, -4), dn_b = flux(n3, -5), jac_b = flux(n3, -6);
                    const Source_func_lw_gpu& s = which < 2 ? p.L() : p.full;
                    if (jac) lw_a.rte_lw(p.lw, top_at_1, s, p.sfc_emis, inc, up_a, dn_a, jac_a, 1);
                    else     lw_a.rte_lw(p.lw, top_at_1, s, p.sfc_emis, inc, up_a, dn_a, 1);
                    lw_b.rte_lw_Ds(p.lw, top_at_1, which < 2 ? p.L() : p.full, p.sfc_emis, inc, p.Ds, up_b, dn_b, jac ? &jac_b : nullptr, 1);
                    ok = same(up_a, up_b) && same(dn_a, dn_b) && (!jac || same(jac_a, jac_b));
                    break;
                }
                case 4:
                {
                    // rte_lw on arrays with one slab per band = bnd_flux_up/dn of rte_lw_byband
                    Array_gpu<Float,3> up_a = flux(NBND, -1), dn_a = flux(NBND, -2), up_b = flux(NBND, -4), dn_b = flux(NBND, -5);
                    lw_a.rte_lw(p.lw, top_at_1, p.L(), p.sfc_emis, inc, up_a, dn_a, 1);
                    lw_b.rte_lw_byband(p.lw, top_at_1, p.L(), p.sfc_emis, inc, up_b, dn_b, no3, no_up, no_dn);
                    ok = same(up_a, up_b) && same(dn_a, dn_b);
                    break;
                }
                case 5: case 6:
                {
                    // the same for rte_sw against rte_sw_byband, mu0 (ncol) and mu0 (ncol, nlay)
                    Array_gpu<Float,3> up_a = flux(NBND, -1), dn_a = flux(NBND, -2), dir_a = flux(NBND, -3);
                    Array_gpu<Float,3> up_b = flux(NBND, -4), dn_b = flux(NBND, -5), dir_b = flux(NBND, -6);
                    if (which == 5)
                    {
                        sw_a.rte_sw(p.sw, top_at_1, p.mu0, p.inc_dir, p.alb_dir, p.alb_dif, inc_dif, up_a, dn_a, dir_a);
                        sw_b.rte_sw_byband(p.sw, top_at_1, p.mu0, p.inc_dir, p.alb_dir, p.alb_dif, inc_dif, up_b, dn_b, dir_b, no3, no_up, no_dn, no_dir);
                    }
                    else
                    {
                        sw_a.rte_sw(p.sw, top_at_1, p.mu0_lay, p.inc_dir, p.alb_dir, p.alb_dif, inc_dif, up_a, dn_a, dir_a);
                        sw_b.rte_sw_byband(p.sw, top_at_1, p.mu0_lay, p.inc_dir, p.alb_dir, p.alb_dif, inc_dif, up_b, dn_b, dir_b, no3, no_up, no_dn, no_dir);
                    }
                    ok = same(up_a, up_b) && same(dn_a, dn_b) && same(dir_a, dir_b);
                    break;
                }
                case 7:
                {
                    // broadband arrays with a Jacobian on sources without fractions (the jac_bb path of the general solver): the
                    // per-g-point call's Jacobian, added over the g-points in order from zero
                    Array_gpu<Float,3> up_a = flux(1, -1), dn_a = flux(1, -2), jac_a = flux(1, -3);
                    Array_gpu<Float,3> up_b = flux(NGPT, -4), dn_b = flux(NGPT, -5), jac_b = flux(NGPT, -6);
                    lw_a.rte_lw(p.lw, top_at_1, p.full, p.sfc_emis, inc, up_a, dn_a, jac_a, 1);
                    lw_b.rte_lw(p.lw, top_at_1, p.full, p.sfc_emis, inc, up_b, dn_b, jac_b, 1);
                    const Array<Float,3> bb(jac_a), gpt(jac_b);
                    for (int i=0; i<NCOL*NLEV; ++i)
                    {
                        Float sum = Float(0.);
                        for (int igpt=0; igpt<NGPT; ++igpt) sum += gpt.ptr()[igpt*NCOL*NLEV + i];
                        ok = ok && std::memcmp(&sum, &bb.ptr()[i], sizeof(Float)) == 0;
                    }
                    break;
                }
                case 8: case 9:
                {
                    // rte_lw_optimal on per-g-point arrays = rte_lw_Ds on the output of rrx_lw_optimal_secants for the same tau and fit
                    const bool jac = which == 9;
                    Array_gpu<Float,3> up_a = flux(NGPT, -1), dn_a = flux(NGPT, -2), jac_a = flux(NGPT, -3);
                    Array_gpu<Float,3> up_b = flux(NGPT, -4), dn_b = flux(NGPT, -5), jac_b = flux(NGPT, -6);
                    Array_gpu<Float,2> secants({NCOL, NGPT});
                    RRX_CALL(rrx_lw_optimal_secants, NCOL, NLAY, NGPT, NBND, p.lw->get_gpoint_bands_gpu().ptr(), p.fit.ptr(),
                             p.lw->get_tau().ptr(), secants.ptr());
                    lw_a.rte_lw_optimal(p.lw, top_at_1, p.full, p.sfc_emis, inc, p.fit, up_a, dn_a, jac ? &jac_a : nullptr, 1);
                    lw_b.rte_lw_Ds(p.lw, top_at_1, p.full, p.sfc_emis, inc, secants, up_b, dn_b, jac ? &jac_b : nullptr, 1);
                    ok = same(up_a, up_b) && same(dn_a, dn_b) && (!jac || same(jac_a, jac_b));
                    break;
                }
                default: return "no such equality";
            }
            if (!ok) return "equality " + std::to_string(which) + " does not hold" + where;
        }
        return "";
    }

    // (b) one call per refusal of Rte.cpp (100..121: exactly one bad argument) and calls that break two checks at once, which hold the
    // order of the checks (122..). Every one of them throws before anything is launched.
    void rte_refused_call(Rte_problem& p, const int which)
    {
        Rte_lw_gpu lw; Rte_sw_gpu sw;
        const Bool top = Bool(1);
        Array_gpu<Float,3> bb_up = flux(1, 0), bb_dn = flux(1, 0), bb_jac = flux(1, 0);
        Array_gpu<Float,3> g_up = flux(NGPT, 0), g_dn = flux(NGPT, 0), g_dir = flux(NGPT, 0), g_jac = flux(NGPT, 0);
        Array_gpu<Float,3> b_up = flux(NBND, 0), b_dn = flux(NBND, 0), b_dir = flux(NBND, 0), b_jac = flux(NBND, 0);
        Array_gpu<Float,3> no3; Array_gpu<Float,2> no_up, no_dn, no_dir;
        const auto sw_byband_lay = [&](const Array_gpu<Float,2>& mu0, Array_gpu<Float,3>& up, Array_gpu<Float,3>& dn, Array_gpu<Float,3>& dir)
        { sw.rte_sw_byband(p.sw, top, mu0, p.inc_dir, p.alb_dir, p.alb_dif, p.none, up, dn, dir, no3, no_up, no_dn, no_dir); };
        switch (which)
        {
            case 100: lw.rte_lw(p.lw, top, p.L(), p.sfc_emis, p.none, b_up, b_dn, b_jac, 1); break;
            case 101: lw.rte_lw(p.lw, top, p.L(), p.sfc_emis, p.none, bb_up, bb_dn, g_jac, 1); break;
            case 102: lw.rte_lw_optimal(p.lw, top, p.L(), p.sfc_emis, p.none, p.fit, bb_up, bb_dn, nullptr, 2); break;
            case 103: lw.rte_lw_optimal(p.lw, top, p.L(), p.sfc_emis, p.none, p.fit_bad, bb_up, bb_dn, nullptr, 1); break;
            case 104: lw.rte_lw_Ds(p.lw, top, p.L(), p.sfc_emis, p.none, p.Ds, bb_up, bb_dn, nullptr, 2); break;
            case 105: lw.rte_lw_Ds(p.lw, top, p.L(), p.sfc_emis, p.none, p.Ds_bad, bb_up, bb_dn, nullptr, 1); break;
            case 106: lw.rte_lw(p.lw, top, p.L(), p.sfc_emis, p.none, bb_up, bb_dn, 5); break;
            case 107: lw.rte_lw_Ds(p.lw, top, p.L(), p.sfc_emis, p.none, p.Ds, b_up, b_dn, nullptr, 1); break;
            case 108: lw.rte_lw_Ds(p.lw, top, p.L(), p.sfc_emis, p.none, p.Ds, bb_up, bb_dn, &g_jac, 1); break;
            case 109: lw.rte_lw(p.lw, top, p.L(), p.sfc_emis, p.none, b_up, b_dn, 2); break;
            case 110: lw.rte_lw_byband(p.lw, top, p.full, p.sfc_emis, p.none, b_up, b_dn, no3, no_up, no_dn); break;
            case 111: lw.rte_lw_byband(p.lw, top, p.L(), p.sfc_emis, p.none, g_up, g_dn, no3, no_up, no_dn); break;
            case 112: lw.rte_lw_2stream(p.lw, top, p.full, p.sfc_emis, p.none, &p.cloud, bb_up, bb_dn); break;
            case 113: lw.rte_lw_2stream(p.lw, top, p.L(), p.sfc_emis, p.none, &p.cloud, g_up, g_dn); break;
            case 114: lw.rte_lw_2stream(p.lw, top, p.L(), p.sfc_emis, p.none, &p.cloud_bad, bb_up, bb_dn); break;
            case 115: lw.rte_lw_rescaled(p.lw, top, p.full, p.sfc_emis, p.none, &p.cloud, bb_up, bb_dn); break;
            case 116: lw.rte_lw_rescaled(p.lw, top, p.L(), p.sfc_emis, p.none, &p.cloud, g_up, g_dn); break;
            case 117: lw.rte_lw_rescaled(p.lw, top, p.L(), p.sfc_emis, p.none, &p.cloud_bad, bb_up, bb_dn); break;
            case 118: sw.rte_sw_byband(p.sw, top, p.mu0, p.inc_dir, p.alb_dir, p.alb_dif, p.none, g_up, g_dn, g_dir, no3, no_up, no_dn, no_dir); break;
            case 119: sw.rte_sw(p.sw, top, p.mu0_lay_bad, p.inc_dir, p.alb_dir, p.alb_dif, p.none, g_up, g_dn, g_dir); break;
            case 120: sw_byband_lay(p.mu0_lay_bad, b_up, b_dn, b_dir); break;
            case 121: sw_byband_lay(p.mu0_lay, g_up, g_dn, g_dir); break;
            // two checks broken at once: the first of them speaks
            case 122: lw.rte_lw(p.lw, top, p.L(), p.sfc_emis, p.none, b_up, b_dn, g_jac, 1); break;               // by-band, Jacobian shape
            case 123: lw.rte_lw(p.lw, top, p.L(), p.sfc_emis, p.none, bb_up, bb_dn, g_jac, 5); break;             // Jacobian shape, angle count
            case 124: lw.rte_lw_optimal(p.lw, top, p.L(), p.sfc_emis, p.none, p.fit_bad, bb_up, bb_dn, nullptr, 2); break;
            case 125: lw.rte_lw_Ds(p.lw, top, p.L(), p.sfc_emis, p.none, p.Ds_bad, bb_up, bb_dn, nullptr, 2); break;
            case 126: lw.rte_lw(p.lw, top, p.L(), p.sfc_emis, p.none, b_up, b_dn, 5); break;                      // angle count, by-band angles
            case 127: lw.rte_lw_Ds(p.lw, top, p.L(), p.sfc_emis, p.none, p.Ds, b_up, b_dn, &g_jac, 1); break;     // by-band, Jacobian shape
            case 128: lw.rte_lw_byband(p.lw, top, p.full, p.sfc_emis, p.none, g_up, g_dn, no3, no_up, no_dn); break;
            case 129: lw.rte_lw_2stream(p.lw, top, p.full, p.sfc_emis, p.none, &p.cloud_bad, g_up, g_dn); break;
            case 130: lw.rte_lw_2stream(p.lw, top, p.L(), p.sfc_emis, p.none, &p.cloud_bad, g_up, g_dn); break;
            case 131: lw.rte_lw_rescaled(p.lw, top, p.full, p.sfc_emis, p.none, &p.cloud_bad, g_up, g_dn); break;
            case 132: lw.rte_lw_rescaled(p.lw, top, p.L(), p.sfc_emis, p.none, &p.cloud_bad, g_up, g_dn); break;
            case 133: sw_byband_lay(p.mu0_lay_bad, g_up, g_dn, g_dir); break;                                      // mu0 shape, band slabs
            // by-band flux arrays leave rte_lw / rte_sw before their own checks: the by-band method's refusals speak
            case 134: sw.rte_sw(p.sw, top, p.mu0_lay_bad, p.inc_dir, p.alb_dir, p.alb_dif, p.none, b_up, b_dn, b_dir); break;
            case 135: lw.rte_lw(p.lw, top, p.full, p.sfc_emis, p.none, b_up, b_dn, 1); break;
            case 136: lw.rte_lw_optimal(p.lw, top, p.L(), p.sfc_emis, p.none, p.fit, b_up, b_dn, nullptr, 1); break;
            default: throw std::runtime_error("no such refusal");
        }
    }
}

extern "C"
{
// Optical_props_2str_gpu::delta_scale() on gas-only optical properties whose asymmetry is held in the lazy "g == 0"
// state (what the SW gas optics leave behind): the result must be the identity on tau and ssa, g must read back as
// zeros, and the stale contents of the g array must never reach the kernel (reference semantics with g = 0:
// /root/reference/src_kernels_cuda/optical_props_kernels.cu:140-161).
int rrx_host_selftest_delta_scale_gzero(void)
{
    try
    {
        const int ncol = 5, nlay = 4;
        Optical_props_2str_gpu op(ncol, nlay, two_bands());
        const int n = ncol*nlay*op.get_ngpt();
        Array<Float,3> tau({ncol, nlay, op.get_ngpt()}), ssa({ncol, nlay, op.get_ngpt()});
        for (int i=0; i<n; ++i) { tau.ptr()[i] = Float(0.01)*(i+1); ssa.ptr()[i] = Float(1.)/(i+2); }
        op.get_tau().set_data(tau); op.get_ssa().set_data(ssa);
        op.get_g().fill(Float(0.7));        // stale values of an earlier use of the workspace (e.g. cloud-incremented g)
        op.set_g_zero();
        if (op.get_g_or_null() != nullptr) return 1;
        op.delta_scale();
        Array<Float,3> t2(op.get_tau()), w2(op.get_ssa());
        for (int i=0; i<n; ++i)
            if (t2.ptr()[i] != tau.ptr()[i] || w2.ptr()[i] != ssa.ptr()[i]) return 2;
        if (op.get_g_or_null() != nullptr) return 3;               // still lazy: nothing materialised, nothing read
        Array<Float,3> g2(op.get_g());                              // first real access fills zeros
        for (int i=0; i<n; ++i) if (g2.ptr()[i] != Float(0.)) return 4;
        // and with a materialised g the kernel runs: f = g^2, tau' = tau (1 - ssa f)
        op.get_g().fill(Float(0.5));
        op.delta_scale();
        Array<Float,3> t3(op.get_tau());
        for (int i=0; i<n; ++i)
        {
            const Float want = tau.ptr()[i] * (Float(1.) - ssa.ptr()[i]*Float(0.25));
            if (std::abs(t3.ptr()[i] - want) > Float(1e-6)*std::abs(want)) return 5;
        }
        return 0;
    }
    catch (const std::exception&) { return 100; }
}

// Rte_lw_gpu / Rte_sw_gpu (host/src/Rte.cpp) on a 5 x 4 x 6 problem set up by hand, for tests/test_gpu_host_classes.py. which < 100:
// an equality in bits between two routes of the classes; 0 when it holds, 1 with the place in msg when it does not. which >= 100: a
// call that Rte.cpp refuses; -1 with what() in msg (which is also what any other exception gives), 0 when the call went through.
int rrx_host_selftest_rte(const int which, char* msg, const int msglen)
{
    try
    {
        Rte_problem p;
        if (which >= 100) { rte_refused_call(p, which); return 0; }
        const std::string diff = rte_equality(p, which);
        std::snprintf(msg, size_t(msglen), "%s", diff.c_str());
        return diff.empty() ? 0 : 1;
    }
    catch (const std::exception& e) { std::snprintf(msg, size_t(msglen), "%s", e.what()); return -1; }
}

// lw_solve_plan() of Radiation_solver.cpp for tests/test_host_lw_options.py; no device involved. flags, from bit 0: broadband_solvers,
// byband_solvers, jacobian, optimal_angles, lw_scattering, lw_rescaling, cloud sampling, switch_fluxes, switch_output_bnd_fluxes,
// switch_cloud_optics, n_bnd < n_gpt; bits 11.. hold n_gauss_angles. Returns broadband | byband << 1 | jac << 2 | cloud_to_solver << 3 |
// form << 4 (Lw_form in the order of its declaration), or -1 with the refusal in msg.
int rrx_host_selftest_lw_plan(const unsigned flags, char* msg, const int msglen)
{
    const auto bit = [flags](const int i) { return ((flags >> i) & 1u) != 0; };
    Lw_solve_options o;
    o.broadband_solvers = bit(0); o.byband_solvers = bit(1); o.jacobian = bit(2); o.optimal_angles = bit(3); o.lw_scattering = bit(4);
    o.lw_rescaling = bit(5); o.cloud_sampling = bit(6); o.switch_fluxes = bit(7); o.switch_output_bnd_fluxes = bit(8);
    o.switch_cloud_optics = bit(9); o.fewer_bands_than_gpoints = bit(10); o.n_gauss_angles = int(flags >> 11);
    try
    {
        const Lw_solve_plan p = lw_solve_plan(o);
        return int(p.broadband) | int(p.byband) << 1 | int(p.jac) << 2 | int(p.cloud_to_solver) << 3 | int(p.form) << 4;
    }
    catch (const std::exception& e) { std::snprintf(msg, size_t(msglen), "%s", e.what()); return -1; }
}

// Any supported file (NetCDF-4 or RRXB, recognised by its first bytes) rewritten in the other format: "rrxb" or "netcdf4".
int rrx_host_netcdf_convert(const char* in_path, const char* out_path, const char* format)
{
    try
    {
        Netcdf_file in(in_path, Netcdf_mode::Read);
        Netcdf_file out(out_path, Netcdf_mode::Create);
        out.set_output_format(format);
        out.copy_contents_of(in);
        out.sync();
        return 0;
    }
    catch (const std::exception& e) { std::fprintf(stderr, "rrx_host_netcdf_convert: %s\n", e.what()); return 1; }
}

// String attribute of a variable of a NetCDF-4 or classic NetCDF file (e.g. "units"); returns the length, -1 when absent or on error.
int rrx_host_netcdf_get_attr(const char* path, const char* var, const char* attr, char* buf, int buflen)
{
    if (rrx_cdf::version(path) != 0)                     // classic NetCDF
    {
        try
        {
            const std::string v = rrx_cdf::get_text_attr(path, var, attr);
            if (v.empty() || int(v.size()) >= buflen) return -1;
            std::memcpy(buf, v.c_str(), v.size() + 1);
            return int(v.size());
        }
        catch (const std::exception& e) { std::fprintf(stderr, "rrx_host_netcdf_get_attr: %s\n", e.what()); return -1; }
    }
#ifdef RRX_HAVE_HDF5_HEADERS
    try
    {
        const std::string v = rrx_h5::get_string_attr(path, var, attr);
        if (v.empty() || int(v.size()) >= buflen) return -1;
        std::memcpy(buf, v.c_str(), v.size() + 1);
        return int(v.size());
    }
    catch (const std::exception& e) { std::fprintf(stderr, "rrx_host_netcdf_get_attr: %s\n", e.what()); return -1; }
#else
    (void)path; (void)var; (void)attr; (void)buf; (void)buflen; return -1;
#endif
}

int rrx_host_netcdf_put_attr(const char* path, const char* var, const char* attr, const char* value)
{
#ifdef RRX_HAVE_HDF5_HEADERS
    try { rrx_h5::put_string_attr(path, var, attr, value); return 0; }
    catch (const std::exception& e) { std::fprintf(stderr, "rrx_host_netcdf_put_attr: %s\n", e.what()); return 1; }
#else
    (void)path; (void)var; (void)attr; (void)value; return 1;
#endif
}

// NetCDF-4 round trip through the HDF5 backend: dimensions, dimension order of each variable, f64 / f32 / i32 / char data,
// a scalar, a coordinate variable; no device involved.
int rrx_host_selftest_netcdf4(const char* dir)
{
    try
    {
        const std::string path = std::string(dir) + "/roundtrip.nc";
        std::vector<double> a(2*3*4); for (size_t i=0; i<a.size(); ++i) a[i] = 0.5*double(i) - 3.25;
        std::vector<float> b(4); for (size_t i=0; i<b.size(); ++i) b[i] = 1.5f*float(i);
        std::vector<int> c(3*2); for (size_t i=0; i<c.size(); ++i) c[i] = int(i)*7 - 5;
        const std::string names = "h2o     co2     o3      ";
        {
            Netcdf_file f(path, Netcdf_mode::Create);
            f.set_output_format("netcdf4");
            f.add_dimension("lay", 2); f.add_dimension("y", 3); f.add_dimension("x", 4); f.add_dimension("pair", 2);
            f.add_dimension("absorber", 3); f.add_dimension("string_len", 8);
            f.add_variable<double>("p_lay", {"lay", "y", "x"}).insert(a, {0, 0, 0});
            f.add_variable<float>("x", {"x"}).insert(b, {0});                                   // coordinate variable
            f.add_variable<int>("limits", {"y", "pair"}).insert(c, {0, 0});
            f.add_variable<char>("gas_names", {"absorber", "string_len"}).insert(std::vector<char>(names.begin(), names.end()), {0, 0});
            f.add_variable<double>("tsi_default").insert(1360.85, {});
        }
        FILE* fp = std::fopen(path.c_str(), "rb");
        unsigned char magic[4] = {0};
        if (!fp || std::fread(magic, 1, 4, fp) != 4 || magic[1] != 'H' || magic[2] != 'D' || magic[3] != 'F') return 1;
        std::fclose(fp);
        Netcdf_file r(path, Netcdf_mode::Read);
        if (r.get_dimension_size("lay") != 2 || r.get_dimension_size("y") != 3 || r.get_dimension_size("x") != 4 || r.get_dimension_size("string_len") != 8) return 2;
        const auto d = r.get_variable_dimensions("p_lay");
        if (d.size() != 3 || d.at("lay") != 2 || d.at("y") != 3 || d.at("x") != 4) return 3;
        if (r.get_variable<double>("p_lay", {2, 3, 4}) != a) return 4;
        if (r.get_variable<float>("x", {4}) != b) return 5;
        if (r.get_variable<int>("limits", {3, 2}) != c) return 6;
        const std::vector<char> g = r.get_variable<char>("gas_names", {3, 8});
        if (std::string(g.begin(), g.end()) != names) return 7;
        if (r.get_variable<double>("tsi_default") != 1360.85) return 8;
        if (!r.variable_exists("limits") || r.variable_exists("nope")) return 9;
        if (r.get_variable<float>("p_lay", {2, 3, 4})[5] != float(a[5])) return 10;              // type conversion on read
        return 0;
    }
    catch (const std::exception& e) { std::fprintf(stderr, "rrx_host_selftest_netcdf4: %s\n", e.what()); return 100; }
}

// The one real NetCDF-4 file of the reference tree (data/aerosol_optics.nc, written by netCDF4-python): dimensions and a few
// values, against numbers obtained independently with h5dump. Returns 0, or the index of the first check that failed.
int rrx_host_selftest_read_aerosol_file(const char* path)
{
    try
    {
        Netcdf_file f(path, Netcdf_mode::Read);
        if (f.get_dimension_size("band_sw") != 14 || f.get_dimension_size("relative_humidity") != 12 ||
            f.get_dimension_size("hydrophilic") != 7 || f.get_dimension_size("hydrophobic") != 14) return 1;
        const auto d = f.get_variable_dimensions("mass_ext_sw_hydrophilic");
        if (d.size() != 3 || d.at("hydrophilic") != 7 || d.at("relative_humidity") != 12 || d.at("band_sw") != 14) return 2;
        const std::vector<double> m = f.get_variable<double>("mass_ext_sw_hydrophilic", {7, 12, 14});
        const double want_m[14] = {123.197, 166.189, 433.198, 245.302, 317.993, 488.143, 809.627, 1028.66, 1760, 3071.97, 4759.77, 6852.52, 8921.85, 10958.8};
        for (int i=0; i<14; ++i) if (std::abs(m[(3*12 + 5)*14 + i] - want_m[i]) > 6e-6*want_m[i]) return 3;
        const std::vector<double> s = f.get_variable<double>("ssa_sw_hydrophobic", {14, 14});
        const double want_s[6] = {0.152659, 0.11512, 0.719504, 0.963146, 0.96859, 0.998038};
        for (int i=0; i<6; ++i) if (std::abs(s[13*14 + i] - want_s[i]) > 6e-6) return 4;
        const std::vector<double> rh = f.get_variable<double>("relative_humidity1", {12});
        const double want_rh[12] = {0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.85, 0.9, 0.95};
        for (int i=0; i<12; ++i) if (std::abs(rh[i] - want_rh[i]) > 1e-6) return 5;
        const std::vector<double> wn = f.get_variable<double>("wavenumber1_sw", {14});
        if (wn[0] != 820. || wn[1] != 2600. || wn[13] != 38000.) return 6;
        return 0;
    }
    catch (const std::exception& e) { std::fprintf(stderr, "rrx_host_selftest_read_aerosol_file: %s\n", e.what()); return 100; }
}
}
