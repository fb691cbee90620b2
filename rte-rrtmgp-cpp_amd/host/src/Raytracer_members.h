// What Raytracer_gpu and Raytracer_bw_gpu share behind their headers: a view of the optional members that both classes keep (the
// phase table, the background, the aerosol triples) and THE ONE PLACE that turns them into the pointer groups of the C entries; and,
// for Raytracer_bw_gpu and Raytracer_thermal_gpu, the one place that lays a sensor out as the C entries take it.
// Everything here has internal linkage: the libraries export what they exported.
#ifndef RAYTRACER_MEMBERS_H
#define RAYTRACER_MEMBERS_H

#include "Array.h"
#include "types.h"

namespace
{
struct Rt_members
{
    bool has_table, has_bg, has_aer;
    const Array_gpu<Float,1>& mu; const Array_gpu<Float,3>& phase; const Array_gpu<Float,3>& cdf; const Array_gpu<Float,2>& cld_re;
    Float re0, dre;
    const Array<Float,1>& dz_bg;
    const Array_gpu<Float,2>& bg_tau; const Array_gpu<Float,2>& bg_ssa;
    const Array_gpu<Float,2>& bg_cld_tau; const Array_gpu<Float,2>& bg_cld_ssa; const Array_gpu<Float,2>& bg_cld_g;
    const Array_gpu<Float,3>& aer_tau; const Array_gpu<Float,3>& aer_ssa; const Array_gpu<Float,3>& aer_g;
    const Array_gpu<Float,2>& bg_aer_tau; const Array_gpu<Float,2>& bg_aer_ssa; const Array_gpu<Float,2>& bg_aer_g;

    int nbg() const { return has_bg ? dz_bg.size() : 0; }
    bool bg_cloudy() const { return has_bg && bg_cld_tau.size() > 0; }
    bool hazy() const { return has_aer && aer_tau.size() > 0; }
    bool bg_hazy() const { return has_aer && bg_aer_tau.size() > 0; }

    // the checks of the members that both classes make in the same words
    void check_table(const std::string& who, const long long ncol, const int nz, const int nbnd) const
    {
        if (has_table && (cld_re.dim(1) != ncol || cld_re.dim(2) != nz || phase.dim(3) != nbnd))
            throw std::runtime_error(who + "the phase table's cld_re is not (nx ny, nz) or its tables are not (nmu, nre, nbnd)");
    }
    void check_aerosol(const std::string& who, const long long ncol, const int nz, const int nbnd) const
    {
        if (hazy() && (aer_tau.dim(1) != ncol || aer_tau.dim(2) != nz || aer_tau.dim(3) != nbnd))
            throw std::runtime_error(who + "the aerosol arrays are not (nx ny, nz, nbnd)");
    }
    void check_bg_aerosol(const std::string& who, const int nbnd) const
    {
        if (has_bg && bg_hazy() && (bg_aer_tau.dim(1) != nbg() || bg_aer_tau.dim(2) != nbnd))
            throw std::runtime_error(who + "the background's aerosol arrays are not (nbg, nbnd)");
    }
    void check_no_bg_aerosol_alone(const std::string& who) const
    {
        if (!has_bg && bg_hazy()) throw std::runtime_error(who + "a background aerosol is set without a background");
    }
};

// the members of the class whose method this is written in
#define RT_MEMBERS Rt_members{has_table, has_bg, has_aer, mu, phase, cdf, cld_re, re0, dre, dz_bg, bg_tau, bg_ssa, bg_cld_tau, bg_cld_ssa, bg_cld_g, \
                              aer_tau, aer_ssa, aer_g, bg_aer_tau, bg_aer_ssa, bg_aer_g}

// The pointer groups of the C entries: what is not set, or empty, is NULL (and nmu, nre, nbg are 0).
struct Rt_pointers
{
    const Float* cld[3];
    int nmu, nre; Float re0, dre; const Float* table[4];
    int nbg; const Float* bg[6];
    const Float* aer[3]; const Float* bg_aer[3];

    Rt_pointers(const Rt_members& m, const Array_gpu<Float,3>& cld_tau, const Array_gpu<Float,3>& cld_ssa, const Array_gpu<Float,3>& cld_g)
    {
        const Float* none = nullptr;
        const bool cloudy = cld_tau.size() > 0, bg_cloudy = m.bg_cloudy(), hazy = m.hazy(), bg_hazy = m.has_bg && m.bg_hazy();
        cld[0] = cloudy ? cld_tau.ptr() : none; cld[1] = cloudy ? cld_ssa.ptr() : none; cld[2] = cloudy ? cld_g.ptr() : none;
        nmu = m.has_table ? m.mu.dim(1) : 0; nre = m.has_table ? m.phase.dim(2) : 0; re0 = m.re0; dre = m.dre;
        table[0] = m.has_table ? m.mu.ptr() : none; table[1] = m.has_table ? m.phase.ptr() : none;
        table[2] = m.has_table ? m.cdf.ptr() : none; table[3] = m.has_table ? m.cld_re.ptr() : none;
        nbg = m.nbg();
        bg[0] = m.has_bg ? m.dz_bg.ptr() : none; bg[1] = m.has_bg ? m.bg_tau.ptr() : none; bg[2] = m.has_bg ? m.bg_ssa.ptr() : none;
        bg[3] = bg_cloudy ? m.bg_cld_tau.ptr() : none; bg[4] = bg_cloudy ? m.bg_cld_ssa.ptr() : none; bg[5] = bg_cloudy ? m.bg_cld_g.ptr() : none;
        aer[0] = hazy ? m.aer_tau.ptr() : none; aer[1] = hazy ? m.aer_ssa.ptr() : none; aer[2] = hazy ? m.aer_g.ptr() : none;
        bg_aer[0] = bg_hazy ? m.bg_aer_tau.ptr() : none; bg_aer[1] = bg_hazy ? m.bg_aer_ssa.ptr() : none; bg_aer[2] = bg_hazy ? m.bg_aer_g.ptr() : none;
    }
};

// a sensor (Sensor_bw) laid out as the 12 numbers of the C entries: position, e_w, e_h, e_d
struct Rt_sensor_numbers
{
    Float s[12];

    template<typename Sensor>
    explicit Rt_sensor_numbers(const Sensor& sensor)
    {
        for (int i=0; i<3; ++i) { s[i] = sensor.position[i]; s[3+i] = sensor.e_w[i]; s[6+i] = sensor.e_h[i]; s[9+i] = sensor.e_d[i]; }
    }
};

// the groups as the arguments of a call
#define RT_CLOUD(p) p.cld[0], p.cld[1], p.cld[2]
#define RT_TABLE(p) p.nmu, p.nre, p.re0, p.dre, p.table[0], p.table[1], p.table[2], p.table[3]
#define RT_BACKGROUND(p) p.nbg, p.bg[0], p.bg[1], p.bg[2], p.bg[3], p.bg[4], p.bg[5]
}

#endif
