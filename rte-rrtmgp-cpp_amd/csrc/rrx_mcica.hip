// McICA cloud sampling (no counterpart in the reference library, upstream RTE+RRTMGP keeps it in mo_cloud_sampling):
// every g-point of a column sees its own sub-column, cloudy or clear in each layer, drawn from the layer cloud fractions under
// maximum-random or exponential-random overlap. Upstream makes a random array, a mask and g-point cloud arrays and increments every
// cell; here one kernel forms the random numbers in registers (Philox4x32-10, counter = the cell's global identity, so a column
// draws the same sub-columns wherever and in whatever order it is processed) and combines the band cloud properties into the
// g-point arrays in place, in the cloudy cells only. A clear layer costs one read of its cloud fraction; a clear cell is not written.
//
// Shape: columns on the lanes (rows of 64 columns of the (col, lay, gpt) arrays: every load and store of a wave is one contiguous
// row segment, one cell per lane -- the store shape that streams at the full rate, profiles/r04_store_pattern.txt), one g-point
// per block row with its band found once, and each thread walks the layers of its (column, g-point) with the rank in a register.
#include "rrx_common.h"
#include "rrx_philox.h"
#include "rrx_hip.h"

namespace
{
using namespace rrx;

// rrx_increment_2stream_by_2stream's arithmetic (inc_2str of rrx_misc.hip), operation for operation
template<typename F>
__device__ __forceinline__ void inc_2str(F& tau1, F& ssa1, F& g1, const F tau2, const F ssa2, const F g2, const F eps)
{
    const F tau12 = tau1 + tau2;
    const F tauscat12 = (tau1 * ssa1) + (tau2 * ssa2);
    g1 = ((tau1 * ssa1 * g1) + (tau2 * ssa2 * g2)) / max(tauscat12, eps);
    ssa1 = tauscat12 / max(eps, tau12);
    tau1 = tau12;
}

// The draws of one (column, g-point): one Philox call per four layers and kind of draw, made when a layer of the group first asks
struct Draws
{
    unsigned c0, c1, k0, k1, dom2;
    int group[2];
    Philox words[2];
    __device__ __forceinline__ unsigned word(const int which, const int ilay)
    {
        const int grp = ilay >> 2;
        if (group[which] != grp)
        {
            words[which] = philox4x32_10(c0, c1, unsigned(grp), dom2 + unsigned(which), k0, k1);
            group[which] = grp;
        }
        const int s = ilay & 3;
        const Philox& p = words[which];
        return s == 0 ? p.w[0] : (s == 1 ? p.w[1] : (s == 2 ? p.w[2] : p.w[3]));
    }
};

// the identities of reordered columns: col_id[i] = perm[i] + offset
__global__ void column_ids_kernel(const int n, const int* __restrict__ perm, const int offset, int* __restrict__ col_id)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i < n) col_id[i] = perm[i] + offset;
}

// MODE 0: the mask only; 1: tau += cld_tau; 2: (tau, ssa, g) combined with (cld_tau, cld_ssa, cld_g)
template<typename F, int MODE>
__global__ void __launch_bounds__(256) mcica_kernel(
        const int ncol, const int nlay, const int nbnd, const int* __restrict__ band_lims_gpt,
        const F* __restrict__ cloud_frac, const F* __restrict__ alpha, const unsigned k0, const unsigned k1, const unsigned dom2,
        const int* __restrict__ col_id, const int col_id0,
        F* __restrict__ tau, F* __restrict__ ssa, F* __restrict__ g,
        const F* __restrict__ cld_tau, const F* __restrict__ cld_ssa, const F* __restrict__ cld_g,
        unsigned char* __restrict__ mask_out, const F eps)
{
    const int igpt = blockIdx.y;
    const int icol = blockIdx.x*blockDim.x + threadIdx.x;
    int ibnd = -1;                      // (the g-points of no band are sampled -- the mask is theirs too -- and left as they are)
    if (MODE != 0)
        for (int b=nbnd-1; b>=0; --b)
            if (igpt+1 >= band_lims_gpt[2*b] && igpt+1 <= band_lims_gpt[2*b+1]) ibnd = b;
    if (MODE != 0 && ibnd < 0 && mask_out == nullptr) return;
    if (icol >= ncol) return;

    Draws d;
    d.c0 = unsigned(col_id != nullptr ? col_id[icol] : col_id0 + icol); d.c1 = unsigned(igpt);
    d.k0 = k0; d.k1 = k1; d.dom2 = dom2; d.group[0] = d.group[1] = -1;

    F rank = F(0.), f_above = F(0.);
    for (int ilay=0; ilay<nlay; ++ilay)
    {
        const size_t cl = size_t(ilay)*ncol + icol;
        const F f = cloud_frac[cl];
        bool cloudy = false;
        if (f > F(0.))       // (a clear layer never uses its rank: the next layer draws its own)
        {
            bool keep = ilay > 0 && f_above > F(0.);
            if (keep && alpha != nullptr)
                keep = uniform<F>(d.word(1, ilay)) < alpha[cl - ncol];
            if (!keep) rank = uniform<F>(d.word(0, ilay));
            cloudy = rank > F(1.) - f;
        }
        f_above = f;
        const size_t o = size_t(igpt)*nlay*ncol + cl;
        if (mask_out != nullptr) mask_out[o] = cloudy ? 1 : 0;
        if (MODE != 0 && cloudy && ibnd >= 0)
        {
            const size_t b = size_t(ibnd)*nlay*ncol + cl;
            if (MODE == 1)
                tau[o] = tau[o] + cld_tau[b];
            else
            {
                F t = tau[o], w = ssa[o], gg = g[o];
                inc_2str(t, w, gg, cld_tau[b], cld_ssa[b], cld_g[b], eps);
                tau[o] = t; ssa[o] = w; g[o] = gg;
            }
        }
    }
}

template<typename F, int MODE>
int launch(const char* entry, int ncol, int nlay, int ngpt, int nbnd, const int* band_lims_gpt, const F* cloud_frac, const F* alpha,
           unsigned long long seed, int domain, const int* col_id, int col_id0, F* tau, F* ssa, F* g,
           const F* cld_tau, const F* cld_ssa, const F* cld_g, unsigned char* mask_out, void* stream)
{
    RRX_TRY
    for (const int n : {ncol, nlay, ngpt, nbnd}) if (n < 0) throw std::runtime_error("negative extent");
    if (ncol == 0 || nlay == 0 || ngpt == 0 || (MODE != 0 && nbnd == 0)) return 0;
    const char* bad = nullptr;
    if (cloud_frac == nullptr) bad = "cloud_frac is NULL";
    else if (MODE == 0 && mask_out == nullptr) bad = "mask_out is NULL";
    else if (MODE != 0 && band_lims_gpt == nullptr) bad = "band_lims_gpt is NULL";
    else if (MODE != 0 && (tau == nullptr || cld_tau == nullptr)) bad = "tau_inout or cld_tau is NULL";
    else if (MODE == 2 && (ssa == nullptr || g == nullptr || cld_ssa == nullptr || cld_g == nullptr)) bad = "ssa_inout, g_inout, cld_ssa or cld_g is NULL";
    else if (ngpt > 65535) bad = "ngpt exceeds 65535 (one g-point per block row)";
    if (bad != nullptr) throw std::runtime_error(bad);
    const dim3 grid(ceil_div(ncol, 256), ngpt);
    mcica_kernel<F, MODE><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(
        ncol, nlay, nbnd, band_lims_gpt, cloud_frac, alpha, unsigned(seed & 0xFFFFFFFFull), unsigned(seed >> 32),
        2u*unsigned(domain), col_id, col_id0, tau, ssa, g, cld_tau, cld_ssa, cld_g, mask_out, Lim<F>::tiny()*F(3.));
    RRX_CATCH(entry)
}
}  // namespace

extern "C"
{
int rrx_mcica_column_ids(int n, const int* perm, int offset, int* col_id, void* stream)
{
    RRX_TRY
    if (n < 0) throw std::runtime_error("negative extent");
    if (n == 0) return 0;
    if (perm == nullptr || col_id == nullptr) throw std::runtime_error("perm or col_id is NULL");
    column_ids_kernel<<<rrx::ceil_div(n, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(n, perm, offset, col_id);
    RRX_CATCH("rrx_mcica_column_ids")
}

#define RRX_DEFINE_MCICA(F, SFX) \
int rrx_mcica_increment_1scalar##SFX(int ncol, int nlay, int ngpt, int nbnd, const int* band_lims_gpt, const F* cloud_frac, const F* alpha, \
        unsigned long long seed, int domain, const int* col_id, int col_id0, F* tau_inout, const F* cld_tau, unsigned char* mask_out, void* stream) \
{ return launch<F, 1>("rrx_mcica_increment_1scalar" #SFX, ncol, nlay, ngpt, nbnd, band_lims_gpt, cloud_frac, alpha, seed, domain, col_id, col_id0, \
                      tau_inout, nullptr, nullptr, cld_tau, nullptr, nullptr, mask_out, stream); } \
int rrx_mcica_increment_2stream##SFX(int ncol, int nlay, int ngpt, int nbnd, const int* band_lims_gpt, const F* cloud_frac, const F* alpha, \
        unsigned long long seed, int domain, const int* col_id, int col_id0, F* tau_inout, F* ssa_inout, F* g_inout, \
        const F* cld_tau, const F* cld_ssa, const F* cld_g, unsigned char* mask_out, void* stream) \
{ return launch<F, 2>("rrx_mcica_increment_2stream" #SFX, ncol, nlay, ngpt, nbnd, band_lims_gpt, cloud_frac, alpha, seed, domain, col_id, col_id0, \
                      tau_inout, ssa_inout, g_inout, cld_tau, cld_ssa, cld_g, mask_out, stream); } \
int rrx_mcica_cloud_mask##SFX(int ncol, int nlay, int ngpt, const F* cloud_frac, const F* alpha, unsigned long long seed, int domain, \
        const int* col_id, int col_id0, unsigned char* mask_out, void* stream) \
{ return launch<F, 0>("rrx_mcica_cloud_mask" #SFX, ncol, nlay, ngpt, 0, nullptr, cloud_frac, alpha, seed, domain, col_id, col_id0, \
                      static_cast<F*>(nullptr), nullptr, nullptr, nullptr, nullptr, nullptr, mask_out, stream); }

RRX_DEFINE_MCICA(double, _f64)
RRX_DEFINE_MCICA(float, _f32)
}
