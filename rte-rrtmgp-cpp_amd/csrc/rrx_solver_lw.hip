// Longwave no-scattering solver, fused (boundary condition + source + both transport sweeps + quadrature
// scaling in ONE kernel, no global scratch). Replaces the reference's launcher
//   Rte_solver_kernels_cuda::lw_solver_noscat   (/root/reference/src_kernels_cuda/rte_solver_kernels_launchers.cu:61-286)
// and its kernels lw_solver_noscat_step_{1,2,3}_kernel, lw_transport_noscat_kernel, apply_BC_kernel
// (/root/reference/src_kernels_cuda/rte_solver_kernels.cu:35-193,351-387).
//
// MI355X design (DESIGN.md section "lw_solver_noscat"):
//   * arrays are (col, lay, gpt) with the column index fastest. One wavefront owns a tile of 8*V columns x all
//     levels of one g-point. The 64 lanes are 8 column-lanes x 8 level-lanes: lane = ll*8 + cl.
//   * level-lane ll owns K consecutive levels/layers (in top-to-surface "sweep" order), held in registers.
//     Every input is read exactly once from HBM, every output written exactly once.
//   * the serial vertical recurrences x' = t*x + s are affine maps; each lane composes its K maps, an 8-lane
//     Hillis-Steele scan (3 __shfl steps, stride 8 lanes) propagates the boundary values between level-lanes,
//     and each lane then replays its K layers from its incoming value.
#include "rrx_common.h"
#include "rrx_hip.h"

#pragma clang fp contract(fast)

namespace
{
using namespace rrx;

constexpr int CL = 8;    // column lanes
constexpr int LL = 8;    // level lanes

// The levels of the same 8*V columns are spread over 16 level-lanes in two adjacent wavefronts (W = 2 waves per column group, two
// column groups per workgroup); the two vertical scans exchange each wave's total through LDS, one block barrier per scan.
template<typename F, int V, int K, bool JAC, bool ACC>
__global__ void __launch_bounds__(256, 2)
lw_noscat_scan_kernel(
        const int ncol, const int nlay, const int ngpt, const int top_at_1, const int imu,
        const F* __restrict__ secants, const F* __restrict__ weights,
        const F* __restrict__ tau, const F* __restrict__ lay_source, const F* __restrict__ lev_source,
        const F* __restrict__ sfc_emis, const F* __restrict__ sfc_src, const F* __restrict__ inc_flux,
        F* __restrict__ flux_up, F* __restrict__ flux_dn,
        const F* __restrict__ sfc_src_jac, F* __restrict__ flux_up_jac, const int sync_waves)
{
    constexpr int W = 2;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int cl = lane & (CL-1);
    const int ll = lane / CL;
    const int h = wave % W;                          // which part of the column this wave holds (0 = TOA side)
    const int wave_col0 = (blockIdx.x*(4/W) + wave/W) * (CL*V);
    __shared__ F xch[4*V][4][CL];                    // wave totals of the two scans

    int icol = wave_col0 + cl*V;
    const bool active = icol < ncol;                  // all V columns exist (ncol % V == 0) or none
    if (!active) icol = (wave_col0 < ncol) ? wave_col0 : 0;    // harmless duplicate loads, no stores
    const bool writer = active && wave_col0 < ncol;

    const int nlev = nlay + 1;
    const size_t ncl = size_t(ncol);
    const int t0 = (h*LL + ll)*K;

    // one g-point per workgroup row (grid.y = ngpt), written as a loop over that range: the form whose instruction stream was measured
    const int g_end = blockIdx.y + 1;
    for (int igpt=blockIdx.y; igpt<g_end; ++igpt)
    {
    // The two waves that share each 128-B line (8 columns x 8 B = 64 B per wave when V = 1) must issue their load
    // bursts together, or the second half of every line is fetched from HBM again once L2 has turned over
    // (measured: +26 % FETCH_SIZE without the barrier). No thread leaves before the barrier.
    if (sync_waves) __syncthreads();
    const size_t lay_base = size_t(igpt)*ncl*nlay + icol;
    const size_t lev_base = size_t(igpt)*ncl*nlev + icol;
    const size_t sfc_idx = size_t(igpt)*ncl + icol;

    const F pi = F(3.14159265358979323846);
    const F eps = Lim<F>::eps();
    const F tau_thres = sqrt(sqrt(eps));

    const Vec<F,V> D = load_cols<F,V>(secants + sfc_idx + size_t(imu)*ncl*ngpt);
    const F w = weights[imu];

    F tr[K][V], sdn[K][V], sup[K][V];
    Vec<F,V> lv[K];

    // level sources at this lane's K levels (sweep order: level t is ABOVE layer t)
    #pragma unroll
    for (int j=0; j<K; ++j)
    {
        const int t = min(t0 + j, nlay);
        const int ml = top_at_1 ? t : nlay - t;
        lv[j] = load_cols<F,V>(lev_source + lev_base + size_t(ml)*ncl);
    }

    // level below the lane's last layer: first level of the next level-lane; across the wave seam it is loaded
    Vec<F,V> lv_next;
    #pragma unroll
    for (int v=0; v<V; ++v) lv_next.v[v] = shfl(lv[0].v[v], lane + CL);
    if (ll == LL-1)
    {
        const int t = min(t0 + K, nlay);
        const int ml = top_at_1 ? t : nlay - t;
        lv_next = load_cols<F,V>(lev_source + lev_base + size_t(ml)*ncl);
    }

    F A[V], Bdn[V], Bup[V];
    #pragma unroll
    for (int v=0; v<V; ++v) { A[v] = F(1.); Bdn[v] = F(0.); Bup[v] = F(0.); }

    #pragma unroll
    for (int j=0; j<K; ++j)
    {
        const int s = t0 + j;
        const bool valid = s < nlay;
        const int sc = min(s, nlay-1);
        const int ml = top_at_1 ? sc : nlay-1-sc;
        const Vec<F,V> tv = load_cols<F,V>(tau + lay_base + size_t(ml)*ncl);
        const Vec<F,V> ls = load_cols<F,V>(lay_source + lay_base + size_t(ml)*ncl);

        #pragma unroll
        for (int v=0; v<V; ++v)
        {
            // level source below this layer: next register, or the first level of the next level-lane
            F lev_below;
            if (j < K-1) lev_below = lv[j+1].v[v];
            else         lev_below = lv_next.v[v];
            const F lev_above = lv[j].v[v];

            // a padding layer (level slot beyond the surface) is made transparent through its optical depth: tau = 0 gives
            // trans = 1 and fact = 0 (series branch) exactly, hence zero sources -- one select instead of three
            const F tau_loc = (valid ? tv.v[v] : F(0.)) * D.v[v];
            const F trans = exp_neg(-tau_loc);
            const F fact = tau_loc > tau_thres ?
                (F(1.) - trans) * fast_rcp(tau_loc) - trans :
                tau_loc * (F(.5) + tau_loc * (F(-1./3.) + tau_loc * F(1./8.)));
            const F omt = F(1.) - trans;
            const F s_dn = omt * lev_below + F(2.) * fact * (ls.v[v] - lev_below);
            const F s_up = omt * lev_above + F(2.) * fact * (ls.v[v] - lev_above);

            tr[j][v]  = trans;
            sdn[j][v] = s_dn;
            sup[j][v] = s_up;

            Bdn[v] = tr[j][v] * Bdn[v] + sdn[j][v];
            Bup[v] += A[v] * sup[j][v];
            A[v] *= tr[j][v];
        }
    }

    const Vec<F,V> emis = load_cols<F,V>(sfc_emis + sfc_idx);
    const Vec<F,V> ssrc = load_cols<F,V>(sfc_src + sfc_idx);
    Vec<F,V> inc;
    if (inc_flux != nullptr) inc = load_cols<F,V>(inc_flux + sfc_idx);
    Vec<F,V> sjac;
    if constexpr (JAC) sjac = load_cols<F,V>(sfc_src_jac + sfc_idx);

    F dn_in[V], up_in[V], jac_in[V];

    #pragma unroll
    for (int v=0; v<V; ++v)
    {
        // ---- downward: inclusive scan over level-lanes 0..ll
        F a = A[v], b = Bdn[v];
        #pragma unroll
        for (int d=1; d<LL; d<<=1)
        {
            const F a2 = shfl(a, lane - d*CL);
            const F b2 = shfl(b, lane - d*CL);
            if (ll >= d) { b = a*b2 + b; a = a*a2; }
        }
        F xa = F(1.), xb = F(0.);                               // composite of the levels above this wave's
        // every wave publishes the composite of its part; (xa, xb) = the parts above this wave's, TOA side first;
        // (fa, fb) = all parts, composed in the same order by every wave (bit-identical dn_sfc in all of them)
        if (ll == LL-1) { xch[4*v+0][wave][cl] = a; xch[4*v+1][wave][cl] = b; }
        __syncthreads();
        const int w0 = wave - h;                         // first wave of this column group
        F fa = F(1.), fb = F(0.);                        // composite of the whole column
        #pragma unroll
        for (int w=0; w<W; ++w)
        {
            const F oa = xch[4*v+0][w0+w][cl], ob = xch[4*v+1][w0+w][cl];
            if (w == h) { xa = fa; xb = fb; }
            fb = oa*fb + ob; fa = oa*fa;
        }
        if (h > 0) { b = a*xb + b; a = a*xa; }
        F ae = shfl(a, lane - CL), be = shfl(b, lane - CL);     // exclusive
        if (ll == 0) { ae = xa; be = xb; }
        const F dn_top = (inc_flux != nullptr) ? inc.v[v] / pi : F(0.);
        dn_in[v] = ae*dn_top + be;
        const F dn_sfc = fa*dn_top + fb;

        // ---- surface
        const F up_sfc = dn_sfc * (F(1.) - emis.v[v]) + emis.v[v] * ssrc.v[v];

        // ---- upward: inclusive suffix scan over level-lanes ll..7
        a = A[v]; b = Bup[v];
        #pragma unroll
        for (int d=1; d<LL; d<<=1)
        {
            const F a2 = shfl(a, lane + d*CL);
            const F b2 = shfl(b, lane + d*CL);
            if (ll + d < LL) { b = a*b2 + b; a = a*a2; }
        }
        xa = F(1.); xb = F(0.);                                 // composite of the levels below this wave's
        if (ll == 0) { xch[4*v+2][wave][cl] = a; xch[4*v+3][wave][cl] = b; }
        __syncthreads();
        #pragma unroll
        for (int w=W-1; w>=1; --w)                       // the parts below this wave's, surface side first
        {
            if (w > h)
            {
                const F oa = xch[4*v+2][w0+w][cl], ob = xch[4*v+3][w0+w][cl];
                xb = oa*xb + ob; xa = oa*xa;
            }
        }
        if (h < W-1) { b = a*xb + b; a = a*xa; }
        ae = shfl(a, lane + CL); be = shfl(b, lane + CL);
        if (ll == LL-1) { ae = xa; be = xb; }
        up_in[v] = ae*up_sfc + be;
        if constexpr (JAC) jac_in[v] = ae * emis.v[v] * sjac.v[v];
    }

    // ---- replay this lane's K layers and store its K levels (each value is stored as soon as it exists: no staging)
    const F scale = pi * w;

    auto put = [&](F* __restrict__ arr, const int j, Vec<F,V> val)
    {
        const int t = t0 + j;
        if (writer && t <= nlay)
        {
            const int ml = top_at_1 ? t : nlay - t;
            F* o = arr + lev_base + size_t(ml)*ncl;
            if constexpr (ACC)
            {
                const Vec<F,V> prev = load_cols<F,V>(o);
                #pragma unroll
                for (int v=0; v<V; ++v) val.v[v] += prev.v[v];
            }
            store_cols<F,V>(o, val);
        }
    };

    {
        F dn[V];
        #pragma unroll
        for (int v=0; v<V; ++v) dn[v] = dn_in[v];
        #pragma unroll
        for (int j=0; j<K; ++j)
        {
            Vec<F,V> o;
            #pragma unroll
            for (int v=0; v<V; ++v) { o.v[v] = scale * dn[v]; dn[v] = tr[j][v]*dn[v] + sdn[j][v]; }
            put(flux_dn, j, o);
        }
    }
    {
        F up[V], jc[V];
        #pragma unroll
        for (int v=0; v<V; ++v) { up[v] = up_in[v]; jc[v] = JAC ? jac_in[v] : F(0.); }
        #pragma unroll
        for (int j=K-1; j>=0; --j)
        {
            Vec<F,V> o, oj;
            #pragma unroll
            for (int v=0; v<V; ++v)
            {
                up[v] = tr[j][v]*up[v] + sup[j][v];
                o.v[v] = scale * up[v];
                if constexpr (JAC) { jc[v] = tr[j][v]*jc[v]; oj.v[v] = scale * jc[v]; }
            }
            put(flux_up, j, o);
            if constexpr (JAC) put(flux_up_jac, j, oj);
        }
    }
    }   // g-point loop
}


// ---------------------------------------------------------------------------------------------------------------------
// Fused broadband form: the workgroup walks over the g-points of its columns with the tiling and scans of lw_noscat_scan_kernel and
// keeps the g-point sums of both fluxes on chip (same summation order as sum_broadband over stored per-g-point fluxes, so the same
// bits); flux_up/flux_dn are then (ncol, nlev) arrays. Saves the per-g-point flux stores and the reduction pass that reads them back.
// The g-point loop is software-pipelined: the loads of g-point g+1 are requested behind the first scan barrier of g-point g and land
// during its scans and replays (tools/labs/lw_lab.hip: 2.78 -> 2.59 ms at C4 fp64).
//   LITE : "Planck-lite" inputs. Instead of lay_source and lev_source the kernel reads the Planck fractions pfrac(col,lay,gpt)
//          and the band-integrated Planck functions B_lay(col,lay,bnd), B_lev(col,lev,bnd), and rebuilds
//          lay_source = pfrac*B_lay, lev_source = sqrt(pfrac*pfrac')*B_lev (first and last level: pfrac*B_lev) itself,
//          exactly the expressions of Planck_source_kernel (gas_optics_rrtmgp_kernels.cu:196-314). Two cell arrays read per
//          g-point instead of three, and the Planck kernel writes one instead of two (LW chain at C4: 9.9 -> 7.5 ms).
//          The band's B values sit in per-thread LDS columns and are refreshed when the band changes.
// One quadrature angle (the general kernel above keeps more); the surface-temperature Jacobian in the JAC form (below).
#ifndef RRX_LW_LACC
#define RRX_LW_LACC 1
#endif
#ifndef RRX_LW_EXP_TABLE
#define RRX_LW_EXP_TABLE 1
#endif
#ifndef RRX_LW_TIMING
#define RRX_LW_TIMING 0   // diagnostic build (tools/sw_timing.sh): every wavefront adds the clocks it spends per phase of a g-point to g_lw_clk
#endif
#if RRX_LW_TIMING
__device__ unsigned long long g_lw_clk[16][8];
#define RRX_LW_T(k) { const unsigned long long t_ = __builtin_readcyclecounter(); lw_acc[k] += t_ - lw_t; lw_t = t_; }
#else
#define RRX_LW_T(k)
#endif
#ifndef RRX_LW_LACC32
#define RRX_LW_LACC32 1    // fp32, two columns per lane: g-point sums in LDS columns too (round 4: the register form spilled 37-41 VGPRs)
#endif
#ifndef RRX_LW_EV
#define RRX_LW_EV 1         // layers of evaluations the scheduler may interleave (2: the same speed, but the fp32 two-column form then keeps 16 B of scratch per lane)
#endif
// NW = wavefronts per workgroup: 4, or 8 with W = 8 for columns of up to 287 layers (round 3: eight waves x four level-lanes x
// nine layers; one workgroup per CU then, the same two waves per SIMD).
// Round 4, fp32: one column per lane with W = 4 and NW = 8 (two column groups per workgroup share each 128-B line of the 64-B
// rows) -- the geometry of the fp32 SW solver (rrx_solver_sw.hip, CLT note); here it serves odd column counts only.
#ifndef RRX_LW_F32_WAVES
#define RRX_LW_F32_WAVES 2
#endif
// BND (by-band outputs): blockIdx.y = band b, whose g-points [band_lims[2b]-1, band_lims[2b+1]) the workgroup sums in order from zero
// (rrx_sum_byband's order); the sums go to band slab b of flux_up/flux_dn, (ncol, nlev, nbnd) arrays. An empty band writes zeros.
// JAC (surface-temperature Jacobian of the upward flux, rrx_lw_solver_noscat_fractions_jac): the upward scan's transmittance product
// below the lane, times emis*sfc_src_jac, is the lane's incoming Jacobian (the general kernel's jac_in); the replay is jc = trans*jc and
// the g-point sums go to flux_up_jac in order with add_rounded, like the fluxes. The sums sit in registers (K more per column) whatever
// LACC says: the LDS of the four-wave fp64 form has no room for a third column at two workgroups per CU.
// MU (several quadrature angles, rrx_lw_solver_noscat_fractions_angles): the g-point's loads are issued once and the sequence evaluate ->
// scans -> replay runs nmus times on them (a run-time, wave-uniform count), with D = secants(col, gpt, imu) read per column and g-point
// one angle ahead and each angle's term added with pi*weights[imu] straight into the running g-point sums. The loaded g-point stays
// in its registers through the angles (no second copy); the prefetch of the next g-point overwrites it behind the first barrier of
// the LAST angle, when the evaluation has consumed it. Through an angle's evaluation the g-point (2K values per column) and tr / sdn /
// sup (3K) are live together, which the one-angle form avoids: the nine-layer forms spill. The source terms pfrac*B_lay
// and sqrt(pfrac*pfrac')*B_lev are recomputed per angle: holding them takes 2K+1 more registers per column.
// Everything MU adds is written so that the one-angle forms keep the statements, and with them the code, they had before it.
// OPT (optimal-angle secants, rrx_lw_solver_noscat_fractions_optimal): no secants array is read. At the top of a g-point, when its
// loads have landed, each lane adds the tau of its K layers, a butterfly over the level-lanes (ds_bpermute, stride CL) gives every
// lane its wave's sum, the W waves of the column group exchange theirs through LDS (xsum) behind a barrier of their own, and every
// lane forms D = fit(1,b)*exp(-S) + fit(2,b) from the band's two coefficients, which are refreshed where the band's Planck functions
// are. Every lane of a column adds the same values in the same order, so all of them hold the same D. The lanes ll = 0 of the
// column group's first wave write D to secants_out(col, gpt) when it is given. One angle, Planck-lite inputs, no by-band form.
template<typename F, int V, int K, int W, int CLT, bool LITE, bool GS = false, int EV = RRX_LW_EV, int NW = (W > 4 ? W : 4), bool BND = false,
         bool JAC = false, bool MU = false, bool OPT = false>
__global__ void __launch_bounds__(64*NW, (NW > W) ? RRX_LW_F32_WAVES : (NW > 4 ? 1 : 2))
lw_noscat_bb_kernel(
        const int ncol, const int nlay, const int ngpt, const int top_at_1,
        const F* __restrict__ secants, const F* __restrict__ weights,
        const F* __restrict__ tau, const F* __restrict__ lay_source /* or pfrac */, const F* __restrict__ lev_source,
        const F* __restrict__ blay, const F* __restrict__ blev, const int* __restrict__ gpoint_bands,
        const F* __restrict__ sfc_emis, const F* __restrict__ sfc_src, const F* __restrict__ inc_flux,
        F* __restrict__ flux_up, F* __restrict__ flux_dn, const int gper, const size_t part_stride,
        const int* __restrict__ band_lims, const F* __restrict__ sfc_src_jac = nullptr, F* __restrict__ flux_up_jac = nullptr,
        const int nmus = 1, const F* __restrict__ opt_fit = nullptr, F* __restrict__ secants_out = nullptr)
{
    static_assert(!(GS && BND), "a by-band launch is its own g-point split");
    static_assert(!(JAC && BND), "no by-band Jacobian");
    static_assert(!MU || (LITE && !BND), "several angles: Planck-lite inputs, no by-band form");
    static_assert(!OPT || (LITE && !BND), "optimal angles: Planck-lite inputs, no by-band form");
    static_assert(!(OPT && MU), "optimal angles are one quadrature angle");
    // GS: blockIdx.y = g-point range [g_lo, g_hi) of this workgroup; its sums go to partial array blockIdx.y
    const int g_lo = BND ? max(band_lims[2*blockIdx.y] - 1, 0) : (GS ? blockIdx.y*gper : 0);
    const int g_hi = BND ? min(band_lims[2*blockIdx.y+1], ngpt) : (GS ? min(ngpt, g_lo + gper) : ngpt);
    if constexpr (GS || BND) { flux_up += blockIdx.y*part_stride; flux_dn += blockIdx.y*part_stride; }
    if constexpr (GS && JAC) flux_up_jac += blockIdx.y*part_stride;
    constexpr int CL = CLT, LL = 64/CLT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cl = lane & (CL-1), ll = lane / CL;
    const int h = wave % W, w0 = wave - h;
    // (a workgroup whose row segment is half a 128-B line: the other half belongs to the next workgroup -- rrx::xcd_contiguous)
    const int bx = ((NW/W)*CL*V*sizeof(F) < 128) ? xcd_contiguous(blockIdx.x, gridDim.x) : int(blockIdx.x);
    const int wave_col0 = (bx*(NW/W) + wave/W) * (CL*V);
    __shared__ F xch[4*V][NW][CL];
    __shared__ F xsum[OPT ? V : 1][NW][CL];              // OPT: each wave's sum of tau over its layers
    __shared__ F lds_b[LITE ? (2*K+1)*V : 1][64*NW];     // per-thread columns: B_lay[K], B_lev[K+1] of the current band
    constexpr bool ETAB = sizeof(F) == 8 && RRX_LW_EXP_TABLE;
    __shared__ F lds_etab[ETAB ? 64 : 1];
    if constexpr (ETAB) { exp_table_fill(lds_etab); __syncthreads(); }
    int icol = wave_col0 + cl*V;
    const bool active = icol < ncol;
    if (!active) icol = (wave_col0 < ncol) ? wave_col0 : 0;
    const bool writer = active && wave_col0 < ncol;
    const int nlev = nlay + 1;
    const size_t ncl = size_t(ncol);
    const int t0 = (h*LL + ll)*K;
    const F pi = F(3.14159265358979323846);
    const F tau_thres = sqrt(sqrt(Lim<F>::eps()));

    // g-point sums of the lane's K levels: in LDS columns for fp64 (the 4*K registers they would take push the kernel past 256
    // VGPRs into scratch; LDS has room for them at the two workgroups per CU the registers allow), in registers for fp32
    constexpr bool LACC = RRX_LW_LACC && ((sizeof(F) == 8 && V == 1) || (sizeof(F) == 4 && V == 2 && RRX_LW_LACC32));
    __shared__ F lds_acc[LACC ? 2*K*V : 1][64*NW];
    F acc_up[LACC ? 1 : K][V], acc_dn[LACC ? 1 : K][V];
    #pragma unroll
    for (int j=0; j<K; ++j)
        #pragma unroll
        for (int v=0; v<V; ++v)
        {
            if constexpr (LACC) { lds_acc[j*V+v][tid] = F(0.); lds_acc[(K+j)*V+v][tid] = F(0.); }
            else { acc_up[j][v] = F(0.); acc_dn[j][v] = F(0.); }
        }
    F acc_jc[JAC ? K : 1][V];
    if constexpr (JAC)
    {
        #pragma unroll
        for (int j=0; j<K; ++j)
            #pragma unroll
            for (int v=0; v<V; ++v) acc_jc[j][v] = F(0.);
    }

    // element offsets inside one g-point slab: sweep layer s = t0+j, sweep level t = t0+j (clamped into the domain)
    auto lay_off = [&](const int j) -> unsigned
    {
        const int sc = min(max(t0 + j, 0), nlay-1);
        return unsigned(top_at_1 ? sc : nlay-1-sc)*unsigned(ncol) + unsigned(icol);
    };
    auto lev_off = [&](const int j) -> unsigned
    {
        const int tc = min(t0 + j, nlay);
        return unsigned(top_at_1 ? tc : nlay-tc)*unsigned(ncol) + unsigned(icol);
    };

    struct Loads { Vec<F,V> a0[K], a1[K], a2[LITE ? 1 : K], x_next, x_prev, emis, ssrc, D, inc; };
    auto issue = [&](const int g, Loads& L, Vec<F,V>& J)
    {
        const F* __restrict__ t_g = tau + size_t(g)*ncl*nlay;
        const F* __restrict__ l_g = lay_source + size_t(g)*ncl*nlay;
        #pragma unroll
        for (int j=0; j<K; ++j) { const unsigned o = lay_off(j); L.a0[j] = load_cols<F,V>(t_g + o); L.a1[j] = load_cols<F,V>(l_g + o); }
        if constexpr (!LITE)
        {
            const F* __restrict__ v_g = lev_source + size_t(g)*ncl*nlev;
            #pragma unroll
            for (int j=0; j<K; ++j) L.a2[j] = load_cols<F,V>(v_g + lev_off(j));
            L.x_next = load_cols<F,V>(v_g + lev_off(K));          // level below the lane's last layer
        }
        else
        {
            L.x_next = load_cols<F,V>(l_g + lay_off(K));          // pfrac of the layer below the lane's last one
            L.x_prev = load_cols<F,V>(l_g + lay_off(-1));         // pfrac of the layer above the lane's first one
        }
        const size_t sfc = size_t(g)*ncl + icol;
        L.emis = load_cols<F,V>(sfc_emis + sfc); L.ssrc = load_cols<F,V>(sfc_src + sfc);
        if constexpr (!MU && !OPT) L.D = load_cols<F,V>(secants + sfc);
        if (inc_flux != nullptr) L.inc = load_cols<F,V>(inc_flux + sfc);
        if constexpr (JAC) J = load_cols<F,V>(sfc_src_jac + sfc);
    };

    Loads nxt;
    Vec<F,V> jnxt, jcur;                                        // sfc_src_jac of the next / current g-point (JAC only)
    if (!BND || g_lo < g_hi) issue(g_lo, nxt, jnxt);        // (an empty band prefetches nothing: g_lo may be ngpt)
    int cur_bnd = -1;
    const F wgt = weights[0];
    const F scale = pi * wgt;
    // MU: the secant of the next (g-point, angle) in sequence, one angle ahead; the surface values of the current g-point (they
    // are used behind the barrier where the prefetch overwrites the g-point); the angle's pi*weight
    Vec<F,V> d_next, c_emis, c_ssrc, c_inc;
    F scale_mu;
    if constexpr (MU) d_next = load_cols<F,V>(secants + size_t(g_lo)*ncl + icol);
    F fit1 = F(0.), fit2 = F(0.);                               // OPT: the band's two coefficients

#if RRX_LW_TIMING
    unsigned long long lw_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, lw_t = __builtin_readcyclecounter();
#endif
    for (int igpt=g_lo; igpt<g_hi; ++igpt)
    {
    RRX_LW_T(7)
    std::conditional_t<MU, Loads&, Loads> cur = nxt;            // MU: the g-point stays where it was loaded
    if constexpr (JAC) jcur = jnxt;
    if constexpr (MU) { c_emis = cur.emis; c_ssrc = cur.ssrc; c_inc = cur.inc; }

    if constexpr (LITE)
    {
        const int ib = gpoint_bands[igpt] - 1;                  // wave-uniform
        if (ib != cur_bnd)
        {
            cur_bnd = ib;
            const F* __restrict__ bl = blay + size_t(ib)*ncl*nlay;
            const F* __restrict__ bv = blev + size_t(ib)*ncl*nlev;
            #pragma unroll
            for (int j=0; j<K; ++j)
            {
                const Vec<F,V> x = load_cols<F,V>(bl + lay_off(j));
                #pragma unroll
                for (int v=0; v<V; ++v) lds_b[j*V+v][tid] = x.v[v];
            }
            #pragma unroll
            for (int j=0; j<=K; ++j)
            {
                const Vec<F,V> x = load_cols<F,V>(bv + lev_off(j));
                #pragma unroll
                for (int v=0; v<V; ++v) lds_b[(K+j)*V+v][tid] = x.v[v];
            }
            if constexpr (OPT) { fit1 = opt_fit[2*ib]; fit2 = opt_fit[2*ib+1]; }
        }
    }

    if constexpr (OPT)
    {
        F s[V];
        #pragma unroll
        for (int v=0; v<V; ++v) s[v] = F(0.);
        #pragma unroll
        for (int j=0; j<K; ++j)
        {
            const bool valid = (t0 + j) < nlay;
            #pragma unroll
            for (int v=0; v<V; ++v) s[v] += valid ? cur.a0[j].v[v] : F(0.);
        }
        #pragma unroll
        for (int d=1; d<LL; d<<=1)
            #pragma unroll
            for (int v=0; v<V; ++v) s[v] += shfl(s[v], lane ^ (d*CL));
        if (ll == 0)
        {
            #pragma unroll
            for (int v=0; v<V; ++v) xsum[v][wave][cl] = s[v];
        }
        RRX_LW_T(4)
        __syncthreads();       // (the next write of xsum lies behind both scan barriers of this g-point)
        #pragma unroll
        for (int v=0; v<V; ++v)
        {
            F t = F(0.);
            #pragma unroll
            for (int w=0; w<W; ++w) t += xsum[v][w0+w][cl];
            F e;
            if constexpr (ETAB) e = exp_neg(-t, lds_etab); else e = exp_neg(-t);
            cur.D.v[v] = fit1*e + fit2;
        }
        if (secants_out != nullptr && writer && ll == 0 && h == 0) store_cols<F,V>(secants_out + size_t(igpt)*ncl + icol, cur.D);
        RRX_LW_T(5)
    }

    // level source at sweep level t0+j for column v
    auto level_src = [&](const int j, const int v) -> F
    {
        if constexpr (!LITE) return (j < K) ? cur.a2[min(j, K-1)].v[v] : cur.x_next.v[v];
        else
        {
            const F pa = (j == 0) ? cur.x_prev.v[v] : cur.a1[max(j-1, 0)].v[v];
            const F pb = (j == K) ? cur.x_next.v[v] : cur.a1[min(j, K-1)].v[v];
            const F bvv = lds_b[(K+j)*V+v][tid];
            // The first and the last level take the fraction of their one layer (gas_optics_rrtmgp_kernels.cu:260-306). No select for
            // that (round 4; rounds 2-3 spent four v_cndmask per level on it): the loads of the neighbouring layer are clamped into the
            // column (lay_off), so there pa == pb and sqrt_nonneg(p*p) returns p -- the residual of its last Newton step is exact.
            return sqrt_nonneg(pa*pb) * bvv;
        }
    };

    int imu = 0;
    do      // the angles (one pass unless MU)
    {
    if constexpr (MU)
    {
        cur.D = d_next;
        scale_mu = pi * weights[imu];
        const bool last = imu == nmus-1;
        d_next = load_cols<F,V>(secants + (size_t(last ? 0 : imu + 1)*ngpt + (last ? min(igpt + 1, g_hi - 1) : igpt))*ncl + icol);
        // the Planck fractions are made opaque per angle, or the compiler hoists the angle-independent source terms out of this
        // loop and holds them: 2K+1 more registers per column, which the nine-layer forms do not have
        #pragma unroll
        for (int j=0; j<K; ++j)
            #pragma unroll
            for (int v=0; v<V; ++v) asm volatile("" : "+v"(cur.a1[j].v[v]));
        #pragma unroll
        for (int v=0; v<V; ++v) asm volatile("" : "+v"(cur.x_prev.v[v]), "+v"(cur.x_next.v[v]));
    }
    F tr[K][V], sdn[K][V], sup[K][V];
    F A[V], Bdn[V], Bup[V], lva[V];
    #pragma unroll
    for (int v=0; v<V; ++v) { A[v] = F(1.); Bdn[v] = F(0.); Bup[v] = F(0.); lva[v] = level_src(0, v); }
    #pragma unroll
    for (int j=0; j<K; ++j)
    {
        const bool valid = (t0 + j) < nlay;
        #pragma unroll
        for (int v=0; v<V; ++v)
        {
            F tvj = cur.a0[j].v[v];
            const int e = j*V + v - EV*V;                      // at most EV layers of evaluations in flight
            if (e >= 0) asm volatile("" : "+v"(tvj) : "v"(sup[e / V][e % V]));
            const F lvb = level_src(j+1, v);
            F lsj = cur.a1[j].v[v];
            if constexpr (LITE) lsj *= lds_b[j*V+v][tid];
            const F tau_loc = (valid ? tvj : F(0.)) * cur.D.v[v];      // padding layer: tau = 0 -> trans = 1, fact = 0, sources 0 (exactly)
            F trans;
            if constexpr (ETAB) trans = exp_neg(-tau_loc, lds_etab); else trans = exp_neg(-tau_loc);
            const F fact = tau_loc > tau_thres ? (F(1.) - trans) * fast_rcp(tau_loc) - trans
                                               : tau_loc * (F(.5) + tau_loc * (F(-1./3.) + tau_loc * F(1./8.)));
            const F omt = F(1.) - trans;
            const F s_dn = omt * lvb + F(2.) * fact * (lsj - lvb);
            const F s_up = omt * lva[v] + F(2.) * fact * (lsj - lva[v]);
            lva[v] = lvb;
            tr[j][v] = trans; sdn[j][v] = s_dn; sup[j][v] = s_up;
            Bdn[v] = tr[j][v]*Bdn[v] + sdn[j][v];
            Bup[v] += A[v]*sup[j][v];
            A[v] *= tr[j][v];
        }
    }

    RRX_LW_T(0)
    F dn_in[V], up_in[V], jc_in[V];
    #pragma unroll
    for (int v=0; v<V; ++v)
    {
        // ---- downward: inclusive scan over the level-lanes, then over the waves of the column group
        F a = A[v], b = Bdn[v];
        #pragma unroll
        for (int d=1; d<LL; d<<=1)
        {
            const F a2 = shfl(a, lane - d*CL), b2 = shfl(b, lane - d*CL);
            if (ll >= d) { b = a*b2 + b; a = a*a2; }
        }
        F xa = F(1.), xb = F(0.);
        if (ll == LL-1) { xch[4*v+0][wave][cl] = a; xch[4*v+1][wave][cl] = b; }
        RRX_LW_T(1)
        __syncthreads();
        RRX_LW_T(6)
        if (v == 0) if (!MU || imu == nmus-1)                  // (several angles: behind the first barrier of the last one)
        {
            // every wave of the workgroup is here: the waves that share 128-B lines ask for them together
            __builtin_amdgcn_sched_barrier(0);
            issue(min(igpt + 1, g_hi - 1), nxt, jnxt);      // (last iteration: a harmless re-read)
            __builtin_amdgcn_sched_barrier(0);
        }
        F fa = F(1.), fb = F(0.);
        #pragma unroll
        for (int w=0; w<W; ++w)
        {
            const F oa = xch[4*v+0][w0+w][cl], ob = xch[4*v+1][w0+w][cl];
            if (w == h) { xa = fa; xb = fb; }
            fb = oa*fb + ob; fa = oa*fa;
        }
        if (h > 0) { b = a*xb + b; a = a*xa; }
        F ae = shfl(a, lane - CL), be = shfl(b, lane - CL);
        if (ll == 0) { ae = xa; be = xb; }
        const F dn_top = (inc_flux != nullptr) ? (MU ? c_inc : cur.inc).v[v] / pi : F(0.);
        dn_in[v] = ae*dn_top + be;
        const F dn_sfc = fa*dn_top + fb;
        const F up_sfc = dn_sfc * (F(1.) - (MU ? c_emis : cur.emis).v[v]) + (MU ? c_emis : cur.emis).v[v] * (MU ? c_ssrc : cur.ssrc).v[v];

        // ---- upward: inclusive suffix scan
        a = A[v]; b = Bup[v];
        #pragma unroll
        for (int d=1; d<LL; d<<=1)
        {
            const F a2 = shfl(a, lane + d*CL), b2 = shfl(b, lane + d*CL);
            if (ll + d < LL) { b = a*b2 + b; a = a*a2; }
        }
        xa = F(1.); xb = F(0.);
        if (ll == 0) { xch[4*v+2][wave][cl] = a; xch[4*v+3][wave][cl] = b; }
        RRX_LW_T(2)
        __syncthreads();
        RRX_LW_T(6)
        #pragma unroll
        for (int w=W-1; w>=1; --w)
            if (w > h) { const F oa = xch[4*v+2][w0+w][cl], ob = xch[4*v+3][w0+w][cl]; xb = oa*xb + ob; xa = oa*xa; }
        if (h < W-1) { b = a*xb + b; a = a*xa; }
        ae = shfl(a, lane + CL); be = shfl(b, lane + CL);
        if (ll == LL-1) { ae = xa; be = xb; }
        up_in[v] = ae*up_sfc + be;
        if constexpr (JAC) jc_in[v] = ae * (MU ? c_emis : cur.emis).v[v] * jcur.v[v];
    }

    #pragma unroll
    for (int v=0; v<V; ++v)
    {
        F dn = dn_in[v];
        #pragma unroll
        for (int j=0; j<K; ++j)
        {
            if constexpr (LACC) { F a = lds_acc[(K+j)*V+v][tid]; add_rounded(a, (MU ? scale_mu : scale)*dn); lds_acc[(K+j)*V+v][tid] = a; }
            else add_rounded(acc_dn[j][v], (MU ? scale_mu : scale)*dn);
            dn = tr[j][v]*dn + sdn[j][v];
        }
        F up = up_in[v];
        #pragma unroll
        for (int j=K-1; j>=0; --j)
        {
            up = tr[j][v]*up + sup[j][v];
            if constexpr (LACC) { F a = lds_acc[j*V+v][tid]; add_rounded(a, (MU ? scale_mu : scale)*up); lds_acc[j*V+v][tid] = a; }
            else add_rounded(acc_up[j][v], (MU ? scale_mu : scale)*up);
        }
        if constexpr (JAC)
        {
            F jc = jc_in[v];
            #pragma unroll
            for (int j=K-1; j>=0; --j) { jc = tr[j][v]*jc; add_rounded(acc_jc[j][v], (MU ? scale_mu : scale)*jc); }
        }
    }
    RRX_LW_T(3)
    } while (MU && ++imu < nmus);
    }   // g-point loop
#if RRX_LW_TIMING
    if (lane == 0) for (int k=0; k<8; ++k) atomicAdd(&g_lw_clk[wave & 15][k], lw_acc[k]);
#endif

    if (!writer) return;
    #pragma unroll
    for (int j=0; j<K; ++j)
    {
        const int t = t0 + j;
        if (t <= nlay)
        {
            const size_t o = size_t(icol) + size_t(top_at_1 ? t : nlay - t)*ncl;
            Vec<F,V> u, d;
            #pragma unroll
            for (int v=0; v<V; ++v)
            {
                if constexpr (LACC) { u.v[v] = lds_acc[j*V+v][tid]; d.v[v] = lds_acc[(K+j)*V+v][tid]; }
                else { u.v[v] = acc_up[j][v]; d.v[v] = acc_dn[j][v]; }
            }
            store_cols<F,V>(flux_up + o, u);
            store_cols<F,V>(flux_dn + o, d);
            if constexpr (JAC)
            {
                Vec<F,V> jv;
                #pragma unroll
                for (int v=0; v<V; ++v) jv.v[v] = acc_jc[j][v];
                store_cols<F,V>(flux_up_jac + o, jv);
            }
        }
    }
}

// Any-nlay fallback: one thread per (col, gpt), layer quantities recomputed in the second sweep
// (no scratch). Used when nlay+1 > 8*K_MAX, and as the A/B baseline in bench.py --variant serial.
template<typename F, bool JAC, bool ACC>
__global__ void __launch_bounds__(256)
lw_noscat_serial_kernel(
        const int ncol, const int nlay, const int ngpt, const int top_at_1, const int imu,
        const F* __restrict__ secants, const F* __restrict__ weights,
        const F* __restrict__ tau, const F* __restrict__ lay_source, const F* __restrict__ lev_source,
        const F* __restrict__ sfc_emis, const F* __restrict__ sfc_src, const F* __restrict__ inc_flux,
        F* __restrict__ flux_up, F* __restrict__ flux_dn,
        const F* __restrict__ sfc_src_jac, F* __restrict__ flux_up_jac)
{
    const int icol = blockIdx.x*blockDim.x + threadIdx.x;
    const int igpt = blockIdx.y;
    if (icol >= ncol) return;

    const int nlev = nlay+1;
    const size_t ncl = size_t(ncol);
    const size_t lay_base = size_t(igpt)*ncl*nlay + icol;
    const size_t lev_base = size_t(igpt)*ncl*nlev + icol;
    const size_t sfc_idx = size_t(igpt)*ncl + icol;
    const F pi = F(3.14159265358979323846);
    const F tau_thres = sqrt(sqrt(Lim<F>::eps()));
    const F D = secants[sfc_idx + size_t(imu)*ncl*ngpt];
    const F scale = pi * weights[imu];

    auto layer = [&](const int s, F& trans, F& s_dn, F& s_up)
    {
        const int ml = top_at_1 ? s : nlay-1-s;
        const int m_above = top_at_1 ? ml : ml+1;
        const int m_below = top_at_1 ? ml+1 : ml;
        const F tau_loc = tau[lay_base + size_t(ml)*ncl] * D;
        const F ls = lay_source[lay_base + size_t(ml)*ncl];
        const F lev_above = lev_source[lev_base + size_t(m_above)*ncl];
        const F lev_below = lev_source[lev_base + size_t(m_below)*ncl];
        trans = exp(-tau_loc);
        const F fact = tau_loc > tau_thres ?
            (F(1.) - trans) / tau_loc - trans :
            tau_loc * (F(.5) + tau_loc * (F(-1./3.) + tau_loc * F(1./8.)));
        s_dn = (F(1.) - trans) * lev_below + F(2.) * fact * (ls - lev_below);
        s_up = (F(1.) - trans) * lev_above + F(2.) * fact * (ls - lev_above);
    };
    auto put = [&](F* arr, const int t, const F val)
    {
        const int ml = top_at_1 ? t : nlay - t;
        const size_t o = lev_base + size_t(ml)*ncl;
        arr[o] = ACC ? arr[o] + scale*val : scale*val;
    };

    F dn = (inc_flux != nullptr) ? inc_flux[sfc_idx] / pi : F(0.);
    for (int s=0; s<nlay; ++s)
    {
        F trans, s_dn, s_up;
        layer(s, trans, s_dn, s_up);
        put(flux_dn, s, dn);
        dn = trans*dn + s_dn;
    }
    put(flux_dn, nlay, dn);

    const F emis = sfc_emis[sfc_idx];
    F up = dn * (F(1.) - emis) + emis * sfc_src[sfc_idx];
    F jc = JAC ? emis * sfc_src_jac[sfc_idx] : F(0.);
    put(flux_up, nlay, up);
    if constexpr (JAC) put(flux_up_jac, nlay, jc);
    for (int s=nlay-1; s>=0; --s)
    {
        F trans, s_dn, s_up;
        layer(s, trans, s_dn, s_up);
        up = trans*up + s_up;
        put(flux_up, s, up);
        if constexpr (JAC) { jc = trans*jc; put(flux_up_jac, s, jc); }
    }
}


template<typename F>
__global__ void lw_secants_array_kernel(
        const int ncol, const int ngpt, const int n_gauss_quad, const int max_gauss_pts,
        const F* __restrict__ gauss_Ds, F* __restrict__ secants)
{
    const size_t n = size_t(ncol)*ngpt*n_gauss_quad;
    for (size_t i = size_t(blockIdx.x)*blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x)*blockDim.x)
    {
        const int imu = int(i / (size_t(ncol)*ngpt));
        secants[i] = gauss_Ds[imu + (n_gauss_quad-1)*max_gauss_pts];
    }
}


// Optimal-angle secants on their own (rrx_lw_optimal_secants; upstream's compute_optimal_angles): D(col, gpt) = fit(1,b)*exp(-S) +
// fit(2,b) with S the sum of tau(col, :, gpt) over the layers, added in layer-index order from zero; b = gpoint_bands(gpt). One pass
// over tau, the column on the lanes (128-B rows), one g-point per workgroup row. fit is (2, nbnd), first index fastest.
template<typename F>
__global__ void __launch_bounds__(256)
lw_optimal_secants_kernel(
        const int ncol, const int nlay, const int* __restrict__ gpoint_bands, const F* __restrict__ fit,
        const F* __restrict__ tau, F* __restrict__ secants)
{
    const int icol = blockIdx.x*blockDim.x + threadIdx.x;
    const int igpt = blockIdx.y;
    if (icol >= ncol) return;
    const size_t ncl = size_t(ncol);
    const F* __restrict__ t = tau + size_t(igpt)*ncl*nlay + icol;
    F s = F(0.);
    #pragma unroll 8
    for (int ilay=0; ilay<nlay; ++ilay) s += t[size_t(ilay)*ncl];
    const int ib = gpoint_bands[igpt] - 1;
    secants[size_t(igpt)*ncl + icol] = fit[2*ib] * exp(-s) + fit[2*ib+1];
}

template<typename F>
int lw_optimal_secants_impl(const int ncol, const int nlay, const int ngpt, const int nbnd, const int* gpoint_bands,
                            const F* optimal_angle_fit, const F* tau, F* secants, void* stream)
{
    const char* entry = "rrx_lw_optimal_secants";
    const char* bad = nullptr;
    if (ncol <= 0) bad = "ncol must be positive";
    else if (nlay <= 0) bad = "nlay must be positive";
    else if (ngpt <= 0 || ngpt > 65535) bad = "ngpt must be 1..65535";
    else if (nbnd <= 0) bad = "nbnd must be positive";
    else if (gpoint_bands == nullptr) bad = "gpoint_bands is null";
    else if (optimal_angle_fit == nullptr) bad = "optimal_angle_fit is null";
    else if (tau == nullptr) bad = "tau is null";
    else if (secants == nullptr) bad = "secants is null";
    if (bad != nullptr) { set_error(std::string(entry) + ": " + bad); return 1; }
    RRX_TRY
    lw_optimal_secants_kernel<F><<<dim3(ceil_div(ncol, 256), ngpt), 256, 0, static_cast<hipStream_t>(stream)>>>(
            ncol, nlay, gpoint_bands, optimal_angle_fit, tau, secants);
    RRX_CATCH(entry)
}

// the general kernel for one quadrature angle; false when the columns are taller than its largest K (the caller takes the serial
// kernel)
template<typename F, int V>
bool launch_scan(
        hipStream_t st, const bool jac, const bool acc,
        const int ncol, const int nlay, const int ngpt, const int top_at_1, const int imu,
        const F* secants, const F* weights, const F* tau, const F* lay_source, const F* lev_source,
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up, F* flux_dn,
        const F* sfc_src_jac, F* flux_up_jac)
{
    const dim3 grid(ceil_div(ncol, 2*CL*V), ngpt);        // two column groups of two waves per workgroup
    const int sync_waves = tuning().sync_waves;
    return with_k<2, 4, 6, 9, 12, 17>(ceil_div(nlay+1, 2*LL), [&](auto kk)
    {
        with_flag(jac, [&](auto j) { with_flag(acc, [&](auto a)
        {
            lw_noscat_scan_kernel<F,V,decltype(kk)::value,decltype(j)::value,decltype(a)::value><<<grid, 256, 0, st>>>(
                ncol, nlay, ngpt, top_at_1, imu, secants, weights, tau, lay_source, lev_source,
                sfc_emis, sfc_src, inc_flux, flux_up, flux_dn, sfc_src_jac, flux_up_jac, sync_waves);
        }); });
    });
}

// the arguments of the fused broadband forms, the same for every tiling that lw_fused_broadband tries
template<typename F>
struct BbArgs
{
    int ncol, nlay, ngpt, top_at_1;
    const F *secants, *weights, *tau, *lay_source /* or pfrac */, *lev_source, *blay, *blev;
    const int* gpoint_bands;
    const F *sfc_emis, *sfc_src, *inc_flux;
    F *flux_up, *flux_dn;
    // what is given below chooses the form (lw_fractions_solve)
    const F* sfc_src_jac = nullptr; F* flux_up_jac = nullptr;      // JAC: (ngpt, ncol) in, (ncol, nlev) out
    int nmus = 1;                                                   // MU: quadrature angles; secants (ncol, ngpt, nmus), weights (nmus)
    const F* opt_fit = nullptr; F* secants_out = nullptr;          // OPT: fit (2, nbnd) in, the secants used (ncol, ngpt) out or null
    const int* band_lims = nullptr; int nbnd = 0;                  // by-band form: flux_up/dn are (ncol, nlev, nbnd) band sums (OPT: nbnd of the fit)
};

// one tiling of the fused broadband kernel (lw_noscat_bb_kernel); false when the shape is outside it (the caller tries the next one).
// LITE: lay_source = pfrac, lev_source unused. JAC: the Jacobian form, in the geometry and g-point split the fluxes alone would take
// (so they come out bit for bit the same). MU: the several-angle form (a.nmus angles), same geometry and split again. OPT: the
// optimal-angle form, same geometry and split again.
template<typename F, int V, int W, int CLT, bool LITE, int NW, bool JAC, bool MU, bool OPT = false>
bool launch_bb2(hipStream_t st, const BbArgs<F>& a)
{
    static_assert(!MU || LITE, "several angles: Planck-lite inputs only");
    static_assert(!OPT || (LITE && !MU), "optimal angles: Planck-lite inputs, one angle");
    if (size_t(a.ncol)*(a.nlay+1) >= (size_t(1) << 31)) return false;      // 32-bit element offsets inside a g-point slab
    const int groups = ceil_div(a.ncol, (NW/W)*CLT*V);
    const int need = ceil_div(a.nlay+1, (64/CLT)*W);
    auto with_tiling_k = [&](auto launch)      // the layers per lane of this tiling
    {
        if constexpr (CLT == 16) return with_k<2, 4, 6, 9>(need, launch);
        else if constexpr (W == 8) return with_k<5, 7, 9>(need, launch);      // (288 ... 319 / 447 / 575 layers: eight waves of 8 x 8 lanes)
        else return with_k<2, 3, 5>(need, launch);
    };
    const size_t nlevcol = size_t(a.ncol)*(a.nlay+1);
    if (!JAC && !MU && !OPT && a.band_lims != nullptr)
    {
        // one band per workgroup (grid.y = band): no store inside the g-point loop, no partial arrays, no allocation. Planck-lite
        // inputs only (the by-band entry is rrx_lw_solver_noscat_fractions_byband).
        if constexpr (LITE)
        {
            const dim3 grid(groups, a.nbnd);
            return with_tiling_k([&](auto kk)
            {
                lw_noscat_bb_kernel<F,V,decltype(kk)::value,W,CLT,LITE,false,RRX_LW_EV,NW,true><<<grid, 64*NW, 0, st>>>(
                    a.ncol, a.nlay, a.ngpt, a.top_at_1, a.secants, a.weights, a.tau, a.lay_source, a.lev_source, a.blay, a.blev,
                    a.gpoint_bands, a.sfc_emis, a.sfc_src, a.inc_flux, a.flux_up, a.flux_dn, 0, nlevcol, a.band_lims);
            });
        }
        return false;
    }
    // few column groups: the g-point loop is split over grid.y (rrx::launch_gsplit; one or two workgroups per CU)
    return launch_gsplit<F,(JAC ? 3 : 2)>(st, groups, a.ngpt, (NW > 4) ? 256 : 512, nlevcol, a.flux_up, a.flux_dn, a.flux_up_jac, with_tiling_k,
        [&](auto kk, auto gs, const dim3 grid, const int gper, F* out_up, F* out_dn, F* out_jc)
    {
        lw_noscat_bb_kernel<F,V,decltype(kk)::value,W,CLT,LITE,decltype(gs)::value,RRX_LW_EV,NW,false,JAC,MU,OPT><<<grid, 64*NW, 0, st>>>(
            a.ncol, a.nlay, a.ngpt, a.top_at_1, a.secants, a.weights, a.tau, a.lay_source, a.lev_source, a.blay, a.blev,
            a.gpoint_bands, a.sfc_emis, a.sfc_src, a.inc_flux, out_up, out_dn, gper, nlevcol, nullptr, a.sfc_src_jac, out_jc,
            MU ? a.nmus : 1, OPT ? a.opt_fit : nullptr, OPT ? a.secants_out : nullptr);
    });
}

// broadband fluxes from tau + (lay_source, lev_source) [LITE = false] or tau + Planck fractions and band Planck functions
// [LITE = true] in the one-kernel form; false when the shape is outside its tilings (the caller takes another path)
// [JAC = true: flux_up_jac too, from the same forms in the same order; MU = true: nmus angles, secants (ncol, ngpt, nmus);
//  OPT = true: secants formed in the kernel from opt_fit (2, nbnd), written to secants_out when it is given]
template<typename F, bool LITE, bool JAC = false, bool MU = false, bool OPT = false>
bool lw_fused_broadband(hipStream_t st, const BbArgs<F>& a)
{
    if constexpr (sizeof(F) == 8)
    {
        // (Round 4 measured six waves x six layers per column group -- 384-thread workgroups, three waves per SIMD, 168 VGPRs with
        //  108-124 B of scratch: 4.2-4.7 ms against 2.7 for this form, profiles/r04_fp32_geometry_ab.txt.)
        if (launch_bb2<F,1,4,16,LITE,4,JAC,MU,OPT>(st, a)) return true;
        // 144 ... 287 layers: eight wavefronts per column group
        if (launch_bb2<F,1,8,16,LITE,8,JAC,MU,OPT>(st, a)) return true;
        // 288 ... 575 layers (round 4: RCEMIP's default is 256 levels, LES grids with a background profile on top exceed 288): the same
        // eight waves with 8 x 8 lanes -- 64 levels per wave at nine layers per lane, 64-B rows (the other half of each 128-B line
        // belongs to the next column group: twice the L2 fetches, on a kernel that stands at a quarter of the HBM roof). Beyond that
        // the one-thread-per-column kernels take over.
        return launch_bb2<F,1,8,8,LITE,8,JAC,MU,OPT>(st, a);
    }
    else
    {
        // one column per lane, two column groups per workgroup, four waves per SIMD (variant 15 = the forms of rounds 1-3)
        // Round 4 measured the one-column-per-lane geometries of the SW solver here too (K = 9 / W = 4 at two waves per SIMD, K = 6 /
        // W = 6 at three, K = 5 / W = 8 at four: 1.82 / 1.88 / 1.95 ms at C4 against 1.31 for two columns per lane with the sums in
        // LDS, profiles/r04_fp32_geometry_ab.txt): the LW chain per g-point is short, so halving the wavefronts per column wins.
        // The one-column form stays for odd column counts (variant 15 forces it for tests).
        if (tuning().lw_variant == 15 && launch_bb2<F,1,4,16,LITE,8,JAC,MU,OPT>(st, a)) return true;
        // 16 x 4 lanes with two columns per lane (128-B rows, K = 9) ahead of 8 x 8 lanes with four. Measured at C4 in the fractions
        // form: 1.77 against 3.26 ms (the four-column lane state spills); the latter still takes 144 ... 159 layers.
        if (a.ncol % 2 == 0 && launch_bb2<F,2,4,16,LITE,4,JAC,MU,OPT>(st, a)) return true;
        if (a.ncol % 4 == 0 && launch_bb2<F,4,4,8,LITE,4,JAC,MU,OPT>(st, a)) return true;
        // 144 ... 287 layers: eight wavefronts per column group
        if (a.ncol % 2 == 0 && launch_bb2<F,2,8,16,LITE,8,JAC,MU,OPT>(st, a)) return true;
        // 288 ... 575 layers: eight waves of 8 x 8 lanes (see fp64)
        if (a.ncol % 2 == 0 && launch_bb2<F,2,8,8,LITE,8,JAC,MU,OPT>(st, a)) return true;
        // odd column counts: one column per lane
        return launch_bb2<F,1,4,16,LITE,8,JAC,MU,OPT>(st, a);
    }
}

#define RRX_LW_ARGS_CALL ncol, nlay, ngpt, top_at_1, imu, secants, weights, tau, lay_source, lev_source, \
        sfc_emis, sfc_src, inc_flux, up, dn, sfc_src_jac, flux_up_jac

template<typename F>
int lw_solver_noscat_impl(
        const int ncol, const int nlay, const int ngpt, const Bool top_at_1, const int nmus,
        const F* secants, const F* weights,
        const F* tau, const F* lay_source, const F* lev_source,
        const F* sfc_emis, const F* sfc_src, const F* inc_flux,
        F* flux_up, F* flux_dn,
        const Bool do_broadband, F* flux_up_loc, F* flux_dn_loc,
        const Bool do_jacobians, const F* sfc_src_jac, F* flux_up_jac,
        void* stream)
{
    RRX_TRY
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ncol <= 0 || nlay <= 0 || ngpt <= 0) throw std::runtime_error("empty problem");
    if (nmus < 1 || nmus > 4) throw std::runtime_error("n_quad_angs must be 1..4");
    if (do_broadband && (flux_up_loc == nullptr || flux_dn_loc == nullptr)) throw std::runtime_error("do_broadband needs flux_*_loc");
    const bool jac = do_jacobians && sfc_src_jac != nullptr && flux_up_jac != nullptr;
    const int variant = tuning().lw_variant;

    // broadband mode, fused form: g-point sums kept on chip, no per-g-point fluxes in memory. With enough column groups
    // to fill the chip one workgroup sums all g-points in order (sum_broadband's order); with fewer the g-point range is split
    // over grid.y and the partial sums are added in range order (rrx::broadband_gsplit).
    if (do_broadband && !jac && nmus == 1 && lw_fused_allowed() &&
        lw_fused_broadband<F,false>(st, BbArgs<F>{ncol, nlay, ngpt, top_at_1, secants, weights, tau, lay_source, lev_source, nullptr, nullptr,
                                                  nullptr, sfc_emis, sfc_src, inc_flux, flux_up_loc, flux_dn_loc}))
        return 0;

    // broadband mode, general form: per-g-point fluxes go to a workspace, then are summed over g-points
    F* up = flux_up; F* dn = flux_dn;
    WorkspaceLease lease(st);
    const size_t nlevcol = size_t(ncol)*(nlay+1);
    if (do_broadband) { up = lease.get<F>(2*nlevcol*ngpt); dn = up + nlevcol*ngpt; }

    // columns per lane: VDEF*8 lanes*sizeof(F) = 64-B row segments, VMAX = 128-B segments. Measured at C4 (tools/
    // bench_solvers.py): two waves per column group with 128-B rows (2 waves/SIMD) is the fastest form in both
    // precisions (fp64 5.4 ms vs 6.0 ms for one wave/64-B rows; fp32 2.4 vs 2.9 ms); variant 4 keeps 64-B rows.
    constexpr int VDEF = (sizeof(F) == 8) ? 1 : 2;
    constexpr int VMAX = 2*VDEF;
    for (int imu=0; imu<nmus; ++imu)
    {
        const bool acc = imu > 0;
        bool done = false;
        if (variant != 1)
        {
            if (variant != 4 && ncol % VMAX == 0) done = launch_scan<F,VMAX>(st, jac, acc, RRX_LW_ARGS_CALL);
            else if (ncol % VDEF == 0)            done = launch_scan<F,VDEF>(st, jac, acc, RRX_LW_ARGS_CALL);
            if (!done)                            done = launch_scan<F,1>(st, jac, acc, RRX_LW_ARGS_CALL);
        }
        if (!done)      // beyond the general kernel's largest K, or variant 1
        {
            const dim3 grid(ceil_div(ncol, 256), ngpt);
            with_flag(jac, [&](auto j) { with_flag(acc, [&](auto a)
            {
                lw_noscat_serial_kernel<F,decltype(j)::value,decltype(a)::value><<<grid, 256, 0, st>>>(RRX_LW_ARGS_CALL);
            }); });
        }
    }

    if (do_broadband)
    {
        const int nb = ceil_div(nlevcol, 256);
        sum_gpt_kernel<F><<<nb, 256, 0, st>>>(nlevcol, ngpt, up, flux_up_loc);
        sum_gpt_kernel<F><<<nb, 256, 0, st>>>(nlevcol, ngpt, dn, flux_dn_loc);
    }
    RRX_CATCH("rrx_lw_solver_noscat")
}
#undef RRX_LW_ARGS_CALL

template<typename F>
__global__ void planck_sources_from_fractions_kernel(
        const int ncol, const int nlay, const int ngpt, const int* __restrict__ gpoint_bands,
        const F* __restrict__ pf, const F* __restrict__ blay, const F* __restrict__ blev,
        F* __restrict__ lay_src, F* __restrict__ lev_src)
{
    // lay_source = pfrac*B_lay; lev_source(level m) = sqrt(pfrac(m)*pfrac(m-1))*B_lev(m), first / last level pfrac*B_lev:
    // the expressions (and rounding) of Planck_source_kernel, gas_optics_rrtmgp_kernels.cu:260-306
    const size_t ncl = ncol; const int nlev = nlay+1;
    const size_t n = ncl*nlev*ngpt;
    for (size_t i = size_t(blockIdx.x)*blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x)*blockDim.x)
    {
        const int icol = int(i % ncl), m = int((i / ncl) % nlev), ig = int(i / (ncl*nlev));
        const int ib = gpoint_bands[ig] - 1;
        const size_t lb = size_t(ig)*ncl*nlay + icol;
        const F bl = blev[(size_t(ib)*nlev + m)*ncl + icol];
        F v;
        if (m == 0) v = pf[lb] * bl;
        else if (m == nlay) v = pf[lb + size_t(nlay-1)*ncl] * bl;
        else v = sqrt(pf[lb + size_t(m)*ncl] * pf[lb + size_t(m-1)*ncl]) * bl;
        lev_src[i] = v;
        if (m < nlay) lay_src[lb + size_t(m)*ncl] = pf[lb + size_t(m)*ncl] * blay[(size_t(ib)*nlay + m)*ncl + icol];
    }
}

template<typename F>
int planck_sources_from_fractions_impl(int ncol, int nlay, int ngpt, const int* gpoint_bands, const F* pfrac, const F* blay,
        const F* blev, F* lay_src, F* lev_src, void* stream)
{
    RRX_TRY
    if (ncol <= 0 || nlay <= 0 || ngpt <= 0) throw std::runtime_error("empty problem");
    const size_t n = size_t(ncol)*(nlay+1)*ngpt;
    planck_sources_from_fractions_kernel<F><<<int(std::min<size_t>((n + 255)/256, 256*16)), 256, 0, static_cast<hipStream_t>(stream)>>>(
            ncol, nlay, ngpt, gpoint_bands, pfrac, blay, blev, lay_src, lev_src);
    RRX_CATCH("rrx_planck_sources_from_fractions")
}

// The fractions entries outside the one-kernel tilings (columns taller than 575 layers, variants 1 and 7): the Planck sources are
// rebuilt and the general entry writes per-g-point fluxes [up | dn], and the Jacobian behind them when a.sfc_src_jac is given, into ONE
// lease of the stream's workspace: [up | dn | (Jacobian) | lay_source | lev_source]. Returns that block, or null with the message set;
// the caller sums it while the lease lives. With a.opt_fit the secants are the optimal-angle ones (one angle), produced by
// lw_optimal_secants_kernel into a.secants_out or, when that is null, into (ncol, ngpt) more elements at the end of the lease.
template<typename F>
const F* lw_fractions_per_gpoint(WorkspaceLease& lease, const BbArgs<F>& a, void* stream)
{
    const size_t n_lay = size_t(a.ncol)*a.nlay*a.ngpt, n_lev = size_t(a.ncol)*(a.nlay+1)*a.ngpt;
    const size_t nout = (a.sfc_src_jac != nullptr) ? 3 : 2;
    const size_t n_sec = (a.opt_fit != nullptr && a.secants_out == nullptr) ? size_t(a.ncol)*a.ngpt : 0;
    F* ws = lease.get<F>(nout*n_lev + n_lay + n_lev + n_sec);
    F* lay = ws + nout*n_lev; F* lev = lay + n_lay;
    F* jac = (a.sfc_src_jac != nullptr) ? ws + 2*n_lev : nullptr;
    const F* secants = a.secants;
    if (a.opt_fit != nullptr)
    {
        F* sec = (a.secants_out != nullptr) ? a.secants_out : lev + n_lev;
        if (lw_optimal_secants_impl<F>(a.ncol, a.nlay, a.ngpt, a.nbnd, a.gpoint_bands, a.opt_fit, a.tau, sec, stream) != 0) return nullptr;
        secants = sec;
    }
    if (planck_sources_from_fractions_impl<F>(a.ncol, a.nlay, a.ngpt, a.gpoint_bands, a.lay_source, a.blay, a.blev, lay, lev, stream) != 0 ||
        lw_solver_noscat_impl<F>(a.ncol, a.nlay, a.ngpt, a.top_at_1, a.nmus, secants, a.weights, a.tau, lay, lev, a.sfc_emis, a.sfc_src,
                                 a.inc_flux, ws, ws + n_lev, Bool(0), (F*)nullptr, (F*)nullptr, Bool(jac != nullptr), a.sfc_src_jac, jac,
                                 stream) != 0)
        return nullptr;
    return ws;
}

// The solve behind the five fractions entries (plain, _jac, _angles, _optimal, _byband), their argument checks done; a.lay_source is
// pfrac. What the struct holds chooses the form: the Jacobian pair -> JAC; nmus > 1 -> MU (one angle through the _angles entry is the
// one-angle form: the same bits); opt_fit -> OPT; band_lims -> the by-band form, a.flux_up / a.flux_dn being the band sums. Exactly
// these instantiations exist: JAC x {one angle, MU, OPT}, and the by-band form without the other three. The one-kernel form where the
// variant allows it and a tiling reaches; otherwise the g-point sums (band sums) of lw_fractions_per_gpoint's fluxes and Jacobian,
// which the general kernel has added up over the angles. False: the message is set.
template<typename F>
bool lw_fractions_solve(void* stream, const BbArgs<F>& a)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool jac = a.sfc_src_jac != nullptr;
    bool fused = false;
    if (lw_fused_allowed() && a.band_lims != nullptr) fused = lw_fused_broadband<F,true>(st, a);
    else if (lw_fused_allowed()) with_flag(jac, [&](auto j)
    {
        constexpr bool JAC = decltype(j)::value;
        if (a.opt_fit != nullptr) fused = lw_fused_broadband<F,true,JAC,false,true>(st, a);
        else if (a.nmus > 1)      fused = lw_fused_broadband<F,true,JAC,true>(st, a);
        else                      fused = lw_fused_broadband<F,true,JAC>(st, a);
    });
    if (fused) return true;

    WorkspaceLease lease(st);
    const F* ws = lw_fractions_per_gpoint<F>(lease, a, stream);
    if (ws == nullptr) return false;
    const size_t nlevcol = size_t(a.ncol)*(a.nlay+1);
    const int nb = ceil_div(nlevcol, 256);
    if (a.band_lims != nullptr)
        sum_bands_kernel<F><<<dim3(nb, a.nbnd, 2), 256, 0, st>>>(nlevcol, a.ngpt, a.band_lims, ws, a.flux_up, a.flux_dn, (F*)nullptr);
    else
    {
        sum_gpt_kernel<F><<<nb, 256, 0, st>>>(nlevcol, a.ngpt, ws, a.flux_up);
        sum_gpt_kernel<F><<<nb, 256, 0, st>>>(nlevcol, a.ngpt, ws + nlevcol*a.ngpt, a.flux_dn);
        if (jac) sum_gpt_kernel<F><<<nb, 256, 0, st>>>(nlevcol, a.ngpt, ws + 2*nlevcol*a.ngpt, a.flux_up_jac);
    }
    return true;
}

template<typename F>
int lw_solver_noscat_fractions_impl(
        const int ncol, const int nlay, const int ngpt, const Bool top_at_1,
        const F* secants, const F* weights, const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands,
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up_loc, F* flux_dn_loc, void* stream)
{
    RRX_TRY
    if (ncol <= 0 || nlay <= 0 || ngpt <= 0) throw std::runtime_error("empty problem");
    if (flux_up_loc == nullptr || flux_dn_loc == nullptr) throw std::runtime_error("broadband outputs missing");
    if (!lw_fractions_solve<F>(stream, {ncol, nlay, ngpt, top_at_1, secants, weights, tau, pfrac, nullptr, blay, blev, gpoint_bands,
                                        sfc_emis, sfc_src, inc_flux, flux_up_loc, flux_dn_loc}))
        return 1;                                                    // (the message is set)
    RRX_CATCH("rrx_lw_solver_noscat_fractions")
}

// fluxes and the surface-temperature Jacobian of the upward flux (rrx_lw_solver_noscat_fractions_jac)
template<typename F>
int lw_solver_noscat_fractions_jac_impl(
        const int ncol, const int nlay, const int ngpt, const Bool top_at_1,
        const F* secants, const F* weights, const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands,
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, const F* sfc_src_jac, F* flux_up_loc, F* flux_dn_loc, F* flux_up_jac,
        void* stream)
{
    RRX_TRY
    if (ncol <= 0 || nlay <= 0 || ngpt <= 0) throw std::runtime_error("empty problem");
    if (flux_up_loc == nullptr || flux_dn_loc == nullptr) throw std::runtime_error("broadband outputs missing");
    if (sfc_src_jac == nullptr) throw std::runtime_error("sfc_src_jac is null");
    if (flux_up_jac == nullptr) throw std::runtime_error("flux_up_jac is null");
    if (!lw_fractions_solve<F>(stream, {ncol, nlay, ngpt, top_at_1, secants, weights, tau, pfrac, nullptr, blay, blev, gpoint_bands,
                                        sfc_emis, sfc_src, inc_flux, flux_up_loc, flux_dn_loc, sfc_src_jac, flux_up_jac}))
        return 1;                                                    // (the message is set)
    RRX_CATCH("rrx_lw_solver_noscat_fractions_jac")
}

// nmus = 1..4 quadrature angles (rrx_lw_solver_noscat_fractions_angles), with the Jacobian when the pair is given
template<typename F>
int lw_solver_noscat_fractions_angles_impl(
        const int ncol, const int nlay, const int ngpt, const Bool top_at_1, const int nmus,
        const F* secants, const F* weights, const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands,
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up_loc, F* flux_dn_loc, const F* sfc_src_jac, F* flux_up_jac,
        void* stream)
{
    const char* entry = "rrx_lw_solver_noscat_fractions_angles";
    const char* bad = nullptr;
    if (nmus < 1 || nmus > 4) bad = "nmus must be 1..4";
    else if (ncol <= 0) bad = "ncol must be positive";
    else if (nlay <= 0) bad = "nlay must be positive";
    else if (ngpt <= 0) bad = "ngpt must be positive";
    else if (secants == nullptr || weights == nullptr) bad = "secants / weights missing";
    else if (flux_up_loc == nullptr) bad = "flux_up_loc is null";
    else if (flux_dn_loc == nullptr) bad = "flux_dn_loc is null";
    else if (sfc_src_jac != nullptr && flux_up_jac == nullptr) bad = "flux_up_jac is null while sfc_src_jac is given";
    else if (sfc_src_jac == nullptr && flux_up_jac != nullptr) bad = "sfc_src_jac is null while flux_up_jac is given";
    if (bad != nullptr) { set_error(std::string(entry) + ": " + bad); return 1; }
    RRX_TRY
    if (!lw_fractions_solve<F>(stream, {ncol, nlay, ngpt, top_at_1, secants, weights, tau, pfrac, nullptr, blay, blev, gpoint_bands,
                                        sfc_emis, sfc_src, inc_flux, flux_up_loc, flux_dn_loc, sfc_src_jac, flux_up_jac, nmus}))
        return 1;                                                    // (the message is set)
    RRX_CATCH(entry)
}

// One angle whose secant is the optimal-angle fit of the column's total optical depth (rrx_lw_solver_noscat_fractions_optimal), with
// the Jacobian when the pair is given
template<typename F>
int lw_solver_noscat_fractions_optimal_impl(
        const int ncol, const int nlay, const int ngpt, const int nbnd, const Bool top_at_1, const F* weights,
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, const F* optimal_angle_fit,
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up_loc, F* flux_dn_loc, const F* sfc_src_jac, F* flux_up_jac,
        F* secants_out, void* stream)
{
    const char* entry = "rrx_lw_solver_noscat_fractions_optimal";
    const char* bad = nullptr;
    if (ncol <= 0) bad = "ncol must be positive";
    else if (nlay <= 0) bad = "nlay must be positive";
    else if (ngpt <= 0 || ngpt > 65535) bad = "ngpt must be 1..65535";
    else if (nbnd <= 0) bad = "nbnd must be positive";
    else if (weights == nullptr) bad = "weights is null";
    else if (gpoint_bands == nullptr) bad = "gpoint_bands is null";
    else if (optimal_angle_fit == nullptr) bad = "optimal_angle_fit is null";
    else if (flux_up_loc == nullptr) bad = "flux_up_loc is null";
    else if (flux_dn_loc == nullptr) bad = "flux_dn_loc is null";
    else if (sfc_src_jac != nullptr && flux_up_jac == nullptr) bad = "flux_up_jac is null while sfc_src_jac is given";
    else if (sfc_src_jac == nullptr && flux_up_jac != nullptr) bad = "sfc_src_jac is null while flux_up_jac is given";
    if (bad != nullptr) { set_error(std::string(entry) + ": " + bad); return 1; }
    RRX_TRY
    if (!lw_fractions_solve<F>(stream, {ncol, nlay, ngpt, top_at_1, nullptr, weights, tau, pfrac, nullptr, blay, blev, gpoint_bands,
                                        sfc_emis, sfc_src, inc_flux, flux_up_loc, flux_dn_loc, sfc_src_jac, flux_up_jac, 1,
                                        optimal_angle_fit, secants_out, nullptr, nbnd}))
        return 1;                                                    // (the message is set)
    RRX_CATCH(entry)
}

// host-model update between radiation calls (rrx_lw_flux_up_adjust): d = jac * (t_new - t_old) of the level's column;
// flux_up += d, flux_net -= d
template<typename F>
__global__ void lw_flux_up_adjust_kernel(const size_t n, const int ncol, const F* __restrict__ jac, const F* __restrict__ t_old,
                                         const F* __restrict__ t_new, F* __restrict__ flux_up, F* __restrict__ flux_net)
{
    const size_t i = size_t(blockIdx.x)*blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int icol = int(i % size_t(ncol));
    const F d = jac[i] * (t_new[icol] - t_old[icol]);
    flux_up[i] += d;
    if (flux_net != nullptr) flux_net[i] -= d;
}

template<typename F>
int lw_flux_up_adjust_impl(const int ncol, const int nlev, const F* flux_up_jac, const F* t_sfc_old, const F* t_sfc_new,
                           F* flux_up, F* flux_net, void* stream)
{
    RRX_TRY
    if (ncol <= 0 || nlev <= 0) throw std::runtime_error("empty problem");
    if (flux_up_jac == nullptr) throw std::runtime_error("flux_up_jac is null");
    if (t_sfc_old == nullptr || t_sfc_new == nullptr) throw std::runtime_error("surface temperatures missing");
    if (flux_up == nullptr) throw std::runtime_error("flux_up is null");
    const size_t n = size_t(ncol)*nlev;
    lw_flux_up_adjust_kernel<F><<<ceil_div(n, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(n, ncol, flux_up_jac, t_sfc_old, t_sfc_new,
                                                                                                 flux_up, flux_net);
    RRX_CATCH("rrx_lw_flux_up_adjust")
}

// by-band fluxes (rrx_lw_solver_noscat_fractions_byband). Band net and broadband outputs come from the band sums in one more pass.
template<typename F>
int lw_solver_noscat_fractions_byband_impl(
        const int ncol, const int nlay, const int ngpt, const int nbnd, const Bool top_at_1,
        const F* secants, const F* weights, const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands,
        const int* band_lims, const F* sfc_emis, const F* sfc_src, const F* inc_flux,
        F* bnd_up, F* bnd_dn, F* bnd_net, F* flux_up, F* flux_dn, void* stream)
{
    RRX_TRY
    check_byband_args(ncol, nlay, ngpt, nbnd, band_lims);
    if (gpoint_bands == nullptr) throw std::runtime_error("gpoint_bands is null");
    if (bnd_up == nullptr || bnd_dn == nullptr) throw std::runtime_error("band flux outputs missing");
    if (!lw_fractions_solve<F>(stream, {ncol, nlay, ngpt, top_at_1, secants, weights, tau, pfrac, nullptr, blay, blev, gpoint_bands,
                                        sfc_emis, sfc_src, inc_flux, bnd_up, bnd_dn, nullptr, nullptr, 1, nullptr, nullptr, band_lims, nbnd}))
        return 1;                                                    // (the message is set)
    launch_byband_outputs<F,2>(static_cast<hipStream_t>(stream), size_t(ncol)*(nlay+1), nbnd, bnd_up, bnd_dn, (const F*)nullptr,
                               bnd_net, flux_up, flux_dn, (F*)nullptr);
    RRX_CATCH("rrx_lw_solver_noscat_fractions_byband")
}

// The math primitives of rrx_common.h applied element-wise (rrx_math_selftest), so that a test can measure on the device what their
// comments claim: y[i] = f(x[i]) with f chosen by `which`. Compiled in this file, i.e. under the solver's contraction mode; the table
// form reads a table that exp_table_fill wrote to LDS behind a barrier, as lw_noscat_bb_kernel does.
enum MathPrimitive { MATH_EXP_NEG = 0, MATH_EXP_NEG_TABLE = 1, MATH_FAST_RCP = 2, MATH_SQRT_POS = 3, MATH_SQRT_NONNEG = 4, MATH_COUNT = 5 };

template<typename F>
__global__ void __launch_bounds__(256)
math_selftest_kernel(const int which, const size_t n, const F* __restrict__ x, F* __restrict__ y)
{
    constexpr bool ETAB = sizeof(F) == 8;                // (fp32: the table form forwards to the fp32 exp_neg)
    __shared__ F lds_etab[ETAB ? 64 : 1];
    if constexpr (ETAB) { exp_table_fill(lds_etab); __syncthreads(); }
    for (size_t i = size_t(blockIdx.x)*blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x)*blockDim.x)
    {
        const F v = x[i];
        F r;
        switch (which)
        {
            case MATH_EXP_NEG:       r = exp_neg(v); break;
            case MATH_EXP_NEG_TABLE: r = exp_neg(v, lds_etab); break;
            case MATH_FAST_RCP:      r = fast_rcp(v); break;
            case MATH_SQRT_POS:      r = sqrt_pos(v); break;
            default:                 r = sqrt_nonneg(v); break;
        }
        y[i] = r;
    }
}

template<typename F>
int math_selftest_impl(const int which, const int n, const F* x, F* y, void* stream)
{
    const char* entry = "rrx_math_selftest";
    const char* bad = nullptr;
    if (which < 0 || which >= MATH_COUNT) bad = "which must be 0 (exp_neg), 1 (exp_neg, table form), 2 (fast_rcp), 3 (sqrt_pos) or 4 (sqrt_nonneg)";
    else if (n < 0) bad = "n is negative";
    else if (n > 0 && x == nullptr) bad = "x is null";
    else if (n > 0 && y == nullptr) bad = "y is null";
    if (bad != nullptr) { set_error(std::string(entry) + ": " + bad); return 1; }
    if (n == 0) return 0;
    RRX_TRY
    math_selftest_kernel<F><<<std::min(ceil_div(n, 256), 1024), 256, 0, static_cast<hipStream_t>(stream)>>>(which, size_t(n), x, y);
    RRX_CATCH(entry)
}
}  // namespace


extern "C"
{
int rrx_set_lw_variant(int v)
{
    if (v != 0 && v != 1 && v != 4 && v != 7 && v != 15)
    {
        rrx::set_error("rrx_set_lw_variant: " + std::to_string(v) + " is not an LW variant; accepted: 0 (default), 1 (serial kernel), "
                       "4 (general kernel with 64-B rows), 7 (no one-kernel broadband form), 15 (fp32: one column per lane in the "
                       "one-kernel broadband form)");
        return 1;
    }
    rrx::tuning().lw_variant = v;
    return 0;
}
#if RRX_LW_TIMING
// diagnostic build only: phase clocks per wavefront of a workgroup (out[16][8]: sources + transmissivities, down scan, up scan, replays + sums,
// OPT's sum of tau, OPT's barrier + secant, barrier waits, loop top) summed over the workgroups since the last call, then reset
int rrx_lw_timing(unsigned long long* out)
{
    unsigned long long zero[16*8] = {0};
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lw_clk), 16*8*sizeof(unsigned long long)) != hipSuccess) return 1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_lw_clk), zero, sizeof(zero)) == hipSuccess ? 0 : 1;
}
#endif

int rrx_lw_secants_array_f64(int ncol, int ngpt, int n_gauss_quad, int max_gauss_pts, const double* gauss_Ds, double* secants, void* stream)
{
    RRX_TRY
    lw_secants_array_kernel<double><<<rrx::ceil_div(size_t(ncol)*ngpt*n_gauss_quad, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
            ncol, ngpt, n_gauss_quad, max_gauss_pts, gauss_Ds, secants);
    RRX_CATCH("rrx_lw_secants_array")
}

int rrx_lw_secants_array_f32(int ncol, int ngpt, int n_gauss_quad, int max_gauss_pts, const float* gauss_Ds, float* secants, void* stream)
{
    RRX_TRY
    lw_secants_array_kernel<float><<<rrx::ceil_div(size_t(ncol)*ngpt*n_gauss_quad, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
            ncol, ngpt, n_gauss_quad, max_gauss_pts, gauss_Ds, secants);
    RRX_CATCH("rrx_lw_secants_array")
}

int rrx_lw_solver_noscat_f64(
        int ncol, int nlay, int ngpt, Bool top_at_1, int nmus,
        const double* secants, const double* weights,
        const double* tau, const double* lay_source, const double* lev_source,
        const double* sfc_emis, const double* sfc_src, const double* inc_flux,
        double* flux_up, double* flux_dn,
        Bool do_broadband, double* flux_up_loc, double* flux_dn_loc,
        Bool do_jacobians, const double* sfc_src_jac, double* flux_up_jac, void* stream)
{
    return lw_solver_noscat_impl<double>(ncol, nlay, ngpt, top_at_1, nmus, secants, weights, tau, lay_source, lev_source,
            sfc_emis, sfc_src, inc_flux, flux_up, flux_dn, do_broadband, flux_up_loc, flux_dn_loc,
            do_jacobians, sfc_src_jac, flux_up_jac, stream);
}

int rrx_lw_solver_noscat_f32(
        int ncol, int nlay, int ngpt, Bool top_at_1, int nmus,
        const float* secants, const float* weights,
        const float* tau, const float* lay_source, const float* lev_source,
        const float* sfc_emis, const float* sfc_src, const float* inc_flux,
        float* flux_up, float* flux_dn,
        Bool do_broadband, float* flux_up_loc, float* flux_dn_loc,
        Bool do_jacobians, const float* sfc_src_jac, float* flux_up_jac, void* stream)
{
    return lw_solver_noscat_impl<float>(ncol, nlay, ngpt, top_at_1, nmus, secants, weights, tau, lay_source, lev_source,
            sfc_emis, sfc_src, inc_flux, flux_up, flux_dn, do_broadband, flux_up_loc, flux_dn_loc,
            do_jacobians, sfc_src_jac, flux_up_jac, stream);
}

#define RRX_DEFINE_LW_FRACTIONS(F, SFX) \
int rrx_lw_solver_noscat_fractions##SFX( \
        int ncol, int nlay, int ngpt, Bool top_at_1, const F* secants, const F* weights, \
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up_loc, F* flux_dn_loc, void* stream) \
{ \
    return lw_solver_noscat_fractions_impl<F>(ncol, nlay, ngpt, top_at_1, secants, weights, tau, pfrac, blay, blev, gpoint_bands, \
            sfc_emis, sfc_src, inc_flux, flux_up_loc, flux_dn_loc, stream); \
} \
int rrx_planck_sources_from_fractions##SFX(int ncol, int nlay, int ngpt, const int* gpoint_bands, const F* pfrac, const F* blay, \
        const F* blev, F* lay_src, F* lev_src, void* stream) \
{ return planck_sources_from_fractions_impl<F>(ncol, nlay, ngpt, gpoint_bands, pfrac, blay, blev, lay_src, lev_src, stream); } \
int rrx_lw_solver_noscat_fractions_byband##SFX( \
        int ncol, int nlay, int ngpt, int nbnd, Bool top_at_1, const F* secants, const F* weights, \
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, const int* band_lims_gpt, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, \
        F* bnd_flux_up, F* bnd_flux_dn, F* bnd_flux_net, F* flux_up, F* flux_dn, void* stream) \
{ \
    return lw_solver_noscat_fractions_byband_impl<F>(ncol, nlay, ngpt, nbnd, top_at_1, secants, weights, tau, pfrac, blay, blev, \
            gpoint_bands, band_lims_gpt, sfc_emis, sfc_src, inc_flux, bnd_flux_up, bnd_flux_dn, bnd_flux_net, flux_up, flux_dn, stream); \
} \
int rrx_lw_solver_noscat_fractions_jac##SFX( \
        int ncol, int nlay, int ngpt, Bool top_at_1, const F* secants, const F* weights, \
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up_loc, F* flux_dn_loc, \
        const F* sfc_src_jac, F* flux_up_jac, void* stream) \
{ \
    return lw_solver_noscat_fractions_jac_impl<F>(ncol, nlay, ngpt, top_at_1, secants, weights, tau, pfrac, blay, blev, gpoint_bands, \
            sfc_emis, sfc_src, inc_flux, sfc_src_jac, flux_up_loc, flux_dn_loc, flux_up_jac, stream); \
} \
int rrx_lw_solver_noscat_fractions_angles##SFX( \
        int ncol, int nlay, int ngpt, Bool top_at_1, int nmus, const F* secants, const F* weights, \
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up_loc, F* flux_dn_loc, \
        const F* sfc_src_jac, F* flux_up_jac, void* stream) \
{ \
    return lw_solver_noscat_fractions_angles_impl<F>(ncol, nlay, ngpt, top_at_1, nmus, secants, weights, tau, pfrac, blay, blev, \
            gpoint_bands, sfc_emis, sfc_src, inc_flux, flux_up_loc, flux_dn_loc, sfc_src_jac, flux_up_jac, stream); \
} \
int rrx_lw_flux_up_adjust##SFX(int ncol, int nlev, const F* flux_up_jac, const F* t_sfc_old, const F* t_sfc_new, \
        F* flux_up, F* flux_net, void* stream) \
{ return lw_flux_up_adjust_impl<F>(ncol, nlev, flux_up_jac, t_sfc_old, t_sfc_new, flux_up, flux_net, stream); } \
int rrx_lw_optimal_secants##SFX(int ncol, int nlay, int ngpt, int nbnd, const int* gpoint_bands, const F* optimal_angle_fit, \
        const F* tau, F* secants, void* stream) \
{ return lw_optimal_secants_impl<F>(ncol, nlay, ngpt, nbnd, gpoint_bands, optimal_angle_fit, tau, secants, stream); } \
int rrx_lw_solver_noscat_fractions_optimal##SFX( \
        int ncol, int nlay, int ngpt, int nbnd, Bool top_at_1, const F* weights, \
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, const F* optimal_angle_fit, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up_loc, F* flux_dn_loc, \
        const F* sfc_src_jac, F* flux_up_jac, F* secants_out, void* stream) \
{ \
    return lw_solver_noscat_fractions_optimal_impl<F>(ncol, nlay, ngpt, nbnd, top_at_1, weights, tau, pfrac, blay, blev, gpoint_bands, \
            optimal_angle_fit, sfc_emis, sfc_src, inc_flux, flux_up_loc, flux_dn_loc, sfc_src_jac, flux_up_jac, secants_out, stream); \
} \
int rrx_math_selftest##SFX(int which, int n, const F* x, F* y, void* stream) \
{ return math_selftest_impl<F>(which, n, x, y, stream); }

RRX_DEFINE_LW_FRACTIONS(double, _f64)
RRX_DEFINE_LW_FRACTIONS(float, _f32)
}
