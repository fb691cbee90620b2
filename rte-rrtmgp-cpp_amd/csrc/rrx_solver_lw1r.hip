// Longwave no-scattering solver on rescaled optical depths with one correction sweep (Tang et al. 2018; current RTE+RRTMGP's
// "1rescl" treatment of two-stream optical properties in the longwave; the reference this project follows declares do_rescaling at
// its CPU boundary). Semantics, one g-point of one column, layers i and levels in sweep order from the top:
//   wb = ssa (1 - g)/2,  st = 1 - ssa + wb,  Cn = 0.4 wb / max(st, 3 tiny),  tl = tau D st,  tr = exp(-tl),  An = 1 - tr tr
//   sdn, sup   the no-scattering layer sources of rrx_lw_solver_noscat evaluated with tl, tr (tau_thres series branch included)
//   pass 1     dn[i+1] = tr dn[i] + sdn                                              dn[0] = inc_flux / pi (0 when null)
//   surface    up[nlay] = dn[nlay] (1 - sfc_emis) + sfc_emis sfc_src                 (pass 1's dn)
//   pass 2     up[i]   = tr up[i+1] + sup + Cn (An dn[i]   - tr sdn - sup)           (pass 1's dn)
//   pass 3     dn[i+1] = tr dn[i]   + sdn + Cn (An up[i+1] - tr sup - sdn)           (pass 2's up)
//   fluxes     pi weight up (pass 2), pi weight dn (pass 3), added over the angles;  Jacobian J[nlay] = sfc_emis sfc_src_jac, J[i] = tr J[i+1]
// With ssa = 0: st = 1, Cn = 0 and the solve is rrx_lw_solver_noscat's.
//
// Two entries. rrx_lw_solver_noscat_rescaled takes g-point arrays and runs one thread per (column, g-point) for any number of layers
// and 1..4 angles: the fallback and the yardstick. rrx_lw_solver_noscat_fractions_rescaled is the hot path: Planck-lite inputs and
// band cloud properties combined inside the kernel, one angle, broadband outputs -- the lane scans, the g-point loop, the on-chip
// g-point sums and the prefetch of lw_noscat_bb_kernel with a third affine scan.
#include "rrx_common.h"
#include "rrx_hip.h"
#include <type_traits>

#pragma clang fp contract(fast)

namespace
{
using namespace rrx;

// ---------------------------------------------------------------------------------------------------------------------
// General entry: one thread per (column, g-point), any nlay, one angle per launch. rad_up / rad_dn hold the angle's radiances (pass
// 2's up, pass 1's dn) at every level; pass 3 reads rad_up and writes the scaled fluxes to out_up / out_dn. With one angle and
// per-g-point outputs the two pairs are the same arrays: each element is read before it is overwritten (no __restrict__ on them).
// ACC: the angle's fluxes are added to what out_up / out_dn / flux_up_jac hold.
template<typename F, bool JAC, bool ACC>
__global__ void __launch_bounds__(256)
lw_rescaled_serial_kernel(
        const int ncol, const int nlay, const int ngpt, const int top_at_1, const int imu,
        const F* __restrict__ secants, const F* __restrict__ weights,
        const F* __restrict__ tau, const F* __restrict__ ssa, const F* __restrict__ g,
        const F* __restrict__ lay_source, const F* __restrict__ lev_source,
        const F* __restrict__ sfc_emis, const F* __restrict__ sfc_src, const F* __restrict__ inc_flux,
        F* rad_up, F* rad_dn, F* out_up, F* out_dn,
        const F* __restrict__ sfc_src_jac, F* __restrict__ flux_up_jac)
{
    const int icol = blockIdx.x*blockDim.x + threadIdx.x;
    const int igpt = blockIdx.y;
    if (icol >= ncol) return;
    const int nlev = nlay + 1;
    const size_t ncl = size_t(ncol);
    const size_t lay_base = size_t(igpt)*ncl*nlay + icol;
    const size_t lev_base = size_t(igpt)*ncl*nlev + icol;
    const size_t sfc_idx = size_t(igpt)*ncl + icol;
    const F pi = F(3.14159265358979323846);
    const F tau_thres = sqrt(sqrt(Lim<F>::eps()));
    const F D = secants[sfc_idx + size_t(imu)*ncl*ngpt];
    const F scale = pi * weights[imu];
    auto mlev = [&](const int t) { return lev_base + size_t(top_at_1 ? t : nlay - t)*ncl; };

    struct Layer { F tr, sdn, sup, cn; };
    auto layer = [&](const int s)
    {
        const size_t il = lay_base + size_t(top_at_1 ? s : nlay-1-s)*ncl;
        const F w = ssa[il];
        const F wb = w * (F(1.) - g[il]) * F(.5);
        const F st = F(1.) - w + wb;
        const F tau_loc = tau[il] * D * st;
        const F ls = lay_source[il];
        const F lev_above = lev_source[mlev(s)], lev_below = lev_source[mlev(s+1)];
        Layer L;
        L.cn = F(.4) * wb / max(st, F(3.)*Lim<F>::tiny());
        L.tr = exp(-tau_loc);
        const F fact = tau_loc > tau_thres ?
            (F(1.) - L.tr) / tau_loc - L.tr :
            tau_loc * (F(.5) + tau_loc * (F(-1./3.) + tau_loc * F(1./8.)));
        L.sdn = (F(1.) - L.tr) * lev_below + F(2.) * fact * (ls - lev_below);
        L.sup = (F(1.) - L.tr) * lev_above + F(2.) * fact * (ls - lev_above);
        return L;
    };
    auto put = [&](F* arr, const int t, const F val)
    {
        const size_t o = mlev(t);
        arr[o] = ACC ? arr[o] + scale*val : scale*val;
    };

    const F dn_top = (inc_flux != nullptr) ? inc_flux[sfc_idx] / pi : F(0.);
    F dn = dn_top;
    for (int s=0; s<nlay; ++s)
    {
        const Layer L = layer(s);
        rad_dn[mlev(s)] = dn;
        dn = L.tr*dn + L.sdn;
    }
    rad_dn[mlev(nlay)] = dn;

    const F emis = sfc_emis[sfc_idx];
    F up = dn * (F(1.) - emis) + emis * sfc_src[sfc_idx];
    F jc = JAC ? emis * sfc_src_jac[sfc_idx] : F(0.);
    rad_up[mlev(nlay)] = up;
    if constexpr (JAC) put(flux_up_jac, nlay, jc);
    for (int s=nlay-1; s>=0; --s)
    {
        const Layer L = layer(s);
        const F an = F(1.) - L.tr*L.tr;
        up = L.tr*up + L.sup + L.cn * (an*rad_dn[mlev(s)] - L.tr*L.sdn - L.sup);
        rad_up[mlev(s)] = up;
        if constexpr (JAC) { jc = L.tr*jc; put(flux_up_jac, s, jc); }
    }

    dn = dn_top;
    {
        const F u = rad_up[mlev(0)];
        put(out_dn, 0, dn); put(out_up, 0, u);
    }
    for (int s=0; s<nlay; ++s)
    {
        const Layer L = layer(s);
        const F an = F(1.) - L.tr*L.tr;
        const F u = rad_up[mlev(s+1)];
        dn = L.tr*dn + L.sdn + L.cn * (an*u - L.tr*L.sup - L.sdn);
        put(out_dn, s+1, dn); put(out_up, s+1, u);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused broadband form, one angle. Tiling as lw_2stream_bb_kernel: CLT column-lanes x 64/CLT level-lanes per wavefront, W wavefronts
// per column group, NW/W groups per workgroup, K consecutive layers per lane in registers, one column per lane. Per g-point:
//   (a) every layer: tau / ssa / g from the gas tau and the band cloud, lay_source = pfrac B_lay, lev_source = sqrt(pfrac pfrac') B_lev,
//       then tr, sdn, sup, Cn; the lane's composite of pass 1;
//   (b) pass 1: prefix scan over level-lanes and waves (every wave also forms the whole column's composite: dn at the surface);
//       replay downward: dn[i] turns sup into pass 2's adjusted source, sdn and Cn into the two terms of pass 3's
//       (q = sdn - Cn (tr sup + sdn), c = Cn An, so that pass 3's source is q + c up[i+1]); the lane's composite of pass 2;
//   (c) pass 2: suffix scan; replay upward: up goes into the g-point sums, up[i+1] completes pass 3's source; the lane's composite;
//   (d) pass 3: prefix scan; replay downward with the g-point sums.
// No level arrays: four registers per layer (tr, sdn, sup, Cn) change their meaning as the replays go. Three block barriers per
// g-point; the loads of g-point g+1 are issued behind the first. The g-point sums and the band's B_lay / B_lev sit in per-thread LDS
// columns (4K+1 values per thread); the band cloud arrays are re-read per g-point through the cache. The cloud is
// combined as in lw_2stream_bb_kernel: tau = tau_g + tau_c, ssa = tau_c ssa_c / tau (0 where tau_c ssa_c = 0), g = g_c. Null cloud
// arrays run the same instructions on zeros, so they give the bits of all-zero arrays.
// GS: blockIdx.y = g-point range of this workgroup, its sums go to partial array blockIdx.y (rrx::broadband_gsplit).
template<typename F, int K, int W, int NW, int CLT, bool GS>
__global__ void __launch_bounds__(64*NW, (NW > 4) ? 1 : 2)
lw_rescaled_bb_kernel(
        const int ncol, const int nlay, const int ngpt, const int top_at_1,
        const F* __restrict__ secants, const F* __restrict__ weights,
        const F* __restrict__ tau, const F* __restrict__ pfrac, const F* __restrict__ blay, const F* __restrict__ blev,
        const int* __restrict__ gpoint_bands,
        const F* __restrict__ cld_tau, const F* __restrict__ cld_ssa, const F* __restrict__ cld_g,
        const F* __restrict__ sfc_emis, const F* __restrict__ sfc_src, const F* __restrict__ inc_flux,
        F* __restrict__ flux_up, F* __restrict__ flux_dn, const int gper, const size_t part_stride)
{
    static_assert(W == 2 || W == 4 || W == 8);
    constexpr int CL = CLT, LL = 64/CLT;
    constexpr bool ETAB = sizeof(F) == 8;
    __shared__ F lds_acc_up[K][64*NW];               // per-thread columns: the g-point sums at the lane's K levels
    __shared__ F lds_acc_dn[K][64*NW];
    __shared__ F lds_blay[K][64*NW];                 // ... B_lay of the current band at the lane's K layers
    __shared__ F lds_blev[K+1][64*NW];               // ... B_lev at its K+1 levels
    __shared__ F xch[6][NW][CL];                     // wave totals of the three scans
    __shared__ F lds_etab[ETAB ? 64 : 1];
    if constexpr (ETAB) { exp_table_fill(lds_etab); __syncthreads(); }

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cl = lane & (CL-1), ll = lane / CL;
    const int h = wave % W, w0 = wave - h;
    // (a workgroup whose row segment is half a 128-B line: the other half belongs to the next workgroup -- rrx::xcd_contiguous)
    const int bx = ((NW/W)*CL*sizeof(F) < 128) ? xcd_contiguous(blockIdx.x, gridDim.x) : int(blockIdx.x);
    const int wave_col0 = (bx*(NW/W) + wave/W) * CL;
    // every wave stays alive until the last barrier; lanes without a column compute on a clamped one
    int icol = wave_col0 + cl;
    const bool active = icol < ncol;
    if (!active) icol = (wave_col0 < ncol) ? wave_col0 : 0;
    const bool writer = active && wave_col0 < ncol;
    const int nlev = nlay + 1;
    const size_t ncl = size_t(ncol);
    const int t0 = (h*LL + ll)*K;
    const F pi = F(3.14159265358979323846);
    const F tau_thres = sqrt(sqrt(Lim<F>::eps()));
    const F scale = pi * weights[0];
    const bool has_cld = cld_tau != nullptr;         // (the entry point refuses a partly-null triple)

    const int g_lo = GS ? blockIdx.y*gper : 0;
    const int g_hi = GS ? min(ngpt, g_lo + gper) : ngpt;
    if constexpr (GS) { flux_up += blockIdx.y*part_stride; flux_dn += blockIdx.y*part_stride; }

    #pragma unroll
    for (int j=0; j<K; ++j) { lds_acc_up[j][tid] = F(0.); lds_acc_dn[j][tid] = F(0.); }

    // element offsets inside one g-point (or band) slab: sweep layer s = t0+j, sweep level t = t0+j, clamped into the column
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

    F nt[K], np[K], n_prev, n_next, n_emis, n_ssrc, n_D, n_inc = F(0.);      // the prefetched g-point
    auto issue = [&](const int gp)
    {
        const F* __restrict__ t_g = tau + size_t(gp)*ncl*nlay;
        const F* __restrict__ p_g = pfrac + size_t(gp)*ncl*nlay;
        #pragma unroll
        for (int j=0; j<K; ++j) { const unsigned o = lay_off(j); nt[j] = t_g[o]; np[j] = p_g[o]; }
        n_next = p_g[lay_off(K)];        // pfrac of the layer below the lane's last one
        n_prev = p_g[lay_off(-1)];       // ... above its first one
        const size_t sfc = size_t(gp)*ncl + icol;
        n_emis = sfc_emis[sfc]; n_ssrc = sfc_src[sfc]; n_D = secants[sfc];
        if (inc_flux != nullptr) n_inc = inc_flux[sfc];
    };
    issue(g_lo);       // (no empty range: rrx::broadband_gsplit)
    int cur_bnd = -1;
    const F* __restrict__ ct_b = cld_tau; const F* __restrict__ cw_b = cld_ssa; const F* __restrict__ cg_b = cld_g;

    for (int igpt=g_lo; igpt<g_hi; ++igpt)
    {
    const int ib = gpoint_bands[igpt] - 1;                  // wave-uniform
    if (ib != cur_bnd)
    {
        cur_bnd = ib;
        const F* __restrict__ bl = blay + size_t(ib)*ncl*nlay;
        const F* __restrict__ bv = blev + size_t(ib)*ncl*nlev;
        #pragma unroll
        for (int j=0; j<K; ++j) lds_blay[j][tid] = bl[lay_off(j)];
        #pragma unroll
        for (int j=0; j<=K; ++j) lds_blev[j][tid] = bv[lev_off(j)];
        if (has_cld) { ct_b = cld_tau + size_t(ib)*ncl*nlay; cw_b = cld_ssa + size_t(ib)*ncl*nlay; cg_b = cld_g + size_t(ib)*ncl*nlay; }
    }

    constexpr int EV = 1;
    // per-layer state; the comments give the meanings in the order they take them
    F tr[K];      // transmittance
    F sd[K];      // sdn -> q = sdn - Cn (tr sup + sdn) -> pass 3's source q + c up[i+1]
    F su[K];      // sup -> pass 2's source
    F cn[K];      // Cn  -> c = Cn An

    // ---- (a) layers: every one independent of the others. The first and the last level source take the fraction of their one
    // layer: the neighbour's load is clamped into the column, so there pa == pb and sqrt_nonneg(p*p) returns p (lw_noscat_bb_kernel's note)
    const F D = n_D;
    F A = F(1.), Bdn = F(0.);
    F lva = sqrt_nonneg(n_prev*np[0]) * lds_blev[0][tid];
    #pragma unroll
    for (int j=0; j<K; ++j)
    {
        const bool valid = (t0 + j) < nlay;
        // a padding layer (level slot beyond the surface) is transparent through its optical depth: tau = 0 gives tr = 1, fact = 0
        // (series branch) exactly, hence no sources and no adjustment
        F tg = valid ? nt[j] : F(0.);
        if (j >= EV) asm volatile("" : "+v"(tg) : "v"(su[max(j-EV, 0)]));      // at most EV evaluations in flight (register budget)
        F tc = F(0.), ts = F(0.), gc = F(0.);
        if (has_cld)
        {
            unsigned o = lay_off(j);
            if (j >= EV) asm volatile("" : "+v"(o) : "v"(su[max(j-EV, 0)]));      // ... and their cloud loads
            tc = valid ? ct_b[o] : F(0.); ts = tc * cw_b[o]; gc = cg_b[o];
        }
        const F tt = tg + tc;
        const F w = (ts > F(0.)) ? ts * fast_rcp(tt) : F(0.);
        const F wb = w * (F(1.) - gc) * F(.5);
        const F st = F(1.) - w + wb;
        cn[j] = F(.4) * wb * fast_rcp(max(st, F(3.)*Lim<F>::tiny()));
        const F pb = (j+1 == K) ? n_next : np[min(j+1, K-1)];
        const F lvb = sqrt_nonneg(np[j]*pb) * lds_blev[j+1][tid];
        const F lsj = np[j] * lds_blay[j][tid];
        const F tau_loc = tt * D * st;
        F trans;
        if constexpr (ETAB) trans = exp_neg(-tau_loc, lds_etab); else trans = exp_neg(-tau_loc);
        const F fact = tau_loc > tau_thres ? (F(1.) - trans) * fast_rcp(tau_loc) - trans
                                           : tau_loc * (F(.5) + tau_loc * (F(-1./3.) + tau_loc * F(1./8.)));
        const F omt = F(1.) - trans;
        const F s_dn = omt * lvb + F(2.) * fact * (lsj - lvb);
        const F s_up = omt * lva + F(2.) * fact * (lsj - lva);
        lva = lvb;
        tr[j] = trans; sd[j] = s_dn; su[j] = s_up;
        Bdn = trans*Bdn + s_dn;
        A *= trans;
    }
    __builtin_amdgcn_sched_barrier(0);
    const F emis = n_emis, ssrc = n_ssrc, dn_top = (inc_flux != nullptr) ? n_inc / pi : F(0.);

    // ---- (b) pass 1: inclusive prefix scan over the level-lanes, then over the waves of the column group
    F a = A, b = Bdn;
    #pragma unroll
    for (int d=1; d<LL; d<<=1)
    {
        const F a2 = shfl(a, lane - d*CL), b2 = shfl(b, lane - d*CL);
        if (ll >= d) { b = a*b2 + b; a = a*a2; }
    }
    F xa = F(1.), xb = F(0.);
    if (ll == LL-1) { xch[0][wave][cl] = a; xch[1][wave][cl] = b; }
    __syncthreads();
    {
        // every wave of the workgroup is here and the g-point's registers are consumed: the waves that share 128-B lines ask for the
        // next one together
        __builtin_amdgcn_sched_barrier(0);
        issue(min(igpt + 1, g_hi - 1));          // (last iteration: a harmless re-read)
        __builtin_amdgcn_sched_barrier(0);
    }
    // (xa, xb) = the parts above this wave's, top first; (fa, fb) = all parts, composed in the same order by every wave
    F fa = F(1.), fb = F(0.);
    #pragma unroll
    for (int w=0; w<W; ++w)
    {
        const F oa = xch[0][w0+w][cl], ob = xch[1][w0+w][cl];
        if (w == h) { xa = fa; xb = fb; }
        fb = oa*fb + ob; fa = oa*fa;
    }
    if (h > 0) { b = a*xb + b; a = a*xa; }
    F ae = shfl(a, lane - CL), be = shfl(b, lane - CL);     // exclusive
    if (ll == 0) { ae = xa; be = xb; }
    F dn = ae*dn_top + be;
    const F dn_sfc = fa*dn_top + fb;
    const F up_sfc = dn_sfc * (F(1.) - emis) + emis * ssrc;

    // replay pass 1 downward: the adjusted sources, and the lane's composite of pass 2 (up at its first level from up at its last)
    F Bup = F(0.), Q = F(1.);
    #pragma unroll
    for (int j=0; j<K; ++j)
    {
        const F t = tr[j], c0 = cn[j], s_dn = sd[j], s_up = su[j];
        const F an = F(1.) - t*t;
        const F s2 = s_up + c0 * (an*dn - t*s_dn - s_up);
        sd[j] = s_dn - c0 * (t*s_up + s_dn);
        cn[j] = c0 * an;
        su[j] = s2;
        dn = t*dn + s_dn;
        Bup += Q*s2;
        Q *= t;
    }

    // ---- (c) pass 2: inclusive suffix scan (lanes below applied first)
    a = A; b = Bup;
    #pragma unroll
    for (int d=1; d<LL; d<<=1)
    {
        const F a2 = shfl(a, lane + d*CL), b2 = shfl(b, lane + d*CL);
        if (ll + d < LL) { b = a*b2 + b; a = a*a2; }
    }
    xa = F(1.); xb = F(0.);
    if (ll == 0) { xch[2][wave][cl] = a; xch[3][wave][cl] = b; }
    __syncthreads();
    #pragma unroll
    for (int w=W-1; w>=1; --w)
        if (w > h) { const F oa = xch[2][w0+w][cl], ob = xch[3][w0+w][cl]; xb = oa*xb + ob; xa = oa*xa; }
    if (h < W-1) { b = a*xb + b; a = a*xa; }
    ae = shfl(a, lane + CL); be = shfl(b, lane + CL);
    if (ll == LL-1) { ae = xa; be = xb; }
    F up = ae*up_sfc + be;                                   // up at the bottom of this lane's chunk

    // replay pass 2 upward: the g-point's upward flux goes into the sums, up[i+1] completes pass 3's source; the lane's composite
    F Bd = F(0.);
    Q = F(1.);
    #pragma unroll
    for (int j=K-1; j>=0; --j)
    {
        const F s3 = sd[j] + cn[j]*up;
        sd[j] = s3;
        up = tr[j]*up + su[j];
        F au = lds_acc_up[j][tid];
        add_rounded(au, scale*up);
        lds_acc_up[j][tid] = au;
        Bd += Q*s3;
        Q *= tr[j];
    }

    // ---- (d) pass 3: inclusive prefix scan
    a = A; b = Bd;
    #pragma unroll
    for (int d=1; d<LL; d<<=1)
    {
        const F a2 = shfl(a, lane - d*CL), b2 = shfl(b, lane - d*CL);
        if (ll >= d) { b = a*b2 + b; a = a*a2; }
    }
    xa = F(1.); xb = F(0.);
    if (ll == LL-1) { xch[4][wave][cl] = a; xch[5][wave][cl] = b; }
    __syncthreads();
    #pragma unroll
    for (int w=0; w<W-1; ++w)
        if (w < h) { const F oa = xch[4][w0+w][cl], ob = xch[5][w0+w][cl]; xb = oa*xb + ob; xa = oa*xa; }
    if (h > 0) { b = a*xb + b; a = a*xa; }
    ae = shfl(a, lane - CL); be = shfl(b, lane - CL);
    if (ll == 0) { ae = xa; be = xb; }
    dn = ae*dn_top + be;

    #pragma unroll
    for (int j=0; j<K; ++j)
    {
        F ad = lds_acc_dn[j][tid];
        add_rounded(ad, scale*dn);
        lds_acc_dn[j][tid] = ad;
        dn = tr[j]*dn + sd[j];
    }
    }   // g-point loop

    if (!writer) return;
    #pragma unroll
    for (int j=0; j<K; ++j)
    {
        const int t = t0 + j;
        if (t <= nlay)
        {
            const size_t o = size_t(icol) + size_t(top_at_1 ? t : nlay - t)*ncl;
            flux_up[o] = lds_acc_up[j][tid];
            flux_dn[o] = lds_acc_dn[j][tid];
        }
    }
}

template<typename F>
struct Lw1rArgs
{
    int ncol, nlay, ngpt, top_at_1;
    const F *secants, *weights, *tau, *pfrac, *blay, *blev; const int* gpoint_bands;
    const F *cld_tau, *cld_ssa, *cld_g /* all three or none */, *sfc_emis, *sfc_src, *inc_flux /* or null */;
    F *flux_up, *flux_dn;
};

// One tiling of the fused form: W waves per column group, CLT column lanes per wave, NW waves per workgroup; false when the columns
// are taller than the tiling's largest K (the caller tries the next one).
template<typename F, int W, int CLT, int NW>
bool launch_lw1r(hipStream_t st, const Lw1rArgs<F>& a)
{
    if (size_t(a.ncol)*(a.nlay+1) >= (size_t(1) << 31)) return false;      // 32-bit element offsets inside a g-point slab
    const int groups = ceil_div(a.ncol, (NW/W)*CLT);
    const int need = ceil_div(a.nlay+1, (64/CLT)*W);
    auto with_tiling_k = [&](auto launch)      // the layers per lane of this tiling
    {
        if constexpr (NW == 4) return with_k<2, 4, 6, 9>(need, launch);
        else return with_k<5, 7, 9>(need, launch);
    };
    // few column groups: the g-point loop is split over grid.y (rrx::launch_gsplit)
    const size_t nlevcol = size_t(a.ncol)*(a.nlay+1);
    return launch_gsplit<F,2>(st, groups, a.ngpt, (NW > 4) ? 256 : 512, nlevcol, a.flux_up, a.flux_dn, (F*)nullptr, with_tiling_k,
        [&](auto kk, auto gs, const dim3 grid, const int gper, F* up, F* dn, F*)
    {
        lw_rescaled_bb_kernel<F,decltype(kk)::value,W,NW,CLT,decltype(gs)::value><<<grid, 64*NW, 0, st>>>(
            a.ncol, a.nlay, a.ngpt, a.top_at_1, a.secants, a.weights, a.tau, a.pfrac, a.blay, a.blev, a.gpoint_bands,
            a.cld_tau, a.cld_ssa, a.cld_g, a.sfc_emis, a.sfc_src, a.inc_flux, up, dn, gper, nlevcol);
    });
}

// the fused kernels in the order of preference; false when no form takes the shape
template<typename F>
bool lw1r_fused(hipStream_t st, const Lw1rArgs<F>& a)
{
    if constexpr (sizeof(F) == 8)
    {
        // up to 143 layers: two waves of 8 x 8 lanes per column group, two groups per workgroup, 2 / 4 / 6 / 9 layers per lane;
        // 144 ... 287: four waves per group, two groups per workgroup, 5 / 7 / 9 layers per lane; 288 ... 575: eight waves on one group
        if (launch_lw1r<F,2,8,4>(st, a)) return true;
        if (launch_lw1r<F,4,8,8>(st, a)) return true;
        return launch_lw1r<F,8,8,8>(st, a);
    }
    else
    {
        // 16 x 4 lanes: four waves per column group up to 143 layers, eight up to 287 (5 / 7 / 9 layers per lane); taller columns on
        // eight waves of 8 x 8 lanes as fp64
        if (launch_lw1r<F,4,16,4>(st, a)) return true;
        if (launch_lw1r<F,8,16,8>(st, a)) return true;
        return launch_lw1r<F,8,8,8>(st, a);
    }
}

template<typename F>
struct Lw1rGeneral
{
    int ncol, nlay, ngpt, top_at_1, nmus;
    const F *secants, *weights, *tau, *ssa, *g, *lay_source, *lev_source, *sfc_emis, *sfc_src, *inc_flux;
    F *flux_up, *flux_dn; bool do_broadband; F *flux_up_loc, *flux_dn_loc;
    bool jac; const F* sfc_src_jac; F* flux_up_jac;
};

// workspace elements the general solve needs: one angle's radiances with several angles or do_broadband, the per-g-point fluxes with
// do_broadband
template<typename F>
size_t lw1r_workspace(const Lw1rGeneral<F>& a)
{
    const size_t n_lev = size_t(a.ncol)*(a.nlay+1)*a.ngpt;
    return ((a.nmus > 1 || a.do_broadband) ? 2*n_lev : 0) + (a.do_broadband ? 2*n_lev : 0);
}

// the general solve on a workspace of lw1r_workspace(a) elements (ws may be null when that is 0)
template<typename F>
void lw1r_general(hipStream_t st, const Lw1rGeneral<F>& a, F* ws)
{
    const size_t nlevcol = size_t(a.ncol)*(a.nlay+1);
    const size_t n_lev = nlevcol*a.ngpt;
    F* up = a.flux_up; F* dn = a.flux_dn;
    F* rad_up = up; F* rad_dn = dn;
    if (a.nmus > 1 || a.do_broadband) { rad_up = ws; rad_dn = ws + n_lev; }
    if (a.do_broadband) { up = ws + 2*n_lev; dn = ws + 3*n_lev; }
    const dim3 grid(ceil_div(a.ncol, 256), a.ngpt);
    for (int imu=0; imu<a.nmus; ++imu)
        with_flag(a.jac, [&](auto j) { with_flag(imu > 0, [&](auto acc)
        {
            lw_rescaled_serial_kernel<F,decltype(j)::value,decltype(acc)::value><<<grid, 256, 0, st>>>(
                a.ncol, a.nlay, a.ngpt, a.top_at_1, imu, a.secants, a.weights, a.tau, a.ssa, a.g, a.lay_source, a.lev_source,
                a.sfc_emis, a.sfc_src, a.inc_flux, rad_up, rad_dn, up, dn, a.sfc_src_jac, a.flux_up_jac);
        }); });
    if (a.do_broadband)
    {
        const int nb = ceil_div(nlevcol, 256);
        sum_gpt_kernel<F><<<nb, 256, 0, st>>>(nlevcol, a.ngpt, up, a.flux_up_loc);
        sum_gpt_kernel<F><<<nb, 256, 0, st>>>(nlevcol, a.ngpt, dn, a.flux_dn_loc);
    }
}

template<typename F>
int lw_solver_noscat_rescaled_impl(
        const int ncol, const int nlay, const int ngpt, const Bool top_at_1, const int nmus,
        const F* secants, const F* weights, const F* tau, const F* ssa, const F* g, const F* lay_source, const F* lev_source,
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up, F* flux_dn,
        const Bool do_broadband, F* flux_up_loc, F* flux_dn_loc, const Bool do_jacobians, const F* sfc_src_jac, F* flux_up_jac, void* stream)
{
    RRX_TRY
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (do_broadband)
    {
        if (empty_problem({{"ncol", ncol}, {"nlay", nlay}, {"ngpt", ngpt}},
                          {{"secants", secants}, {"weights", weights}, {"tau", tau}, {"ssa", ssa}, {"g", g}, {"lay_source", lay_source},
                           {"lev_source", lev_source}, {"sfc_emis", sfc_emis}, {"sfc_src", sfc_src},
                           {"flux_up_loc", flux_up_loc}, {"flux_dn_loc", flux_dn_loc}}))
            return 0;
    }
    else if (empty_problem({{"ncol", ncol}, {"nlay", nlay}, {"ngpt", ngpt}},
                           {{"secants", secants}, {"weights", weights}, {"tau", tau}, {"ssa", ssa}, {"g", g}, {"lay_source", lay_source},
                            {"lev_source", lev_source}, {"sfc_emis", sfc_emis}, {"sfc_src", sfc_src},
                            {"flux_up", flux_up}, {"flux_dn", flux_dn}}))
        return 0;
    if (nmus < 1 || nmus > 4) throw std::runtime_error("n_quad_angs must be 1..4");
    const bool jac = do_jacobians && sfc_src_jac != nullptr && flux_up_jac != nullptr;
    const Lw1rGeneral<F> a{ncol, nlay, ngpt, top_at_1, nmus, secants, weights, tau, ssa, g, lay_source, lev_source, sfc_emis, sfc_src,
                           inc_flux, flux_up, flux_dn, bool(do_broadband), flux_up_loc, flux_dn_loc, jac, sfc_src_jac, flux_up_jac};
    WorkspaceLease lease(st);
    const size_t n = lw1r_workspace(a);
    lw1r_general<F>(st, a, n > 0 ? lease.get<F>(n) : nullptr);
    RRX_CATCH("rrx_lw_solver_noscat_rescaled")
}

template<typename F>
int lw_solver_noscat_fractions_rescaled_impl(
        const int ncol, const int nlay, const int ngpt, const int nbnd, const Bool top_at_1, const F* secants, const F* weights,
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, const int* band_lims,
        const F* cld_tau, const F* cld_ssa, const F* cld_g, const F* sfc_emis, const F* sfc_src, const F* inc_flux,
        F* flux_up, F* flux_dn, void* stream)
{
    const char* entry = "rrx_lw_solver_noscat_fractions_rescaled";
    RRX_TRY
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (empty_problem({{"ncol", ncol}, {"nlay", nlay}, {"ngpt", ngpt}, {"nbnd", nbnd}},
                      {{"secants", secants}, {"weights", weights}, {"tau", tau}, {"pfrac", pfrac}, {"blay", blay}, {"blev", blev},
                       {"gpoint_bands", gpoint_bands}, {"band_lims_gpt", band_lims}, {"sfc_emis", sfc_emis}, {"sfc_src", sfc_src},
                       {"flux_up", flux_up}, {"flux_dn", flux_dn}}))
        return 0;
    const int ncld = (cld_tau != nullptr) + (cld_ssa != nullptr) + (cld_g != nullptr);
    if (ncld != 0 && ncld != 3)
        throw std::runtime_error(std::string(cld_tau == nullptr ? "cld_tau" : (cld_ssa == nullptr ? "cld_ssa" : "cld_g")) +
                                 " is null while another cloud array is given (cld_tau, cld_ssa, cld_g: all three or none)");
    const Lw1rArgs<F> a{ncol, nlay, ngpt, top_at_1, secants, weights, tau, pfrac, blay, blev, gpoint_bands, cld_tau, cld_ssa, cld_g,
                        sfc_emis, sfc_src, inc_flux, flux_up, flux_dn};
    if (lw_fused_allowed() && lw1r_fused<F>(st, a)) return check_launch(entry);

    // outside the tilings (and LW variants 1, 7): the combined g-point properties and the sources are materialised in ONE lease of
    // the stream's workspace, [the general solve's part | tau | ssa | g | lay_source | lev_source], and the general kernel solves them
    const size_t n_lay = size_t(ncol)*nlay*ngpt, n_lev = size_t(ncol)*(nlay+1)*ngpt;
    Lw1rGeneral<F> ga{ncol, nlay, ngpt, top_at_1, 1, secants, weights, nullptr, nullptr, nullptr, nullptr, nullptr, sfc_emis, sfc_src,
                      inc_flux, nullptr, nullptr, true, flux_up, flux_dn, false, nullptr, nullptr};
    const size_t n_gen = lw1r_workspace(ga);
    WorkspaceLease lease(st);
    F* ws = lease.get<F>(n_gen + 4*n_lay + n_lev);
    F* c_tau = ws + n_gen; F* c_ssa = c_tau + n_lay; F* c_g = c_ssa + n_lay; F* lay = c_g + n_lay; F* lev = lay + n_lay;
    gas_plus_cloud<F>(stream, ncol, nlay, ngpt, nbnd, band_lims, tau, cld_tau, cld_ssa, cld_g, c_tau);
    if (planck_sources(ncol, nlay, ngpt, gpoint_bands, pfrac, blay, blev, lay, lev, stream) != 0)
        throw std::runtime_error(std::string("forming the sources failed: ") + rrx_last_error());
    ga.tau = c_tau; ga.ssa = c_ssa; ga.g = c_g; ga.lay_source = lay; ga.lev_source = lev;
    lw1r_general<F>(st, ga, ws);
    RRX_CATCH(entry)
}
}  // namespace


extern "C"
{
#define RRX_DEFINE_LW1R(F, SFX) \
int rrx_lw_solver_noscat_rescaled##SFX( \
        int ncol, int nlay, int ngpt, RrxBool top_at_1, int nmus, const F* secants, const F* weights, \
        const F* tau, const F* ssa, const F* g, const F* lay_source, const F* lev_source, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up, F* flux_dn, \
        RrxBool do_broadband, F* flux_up_loc, F* flux_dn_loc, RrxBool do_jacobians, const F* sfc_src_jac, F* flux_up_jac, void* stream) \
{ \
    return lw_solver_noscat_rescaled_impl<F>(ncol, nlay, ngpt, top_at_1, nmus, secants, weights, tau, ssa, g, lay_source, lev_source, \
            sfc_emis, sfc_src, inc_flux, flux_up, flux_dn, do_broadband, flux_up_loc, flux_dn_loc, do_jacobians, sfc_src_jac, flux_up_jac, \
            stream); \
} \
int rrx_lw_solver_noscat_fractions_rescaled##SFX( \
        int ncol, int nlay, int ngpt, int nbnd, RrxBool top_at_1, const F* secants, const F* weights, \
        const F* tau, const F* pfrac, const F* blay, const F* blev, const int* gpoint_bands, const int* band_lims_gpt, \
        const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up, F* flux_dn, void* stream) \
{ \
    return lw_solver_noscat_fractions_rescaled_impl<F>(ncol, nlay, ngpt, nbnd, top_at_1, secants, weights, tau, pfrac, blay, blev, \
            gpoint_bands, band_lims_gpt, cld_tau, cld_ssa, cld_g, sfc_emis, sfc_src, inc_flux, flux_up, flux_dn, stream); \
}

RRX_DEFINE_LW1R(double, _f64)
RRX_DEFINE_LW1R(float, _f32)
}
