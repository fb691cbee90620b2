// Longwave two-stream solver with scattering (current RTE+RRTMGP's lw_solver_2stream; the reference this project follows never had
// it). Semantics, one g-point of one column, layers and levels in sweep order from the top of the atmosphere:
//   layer    gamma1 = D (1 - ssa (1 + g)/2), gamma2 = D ssa (1 - g)/2, D = 1.66, k = sqrt(max((gamma1 - gamma2)(gamma1 + gamma2), 1e-12)),
//            e1 = exp(-tau k), e2 = e1^2, RT = 1/(k (1 + e2) + gamma1 (1 - e2)), Rdif = RT gamma2 (1 - e2), Tdif = 2 RT k e1
//   sources  tau > 1e-8: Z = (lev_bot - lev_top)/(tau (gamma1 + gamma2)),
//            src_up = pi ((Z + lev_top) - Rdif (-Z + lev_top) - Tdif (Z + lev_bot)),
//            src_dn = pi ((-Z + lev_bot) - Rdif (Z + lev_bot) - Tdif (-Z + lev_top));   thinner layers: both 0
//   surface  albedo 1 - emis, source pi emis sfc_src;   top: flux_dn = inc_flux (0 when null)
//   adding   the diffuse recurrences of the SW solver (rrx_solver_sw.hip): albedo and source upward, flux downward.
// No quadrature weights and no secants: the outputs are fluxes.
//
// Two entries. rrx_lw_solver_2stream takes g-point arrays (tau, ssa, g, lev_source) and runs one thread per (column, g-point) for
// any number of layers: the fallback and the yardstick. rrx_lw_solver_2stream_fractions is the hot path: Planck-lite inputs (gas tau,
// Planck fractions, band Planck functions at the levels) and band cloud properties, combined inside the kernel, broadband outputs --
// the lane-scan scheme of sw_2stream_scan_kernel (layers in registers, Moebius / affine composites scanned over level-lanes and
// waves, a downward replay) with the g-point loop, the on-chip g-point sums and the prefetch of lw_noscat_bb_kernel.
#include "rrx_common.h"
#include "rrx_hip.h"
#include <type_traits>

#pragma clang fp contract(fast)

namespace
{
using namespace rrx;

template<typename F>
struct Lw2sLayer { F r, t, su, sd, ab; };      // ab: the absorptance 1 - Rdif - Tdif, formed without that subtraction

// 1 - exp(-x) for x >= 0 to a relative error of a few eps, given e1 = exp(-x): below 1/4 the series x (1 - x/2 (1 - x/3 ...)) (its first
// neglected term is below eps/2 of the sum), from there on the difference, which loses at most two bits
template<typename F>
__device__ __forceinline__ F one_minus_exp_neg(const F x, const F e1)
{
    constexpr int N = (sizeof(F) == 8) ? 13 : 7;
    F p = F(1.);
    #pragma unroll
    for (int n=N; n>=2; --n) p = F(1.) - (x * F(1./n)) * p;
    return (x < F(.25)) ? x * p : F(1.) - e1;
}

// one layer: diffuse reflectance / transmittance and the two sources (the formulas at the top of this file). TAB: fp64 exponential
// through the 2^(j/64) table in LDS (rrx_common.h).
// The sources are evaluated in a regrouped form. As written, Z (1 + Rdif - Tdif) forms a difference that is O(tau) from terms of O(1)
// and multiplies its rounding error by Z = O(1/tau): a last-bit change of tau moved the source of a layer of tau = 1e-6 in its sixth
// digit. With u = 1 - e1, m = 1 - e2 = u (1 + e1), both free of cancellation:
//   1 - Tdif          = RT (k u^2 + gamma1 m)
//   1 + Rdif - Tdif   = RT (k u^2 + (gamma1 + gamma2) m)
//   c := (1 + Rdif - Tdif)/(tau (gamma1 + gamma2)) - 1 = RT ((k u^2/(tau (gamma1 + gamma2)) - gamma1 m) + (m/tau - k (1 + e2)))
//   src_up = pi ( (lev_bot - lev_top) c + lev_bot (1 - Tdif) - Rdif lev_top)
//   src_dn = pi (-(lev_bot - lev_top) c + lev_top (1 - Tdif) - Rdif lev_bot)
// which is the same function of the inputs; what is left is an absolute error of a few eps in c, times lev_bot - lev_top.
// The absorptance 1 - Rdif - Tdif = RT (k u^2 + (gamma1 - gamma2) m) comes with it (for the fused kernel's albedo scan); it is clamped at 0,
// since gamma1 - gamma2 of a conservative layer may round to -1 ulp.
template<typename F, bool TAB>
__device__ __forceinline__ Lw2sLayer<F> lw_two_stream(const F tau, const F ssa, const F g, const F lev_top, const F lev_bot, const F* etab)
{
    const F D = F(1.66), pi = F(3.14159265358979323846);
    const F gamma1 = D * (F(1.) - F(.5) * ssa * (F(1.) + g));
    const F gamma2 = D * F(.5) * ssa * (F(1.) - g);
    const F gsum = gamma1 + gamma2;
    const F k = sqrt_pos(max((gamma1 - gamma2) * gsum, F(1.e-12)));
    const F x = tau * k;
    F e1;
    if constexpr (TAB) e1 = exp_neg(-x, etab); else e1 = exp_neg(-x);
    const F u = one_minus_exp_neg(x, e1);
    const F m = u * (F(1.) + e1);
    const F kp = k * (F(1.) + e1 * e1);
    const F rt = fast_rcp(kp + gamma1 * m);
    const F ku2 = k * u * u, g1m = gamma1 * m;
    Lw2sLayer<F> o;
    o.r = rt * gamma2 * m;
    o.t = rt * F(2.) * k * e1;
    const F omt = rt * (ku2 + g1m);
    o.ab = max(rt * (ku2 + (gamma1 - gamma2) * m), F(0.));
    const bool thick = tau > F(1.e-8);
    const F itg = fast_rcp(thick ? tau * gsum : F(1.));
    const F c = rt * ((ku2 * itg - g1m) + (m * gsum * itg - kp));
    const F dc = (lev_bot - lev_top) * c;
    const F su = pi * (dc + (lev_bot * omt - o.r * lev_top));
    const F sd = pi * ((lev_top * omt - o.r * lev_bot) - dc);
    o.su = thick ? su : F(0.);
    o.sd = thick ? sd : F(0.);
    return o;
}

// ---------------------------------------------------------------------------------------------------------------------
// General entry: one thread per (column, g-point), any nlay, no workspace. The upward sweep leaves the albedo and the source of every
// level in flux_dn and flux_up; the downward sweep evaluates each layer a second time and overwrites them with the fluxes.
template<typename F>
__global__ void __launch_bounds__(256)
lw_2stream_serial_kernel(
        const int ncol, const int nlay, const int ngpt, const int top_at_1,
        const F* __restrict__ tau, const F* __restrict__ ssa, const F* __restrict__ g, const F* __restrict__ lev_source,
        const F* __restrict__ sfc_emis, const F* __restrict__ sfc_src, const F* __restrict__ inc_flux,
        F* __restrict__ flux_up, F* __restrict__ flux_dn)
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
    auto mlev = [&](const int t) { return lev_base + size_t(top_at_1 ? t : nlay - t)*ncl; };
    auto mlay = [&](const int s) { return lay_base + size_t(top_at_1 ? s : nlay-1-s)*ncl; };
    auto layer = [&](const int s)
    {
        const size_t il = mlay(s);
        return lw_two_stream<F,false>(tau[il], ssa[il], g[il], lev_source[mlev(s)], lev_source[mlev(s+1)], nullptr);
    };

    const F emis = sfc_emis[sfc_idx];
    F a = F(1.) - emis;
    F sr = pi * emis * sfc_src[sfc_idx];
    flux_dn[mlev(nlay)] = a; flux_up[mlev(nlay)] = sr;
    for (int s=nlay-1; s>=0; --s)
    {
        const Lw2sLayer<F> L = layer(s);
        const F denom = F(1.)/(F(1.) - L.r*a);
        sr = L.su + L.t*denom*(sr + a*L.sd);
        a = L.r + L.t*L.t*a*denom;
        flux_dn[mlev(s)] = a; flux_up[mlev(s)] = sr;
    }

    F dn = (inc_flux != nullptr) ? inc_flux[sfc_idx] : F(0.);
    flux_up[mlev(0)] = dn*a + sr;
    flux_dn[mlev(0)] = dn;
    for (int s=0; s<nlay; ++s)
    {
        const Lw2sLayer<F> L = layer(s);
        const size_t lv = mlev(s+1);
        const F a_below = flux_dn[lv], s_below = flux_up[lv];
        const F denom = F(1.)/(F(1.) - L.r*a_below);
        dn = (L.t*dn + L.r*s_below + L.sd) * denom;
        flux_up[lv] = dn*a_below + s_below;
        flux_dn[lv] = dn;
    }
}

// lev_source(level m) = sqrt(pfrac(m) pfrac(m-1)) B_lev(m), first / last level pfrac B_lev: what rrx_planck_sources_from_fractions
// writes to lev_src (the route outside the fused tilings has no B_lay to hand that entry)
template<typename F>
__global__ void lw2s_level_sources_kernel(const int ncol, const int nlay, const int ngpt, const int* __restrict__ gpoint_bands,
        const F* __restrict__ pf, const F* __restrict__ blev, F* __restrict__ lev_src)
{
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
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused broadband form. Tiling as sw_2stream_scan_kernel: CLT column-lanes x 64/CLT level-lanes per wavefront, W wavefronts per column
// group, NW/W groups per workgroup, K consecutive layers per lane in registers, one column per lane. Per g-point:
//   (a) every layer: combined tau / ssa / g from the gas tau and the band cloud, level sources sqrt(pfrac pfrac') B_lev, lw_two_stream;
//   (b) albedo     a' = r + t^2 a/(1 - r a)     Moebius composite per lane, suffix scan over level-lanes and waves, replay upward;
//   (c) source     s' = alpha s + beta          affine composite, suffix scan, replay upward;
//   (d) flux down  d' = alpha d + b             affine composite, prefix scan, replay downward with the g-point sums.
// Three block barriers per g-point; the loads of g-point g+1 (tau, pfrac, surface values) are issued behind the first and land
// during the scans. The g-point sums of both fluxes sit in per-thread LDS columns and are added in g-point order with add_rounded,
// rrx_sum_broadband's order. B_lev of the current band sits in per-thread LDS columns, refreshed when the band changes.
// The band cloud arrays are re-read per g-point through the cache (in LDS columns next to B_lev they cost the second workgroup per CU
// and do not fit at all at nine layers per lane: DESIGN.md 4.10). The combination is rrx_inc_2stream_by_2stream_bybnd's on gas (tau_g, 0, 0): tau = tau_g + tau_c,
// ssa = tau_c ssa_c / tau; g = (tau_c ssa_c g_c)/(tau_c ssa_c) is taken as g_c (where tau_c ssa_c = 0, ssa = 0 and g multiplies nothing).
// Null cloud arrays run the same instructions on zeros, so they give the bits of all-zero arrays.
// GS: blockIdx.y = g-point range of this workgroup, its sums go to partial array blockIdx.y (rrx::broadband_gsplit).
template<typename F, int K, int W, int NW, int CLT, bool GS>
__global__ void __launch_bounds__(64*NW, (CLT == 16) ? 2 : ((NW > 4) ? 1 : 2))
lw_2stream_bb_kernel(
        const int ncol, const int nlay, const int ngpt, const int top_at_1,
        const F* __restrict__ tau, const F* __restrict__ pfrac, const F* __restrict__ blev, const int* __restrict__ gpoint_bands,
        const F* __restrict__ cld_tau, const F* __restrict__ cld_ssa, const F* __restrict__ cld_g,
        const F* __restrict__ sfc_emis, const F* __restrict__ sfc_src, const F* __restrict__ inc_flux,
        F* __restrict__ flux_up, F* __restrict__ flux_dn, const int gper, const size_t part_stride)
{
    static_assert(W == 2 || W == 4 || W == 8);
    constexpr int CL = CLT, LL = 64/CLT;
    constexpr bool ETAB = sizeof(F) == 8;
    __shared__ F lds_alb[K][64*NW];                  // per-thread columns: albedo at the lane's K levels
    __shared__ F lds_acc_up[K][64*NW];               // ... the g-point sums
    __shared__ F lds_acc_dn[K][64*NW];
    __shared__ F lds_blev[K+1][64*NW];               // ... B_lev of the current band at the lane's K+1 levels
    __shared__ F xch[7][NW][CL];                     // wave totals of the scans (one slot per scan component)
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

    F nt[K], np[K], n_prev, n_next, n_emis, n_ssrc, n_inc = F(0.);      // the prefetched g-point
    auto issue = [&](const int gp)
    {
        const F* __restrict__ t_g = tau + size_t(gp)*ncl*nlay;
        const F* __restrict__ p_g = pfrac + size_t(gp)*ncl*nlay;
        #pragma unroll
        for (int j=0; j<K; ++j) { const unsigned o = lay_off(j); nt[j] = t_g[o]; np[j] = p_g[o]; }
        n_next = p_g[lay_off(K)];        // pfrac of the layer below the lane's last one
        n_prev = p_g[lay_off(-1)];       // ... above its first one
        const size_t sfc = size_t(gp)*ncl + icol;
        n_emis = sfc_emis[sfc]; n_ssrc = sfc_src[sfc];
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
        const F* __restrict__ bv = blev + size_t(ib)*ncl*nlev;
        #pragma unroll
        for (int j=0; j<=K; ++j) lds_blev[j][tid] = bv[lev_off(j)];
        if (has_cld) { ct_b = cld_tau + size_t(ib)*ncl*nlay; cw_b = cld_ssa + size_t(ib)*ncl*nlay; cg_b = cld_g + size_t(ib)*ncl*nlay; }
    }

    // level source at sweep level t0+j. The first and the last level take the fraction of their one layer: the neighbour's load is
    // clamped into the column, so there pa == pb and sqrt_nonneg(p*p) returns p (lw_noscat_bb_kernel's note)
    auto level_src = [&](const int j) -> F
    {
        const F pa = (j == 0) ? n_prev : np[max(j-1, 0)];
        const F pb = (j == K) ? n_next : np[min(j, K-1)];
        return sqrt_nonneg(pa*pb) * lds_blev[j][tid];
    };

    constexpr int EV = 2;
    // per-layer state; names follow their LAST meaning (sw_2stream_scan_kernel)
    F rp[K];      // Rdif   -> p = Rdif*denom
    F al[K];      // Tdif   -> alpha = Tdif*denom
    F sb[K];      // src_up -> beta -> src at level t0+j
    F qb[K];      // src_dn -> q = src_dn*denom -> b

    // ---- (a) layers: every one independent of the others; (b) with them the Moebius composite of this lane's layers for the albedo
    // scan, normalised to m11 = 1 below. The composite acts on the CO-ALBEDO b = 1 - albedo: with rho = 1 - Rdif = Tdif + ab the
    // adding step a' = r + t^2 a/(1 - r a) is b' = ((rho r + t^2) b + ab (rho + t))/(r b + rho), a map whose four coefficients are
    // non-negative, so neither a lane's product nor the compositions of the scan (n11 = m10 p01 + 1 >= 1) subtract anything. In albedo
    // space the same normalisation is 1 - R R' of two sub-stacks, which cancels as both reflectances near 1: a conservative column of
    // 500 layers left the albedo at the lanes' chunk boundaries 7e2 eps off (the sequential recurrence: 8 eps) and the fluxes of that
    // g-point 30 x further from truth than the serial kernel's (tests/test_gpu_lw2s_truth.py).
    F m00 = F(1.), m01 = F(0.), m10 = F(0.), m11 = F(1.);
    F lva = level_src(0);
    #pragma unroll
    for (int j=0; j<K; ++j)
    {
        const bool valid = (t0 + j) < nlay;
        // a padding layer (level slot beyond the surface) is transparent through its optical depth: tau = 0 gives Rdif = 0, Tdif = 1
        // to an ulp and no sources
        F tg = valid ? nt[j] : F(0.);
        if (j >= EV) asm volatile("" : "+v"(tg) : "v"(qb[max(j-EV, 0)]));      // at most EV evaluations in flight (register budget)
        F tc = F(0.), ts = F(0.), gc = F(0.);
        if (has_cld)
        {
            unsigned o = lay_off(j);
            if (j >= EV) asm volatile("" : "+v"(o) : "v"(qb[max(j-EV, 0)]));      // ... and their cloud loads
            tc = valid ? ct_b[o] : F(0.); ts = tc * cw_b[o]; gc = cg_b[o];
        }
        const F tt = tg + tc;
        const F ssa = (ts > F(0.)) ? ts * fast_rcp(tt) : F(0.);
        F pb = (j+1 == K) ? n_next : np[min(j+1, K-1)];
        if (j >= EV) asm volatile("" : "+v"(pb) : "v"(qb[max(j-EV, 0)]));      // ... and their level sources
        const F lvb = sqrt_nonneg(np[j]*pb) * lds_blev[j+1][tid];
        const Lw2sLayer<F> L = lw_two_stream<F,ETAB>(tt, ssa, gc, lva, lvb, lds_etab);
        lva = lvb;
        rp[j] = L.r; al[j] = L.t; sb[j] = L.su; qb[j] = L.sd;
        {
            // M <- M * L_j (layer 0 is the outermost map): the same product as applying layer K-1 first
            const F rho = L.t + L.ab;
            const F l00 = rho*L.r + L.t*L.t, l01 = L.ab*(rho + L.t);
            const F n00 = m00*l00 + m01*L.r, n01 = m00*l01 + m01*rho;
            const F n10 = m10*l00 + m11*L.r, n11 = m10*l01 + m11*rho;
            m00 = n00; m01 = n01; m10 = n10; m11 = n11;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    const F emis = n_emis, ssrc = n_ssrc, dn_top = (inc_flux != nullptr) ? n_inc : F(0.);

    // ---- (b) albedo: this lane's composite, normalised to m11 = 1 (m11 > 0: a product of sums of non-negative terms with rho > 0)
    {
        const F inv = fast_rcp(m11);
        m00 *= inv; m01 *= inv; m10 *= inv; m11 = F(1.);
    }
    // inclusive suffix scan over the level-lanes: S(ll) = M_ll * M_{ll+1} * ...
    #pragma unroll
    for (int d=1; d<LL; d<<=1)
    {
        const F p00 = shfl(m00, lane + d*CL), p01 = shfl(m01, lane + d*CL);
        const F p10 = shfl(m10, lane + d*CL);            // partner m11 == 1
        if (ll + d < LL)
        {
            const F n00 = m00*p00 + m01*p10, n01 = m00*p01 + m01;
            const F n10 = m10*p00 + p10,     n11 = m10*p01 + F(1.);
            const F inv = fast_rcp(n11);
            m00 = n00*inv; m01 = n01*inv; m10 = n10*inv;
        }
    }
    F x00 = F(1.), x01 = F(0.), x10 = F(0.);      // composite of everything below this wave's levels
    if (ll == 0) { xch[0][wave][cl] = m00; xch[1][wave][cl] = m01; xch[2][wave][cl] = m10; }
    __syncthreads();
    {
        // every wave of the workgroup is here and the g-point's registers are consumed: the waves that share 128-B lines ask for the
        // next one together
        __builtin_amdgcn_sched_barrier(0);
        issue(min(igpt + 1, g_hi - 1));          // (last iteration: a harmless re-read)
        __builtin_amdgcn_sched_barrier(0);
    }
    // composite of the waves below this one (the lowest applied first), then this wave's on top of it
    #pragma unroll
    for (int w=W-1; w>=1; --w)
        if (w > h)
        {
            const F o00 = xch[0][w0+w][cl], o01 = xch[1][w0+w][cl], o10 = xch[2][w0+w][cl];
            const F n00 = o00*x00 + o01*x10, n01 = o00*x01 + o01;
            const F n10 = o10*x00 + x10,     n11 = o10*x01 + F(1.);
            const F inv = fast_rcp(n11);
            x00 = n00*inv; x01 = n01*inv; x10 = n10*inv;
        }
    if (h < W-1)
    {
        const F n00 = m00*x00 + m01*x10, n01 = m00*x01 + m01;
        const F n10 = m10*x00 + x10,     n11 = m10*x01 + F(1.);
        const F inv = fast_rcp(n11);
        m00 = n00*inv; m01 = n01*inv; m10 = n10*inv;
    }
    F e00 = shfl(m00, lane + CL), e01 = shfl(m01, lane + CL), e10 = shfl(m10, lane + CL);
    if (ll == LL-1) { e00 = x00; e01 = x01; e10 = x10; }
    // albedo at the bottom of this lane's chunk: 1 - the co-albedo there; the surface's co-albedo is emis
    F a = F(1.) - (e00*emis + e01) * fast_rcp(e10*emis + F(1.));

    // replay the albedo upward; build alpha, beta, p, q and the lane's affine composites
    F As = F(1.), Bs = F(0.), Bd = F(0.);    // As: product of alpha (shared); Bs: source (upward); Bd: down
    #pragma unroll
    for (int j=K-1; j>=0; --j)
    {
        const F r = rp[j], t = al[j];
        const F denom = fast_rcp(F(1.) - r*a);
        const F alpha = t*denom;
        const F beta = sb[j] + alpha*a*qb[j];
        a = r + t*alpha*a;
        lds_alb[j][tid] = a;
        al[j] = alpha;
        sb[j] = beta;
        rp[j] = r*denom;
        qb[j] = qb[j]*denom;
        Bs = alpha*Bs + beta;
        As *= alpha;
    }

    // ---- (c) source: suffix affine scan (lanes below applied first)
    F sa = As, sbb = Bs;
    #pragma unroll
    for (int d=1; d<LL; d<<=1)
    {
        const F a2 = shfl(sa, lane + d*CL), b2 = shfl(sbb, lane + d*CL);
        if (ll + d < LL) { sbb = sa*b2 + sbb; sa = sa*a2; }
    }
    F xa = F(1.), xb = F(0.);
    if (ll == 0) { xch[3][wave][cl] = sa; xch[4][wave][cl] = sbb; }
    __syncthreads();
    #pragma unroll
    for (int w=W-1; w>=1; --w)
        if (w > h) { const F oa = xch[3][w0+w][cl], ob = xch[4][w0+w][cl]; xb = oa*xb + ob; xa = oa*xa; }
    if (h < W-1) { sbb = sa*xb + sbb; sa = sa*xa; }
    F ae = shfl(sa, lane + CL), be = shfl(sbb, lane + CL);
    if (ll == LL-1) { ae = xa; be = xb; }
    const F src_sfc = pi * emis * ssrc;
    F s = ae*src_sfc + be;                                   // src at the bottom of this lane's chunk

    // replay src upward; b_j = p_j*src_below + q_j; accumulate the downward composite
    F Q = F(1.);
    #pragma unroll
    for (int j=K-1; j>=0; --j)
    {
        const F b = rp[j]*s + qb[j];
        s = al[j]*s + sb[j];
        sb[j] = s;
        qb[j] = b;
        Bd += Q*b;
        Q *= al[j];
    }

    // ---- (d) diffuse down: prefix affine scan
    F da = As, db = Bd;
    #pragma unroll
    for (int d=1; d<LL; d<<=1)
    {
        const F a2 = shfl(da, lane - d*CL), b2 = shfl(db, lane - d*CL);
        if (ll >= d) { db = da*b2 + db; da = da*a2; }
    }
    xa = F(1.); xb = F(0.);
    if (ll == LL-1) { xch[5][wave][cl] = da; xch[6][wave][cl] = db; }
    __syncthreads();
    #pragma unroll
    for (int w=0; w<W-1; ++w)
        if (w < h) { const F oa = xch[5][w0+w][cl], ob = xch[6][w0+w][cl]; xb = oa*xb + ob; xa = oa*xa; }
    if (h > 0) { db = da*xb + db; da = da*xa; }
    ae = shfl(da, lane - CL); be = shfl(db, lane - CL);
    if (ll == 0) { ae = xa; be = xb; }
    F dn = ae*dn_top + be;

    // replay the downward flux; the g-point's fluxes go into the sums as soon as each value exists
    #pragma unroll
    for (int j=0; j<K; ++j)
    {
        const F up = dn*lds_alb[j][tid] + sb[j];
        F au = lds_acc_up[j][tid], ad = lds_acc_dn[j][tid];
        add_rounded(au, up); add_rounded(ad, dn);
        lds_acc_up[j][tid] = au; lds_acc_dn[j][tid] = ad;
        dn = al[j]*dn + qb[j];
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
struct Lw2sArgs
{
    int ncol, nlay, ngpt, top_at_1;
    const F *tau, *pfrac, *blev; const int* gpoint_bands;
    const F *cld_tau, *cld_ssa, *cld_g /* all three or none */, *sfc_emis, *sfc_src, *inc_flux /* or null */;
    F *flux_up, *flux_dn;
};

// One tiling of the fused form: W waves per column group, CLT column lanes per wave, NW waves per workgroup; false when the columns
// are taller than the tiling's largest K (the caller tries the next one).
template<typename F, int W, int CLT, int NW>
bool launch_lw2s(hipStream_t st, const Lw2sArgs<F>& a)
{
    if (size_t(a.ncol)*(a.nlay+1) >= (size_t(1) << 31)) return false;      // 32-bit element offsets inside a g-point slab
    const int groups = ceil_div(a.ncol, (NW/W)*CLT);
    const int need = ceil_div(a.nlay+1, (64/CLT)*W);
    auto with_tiling_k = [&](auto launch)      // the layers per lane of this tiling
    {
        if constexpr (CLT == 16 && NW == 4) return with_k<2, 4, 6, 9>(need, launch);
        else if constexpr (CLT == 16) return with_k<12>(need, launch);
        else if constexpr (W == 2) return with_k<2, 4, 6, 9, 12>(need, launch);
        else if constexpr (W == 8) return with_k<5, 7, 9>(need, launch);
        else return with_k<9>(need, launch);
    };
    // few column groups: the g-point loop is split over grid.y (rrx::launch_gsplit)
    const size_t nlevcol = size_t(a.ncol)*(a.nlay+1);
    return launch_gsplit<F,2>(st, groups, a.ngpt, (NW > 4) ? 256 : 512, nlevcol, a.flux_up, a.flux_dn, (F*)nullptr, with_tiling_k,
        [&](auto kk, auto gs, const dim3 grid, const int gper, F* up, F* dn, F*)
    {
        lw_2stream_bb_kernel<F,decltype(kk)::value,W,NW,CLT,decltype(gs)::value><<<grid, 64*NW, 0, st>>>(
            a.ncol, a.nlay, a.ngpt, a.top_at_1, a.tau, a.pfrac, a.blev, a.gpoint_bands, a.cld_tau, a.cld_ssa, a.cld_g,
            a.sfc_emis, a.sfc_src, a.inc_flux, up, dn, gper, nlevcol);
    });
}

// the fused kernels in the order of preference; false when no form takes the shape
template<typename F>
bool lw2s_fused(hipStream_t st, const Lw2sArgs<F>& a)
{
    if constexpr (sizeof(F) == 8)
    {
        // up to 191 layers: two waves of 8 x 8 lanes per column group, two groups per workgroup; 192 ... 287: four waves per group;
        // 288 ... 575: eight waves on one column group per workgroup
        if (launch_lw2s<F,2,8,4>(st, a)) return true;
        if (launch_lw2s<F,4,8,8>(st, a)) return true;
        return launch_lw2s<F,8,8,8>(st, a);
    }
    else
    {
        // 16 x 4 lanes, four waves per column group: up to 143 layers with one group per workgroup, 144 ... 191 with two; taller
        // columns on 8 x 8 lanes as fp64
        if (launch_lw2s<F,4,16,4>(st, a)) return true;
        if (launch_lw2s<F,4,16,8>(st, a)) return true;
        if (launch_lw2s<F,4,8,8>(st, a)) return true;
        return launch_lw2s<F,8,8,8>(st, a);
    }
}

template<typename F>
int lw_solver_2stream_impl(
        const int ncol, const int nlay, const int ngpt, const Bool top_at_1,
        const F* tau, const F* ssa, const F* g, const F* lev_source, const F* sfc_emis, const F* sfc_src, const F* inc_flux,
        F* flux_up, F* flux_dn, const Bool do_broadband, F* flux_up_loc, F* flux_dn_loc, void* stream, const char* entry = "rrx_lw_solver_2stream")
{
    RRX_TRY
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (do_broadband)
    {
        if (empty_problem({{"ncol", ncol}, {"nlay", nlay}, {"ngpt", ngpt}},
                          {{"tau", tau}, {"ssa", ssa}, {"g", g}, {"lev_source", lev_source}, {"sfc_emis", sfc_emis}, {"sfc_src", sfc_src},
                           {"flux_up_loc", flux_up_loc}, {"flux_dn_loc", flux_dn_loc}}))
            return 0;
    }
    else if (empty_problem({{"ncol", ncol}, {"nlay", nlay}, {"ngpt", ngpt}},
                           {{"tau", tau}, {"ssa", ssa}, {"g", g}, {"lev_source", lev_source}, {"sfc_emis", sfc_emis}, {"sfc_src", sfc_src},
                            {"flux_up", flux_up}, {"flux_dn", flux_dn}}))
        return 0;
    // broadband mode: per-g-point fluxes go to the stream's workspace (the caller's flux_up / flux_dn when it gives both), then are summed
    const size_t nlevcol = size_t(ncol)*(nlay+1);
    WorkspaceLease lease(st);
    F* up = flux_up; F* dn = flux_dn;
    if (do_broadband && (up == nullptr || dn == nullptr)) { up = lease.get<F>(2*nlevcol*ngpt); dn = up + nlevcol*ngpt; }
    lw_2stream_serial_kernel<F><<<dim3(ceil_div(ncol, 256), ngpt), 256, 0, st>>>(ncol, nlay, ngpt, top_at_1, tau, ssa, g, lev_source,
            sfc_emis, sfc_src, inc_flux, up, dn);
    if (do_broadband)
    {
        const int nb = ceil_div(nlevcol, 256);
        sum_gpt_kernel<F><<<nb, 256, 0, st>>>(nlevcol, ngpt, up, flux_up_loc);
        sum_gpt_kernel<F><<<nb, 256, 0, st>>>(nlevcol, ngpt, dn, flux_dn_loc);
    }
    RRX_CATCH(entry)
}

template<typename F>
int lw_solver_2stream_fractions_impl(
        const int ncol, const int nlay, const int ngpt, const int nbnd, const Bool top_at_1,
        const F* tau, const F* pfrac, const F* blev, const int* gpoint_bands, const int* band_lims,
        const F* cld_tau, const F* cld_ssa, const F* cld_g, const F* sfc_emis, const F* sfc_src, const F* inc_flux,
        F* flux_up, F* flux_dn, void* stream)
{
    const char* entry = "rrx_lw_solver_2stream_fractions";
    RRX_TRY
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (empty_problem({{"ncol", ncol}, {"nlay", nlay}, {"ngpt", ngpt}, {"nbnd", nbnd}},
                      {{"tau", tau}, {"pfrac", pfrac}, {"blev", blev}, {"gpoint_bands", gpoint_bands}, {"band_lims_gpt", band_lims},
                       {"sfc_emis", sfc_emis}, {"sfc_src", sfc_src}, {"flux_up", flux_up}, {"flux_dn", flux_dn}}))
        return 0;
    const int ncld = (cld_tau != nullptr) + (cld_ssa != nullptr) + (cld_g != nullptr);
    if (ncld != 0 && ncld != 3)
        throw std::runtime_error(std::string(cld_tau == nullptr ? "cld_tau" : (cld_ssa == nullptr ? "cld_ssa" : "cld_g")) +
                                 " is null while another cloud array is given (cld_tau, cld_ssa, cld_g: all three or none)");
    const Lw2sArgs<F> a{ncol, nlay, ngpt, top_at_1, tau, pfrac, blev, gpoint_bands, cld_tau, cld_ssa, cld_g, sfc_emis, sfc_src, inc_flux,
                        flux_up, flux_dn};
    if (lw_fused_allowed() && lw2s_fused<F>(st, a)) return check_launch(entry);

    // outside the tilings (and LW variants 1, 7): the combined g-point properties and the level sources are materialised in ONE
    // lease of the stream's workspace, [up | dn | tau | ssa | g | lev_source], and the general kernel solves them
    const size_t n_lay = size_t(ncol)*nlay*ngpt, n_lev = size_t(ncol)*(nlay+1)*ngpt;
    WorkspaceLease lease(st);
    F* ws = lease.get<F>(2*n_lev + 3*n_lay + n_lev);
    F* c_tau = ws + 2*n_lev; F* c_ssa = c_tau + n_lay; F* c_g = c_ssa + n_lay; F* lev = c_g + n_lay;
    gas_plus_cloud<F>(stream, ncol, nlay, ngpt, nbnd, band_lims, tau, cld_tau, cld_ssa, cld_g, c_tau);      // (a failure is named after this entry below)
    lw2s_level_sources_kernel<F><<<int(std::min<size_t>((n_lev + 255)/256, 256*16)), 256, 0, st>>>(ncol, nlay, ngpt, gpoint_bands, pfrac, blev, lev);
    if (lw_solver_2stream_impl<F>(ncol, nlay, ngpt, top_at_1, c_tau, c_ssa, c_g, lev, sfc_emis, sfc_src, inc_flux, ws, ws + n_lev,
                                  Bool(1), flux_up, flux_dn, stream, entry) != 0)
        return 1;
    RRX_CATCH(entry)
}
}  // namespace


extern "C"
{
#define RRX_DEFINE_LW2S(F, SFX) \
int rrx_lw_solver_2stream##SFX( \
        int ncol, int nlay, int ngpt, RrxBool top_at_1, \
        const F* tau, const F* ssa, const F* g, const F* lev_source, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, \
        F* flux_up, F* flux_dn, RrxBool do_broadband, F* flux_up_loc, F* flux_dn_loc, void* stream) \
{ \
    return lw_solver_2stream_impl<F>(ncol, nlay, ngpt, top_at_1, tau, ssa, g, lev_source, sfc_emis, sfc_src, inc_flux, \
            flux_up, flux_dn, do_broadband, flux_up_loc, flux_dn_loc, stream); \
} \
int rrx_lw_solver_2stream_fractions##SFX( \
        int ncol, int nlay, int ngpt, int nbnd, RrxBool top_at_1, \
        const F* tau, const F* pfrac, const F* blev, const int* gpoint_bands, const int* band_lims_gpt, \
        const F* cld_tau, const F* cld_ssa, const F* cld_g, \
        const F* sfc_emis, const F* sfc_src, const F* inc_flux, F* flux_up, F* flux_dn, void* stream) \
{ \
    return lw_solver_2stream_fractions_impl<F>(ncol, nlay, ngpt, nbnd, top_at_1, tau, pfrac, blev, gpoint_bands, band_lims_gpt, \
            cld_tau, cld_ssa, cld_g, sfc_emis, sfc_src, inc_flux, flux_up, flux_dn, stream); \
}

RRX_DEFINE_LW2S(double, _f64)
RRX_DEFINE_LW2S(float, _f32)
}
