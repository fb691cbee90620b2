// Tabulated cloud phase functions of the ray tracers (the specification: rrx_rt_phase.h): the table builder and
// the two device functions phase_sample and phase_eval over arrays, which is the tracers' own code without a tracer around it.
//
// rrx_rt_phase_tables: from the nodes mu (nmu) and phase_raw (nmu, nre, nbnd) >= 0 of any normalisation to phase and cdf. One
// thread per (ire, ibnd), as k_null is built by one thread per block. The trapezoid sums A_i = sum_{j<i} 1/2 (P_j + P_j+1)
// (mu_j+1 - mu_j) are accumulated IN DOUBLE IN NODE ORDER in both precisions (numpy's cumsum restates them exactly), then
// cdf_i = F(A_i / A_last), so that the last node is exactly 1, and phase_i = F(P_i / (A_last/2)). A device flag reports
// 1: nodes that do not increase strictly from -1 to +1, 2: a table whose integral is not > 0 or not finite, or that holds a negative
// number; the entry waits for the launch and returns non-zero with the flag set (the outputs of a flagged table are not written).
#include "rrx_rt_phase.h"
#include "rrx_hip.h"

namespace
{
using namespace rrx;
using namespace rrx::rt;

template<typename F>
__global__ void __launch_bounds__(64) phase_tables_kernel(const int nmu, const int ntab, const F* __restrict__ mu,
                                                          const F* __restrict__ phase_raw, F* __restrict__ phase, F* __restrict__ cdf,
                                                          int* __restrict__ flag)
{
    const int n = blockIdx.x*blockDim.x + threadIdx.x;
    if (n >= ntab) return;
    const F* __restrict__ raw = phase_raw + size_t(n)*nmu;
    F* __restrict__ p = phase + size_t(n)*nmu;
    F* __restrict__ c = cdf + size_t(n)*nmu;
    bool nodes_ok = mu[0] == F(-1.) && mu[nmu-1] == F(1.), table_ok = raw[0] >= F(0.);
    double total = 0.;
    for (int i=1; i<nmu; ++i)
    {
        nodes_ok = nodes_ok && mu[i] > mu[i-1];
        table_ok = table_ok && raw[i] >= F(0.);
        total = total + (0.5*(double(raw[i-1]) + double(raw[i])))*(double(mu[i]) - double(mu[i-1]));
    }
    table_ok = table_ok && total > 0. && total < double(INFINITY);
    if (!nodes_ok) atomicOr(flag, 1);
    if (!table_ok) atomicOr(flag, 2);
    if (!nodes_ok || !table_ok) return;
    const double half = 0.5*total;
    double sum = 0.;
    c[0] = F(0.); p[0] = F(double(raw[0]) / half);
    for (int i=1; i<nmu; ++i)
    {
        sum = sum + (0.5*(double(raw[i-1]) + double(raw[i])))*(double(mu[i]) - double(mu[i-1]));
        c[i] = F(sum / total);
        p[i] = F(double(raw[i]) / half);
    }
}

template<typename F>
__global__ void __launch_bounds__(256) phase_sample_kernel(const long long n, const PhaseTable<F> t, const F* __restrict__ mu,
                                                           const F* __restrict__ u, const F* __restrict__ re, F* __restrict__ cos_out)
{
    const long long i = (long long)blockIdx.x*blockDim.x + threadIdx.x;
    if (i < n) cos_out[i] = phase_sample(t, mu, re[i], u[i]);
}

template<typename F>
__global__ void __launch_bounds__(256) phase_eval_kernel(const long long n, const PhaseTable<F> t, const F* __restrict__ mu,
                                                         const F* __restrict__ cs, const F* __restrict__ re, F* __restrict__ p_out)
{
    const long long i = (long long)blockIdx.x*blockDim.x + threadIdx.x;
    if (i < n) p_out[i] = phase_eval(t, mu, re[i], clampf(cs[i], F(-1.), F(1.)));
}

template<typename F>
int phase_tables_entry(const char* entry, int nmu, int nre, int nbnd, const F* mu, const F* phase_raw, F* phase, F* cdf, void* stream)
{
    RRX_TRY
    if (check_extents({{"nmu", nmu}, {"nre", nre}, {"nbnd", nbnd}}) && nbnd == 0) return 0;
    check_phase_extents(nmu, nre, F(1.));
    check_needed({{"mu", mu}, {"phase_raw", phase_raw}, {"phase", phase}, {"cdf", cdf}});
    if ((long long)nre*nbnd > 0x7FFFFFFFll) throw std::runtime_error("nre nbnd exceeds 2^31 - 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    WorkspaceLease lease(st);
    int* flag = lease.get<int>(1);
    if (hipMemsetAsync(flag, 0, sizeof(int), st) != hipSuccess) throw std::runtime_error("zeroing the flag failed");
    const int ntab = nre*nbnd;
    phase_tables_kernel<F><<<ceil_div(ntab, 64), 64, 0, st>>>(nmu, ntab, mu, phase_raw, phase, cdf, flag);
    int h = 0;
    if (hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        throw std::runtime_error("reading the flag failed");
    if (h & 1) throw std::runtime_error("mu does not increase strictly from -1 to +1");
    if (h & 2) throw std::runtime_error("a table of phase_raw has an integral that is not > 0 or not finite, or holds a negative number");
    RRX_CATCH(entry)
}

template<typename F, bool SAMPLE>
int phase_array_entry(const char* entry, long long n, int nmu, int nre, int nbnd, int ibnd, F re0, F dre, const F* mu, const F* phase,
                      const F* cdf, const F* in, const F* re, F* out, void* stream)
{
    RRX_TRY
    if (check_extents({{"n", n}})) return 0;
    check_phase_extents(nmu, nre, dre);
    if (nbnd < 1) throw std::runtime_error("nbnd must be >= 1");
    if (ibnd < 0 || ibnd >= nbnd) throw std::runtime_error("ibnd is outside [0, nbnd)");
    check_needed({{"mu", mu}, {"phase", phase}, {"cdf", cdf}, {SAMPLE ? "u" : "cs", in}, {"re", re}, {SAMPLE ? "cos_out" : "p_out", out}});
    const size_t off = size_t(nmu)*nre*ibnd;
    const PhaseTable<F> t{nmu, nre, re0, dre, phase + off, cdf + off};
    const unsigned blocks = unsigned((n + 255) / 256);
    if ((n + 255) / 256 > 0x7FFFFFFFll) throw std::runtime_error("n is too large for one launch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (SAMPLE) phase_sample_kernel<F><<<blocks, 256, 0, st>>>(n, t, mu, in, re, out);
    else phase_eval_kernel<F><<<blocks, 256, 0, st>>>(n, t, mu, in, re, out);
    RRX_CATCH(entry)
}
}  // namespace

extern "C"
{
#define RRX_DEFINE_RT_PHASE(F, SFX) \
int rrx_rt_phase_tables##SFX(int nmu, int nre, int nbnd, const F* mu, const F* phase_raw, F* phase, F* cdf, void* stream) \
{ return phase_tables_entry<F>("rrx_rt_phase_tables" #SFX, nmu, nre, nbnd, mu, phase_raw, phase, cdf, stream); } \
int rrx_rt_phase_sample##SFX(long long n, int nmu, int nre, int nbnd, int ibnd, F re0, F dre, const F* mu, const F* phase, const F* cdf, \
        const F* u, const F* re, F* cos_out, void* stream) \
{ return phase_array_entry<F,true>("rrx_rt_phase_sample" #SFX, n, nmu, nre, nbnd, ibnd, re0, dre, mu, phase, cdf, u, re, cos_out, stream); } \
int rrx_rt_phase_eval##SFX(long long n, int nmu, int nre, int nbnd, int ibnd, F re0, F dre, const F* mu, const F* phase, const F* cdf, \
        const F* cs, const F* re, F* p_out, void* stream) \
{ return phase_array_entry<F,false>("rrx_rt_phase_eval" #SFX, n, nmu, nre, nbnd, ibnd, re0, dre, mu, phase, cdf, cs, re, p_out, stream); }

RRX_DEFINE_RT_PHASE(double, _f64)
RRX_DEFINE_RT_PHASE(float, _f32)
}
