// Column ordering for the product chain (round 4; no counterpart in the reference library): columns are independent, so a solve
// may process them in any order. Two uses, one mechanism -- a gather index `perm` of length ncol + npad:
//   * order: ascending surface pressure. The windowed gas optics stages one box of LUT nodes per 256 neighbouring cells; columns
//     that differ by more than about one cell of the LUT's pressure grid do not fit a box and are handed back to the gather kernels
//     (+60 % per step at +-35 % pressure spread). Sorted, neighbours are alike again.
//   * padding: perm[ncol .. ncol+npad) repeats the last column, so that the solve runs on a multiple of 16 columns (rows of the
//     (col, lay, gpt) arrays then start on 128-B lines: 16 385 columns cost 20 % more than 16 384 unpadded).
// Inputs are gathered through perm, outputs scattered back through its first ncol entries. Pure data movement + one radix sort.
#include "rrx_common.h"
#include "rrx_hip.h"
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

namespace
{
using namespace rrx;

__global__ void iota_pad_kernel(const int ncol, const int npad, int* __restrict__ perm)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i < ncol + npad) perm[i] = min(i, ncol-1);
}

__global__ void pad_perm_kernel(const int ncol, const int npad, int* __restrict__ perm)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i < npad) perm[ncol + i] = perm[ncol-1];
}

// flag = 1 where some run of `block` consecutive columns spans more than `threshold` of its mean (one workgroup per run)
template<typename F>
__global__ void __launch_bounds__(256) column_spread_kernel(const int ncol, const F* __restrict__ key, const int block, const F threshold, int* __restrict__ flag)
{
    __shared__ F s_min[256], s_max[256], s_sum[256];
    const int c0 = blockIdx.x*block;
    F lo = (sizeof(F) == 8) ? F(1e300) : F(3e38), hi = -lo, sum = F(0.);
    for (int i = c0 + threadIdx.x; i < min(c0 + block, ncol); i += 256) { const F v = key[i]; lo = min(lo, v); hi = max(hi, v); sum += v; }
    s_min[threadIdx.x] = lo; s_max[threadIdx.x] = hi; s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int s=128; s>0; s>>=1)
    {
        if (int(threadIdx.x) < s)
        {
            s_min[threadIdx.x] = min(s_min[threadIdx.x], s_min[threadIdx.x+s]); s_max[threadIdx.x] = max(s_max[threadIdx.x], s_max[threadIdx.x+s]);
            s_sum[threadIdx.x] += s_sum[threadIdx.x+s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0)
    {
        const int n = min(c0 + block, ncol) - c0;
        if (n == block && (s_max[0] - s_min[0]) > threshold * (s_sum[0] / F(n))) atomicExch(flag, 1);
    }
}

// out(i, r) = in(perm[i], r): arrays whose FIRST (fastest) dimension is the column
template<typename T>
__global__ void gather_cols_kernel(const int nout, const size_t nrest, const int* __restrict__ perm, const int ncol_in, const T* __restrict__ in, T* __restrict__ out)
{
    const size_t r = blockIdx.y;
    for (int i = blockIdx.x*blockDim.x + threadIdx.x; i < nout; i += gridDim.x*blockDim.x)
        for (size_t rr = r; rr < nrest; rr += gridDim.y) out[i + rr*nout] = in[perm[i] + rr*ncol_in];
}

// out(perm[i], r) = in(i, r), i < n: the inverse, into an array of ncol_dst columns from one of ncol_src
template<typename T>
__global__ void scatter_cols_kernel(const int n, const size_t nrest, const int* __restrict__ perm, const int ncol_src, const T* __restrict__ in, const int ncol_dst, T* __restrict__ out)
{
    const size_t r = blockIdx.y;
    for (int i = blockIdx.x*blockDim.x + threadIdx.x; i < n; i += gridDim.x*blockDim.x)
        for (size_t rr = r; rr < nrest; rr += gridDim.y) out[perm[i] + rr*ncol_dst] = in[i + rr*ncol_src];
}

// out(b, i) = in(b, perm[i]): arrays whose LAST dimension is the column, e.g. emis_sfc(nbnd, ncol)
template<typename T>
__global__ void gather_lastdim_kernel(const int n1, const int nout, const int* __restrict__ perm, const T* __restrict__ in, T* __restrict__ out)
{
    const size_t n = size_t(n1)*nout;
    for (size_t k = size_t(blockIdx.x)*blockDim.x + threadIdx.x; k < n; k += size_t(gridDim.x)*blockDim.x)
    {
        const int b = int(k % n1), i = int(k / n1);
        out[k] = in[b + size_t(perm[i])*n1];
    }
}

// Sunlit columns: perm[0 .. count) = the entries of `order` (or 0..ncol-1) whose mu0 > 0, in order; then repeats of the last one up
// to a multiple of pad_to. One workgroup of 16 waves walks the list in chunks of SUNLIT_PER_THREAD x 1024 entries: element
// (j, wave, lane) of a chunk is entry base + j*1024 + wave*64 + lane, so a wave64 ballot per (j, wave) plus one scan over the
// 16 x SUNLIT_PER_THREAD ballot counts gives every kept entry its place. Night = not (mu0 > 0): 0, -0.0, negatives and NaN.
constexpr int SUNLIT_WAVES = 16, SUNLIT_PER_THREAD = 8, SUNLIT_SLOTS = SUNLIT_WAVES*SUNLIT_PER_THREAD;
static_assert(SUNLIT_SLOTS == 128, "the slot scan gives two slots to each lane of one wave");

template<typename F>
__global__ void __launch_bounds__(64*SUNLIT_WAVES) sunlit_columns_kernel(
        const int ncol, const F* __restrict__ mu0, const int* __restrict__ order, const int pad_to, int* __restrict__ perm, int* __restrict__ count)
{
    __shared__ int s_off[SUNLIT_SLOTS];
    __shared__ int s_total, s_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int carry = 0, last = 0;
    for (int base = 0; base < ncol; base += SUNLIT_PER_THREAD*64*SUNLIT_WAVES)
    {
        int col[SUNLIT_PER_THREAD];
        bool day[SUNLIT_PER_THREAD];
        #pragma unroll
        for (int j=0; j<SUNLIT_PER_THREAD; ++j)
        {
            const int i = base + j*64*SUNLIT_WAVES + int(threadIdx.x);
            col[j] = (i < ncol) ? (order ? order[i] : i) : 0;
        }
        #pragma unroll
        for (int j=0; j<SUNLIT_PER_THREAD; ++j)
        {
            const int i = base + j*64*SUNLIT_WAVES + int(threadIdx.x);
            day[j] = (i < ncol) && (mu0[col[j]] > F(0.));
        }
        unsigned long long mask[SUNLIT_PER_THREAD];
        #pragma unroll
        for (int j=0; j<SUNLIT_PER_THREAD; ++j)
        {
            mask[j] = __ballot(day[j]);
            if (lane == 0) s_off[j*SUNLIT_WAVES + wave] = __popcll(mask[j]);
        }
        __syncthreads();
        if (wave == 0)          // exclusive scan of the 128 slot counts: two slots per lane, then a wave64 shuffle scan
        {
            const int a = s_off[2*lane], b = s_off[2*lane+1];
            int incl = a + b;
            #pragma unroll
            for (int d=1; d<64; d<<=1)
            {
                const int v = __shfl_up(incl, d, 64);
                if (lane >= d) incl += v;
            }
            const int excl = incl - (a + b);
            s_off[2*lane] = excl; s_off[2*lane+1] = excl + a;
            if (lane == 63) s_total = incl;
        }
        __syncthreads();
        const int total = s_total;
        #pragma unroll
        for (int j=0; j<SUNLIT_PER_THREAD; ++j)
            if (day[j])
            {
                const int p = s_off[j*SUNLIT_WAVES + wave] + __popcll(mask[j] & below);
                perm[carry + p] = col[j];
                if (p == total - 1) s_last = col[j];     // the chunk's last kept entry (the padding repeats the list's last)
            }
        carry += total;
        __syncthreads();
        if (total > 0) last = s_last;
        __syncthreads();        // s_off / s_total / s_last are rewritten by the next chunk
    }
    const long long n_out = (carry + (long long)pad_to - 1) / pad_to * pad_to;
    for (long long i = carry + int(threadIdx.x); i < n_out; i += 64*SUNLIT_WAVES) perm[i] = last;
    if (threadIdx.x == 0) *count = carry;
}

// out(:, r) = 0, then out(perm[i], r) = in(i, r) for i < n: the night columns of a sunlit-only solve (and any other column not in
// perm[0 .. n)) come out as exact zeros
template<typename T>
__global__ void fill_zero_kernel(const size_t n, T* __restrict__ out)
{
    for (size_t k = size_t(blockIdx.x)*blockDim.x + threadIdx.x; k < n; k += size_t(gridDim.x)*blockDim.x) out[k] = T(0);
}

inline dim3 grid2(const int n, const size_t nrest) { return dim3(std::min(ceil_div(n, 256), 256), unsigned(std::min<size_t>(nrest, 4096))); }

template<typename F>
int sunlit_columns_impl(const int ncol, const F* mu0, const int* order, const int pad_to, int* perm, int* count, void* stream, const char* name)
{
    RRX_TRY
    if (ncol < 0) throw std::runtime_error("ncol < 0");
    if (pad_to < 1) throw std::runtime_error("pad_to < 1");
    if (mu0 == nullptr && ncol > 0) throw std::runtime_error("mu0 is null");
    if (perm == nullptr) throw std::runtime_error("perm is null");
    if (count == nullptr) throw std::runtime_error("count is null");
    sunlit_columns_kernel<F><<<1, 64*SUNLIT_WAVES, 0, static_cast<hipStream_t>(stream)>>>(ncol, mu0, order, pad_to, perm, count);
    RRX_CATCH(name)
}

template<typename F>
int scatter_cols_fill_impl(const int n, const unsigned long long nrest, const int* perm, const int ncol_src, const F* in, const int ncol_dst,
                           F* out, void* stream, const char* name)
{
    RRX_TRY
    if (n < 0 || ncol_dst < 0 || ncol_src < 0) throw std::runtime_error("negative column count");
    if (n > ncol_src) throw std::runtime_error("n > ncol_src");
    if (n > 0 && (perm == nullptr || in == nullptr)) throw std::runtime_error("perm or in is null");
    if (out == nullptr && ncol_dst > 0 && nrest > 0) throw std::runtime_error("out is null");
    if (ncol_dst == 0 || nrest == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t ntot = size_t(ncol_dst)*size_t(nrest);
    fill_zero_kernel<F><<<unsigned(std::min<size_t>(ceil_div(ntot, size_t(256)), 4096)), 256, 0, st>>>(ntot, out);
    if (n > 0) scatter_cols_kernel<F><<<grid2(n, nrest), 256, 0, st>>>(n, size_t(nrest), perm, ncol_src, in, ncol_dst, out);
    RRX_CATCH(name)
}

// Spherical-geometry correction of the solar zenith angle: one thread per (column, layer), the column on the lanes.
// The operations are written one by one in the order of the formula (no contraction), so that a host evaluation in the same
// precision rounds alike.
template<typename F>
__global__ void __launch_bounds__(256)
zenith_spherical_kernel(const int ncol, const int nlay, const F* __restrict__ ref_alt, const F* __restrict__ ref_mu,
                        const F* __restrict__ alt, const F radius, F* __restrict__ mu0_lay)
{
    #pragma clang fp contract(off)
    const int icol = blockIdx.x*blockDim.x + threadIdx.x;
    if (icol >= ncol) return;
    const F m = ref_mu[icol];
    const F r0 = radius + ((ref_alt != nullptr) ? ref_alt[icol] : F(0.));
    const F sin2 = F(1.) - m*m;
    for (int ilay = blockIdx.y; ilay < nlay; ilay += gridDim.y)
    {
        const size_t o = size_t(ilay)*size_t(ncol) + icol;
        const F ratio = r0 / (radius + alt[o]);
        const F c2 = F(1.) - sin2*(ratio*ratio);
        mu0_lay[o] = (m > F(0.)) ? sqrt(max(F(0.), c2)) : m;
    }
}

template<typename F>
int zenith_spherical_impl(const int ncol, const int nlay, const F* ref_alt, const F* ref_mu, const F* alt, const F radius, F* mu0_lay,
                          void* stream, const char* name)
{
    RRX_TRY
    if (ncol < 0 || nlay < 0) throw std::runtime_error("negative extent");
    if (!(radius > F(0.))) throw std::runtime_error("planet_radius must be positive");
    if (ncol == 0 || nlay == 0) return 0;
    if (ref_mu == nullptr) throw std::runtime_error("ref_mu is NULL");
    if (alt == nullptr) throw std::runtime_error("alt is NULL");
    if (mu0_lay == nullptr) throw std::runtime_error("mu0_lay is NULL");
    zenith_spherical_kernel<F><<<dim3(ceil_div(ncol, 256), std::min(nlay, 4096)), 256, 0, static_cast<hipStream_t>(stream)>>>(
            ncol, nlay, ref_alt, ref_mu, alt, radius, mu0_lay);
    RRX_CATCH(name)
}

template<typename F>
int sort_columns_impl(const int ncol, const F* key, const int npad, int* perm, void* stream)
{
    RRX_TRY
    if (ncol <= 0 || npad < 0) throw std::runtime_error("empty problem");
    hipStream_t st = static_cast<hipStream_t>(stream);
    StreamScratch scratch(st);
    int* iota = scratch.get<int>(size_t(ncol));
    F* keys_out = scratch.get<F>(size_t(ncol));
    iota_pad_kernel<<<ceil_div(ncol, 256), 256, 0, st>>>(ncol, 0, iota);
    size_t temp_bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, temp_bytes, key, keys_out, iota, perm, size_t(ncol), 0, 8*sizeof(F), st) != hipSuccess)
        throw std::runtime_error("radix sort set-up failed");
    void* temp = scratch.get<char>(std::max<size_t>(temp_bytes, 16));
    if (rocprim::radix_sort_pairs(temp, temp_bytes, key, keys_out, iota, perm, size_t(ncol), 0, 8*sizeof(F), st) != hipSuccess)
        throw std::runtime_error("radix sort failed");
    if (npad > 0) pad_perm_kernel<<<ceil_div(npad, 256), 256, 0, st>>>(ncol, npad, perm);
    RRX_CATCH("rrx_sort_columns")
}
}  // namespace


extern "C"
{
int rrx_identity_columns(int ncol, int npad, int* perm, void* stream)
{
    RRX_TRY
    if (ncol <= 0 || npad < 0) throw std::runtime_error("empty problem");
    iota_pad_kernel<<<rrx::ceil_div(ncol + npad, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(ncol, npad, perm);
    RRX_CATCH("rrx_identity_columns")
}

#define RRX_DEFINE_COLUMNS(F, SFX) \
int rrx_sort_columns##SFX(int ncol, const F* key, int npad, int* perm, void* stream) { return sort_columns_impl<F>(ncol, key, npad, perm, stream); } \
int rrx_column_spread##SFX(int ncol, const F* key, int block, F threshold, int* flag, void* stream) \
{ RRX_TRY if (ncol <= 0 || block <= 0) throw std::runtime_error("empty problem"); \
  hipStream_t st = static_cast<hipStream_t>(stream); \
  if (hipMemsetAsync(flag, 0, sizeof(int), st) != hipSuccess) throw std::runtime_error("memset failed"); \
  column_spread_kernel<F><<<rrx::ceil_div(ncol, block), 256, 0, st>>>(ncol, key, block, threshold, flag); RRX_CATCH("rrx_column_spread") } \
int rrx_gather_cols##SFX(int nout, unsigned long long nrest, const int* perm, int ncol_in, const F* in, F* out, void* stream) \
{ RRX_TRY if (nout <= 0 || nrest == 0) return 0; \
  gather_cols_kernel<F><<<grid2(nout, nrest), 256, 0, static_cast<hipStream_t>(stream)>>>(nout, size_t(nrest), perm, ncol_in, in, out); RRX_CATCH("rrx_gather_cols") } \
int rrx_scatter_cols##SFX(int n, unsigned long long nrest, const int* perm, int ncol_src, const F* in, int ncol_dst, F* out, void* stream) \
{ RRX_TRY if (n <= 0 || nrest == 0) return 0; \
  scatter_cols_kernel<F><<<grid2(n, nrest), 256, 0, static_cast<hipStream_t>(stream)>>>(n, size_t(nrest), perm, ncol_src, in, ncol_dst, out); RRX_CATCH("rrx_scatter_cols") } \
int rrx_gather_lastdim##SFX(int n1, int nout, const int* perm, const F* in, F* out, void* stream) \
{ RRX_TRY if (n1 <= 0 || nout <= 0) return 0; \
  gather_lastdim_kernel<F><<<rrx::ceil_div(size_t(n1)*nout, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(n1, nout, perm, in, out); RRX_CATCH("rrx_gather_lastdim") } \
int rrx_sunlit_columns##SFX(int ncol, const F* mu0, const int* order, int pad_to, int* perm, int* count, void* stream) \
{ return sunlit_columns_impl<F>(ncol, mu0, order, pad_to, perm, count, stream, "rrx_sunlit_columns" #SFX); } \
int rrx_scatter_cols_fill##SFX(int n, unsigned long long nrest, const int* perm, int ncol_src, const F* in, int ncol_dst, F* out, void* stream) \
{ return scatter_cols_fill_impl<F>(n, nrest, perm, ncol_src, in, ncol_dst, out, stream, "rrx_scatter_cols_fill" #SFX); } \
int rrx_zenith_angle_spherical_correction##SFX(int ncol, int nlay, const F* ref_alt, const F* ref_mu, const F* alt, F planet_radius, \
        F* mu0_lay, void* stream) \
{ return zenith_spherical_impl<F>(ncol, nlay, ref_alt, ref_mu, alt, planet_radius, mu0_lay, stream, "rrx_zenith_angle_spherical_correction" #SFX); }

RRX_DEFINE_COLUMNS(double, _f64)
RRX_DEFINE_COLUMNS(float, _f32)
}
