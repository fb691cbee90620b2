// Counter-based random numbers shared by the device files that draw them (rrx_mcica.hip, rrx_raytracer.hip): Philox4x32-10 and
// the 24-bit uniform. Each file documents its own counter and draw convention.
#ifndef RRX_PHILOX_H
#define RRX_PHILOX_H

#include <hip/hip_runtime.h>

namespace rrx
{
    struct Philox { unsigned w[4]; };

    // Philox4x32-10 (Salmon et al. 2011)
    __device__ __forceinline__ Philox philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
    {
        #pragma unroll
        for (int r=0; r<10; ++r)
        {
            const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
            const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
            c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        return Philox{{c0, c1, c2, c3}};
    }

    // 24 significant bits: exact in fp32 and fp64, in (0, 1), the same value in both
    template<typename F>
    __device__ __forceinline__ F uniform(const unsigned x) { return (F(x >> 9) + F(0.5)) * F(1.1920928955078125e-07); }
}

#endif
