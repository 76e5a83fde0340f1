// wrnn_philox.h -- the counter-based generator of the library's own sampling noise (wrnn_options.noise_lib, wrnn_noise_fill*), for host and device.
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants).  One round of a
// block (c0, c1, c2, c3) under the key (k0, k1):
//     (hi0, lo0) = 0xD2511F53 * c0,   (hi1, lo1) = 0xCD9E8D57 * c2            (32 x 32 -> 64 bit products)
//     (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
// ten rounds, the key stepped by (0x9E3779B9, 0xBB67AE85) between them (nine times).
//
// The noise value of (segment b, step t, index j) is made from ONE word and depends on nothing else:
//     key     = the call's 64-bit seed (lo, hi)
//     counter = (t, j / 4, id_lo, id_hi),  id = the segment's 64-bit stream id;   w = word j % 4 of the block;   k = w >> 8 (24 bits)
//     MOL (j = 0..9: the mixture-selection uniforms of utils/distribution.py:106, j = 10: the logistic uniform of :118 -- `uniform_(1e-5, 1 - 1e-5)`):
//         u = min(((float)k * 0x1p-24f) * 0.99998f + 1e-5f, 0.99999f)
//       every operation rounded to float32 on its own, nothing fused (the conversion and the first product are exact): any IEEE float32 arithmetic
//       reproduces it bit for bit.  k = 0 gives 1e-5f, k = 2^24 - 1 lands one ulp below 0.99999f: the min is a guard that no word triggers.
//     RAW (j = class; `exponential_`, as Categorical.sample -> multinomial draws it):
//         q = -logf(min(((float)k + 0.5f) * 0x1p-24f, 1 - 0x1p-24f))
//       finite and > 0 for every word.  From k = 2^23 on k + 0.5 is not a float32 and rounds to an even integer; for the single k = 2^24 - 1 that is
//       2^24, the argument would be 1 and q = 0 -- which the sampler divides by --, hence the min: that word gives q = -logf(1 - 2^-24) = 5.96e-8.
#pragma once
#include <stdint.h>
#include <math.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WRNN_HD __host__ __device__ inline
#else
#define WRNN_HD inline
#endif

namespace wrnn {

struct PhiloxBlock { uint32_t w[4]; };

WRNN_HD PhiloxBlock philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    PhiloxBlock b;
    b.w[0] = c0; b.w[1] = c1; b.w[2] = c2; b.w[3] = c3;
    return b;
}

// the block of (step t, indices 4 q .. 4 q + 3) of the segment with stream id `id`
WRNN_HD PhiloxBlock noise_block(uint64_t seed, uint64_t id, int32_t t, uint32_t q)
{
    return philox4x32_10((uint32_t)t, q, (uint32_t)id, (uint32_t)(id >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

WRNN_HD float noise_mol_value(uint32_t w)
{
#pragma clang fp contract(off)
    const float k = (float)(w >> 8);
    const float s = k * 0x1p-24f;       // (plain operators under the pragma, on the device too: the product and the sum inside __fmul_rn / __fadd_rn carry the
    const float m = s * 0.99998f;       // header's own contraction setting and are fused into one v_fma_f32 once inlined -- one ulp off in ~1 value of 5)
    const float u = m + 1e-5f;
    return u < 0.99999f ? u : 0.99999f;
}

WRNN_HD float noise_raw_value(uint32_t w)
{
#pragma clang fp contract(off)
    const float k = (float)(w >> 8);
    const float h = k + 0.5f;
    const float x = h * 0x1p-24f;
    return -logf(x < 0x1.fffffep-1f ? x : 0x1.fffffep-1f);
}

}  // namespace wrnn
