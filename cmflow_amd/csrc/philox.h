// Philox4x32-10, the one generator of the library: the sampling of cmf_draw_batch (draw_batch.hip) and the per-slot transform of
// cmf_augment_batch (augment.hip) take their words from it, on the host (the key of a call) and on the device (a slot's words).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

struct Philox { uint32_t x, y, z, w; };

__host__ __device__ inline uint32_t draw_mulhi(uint32_t a, uint32_t b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __umulhi(a, b);
#else
    return (uint32_t)(((unsigned long long)a * b) >> 32);
#endif
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): ten rounds of two 32 x 32 -> 64 multiplies, key bumped by the Weyl constants
__host__ __device__ inline Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = draw_mulhi(M0, c0), l0 = M0 * c0, h1 = draw_mulhi(M1, c2), l1 = M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += W0;
        k1 += W1;
    }
    return Philox{c0, c1, c2, c3};
}

// the key of a call: words 0, 1 with counter (seed lo, seed hi, draw lo, draw hi) and key (0, 0)
inline Philox philox_call_key(unsigned long long seed, unsigned long long draw)
{
    return philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)draw, (uint32_t)(draw >> 32), 0u, 0u);
}
