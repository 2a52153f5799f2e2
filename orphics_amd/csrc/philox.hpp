// Philox4x32-10 counter RNG + Box-Muller: the draw arithmetic shared by the GRF kernels (rng.hip) and by the draw fused into the
// inverse column pass (fft_kernels.hpp: GrfColLoad).  One counter -> four N(0, 1).  Host and device functions: the thread emulator
// runs them with the host's logf / sinf / cosf, so only the device's values are the pinned ones (tests/test_rng_parity_gpu.py).
#pragma once
#include <cmath>
#include <cstdint>
#include "cx.hpp"

namespace oa {

struct U4 { uint32_t x, y, z, w; };

OA_HD U4 philox4x32_10(U4 ctr, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // one 32 x 32 -> 64 multiply per product (v_mad_u64_u32) instead of a high and a low one: the quarter-rate integer
        // multiplies are what the draw kernels spend their time on
        const uint64_t p0 = (uint64_t)M0 * (uint64_t)ctr.x, p1 = (uint64_t)M1 * (uint64_t)ctr.z;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        U4 n;
        n.x = hi1 ^ ctr.y ^ k0;
        n.y = lo1;
        n.z = hi0 ^ ctr.w ^ k1;
        n.w = lo0;
        ctr = n;
        k0 += W0;
        k1 += W1;
    }
    return ctr;
}

// two N(0,1) from two 32-bit words
OA_HD void box_muller(uint32_t a, uint32_t b, float& n0, float& n1) {
    const float u1 = ((float)a + 0.5f) * 2.3283064365386963e-10f;  // (0,1]
    const float u2 = ((float)b + 0.5f) * 2.3283064365386963e-10f;
#if defined(OA_FAST_BOXMULLER) && defined(__HIP_DEVICE_COMPILE__)     // experiment: hardware log2 / sqrt / sin / cos (v_log_f32, v_sqrt_f32, v_sin_f32, v_cos_f32 take revolutions)
    const float l2 = __builtin_amdgcn_logf(u1);                    // log2(u1) <= 0
    const float r = __builtin_amdgcn_sqrtf(fmaxf(-1.3862943611198906f * l2, 0.0f));
    n0 = r * __builtin_amdgcn_cosf(u2);
    n1 = r * __builtin_amdgcn_sinf(u2);
#else
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
#if defined(__HIP_DEVICE_COMPILE__)
    sincospif(2.0f * u2, &s, &c);
#else      // host (the CPU thread emulator of tests/emul): the library's sine and cosine -- the same draw up to their rounding
    s = sinf(6.283185307179586f * u2); c = cosf(6.283185307179586f * u2);
#endif
    n0 = r * c;
    n1 = r * s;
#endif
}

// 4 normals for counter index `idx` of stream (seed, sid)
OA_HD void normals4(uint64_t seed, uint64_t sid, uint64_t idx, float* n) {
    U4 c;
    c.x = (uint32_t)idx; c.y = (uint32_t)(idx >> 32); c.z = (uint32_t)sid; c.w = (uint32_t)(sid >> 32);
    const U4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    box_muller(r.x, r.y, n[0], n[1]);
    box_muller(r.z, r.w, n[2], n[3]);
}

}  // namespace oa
