// philox.h -- the library's counter-based random stream: Philox4x32-10 keyed by a 64-bit seed, counter (index, call lo,
// call hi, purpose).  A draw is a function of its counter alone, so a kernel recomputes it wherever it needs it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hpl {

// The purposes in use (the counter's fourth word): no two users of one (seed, call) share a stream.
constexpr uint32_t PHILOX_JITTER1 = 0;           // transforms.hip: the jitter of cloud 1 / cloud 2,
constexpr uint32_t PHILOX_JITTER2 = 1;
constexpr uint32_t PHILOX_SELECT1 = 2;           // the selection keys of cloud 1 / cloud 2
constexpr uint32_t PHILOX_SELECT2 = 3;
constexpr uint32_t PHILOX_GROUND = 16;           // ground_fit.hip: the three points of hypothesis h

struct u4 { uint32_t x, y, z, w; };

__host__ __device__ inline uint32_t mulhilo(uint32_t a, uint32_t b, uint32_t *hi) {
    const uint64_t p = (uint64_t)a * b;
    *hi = (uint32_t)(p >> 32);
    return (uint32_t)p;
}

// Philox4x32-10 (Salmon et al., SC'11): 10 rounds, key bumped between rounds.
__host__ __device__ inline u4 philox4x32_10(u4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        uint32_t hi0, hi1;
        const uint32_t lo0 = mulhilo(0xD2511F53u, c.x, &hi0);
        const uint32_t lo1 = mulhilo(0xCD9E8D57u, c.z, &hi1);
        c = u4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    }
    return c;
}

}  // namespace hpl
