// Philox4x32-10 (Salmon et al., SC'11) as include/lisec_hip.h section 5c uses it: key = the 64-bit seed (low word, high
// word), counter = (stream, item, epoch, index).  Integer-exact, so a numpy restatement reproduces every draw bit for bit.
#pragma once
#include <cstdint>

namespace lisec {

struct U4 { uint32_t v[4]; };

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return U4{{c0, c1, c2, c3}};
}

}  // namespace lisec
