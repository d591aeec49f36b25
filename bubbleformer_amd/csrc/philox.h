// Philox4x32-10 with Random123's constants, one definition for the translation units that draw from it: the input noise (noise.hip: one block
// per group of four elements, counter word 0 = the group, < 2^29) and the clip augmentation (clip_store.hip: one block per sample, counter
// word 0 = 0xFFFFFFFF).  The key is a 64-bit seed, low word first.
#pragma once
#include "bf_common.h"

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

struct Quad { uint32_t w[4]; };
__device__ __forceinline__ Quad philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    return Quad{{c0, c1, c2, c3}};
}
