// yk_philox.h - the library's one Philox4x32-10 (the RNG contract of oracle/spec.py) and the registry of its
// counter domains.  Every random number of the library is a function of (seed, counter) only: the 64-bit seed
// is the key (lo, hi), the four counter words say which draw it is.
//
// Counter word 3 is the domain.  Two draws of different domains can never coincide, whatever words 0..2
// hold, so a feature's draws do not disturb, and are not disturbed by, any other's:
//   PHILOX_GAME       (ctr lo, ctr hi, env, .)      a game's draw stream (philox_draw; the trainers' dropout
//                                                   masks are such streams, env = 0x44524F50 + layer)
//   PHILOX_REANALYSE  (k lo, k hi, key, .)          whether a refresh searches example k again
//   PHILOX_SAMPLE     (j lo, j hi, key, .)          draw j of weighted minibatch sampling
//   PHILOX_PLAYOUT    (move, env base, 0, .)        whether a self-play batch searches that move in full
//   PHILOX_SYMMETRY   (draw, example, epoch key, .) the symmetry drawn for an example
//   PHILOX_NOISE|move (draw, action, env, .)        Dirichlet root noise: every word with bit 31 set
// A new feature takes the lowest multiple of 0x10000000 below 0x80000000 that is not listed (0x50000000
// next), names it here and in this comment, and uses no other word 3.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace yk {

constexpr uint32_t PHILOX_GAME = 0u;
constexpr uint32_t PHILOX_REANALYSE = 0x10000000u;
constexpr uint32_t PHILOX_SAMPLE = 0x20000000u;
constexpr uint32_t PHILOX_PLAYOUT = 0x30000000u;
constexpr uint32_t PHILOX_SYMMETRY = 0x40000000u;
constexpr uint32_t PHILOX_NOISE = 0x80000000u;

struct Philox4 {
    uint32_t x0, x1, x2, x3;
};
__device__ __host__ __forceinline__ Philox4 philox4x32_10(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2,
                                                          uint32_t c3) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{c0, c1, c2, c3};
}
// the 64-bit draw: x0 | x1 << 32
__device__ __host__ __forceinline__ uint64_t philox_u64(const Philox4& x) { return (uint64_t)x.x0 | ((uint64_t)x.x1 << 32); }
// uniform in [0, 1) from the top 53 bits of a 64-bit draw
constexpr double TWO_M53 = 1.0 / 9007199254740992.0;
__device__ __host__ __forceinline__ double u53(uint64_t x) { return (double)(x >> 11) * TWO_M53; }

}  // namespace yk
