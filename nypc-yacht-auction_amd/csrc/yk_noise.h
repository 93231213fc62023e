// yk_noise.h - the Dirichlet root-noise sampler: eta ~ Dir(alpha) over the V valid
// actions of a root, a function of (seed, env id, move, V, alpha) only.  One device function,
// block_dirichlet, is shared by the engine's k_root_noise and by yk_dirichlet_noise, so the noise a
// search sees and the noise the standalone entry point returns are the same bits.
//
// Counter domain (yk_philox.h): the noise uses counter (i, j, env, PHILOX_NOISE | move), so no noise draw
// can coincide with a draw of any game stream, and the game's own counter is not advanced.
//
// All arithmetic is f64 without contraction (-ffp-contract=off): an accept test of the rejection
// loop then differs between this code and a host restatement only when it lands within an ulp or
// two of equality.
#pragma once
#include <math.h>
#include <stdint.h>

#include "yk_common.h"

namespace yk {

constexpr int NOISE_THREADS = 256;   // workgroup size block_dirichlet is written for
constexpr int NOISE_MAX_TRIES = 4096;  // rejection-loop bound (acceptance > 0.95 per try: never reached)

// uniform in (0, 1) from draw i of valid action j: ((x >> 11) + 0.5) 2^-53, the sum rounded to f64
__device__ __host__ inline double noise_u53(uint64_t seed, uint32_t env, uint32_t move, uint32_t j, uint32_t i) {
    const uint64_t x = philox_u64(philox4x32_10(seed, i, j, env, PHILOX_NOISE | move));
    return ((double)(x >> 11) + 0.5) * TWO_M53;
}

// Gamma(alpha, 1) of valid action j: Marsaglia-Tsang, alpha < 1 boosted by u^(1 / alpha)
__device__ __host__ inline double noise_gamma(uint64_t seed, uint32_t env, uint32_t move, uint32_t j, double alpha) {
    const double a = alpha < 1.0 ? alpha + 1.0 : alpha;
    const double d = a - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    uint32_t i = 0;
    double g = d;
    for (int tries = 0; tries < NOISE_MAX_TRIES; tries++) {
        const double u1 = noise_u53(seed, env, move, j, i);
        const double u2 = noise_u53(seed, env, move, j, i + 1);
        const double u3 = noise_u53(seed, env, move, j, i + 2);
        i += 3;
        const double x = sqrt(-2.0 * log(u1)) * cos(2.0 * 3.141592653589793 * u2);
        const double t = 1.0 + c * x;
        if (t <= 0.0) continue;
        const double v = t * t * t;
        if (log(u3) < 0.5 * x * x + d - d * v + d * log(v)) {
            g = d * v;
            break;
        }
    }
    if (alpha < 1.0) g *= pow(noise_u53(seed, env, move, j, i), 1.0 / alpha);
    return g;
}

#ifdef __HIPCC__
// eta[0 .. V-1] into `eta` (LDS, >= V doubles) for one root, by a workgroup of NOISE_THREADS threads:
// thread tid samples the gammas of j = tid, tid + 256, ... (each lane runs its own rejection loop);
// the sum is taken in a fixed order - each thread's entries in ascending j, the wave's 64 partials in
// xlane_sum's butterfly, the four waves' sums left to right; eta[j] = g[j] / sum, or 1 / V when every
// gamma underflowed.  `wsum` is 4 doubles of LDS.  Ends with the block synchronised.
__device__ __forceinline__ void block_dirichlet(uint64_t seed, uint32_t env, uint32_t move, int V, double alpha,
                                                double* eta, double* wsum) {
    const int tid = threadIdx.x;
    double part = 0.0;
    for (int j = tid; j < V; j += NOISE_THREADS) {
        const double g = noise_gamma(seed, env, move, (uint32_t)j, alpha);
        eta[j] = g;
        part += g;
    }
    part = xlane_sum(part);
    if ((tid & 63) == 0) wsum[tid >> 6] = part;
    __syncthreads();
    const double sum = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    const double unif = 1.0 / (double)V;
    for (int j = tid; j < V; j += NOISE_THREADS) eta[j] = sum > 0.0 ? eta[j] / sum : unif;
    __syncthreads();
}
#endif

}  // namespace yk
