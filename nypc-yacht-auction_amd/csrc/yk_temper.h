// yk_temper.h - the two self-play temperatures, stated once: the draw of a real move from
// N^(1/T), and the root prior P^(1/T) renormalised.  The engine's k_move_end and k_root_noise and the
// standalone entry points yk_temperature_pick and yk_root_temper (yk_temper.hip) run these device functions,
// so a game and a crafted row see the same bits.
//
// The temperatures themselves come from tables the host builds (yk_temperature_schedule): the device reads
// T and never evaluates the schedule.  All arithmetic is f64 without contraction (-ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#include "yk_common.h"

namespace yk {

constexpr int TEMPER_THREADS = 256;  // workgroup size block_temper_weights is written for (NOISE_THREADS)

// The schedules of one engine as the kernels see them: max_moves doubles each, indexed by the real move.
struct TemperDev {
    const double* move_t;  // move-selection temperature (NULL: off)
    const double* root_t;  // root policy temperature (NULL: off)
};

#ifdef __HIPCC__
// LDS writes of this wave are visible to its other lanes after this (no workgroup barrier: one wave per row)
__device__ __forceinline__ void temper_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// The move draw, by one wave: entry i of a row of n visit counts (count(i), ascending action) is picked with
// probability proportional to w_i = pow((double)n_i, inv_t).  The arithmetic is the temp-1 sampler's
// (np.random.choice: cumsum, /= cdf[-1], searchsorted(u, 'right')) on w in place of the counts, every sum
// sequential and left to right:
//   total = sum w_i;  c_i = c_(i-1) + w_i / total;  last = c_(n-1);  the first i with c_i / last > u.
// The wave computes 64 entries' terms at a time, each lane one pow (and one division), into `stage` (64
// doubles of LDS, this wave's own); lane 0 adds a piece's terms in ascending order, so the sums are the
// sequential ones.  Three passes (total, last, the pick), each recomputing its terms: no array of n doubles.
// Returns the picked index on every lane - -1 when total is not > 0 (an empty row) or no entry passes u - and
// the total in *total.
template <class C>
__device__ __forceinline__ int wave_temper_pick(C&& count, int n, double inv_t, double u, double* stage, int lane,
                                                double* total) {
    double tot = 0.0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        stage[lane] = i < n ? pow((double)count(i), inv_t) : 0.0;
        temper_wave_sync();
        if (lane == 0) {
            const int m = min(64, n - i0);
            for (int k = 0; k < m; k++) tot += stage[k];
        }
        temper_wave_sync();
    }
    tot = lane_val(tot, 0);
    *total = tot;
    if (!(tot > 0.0)) return -1;
    double last = 0.0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        stage[lane] = i < n ? pow((double)count(i), inv_t) / tot : 0.0;
        temper_wave_sync();
        if (lane == 0) {
            const int m = min(64, n - i0);
            for (int k = 0; k < m; k++) last += stage[k];
        }
        temper_wave_sync();
    }
    last = lane_val(last, 0);
    double c = 0.0;
    int pick = -1;
    for (int i0 = 0; i0 < n && pick < 0; i0 += 64) {
        const int i = i0 + lane;
        stage[lane] = i < n ? pow((double)count(i), inv_t) / tot : 0.0;
        temper_wave_sync();
        if (lane == 0) {
            const int m = min(64, n - i0);
            for (int k = 0; k < m; k++) {
                c += stage[k];
                if (c / last > u) {
                    pick = i0 + k;
                    break;
                }
            }
        }
        temper_wave_sync();
        pick = (int)lane_val((uint32_t)pick, 0);
    }
    return pick;
}

// First pass of the root prior transform, by a workgroup of TEMPER_THREADS threads: w[j] = pow((double)P[j],
// inv_t) for the V entries of a compact prior into `w` (LDS, >= V doubles) and their sum S - each thread's
// entries in ascending j, the wave's 64 partials in xlane_sum's butterfly, the four waves' sums left to right
// (block_dirichlet's order).  P is read once; seen(j, P[j]) is called for every entry (the engine records the
// prior it found there).  `tsum` is 4 doubles of LDS of its own.  Thread tid writes and later reads w[tid],
// w[tid + 256], ...: the second pass needs no barrier beyond the one this ends with.
template <class F>
__device__ __forceinline__ double block_temper_weights(const float* P, int V, double inv_t, double* w, double* tsum,
                                                       F&& seen) {
    const int tid = threadIdx.x;
    double part = 0.0;
    for (int j = tid; j < V; j += TEMPER_THREADS) {
        const float p = P[j];
        seen(j, p);
        const double x = pow((double)p, inv_t);
        w[j] = x;
        part += x;
    }
    part = xlane_sum(part);
    if ((tid & 63) == 0) tsum[tid >> 6] = part;
    __syncthreads();
    return ((tsum[0] + tsum[1]) + tsum[2]) + tsum[3];
}
// Second pass, per entry: P'[j] = (float)(w[j] / S)
__device__ __forceinline__ float tempered_prior(double w, double S) { return (float)(w / S); }
#endif

}  // namespace yk
