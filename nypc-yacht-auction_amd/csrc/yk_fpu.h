// yk_fpu.h - first-play urgency (FPU reduction: Leela, KataGo): the one statement of the
// arithmetic, shared by the search kernels (yk_engine.hip: the full UCB scan and root_scan) and the stand-alone
// entry point (yk_fpu.hip).  Every quantity is a double or an integer unless it says float; the units are
// built with -ffp-contract=off, so each operation rounds once and plain Python ints and floats give the same bits.
//
// At a node with Ns > 0, a visited edge and an unvisited valid edge:
//   visited candidate     the largest u_j = f32(Q_j) + ((c32 P_j) sq) / f32(1 + N_j), the lowest index among equals
//   unvisited candidate   the largest x_j = (c32 P_j) sqe, the lowest index among equals
//   parent estimate       W  = sum N_j llrint(Q_j 2^32)      (int64, over the visited edges)
//                         Mi = sum (uint64)((double)P_j 2^40) (truncated, over the visited edges)
//                         fq = (float)((W / Ns) / 2^32 - r sqrt(Mi / 2^40))
//   winner                u_unv = fq + x_best (one f32 add) against the visited u: the larger, the lower index
//                         on equality
// The sums are integers, so every order of summation - lanes, wave reductions, a visited list in backup order -
// gives the same bits.  |W| <= Ns 2^32 (|Q| <= 1) and Mi <= V 2^40 are exact in a double.
#pragma once
#include <math.h>
#include <stdint.h>

#include "yk_common.h"

namespace {

// The feature's own kernel argument (as ForcedDev: EngDev is the same with and without the feature).  Only
// the FPU instantiations of the search kernels read it.
struct FpuDev {
    double r;       // the reduction at interior nodes (>= 0)
    double r_root;  // and at depth 0 of a search
};

// One visited edge's terms of the two sums
__device__ __forceinline__ int64_t fpu_w_term(uint32_t N, double Q) {
    return (int64_t)N * (int64_t)llrint(Q * 4294967296.0);  // (ties to even: the default rounding mode)
}
__device__ __forceinline__ uint64_t fpu_m_term(float P) {
    return (uint64_t)((double)P * 1099511627776.0);  // (a P below 2^-40 adds nothing)
}

// The wave's sum of a 64-bit integer, on every lane (two's complement: W's terms add as unsigned words)
template <int O = 32>
__device__ __forceinline__ uint64_t fpu_wave_sum(uint64_t v) {
    v += (uint64_t)yk::xlane_u<O>((uint32_t)v) | ((uint64_t)yk::xlane_u<O>((uint32_t)(v >> 32)) << 32);
    if constexpr (O > 1) return fpu_wave_sum<O / 2>(v);
    return v;
}

// The unvisited edges' starting value: the visited children's visit-weighted mean less r sqrt(prior mass tried)
__device__ __forceinline__ float fpu_value(int64_t W, uint64_t Mi, uint32_t Ns, double r) {
    const double qbar = ((double)W / (double)Ns) / 4294967296.0;
    const double mass = (double)Mi / 1099511627776.0;
    return (float)(qbar - r * sqrt(mass));
}

// The winner of a node with both kinds of edge: true when the unvisited candidate (x at index ju) beats the
// visited one (u at index jv)
__device__ __forceinline__ bool fpu_unvisited_wins(float fq, float x, int ju, float u, int jv) {
    const float uu = fq + x;
    return uu > u || (uu == u && ju < jv);
}

}  // namespace
