// yk_forced.h - forced playouts and policy target pruning (KataGo): the one statement of the
// arithmetic, shared by the search kernels (yk_engine.hip: the root's UCB pick, k_move_end) and the
// stand-alone entry point (yk_forced.hip).  Every quantity is a double unless it says float; the units are
// built with -ffp-contract=off, so each operation rounds once and plain Python floats give the same bits.
//
// For one move's root: Ns the root record's visit count, P the edge's prior (the float the search uses: the
// noised one under root noise), N and Q the edge's count and value, c = cpuct, k the knob.
#pragma once
#include <math.h>
#include <stdint.h>

namespace {

// The feature's own kernel argument (as NoiseDev: EngDev is the same with and without the feature).  Only
// the FORCED / PRUNE instantiations of the search kernels read it.
struct ForcedDev {
    double k;  // forced_playouts_k (> 0 in every kernel that reads it)
    double c;  // cpuct as the double the engine was configured with
};

// A visited edge is forced - its u is +inf in the root's scan - while N^2 < (k P) Ns.  Unvisited: never.
__device__ __forceinline__ bool forced_edge(uint32_t N, float P, uint32_t Ns, double k) {
    const double n = (double)N;
    return N > 0 && n * n < (k * (double)P) * (double)Ns;
}

// Q + (c P) sqrt(Ns) / (1 + n): an edge's PUCT value with n visits, in double (the search itself picks in
// float; this one only judges the finished move's counts).  f64 sqrt and division are correctly rounded.
__device__ __forceinline__ double puct_value(double Q, float P, uint32_t Ns, double c, uint32_t n) {
    return Q + (c * (double)P) * sqrt((double)Ns) / (double)(1u + n);
}

// One edge's pruned count (not the best child's, which keeps N): starting at n = N, one visit is taken off
// while n > 0, fewer than f were taken (f the largest integer with f^2 <= (k P) Ns: N - n < f is
// (N - n + 1)^2 <= (k P) Ns, both sides exact in double at these sizes and the square monotone beyond), and
// the edge with n - 1 visits would still rank below the best child (puct_best).  A lone visit left over by
// that is dropped.  At most min(N, f) steps.
__device__ __forceinline__ uint32_t pruned_count(uint32_t N, double Q, float P, uint32_t Ns, double k, double c,
                                                 double puct_best) {
    const double x = (k * (double)P) * (double)Ns;
    uint32_t n = N;
    while (n > 0) {
        const double taken1 = (double)(N - n) + 1.0;
        if (!(taken1 * taken1 <= x)) break;
        if (!(puct_value(Q, P, Ns, c, n - 1u) < puct_best)) break;
        n--;
    }
    if (n == 1u && n < N) n = 0u;
    return n;
}

}  // namespace
