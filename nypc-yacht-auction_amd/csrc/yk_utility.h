// yk_utility.h - the score-margin utility (KataGo's score utility): the one statement of the rule,
// shared by the search kernels (yk_engine.hip: the terminal branch of select_game), the value targets
// (yk_value_targets.hip) and the stand-alone entry point (yk_utility.hip).  Every operation is one IEEE double
// operation, rounded on its own (the units are built with -ffp-contract=off; division and addition are correctly
// rounded), so numpy float64 gives the same bits.
//
// For a terminal state s (game_ended(s, 1) != 0) seen from `player` (+1 / -1), weight w in [0, 1], scale c > 0:
//   z = game_ended(s, player)                                  (+-1; 1e-4 for a draw, for either player)
//   m = total_with_bonus(s, 0) - total_with_bonus(s, 1)        (int, game points)
//   x = (double)(player * m) / c ;  g = x / (1.0 + fabs(x))    (the rational squash, |g| < 1)
//   u = (1.0 - w) * z + w * g                                  (1.0 - w computed once on the host: `keep`)
// |u| <= 1.  Whether a state is terminal is game_ended != 0, never u != 0 (at w = 1 a draw has u = 0).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "yk_common.h"

namespace {

// The feature's own kernel argument (as FpuDev: EngDev is the same with and without the feature).  Only the
// utility instantiations read it.  `terminals` is the search kernels' counter, [E] (the per-game gstats have no
// free slot, and a wider GST would change the address arithmetic of every instantiation); NULL elsewhere.
struct UtilDev {
    double keep;  // 1.0 - w
    double w;
    double c;     // the scale, in game points: the rule divides by it (no multiplication by 1 / c)
    unsigned long long* terminals;
};

// Whether (w, c) are a legal weight and scale (a NaN fails the comparisons)
__device__ __host__ inline bool score_knobs_ok(double w, double c) { return w >= 0.0 && w <= 1.0 && c > 0.0 && c <= DBL_MAX; }

// m of a state
__device__ __host__ inline int score_margin(const yk::YkS& s) { return yk::total_with_bonus(s, 0) - yk::total_with_bonus(s, 1); }

// g for `player` (+1 / -1) from m
__device__ __host__ inline double score_squash(int player, int m, double c) {
    const double x = (double)(player * m) / c;
    return x / (1.0 + fabs(x));
}

// u from z = game_ended(s, player) (not 0) and g = score_squash(player, m, c)
__device__ __host__ inline double score_blend(double z, double g, double keep, double w) { return keep * z + w * g; }

// u of a terminal state whose z = game_ended(s, player) the caller already holds
__device__ __host__ inline double score_utility(const yk::YkS& s, int player, double z, const UtilDev& u) {
    return score_blend(z, score_squash(player, score_margin(s), u.c), u.keep, u.w);
}

}  // namespace
