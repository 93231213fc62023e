// yk_utility.hip - the score-margin utility as a stand-alone entry point: the rule of yk_utility.h,
// the one the search kernels and the value targets use, applied to states given by the caller - the sibling of
// yk_ended.  Its own translation unit: every other kernel compiles as before.
//
// No atomics, and nothing depends on the order in which workgroups run: one thread per state, each output
// written once.  Equal inputs give equal bits.
#include "yk_api.h"
#include "yk_common.h"
#include "yk_utility.h"

using namespace yk;

namespace {

// u[i] = the utility of states[i] seen from players[i], 0.0 where the state is not terminal (game_ended == 0);
// margin[i] = total_with_bonus(s, 0) - total_with_bonus(s, 1), terminal or not.
__global__ __launch_bounds__(256) void k_score_utility(const yk_state_t* __restrict__ in, const int32_t* __restrict__ players,
                                                       int n, UtilDev ud, double* __restrict__ u, int32_t* __restrict__ margin) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    YkS s;
#pragma unroll
    for (int k = 0; k < 8; k++) s.w[k] = in[i].w[k];
    const int player = players[i];
    const double z = game_ended(s, player);
    u[i] = z != 0.0 ? score_utility(s, player, z, ud) : 0.0;
    if (margin) margin[i] = score_margin(s);
}

}  // namespace

extern "C" int yk_score_utility(const yk_state_t* states, const int32_t* players, int n, double weight, double scale,
                                double* u, int32_t* margin, void* stream) {
    if (n < 0 || !score_knobs_ok(weight, scale)) return YK_ERR_ARG;  // (the setter's checks; a NaN fails them)
    if (n == 0) return YK_OK;
    if (!states || !players || !u) return YK_ERR_ARG;
    hipLaunchKernelGGL(k_score_utility, dim3((unsigned)grid_for(n, 256)), dim3(256), 0, as_stream(stream), states, players, n,
                       UtilDev{1.0 - weight, weight, scale, nullptr}, u, margin);
    YK_LAUNCHED();
    return YK_OK;
}
