// yk_value_targets.hip - value targets from the search: the record images' outcome z
// and per-move root values q (info[..][7], written by k_root_value with record_root_values) -> the float32
// value each example is trained on,
//     G_{T-1} = Z_{T-1} ;  G_t = (1 - lambda) W_{t+1} + lambda G_{t+1} ;  v_t = (1 - beta) p_t G_t + beta q_t
// in float64 without contraction (-ffp-contract=off), rounded to float32 once.  Its own translation unit:
// yk_replay.hip's kernels compile as before.  The examples are numbered by yk_replay_dev.h's offsets, as
// yk_examples_from_records numbers them.
//
// The score-margin utility (yk_examples_utility_targets): the same kernel with a UtilDev optional
// argument (yk_optarg.h), which reads U_t = (1 - w) Z_t + w g1 wherever the formulas read Z_t - g1 the squashed
// final margin for player 1, from the game's final board in the images (REC_FINAL; one value per game).  The
// default instantiation keeps the arguments and the code it had.
#include <math.h>

#include "yk_replay_dev.h"  // (first: the HIP runtime)

#include "yk_optarg.h"
#include "yk_utility.h"

namespace {

// One wavefront per game.  The game's moves are taken 64 at a time from the last chunk down, lane i move
// c0 + i; within a chunk the backward recursion runs from the chunk's last move to its first, every lane
// carrying the same (G_{t+1}, W_{t+1}) in uniform registers and lane i keeping G of its own move - no LDS.
// The whole game is walked even where skip / cap cut it: a kept move's G depends on the moves after it.
// Example k = off[g] + m - skip, kept if 0 <= k < cap (as k_examples).  `missing` counts the kept examples
// whose formula reads a root value that is absent (word 0).
// UD, the optional argument: UtilDev for the utility targets, nothing for the default.
template <class... UD>
__global__ void __launch_bounds__(64) k_value_targets(ImgView v, const int64_t* off, int64_t skip, int64_t cap,
                                                      double beta, double lambda, float* values, float* root_values,
                                                      unsigned long long* missing, UD... ud) {
    static_assert(yk::args_in(yk::Args<UtilDev>{}, yk::Args<UD...>{}), "UtilDev, no further argument");
    constexpr bool UTIL = yk::has_arg<UtilDev, UD...>;
    const int64_t g = blockIdx.x;
    const int lane = threadIdx.x;
    const int img = (int)(g / v.E), e = (int)(g % v.E);
    const int64_t base = off[g] - skip;
    const int n = (int)(off[g + 1] - off[g]);  // <= M
    const int32_t* info = reinterpret_cast<const int32_t*>(v.part(img, REC_INFO)) + (int64_t)e * v.M * 8;
    const double* val = reinterpret_cast<const double*>(v.part(img, REC_VALUES)) + (int64_t)e * v.M;
    const bool td = lambda != 1.0, mix = beta != 0.0;
    const double keep_l = 1.0 - lambda, keep_b = 1.0 - beta;
    double G = 0.0, Wn = 0.0;  // G_{t+1}, W_{t+1} of the move last done (wave-uniform)
    bool absent_later = false;  // a move after t has no root value (wave-uniform)
    unsigned miss = 0;
    [[maybe_unused]] UtilDev ut{1.0, 0.0, 1.0, nullptr};
    [[maybe_unused]] double g1 = 0.0;  // the game's squashed final margin for player 1 (wave-uniform)
    if constexpr (UTIL) {
        ut = yk::get_arg<UtilDev>(ud...);
        const yk_state_t* fin = reinterpret_cast<const yk_state_t*>(v.part(img, REC_FINAL)) + e;
        YkS fs;
#pragma unroll
        for (int k = 0; k < 8; k++) fs.w[k] = fin->w[k];
        g1 = score_squash(1, score_margin(fs), ut.c);
    }
    for (int c0 = n > 0 ? ((n - 1) / 64) * 64 : -1; c0 >= 0; c0 -= 64) {
        const int m = c0 + lane;
        const bool in = m < n;
        const int p_i = in ? info[m * 8 + 1] : 1;
        const uint32_t word = in ? (uint32_t)info[m * 8 + 7] : 0u;
        const double z = in ? val[m] : 0.0;
        const float q32 = word ? __uint_as_float(word) : __uint_as_float(0x7FC00000u);
        const double p = (double)p_i, q = (double)q32;
        const double W = p * q;
        double Z = p * z;
        if constexpr (UTIL) Z = score_blend(Z, g1, ut.keep, ut.w);  // U_t for Z_t, everywhere below
        double Gm = Z;  // lambda == 1: G_t = Z_t
        bool need_later = false;
        if (td) {
            const uint64_t has = __ballot(in && word != 0u);
            for (int i = min(63, n - 1 - c0); i >= 0; i--) {
                const int t = c0 + i;
                const double Wt = lane_val(W, i);
                const double Gt = t == n - 1 ? lane_val(Z, i) : keep_l * Wn + lambda * G;
                if (lane == i) {
                    Gm = Gt;
                    need_later = absent_later;
                }
                G = Gt;
                Wn = Wt;
                absent_later = absent_later || !((has >> i) & 1ull);
            }
        }
        const int64_t k = base + m;
        const bool kept = in && k >= 0 && k < cap;
        if (kept) {
            const double target = p * Gm;
            const double vt = mix ? keep_b * target + beta * q : target;
            values[k] = (float)vt;
            if (root_values) root_values[k] = q32;
        }
        miss += (unsigned)__popcll(__ballot(kept && ((mix && word == 0u) || need_later)));
    }
    if (lane == 0 && miss) atomicAdd(missing, (unsigned long long)miss);
}

}  // namespace

// Both entry points: `util` NULL is the default instantiation
static int value_targets(const void* images, int n_images, int n_envs, int max_moves, int sims, int64_t n_games,
                         int64_t skip, int64_t n_examples, double beta, double lambda, float* values,
                         float* root_values, int64_t* n_missing, const UtilDev* util, void* stream) {
    // (a NaN fails both comparisons)
    if (!(beta >= 0.0 && beta <= 1.0) || !(lambda >= 0.0 && lambda <= 1.0)) return YK_ERR_ARG;
    if (!images || n_images <= 0 || n_envs <= 0 || max_moves <= 0 || sims < 0 || skip < 0 || n_examples < 0 ||
        (!values && n_examples > 0))
        return YK_ERR_ARG;
    hipStream_t s = as_stream(stream);
    Prep p(s);
    YK_TRY(prepare(images, n_images, n_envs, max_moves, sims, n_games, &p));
    YK_HIP(hipStreamSynchronize(s));
    if (n_examples > p.total - skip) return YK_ERR_ARG;  // asks for examples the images do not hold
    Scratch miss(s);
    unsigned long long host_miss = 0;
    if (p.n_games > 0 && n_examples > 0) {
        YK_TRY(miss.alloc(sizeof(host_miss)));
        YK_HIP(hipMemsetAsync(miss.p, 0, sizeof(host_miss), s));
        yk::with_opts([&](const auto&... o) {
            hipLaunchKernelGGL((k_value_targets<std::decay_t<decltype(o)>...>), dim3((unsigned)p.n_games), dim3(64), 0, s,
                               p.v, p.offsets(), skip, n_examples, beta, lambda, values, root_values,
                               miss.as<unsigned long long>(), o...);
        }, yk::opt(util != nullptr, util ? *util : UtilDev{1.0, 0.0, 1.0, nullptr}));
        YK_LAUNCHED();
        YK_HIP(hipMemcpyAsync(&host_miss, miss.p, sizeof(host_miss), hipMemcpyDeviceToHost, s));
        YK_HIP(miss.release());
    }
    YK_HIP(p.off.release());
    YK_HIP(hipStreamSynchronize(s));
    if (n_missing) *n_missing = (int64_t)host_miss;
    return host_miss ? YK_ERR_STATE : YK_OK;
}

extern "C" int yk_examples_value_targets(const void* images, int n_images, int n_envs, int max_moves, int sims,
                                         int64_t n_games, int64_t skip, int64_t n_examples, double beta,
                                         double lambda, float* values, float* root_values, int64_t* n_missing,
                                         void* stream) {
    return value_targets(images, n_images, n_envs, max_moves, sims, n_games, skip, n_examples, beta, lambda, values,
                         root_values, n_missing, nullptr, stream);
}

extern "C" int yk_examples_utility_targets(const void* images, int n_images, int n_envs, int max_moves, int sims,
                                           int64_t n_games, int64_t skip, int64_t n_examples, double beta,
                                           double lambda, double weight, double scale, float* values,
                                           float* root_values, int64_t* n_missing, void* stream) {
    if (!score_knobs_ok(weight, scale)) return YK_ERR_ARG;  // (the setter's checks)
    const UtilDev util{1.0 - weight, weight, scale, nullptr};
    return value_targets(images, n_images, n_envs, max_moves, sims, n_games, skip, n_examples, beta, lambda, values,
                         root_values, n_missing, &util, stream);
}
