// yk_replay_dev.h - what every reader of the packed trajectory record images shares: the device view of
// the stacked images and the per-game example offsets, which number the examples in (image, game, move)
// order.  Used by yk_replay.hip (examples and policies) and yk_value_targets.hip (value targets), so both
// number the examples alike.  Internal linkage: each unit compiles its own copy.
#pragma once
#include "yk_api.h"
#include "yk_common.h"
#include "yk_scan.h"

using namespace yk;

namespace {

struct ImgView {
    const char* base;
    int64_t stride;  // bytes per image
    RecordLayout L;
    int E, M, VCAP;
    __device__ const char* part(int img, int p) const { return base + (int64_t)img * stride + L.off[p]; }
};

// Exclusive prefix of per-game move counts (clamped to 0..M) over the first n_games games (image-major order).
__global__ void __launch_bounds__(SCAN_THREADS) k_example_offsets(ImgView v, int64_t n_games, int64_t* off) {
    block_scan(
        n_games,
        [&v](int64_t g) -> int64_t {
            const int img = (int)(g / v.E), e = (int)(g % v.E);
            const int nm = reinterpret_cast<const int32_t*>(v.part(img, REC_NMOVES))[e];
            return nm < 0 ? 0 : (nm > v.M ? v.M : nm);
        },
        off);
}

struct Prep {
    ImgView v;
    int64_t n_games, total;
    Scratch off;  // device int64[n_games + 1]
    explicit Prep(hipStream_t s) : off(s) {}
    const int64_t* offsets() const { return off.as<int64_t>(); }
};

// The view of the images and the per-game example offsets (HOST total = all examples, valid once the
// stream is synchronised).
int prepare(const void* images, int n_images, int n_envs, int max_moves, int sims, int64_t n_games, Prep* p) {
    const int64_t all = (int64_t)n_images * n_envs;
    p->n_games = (n_games < 0 || n_games > all) ? all : n_games;
    p->v.base = static_cast<const char*>(images);
    p->v.E = n_envs;
    p->v.M = max_moves;
    p->v.VCAP = (int)record_vcap(max_moves, sims);
    p->v.L = record_layout(n_envs, max_moves, p->v.VCAP);
    p->v.stride = p->v.L.total;
    YK_TRY(p->off.alloc(sizeof(int64_t) * (size_t)(p->n_games + 1)));
    hipLaunchKernelGGL(k_example_offsets, dim3(1), dim3(SCAN_THREADS), 0, p->off.st, p->v, p->n_games,
                       p->off.as<int64_t>());
    YK_LAUNCHED();
    p->total = 0;
    YK_HIP(hipMemcpyAsync(&p->total, p->offsets() + p->n_games, sizeof(int64_t), hipMemcpyDeviceToHost, p->off.st));
    return YK_OK;
}

}  // namespace
