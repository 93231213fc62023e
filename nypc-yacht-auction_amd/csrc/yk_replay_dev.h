// yk_replay_dev.h - what every reader of the packed trajectory record images shares: the device view of
// the stacked images and the per-game example offsets, which number the examples in (image, game, move)
// order.  Used by yk_replay.hip (examples and policies) and yk_value_targets.hip (value targets), so both
// number the examples alike.  Internal linkage: each unit compiles its own copy.
#pragma once
#include "yk_api.h"
#include "yk_common.h"

using namespace yk;

namespace {

constexpr int SCAN_THREADS = 1024;

struct ImgView {
    const char* base;
    int64_t stride;  // bytes per image
    RecordLayout L;
    int E, M, VCAP;
    __device__ const char* part(int img, int p) const { return base + (int64_t)img * stride + L.off[p]; }
};

// Exclusive prefix of per-game move counts over the first n_games games (image-major order).
// One workgroup: each thread sums a contiguous chunk, then a workgroup scan of the chunk sums.
__global__ void __launch_bounds__(SCAN_THREADS) k_example_offsets(ImgView v, int64_t n_games, int64_t* off) {
    __shared__ int64_t part[SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t chunk = (n_games + SCAN_THREADS - 1) / SCAN_THREADS;
    const int64_t g0 = min<int64_t>((int64_t)t * chunk, n_games), g1 = min<int64_t>(g0 + chunk, n_games);
    int64_t s = 0;
    for (int64_t g = g0; g < g1; g++) {
        const int img = (int)(g / v.E), e = (int)(g % v.E);
        const int nm = reinterpret_cast<const int32_t*>(v.part(img, REC_NMOVES))[e];
        s += nm < 0 ? 0 : (nm > v.M ? v.M : nm);
    }
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {  // Hillis-Steele inclusive scan
        const int64_t x = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    int64_t run = part[t] - s;  // exclusive start of this chunk
    for (int64_t g = g0; g < g1; g++) {
        off[g] = run;
        const int img = (int)(g / v.E), e = (int)(g % v.E);
        const int nm = reinterpret_cast<const int32_t*>(v.part(img, REC_NMOVES))[e];
        run += nm < 0 ? 0 : (nm > v.M ? v.M : nm);
    }
    if (t == SCAN_THREADS - 1) off[n_games] = part[t];
}

struct Prep {
    ImgView v;
    int64_t n_games, total;
    int64_t* off;  // device [n_games + 1], freed by the caller (hipFreeAsync)
};

// The view of the images and the per-game example offsets (HOST total = all examples, valid once the
// stream is synchronised).
int prepare(const void* images, int n_images, int n_envs, int max_moves, int sims, int64_t n_games, hipStream_t s,
            Prep* p) {
    const int64_t all = (int64_t)n_images * n_envs;
    p->n_games = (n_games < 0 || n_games > all) ? all : n_games;
    p->v.base = static_cast<const char*>(images);
    p->v.E = n_envs;
    p->v.M = max_moves;
    p->v.VCAP = (int)record_vcap(max_moves, sims);
    p->v.L = record_layout(n_envs, max_moves, p->v.VCAP);
    p->v.stride = p->v.L.total;
    p->off = nullptr;
    YK_HIP(hipMallocAsync(reinterpret_cast<void**>(&p->off), sizeof(int64_t) * (size_t)(p->n_games + 1), s));
    hipLaunchKernelGGL(k_example_offsets, dim3(1), dim3(SCAN_THREADS), 0, s, p->v, p->n_games, p->off);
    YK_LAUNCHED();
    p->total = 0;
    YK_HIP(hipMemcpyAsync(&p->total, p->off + p->n_games, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    return YK_OK;
}

}  // namespace
