// yk_forced.hip - policy target pruning as a stand-alone entry point: the pruning k_move_end
// applies to a self-play root after a forced move, applied to rows given as a CSR.  Its own translation unit:
// every other kernel compiles as before.  The arithmetic is yk_forced.h's, the one the search kernels use.
//
// No atomics on data, and nothing depends on the order in which workgroups run: one wavefront per row, each
// output written once by one lane.  Equal inputs give equal bits.
#include "yk_api.h"
#include "yk_common.h"
#include "yk_forced.h"

using namespace yk;

namespace {

constexpr int ROWS_PER_BLOCK = 4;  // wave-per-row kernel: 4 waves of 64 per block

__device__ __forceinline__ int wave_min_i(int v) {
    v = min(v, xlane<32>(v));
    v = min(v, xlane<16>(v));
    v = min(v, xlane<8>(v));
    v = min(v, xlane<4>(v));
    v = min(v, xlane<2>(v));
    return min(v, xlane<1>(v));
}

// *flag = 1 when indptr[0 .. n] starts below 0 or decreases anywhere (or a row is longer than an int counts)
__global__ __launch_bounds__(256) void k_prune_check(const int64_t* __restrict__ indptr, int64_t n,
                                                     int* __restrict__ flag) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n) return;
    if (indptr[r] < 0 || (r < n && (indptr[r + 1] < indptr[r] || indptr[r + 1] - indptr[r] > INT32_MAX))) *flag = 1;  // (every writer stores the same value)
}

// One wavefront per row; lanes stride the row's edges.  The best child c* - the largest count among the visited
// edges (count > 0), the lowest column among equals (and the first entry, should a column repeat) - keeps its
// count and sets the bound; every other visited edge gets pruned_count; an edge without visits keeps its word.
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void k_policy_prune(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ cols, const int32_t* __restrict__ counts,
    const double* __restrict__ q, const float* __restrict__ p, const int32_t* __restrict__ ns, int64_t n, double k,
    double c, int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= n) return;  // (wave-uniform)
    const int64_t s0 = indptr[r];
    const int len = (int)(indptr[r + 1] - s0);
    const uint32_t Ns = (uint32_t)max(ns[r], 0);
    int bn = 0, bc = 0x7FFFFFFF;
    for (int i = lane; i < len; i += 64) {
        const int cnt = counts[s0 + i], col = cols[s0 + i];
        if (cnt > bn || (cnt == bn && cnt > 0 && col < bc)) {
            bn = cnt;
            bc = col;
        }
    }
    wave_argmax_step(bn, bc);
    if (bn <= 0) {  // no visited edge: nothing to prune
        for (int i = lane; i < len; i += 64) out[s0 + i] = counts[s0 + i];
        return;
    }
    // c*'s entry: the first with (bn, bc)
    int bi = 0x7FFFFFFF;
    for (int i = lane; i < len; i += 64)
        if (counts[s0 + i] == bn && cols[s0 + i] == bc) {
            bi = i;
            break;
        }
    bi = wave_min_i(bi);
    const double pstar = puct_value(q[s0 + bi], p[s0 + bi], Ns, c, (uint32_t)bn);
    for (int i = lane; i < len; i += 64) {
        const int32_t cnt = counts[s0 + i];
        int32_t v = cnt;
        if (cnt > 0 && i != bi) v = (int32_t)pruned_count((uint32_t)cnt, q[s0 + i], p[s0 + i], Ns, k, c, pstar);
        out[s0 + i] = v;
    }
}

}  // namespace

extern "C" {

int yk_policy_prune(const int64_t* indptr, const int32_t* cols, const int32_t* counts, const double* q, const float* p,
                    const int32_t* ns, int64_t n, double k, double cpuct, int32_t* out, void* stream) {
    if (!indptr || !cols || !counts || !q || !p || !ns || !out || n < 0 || !(k >= 0.0) || std::isinf(k))
        return YK_ERR_ARG;  // (a NaN k fails k >= 0)
    if ((const void*)out == cols || (const void*)out == counts || (const void*)out == ns) return YK_ERR_ARG;
    hipStream_t st = as_stream(stream);
    Scratch s(st);  // the flag word
    YK_TRY(s.alloc(sizeof(int)));
    int* flag = s.as<int>();
    YK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_prune_check, dim3((unsigned)grid_for(n + 1, 256)), dim3(256), 0, st, indptr, n, flag);
    YK_LAUNCHED();
    int bad = 0;
    YK_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    YK_HIP(hipStreamSynchronize(st));
    if (bad) return YK_ERR_RANGE;  // before any row is read through it
    if (n > 0) {
        hipLaunchKernelGGL(k_policy_prune, dim3((unsigned)grid_for(n, ROWS_PER_BLOCK)), dim3(64 * ROWS_PER_BLOCK), 0, st,
                           indptr, cols, counts, q, p, ns, n, k, cpuct, out);
        YK_LAUNCHED();
        YK_HIP(hipStreamSynchronize(st));
    }
    return YK_OK;
}

}  // extern "C"
