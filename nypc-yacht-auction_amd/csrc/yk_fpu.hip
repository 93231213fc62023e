// yk_fpu.hip - the first-play-urgency pick as a stand-alone entry point: the UCB pick of the
// search kernels' FPU instantiations, applied to nodes given as a CSR.  Its own translation unit: every other
// kernel compiles as before.  The arithmetic is yk_fpu.h's, the one the search kernels use, and the scan has
// the full scan's shape (four adjacent entries per lane, 256 per pass, strict '>' in ascending order, then the
// wave's argmax), so hand-made ties - which games do not reach - meet the same comparisons.
//
// No atomics on data, and nothing depends on the order in which workgroups run: one wavefront per row, each
// output written once by one lane.  Equal inputs give equal bits.
#include "yk_api.h"
#include "yk_common.h"
#include "yk_fpu.h"

using namespace yk;

namespace {

constexpr int ROWS_PER_BLOCK = 4;  // wave-per-row kernel: 4 waves of 64 per block

// *flag = 1 when indptr[0 .. n] starts below 0 or decreases anywhere (or a row is longer than an int counts)
__global__ __launch_bounds__(256) void k_fpu_check(const int64_t* __restrict__ indptr, int64_t n, int* __restrict__ flag) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n) return;
    if (indptr[r] < 0 || (r < n && (indptr[r + 1] < indptr[r] || indptr[r + 1] - indptr[r] > INT32_MAX))) *flag = 1;  // (every writer stores the same value)
}

// One wavefront per row.  An entry with N > 0 is a visited edge (u = f32(Q) + ((c32 P) sq) / f32(1 + N)), any
// other an unvisited one (x = (c32 P) sqe).  With Ns > 0 and both kinds in the row the winner is yk_fpu.h's;
// otherwise - a row at Ns = 0, all visited, none visited - it is the plain argmax over u and x, the lowest
// index among equals.  pick: the entry's index within its row (-1: an empty row); unv: 1 when it is unvisited.
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void k_fpu_pick(
    const int64_t* __restrict__ indptr, const float* __restrict__ p, const int32_t* __restrict__ cnt,
    const double* __restrict__ q, const int32_t* __restrict__ ns, int64_t n, float c32, double r,
    int32_t* __restrict__ pick, int32_t* __restrict__ unv_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= n) return;  // (wave-uniform)
    const int64_t s0 = indptr[row];
    const int len = (int)(indptr[row + 1] - s0);
    const uint32_t Ns = (uint32_t)max(ns[row], 0);
    const float sq = (float)sqrt((double)Ns), sqe = (float)sqrt((double)Ns + 1e-8);
    float best = -INFINITY, bestx = -INFINITY;
    int bj = 0x7FFFFFFF, bjx = 0x7FFFFFFF;
    int64_t fw = 0;
    uint64_t fm = 0;
    for (int j0 = lane * 4; j0 < len; j0 += 256)
        for (int t = 0; t < 4; t++) {
            const int j = j0 + t;
            if (j >= len) break;
            const float pj = p[s0 + j];
            const int32_t N = cnt[s0 + j];
            const float cp = c32 * pj;
            if (N > 0) {
                const double Q = q[s0 + j];
                const float u = (float)Q + (cp * sq) / (float)((uint32_t)N + 1u);
                fw += fpu_w_term((uint32_t)N, Q);
                fm += fpu_m_term(pj);
                if (u > best) {
                    best = u;
                    bj = j;
                }
            } else {
                const float x = cp * sqe;
                if (x > bestx) {
                    bestx = x;
                    bjx = j;
                }
            }
        }
    wave_argmax_step(best, bj);
    wave_argmax_step(bestx, bjx);
    const bool vis = bj != 0x7FFFFFFF, unv = bjx != 0x7FFFFFFF;
    bool unv_won;
    if (vis && unv && Ns > 0) {
        const float fq = fpu_value((int64_t)fpu_wave_sum((uint64_t)fw), fpu_wave_sum(fm), Ns, r);
        unv_won = fpu_unvisited_wins(fq, bestx, bjx, best, bj);
    } else {
        unv_won = unv && (!vis || bestx > best || (bestx == best && bjx < bj));
    }
    if (lane == 0) {
        pick[row] = len == 0 ? -1 : (unv_won ? bjx : bj);
        unv_out[row] = unv_won ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int yk_fpu_pick(const int64_t* indptr, const float* p, const int32_t* counts, const double* q, const int32_t* ns,
                int64_t n, double cpuct, double reduction, int32_t* pick, int32_t* unvisited, void* stream) {
    if (!indptr || !p || !counts || !q || !ns || !pick || !unvisited || n < 0 || !(reduction >= 0.0) ||
        std::isinf(reduction) || !std::isfinite(cpuct))
        return YK_ERR_ARG;  // (a NaN reduction fails >= 0)
    if ((const void*)pick == counts || (const void*)pick == ns || (const void*)unvisited == counts ||
        (const void*)unvisited == ns || pick == unvisited)
        return YK_ERR_ARG;
    hipStream_t st = as_stream(stream);
    Scratch s(st);  // the flag word
    YK_TRY(s.alloc(sizeof(int)));
    int* flag = s.as<int>();
    YK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_fpu_check, dim3((unsigned)grid_for(n + 1, 256)), dim3(256), 0, st, indptr, n, flag);
    YK_LAUNCHED();
    int bad = 0;
    YK_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    YK_HIP(hipStreamSynchronize(st));
    if (bad) return YK_ERR_RANGE;  // before any row is read through it
    if (n > 0) {
        hipLaunchKernelGGL(k_fpu_pick, dim3((unsigned)grid_for(n, ROWS_PER_BLOCK)), dim3(64 * ROWS_PER_BLOCK), 0, st, indptr, p,
                           counts, q, ns, n, (float)cpuct, reduction, pick, unvisited);
        YK_LAUNCHED();
        YK_HIP(hipStreamSynchronize(st));
    }
    return YK_OK;
}

}  // extern "C"
