// yk_temper.hip - the self-play temperatures as stand-alone entry points: the schedule the host
// builds, the move draw k_move_end makes from N^(1/T) and the root prior transform k_root_noise applies, the
// last two on crafted rows.  Its own translation unit: every other kernel compiles as before.  The arithmetic
// is yk_temper.h's, the one the engine's kernels use.
//
// No atomics on data, and nothing depends on the order in which workgroups run: one wavefront (pick) or one
// workgroup (root) per row, each output written once by one lane.  Equal inputs give equal bits.
#include <math.h>

#include "yk_api.h"
#include "yk_common.h"
#include "yk_temper.h"

using namespace yk;

namespace {

constexpr int ROWS_PER_BLOCK = 4;  // wave-per-row kernel: 4 waves of 64 per block

// *flag = 1 when indptr[0 .. n] starts below 0 or decreases anywhere (or a row is longer than an int counts),
// or when a row's temperature is not a finite number > 0
__global__ __launch_bounds__(256) void k_temper_check(const int64_t* __restrict__ indptr,
                                                      const double* __restrict__ temps, int64_t n,
                                                      int* __restrict__ flag) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n) return;
    bool bad = false;
    if (indptr) bad = indptr[r] < 0 || (r < n && (indptr[r + 1] < indptr[r] || indptr[r + 1] - indptr[r] > INT32_MAX));
    if (r < n) bad = bad || !(temps[r] > 0.0) || isinf(temps[r]);
    if (bad) *flag = 1;  // (every writer stores the same value)
}

// One wavefront per row: wave_temper_pick over the row's counts (a count below 0 is taken as 0) with the row's
// T and u -> the picked entry's index within the row (-1: an empty row, or counts that are all 0) and the total.
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void k_temperature_pick(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ counts, const double* __restrict__ temps,
    const double* __restrict__ u, int64_t n, int32_t* __restrict__ pick, double* __restrict__ total) {
    __shared__ double stage[ROWS_PER_BLOCK][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + w;
    if (r >= n) return;  // (wave-uniform)
    const int64_t s0 = indptr[r];
    const int len = (int)(indptr[r + 1] - s0);
    double tot = 0.0;
    const int p = wave_temper_pick([&](int i) { return max(counts[s0 + i], 0); }, len, 1.0 / temps[r], u[r], stage[w],
                                   lane, &tot);
    if (lane == 0) {
        pick[r] = p;
        total[r] = tot;
    }
}

// One workgroup per row: the engine's transform of a compact prior of V = nvalid[i] entries (clamped to
// 0 .. 3226) under T = temps[i]; columns past V are 0.  T == 1.0 exactly, or weights that do not sum to > 0,
// copy the row.
__global__ __launch_bounds__(TEMPER_THREADS) void k_root_temper_rows(const float* __restrict__ p,
                                                                     const int32_t* __restrict__ nvalid,
                                                                     const double* __restrict__ temps,
                                                                     float* __restrict__ out, int n) {
    __shared__ double tw[ASIZE];
    __shared__ double tsum[4];
    const int i = (int)blockIdx.x;
    if (i >= n) return;
    const int V = min(max(nvalid[i], 0), ASIZE);
    const float* P = p + (long)i * ASIZE;
    float* o = out + (long)i * ASIZE;
    const double T = temps[i];
    bool tempered = false;  // (block-uniform)
    double S = 0.0;
    if (T != 1.0 && V > 0) {
        S = block_temper_weights(P, V, 1.0 / T, tw, tsum, [](int, float) {});
        tempered = S > 0.0;
    }
    for (int j = threadIdx.x; j < ASIZE; j += TEMPER_THREADS)
        o[j] = j < V ? (tempered ? tempered_prior(tw[j], S) : P[j]) : 0.f;
}

// the flag word of k_temper_check, read back: YK_ERR_RANGE when it is set
int check_rows(const int64_t* indptr, const double* temps, int64_t n, hipStream_t st) {
    Scratch s(st);
    YK_TRY(s.alloc(sizeof(int)));
    int* flag = s.as<int>();
    YK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_temper_check, dim3((unsigned)grid_for(n + 1, 256)), dim3(256), 0, st, indptr, temps, n, flag);
    YK_LAUNCHED();
    int bad = 0;
    YK_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    YK_HIP(hipStreamSynchronize(st));
    return bad ? YK_ERR_RANGE : YK_OK;
}

}  // namespace

extern "C" {

int yk_temperature_schedule(double early, double final_t, double halflife, int n_moves, double* out) {
    // (a NaN fails every comparison)
    if (!out || n_moves < 0 || !(early > 0.0) || std::isinf(early) || !(final_t > 0.0) || std::isinf(final_t))
        return YK_ERR_ARG;
    if (!(halflife >= 0.0) || std::isinf(halflife) || (halflife == 0.0 && early != final_t)) return YK_ERR_ARG;
    for (int m = 0; m < n_moves; m++)  // a flat schedule needs no halflife (and divides by none)
        out[m] = early == final_t ? final_t : final_t + (early - final_t) * pow(2.0, (double)(-m) / halflife);
    return YK_OK;
}

int yk_temperature_pick(const int64_t* indptr, const int32_t* counts, const double* temps, const double* u, int64_t n,
                        int32_t* pick, double* total, void* stream) {
    if (!indptr || !counts || !temps || !u || !pick || !total || n < 0) return YK_ERR_ARG;
    if ((const void*)pick == counts || (const void*)total == temps || (const void*)total == u) return YK_ERR_ARG;
    hipStream_t st = as_stream(stream);
    YK_TRY(check_rows(indptr, temps, n, st));  // before any row is read through indptr
    if (n > 0) {
        hipLaunchKernelGGL(k_temperature_pick, dim3((unsigned)grid_for(n, ROWS_PER_BLOCK)), dim3(64 * ROWS_PER_BLOCK), 0,
                           st, indptr, counts, temps, u, n, pick, total);
        YK_LAUNCHED();
        YK_HIP(hipStreamSynchronize(st));
    }
    return YK_OK;
}

int yk_root_temper(const float* p, const int32_t* nvalid, const double* temps, int n, float* out, void* stream) {
    if (!p || !nvalid || !temps || !out || n < 0 || (const void*)out == p) return YK_ERR_ARG;
    hipStream_t st = as_stream(stream);
    YK_TRY(check_rows(nullptr, temps, n, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_root_temper_rows, dim3((unsigned)n), dim3(TEMPER_THREADS), 0, st, p, nvalid, temps, out, n);
        YK_LAUNCHED();
        YK_HIP(hipStreamSynchronize(st));
    }
    return YK_OK;
}

}  // extern "C"
