// yk_scan.h - the exclusive scans of int64 lengths into offsets that the replay and reanalysis units share.
// Integer sums: the order cannot change a bit.  No atomics, and nothing depends on the order in which
// workgroups run.  Internal linkage: each unit compiles its own copy.
//
// block_scan:  one workgroup of 1024 threads over any n - each thread sums a contiguous chunk, a workgroup
//              scan of the chunk sums, then the chunk again.
// scan_rows:   three passes for long arrays - every block of 256 rows scans its own rows and leaves its
//              total (k_rows_scan), one workgroup scans the blocks' totals (k_scan_inplace), and every block
//              adds its offset (k_rows_add).
#pragma once
#include "yk_api.h"

namespace {

constexpr int SCAN_THREADS = 1024;  // the one workgroup of block_scan
constexpr int SCAN_ROWS = 256;      // rows per block of scan_rows' first and third pass

// out[i] = load(0) + .. + load(i - 1) for i in 0..n, so out[n] = the total.  Called by all SCAN_THREADS
// threads of a workgroup.  load(i) is read before out[i] is written: out may be the array load reads.
template <class Load>
__device__ __forceinline__ void block_scan(int64_t n, Load load, int64_t* out) {
    __shared__ int64_t part[SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t chunk = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const int64_t i0 = min<int64_t>((int64_t)t * chunk, n), i1 = min<int64_t>(i0 + chunk, n);
    int64_t s = 0;
    for (int64_t i = i0; i < i1; i++) s += load(i);
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {  // Hillis-Steele inclusive scan
        const int64_t x = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    int64_t run = part[t] - s;  // exclusive start of this chunk
    for (int64_t i = i0; i < i1; i++) {
        const int64_t x = load(i);
        out[i] = run;
        run += x;
    }
    if (t == SCAN_THREADS - 1) out[n] = part[t];
}

// In-place exclusive scan of a[0..n) into a[0..n], a[n] = the total.  One workgroup.
__global__ void __launch_bounds__(SCAN_THREADS) k_scan_inplace(int64_t* a, int64_t n) {
    block_scan(n, [a](int64_t i) { return a[i]; }, a);
}

// Pass 1: block b's rows a[256 b ..] become their exclusive prefix within the block; bsum[b] = their total.
__global__ __launch_bounds__(SCAN_ROWS) void k_rows_scan(int64_t* __restrict__ a, int64_t n, int64_t* __restrict__ bsum) {
    __shared__ int64_t part[SCAN_ROWS];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * SCAN_ROWS + t;
    const int64_t x = i < n ? a[i] : 0;
    part[t] = x;
    __syncthreads();
    for (int d = 1; d < SCAN_ROWS; d <<= 1) {  // Hillis-Steele inclusive scan
        const int64_t y = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += y;
        __syncthreads();
    }
    if (i < n) a[i] = part[t] - x;
    if (t == SCAN_ROWS - 1) bsum[blockIdx.x] = part[t];
}

// Pass 3: a[i] += the offset of i's block; a[n] = the total.
__global__ __launch_bounds__(SCAN_ROWS) void k_rows_add(int64_t* __restrict__ a, int64_t n, const int64_t* __restrict__ bsum,
                                                        int64_t nb) {
    const int64_t i = (int64_t)blockIdx.x * SCAN_ROWS + threadIdx.x;
    if (i < n) a[i] += bsum[blockIdx.x];
    if (i == n) a[n] = bsum[nb];  // (the grid covers n + 1 elements)
}

// a[0..n) row lengths -> a[0..n] exclusive offsets, a[n] the total; bsum: DEVICE int64[blocks_of(n) + 1]
inline int64_t blocks_of(int64_t n) { return (n + SCAN_ROWS - 1) / SCAN_ROWS; }
int scan_rows(int64_t* a, int64_t n, int64_t* bsum, hipStream_t st) {
    const int64_t nb = blocks_of(n);
    if (nb > 0) {
        hipLaunchKernelGGL(k_rows_scan, dim3((unsigned)nb), dim3(SCAN_ROWS), 0, st, a, n, bsum);
        YK_LAUNCHED();
    }
    hipLaunchKernelGGL(k_scan_inplace, dim3(1), dim3(SCAN_THREADS), 0, st, bsum, nb);
    YK_LAUNCHED();
    hipLaunchKernelGGL(k_rows_add, dim3((unsigned)blocks_of(n + 1)), dim3(SCAN_ROWS), 0, st, a, n, bsum, nb);
    YK_LAUNCHED();
    return YK_OK;
}

}  // namespace
