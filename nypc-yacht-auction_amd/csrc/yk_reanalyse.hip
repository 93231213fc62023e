// yk_reanalyse.hip - reanalysis of replay-window examples: which examples of the window a
// refresh searches again (a Philox draw per example), the search's dense root visit counts as policy rows of
// a CSR, and those rows spliced into a shard's CSR.  Its own translation unit: every other kernel compiles as
// before.  -ffp-contract=off: the one float64 operation per entry (N / sum) is rounded on its own, so
// tests/reanalyse_ref.py's numpy restatement matches bit for bit.
//
// No atomics on data, and nothing depends on the order in which workgroups run.  Row offsets come from
// yk_scan.h's three-pass exclusive scan of int64 row lengths (scan_rows).
#include <math.h>

#include "yk_api.h"
#include "yk_common.h"
#include "yk_scan.h"

using namespace yk;

namespace {

constexpr int ASIZE_ = YK_ACTION_SIZE;
constexpr int ROWS_PER_BLOCK = 4;  // wave-per-row kernels: 4 waves of 64 per block

// ---------------------------------------------------------------- select
// pos[i] = 1 when row i is chosen (u < fraction), else 0
__global__ __launch_bounds__(256) void k_select_flags(int64_t n, uint64_t index_base, uint64_t seed, uint32_t key,
                                                      double fraction, int64_t* __restrict__ pos) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = index_base + (uint64_t)i;
    const double u = u53(philox_u64(philox4x32_10(seed, (uint32_t)k, (uint32_t)(k >> 32), key, PHILOX_REANALYSE)));
    pos[i] = u < fraction ? 1 : 0;
}

// idx[pos[i]] = i for the chosen rows (pos scanned: a chosen row is one whose offset steps); cap entries at most
__global__ __launch_bounds__(256) void k_select_write(const int64_t* __restrict__ pos, int64_t n, int64_t cap,
                                                      int32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pos[i];
    if (pos[i + 1] != p && p < cap) idx[p] = (int32_t)i;
}

// ---------------------------------------------------------------- from counts
// One wavefront per row.  len[r] = #{a : counts[r][a] > 0}; targets[r] = the lowest action among those with the
// largest count, -1 for a row without one.
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void k_counts_rows(const int32_t* __restrict__ counts, int64_t n,
                                                                    int64_t* __restrict__ len,
                                                                    int32_t* __restrict__ targets) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= n) return;  // (wave-uniform)
    const int32_t* c = counts + r * ASIZE_;
    int cnt = 0, best = 0, arg = -1;
    for (int a = lane; a < ASIZE_; a += 64) {
        const int32_t x = c[a];
        cnt += x > 0;
        if (x > best) {  // (ascending within the lane: the lowest action of the lane's largest count)
            best = x;
            arg = a;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        cnt += __shfl_xor(cnt, d, 64);
        const int ob = __shfl_xor(best, d, 64), oa = __shfl_xor(arg, d, 64);
        if (ob > best || (ob == best && ob > 0 && oa < arg)) {
            best = ob;
            arg = oa;
        }
    }
    if (lane == 0) {
        len[r] = cnt;
        if (targets) targets[r] = arg;
    }
}

// *out = #{r : len[r] == 0}.  One workgroup; an integer sum.
__global__ __launch_bounds__(SCAN_THREADS) void k_count_empty(const int64_t* __restrict__ len, int64_t n,
                                                               int64_t* __restrict__ out) {
    __shared__ int64_t part[SCAN_THREADS];
    const int t = threadIdx.x;
    int64_t s = 0;
    for (int64_t i = t; i < n; i += SCAN_THREADS) s += len[i] == 0;
    part[t] = s;
    __syncthreads();
    for (int d = SCAN_THREADS / 2; d > 0; d >>= 1) {
        if (t < d) part[t] += part[t + d];
        __syncthreads();
    }
    if (t == 0) *out = part[0];
}

// One wavefront per row: the entries (cols ascending, vals = (double)N / sum).  The sum of the positive counts
// is at most 3226 * (2^31 - 1) < 2^43: every partial sum is an integer a float64 holds exactly, so the int64
// sum converted once is the sequential float64 sum in ascending action order, bit for bit.
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void k_counts_fill(const int32_t* __restrict__ counts, int64_t n,
                                                                    const int64_t* __restrict__ indptr,
                                                                    int32_t* __restrict__ cols,
                                                                    double* __restrict__ vals) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= n) return;  // (wave-uniform)
    const int32_t* c = counts + r * ASIZE_;
    const int64_t o0 = indptr[r], o1 = indptr[r + 1];
    if (o1 == o0) return;
    int64_t tot = 0;
    for (int a = lane; a < ASIZE_; a += 64) {
        const int32_t x = c[a];
        if (x > 0) tot += x;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) tot += __shfl_xor(tot, d, 64);
    const double sum = (double)tot;
    int64_t o = o0;
    for (int a0 = 0; a0 < ASIZE_; a0 += 64) {  // (every lane runs every trip: the ballot is over the whole wave)
        const int a = a0 + lane;
        const int32_t x = a < ASIZE_ ? c[a] : 0;
        const unsigned long long mask = __ballot(x > 0);
        if (x > 0) {
            const int64_t p = o + __popcll(mask & ((1ull << lane) - 1ull));
            if (p < o1) {  // (always: the row was counted from the same table)
                cols[p] = a;
                vals[p] = (double)x / sum;
            }
        }
        o += __popcll(mask);
    }
}

// ---------------------------------------------------------------- splice
// *flag = 1 unless idx[0..m) is strictly ascending and within [0, n)
__global__ __launch_bounds__(256) void k_splice_check(const int32_t* __restrict__ idx, int64_t m, int64_t n,
                                                      int* __restrict__ flag) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const int32_t x = idx[j];
    if (x < 0 || x >= n || (j > 0 && idx[j - 1] >= x)) *flag = 1;
}

__global__ __launch_bounds__(256) void k_fill_i32(int32_t* __restrict__ a, int64_t n, int32_t v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = v;
}

// src[idx[j]] = j for the new rows that have entries (an empty new row keeps the old one).  An idx outside
// [0, n) is skipped (k_splice_check reports it); strictly ascending idx never write one element twice.
__global__ __launch_bounds__(256) void k_splice_map(const int32_t* __restrict__ idx, int64_t m, int64_t n,
                                                    const int64_t* __restrict__ nindptr, int32_t* __restrict__ src) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const int32_t x = idx[j];
    if (x < 0 || x >= n) return;
    if (nindptr[j + 1] > nindptr[j]) src[x] = (int32_t)j;
}

// len[i] = the length of the row the output's row i is
__global__ __launch_bounds__(256) void k_splice_len(const int64_t* __restrict__ indptr, const int64_t* __restrict__ nindptr,
                                                    const int32_t* __restrict__ src, int64_t n, int64_t m,
                                                    int64_t* __restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t j = src ? src[i] : -1;
    int64_t l = (j >= 0 && j < m) ? nindptr[j + 1] - nindptr[j] : indptr[i + 1] - indptr[i];
    len[i] = l < 0 ? 0 : l;  // (an indptr that decreases is the caller's error; never a negative length)
}

// One wavefront per row: the row's entries copied, lane by lane
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void k_splice_fill(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ cols, const double* __restrict__ vals,
    const int64_t* __restrict__ nindptr, const int32_t* __restrict__ ncols, const double* __restrict__ nvals,
    const int32_t* __restrict__ src, int64_t n, int64_t m, const int64_t* __restrict__ out_indptr,
    int32_t* __restrict__ out_cols, double* __restrict__ out_vals) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= n) return;
    const int32_t j = src ? src[i] : -1;
    const bool fresh = j >= 0 && j < m;
    const int64_t s0 = fresh ? nindptr[j] : indptr[i];
    const int32_t* sc = fresh ? ncols : cols;
    const double* sv = fresh ? nvals : vals;
    const int64_t o0 = out_indptr[i], l = out_indptr[i + 1] - o0;
    for (int64_t k = lane; k < l; k += 64) {
        out_cols[o0 + k] = sc[s0 + k];
        out_vals[o0 + k] = sv[s0 + k];
    }
}

}  // namespace

extern "C" {

int yk_reanalyse_select(int64_t n, uint64_t index_base, uint64_t seed, uint32_t key, double fraction, int32_t* idx,
                        int64_t capacity, int64_t* m, void* stream) {
    if (!m || n < 0 || n > INT32_MAX || !(fraction >= 0.0 && fraction <= 1.0) || (idx && capacity < 0))
        return YK_ERR_ARG;
    *m = 0;
    if (n == 0) return YK_OK;
    hipStream_t st = as_stream(stream);
    const int64_t nb = blocks_of(n);
    Scratch s(st);  // pos[n + 1] | bsum[nb + 1]
    YK_TRY(s.alloc(sizeof(int64_t) * (size_t)(n + 1 + nb + 1)));
    int64_t* pos = s.as<int64_t>();
    int64_t* bsum = pos + n + 1;
    hipLaunchKernelGGL(k_select_flags, dim3((unsigned)grid_for(n, 256)), dim3(256), 0, st, n, index_base, seed, key,
                       fraction, pos);
    YK_LAUNCHED();
    YK_TRY(scan_rows(pos, n, bsum, st));
    if (idx && capacity > 0) {
        hipLaunchKernelGGL(k_select_write, dim3((unsigned)grid_for(n, 256)), dim3(256), 0, st, pos, n, capacity, idx);
        YK_LAUNCHED();
    }
    int64_t total = 0;
    YK_HIP(hipMemcpyAsync(&total, pos + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    YK_HIP(hipStreamSynchronize(st));
    *m = total;
    return (idx && total > capacity) ? YK_ERR_CAPACITY : YK_OK;
}

int yk_policies_from_counts(const int32_t* counts, int64_t n, int64_t* pi_indptr, int32_t* pi_cols, double* pi_vals,
                            int64_t nnz_capacity, int32_t* targets, int64_t* nnz, int64_t* n_empty, void* stream) {
    if (!pi_indptr || !nnz || n < 0 || n > INT32_MAX || (n > 0 && !counts) || (pi_cols && (!pi_vals || nnz_capacity < 0)))
        return YK_ERR_ARG;
    hipStream_t st = as_stream(stream);
    const int64_t nb = blocks_of(n);
    Scratch s(st);  // bsum[nb + 1] | the empty rows' count
    YK_TRY(s.alloc(sizeof(int64_t) * (size_t)(nb + 2)));
    int64_t* bsum = s.as<int64_t>();
    int64_t* dempty = bsum + nb + 1;
    if (n > 0) {
        hipLaunchKernelGGL(k_counts_rows, dim3((unsigned)grid_for(n, ROWS_PER_BLOCK)), dim3(64 * ROWS_PER_BLOCK), 0, st,
                           counts, n, pi_indptr, targets);
        YK_LAUNCHED();
    }
    hipLaunchKernelGGL(k_count_empty, dim3(1), dim3(SCAN_THREADS), 0, st, pi_indptr, n, dempty);
    YK_LAUNCHED();
    YK_TRY(scan_rows(pi_indptr, n, bsum, st));
    int64_t total = 0, empty = 0;
    YK_HIP(hipMemcpyAsync(&total, pi_indptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    YK_HIP(hipMemcpyAsync(&empty, dempty, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    YK_HIP(hipStreamSynchronize(st));
    *nnz = total;
    if (n_empty) *n_empty = empty;
    if (!pi_cols) return YK_OK;
    if (total > nnz_capacity) return YK_ERR_CAPACITY;
    if (n > 0 && total > 0) {
        hipLaunchKernelGGL(k_counts_fill, dim3((unsigned)grid_for(n, ROWS_PER_BLOCK)), dim3(64 * ROWS_PER_BLOCK), 0, st,
                           counts, n, pi_indptr, pi_cols, pi_vals);
        YK_LAUNCHED();
        YK_HIP(hipStreamSynchronize(st));
    }
    return YK_OK;
}

int yk_policies_splice(const int64_t* indptr, const int32_t* cols, const double* vals, int64_t n, const int32_t* idx,
                       int64_t m, const int64_t* new_indptr, const int32_t* new_cols, const double* new_vals,
                       int64_t* out_indptr, int32_t* out_cols, double* out_vals, int64_t nnz_capacity, int64_t* nnz,
                       void* stream) {
    if (!indptr || !out_indptr || !nnz || n < 0 || n > INT32_MAX || m < 0 || m > INT32_MAX || (m > 0 && (!idx || !new_indptr)))
        return YK_ERR_ARG;
    if (out_cols && (!out_vals || nnz_capacity < 0 || !cols || !vals || (m > 0 && (!new_cols || !new_vals))))
        return YK_ERR_ARG;
    if (out_indptr == indptr || out_indptr == new_indptr ||
        (out_cols && (out_cols == cols || out_cols == new_cols || out_vals == vals || out_vals == new_vals)))
        return YK_ERR_ARG;
    hipStream_t st = as_stream(stream);
    const int64_t nb = blocks_of(n);
    Scratch s(st);  // bsum[nb + 1] | src[n] | the flag word
    YK_TRY(s.alloc(sizeof(int64_t) * (size_t)(nb + 1) + sizeof(int32_t) * (size_t)(n + 1)));
    int64_t* bsum = s.as<int64_t>();
    int32_t* src = reinterpret_cast<int32_t*>(bsum + nb + 1);
    int* flag = reinterpret_cast<int*>(src + n);
    YK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    if (m > 0) {
        hipLaunchKernelGGL(k_splice_check, dim3((unsigned)grid_for(m, 256)), dim3(256), 0, st, idx, m, n, flag);
        YK_LAUNCHED();
        hipLaunchKernelGGL(k_fill_i32, dim3((unsigned)grid_for(n, 256)), dim3(256), 0, st, src, n, -1);
        YK_LAUNCHED();
        hipLaunchKernelGGL(k_splice_map, dim3((unsigned)grid_for(m, 256)), dim3(256), 0, st, idx, m, n, new_indptr, src);
        YK_LAUNCHED();
    } else {
        src = nullptr;
    }
    if (n > 0) {
        hipLaunchKernelGGL(k_splice_len, dim3((unsigned)grid_for(n, 256)), dim3(256), 0, st, indptr, new_indptr, src, n, m,
                           out_indptr);
        YK_LAUNCHED();
    }
    YK_TRY(scan_rows(out_indptr, n, bsum, st));
    int64_t total = 0;
    int bad = 0;
    YK_HIP(hipMemcpyAsync(&total, out_indptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    YK_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    YK_HIP(hipStreamSynchronize(st));
    *nnz = total;
    if (bad) return YK_ERR_RANGE;
    if (!out_cols) return YK_OK;
    if (total > nnz_capacity) return YK_ERR_CAPACITY;
    if (n > 0 && total > 0) {
        hipLaunchKernelGGL(k_splice_fill, dim3((unsigned)grid_for(n, ROWS_PER_BLOCK)), dim3(64 * ROWS_PER_BLOCK), 0, st,
                           indptr, cols, vals, new_indptr, new_cols, new_vals, src, n, m, out_indptr, out_cols, out_vals);
        YK_LAUNCHED();
        YK_HIP(hipStreamSynchronize(st));
    }
    return YK_OK;
}

}  // extern "C"
