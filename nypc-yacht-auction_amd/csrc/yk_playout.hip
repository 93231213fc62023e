// yk_playout.hip - the example side of the playout cap: which examples of the record images
// come from full moves (their record's status word lacks YK_REC_FAST), and the rows of a policy CSR gathered
// by such a list.  Its own translation unit: every other kernel compiles as before.  Integer work and copies
// only.
//
// No atomics on data, and nothing depends on the order in which workgroups run.  Offsets come from
// yk_scan.h's three-pass exclusive scan of int64 lengths (scan_rows).
#include "yk_replay_dev.h"  // ImgView, k_example_offsets, prepare: the example numbering of yk_replay.hip

namespace {

constexpr int ROWS_PER_BLOCK = 4;  // wave-per-row kernels: 4 waves of 64 per block

// ---------------------------------------------------------------- full rows
// One wavefront per game, lane m = move m (k_examples' grid).  pos[k] = 1 when example k = off[g] + m is a full
// move's, else 0; k < total by the offsets' construction.
__global__ void __launch_bounds__(64) k_full_flags(ImgView v, const int64_t* __restrict__ off, int64_t total,
                                                   int64_t* __restrict__ pos) {
    const int64_t g = blockIdx.x;
    const int img = (int)(g / v.E), e = (int)(g % v.E);
    const int64_t base = off[g], n = off[g + 1] - off[g];
    const int32_t* info = reinterpret_cast<const int32_t*>(v.part(img, REC_INFO)) + (int64_t)e * v.M * 8;
    for (int m = threadIdx.x; m < n; m += 64) {
        const int64_t k = base + m;
        if (k < total) pos[k] = (info[m * 8 + 6] & YK_REC_FAST) ? 0 : 1;
    }
}

// idx[pos[k]] = k for the full rows (pos scanned: a full row is one whose offset steps); cap entries at most
__global__ __launch_bounds__(256) void k_full_write(const int64_t* __restrict__ pos, int64_t n, int64_t cap,
                                                    int32_t* __restrict__ idx) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t p = pos[k];
    if (pos[k + 1] != p && p < cap) idx[p] = (int32_t)k;
}

// ---------------------------------------------------------------- take
// len[j] = the length of row idx[j]; *flag = 1 when an index lies outside [0, n) (its length is then 0)
__global__ __launch_bounds__(256) void k_take_len(const int64_t* __restrict__ indptr, int64_t n,
                                                  const int32_t* __restrict__ idx, int64_t m, int64_t* __restrict__ len,
                                                  int* __restrict__ flag) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const int32_t r = idx[j];
    if (r < 0 || r >= n) {
        *flag = 1;  // (every writer stores the same value)
        len[j] = 0;
        return;
    }
    const int64_t l = indptr[r + 1] - indptr[r];
    len[j] = l < 0 ? 0 : l;  // (an indptr that decreases is the caller's error; never a negative length)
}

// One wavefront per output row: the row's entries copied, lane by lane
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void k_take_fill(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ cols, const double* __restrict__ vals, int64_t n,
    const int32_t* __restrict__ idx, int64_t m, const int64_t* __restrict__ out_indptr, int32_t* __restrict__ out_cols,
    double* __restrict__ out_vals) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (j >= m) return;  // (wave-uniform)
    const int32_t r = idx[j];
    if (r < 0 || r >= n) return;  // (not reached: the call returns YK_ERR_RANGE before this launch)
    const int64_t s0 = indptr[r];
    const int64_t o0 = out_indptr[j], l = out_indptr[j + 1] - o0;
    for (int64_t k = lane; k < l; k += 64) {
        out_cols[o0 + k] = cols[s0 + k];
        out_vals[o0 + k] = vals[s0 + k];
    }
}

}  // namespace

extern "C" {

int yk_examples_full_rows(const void* images, int n_images, int n_envs, int max_moves, int sims, int64_t n_games,
                          int32_t* idx, int64_t capacity, int64_t* n_full, void* stream) {
    if (!images || n_images <= 0 || n_envs <= 0 || max_moves <= 0 || sims < 0 || !n_full || (idx && capacity < 0))
        return YK_ERR_ARG;
    *n_full = 0;
    hipStream_t s = as_stream(stream);
    Prep p(s);
    YK_TRY(prepare(images, n_images, n_envs, max_moves, sims, n_games, &p));
    YK_HIP(hipStreamSynchronize(s));  // p.total
    const int64_t n = p.total;
    if (n > INT32_MAX) return YK_ERR_ARG;  // the indices are int32
    if (n == 0) return YK_OK;
    const int64_t nb = blocks_of(n);
    Scratch w(s);  // pos[n + 1] | bsum[nb + 1]
    YK_TRY(w.alloc(sizeof(int64_t) * (size_t)(n + 1 + nb + 1)));
    int64_t* pos = w.as<int64_t>();
    int64_t* bsum = pos + n + 1;
    // (every example k < n belongs to one move of one game, so k_full_flags writes all of pos[0 .. n))
    hipLaunchKernelGGL(k_full_flags, dim3((unsigned)p.n_games), dim3(64), 0, s, p.v, p.offsets(), n, pos);
    YK_LAUNCHED();
    YK_TRY(scan_rows(pos, n, bsum, s));
    if (idx && capacity > 0) {
        hipLaunchKernelGGL(k_full_write, dim3((unsigned)grid_for(n, 256)), dim3(256), 0, s, pos, n, capacity, idx);
        YK_LAUNCHED();
    }
    int64_t total = 0;
    YK_HIP(hipMemcpyAsync(&total, pos + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    YK_HIP(hipStreamSynchronize(s));
    *n_full = total;
    return (idx && total > capacity) ? YK_ERR_CAPACITY : YK_OK;
}

int yk_policies_take(const int64_t* indptr, const int32_t* cols, const double* vals, int64_t n, const int32_t* idx,
                     int64_t m, int64_t* out_indptr, int32_t* out_cols, double* out_vals, int64_t nnz_capacity,
                     int64_t* nnz, void* stream) {
    if (!indptr || !out_indptr || !nnz || n < 0 || n > INT32_MAX || m < 0 || m > INT32_MAX || (m > 0 && !idx))
        return YK_ERR_ARG;
    if (out_cols && (!out_vals || nnz_capacity < 0 || !cols || !vals)) return YK_ERR_ARG;
    if (out_indptr == indptr || (out_cols && (out_cols == cols || out_cols == idx || out_vals == vals)))
        return YK_ERR_ARG;
    hipStream_t st = as_stream(stream);
    const int64_t nb = blocks_of(m);
    Scratch s(st);  // bsum[nb + 1] | the flag word
    YK_TRY(s.alloc(sizeof(int64_t) * (size_t)(nb + 2)));
    int64_t* bsum = s.as<int64_t>();
    int* flag = reinterpret_cast<int*>(bsum + nb + 1);
    YK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    if (m > 0) {
        hipLaunchKernelGGL(k_take_len, dim3((unsigned)grid_for(m, 256)), dim3(256), 0, st, indptr, n, idx, m, out_indptr,
                           flag);
        YK_LAUNCHED();
    }
    YK_TRY(scan_rows(out_indptr, m, bsum, st));  // (m == 0: out_indptr[0] = 0)
    int64_t total = 0;
    int bad = 0;
    YK_HIP(hipMemcpyAsync(&total, out_indptr + m, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    YK_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    YK_HIP(hipStreamSynchronize(st));
    *nnz = total;
    if (bad) return YK_ERR_RANGE;
    if (!out_cols) return YK_OK;
    if (total > nnz_capacity) return YK_ERR_CAPACITY;
    if (m > 0 && total > 0) {
        hipLaunchKernelGGL(k_take_fill, dim3((unsigned)grid_for(m, ROWS_PER_BLOCK)), dim3(64 * ROWS_PER_BLOCK), 0, st,
                           indptr, cols, vals, n, idx, m, out_indptr, out_cols, out_vals);
        YK_LAUNCHED();
        YK_HIP(hipStreamSynchronize(st));
    }
    return YK_OK;
}

}  // extern "C"
