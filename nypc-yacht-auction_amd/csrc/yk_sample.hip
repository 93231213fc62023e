// yk_sample.hip - weighted minibatch sampling for training: per-example weights out of
// the held-out evaluation's per-row table (recency x policy surprise), their float64 cumulative distribution
// in an order fixed by n alone, and Philox draws located in it.  Its own translation unit: every other kernel
// compiles as before.  -ffp-contract=off: every float64 operation is rounded on its own, in the order of
// include/yacht_hip.h, so tests/sample_ref.py's numpy restatement matches bit for bit.
//
// The cumulative distribution is two-level: L[i], the sequential inclusive sum within the chunk of 256
// elements holding i, and O[c], the sequential sum of the chunks' last L before chunk c; cdf[i] = O[c] + L[i].
// cdf[last of c] is O[c + 1] exactly, so the table is nondecreasing and the chunks' ends - every 256th
// element of cdf itself - are the upper level of a two-level search that equals the flat one.
#include <math.h>

#include <algorithm>

#include "yk_api.h"
#include "yk_common.h"

using namespace yk;

namespace {

constexpr int CHUNK = 256;                         // elements per chunk of the cdf
constexpr int NPART = 256;                         // partial sums of K (section 7e's reduction order)
constexpr int SCAN_CPB = 16;                       // chunks per block of k_scan
constexpr int SCAN_LD = CHUNK + 1;                 // LDS row stride in doubles: lane c's row starts on bank 2 c
constexpr int DRAWS = 4;                           // k_draw: draws a thread locates together, their loads overlapping
constexpr int DRAW_BLOCKS = 256;                   // k_draw: blocks before a thread takes more than one draw (the CUs)
constexpr int DRAW_MAX_BLOCKS = 1024;              // k_draw: the largest grid; past it a thread takes further groups
constexpr int KSUM_FLIGHT = 32;                    // k_sample_ksum: loads in flight per thread
constexpr int COL_S = 5, COL_CE = 6, COL_H = 7;    // yk_net_evaluate's columns: mass, soft CE, target entropy

// ---------------------------------------------------------------- weights
// k[i] = max(0, (c - h) / S): the KL of example i's search policy from the net's, 0 for a row without a
// policy, a NaN row or a negative quotient
__global__ __launch_bounds__(256) void k_sample_kl(const double* __restrict__ rows, int64_t ld, int64_t n,
                                                   double* __restrict__ k) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* r = rows + i * ld;
    const double S = r[COL_S], c = r[COL_CE], h = r[COL_H];
    double out = 0.0;
    if (S > 0.0) {
        const double q = (c - h) / S;
        if (isfinite(q) && q > 0.0) out = q;
    }
    k[i] = out;
}

// *K = the sum of k[0..n) in section 7e's order: partial j = ((0.0 + k[j]) + k[j + 256]) + ..., K = ((0.0 +
// partial 0) + partial 1) + ... + partial 255.  One block of 256 threads (coalesced: thread j reads k[j + 256 g])
__global__ __launch_bounds__(NPART) void k_sample_ksum(const double* __restrict__ k, int64_t n, double* __restrict__ K) {
    __shared__ double part[NPART];
    const int j = threadIdx.x;
    double acc = 0.0;
    int64_t i = j;
    // (32 loads in flight per thread, added in the same ascending order: the one block is bound by the loads'
    // latency - with 8 in flight the kernel took 256 us over 983,040 rows)
    for (; i + (KSUM_FLIGHT - 1) * NPART < n; i += KSUM_FLIGHT * NPART) {
        double t[KSUM_FLIGHT];
#pragma unroll
        for (int u = 0; u < KSUM_FLIGHT; u++) t[u] = k[i + u * NPART];
#pragma unroll
        for (int u = 0; u < KSUM_FLIGHT; u++) acc += t[u];
    }
    for (; i < n; i += NPART) acc += k[i];
    part[j] = acc;
    __syncthreads();
    if (j == 0) {
        double s = 0.0;
        for (int p = 0; p < NPART; p++) s += part[p];
        *K = s;
    }
}

// w[i] = factor * s_i over one segment (w points at its first element, len its length); k == NULL or *K == 0:
// s_i = 1.0, else s_i = (1 - sigma) + sigma * ((n k_i) / K).  In place: k may be w.
__global__ __launch_bounds__(256) void k_sample_weights(const double* k, const double* __restrict__ K, int64_t len,
                                                        double nd, double sigma, double factor, double* w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    double s = 1.0;
    if (k) {
        const double Kv = *K;
        if (Kv != 0.0) {
            const double a = nd * k[i];
            const double b = a / Kv;
            const double c2 = sigma * b;
            s = (1.0 - sigma) + c2;
        }
    }
    w[i] = factor * s;
}

// ---------------------------------------------------------------- cdf
// L[i] within every chunk.  A block takes 16 chunks (32 KB, contiguous): the 256 threads stage them in LDS
// with coalesced loads, lanes 0..15 run one chunk's 256 sequential additions each over LDS rows that start on
// different banks, and the block writes the sums back coalesced.  *flag |= 1 for a weight that is negative or NaN.
__global__ __launch_bounds__(256) void k_sample_scan(const double* __restrict__ w, int64_t n, double* __restrict__ L,
                                                     int* __restrict__ flag) {
    __shared__ double tile[SCAN_CPB * SCAN_LD];
    const int64_t base = (int64_t)blockIdx.x * (SCAN_CPB * CHUNK);
    const int tid = threadIdx.x;
    bool bad = false;
#pragma unroll
    for (int c = 0; c < SCAN_CPB; c++) {
        const int64_t i = base + c * CHUNK + tid;
        if (i < n) {
            const double x = w[i];
            bad |= !(x >= 0.0);
            tile[c * SCAN_LD + tid] = x;
        }
    }
    if (bad) *flag = 1;
    __syncthreads();
    if (tid < SCAN_CPB) {
        const int64_t left = n - (base + (int64_t)tid * CHUNK);
        const int len = left < 0 ? 0 : left > CHUNK ? CHUNK : (int)left;
        double* row = tile + tid * SCAN_LD;
        double acc = 0.0;
        for (int e = 0; e < len; e++) {
            acc += row[e];
            row[e] = acc;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < SCAN_CPB; c++) {
        const int64_t i = base + c * CHUNK + tid;
        if (i < n) L[i] = tile[c * SCAN_LD + tid];
    }
}

// O[0] = 0.0, O[c + 1] = O[c] + L[last of c], sequentially: one block, 256 chunks at a time - the threads put
// the chunks' last sums into LDS (0.0 past the last chunk: adding it changes nothing), thread 0 runs the 256
// additions over 16-byte LDS reads and writes, the threads store the offsets.  The next tile's sums are
// fetched before the additions start and arrive under them.
__global__ __launch_bounds__(256) void k_sample_offsets(const double* __restrict__ L, int64_t n, int64_t nchunks,
                                                        double* __restrict__ O) {
    __shared__ __attribute__((aligned(16))) double last[256];
    __shared__ __attribute__((aligned(16))) double off[256];
    const int tid = threadIdx.x;
    auto fetch = [&](int64_t c) { return c < nchunks ? L[std::min<int64_t>(c * CHUNK + CHUNK - 1, n - 1)] : 0.0; };
    double nxt = fetch(tid);
    double acc = 0.0;  // (thread 0's: the offset of the tile's first chunk)
    for (int64_t c0 = 0; c0 < nchunks; c0 += 256) {
        last[tid] = nxt;
        __syncthreads();
        nxt = fetch(c0 + 256 + tid);
        if (tid == 0) {
#pragma unroll 8
            for (int k = 0; k < 256; k += 2) {
                const double2 v = *reinterpret_cast<const double2*>(&last[k]);
                double2 o;
                o.x = acc;
                acc += v.x;
                o.y = acc;
                acc += v.y;
                *reinterpret_cast<double2*>(&off[k]) = o;
            }
        }
        __syncthreads();
        if (c0 + tid < nchunks) O[c0 + tid] = off[tid];
    }
    if (tid == 0) O[nchunks] = acc;
}

// cdf[i] = O[chunk of i] + L[i], in place
__global__ __launch_bounds__(256) void k_sample_add(double* __restrict__ cdf, int64_t n, const double* __restrict__ O) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) cdf[i] = O[blockIdx.x] + cdf[i];  // (a block is a chunk: CHUNK == 256)
}
static_assert(CHUNK == 256, "k_sample_add: one block per chunk");

// ---------------------------------------------------------------- draw
// DRAWS searches advanced in lock step, so that their loads overlap (one search is a chain of
// floor(log2 nchunks) + 9 dependent loads, 20 at 3840 chunks): out[d] = #{i < n : cdf[i] <= t[d]} (UPPER) or #{i < n : cdf[i] < t[d]}, the flat bound over the
// nondecreasing cdf[0..n) in two levels - the chunk by the chunks' ends (every 256th element of cdf itself:
// the upper levels of every search fall on the same few thousand cache lines), then inside that chunk's
// 2 KB; equal to the flat search because end c is cdf's own element 256 c + 255 (the last chunk's: cdf[n - 1]).
// Each level steps down from a power of two (top: the largest <= nchunks): pos += step where element pos + step - 1 exists and lies before t - the same count as a
// bisection, with a trip count that does not depend on the data, and a result inside 0..n whatever cdf holds.
template <bool UPPER>
__device__ __forceinline__ void locate(const double* __restrict__ cdf, int64_t n, int nchunks, int top,
                                       const double (&t)[DRAWS], int64_t (&out)[DRAWS]) {
    int c[DRAWS];
#pragma unroll
    for (int d = 0; d < DRAWS; d++) c[d] = 0;
    for (int step = top; step > 0; step >>= 1) {
        double x[DRAWS];
        bool in[DRAWS];
#pragma unroll
        for (int d = 0; d < DRAWS; d++) {
            in[d] = c[d] + step <= nchunks;
            const int e = in[d] ? c[d] + step - 1 : 0;
            x[d] = cdf[std::min<int64_t>((int64_t)e * CHUNK + CHUNK - 1, n - 1)];
        }
#pragma unroll
        for (int d = 0; d < DRAWS; d++)
            if (in[d] && (UPPER ? x[d] <= t[d] : x[d] < t[d])) c[d] += step;
    }
    int64_t i0[DRAWS];
    int len[DRAWS], p[DRAWS];
#pragma unroll
    for (int d = 0; d < DRAWS; d++) {
        i0[d] = (int64_t)c[d] * CHUNK;
        len[d] = c[d] >= nchunks ? 0 : (int)std::min<int64_t>(CHUNK, n - i0[d]);
        p[d] = 0;
    }
    // (the chunk's last element is its end, which the first level found not to lie before t: 255 remain)
#pragma unroll
    for (int step = CHUNK / 2; step > 0; step >>= 1) {
        double x[DRAWS];
        bool in[DRAWS];
#pragma unroll
        for (int d = 0; d < DRAWS; d++) {
            in[d] = p[d] + step <= len[d];
            x[d] = cdf[in[d] ? i0[d] + p[d] + step - 1 : 0];
        }
#pragma unroll
        for (int d = 0; d < DRAWS; d++)
            if (in[d] && (UPPER ? x[d] <= t[d] : x[d] < t[d])) p[d] += step;
    }
#pragma unroll
    for (int d = 0; d < DRAWS; d++) out[d] = c[d] >= nchunks ? n : i0[d] + p[d];
}

// idx[r] = the element draw first + r falls on.  A thread takes draws r, r + stride, r + 2 stride, r + 3 stride of
// the grid together (stride = the grid's threads: the stores stay coalesced), then the next four.
__global__ __launch_bounds__(256) void k_sample_draw(const double* __restrict__ cdf, int64_t n, int nchunks, int top,
                                                     uint64_t seed, uint32_t key, uint64_t first, int64_t m,
                                                     int32_t* __restrict__ idx) {
    const double total = cdf[n - 1];
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t r0 = (int64_t)blockIdx.x * 256 + threadIdx.x; r0 < m; r0 += DRAWS * stride) {
        double t[DRAWS];
        int64_t i[DRAWS];
        bool past = false;
#pragma unroll
        for (int d = 0; d < DRAWS; d++) {
            const uint64_t j = first + (uint64_t)(r0 + d * stride);
            const double u = u53(philox_u64(philox4x32_10(seed, (uint32_t)j, (uint32_t)(j >> 32), key, PHILOX_SAMPLE)));
            // (a draw past m searches for -1: every lane's probes then fall on the same elements; not stored)
            t[d] = r0 + d * stride < m ? u * total : -1.0;
        }
        locate<true>(cdf, n, nchunks, top, t, i);
#pragma unroll
        for (int d = 0; d < DRAWS; d++) past |= i[d] >= n;
        if (past) {  // u * total rounded up to the total: the first element that reaches it
            double tt[DRAWS];
            int64_t lo[DRAWS];
#pragma unroll
            for (int d = 0; d < DRAWS; d++) tt[d] = total;
            locate<false>(cdf, n, nchunks, top, tt, lo);
#pragma unroll
            for (int d = 0; d < DRAWS; d++)
                if (i[d] >= n) i[d] = std::min<int64_t>(lo[d], n - 1);  // (n - 1: only a NaN total gets there)
        }
#pragma unroll
        for (int d = 0; d < DRAWS; d++)
            if (r0 + d * stride < m) idx[r0 + d * stride] = (int32_t)i[d];
    }
}

}  // namespace

extern "C" {

int yk_sample_weights(const double* rows, int64_t ld, const int64_t* seg_ptr, const double* seg_factor, int nseg,
                      double surprise, int64_t n, double* w, double* ksum, void* stream) {
    if (!seg_ptr || !seg_factor || !w || !ksum || n <= 0 || n > INT32_MAX || nseg < 1 || nseg > 64 ||
        !(surprise >= 0.0 && surprise <= 1.0) || (!rows && surprise != 0.0) || (rows && ld < 16))
        return YK_ERR_ARG;
    if (seg_ptr[0] != 0 || seg_ptr[nseg] != n) return YK_ERR_ARG;
    for (int s = 0; s < nseg; s++)
        if (seg_ptr[s + 1] < seg_ptr[s] || !(seg_factor[s] >= 0.0) || !std::isfinite(seg_factor[s])) return YK_ERR_ARG;
    hipStream_t st = as_stream(stream);
    Scratch K(st);
    *ksum = 0.0;
    int rc = YK_OK;
    if (rows) {
        YK_TRY(K.alloc(sizeof(double)));
        hipLaunchKernelGGL(k_sample_kl, dim3((unsigned)grid_for(n, 256)), dim3(256), 0, st, rows, ld, n, w);
        rc = launched();
        if (rc == YK_OK) {
            hipLaunchKernelGGL(k_sample_ksum, dim3(1), dim3(NPART), 0, st, w, n, K.as<double>());
            rc = launched();
        }
    }
    const double* kin = rows && surprise != 0.0 ? w : nullptr;
    for (int s = 0; s < nseg && rc == YK_OK; s++) {
        const int64_t a = seg_ptr[s], len = seg_ptr[s + 1] - a;
        if (len == 0) continue;
        hipLaunchKernelGGL(k_sample_weights, dim3((unsigned)grid_for(len, 256)), dim3(256), 0, st,
                           kin ? kin + a : nullptr, K.as<double>(), len, (double)n, surprise, seg_factor[s], w + a);
        rc = launched();
    }
    if (K.p && rc == YK_OK && hipMemcpyAsync(ksum, K.p, sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = YK_ERR_HIP;
    (void)K.release();
    YK_HIP(hipStreamSynchronize(st));
    return rc;
}

int yk_sample_cdf(const double* w, int64_t n, double* cdf, double* total, void* stream) {
    if (!w || !cdf || !total || n <= 0 || n > INT32_MAX) return YK_ERR_ARG;
    hipStream_t st = as_stream(stream);
    const int64_t nchunks = (n + CHUNK - 1) / CHUNK;
    // one allocation: O[nchunks + 1] | the flag word
    Scratch buf(st);
    YK_TRY(buf.alloc(sizeof(double) * (size_t)(nchunks + 2)));
    double* O = buf.as<double>();
    int* flag = reinterpret_cast<int*>(O + nchunks + 1);
    int rc = YK_OK, bad = 0;
    double tot = 0.0;
    if (hipMemsetAsync(flag, 0, sizeof(int), st) != hipSuccess) rc = YK_ERR_HIP;
    if (rc == YK_OK) {
        hipLaunchKernelGGL(k_sample_scan, dim3((unsigned)grid_for(nchunks, SCAN_CPB)), dim3(256), 0, st, w, n, cdf, flag);
        rc = launched();
    }
    if (rc == YK_OK) {
        hipLaunchKernelGGL(k_sample_offsets, dim3(1), dim3(256), 0, st, cdf, n, nchunks, O);
        rc = launched();
    }
    if (rc == YK_OK) {
        hipLaunchKernelGGL(k_sample_add, dim3((unsigned)nchunks), dim3(256), 0, st, cdf, n, O);
        rc = launched();
    }
    if (rc == YK_OK && (hipMemcpyAsync(&tot, cdf + (n - 1), sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess))
        rc = YK_ERR_HIP;
    (void)buf.release();
    YK_HIP(hipStreamSynchronize(st));
    if (rc != YK_OK) return rc;
    *total = tot;
    return (bad || !std::isfinite(tot) || !(tot > 0.0)) ? YK_ERR_RANGE : YK_OK;
}

int yk_sample_draw(const double* cdf, int64_t n, uint64_t seed, uint32_t key, uint64_t first, int64_t m, int32_t* idx,
                   void* stream) {
    if (!cdf || n <= 0 || n > INT32_MAX || m < 0 || (!idx && m > 0)) return YK_ERR_ARG;
    if (m == 0) return YK_OK;
    hipStream_t st = as_stream(stream);
    const int64_t nchunks = (n + CHUNK - 1) / CHUNK;
    int top = 1;
    while (2 * (int64_t)top <= nchunks) top *= 2;  // the largest power of two <= nchunks
    // every probe of a wave is a cache line of its own, and a CU's texture unit takes them one per cycle: the
    // draws are spread over all CUs (at least DRAW_BLOCKS blocks once m fills them) before a thread takes four.
    // m <= 65536: one draw per thread; up to 1,048,576: up to four, in one group; beyond: the loop over groups
    const int64_t want = std::max<int64_t>(grid_for(m, 256 * DRAWS), std::min<int64_t>(grid_for(m, 256), DRAW_BLOCKS));
    const unsigned grid = (unsigned)std::min<int64_t>(want, DRAW_MAX_BLOCKS);
    hipLaunchKernelGGL(k_sample_draw, dim3(grid), dim3(256), 0, st, cdf, n, (int)nchunks, top, seed, key, first, m, idx);
    YK_LAUNCHED();
    return YK_OK;
}

}  // extern "C"
