// yk_eval.hip - held-out evaluation of a net on examples: a forward without dropout
// (yk::launch_forward, the predict's own) and, over its raw logits, 16 float64 numbers per example -
// log-sum-exp, hard and soft cross-entropy, the target's rank, the policy's entropy and its mass on the
// legal moves, the value error - then their column sums in an order that depends on n alone.  Its own
// translation unit: every other kernel compiles as before.  -ffp-contract=off: every float64 operation is
// rounded on its own.
//
// The columns of rows[i] (x the row's 3226 logits, t / z / (c_k, p_k) the example's target, value and CSR
// policy row, v the net's value; all arithmetic float64, x, v and z widened from f32):
//    0 lse = m + log(s), m = max x, e_a = exp(x_a - m), s = sum e_a
//    1 lse - x_t                               (0 when t is outside 0..3225)
//    2 #{a : x_a > x_t or (x_a == x_t and a < t)}   (3226 when t is outside)
//    3 lse - (sum e_a x_a) / s                 the policy's entropy
//    4 (sum over the valid actions of player 1 of e_a) / s
//    5 S = sum p_k                             6 sum p_k (lse - x[c_k]) over 0 <= c_k < 3226
//    7 -sum over p_k > 0 of p_k log p_k        (5-7: 0 without a CSR)
//    8 v    9 d = v - z    10 d d    11 v z > 0    12 col 2 == 0    13 col 2 < 5    14 t outside    15 1.0
//
// The column sums (k_eval_reduce, k_eval_sums; no atomics): partial j (0..255) of column c is the
// sequential sum, from 0.0, of rows j, j + 256, j + 512, ... in ascending order; sums[c] is the sequential
// sum, from 0.0, of partials 0..255 in ascending j.  Neither the grid, the chunk size nor timing enters.
#include <math.h>

#include <algorithm>

#include "yk_api.h"
#include "yk_common.h"
#include "yk_legal.h"
#include "yk_net.h"

using namespace yk;

namespace {

constexpr int NCOL = 16;          // = YK_EVAL_COLS
constexpr int NPART = 256;        // partial sums per column
constexpr int PER_LANE = 51;      // ceil(3226 / 64) logits per lane
constexpr int TAIL_LANES = ASIZE - 64 * (PER_LANE - 1);  // lanes holding a 51st logit (26)
static_assert(NCOL == YK_EVAL_COLS, "rows[n][16]");

// x[c] of the row for each lane's own column c (0 <= c < 3226, or negative: 0.f), out of the registers that
// hold the row: for every register index k some lane asks for, one ds_bpermute (the LDS crossbar; no LDS is
// allocated) brings lane c & 63's x[k] - a static register index, so the row never leaves the registers
__device__ __forceinline__ float row_gather(const float (&x)[PER_LANE], int c) {
    const int kc = c >> 6;  // (negative for a negative c: matches no k)
    float out = 0.f;
#pragma unroll
    for (int k = 0; k < PER_LANE; k++)
        if (__ballot(kc == k)) {  // wave-uniform
            const float g = __shfl(x[k], c & 63, 64);
            if (kc == k) out = g;
        }
    return out;
}

// One wavefront per example row, four rows per block.  Lane l keeps logits l, l + 64, ... (51 registers),
// read once; the target's and the CSR columns' logits are taken out of those registers (row_gather).
// MASK (yk_examples_metrics_legal / yk_net_evaluate_legal): the same columns over x', the
// logits with -inf at the actions action_valid refuses - the predicate of column 4, which is then 1; the rank
// counts valid actions only, and the entropy skips the terms with e_a = 0 (never 0 * -inf).  The additions
// run in the same order, so the unmasked instantiation is the code it was.
template <bool MASK>
__global__ __launch_bounds__(256) void k_eval_rows(const float* __restrict__ logits, int64_t ld,
                                                   const float* __restrict__ v, const yk_state_t* __restrict__ states,
                                                   const int32_t* __restrict__ targets,
                                                   const float* __restrict__ values,
                                                   const int64_t* __restrict__ indptr,
                                                   const int32_t* __restrict__ cols, const double* __restrict__ vals,
                                                   const int32_t* __restrict__ batch_idx, int64_t ex0, int n,
                                                   double* __restrict__ rows) {
    // (readfirstlane: the row is the wave's, so the example's index, board, target and CSR bounds are scalar
    // loads and the board's decoding in action_valid is scalar work, done once per row)
    const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const int64_t r = batch_idx ? (int64_t)batch_idx[row] : ex0 + row;
    const float* xp = logits + (int64_t)row * ld;
    float x[PER_LANE];
#pragma unroll
    for (int k = 0; k < PER_LANE - 1; k++) x[k] = xp[lane + 64 * k];
    const bool tail = lane < TAIL_LANES;
    x[PER_LANE - 1] = tail ? xp[lane + 64 * (PER_LANE - 1)] : -INFINITY;  // (never enters a result)
    YkS s;
#pragma unroll
    for (int k = 0; k < 8; k++) s.w[k] = states[r].w[k];
    if constexpr (MASK) {
#pragma unroll
        for (int k = 0; k < PER_LANE; k++)
            if (!action_valid(s, 1, lane + 64 * k)) x[k] = -INFINITY;  // (past 3225 x is -inf already)
    }
    const int t = targets[r];
    const bool t_in = t >= 0 && t < ASIZE;
    // the CSR row's bounds and its first 64 entries are asked for now: they arrive under the exp pass
    int64_t a0 = 0, a1 = 0;
    int c_first = -1;
    double p_first = 0.0;
    if (indptr) {
        a0 = indptr[r];
        a1 = indptr[r + 1];
        if (a0 + lane < a1) {
            c_first = cols[a0 + lane];
            p_first = vals[a0 + lane];
        }
    }

    float mf = -INFINITY;
#pragma unroll
    for (int k = 0; k < PER_LANE; k++) mf = fmaxf(mf, x[k]);  // (the 51st is -inf off the tail)
    mf = fmaxf(mf, xlane<32>(mf));
    mf = fmaxf(mf, xlane<16>(mf));
    mf = fmaxf(mf, xlane<8>(mf));
    mf = fmaxf(mf, xlane<4>(mf));
    mf = fmaxf(mf, xlane<2>(mf));
    mf = fmaxf(mf, xlane<1>(mf));
    const double m = (double)mf;
    const float xt = row_gather(x, t_in ? t : -1);

    double se = 0.0, sex = 0.0, sv = 0.0;
    int above = 0;
#pragma unroll
    for (int k = 0; k < PER_LANE; k++) {
        const int a = lane + 64 * k;
        if (k < PER_LANE - 1 || tail) {
            const double xa = (double)x[k];
            const double e = exp(xa - m);
            se += e;
            if constexpr (MASK) {
                const bool ok = action_valid(s, 1, a);
                if (e > 0.0) sex += e * xa;
                if (ok) sv += e;
                above += (ok && (x[k] > xt || (x[k] == xt && a < t))) ? 1 : 0;
            } else {
                sex += e * xa;
                if (action_valid(s, 1, a)) sv += e;
                above += (x[k] > xt || (x[k] == xt && a < t)) ? 1 : 0;
            }
        }
    }
    se = xlane_sum(se);
    sex = xlane_sum(sex);
    sv = xlane_sum(sv);
    above = xlane_sum(above);
    const double lse = m + log(se);
    const int rank = t_in ? above : ASIZE;

    double S = 0.0, soft = 0.0, tent = 0.0;
    if (indptr) {
        for (int64_t k0 = a0; k0 < a1; k0 += 64) {
            const bool in = k0 + lane < a1;
            const int c = k0 == a0 ? c_first : in ? cols[k0 + lane] : -1;
            const double p = k0 == a0 ? p_first : in ? vals[k0 + lane] : 0.0;
            const float xc = row_gather(x, c < ASIZE ? c : -1);
            if (in) {
                S += p;
                if (c >= 0 && c < ASIZE) soft += p * (lse - (double)xc);
                if (p > 0.0) tent -= p * log(p);
            }
        }
        S = xlane_sum(S);
        soft = xlane_sum(soft);
        tent = xlane_sum(tent);
    }
    if (lane == 0) {
        const double vd = (double)v[row], z = (double)values[r];
        const double d = vd - z;
        double* o = rows + (int64_t)row * NCOL;
        o[0] = lse;
        o[1] = t_in ? lse - (double)xt : 0.0;
        o[2] = (double)rank;
        o[3] = lse - sex / se;
        o[4] = sv / se;
        o[5] = S;
        o[6] = soft;
        o[7] = tent;
        o[8] = vd;
        o[9] = d;
        o[10] = d * d;
        o[11] = vd * z > 0.0 ? 1.0 : 0.0;
        o[12] = rank == 0 ? 1.0 : 0.0;
        o[13] = rank < 5 ? 1.0 : 0.0;
        o[14] = t_in ? 0.0 : 1.0;
        o[15] = 1.0;
    }
}

// partials[j][c] = ((0.0 + rows[j][c]) + rows[j + 256][c]) + ...: thread (j, c), 16 partials per block, so
// a block's threads read 16 whole rows (2 KB, contiguous) per step
__global__ __launch_bounds__(256) void k_eval_reduce(const double* __restrict__ rows, int64_t n,
                                                     double* __restrict__ partials) {
    const int tid = blockIdx.x * 256 + threadIdx.x;  // < NPART * NCOL
    const int j = tid / NCOL, c = tid % NCOL;
    double acc = 0.0;
    int64_t i = j;
    for (; i + 7 * NPART < n; i += 8 * NPART) {  // eight loads in flight, added in the same ascending order
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; u++) t[u] = rows[(i + u * NPART) * NCOL + c];
#pragma unroll
        for (int u = 0; u < 8; u++) acc += t[u];
    }
    for (; i < n; i += NPART) acc += rows[i * NCOL + c];
    partials[tid] = acc;
}

// sums[c] = ((0.0 + partials[0][c]) + partials[1][c]) + ... + partials[255][c]
__global__ __launch_bounds__(64) void k_eval_sums(const double* __restrict__ partials, double* __restrict__ sums) {
    const int c = threadIdx.x;
    if (c >= NCOL) return;
    double acc = 0.0;
    for (int j = 0; j < NPART; j++) acc += partials[j * NCOL + c];
    sums[c] = acc;
}

struct Csr {
    const int64_t* indptr;
    const int32_t* cols;
    const double* vals;
};

void launch_rows(const float* logits, int64_t ld, const float* v, const yk_state_t* states, const int32_t* targets,
                 const float* values, const Csr& p, const int32_t* batch_idx, int64_t ex0, int n, double* rows,
                 bool masked, hipStream_t s) {
    if (masked)
        hipLaunchKernelGGL(k_eval_rows<true>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, logits, ld, v, states,
                           targets, values, p.indptr, p.cols, p.vals, batch_idx, ex0, n, rows);
    else
        hipLaunchKernelGGL(k_eval_rows<false>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, logits, ld, v, states,
                           targets, values, p.indptr, p.cols, p.vals, batch_idx, ex0, n, rows);
}

// rows[n][16] (device) -> HOST sums[16]; `work` is device scratch of (NPART + 1) * NCOL doubles
int reduce_to_host(const double* rows, int64_t n, double* work, double* sums, hipStream_t s) {
    hipLaunchKernelGGL(k_eval_reduce, dim3(NPART * NCOL / 256), dim3(256), 0, s, rows, n, work);
    YK_LAUNCHED();
    hipLaunchKernelGGL(k_eval_sums, dim3(1), dim3(64), 0, s, work, work + NPART * NCOL);
    YK_LAUNCHED();
    YK_HIP(hipMemcpyAsync(sums, work + NPART * NCOL, sizeof(double) * NCOL, hipMemcpyDeviceToHost, s));
    return YK_OK;
}

bool csr_ok(const int64_t* a, const int32_t* b, const double* c) { return (a && b && c) || (!a && !b && !c); }

// ---- yk_examples_check_legal: the contract of the legal-move mask over n examples.
// One wavefront per row, four rows per block.  A row's finding: 0 clean, 1 no valid action, 2 the hard
// target invalid or outside 0..3225, 3 a CSR entry with p > 0 whose column is invalid (or outside).  Block b
// writes code[b] = 4 * (its lowest offending row) + kind, or INT64_MAX; k_check_min takes the minimum of the
// codes - a minimum does not depend on the order, and no atomics touch data.
constexpr int64_t CLEAN = INT64_MAX;
__global__ __launch_bounds__(256) void k_check_legal(const yk_state_t* __restrict__ states,
                                                     const int32_t* __restrict__ targets,
                                                     const int64_t* __restrict__ indptr,
                                                     const int32_t* __restrict__ cols, const double* __restrict__ vals,
                                                     const int32_t* __restrict__ batch_idx, int n,
                                                     int64_t* __restrict__ code) {
    __shared__ int kinds[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + wave));
    int kind = 0;
    if (row < n) {
        const int64_t r = batch_idx ? (int64_t)batch_idx[row] : row;
        YkS s;
#pragma unroll
        for (int k = 0; k < 8; k++) s.w[k] = states[r].w[k];
        if (valid_row_bits<false>(s, 1, lane, nullptr) == 0) {
            kind = 1;
        } else {
            if (targets) {
                const int t = targets[r];
                if (t < 0 || t >= ASIZE || !action_valid(s, 1, t)) kind = 2;
            }
            if (kind == 0 && indptr) {
                const int64_t a1 = indptr[r + 1];
                bool bad = false;
                for (int64_t k = indptr[r] + lane; k < a1; k += 64) {
                    const int c = cols[k];
                    if (vals[k] > 0.0 && (c < 0 || c >= ASIZE || !action_valid(s, 1, c))) bad = true;
                }
                if (__ballot(bad)) kind = 3;
            }
        }
    }
    if (lane == 0) kinds[wave] = kind;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t c = CLEAN;
        for (int w = 3; w >= 0; w--)
            if (kinds[w]) c = 4 * ((int64_t)blockIdx.x * 4 + w) + kinds[w];
        code[blockIdx.x] = c;
    }
}
// out[0] = min of code[0 .. nb - 1]: thread t takes codes t, t + 256, ..., then a tree over the 256
__global__ __launch_bounds__(256) void k_check_min(const int64_t* __restrict__ code, int64_t nb,
                                                   int64_t* __restrict__ out) {
    __shared__ int64_t part[256];
    int64_t m = CLEAN;
    for (int64_t i = threadIdx.x; i < nb; i += 256) m = code[i] < m ? code[i] : m;
    part[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o && part[threadIdx.x + o] < part[threadIdx.x]) part[threadIdx.x] = part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = part[0];
}

int metrics_impl(const float* logits, int64_t ld, const float* v, const yk_state_t* states, const int32_t* targets,
                 const float* values, const int64_t* pi_indptr, const int32_t* pi_cols, const double* pi_vals,
                 const int32_t* batch_idx, int64_t n, double* rows, double* sums, bool masked, void* stream);
int evaluate_impl(yk_net_t* net, const yk_state_t* states, const int32_t* targets, const float* values,
                  const int64_t* pi_indptr, const int32_t* pi_cols, const double* pi_vals, const int32_t* batch_idx,
                  int64_t n, int chunk, double* rows, double* sums, bool masked, void* stream);

}  // namespace

extern "C" {

int yk_net_logits(yk_net_t* net, const yk_state_t* states, float* logits, float* v, int n, void* stream) {
    if (!net || !states || !logits || !v || n < 0) return YK_ERR_ARG;
    return launch_forward(net->dev, states, nullptr, nullptr, nullptr, n, logits, v, as_stream(stream));
}

int yk_examples_metrics(const float* logits, int64_t ld, const float* v, const yk_state_t* states,
                        const int32_t* targets, const float* values, const int64_t* pi_indptr,
                        const int32_t* pi_cols, const double* pi_vals, const int32_t* batch_idx, int64_t n,
                        double* rows, double* sums, void* stream) {
    return metrics_impl(logits, ld, v, states, targets, values, pi_indptr, pi_cols, pi_vals, batch_idx, n, rows, sums,
                        false, stream);
}

int yk_examples_metrics_legal(const float* logits, int64_t ld, const float* v, const yk_state_t* states,
                              const int32_t* targets, const float* values, const int64_t* pi_indptr,
                              const int32_t* pi_cols, const double* pi_vals, const int32_t* batch_idx, int64_t n,
                              double* rows, double* sums, void* stream) {
    return metrics_impl(logits, ld, v, states, targets, values, pi_indptr, pi_cols, pi_vals, batch_idx, n, rows, sums,
                        true, stream);
}

int yk_net_evaluate(yk_net_t* net, const yk_state_t* states, const int32_t* targets, const float* values,
                    const int64_t* pi_indptr, const int32_t* pi_cols, const double* pi_vals,
                    const int32_t* batch_idx, int64_t n, int chunk, double* rows, double* sums, void* stream) {
    return evaluate_impl(net, states, targets, values, pi_indptr, pi_cols, pi_vals, batch_idx, n, chunk, rows, sums,
                         false, stream);
}

int yk_net_evaluate_legal(yk_net_t* net, const yk_state_t* states, const int32_t* targets, const float* values,
                          const int64_t* pi_indptr, const int32_t* pi_cols, const double* pi_vals,
                          const int32_t* batch_idx, int64_t n, int chunk, double* rows, double* sums, void* stream) {
    return evaluate_impl(net, states, targets, values, pi_indptr, pi_cols, pi_vals, batch_idx, n, chunk, rows, sums,
                         true, stream);
}

int yk_examples_check_legal(const yk_state_t* states, const int32_t* targets, const int64_t* pi_indptr,
                            const int32_t* pi_cols, const double* pi_vals, const int32_t* batch_idx, int64_t n,
                            int64_t* first_bad, int* kind, void* stream) {
    if (!states || !first_bad || !kind || n < 0 || n > INT32_MAX || !csr_ok(pi_indptr, pi_cols, pi_vals))
        return YK_ERR_ARG;
    *first_bad = -1;
    *kind = 0;
    if (n == 0) return YK_OK;
    hipStream_t s = as_stream(stream);
    const int64_t nb = (n + 3) / 4;
    Scratch buf(s);
    YK_TRY(buf.alloc(sizeof(int64_t) * (size_t)(nb + 1)));
    int64_t* code = buf.as<int64_t>();
    hipLaunchKernelGGL(k_check_legal, dim3((unsigned)nb), dim3(256), 0, s, states, targets, pi_indptr, pi_cols, pi_vals,
                       batch_idx, (int)n, code);
    int rc = launched();
    if (rc == YK_OK) {
        hipLaunchKernelGGL(k_check_min, dim3(1), dim3(256), 0, s, code, nb, code + nb);
        rc = launched();
    }
    int64_t c = CLEAN;
    if (rc == YK_OK) rc = hip_rc(hipMemcpyAsync(&c, code + nb, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    (void)buf.release();
    YK_HIP(hipStreamSynchronize(s));
    if (rc == YK_OK && c != CLEAN) {
        *first_bad = c / 4;
        *kind = (int)(c % 4);
    }
    return rc;
}

}  // extern "C"

namespace {

int metrics_impl(const float* logits, int64_t ld, const float* v, const yk_state_t* states, const int32_t* targets,
                 const float* values, const int64_t* pi_indptr, const int32_t* pi_cols, const double* pi_vals,
                 const int32_t* batch_idx, int64_t n, double* rows, double* sums, bool masked, void* stream) {
    if (!logits || !v || !states || !targets || !values || !sums || n < 0 || n > INT32_MAX || ld < ASIZE ||
        !csr_ok(pi_indptr, pi_cols, pi_vals))
        return YK_ERR_ARG;
    for (int c = 0; c < NCOL; c++) sums[c] = 0.0;
    if (n == 0) return YK_OK;
    hipStream_t s = as_stream(stream);
    const size_t nwork = (size_t)(NPART + 1) * NCOL, nrows = rows ? 0 : (size_t)n * NCOL;
    Scratch buf(s);
    YK_TRY(buf.alloc(sizeof(double) * (nwork + nrows)));
    double* work = buf.as<double>();
    double* out = rows ? rows : work + nwork;
    launch_rows(logits, ld, v, states, targets, values, Csr{pi_indptr, pi_cols, pi_vals}, batch_idx, 0, (int)n, out,
                masked, s);
    int rc = launched();
    if (rc == YK_OK) rc = reduce_to_host(out, n, work, sums, s);
    (void)buf.release();
    YK_HIP(hipStreamSynchronize(s));
    return rc;
}

int evaluate_impl(yk_net_t* net, const yk_state_t* states, const int32_t* targets, const float* values,
                  const int64_t* pi_indptr, const int32_t* pi_cols, const double* pi_vals, const int32_t* batch_idx,
                  int64_t n, int chunk, double* rows, double* sums, bool masked, void* stream) {
    if (!net || !states || !targets || !values || !sums || n < 0 || n > INT32_MAX ||
        !csr_ok(pi_indptr, pi_cols, pi_vals))
        return YK_ERR_ARG;
    for (int c = 0; c < NCOL; c++) sums[c] = 0.0;
    if (n == 0) return YK_OK;
    hipStream_t s = as_stream(stream);
    const int64_t ch = std::min<int64_t>(chunk <= 0 ? 16384 : chunk, n);
    // one allocation: logits[ch][PI_LD] f32 | v[ch] f32 (padded to 8 B) | work | rows (when not given)
    const size_t nf = (size_t)ch * PI_LD + (((size_t)ch + 1) & ~(size_t)1);
    const size_t nwork = (size_t)(NPART + 1) * NCOL, nrows = rows ? 0 : (size_t)n * NCOL;
    Scratch buf(s);
    YK_TRY(buf.alloc(sizeof(float) * nf + sizeof(double) * (nwork + nrows)));
    float* logits = buf.as<float>();
    float* v = logits + (size_t)ch * PI_LD;
    double* work = reinterpret_cast<double*>(logits + nf);
    double* out = rows ? rows : work + nwork;
    const Csr p{pi_indptr, pi_cols, pi_vals};
    int rc = YK_OK;
    for (int64_t c0 = 0; c0 < n && rc == YK_OK; c0 += ch) {
        const int m = (int)std::min<int64_t>(ch, n - c0);
        const int32_t* idx = batch_idx ? batch_idx + c0 : nullptr;
        rc = launch_forward(net->dev, idx ? states : states + c0, nullptr, idx, nullptr, m, logits, v, s);
        if (rc != YK_OK) break;
        launch_rows(logits, PI_LD, v, states, targets, values, p, idx, c0, m, out + c0 * NCOL, masked, s);
        rc = launched();
    }
    if (rc == YK_OK) rc = reduce_to_host(out, n, work, sums, s);
    (void)buf.release();
    YK_HIP(hipStreamSynchronize(s));
    return rc;
}

}  // namespace
