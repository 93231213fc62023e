// yk_ema.hip - the averaged (EMA) weights: one streaming pass that moves a shadow of the
// trainer's flat parameter buffer toward it, and the host weight schedule.  Its own translation unit: every other
// kernel compiles as before.
//
//     e <- e + w * (p - e)      three float32 operations, each rounded once (-ffp-contract=off: never an fma)
//
// Each element is read and written by one thread and depends on nothing else: no atomics, no LDS, no workgroup
// waits for another, and equal inputs give equal bits whatever the grid.
#include "yk_api.h"

namespace {

constexpr int TPB = 256;
// The stream is 12 bytes per element; 2048 workgroups of 256 threads (8 per CU on 256 CUs) keep every CU's
// memory queue full, and a larger buffer strides over the grid.  One pass of the full grid covers
// MAX_BLOCKS * 256 * 4 elements (2^21) on the vector path, MAX_BLOCKS * 256 on the scalar one.
constexpr int MAX_BLOCKS = 2048;

typedef float f4v_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f4v_t gf4_t;
typedef __attribute__((address_space(1))) float gf_t;
typedef const __attribute__((address_space(1))) f4v_t cgf4_t;
typedef const __attribute__((address_space(1))) float cgf_t;

__device__ __forceinline__ float ema1(float e, float p, float w) {
    const float d = p - e;
    const float s = w * d;
    return e + s;
}

// vec: both pointers are 16-byte aligned - elements 0 .. 4 * (n / 4) - 1 go as float4, the tail as scalars;
// otherwise every element takes the scalar path.
__global__ void __launch_bounds__(TPB) k_ema(float* ema, const float* params, int64_t n, float w, int vec) {
    const int64_t tid = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * TPB;
    gf_t* e1 = (gf_t*)ema;
    cgf_t* p1 = (cgf_t*)params;
    int64_t done = 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        gf4_t* e4 = (gf4_t*)ema;
        cgf4_t* p4 = (cgf4_t*)params;
        for (int64_t i = tid; i < n4; i += stride) {
            const f4v_t e = e4[i], p = p4[i];
            f4v_t r;
            r.x = ema1(e.x, p.x, w);
            r.y = ema1(e.y, p.y, w);
            r.z = ema1(e.z, p.z, w);
            r.w = ema1(e.w, p.w, w);
            e4[i] = r;
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += stride) e1[i] = ema1(e1[i], p1[i], w);
}

}  // namespace

extern "C" {

int yk_ema_weight(double decay, int64_t t, float* w) {
    if (!w || !(decay >= 0.0 && decay < 1.0) || t < 0) return YK_ERR_ARG;
    const double warm = (1.0 + (double)t) / (10.0 + (double)t);
    const double d = decay < warm ? decay : warm;
    *w = (float)(1.0 - d);
    return YK_OK;
}

int yk_ema_update(float* ema, const float* params, int64_t n, float w, void* stream) {
    if (!ema || !params || n < 0 || !(w >= 0.0f && w <= 1.0f)) return YK_ERR_ARG;
    if (n == 0) return YK_OK;
    const int vec = (((uintptr_t)ema | (uintptr_t)params) & 15) == 0;
    const int64_t items = vec ? ((n >> 2) > 0 ? (n >> 2) : 1) : n;  // (n < 4: one block for the tail)
    int64_t blocks = (items + TPB - 1) / TPB;
    if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
    hipLaunchKernelGGL(k_ema, dim3((unsigned)blocks), dim3(TPB), 0, yk::as_stream(stream), ema, params, n, w, vec);
    YK_LAUNCHED();
    return YK_OK;
}

}  // extern "C"
