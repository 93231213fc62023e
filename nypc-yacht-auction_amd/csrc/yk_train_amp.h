// yk_train_amp.h - the mixed-precision train step (yk_train_amp.hip) as the f32 trainer
// (yk_train.hip) drives it: NNetWrapper.train under autocast('cuda') + GradScaler
// (yacht/NNet.py:113-116, 141-155) on hand-written fp16 MFMA kernels with f32 accumulation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yacht_hip.h"

namespace yk {

struct AmpTrain;  // device buffers of the mixed-precision step (fp16 weight copies, saved activations)

// Soft policy targets (yk_trainer_*_soft): the visit policies as the device CSR yk_examples_policies
// writes.  Batch row i's entries are indptr[src] .. indptr[src + 1] - 1 of replay entry src.
struct SoftCsr {
    const int64_t* indptr;
    const int32_t* cols;
    const double* vals;
    float* psum;    // trainer scratch: [batch] each row's sum of probabilities s_i
    int64_t* pcut;  // (amp) [batch][BQ + 1]: where the head-backward parts' runs of a row begin
};
// entry k's probability as a float32 tensor holds it (torch.as_tensor(pi).float()); 0 for an
// entry whose column is not an action (ignored everywhere)
__device__ __forceinline__ float soft_p(const SoftCsr& c, int64_t k, int col) {
    return (unsigned)col < (unsigned)YK_ACTION_SIZE ? (float)c.vals[k] : 0.0f;
}
// s_i = the float32 sum of a row's probabilities in CSR order, by one wave: 64 entries load at
// once, the adds run in entry order (a lane past the row adds +0).  The same value on every lane.
__device__ __forceinline__ float soft_row_sum(const SoftCsr& c, int64_t a0, int64_t a1, int lane) {
    float s = 0.0f;
    for (int64_t b = a0; b < a1; b += 64) {
        const int64_t k = b + lane;
        float v = 0.0f;
        if (k < a1) v = soft_p(c, k, c.cols[k]);
#pragma unroll
        for (int j = 0; j < 64; j++)
            s += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
    }
    return s;
}

// P / G / M / V: the trainer's flat f32 parameter, gradient and AdamW moment buffers (nparams each) in
// YachtNNet.state_dict() order, off[k]: offset of tensor k.  lrow / lsum: the trainer's per-row losses
// [Bmax] and their two column sums.  init_scale / growth_interval: GradScaler('cuda') (65536, 2000).
int amp_create(AmpTrain** out, int H, int NB, int Bmax, float* P, float* G, float* M, float* V, long nparams,
               const long* off, float2* lrow, float* lsum, float init_scale, int growth_interval);
void amp_destroy(AmpTrain* a);
// fp16 copies of every weight matrix (both MFMA operand orientations) from P
int amp_pack(AmpTrain* a, hipStream_t s);
// forward + backward of `B` examples into G (gradients of loss_scale x loss, each fp16-rounded as
// autocast's fp16 GEMMs return them); lrow[i] = (cross-entropy, squared value error) of row i,
// lsum = their column sums.  Dropout masks: rows are numbered row_base + i.  fuse_norm: the
// gradient launches also sum the unscaled sq-norm, and the next amp_apply uses it instead of
// re-reading G (only when nothing changes G in between: yk_trainer_step, not the DDP split).
// soft: the visit policies as targets (cross-entropy with probability targets; `targets` unused),
// or null for the hard labels.  legal: the batch rows' valid-action bits [B][LEGAL_LD] (yk_legal.h; the
// legal-move mask: an invalid action's fp16 logit becomes -inf where k_amp_head makes it), or null.
int amp_backward(AmpTrain* a, const yk_state_t* states, const int32_t* targets, const SoftCsr* soft,
                 const float* values, const int32_t* idx, int B, float dropout, uint64_t seed, uint64_t step, int64_t row_base,
                 float vloss_weight, bool fuse_norm, const uint32_t* legal, hipStream_t s);
// GradScaler.unscale_ + clip_grad_norm_(max_norm) + AdamW step (skipped, with the scale halved,
// when a gradient is inf / nan) + GradScaler.update + fp16 repack.  sq_out: the unscaled grad
// sq-norm (double).  dropout / seed / next_step: the next backward's dropout draws, which the
// update launch makes ahead (for row offset 0) so that backward needs no mask launch of its own.
int amp_apply(AmpTrain* a, double* sq_out, float max_norm, float lr, float wd, float b1, float b2, float eps,
              float dropout, uint64_t seed, uint64_t next_step, hipStream_t s);
// HOST out[4]: loss scale, growth tracker, optimiser steps taken, whether the last step found inf
int amp_state(AmpTrain* a, double* out);
int amp_set_steps(AmpTrain* a, int64_t steps);
int64_t amp_steps(AmpTrain* a);

}  // namespace yk
