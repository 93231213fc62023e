// yk_api.h - host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "yacht_hip.h"

namespace yk {
void set_hip_error(hipError_t e);
inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline int grid_for(long n, int per_block) { return (int)((n + per_block - 1) / per_block); }

// The packed trajectory record image of one engine batch (yk_engine_pack_records), shared by
// the engine (writer) and the replay kernels (reader): 8 parts, each padded to 16 B -
// states[E][M] (64 B) | info[E][M][8] i32 | ctr[E][M][2] u64 | values[E][M] f64 |
// visits[E][VCAP] u32 | visits_off[E][M+1] i32 | n_moves[E] i32 | final[E] (64 B).
enum { REC_STATES, REC_INFO, REC_CTR, REC_VALUES, REC_VISITS, REC_VOFF, REC_NMOVES, REC_FINAL, REC_PARTS };
struct RecordLayout {
    int64_t off[REC_PARTS], bytes[REC_PARTS], total;
};
inline int64_t record_vcap(int64_t M, int64_t sims) { return 2 * M * (sims > 32 ? sims : 32); }
inline RecordLayout record_layout(int64_t E, int64_t M, int64_t VCAP) {
    RecordLayout L;
    const int64_t b[REC_PARTS] = {E * M * 64, E * M * 8 * 4, E * M * 2 * 8, E * M * 8,
                                  E * VCAP * 4, E * (M + 1) * 4, E * 4, E * 64};
    int64_t off = 0;
    for (int i = 0; i < REC_PARTS; i++) {
        L.off[i] = off;
        L.bytes[i] = b[i];
        off += (b[i] + 15) & ~15LL;
    }
    L.total = off;
    return L;
}

// YK_ERR_HIP (and the error kept for yk_last_hip_error) unless `e` is hipSuccess
inline int hip_rc(hipError_t e) {
    if (e == hipSuccess) return YK_OK;
    set_hip_error(e);
    return YK_ERR_HIP;
}
// after a kernel launch: whether the launch was accepted
inline int launched() { return hip_rc(hipGetLastError()); }
// drops the error a failed hipMalloc leaves behind (its caller reports YK_ERR_NOMEM)
inline void clear_hip_error() { (void)hipGetLastError(); }

// One stream-ordered device allocation (alloc() once).  Its hipFreeAsync is issued by release(), or by the
// destructor on every path that returns before it: an early return cannot leak.  Where the free has to
// precede a hipStreamSynchronize, call release() before it.
struct Scratch {
    void* p = nullptr;
    hipStream_t st;
    explicit Scratch(hipStream_t s) : st(s) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { (void)release(); }
    int alloc(size_t bytes) {
        const int rc = hip_rc(hipMallocAsync(&p, bytes, st));
        if (rc != YK_OK) p = nullptr;
        return rc;
    }
    hipError_t release() {  // (not recorded: after an earlier error the caller ignores it, and that error stays)
        void* q = p;
        p = nullptr;
        return q ? hipFreeAsync(q, st) : hipSuccess;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// The persistent hipMalloc blocks of one handle (engine, trainer, net): the destructor frees them all,
// so a handle that owns one cannot leak its device memory on any path that destroys it.
struct DeviceBlocks {
    std::vector<void*> blocks;
    DeviceBlocks() = default;
    DeviceBlocks(const DeviceBlocks&) = delete;
    DeviceBlocks& operator=(const DeviceBlocks&) = delete;
    ~DeviceBlocks() {
        for (void* p : blocks) (void)hipFree(p);
    }
    // `count` elements (0: one, so the pointer is always valid); YK_ERR_NOMEM, the HIP error dropped, else
    template <class T>
    int alloc(T** p, size_t count) {
        void* q = nullptr;
        if (hipMalloc(&q, sizeof(T) * (count ? count : 1)) != hipSuccess) {
            clear_hip_error();
            return YK_ERR_NOMEM;
        }
        blocks.push_back(q);
        *p = static_cast<T*>(q);
        return YK_OK;
    }
};
// The state_dict tensors that are weight matrices (packed to fp16 by yk_net_create, cast to fp16 by the
// mixed-precision trainer): input_fc.weight 0, block b's fc1.weight 4 + 8 b and fc2.weight 8 + 8 b,
// pi_head.2.weight 6 + 8 NB, v_head.2.weight 10 + 8 NB.  Whether fp16(w) is finite for every finite weight
// of them: |w| >= 65520 rounds to inf, where torch's float32 holds a number.  (yk_net.hip)
bool matrices_fit_fp16(const float* const* params, int H, int NB);
}  // namespace yk

// return the YK_* code of `call` unless it is YK_OK
#define YK_TRY(call)                                   \
    do {                                               \
        const int rc_ = (call);                        \
        if (rc_ != YK_OK) return rc_;                  \
    } while (0)
#define YK_HIP(call) YK_TRY(yk::hip_rc(call))
#define YK_LAUNCHED() YK_TRY(yk::launched())
