// yk_rootval.hip - the search's own value of each real move of self-play: the kernel
// that writes the visit-weighted mean of the root's edge values into the record's spare word
// info[e][m][7].  Its own translation unit and its own kernel argument, as the root noise (yk_noise.hip):
// EngDev and the search kernels' code object are the same with and without the feature.
#include <string.h>

#include "yk_engine_dev.h"

namespace {

// One wave per game, launched after k_move_end(move): the games that made this move are those with
// nmoves[e] == move + 1 (k_move_end sets it, also when the real step failed), and root[e] is still the
// move's root (k_move_begin of the next move replaces it).  Over the root's visited edges (N > 0) in
// ascending compact order, which is ascending action order:
//     num += (double)N * Q ;  den += (double)N ;  q32 = (float)(num / den)
// every operation rounded on its own (-ffp-contract=off).  64 entries at a time: each lane loads its
// entry's slot and edge, the ballot of the visited ones is walked from the lowest lane up and each
// (N, Q) is read out of its lane into uniform registers, so the whole wave carries the one sequential
// sum and nothing goes through LDS.  The word is q32's bit pattern, +-0 as 0x80000000: a recorded
// value is never the zero word.  A root that is not in the tree or has no visited edge leaves the 0
// k_move_end wrote (both are error states it reports).
__global__ __launch_bounds__(64 * GAMES_PER_BLOCK) void k_root_value(EngDev d, RootValDev rv) {
    const int lane = threadIdx.x & 63;
    const int e = d.e_lo + (int)blockIdx.x * GAMES_PER_BLOCK + ((int)threadIdx.x >> 6);
    const int move = rv.move;
    if (e >= d.e_hi || move >= d.M || d.nmoves[e] != move + 1 || d.idle[e]) return;
    int32_t* info = d.rec_info + ((long)e * d.M + move) * 8;
    // the tree k_move_end searched: tree_of() before the real step changed cur, i.e. with the recorded mover
    const int t = (d.dual && info[1] != d.seat[e]) ? e + d.E : e;
    const int g = d.gen[t];
    const YkS r = ld_state(d.root + e);
    const int nid = lookup(d, g, t, r, index_hash(r));
    if (nid < 0) return;
    const NodeRec& nd = d.nodes[g][(long)t * d.NCAP + nid];
    const uint16_t* S = d.arenaS + (long)t * d.AE + nd.p_off;
    const Edge* edges = d.edges[g] + (long)t * d.ECAP;
    const int nv = (int)nd.nvalid;
    double num = 0.0, den = 0.0;
    // 8 pieces of 64 entries per round trip, as k_move_end reads the same lists
    constexpr int MB = 8;
    for (int j0 = 0; j0 < nv; j0 += 64 * MB) {
        uint16_t sl[MB];
#pragma unroll
        for (int b = 0; b < MB; b++) {
            const int j = j0 + 64 * b + lane;
            const uint16_t x = S[j < nv ? j : 0];  // unconditional loads (in bounds)
            sl[b] = j < nv ? x : 0;
        }
        uint32_t n[MB];
        double q[MB];
#pragma unroll
        for (int b = 0; b < MB; b++) {
            const Edge ed = edges[sl[b] ? sl[b] - 1 : 0];
            n[b] = sl[b] ? ed.N : 0u;
            q[b] = ed.Q;
        }
#pragma unroll
        for (int b = 0; b < MB; b++) {
            const uint32_t qlo = (uint32_t)__double_as_longlong(q[b]);
            const uint32_t qhi = (uint32_t)((uint64_t)__double_as_longlong(q[b]) >> 32);
            uint64_t bal = __ballot(n[b] != 0);
            while (bal) {  // (wave-uniform) ascending lanes = ascending compact index
                const int src = __ffsll((long long)bal) - 1;
                bal &= bal - 1;
                const uint32_t ni = (uint32_t)__builtin_amdgcn_readlane((int)n[b], src);
                const uint64_t qb = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)qlo, src) |
                                    ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)qhi, src) << 32);
                const double w = (double)ni;
                num = num + w * __longlong_as_double((long long)qb);
                den = den + w;
            }
        }
    }
    if (lane != 0 || den == 0.0) return;
    const uint32_t bits = __float_as_uint((float)(num / den));
    info[7] = (int32_t)((bits << 1) == 0u ? 0x80000000u : bits);
}

}  // namespace

int yk_launch_root_value(const void* engdev, size_t engdev_bytes, const void* rvdev, size_t rvdev_bytes,
                         hipStream_t stream) {
    if (!engdev || !rvdev || engdev_bytes != sizeof(EngDev) || rvdev_bytes != sizeof(RootValDev)) return YK_ERR_ARG;
    EngDev d;
    RootValDev rv;
    memcpy(&d, engdev, sizeof(d));
    memcpy(&rv, rvdev, sizeof(rv));
    if (d.e_hi <= d.e_lo) return YK_OK;
    const unsigned blocks = (unsigned)((d.e_hi - d.e_lo + GAMES_PER_BLOCK - 1) / GAMES_PER_BLOCK);
    hipLaunchKernelGGL(k_root_value, dim3(blocks), dim3(64 * GAMES_PER_BLOCK), 0, stream, d, rv);
    YK_LAUNCHED();
    return YK_OK;
}
