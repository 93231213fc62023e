// yk_augment.hip - symmetry augmentation of training examples: yk_examples_augment.
//
// The game depends only on the multisets of the dice and is symmetric in the two auction groups, but
// state_to_vec and the score actions are positional.  Per example and epoch this kernel draws a random
// member of that symmetry group - a permutation of each carry and each roll, an exchange of the groups -
// and writes the transformed board, the target under the matching action bijection and the example's
// policy row under it, re-sorted.  Its own translation unit, as yk_noise.hip: no other code object of
// the library changes with it.
//
// One wave per example.  Lane i draws Philox word x1 of draw i (49 draws, one round trip); every
// Fisher-Yates step then reads its draw with v_readlane, so the state transform is wave-uniform
// arithmetic on nibble-packed permutations in registers.  The CSR row: the mapped columns set bits in a
// 101-word LDS bitmap, a wave prefix over the word popcounts numbers the set bits, and each entry goes
// to the slot numbered by the set bits below its own - ascending order, no global atomics, any row length.
#include "yk_api.h"
#include "yk_common.h"

using namespace yk;

namespace {

constexpr int AUG_CARRY = 1, AUG_ROLLS = 2, AUG_GROUPS = 4;
constexpr int DRAW_P1 = 0, DRAW_P2 = 16, DRAW_A = 32, DRAW_B = 40, DRAW_SWAP = 48;  // first draw of each list
constexpr uint64_t IDENT = 0x9876543210ull;   // the identity permutation of 10 positions as nibbles
constexpr int64_t AUG_MAX_GRID = 1 << 30;

// rank of a 5-of-10 combo (its index in itertools.combinations(range(10), 5) order, YachtGame.py:35)
// from its position bitmask
struct RankTab {
    uint8_t r[1024];
};
constexpr RankTab make_rank() {
    RankTab t{};
    for (int m = 0; m < 1024; m++) t.r[m] = 0xFF;
    for (int i = 0; i < NCOMB; i++) t.r[h_tab.comb_mask[i]] = (uint8_t)i;
    return t;
}
constexpr bool rank_is_combo_order() {
    const RankTab t = make_rank();
    int seen = 0;
    for (int m = 0; m < 1024; m++) {
        int bits = 0;
        for (int b = 0; b < 10; b++) bits += (m >> b) & 1;
        if ((t.r[m] != 0xFF) != (bits == 5)) return false;  // exactly the 252 masks of five positions
        seen += t.r[m] != 0xFF;
    }
    if (seen != NCOMB) return false;
    for (int i = 0; i < NCOMB; i++) {
        uint32_t m = 0, key = 0;  // key: the positions as digits, first position most significant
        for (int k = 0; k < 5; k++) {
            const uint32_t p = (h_tab.comb_pos[i] >> (4 * k)) & 0xF;
            if (p > 9) return false;
            m |= 1u << p;
            key = key * 16 + p;
        }
        if (m != h_tab.comb_mask[i] || t.r[m] != i) return false;
        if (i > 0) {  // lexicographic, strictly ascending: the order of itertools.combinations
            uint32_t prev = 0;
            for (int k = 0; k < 5; k++) prev = prev * 16 + ((h_tab.comb_pos[i - 1] >> (4 * k)) & 0xF);
            if (prev >= key) return false;
        }
    }
    return true;
}
static_assert(rank_is_combo_order(), "rank table == index in COMB_5_OF_10 order");
__constant__ RankTab c_rank = make_rank();

// Fisher-Yates over L <= 10 positions with first draw b (lane i of x1 holds draw i): perm = [0 .. L-1];
// for m = L-1 .. 1: j = below_{b + (L-1-m)}(m + 1), swap perm[m], perm[j].  Nibble i of the result is
// perm[i]; i >= L: i.
__device__ __forceinline__ uint64_t fisher_yates(int L, int b, uint32_t x1) {
    uint64_t perm = IDENT;
    for (int m = L - 1; m >= 1; m--) {
        const int j = (int)(((uint64_t)lane_val(x1, b + (L - 1 - m)) * (uint32_t)(m + 1)) >> 32);
        const uint64_t pm = (perm >> (4 * m)) & 0xF, pj = (perm >> (4 * j)) & 0xF;
        perm = (perm & ~(0xFull << (4 * m)) & ~(0xFull << (4 * j))) | (pj << (4 * m)) | (pm << (4 * j));
    }
    return perm;
}
// new[i] = old[perm[i]] on the low L nibbles of v; the bits above them are kept
__device__ __forceinline__ uint64_t permute_nibbles(uint64_t v, uint64_t perm, int L) {
    uint64_t nw = 0;
#pragma unroll
    for (int i = 0; i < 10; i++)
        if (i < L) nw |= ((v >> (4 * ((perm >> (4 * i)) & 0xF))) & 0xF) << (4 * i);
    return (v & ~((1ull << (4 * L)) - 1)) | nw;
}
__device__ __forceinline__ uint64_t inverse_perm(uint64_t perm) {
    uint64_t inv = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) inv |= (uint64_t)i << (4 * ((perm >> (4 * i)) & 0xF));
    return inv;
}

// what example k's draws decided, as far as the actions see it
struct ActMap {
    int phase, n1;  // the board's phase; len(p1 carry)
    bool swap;      // the groups were exchanged
    uint64_t inv1;  // perm1^-1 as nibbles: old carry position p moves to nibble p
};
// A_k (per lane): bids move with their group; a score action's combo moves with the carry positions
__device__ __forceinline__ int map_action(const ActMap& am, int a) {
    if (am.phase == 0) {
        if (am.swap && a >= 0 && a < NBID) a = a >= BID_LEVELS ? a - BID_LEVELS : a + BID_LEVELS;
        return a;
    }
    if (a >= NBID && a < ASIZE) {
        const int base = a - NBID, cat = base / NCOMB, ci = base - cat * NCOMB;
        // (the 16-bit mask table, not comb_pos: for a wave-uniform ci the compiler split &comb_pos[ci] into an
        // unaligned scalar base and offset, and that s_load_dword read entry ci - 1 on gfx950)
        const uint32_t mask = c_tab.comb_mask[ci];
        if ((mask >> am.n1) == 0) {  // max(comb) < len(p1 carry)
            uint32_t m = 0;
#pragma unroll
            for (int p = 0; p < 10; p++) m |= ((mask >> p) & 1u) << (uint32_t)((am.inv1 >> (4 * p)) & 0xF);
            a = NBID + cat * NCOMB + (int)c_rank.r[m & 1023u];
        }
    }
    return a;
}

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// One wave (= one workgroup) per row; row i of the call is example index_base + i.
__global__ __launch_bounds__(64) void k_augment(const yk_state_t* states, const int32_t* targets,
                                                const int64_t* indptr, const int32_t* cols, const double* vals,
                                                int64_t row0, int64_t index_base, uint64_t seed, uint32_t epoch_key,
                                                int flags, yk_state_t* out_states, int32_t* out_targets,
                                                int32_t* out_cols, double* out_vals) {
    __shared__ uint32_t s_bits[MASK_WORDS];  // the mapped columns of this row
    __shared__ uint32_t s_below[MASK_WORDS];  // set bits in the words before each word
    const int lane = threadIdx.x;
    const int64_t r = row0 + (int64_t)blockIdx.x;
    const uint64_t mine = lane < 8 ? states[r].w[lane] : 0;
    // draw `lane` of this example: word 1 of the Philox output
    const uint32_t x1 =
        philox4x32_10(seed, (uint32_t)lane, (uint32_t)(uint64_t)(index_base + r), epoch_key, PHILOX_SYMMETRY).x1;
    YkS s;
#pragma unroll
    for (int i = 0; i < 8; i++) s.w[i] = lane_val(mine, i);

    // ---- the state (wave-uniform)
    const int n1 = min(wa_n(s.w[1]), 10), n2 = min(wa_n(s.w[4]), 10);
    uint64_t perm1 = IDENT;
    if (flags & AUG_CARRY) {
        perm1 = fisher_yates(n1, DRAW_P1, x1);
        s.w[1] = permute_nibbles(s.w[1], perm1, n1);
        s.w[4] = permute_nibbles(s.w[4], fisher_yates(n2, DRAW_P2, x1), n2);
    }
    uint64_t w0 = s.w[0];
    uint64_t rA = (w0 >> 24) & 0xFFFFF, rB = (w0 >> 44) & 0xFFFFF;
    uint64_t hasA = (w0 >> 5) & 1, hasB = (w0 >> 6) & 1, b1 = (w0 >> 8) & 0xFF, b2 = (w0 >> 16) & 0xFF;
    if (flags & AUG_ROLLS) {
        if (hasA) rA = permute_nibbles(rA, fisher_yates(5, DRAW_A, x1), 5);
        if (hasB) rB = permute_nibbles(rB, fisher_yates(5, DRAW_B, x1), 5);
    }
    const bool swap = (flags & AUG_GROUPS) && (lane_val(x1, DRAW_SWAP) >> 31);
    if (swap) {
        uint64_t t = rA;
        rA = rB;
        rB = t;
        t = hasA;
        hasA = hasB;
        hasB = t;
        if (b1 != 0xFF) b1 ^= 0x80;
        if (b2 != 0xFF) b2 ^= 0x80;
    }
    ActMap am;
    am.phase = s_phase(s);
    am.n1 = n1;
    am.swap = swap;
    am.inv1 = inverse_perm(perm1);
    s.w[0] = (w0 & 0x9Full) | (hasA << 5) | (hasB << 6) | (b1 << 8) | (b2 << 16) | (rA << 24) | (rB << 44);
    uint64_t o = s.w[0];
#pragma unroll
    for (int i = 1; i < 8; i++) o = lane == i ? s.w[i] : o;
    if (lane < 8) out_states[r].w[lane] = o;
    if (targets && lane == 0) out_targets[r] = map_action(am, targets[r]);
    if (!indptr) return;

    // ---- the policy row
    const int64_t e0 = indptr[r], e1 = indptr[r + 1];
    if (e1 - e0 <= 1) {  // (one-hot rows, most of a shard: nothing to order)
        if (e1 - e0 == 1 && lane == 0) {
            out_cols[e0] = map_action(am, cols[e0]);
            out_vals[e0] = vals[e0];
        }
        return;
    }
    for (int i = lane; i < MASK_WORDS; i += 64) s_bits[i] = 0;
    __syncthreads();
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        const int c = cols[e];
        if (c < 0 || c >= ASIZE) continue;  // not an action: no bit, no slot (the row's output is unspecified)
        const int a = map_action(am, c);    // (a bijection of 0 .. 3225: inside the bitmap)
        atomicOr(&s_bits[a >> 5], 1u << (a & 31));
    }
    __syncthreads();
    const uint32_t p0 = (uint32_t)__popc(s_bits[lane]), p1 = lane + 64 < MASK_WORDS ? (uint32_t)__popc(s_bits[lane + 64]) : 0u;
    const uint32_t i0 = wave_inclusive_scan(p0, lane), i1 = wave_inclusive_scan(p1, lane);
    const uint32_t first64 = lane_val(i0, 63);
    s_below[lane] = i0 - p0;
    if (lane + 64 < MASK_WORDS) s_below[lane + 64] = first64 + i1 - p1;
    __syncthreads();
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        const int c = cols[e];
        if (c < 0 || c >= ASIZE) continue;
        const int a = map_action(am, c);
        // set bits below a's: at most (entries of the row) - 1, so the slot is inside the row
        const int64_t slot = e0 + s_below[a >> 5] + (uint32_t)__popc(s_bits[a >> 5] & ((1u << (a & 31)) - 1u));
        out_cols[slot] = a;
        out_vals[slot] = vals[e];
    }
}

}  // namespace

extern "C" int yk_examples_augment(const yk_state_t* states, const int32_t* targets, const int64_t* pi_indptr,
                                   const int32_t* pi_cols, const double* pi_vals, int64_t n, int64_t index_base,
                                   uint64_t seed, uint32_t epoch_key, int flags, yk_state_t* out_states,
                                   int32_t* out_targets, int32_t* out_cols, double* out_vals, void* stream) {
    if (n < 0 || flags < 0 || flags > (AUG_CARRY | AUG_ROLLS | AUG_GROUPS)) return YK_ERR_ARG;
    if ((targets == nullptr) != (out_targets == nullptr)) return YK_ERR_ARG;
    const int csr = (pi_indptr != nullptr) + (pi_cols != nullptr) + (pi_vals != nullptr) + (out_cols != nullptr) +
                    (out_vals != nullptr);
    if (csr != 0 && csr != 5) return YK_ERR_ARG;
    if (n > 0 && (!states || !out_states)) return YK_ERR_ARG;
    if (n > 0 && (states == out_states || (targets && targets == out_targets) ||
                  (csr && (pi_cols == out_cols || pi_vals == out_vals))))
        return YK_ERR_ARG;
    for (int64_t row0 = 0; row0 < n; row0 += AUG_MAX_GRID) {
        const int64_t rows = n - row0 < AUG_MAX_GRID ? n - row0 : AUG_MAX_GRID;
        hipLaunchKernelGGL(k_augment, dim3((unsigned)rows), dim3(64), 0, as_stream(stream), states, targets, pi_indptr,
                           pi_cols, pi_vals, row0, index_base, seed, epoch_key, flags, out_states, out_targets,
                           out_cols, out_vals);
        YK_LAUNCHED();
    }
    return YK_OK;
}
