// yk_legal.h - one state's valid-action bits by one wavefront: the row routine of yk_valid_mask
// (yk_env.hip), shared with the trainers' legal-move mask (yk_train.hip) and
// yk_examples_check_legal (yk_eval.hip).
#pragma once
#include "yk_common.h"

namespace yk {

// row stride (u32 words) of the trainers' legal-bits buffer: MASK_WORDS = 101 are used, 104 keeps
// every row 16-byte aligned
constexpr int LEGAL_LD = 104;
static_assert(LEGAL_LD >= MASK_WORDS && LEGAL_LD % 4 == 0, "legal rows: 101 words, 16-byte aligned");

// The wave's 64 lanes ballot 64 action bits per iteration; lanes 0 and 1 store the two words into
// row[0 .. MASK_WORDS - 1] (bit a & 31 of word a >> 5 = action_valid(s, pl, a); STORE false: no
// stores, row unused).  Returns the number of valid actions, the same on every lane.
// part / nparts: the wave takes the 64-action iterations part, part + nparts, ... only (several waves share a
// row: each stores its own words and returns its own count); the default is the whole row.
template <bool STORE = true>
__device__ __forceinline__ int valid_row_bits(const YkS& s, int pl, int lane, uint32_t* row, int part = 0,
                                              int nparts = 1) {
    int total = 0;
    for (int base = 64 * part; base < 64 * ((ASIZE + 63) / 64); base += 64 * nparts) {
        const int a = base + lane;
        const bool v = a < ASIZE && action_valid(s, pl, a);
        const uint64_t b = __ballot(v);
        total += __popcll(b);
        const int word = base / 32;
        if (STORE && lane == 0 && word < MASK_WORDS) row[word] = (uint32_t)b;
        if (STORE && lane == 1 && word + 1 < MASK_WORDS) row[word + 1] = (uint32_t)(b >> 32);
    }
    return total;
}

}  // namespace yk
