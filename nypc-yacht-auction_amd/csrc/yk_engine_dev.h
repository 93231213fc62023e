// yk_engine_dev.h - the self-play engine's device-side data layout and tree lookups, shared
// by yk_engine.hip (the search kernels), yk_noise.hip (the root-noise kernel) and yk_rootval.hip (the
// root-value kernel).  The root noise and the root value are their own translation units, so the search
// kernels' code object is the same whether or not the features are built in.  Internal linkage
// throughout: each unit compiles its own copy.
#pragma once
#include <math.h>
#include <stddef.h>

#include <type_traits>

#include "yk_api.h"
#include "yk_common.h"

using namespace yk;

namespace {

constexpr int MAXD = 64;          // max search depth (path entries)
constexpr int LUT_N = 1 << 16;    // f32(sqrt(Ns)), f32(sqrt(Ns + 1e-8)) table size
constexpr int GAMES_PER_BLOCK = 4;
constexpr int GROUP_ALIGN = 16;   // group boundaries on forward row tiles
constexpr int YK_EXPAND_WPE = 4;  // waves per SIMD the expand kernel is register-budgeted for
// The root's incremental UCB scan: per tree, the root's compact set sorted by P
// (descending, ascending index on ties) and the list of its visited edges, valid for one move
constexpr int RO_CAP = 3072;      // >= the largest compact valid set (3024)
constexpr int RO_K = 512;         // entries of the order kept: the top RO_K by (P, -j); the walk needs
                                  // about (visited edges + 1) of them, and past them falls back to a full scan
constexpr int RV_CAP = 1024;      // visited root edges kept; more -> the move falls back to full scans
constexpr uint32_t RV_OFF = 0xFFFFFFFFu;
// The expansion's compact-first prior: floats of the per-wave LDS window, laid out by
// action, that holds the unnormalised priors of a leaf whose valid actions span at most this many
// (eight adjacent categories: 2024 with the alignment).  32 KB per block of 4 waves, so the 16 waves per
// CU the expand kernel is budgeted for still fit the CU's 160 KB; 512 measured 0.28 % slower
constexpr int PF_WCAP = 2048;

// python value kinds on the search path (MCTS.py:82, 115, 147)
enum : uint32_t { T_INT = 0, T_F64 = 1, T_F32 = 2 };

struct NodeRec {          // 96 bytes
    uint64_t key[8];      // packed canonical state
    uint64_t hash;
    uint64_t vinfo;       // cats nibbles [0:48] | k [48:52] | n [52:56] | W [56:64]
    uint32_t p_off;       // arena offset (entries) of P / slots
    uint32_t nvalid;
    uint32_t Ns;
    uint32_t first_j;     // the node summary: the full UCB scan's pick at Ns = 0 (0x7FFFFFFF: none), so a
                          // node's first scan reads neither its P nor its slots
};
static_assert(sizeof(NodeRec) == 96, "NodeRec: 96 bytes");
struct Edge {             // 16 bytes
    double Q;
    uint32_t N;
    uint32_t tag;         // [0:2) python value kind of Q; [2:32) child node id + 1 when the edge's
                          // transition draws no dice (0: not known) - a revisit then skips the
                          // step, the canonical form and the index probe (section 6)
};
__device__ __forceinline__ uint32_t edge_kind(uint32_t tag) { return tag & 3u; }
constexpr uint32_t PATH_DET = 0x80000000u;  // path entry low word: node id | PATH_DET when the
                                            // level's transition consumed no random draw

constexpr int GST = 16;  // per-game counters (gstats)
struct EngDev {
    int E, NCAP, HCAP, ECAP, M, VCAP;
    int e_lo, e_hi;        // the game group a per-game launch covers ([0, E) unless pipelined)
    int T, dual;           // trees: T = E, or 2E with dual trees (one per arena seat: tree e is the
                           // agent's, tree E + e the opponent's - two MCTS objects, Coach.py:120-125)
    int64_t AE;
    int sims, temp_threshold;
    float c32;
    int prior;  // 0 net, 1 hash
    int fparts; // forward head split: workgroups per 16-row tile (mlse holds fparts partials [p][E])
    int rec_pred, max_exp, rec_stride;  // record_predictions: games e % rec_stride == 0, slot e / rec_stride
    int arena;             // 1 while yk_arena runs
    int arena_agent, arena_opp;  // YK_PLAYER_* of the seat-agent_seat player and of the other seat
    uint64_t seed;
    NodeRec* nodes[2];
    uint32_t* hidx[2];
    Edge* edges[2];
    uint32_t* node_count;  // [2][E]
    uint32_t* edge_count;  // [2][E]
    float* arenaP;
    uint16_t* arenaS;
    uint32_t* arena_top;   // [E]
    uint8_t* gen;          // [T]
    uint8_t* cur_round;    // [T]
    uint4* root_c;         // [T][2] the move's root once a descent found it: {id + 1 (0: not yet), p_off,
                           //        nvalid, entries of its P order}, {vinfo lo, hi, visited root edges in
                           //        rv (RV_OFF: no P order this move), walk start: the order's entries
                           //        before it are all visited}; one 32-byte read for root_scan
    int node_summary;      // 1: a node's first UCB scan takes the record's first_j (YK_NODE_SUMMARY=0: full scans)
    int prior_fast;        // >= 1: a leaf with a small valid set computes its priors in compact order; >= 2:
                           //    a general leaf's P write also reads its priors back from the window, staged there in
                           //    two pieces of the pairwise tree's leaves, four entries per lane at 10 dice; 3 (the
                           //    default): a general leaf's priors at 10 dice are computed compact-first too, through
                           //    the window in the same two pieces, in place of the dense pass
                           //    (YK_PRIOR_FAST=0: every leaf takes the dense pass and the gather P write, =1: general
                           //    leaves unstaged, =2: general leaves staged after the dense pass)
    int ro_k;              // entries of the root's order k_root_sort keeps (RO_K; YK_ROOT_K for the tests)
    uint32_t* rv;          // [T][RV_CAP] j | slot << 12 of each visited root edge
    uint16_t* ro_j;        // [T][RO_K] the root's top compact indices by descending P (ascending j on ties)
    float* ro_p;           // [T][RO_K] their P
    // game state
    yk_state_t* board;
    int32_t* cur;
    uint64_t* ctr;
    uint32_t* env_id;
    uint8_t* done;
    int32_t* nmoves;
    yk_state_t* root;
    int32_t* seat;         // [E] arena: the agent's seat (1 / -1)
    uint8_t* idle;         // [E] arena: a non-MCTS player is to move (no search this move)
    // per-sim
    yk_state_t* leaf_state;
    uint64_t* leaf_hash;
    uint8_t* leaf_flag;
    uint64_t* path;        // [E][MAXD]: (p_off + j) << 32 | node id
    uint8_t* path_len;
    uint32_t* end_node;    // [E] id + 1 of the node the descent stopped at (no valid action), else 0
    double* res_v;
    uint32_t* res_t;
    const float* logits;   // [E][PI_LD]
    const float* vpred;    // [E]
    const float2* mlse;    // [E] per-row (max, log sum exp) of the logits, from the forward; with
                           // fparts > 1, [fparts][E] raw partials (max, sum exp) merged by the expand
    const float* lut_sq;
    const float* lut_sqe;
    // records
    yk_state_t* rec_state; // [E][M]
    int32_t* rec_info;     // [E][M][8]
    uint64_t* rec_ctr;     // [E][M][2]
    double* rec_val;       // [E][M]
    uint32_t* rec_visits;  // [E][VCAP]: action << 16 | N
    int32_t* rec_voff;     // [E][M+1]
    double* final_r;       // [E]
    int32_t* final_cur;    // [E]
    int32_t* final_tot;    // [E][2] score totals with bonus (getGameEnded, YachtGame.py:408-428)
    float* rec_pi;         // [R][max_exp][3226]  (record_predictions; R = ceil(E / rec_stride))
    float* rec_v;          // [R][max_exp]
    yk_state_t* rec_leaf;  // [R][max_exp] the expanded leaf (canonical state)
    // stats
    uint64_t* gstats;      // [E][GST]: expansions, scanned, path edges, vnew, max nodes, max edges, max arena, sims,
                           // edge gathers of the UCB scans, expansions by prior path (window, sparse, general),
                           // forced root picks, pruned visits (s6f), first-play urgency's unvisited picks and picks (s6g)
    uint32_t* err;         // [1] error bits
};

// Dirichlet root noise, self-play only.  Its own kernel argument: EngDev, and with it
// the argument layout of every other kernel, is the same with and without the feature.
struct NoiseDev {
    double alpha, eps;
    uint8_t* noised;      // [E] 1 once the move's root was noised or tempered (phase 0), so phase 1 passes it by
    float* prior_before;  // [R][M][3226] record_predictions: the root's P, dense by action, before the mix
    float* prior_after;   // [R][M][3226] and after it (NULL: not recorded)
};

// The root value of each real move, self-play only: k_root_value's own kernel argument.
struct RootValDev {
    int move;             // the move k_move_end has just recorded
};

enum : uint32_t {
    ERR_NODES = 1u, ERR_EDGES = 2u, ERR_ARENA = 4u, ERR_DEPTH = 8u, ERR_STEP = 16u, ERR_ROUND = 32u,
    ERR_VISITS = 64u, ERR_MOVES = 128u, ERR_ZERO_COUNTS = 256u, ERR_ROOT = 512u, ERR_HASH = 1024u,
    ERR_FWD_SYNC = 2048u  // a forward's value head timed out on its v_head.2 hand-off (the net's flag word)
};

__device__ __forceinline__ YkS ld_state(const yk_state_t* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    YkS s;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint4 v = q[k];
        s.w[2 * k] = (uint64_t)v.x | ((uint64_t)v.y << 32);
        s.w[2 * k + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
    }
    return s;
}
__device__ __forceinline__ void st_state(yk_state_t* p, const YkS& s) {
    uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
    for (int k = 0; k < 4; k++)
        q[k] = make_uint4((uint32_t)s.w[2 * k], (uint32_t)(s.w[2 * k] >> 32), (uint32_t)s.w[2 * k + 1],
                          (uint32_t)(s.w[2 * k + 1] >> 32));
}
// A record's words after the key (bytes 64 .. 95), as one batch of two 16-byte loads: everything a
// descent level reads of its node but the state.  Issued together (and with the key's four loads
// where the level also needs the state), one round trip brings them all.
struct NodeF {
    uint64_t hash, vinfo;
    uint32_t p_off, nvalid, Ns, first_j;
};
static_assert(offsetof(NodeRec, hash) == 64 && offsetof(NodeRec, p_off) == 80 && offsetof(NodeRec, first_j) == 92,
              "ld_node reads NodeRec bytes 64 .. 95 as two uint4");
__device__ __forceinline__ NodeF ld_node(const NodeRec* r) {
    const uint4* q = reinterpret_cast<const uint4*>(r);
    const uint4 a = q[4], b = q[5];
    return NodeF{(uint64_t)a.x | ((uint64_t)a.y << 32), (uint64_t)a.z | ((uint64_t)a.w << 32), b.x, b.y, b.z, b.w};
}
// Every lane loaded the same record: as scalars, the tests on the fields compare scalars and a
// level's addresses are scalar arithmetic (fewer vector registers hold pieces of the record)
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uni(uint64_t x) { return (uint64_t)uni((uint32_t)x) | ((uint64_t)uni((uint32_t)(x >> 32)) << 32); }
__device__ __forceinline__ NodeF uniform(const NodeF& f) {
    return NodeF{uni(f.hash), uni(f.vinfo), uni(f.p_off), uni(f.nvalid), uni(f.Ns), uni(f.first_j)};
}
__device__ __forceinline__ bool key_eq(const NodeRec& r, const YkS& s) {
    bool eq = true;
#pragma unroll
    for (int i = 0; i < 8; i++) eq &= r.key[i] == s.w[i];
    return eq;
}
__device__ __forceinline__ uint64_t pack_vinfo(const VInfo& v) {
    return (v.cats & 0xFFFFFFFFFFFFull) | ((uint64_t)v.k << 48) | ((uint64_t)v.n << 52) | ((uint64_t)v.W << 56);
}
__device__ __forceinline__ VInfo unpack_vinfo(uint64_t x, uint32_t V) {
    VInfo v;
    v.cats = x & 0xFFFFFFFFFFFFull;
    v.k = (int)((x >> 48) & 0xF);
    v.n = (int)((x >> 52) & 0xF);
    v.W = (int)(x >> 56);
    v.V = (int)V;
    return v;
}
__device__ __forceinline__ int pad4(int v) { return (v + 3) & ~3; }

// The transposition index's hash of a packed state: 32-bit multiply-rotate over the 16 words
// (the index only needs spread; a key compare settles every probe).  key_hash (yk_common.h, the
// spec's) is computed only where the hash prior needs it.
__device__ __forceinline__ uint64_t index_hash(const YkS& s) {
    uint32_t a = 0x9E3779B9u, b = 0x85EBCA6Bu;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        a = (a ^ (uint32_t)s.w[i]) * 0xCC9E2D51u;
        a = (a << 15) | (a >> 17);
        b = (b ^ (uint32_t)(s.w[i] >> 32)) * 0x1B873593u;
        b = (b << 13) | (b >> 19);
    }
    a ^= b * 0x85EBCA6Bu;
    a ^= a >> 16;
    a *= 0xC2B2AE35u;
    a ^= a >> 13;
    return ((uint64_t)b << 32) | a;
}

// open-addressing lookup; returns node id or -1.  Uniform across the wave.  The probe reads the whole
// record to compare hash and key, so `f` gets the matched record's other fields from that same
// round trip (a descent level then needs no second one for them).
__device__ __forceinline__ int lookup(const EngDev& d, int g, int t, const YkS& s, uint64_t h, NodeF& f) {  // t: tree
    const uint32_t* hx = d.hidx[g] + (long)t * d.HCAP;
    const NodeRec* nodes = d.nodes[g] + (long)t * d.NCAP;
    const uint32_t mask = (uint32_t)d.HCAP - 1;
    uint32_t slot = (uint32_t)h & mask;
    for (int probe = 0; probe < d.HCAP; probe++) {
        const uint32_t v = hx[slot];
        if (v == 0) return -1;
        const NodeRec& r = nodes[v - 1];
        f = ld_node(&r);
        if ((f.hash == h) & key_eq(r, s)) return (int)(v - 1);  // ('&': one wait for the whole batch)
        slot = (slot + 1) & mask;
    }
    return -1;
}
__device__ __forceinline__ int lookup(const EngDev& d, int g, int t, const YkS& s, uint64_t h) {
    NodeF f;
    return lookup(d, g, t, s, h, f);
}
__device__ __forceinline__ bool insert_index(const EngDev& d, int g, int t, uint64_t h, uint32_t id) {
    uint32_t* hx = d.hidx[g] + (long)t * d.HCAP;
    const uint32_t mask = (uint32_t)d.HCAP - 1;
    uint32_t slot = (uint32_t)h & mask;
    for (int probe = 0; probe < d.HCAP; probe++) {
        if (hx[slot] == 0) {
            hx[slot] = id + 1;
            return true;
        }
        slot = (slot + 1) & mask;
    }
    return false;
}

// the tree game e searches with at its current move: its own, or with dual trees the one of the
// seat to move (the agent's tree e, the opponent's tree E + e)
__device__ __forceinline__ int tree_of(const EngDev& d, int e) {
    return (d.dual && d.cur[e] != d.seat[e]) ? e + d.E : e;
}

}  // namespace

// yk_noise.hip: launches k_root_noise for the games [e_lo, e_hi) of `engdev` (an EngDev) with `noisedev`
// (a NoiseDev), both passed by address and copied because their types have internal linkage: each unit
// compiles its own copy of the structs from this header.  The caller passes its sizeof of each; a unit
// built against another layout gets YK_ERR_ARG instead of a kernel reading the wrong fields.  Not part
// of the C ABI: hidden in the shared library.
static_assert(std::is_trivially_copyable<EngDev>::value && std::is_trivially_copyable<NoiseDev>::value &&
                  std::is_trivially_copyable<RootValDev>::value,
              "EngDev / NoiseDev / RootValDev cross translation units as bytes");
__attribute__((visibility("hidden"))) int yk_launch_root_noise(const void* engdev, size_t engdev_bytes,
                                                               const void* noisedev, size_t noisedev_bytes, int move,
                                                               int phase, hipStream_t stream);
// yk_noise.hip: the same launch with the root policy temperature - `root_t` the DEVICE table of T
// by move (M entries) - and, with_noise, the noise mixed from the tempered prior in the same kernel; without
// it the form that has no sampler.  `noisedev` carries the per-game byte and the prior records either way.
__attribute__((visibility("hidden"))) int yk_launch_root_temper(const void* engdev, size_t engdev_bytes,
                                                                const void* noisedev, size_t noisedev_bytes,
                                                                const double* root_t, int with_noise, int move,
                                                                int phase, hipStream_t stream);
// yk_rootval.hip: launches k_root_value for the games [e_lo, e_hi) of `engdev` after k_move_end(rvdev.move),
// on the same terms.
__attribute__((visibility("hidden"))) int yk_launch_root_value(const void* engdev, size_t engdev_bytes,
                                                               const void* rvdev, size_t rvdev_bytes,
                                                               hipStream_t stream);
